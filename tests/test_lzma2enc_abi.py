"""CPU-side checks of the LZMA2 / xz writers' C ABI (no GPU needed): the
exports, CLzma2EncProps' layout, the props drop-ins against the emulator test's
hand-worked table, Lzma2EncGpu_DescFromProps, the planner over the LZMA2
slices, and the loud failure without a device."""
import ctypes
import os
import subprocess

import pytest

import lzma2enc_cases as C
import native

LIB = os.path.join(native.ROOT, "lzma-sdk-zliblike_amd", "lib", "liblzmagpu.so")
NAMES = {"Lzma2EncProps_Init", "Lzma2EncProps_Normalize", "Lzma2EncGpu_BlockBound",
         "Lzma2EncGpu_DescFromProps", "Lzma2EncGpu_PlanBatch", "Lzma2EncGpu_EncodeBatch",
         "Lzma2EncGpu_EncodeBatchHost", "Lzma2EncGpu_Compact", "LzmaGpu_Lzma2EncodeHost",
         "Lzma2Enc_Create", "Lzma2Enc_Destroy", "Lzma2Enc_SetProps", "Lzma2Enc_WriteProperties",
         "Lzma2Enc_Encode", "LzmaGpu_XzEncode"}


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def test_struct_layout_and_exports(L):
    assert ctypes.sizeof(L.CLzma2EncProps) == 64 and L.CLzma2EncProps.blockSize.offset == 48
    assert L.CLzma2EncProps.numBlockThreads.offset == 56
    assert L.CLzma2EncProps.numTotalThreads.offset == 60
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert NAMES <= exported and NAMES <= set(L.EXPORTED)
    header = open(os.path.join(native.ROOT, "include", "lzma_gpu.h")).read()
    assert all(n + "(" in header for n in NAMES)


def test_props_dropins(L):
    p = L.CLzma2EncProps()
    L.lib.Lzma2EncProps_Init(ctypes.byref(p))
    assert (p.lzmaProps.level, p.blockSize, p.numBlockThreads, p.numTotalThreads) == (5, 0, -1, -1)
    for given, want in C.NORMALIZE:
        L.lib.Lzma2EncProps_Init(ctypes.byref(p))
        (p.lzmaProps.level, p.lzmaProps.dictSize, p.blockSize, p.numBlockThreads,
         p.numTotalThreads, p.lzmaProps.numThreads) = given
        L.lib.Lzma2EncProps_Normalize(ctypes.byref(p))
        assert (p.lzmaProps.numThreads, p.numBlockThreads, p.numTotalThreads, p.blockSize,
                p.lzmaProps.dictSize) == want, given
    for n in (0, 1, 1023, 1024, 65536, 1 << 20, (1 << 31) - 1):
        assert L.block_bound(n) == n + (n >> 10) + 16


def test_desc_from_props(L):
    r, d, prop = L.enc2_desc_from_props(L.enc2_props(1, 1 << 16))
    assert (r, prop) == (0, 8)
    assert (d.dict_size, d.lc, d.lp, d.pb, d.fb, d.mc, d.write_end_mark) == (1 << 16, 3, 0, 2, 32,
                                                                             16, 0)
    assert L.enc2_desc_from_props(L.enc2_props(4))[2] == 20            # 4 MiB
    assert L.enc2_desc_from_props(L.enc2_props(1, 4097))[2] == 1       # 6 KiB
    for lc, lp in ((4, 1), (3, 2), (0, 5), (5, 0)):
        r, d, prop = L.enc2_desc_from_props(L.enc2_props(1, lc=lc, lp=lp))
        assert (r, d.dict_size, prop) == (C.PARAM, 0, 0)
    assert L.enc2_desc_from_props(L.enc2_props(1, lc=4, lp=0))[0] == 0
    assert L.enc2_desc_from_props(L.enc2_props(5, lc=4, lp=1))[0] == C.PARAM
    assert L.enc2_desc_from_props(L.enc2_props(5))[0] == C.UNSUPPORTED
    assert "optimal parser" in L.last_error()


def test_plan_batch_appends_the_saved_table(L):
    lens = [100, 70000, 0, 4097, 12]
    one = (L.EncStreamDesc * len(lens))()
    two = (L.EncStreamDesc * len(lens))()
    for i, n in enumerate(lens):
        r, d, _ = L.enc2_desc_from_props(L.enc2_props(1, 4096))
        assert r == 0
        for arr in (one, two):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(d), ctypes.sizeof(d))
            arr[i].src_len = n
    two[4].lc, two[4].lp = 3, 2        # fine for LZMA, refused for LZMA2: no slice
    one[4].lc, one[4].lp = 3, 2
    r1, order1, ws1 = L.enc_plan(one, len(lens))
    r2, order2, ws2 = L.enc2_plan(two, len(lens))
    assert (r1, r2) == (0, 0) and order2 == [1, 3, 0, 4, 2]
    saved = (((1846 + (0x300 << 3)) * 2 + 15 & ~15) + 255) & ~255
    at = 0
    for i in range(4):
        assert two[i].ws_off == at and at % 256 == 0
        at += (one[i + 1].ws_off - one[i].ws_off) + saved     # the LZMA slice, then the table
    assert two[4].ws_off == 0 and one[4].ws_off != 0 and ws2 == at
    assert L.lib.Lzma2EncGpu_PlanBatch(two, 1 << 31, None, None) == C.PARAM


def test_no_device_fails_loudly(L):
    # the checks the reference makes before it encodes come first, device or not
    assert L.Lzma2EncodeHost(b"abc", L.enc2_props(5), 100)[0] == C.UNSUPPORTED
    assert "optimal parser" in L.last_error()
    assert L.XzEncode(b"abc", L.enc2_props(5), 1, 100)[0] == C.UNSUPPORTED
    assert L.Lzma2EncodeHost(b"abc", L.enc2_props(1, lc=4, lp=1), 100)[0] == C.PARAM
    assert L.XzEncode(b"abc", L.enc2_props(1), 2, 100)[0] == C.UNSUPPORTED      # check id 2
    h = L.lib.Lzma2Enc_Create(ctypes.byref(L.g_alloc), ctypes.byref(L.g_alloc))
    assert h
    assert L.lib.Lzma2Enc_SetProps(h, ctypes.byref(L.enc2_props(1, lc=4, lp=1))) == C.PARAM
    assert L.lib.Lzma2Enc_SetProps(h, ctypes.byref(L.enc2_props(1, 1 << 20))) == 0
    assert L.lib.Lzma2Enc_WriteProperties(h) == 16

    def read(p, buf, size):
        size[0] = 0
        return 0
    keep = (L.SeqWrite(lambda p, buf, size: size), L.SeqRead(read))
    out, inp = L.ISeqOutStream(keep[0]), L.ISeqInStream(keep[1])
    if L.device_count() <= 0:
        assert L.lib.Lzma2Enc_Encode(h, ctypes.byref(out), ctypes.byref(inp), None) == \
            L.SZ_ERROR_FAIL
    assert L.lib.Lzma2Enc_SetProps(h, ctypes.byref(L.enc2_props(5))) == 0
    assert L.lib.Lzma2Enc_Encode(h, ctypes.byref(out), ctypes.byref(inp), None) == C.UNSUPPORTED
    L.lib.Lzma2Enc_Destroy(h)
    if L.device_count() > 0:
        return
    assert L.Lzma2EncodeHost(b"abc" * 50, L.enc2_props(1), 1000)[0] == L.SZ_ERROR_FAIL
    assert "no HIP device" in L.last_error()
    assert L.Lzma2EncodeHost(b"", L.enc2_props(1), 10)[0] == L.SZ_ERROR_FAIL
    assert L.XzEncode(b"abc" * 50, L.enc2_props(1), 1, 1000)[0] == L.SZ_ERROR_FAIL
    assert L.XzEncode(b"", L.enc2_props(1), 1, 1000)[0] == L.SZ_ERROR_FAIL
    assert L.lib.Lzma2EncGpu_EncodeBatch(None, None, 1, None, None, None, None, 0, None) == \
        L.SZ_ERROR_FAIL
    assert L.lib.Lzma2EncGpu_Compact(None, None, 0, None, None, 0, None, None, None) == \
        L.SZ_ERROR_FAIL
    d = (L.EncStreamDesc * 1)()
    assert L.lzma2_encode_batch_host(d, 1, b"", b"")[0] == L.SZ_ERROR_FAIL

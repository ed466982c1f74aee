"""The encoder-session ABI without a device: the record's layout, the exported
names in the library, the header and the binding, and the host-only calls
(LzmaEncGpu_SessionWorkspaceBytes, _SessionInit, _SessionScratchBytes, the
handle's SetProps / WriteProperties)."""
import ctypes
import os
import subprocess
import sys

import pytest

import lzmaenc_cases as C
import lzmaenc_session_cases as S
import native

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))
LIB = os.path.join(native.ROOT, "lzma-sdk-zliblike_amd", "lib", "liblzmagpu.so")
NAMES = {"LzmaEncGpu_SessionWorkspaceBytes", "LzmaEncGpu_SessionInit",
         "LzmaEncGpu_SessionScratchBytes", "LzmaEncGpu_SessionEncodeBatch",
         "LzmaEncGpu_SessionListPass", "LzmaEnc_Create", "LzmaEnc_Destroy", "LzmaEnc_SetProps",
         "LzmaEnc_WriteProperties", "LzmaEnc_Encode", "LzmaEnc_MemEncode"}


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def test_record_constants_and_exports(L):
    assert ctypes.sizeof(L.EncSession) == ctypes.sizeof(S.Session) == 200
    assert [(f, getattr(L.EncSession, f).offset) for f, _ in L.EncSession._fields_] == \
        [(f, getattr(S.Session, f).offset) for f, _ in S.Session._fields_]
    assert (L.ENC_SESSION_HOLD, L.ENC_SESSION_NEEDS_INPUT, L.ENC_SESSION_FINISHED,
            L.ENC_SESSION_BUDGET) == (546, 0, 1, 2)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert NAMES <= exported and NAMES <= set(L.EXPORTED)
    header = open(os.path.join(native.ROOT, "include", "lzma_gpu.h")).read()
    assert all(n + "(" in header for n in NAMES)
    assert "#define LZMA_ENC_GPU_SESSION_HOLD 546u" in header
    integration = open(os.path.join(native.ROOT, "INTEGRATION.md")).read()
    assert all(n.split("_")[0] in integration for n in NAMES)
    assert "LzmaEncGpu_SessionEncodeBatch" in integration and "LzmaEnc_MemEncode" in integration


def test_workspace_is_the_one_shot_slice_sized_by_the_capacity(L, tmp_path):
    one = C.load_emu(C.build_emu(tmp_path))
    for dict_size, lc, lp, src_cap in ((4096, 3, 0, 100), (4096, 3, 0, 1 << 20), (1 << 16, 0, 4, 20000),
                                       (1 << 20, 8, 4, 10), (1 << 24, 3, 0, 1 << 16)):
        p = L.enc_props(level=1, dict_size=dict_size, lc=lc, lp=lp)
        assert L.enc_session_workspace_bytes(p, src_cap) == \
            one.lzmaenc_emu_slice_bytes(dict_size, lc, lp, src_cap)
    assert L.enc_session_workspace_bytes(L.enc_props(level=1), 1 << 31) == 0
    assert L.enc_session_workspace_bytes(L.enc_props(level=5), 4096) == 0
    assert L.enc_session_scratch_bytes(0) == 16 and L.enc_session_scratch_bytes(200) == 16 + 1600


def test_session_init(L):
    s = L.EncSession()
    ctypes.memset(ctypes.byref(s), 0xA5, ctypes.sizeof(s))
    r, props5 = L.enc_session_init(s, L.enc_props(level=1, fb=300, lc=0, lp=2, pb=1), 0x1000, 5000,
                                   0x2000, 77, 0x3000, end_mark=True)
    want = L.enc_desc_from_props(L.enc_props(level=1, fb=300, lc=0, lp=2, pb=1), True)
    assert (r, props5) == (0, want[2])
    d = want[1]
    assert (s.dict_size, s.lc, s.lp, s.pb, s.fb, s.mc, s.write_end_mark) == \
        (d.dict_size, d.lc, d.lp, d.pb, d.fb, d.mc, 1) and s.fb == 273
    assert (s.src, s.src_cap, s.dst, s.dst_cap, s.ws) == (0x1000, 5000, 0x2000, 77, 0x3000)
    assert (s.needs_init, s.finished, s.status, s.res, s.in_pos, s.out_pos, s.src_len) == \
        (1, 0, S.NEEDS_INPUT, 0, 0, 0, 0)
    # refused: *s stays as it was
    before = bytes(s)
    prev = L.enc_set_modes(3)
    try:
        for kw, res in ((dict(level=5), C.UNSUPPORTED), (dict(level=1, algo=1), C.UNSUPPORTED),
                        (dict(level=1, bt_mode=1), C.UNSUPPORTED), (dict(level=1, lc=9), C.PARAM)):
            assert L.enc_session_init(s, L.enc_props(**kw), 0, 100, 0, 100, 0)[0] == res, kw
            if res == C.UNSUPPORTED:
                assert "props field" in L.last_error() and "session" in L.last_error()
    finally:
        L.enc_set_modes(prev)
    assert L.enc_session_init(s, L.enc_props(level=1), 0, 1 << 31, 0, 100, 0)[0] == C.UNSUPPORTED
    assert L.enc_session_init(s, L.enc_props(level=1), 0, 100, 0, 100, 8)[0] == C.PARAM
    assert bytes(s) == before


def test_handle_props_without_a_device(L):
    golden = C.load_golden()
    g = next(g for g in golden["cases"] if g["res"] == C.OK)
    h = L.lib.LzmaEnc_Create(ctypes.byref(L.g_alloc))
    try:
        p = L.enc_props(lc=9)
        assert L.lib.LzmaEnc_SetProps(h, ctypes.byref(p)) == C.PARAM
        c = g["case"]
        p = L.enc_props(c["level"], c["dict"], c["lc"], c["lp"], c["pb"], c["fb"], c["mc"])
        assert L.lib.LzmaEnc_SetProps(h, ctypes.byref(p)) == 0
        buf, size = ctypes.create_string_buffer(5), ctypes.c_size_t(4)
        assert L.lib.LzmaEnc_WriteProperties(h, buf, ctypes.byref(size)) == C.PARAM
        size = ctypes.c_size_t(8)
        assert L.lib.LzmaEnc_WriteProperties(h, buf, ctypes.byref(size)) == 0
        assert (size.value, buf.raw.hex()) == (5, g["props5"])
    finally:
        L.lib.LzmaEnc_Destroy(h, ctypes.byref(L.g_alloc), ctypes.byref(L.g_alloc))

"""CPU-side checks of the Lzma86 and xz filter-chain surface (no GPU needed):
constants, struct sizes and signatures against include/lzma_gpu.h, and without
a device the calls fail loudly."""
import ctypes
import os
import re
import subprocess
import sys

import native

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))
HEADER = os.path.join(native.ROOT, "include", "lzma_gpu.h")
LIB = os.path.join(native.ROOT, "lzma-sdk-zliblike_amd", "lib", "liblzmagpu.so")
NAMES = ("Lzma86_Encode", "Lzma86_GetUnpackSize", "Lzma86_Decode", "Lzma86Gpu_EncodeScratch",
         "Lzma86Gpu_EncodeBatch", "Lzma86Gpu_EncodeBatchHost", "Lzma86Gpu_DecodeScratch",
         "Lzma86Gpu_DecodeBatch", "Lzma86Gpu_DecodeBatchHost", "LzmaGpu_XzEncodeEx")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_constants_and_guard():
    txt = header_text()
    guard = txt[txt.index("#ifndef __LZMA86_H"):]
    guard = guard[:guard.index("#endif")]
    assert "#define LZMA86_SIZE_OFFSET (1 + 5)" in guard
    assert "#define LZMA86_HEADER_SIZE (LZMA86_SIZE_OFFSET + 8)" in guard
    assert re.search(r"enum ESzFilterMode \{ SZ_FILTER_NO, SZ_FILTER_YES, SZ_FILTER_AUTO \};", guard)
    import lzmagpu as L
    assert (L.LZMA86_HEADER_SIZE, L.SZ_FILTER_NO, L.SZ_FILTER_YES, L.SZ_FILTER_AUTO) == (14, 0, 1, 2)
    assert "#define LZMA_GPU_XZ_ENC_FILTERS_MAX 3" in txt


def test_signatures_are_the_references():
    txt = " ".join(header_text().split())
    assert ("SRes Lzma86_Encode(Byte *dest, size_t *destLen, const Byte *src, size_t srcLen, "
            "int level, UInt32 dictSize, int filterMode);") in txt
    assert "SRes Lzma86_GetUnpackSize(const Byte *src, SizeT srcLen, UInt64 *unpackSize);" in txt
    assert "SRes Lzma86_Decode(Byte *dest, SizeT *destLen, const Byte *src, SizeT *srcLen);" in txt
    assert ("SRes LzmaGpu_XzEncodeEx(Byte *dest, SizeT *destLen, const Byte *src, SizeT srcLen, "
            "const CLzma2EncProps *props, unsigned check_type, const LzmaGpuXzFilter *filters, "
            "unsigned num_filters);") in txt


def test_struct_layouts_match_a_c_compiler(tmp_path):
    import lzmagpu as L
    prog = tmp_path / "sizes.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lzma_gpu.h"\n'
                    "int main(void) { printf(\"%zu %zu %zu %zu %zu %zu %zu\\n\", "
                    "sizeof(Lzma86GpuStreamDesc), sizeof(Lzma86GpuResult), sizeof(Lzma86GpuStats), "
                    "sizeof(LzmaGpuXzFilter), offsetof(Lzma86GpuStreamDesc, filterMode), "
                    "offsetof(Lzma86GpuResult, src_len), offsetof(Lzma86GpuStats, stage_ns)); "
                    "return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [48, 24, 64, 8, 40, 16, 32]
    assert got[:4] == [ctypes.sizeof(L.Lzma86StreamDesc), ctypes.sizeof(L.Lzma86Result),
                       ctypes.sizeof(L.Lzma86Stats), ctypes.sizeof(L.XzFilter)]
    assert (L.Lzma86StreamDesc.filterMode.offset, L.Lzma86Result.src_len.offset,
            L.Lzma86Stats.stage_ns.offset) == (40, 16, 32)


def test_symbols_exported_and_bound():
    import lzmagpu as L
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for n in NAMES:
        assert n in exported and n in L.EXPORTED, n


def test_host_only_calls():
    import lzmagpu as L
    head = bytes([1, 0x5D, 0, 0, 1, 0]) + (123456789).to_bytes(8, "little")
    assert L.Lzma86_GetUnpackSize(head) == (0, 123456789)
    assert L.Lzma86_GetUnpackSize(head[:13])[0] == 6
    # the reference's own checks come before the device
    assert L.Lzma86_Encode(b"abc", 13) == (7, 0, b"")
    assert L.Lzma86_Decode(head[:13], 10)[0] == 6
    assert L.Lzma86_Decode(b"\x02" + head[1:], 10)[:2] == (4, 0)
    d = L.lzma86_descs([dict(src_off=0, src_len=100, dst_off=0, dst_cap=200, mode=2),
                        dict(src_off=100, src_len=50, dst_off=200, dst_cap=13, mode=2),
                        dict(src_off=150, src_len=50, dst_off=213, dst_cap=100, mode=0)])
    r, scratch = L.lzma86_encode_scratch(d, 3)
    assert r == 0 and scratch % 256 == 0 and scratch > 3 * 64
    r, one = L.lzma86_encode_scratch(d, 1)
    assert r == 0 and 0 < one < scratch


def test_without_a_device_the_calls_fail_loudly():
    import lzmagpu as L
    if L.device_count() > 0:
        return
    d = L.lzma86_descs([dict(src_off=0, src_len=3, dst_off=0, dst_cap=100)])
    assert L.lzma86_encode_batch_host(d, 1, b"abc", bytes(100))[0] == L.SZ_ERROR_FAIL
    assert L.lzma86_decode_batch_host(d, 1, bytes(20), bytes(100))[0] == L.SZ_ERROR_FAIL
    assert L.lib.Lzma86Gpu_EncodeBatch(d, 1, None, None, None, 0, None, None) == L.SZ_ERROR_FAIL
    assert L.lib.Lzma86Gpu_DecodeBatch(d, 1, bytes(14), None, None, None, 0, None,
                                       None) == L.SZ_ERROR_FAIL
    assert L.Lzma86_Encode(b"abc", 100)[0] == L.SZ_ERROR_FAIL
    assert L.Lzma86_Decode(bytes(20), 100)[0] == L.SZ_ERROR_FAIL
    assert L.XzEncodeEx(b"abc", L.enc2_props(1), 1, 200, [(4, 0)])[0] == L.SZ_ERROR_FAIL
    assert "no HIP device" in L.last_error()

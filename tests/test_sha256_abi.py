"""CPU-side checks of the SHA-256 C ABI (no GPU needed), in the manner of
test_abi.py: CSha256 has the reference's layout, the library exports the
drop-ins and the batch form, and the three drop-in prototypes read as the
reference header's do where that header is present.
"""
import ctypes
import os
import re
import subprocess

import native

HEADER = os.path.join(native.ROOT, "include", "lzma_gpu.h")
LIB = os.path.join(native.ROOT, "lzma-sdk-zliblike_amd", "lib", "liblzmagpu.so")
REF_HEADER = "/root/reference/Sha256.h"  # the build container only

DROPINS = ("Sha256_Init", "Sha256_Update", "Sha256_Final")


def prototypes(path):
    """{name: normalised prototype} of the Sha256_* functions a header declares."""
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bvoid\s+(Sha256_\w+)\s*\(([^)]*)\)\s*;", txt):
        out[m.group(1)] = re.sub(r"\s+", " ", m.group(2).replace("*", " * ")).strip()
    return out


def test_csha256_layout():
    import lzmagpu as L
    assert ctypes.sizeof(L.CSha256) == 104
    assert (L.CSha256.state.offset, L.CSha256.count.offset, L.CSha256.buffer.offset) == (0, 32, 40)
    assert (L.CSha256.state.size, L.CSha256.count.size, L.CSha256.buffer.size) == (32, 8, 64)
    assert L.SHA256_DIGEST_SIZE == 32
    # the C header's struct, as the compiler lays it out
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "lzma_gpu.h"\n'
           "int main(void) { printf(\"%zu %zu %zu %zu %d\\n\", sizeof(CSha256), "
           "offsetof(CSha256, state), offsetof(CSha256, count), offsetof(CSha256, buffer), "
           "SHA256_DIGEST_SIZE); return 0; }\n")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write(src)
        subprocess.run(["gcc", "-I", os.path.join(native.ROOT, "include"), "-o",
                        os.path.join(d, "t"), os.path.join(d, "t.c")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True)
    assert out.stdout.split() == ["104", "0", "32", "40", "32"]


def test_library_exports_sha256_surface():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in DROPINS + ("Sha256Gpu_Batch",):
        assert name in exported, name
    ours = prototypes(HEADER)
    assert sorted(ours) == sorted(DROPINS)
    txt = open(HEADER).read()
    for macro, val in (("LZMA_GPU_SHA256_AUTO", 0), ("LZMA_GPU_SHA256_LANE", 1),
                       ("LZMA_GPU_SHA256_WAVE", 2), ("SHA256_DIGEST_SIZE", 32)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, val), txt), macro


def test_dropin_prototypes_agree_with_reference_header():
    ours = prototypes(HEADER)
    assert ours == {"Sha256_Init": "CSha256 * p",
                    "Sha256_Update": "CSha256 * p, const Byte * data, size_t size",
                    "Sha256_Final": "CSha256 * p, Byte * digest"}
    if os.path.exists(REF_HEADER):
        assert prototypes(REF_HEADER) == ours
        ref = re.sub(r"\s+", " ", open(REF_HEADER).read())
        assert "UInt32 state[8]; UInt64 count; Byte buffer[64];" in ref


def test_no_host_sha256_compression_in_the_product():
    """The round constants live in the device header only: no host translation
    unit of the product carries a SHA-256 compression function."""
    csrc = os.path.join(native.ROOT, "lzma-sdk-zliblike_amd", "csrc")
    holders = [f for f in sorted(os.listdir(csrc))
               if re.search(r"0x428a2f98", open(os.path.join(csrc, f)).read(), flags=re.I)]
    assert holders == ["sha256_device.h"]
    users = [f for f in sorted(os.listdir(csrc))
             if '#include "sha256_device.h"' in open(os.path.join(csrc, f)).read()]
    assert users == ["sha256_kernels.hip"]

"""tests/golden/lzma86/: the outputs of the reference's own Lzma86_Encode
(Lzma86Enc.c) for six inputs.  The expectation the other Lzma86 tests compose
from ref_lzma_encode and x86_Convert must equal them (no GPU needed), and so
must the GPU's bytes."""
import os
import sys

import pytest

import lzma86_cases as C
import native

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


def test_golden_files_are_the_listed_cases(golden):
    assert [g["case"] for g in golden] == C.golden_cases() and len(golden) == 6
    for g in golden:
        b = g["bytes"]
        assert g["res"] == C.OK and len(b) == g["dest_len"] < 8192 and b[0] == g["flag"]
        assert int.from_bytes(b[6:14], "little") == g["case"]["n"]
    flags = {g["case"]["name"]: g["flag"] for g in golden}
    assert flags == {"code_auto": 1, "code_yes": 1, "text_auto": 0, "text_yes": 1,
                     "noise_auto": 0, "noise_yes": 1}


def test_composed_expectation_equals_lzma86enc(golden):
    assert C.have_refs()
    for g in golden:
        assert C.expect(g["case"]) == (g["res"], g["dest_len"], g["bytes"]), g["file"]


@pytest.mark.gpu
def test_gpu_bytes_equal_lzma86enc(golden):
    import lzmagpu as L
    src, rows, dst_off = bytearray(), [], 0
    for g in golden:
        c, data = g["case"], C.src_of(g["case"])
        rows.append(dict(src_off=len(src), src_len=len(data), dst_off=dst_off,
                         dst_cap=C.cap_of(c), level=c["level"], dict_size=c["dict"],
                         mode=c["mode"]))
        src += data
        dst_off += C.cap_of(c)
    d = L.lzma86_descs(rows)
    r, res, out = L.lzma86_encode_batch_host(d, len(rows), bytes(src), bytes(dst_off))
    assert r == 0, L.last_error()
    for k, g in enumerate(golden):
        assert (res[k].res, res[k].dest_len, res[k].filter) == (g["res"], g["dest_len"],
                                                                g["flag"]), g["file"]
        assert out[d[k].dst_off:d[k].dst_off + res[k].dest_len] == g["bytes"], g["file"]

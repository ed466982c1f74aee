"""Writes tests/golden/lzmaenc_cases.json from the live reference encoder
(oracle/_ref/libref_lzma.so: the reference's LzmaEnc.c / LzFind.c).

For every case of lzmaenc_cases.golden_cases() it stores the generator
parameters and props (no input bytes: inputs come from the generator), the
resolved capacity, res, dest_len, the 5 props bytes, and the length, SHA-256
and first 32 bytes of the reference's output.  Cases with an explicit mc, algo
or btMode go through the reference's LzmaEncode with a full CLzmaEncProps
(ctypes, allocator callbacks via CFUNCTYPE), because the committed shim takes
none of them; the rest go through the shim's ref_lzma_encode.

Run from the repository root:  python tests/golden/make_golden_lzmaenc.py"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import lzmaenc_cases as C  # noqa: E402
import native  # noqa: E402


def main():
    assert native.have_ref(), "build the reference library first (oracle/Makefile.ref)"
    cases = []
    for c in C.golden_cases():
        res, dl, props5, out, cap, full_len = C.ref_expect(c)
        cases.append({"case": c, "norm": C.ref_normalize(c),   # LzmaEncProps_Normalize's result
                      "cap": cap, "res": res, "dest_len": dl, "props5": props5.hex(),
                      "len": len(out), "sha256": C.sha(out), "head": out[:32].hex()})
    with open(C.GOLDEN, "w") as f:
        json.dump({"note": "recorded from the reference's LzmaEncode; see make_golden_lzmaenc.py",
                   "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(cases), "cases,", os.path.getsize(C.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

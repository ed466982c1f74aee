"""Writes tests/golden/lzma2enc_cases.json from the live reference encoder
(oracle/_ref/libref_lzma.so: the reference's Lzma2Enc.c over LzmaEnc.c /
LzFind.c, single-threaded, through the shim's ref_lzma2_encode).

For every case of lzma2enc_cases.golden_cases() it stores the generator
segments and props (no input bytes: inputs come from native.gen), res, the prop
byte, and of the reference's output the length, SHA-256, first 32 bytes and the
chunk list (control, unpack size, pack size; the final 0x00 is (0, 0, 0)).
"multiblock" holds, for every buffer of lzma2enc_cases.MULTIBLOCK cut into
blocks, the length and SHA-256 of each block's chunks and of the whole stream.

Run from the repository root:  python tests/golden/make_golden_lzma2enc.py"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import lzma2enc_cases as C  # noqa: E402
import native  # noqa: E402


def main():
    assert native.have_ref(), "build the reference library first (oracle/Makefile.ref)"
    cases = []
    for c in C.golden_cases():
        res, prop, out = C.ref_stream(c)
        cases.append(C.record(c, res, prop, out))
    multi = [C.multiblock_record(c, block, *C.ref_multiblock(c, block))
             for c, block in C.MULTIBLOCK]
    with open(C.GOLDEN, "w") as f:
        json.dump({"note": "recorded from the reference's Lzma2Enc_Encode; see "
                           "make_golden_lzma2enc.py", "cases": cases, "multiblock": multi}, f,
                  indent=0, sort_keys=True)
        f.write("\n")
    print(len(cases), "cases,", os.path.getsize(C.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

"""Writes tests/golden/lzmaenc_bigdict_cases.json from the live reference encoder
(oracle/_ref/libref_lzma.so: the reference's LzmaEnc.c / LzFind.c / Lzma2Enc.c,
single-threaded) for the encoder tests above 64 KiB dictionaries.

"cases": for every case of lzmaenc_bigdict_cases.golden_cases() the generator
parameters and props (no input bytes), the resolved capacity, res, dest_len, the
5 props bytes, and the length, SHA-256 and first 32 bytes of the output of the
reference's LzmaEncode with the case's full CLzmaEncProps.
"lzma2": lzma2enc_cases.record of every case of
lzmaenc_bigdict_cases.lzma2_cases() by the reference's Lzma2Enc_Encode.

Run from the repository root:  python tests/golden/make_golden_lzmaenc_bigdict.py"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import lzma2enc_cases as C2  # noqa: E402
import lzmaenc_bigdict_cases as B  # noqa: E402
import lzmaenc_cases as C  # noqa: E402
import lzmaenc_opt_cases as O  # noqa: E402
import native  # noqa: E402


def main():
    assert native.have_ref(), "build the reference library first (oracle/Makefile.ref)"
    cases = []
    for c in B.golden_cases():
        res, dl, props5, out, cap, full_len = O.ref_expect(c)
        cases.append({"case": c, "norm": C.ref_normalize(c), "cap": cap, "res": res,
                      "dest_len": dl, "props5": props5.hex(), "len": len(out),
                      "sha256": C.sha(out), "head": out[:32].hex()})
    lzma2 = []
    for c in B.lzma2_cases():
        res, prop, out = C2.ref_stream(c)
        lzma2.append(C2.record(c, res, prop, out))
    with open(B.GOLDEN, "w") as f:
        json.dump({"note": "recorded from the reference's LzmaEncode and Lzma2Enc_Encode; see "
                           "make_golden_lzmaenc_bigdict.py", "cases": cases, "lzma2": lzma2}, f,
                  indent=0, sort_keys=True)
        f.write("\n")
    print(len(cases), "+", len(lzma2), "cases,", os.path.getsize(B.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

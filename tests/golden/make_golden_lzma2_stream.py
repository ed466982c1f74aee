"""Writes tests/golden/lzma2_stream_cases.json: the reference's own
Lzma2Dec_DecodeToBuf / Lzma2Dec_DecodeToDic (oracle/_ref/libref_lzma.so: its
Lzma2Dec.c and LzmaDec.c compiled in place) driven call by call by
tests/lzma2_stream.py over every cell of its grid.  Per run: the call count and
SHA-256 of trace and output; per liblzma-made input the SHA-256 of the stream;
per coverage condition the first recorded run (and call) at which it holds.

    python tests/golden/make_golden_lzma2_stream.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "lzma-sdk-zliblike_amd"))

import lzma2_stream as S  # noqa: E402
import native  # noqa: E402


def main():
    lib = native.ref()
    runs, witness, calls = {}, {}, 0
    for cell in S.grid():
        c, f, lp, i, o = cell
        r = S.run(lib, cell)
        k = S.key(*cell)
        assert k not in runs, k
        runs[k] = S.record(r)
        calls += len(r[0])
        if S.well_formed(c):
            for cond in S.CONDITIONS:
                if cond not in witness:
                    at = S.holds(cond, cell, r)
                    if at is not None:
                        witness[cond] = [k, at]
    missing = [c for c in S.CONDITIONS if c not in witness]
    assert not missing, missing
    doc = dict(generator="tests/golden/make_golden_lzma2_stream.py",
               reference="Lzma2Dec.c + LzmaDec.c compiled in place (oracle/Makefile.ref)",
               total_calls=calls,
               streams={c["name"]: hashlib.sha256(c["src"]).hexdigest()
                        for c in S.cases() if "plain" in c},
               witness=witness, runs=runs)
    with open(S.GOLDEN, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(runs), "runs,", calls, "calls ->", S.GOLDEN)


if __name__ == "__main__":
    main()

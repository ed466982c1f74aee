#!/usr/bin/env python3
"""Record the reference's answers for the hand-made decoder set
(tests/handmade_cases.py) in tests/golden/handmade_cases.json: per case and
finish mode {res, status, dest_len, src_len} and the SHA-256 of the output,
from the reference's LzmaDec.c / Lzma2Dec.c compiled in place
(oracle/_ref/libref_lzma.so).  Results only: the streams are generated.

    python tests/golden/make_golden_handmade.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import handmade_cases as H  # noqa: E402
import native  # noqa: E402


def main():
    if not native.have_ref():
        sys.exit("oracle/_ref/libref_lzma.so is not built")
    out = {}
    for c in H.cases():
        for finish in (0, 1):
            row, data = H.from_reference(c, finish)
            k = H.key(c, finish)
            assert k not in out, k
            out[k] = {"res": row[0], "status": row[1], "dest_len": row[2], "src_len": row[3],
                      "sha256": H.sha(data)}
    with open(H.GOLDEN, "w") as f:
        json.dump({"source": "reference LzmaDec.c / Lzma2Dec.c via oracle/_ref/libref_lzma.so",
                   "cases": out}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} records -> {H.GOLDEN}")


if __name__ == "__main__":
    main()

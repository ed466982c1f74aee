#!/usr/bin/env python3
"""Record the reference's LzmaDec_DecodeToBuf loops over the hand-made LZMA
set in tests/golden/handmade_stream_cases.json: per case and finish mode one
SHA-256 over every run of the chunk grid (tests/handmade_stream.py: the grid,
its order and what of a run the digest covers), the grid itself and the
largest call count of each chunking.  From the reference's LzmaDec.c compiled
in place (oracle/_ref/libref_lzma.so, ref_lzma_stream_decode).  Digests only:
the streams are generated.

    python tests/golden/make_golden_handmade_stream.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import handmade_stream as S  # noqa: E402
import native  # noqa: E402


def main():
    if not native.have_ref():
        sys.exit("oracle/_ref/libref_lzma.so is not built")
    digests, top = S.digests(S.reference_fn())
    with open(S.GOLDEN, "w") as f:
        json.dump({"source": "reference LzmaDec.c via oracle/_ref/libref_lzma.so "
                             "(ref_lzma_stream_decode)",
                   "grid": {"in_chunks": list(S.IN_CHUNKS), "out_chunks": list(S.OUT_CHUNKS),
                            "small": S.SMALL, "large_min_in": 19, "large_min_out": 272},
                   "max_calls": top, "cases": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests -> {S.GOLDEN}")


if __name__ == "__main__":
    main()

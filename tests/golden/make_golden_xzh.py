"""Generate tests/golden/xzh_cases.json: the reference's answers for the
hand-made xz files of tests/xz_handmade.py.

Run where oracle/_ref/libref.so is built (`make -f oracle/Makefile.ref`, which
compiles XzIn.c and XzDec.c in place):

    python tests/golden/make_golden_xzh.py

Per case: the SHA-256 of the generated file (so generator drift is caught),
ref_xz_index's full result (Xzs_ReadBackward: SRes, stream flags, every
block's {stream, totalSize, unpackSize}, Xzs_GetUnpackSize), ref_xz_decode's
{res, status, dest_len, src_len, finished} with the SHA-256 of what it wrote
(XzUnpacker_Code), and whether liblzma (Python's lzma) accepts the file.
Results only: no input is stored.

Prints the per-class counts, the share of refused cases tagged code_differs
(at most 20 %) and the STRICTER list, and asserts the case table's conditions
(xz_handmade.check_table).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import xz_handmade as H  # noqa: E402


def main():
    assert H.have_ref(), "build oracle/_ref first: make -f oracle/Makefile.ref"
    cs = H.all_cases()
    rec = {c["name"]: H.record(c) for c in cs}
    stats = H.check_table(cs, rec)
    for cls, n in stats["classes"].items():
        print(f"{cls:14s} {n[0]:4d} cases, {n[1]:3d} refused, {n[2]:2d} tagged code_differs")
    print(f"{len(cs)} cases; {stats['refused']} refused, {stats['tagged']} of them tagged "
          f"code_differs ({100.0 * stats['tagged'] / stats['refused']:.1f} %)")
    print("STRICTER (the reference accepts, liblzma and this project refuse):")
    for name, why in H.STRICTER.items():
        print(f"  {name}: {why}")
    with open(H.GOLDEN, "w") as f:
        json.dump({"generator": "tests/golden/make_golden_xzh.py",
                   "reference": "LZMA SDK 9.20 Xzs_ReadBackward (XzIn.c), XzUnpacker_Code "
                                "(XzDec.c) -- oracle/Makefile.ref, oracle/ref_shim.c",
                   "cases": rec}, f, indent=0, sort_keys=True)
    print(f"wrote {os.path.relpath(H.GOLDEN)}: {os.path.getsize(H.GOLDEN)} bytes")


if __name__ == "__main__":
    main()

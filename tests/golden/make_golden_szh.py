"""Generate tests/golden/szh_cases.json: the reference's answers for the
hand-made 7z archives of tests/sz_handmade.py.

Run where oracle/_ref is built (`make -f oracle/Makefile.ref`, which compiles
7zIn.c and 7zDec.c in place into libref.so and, with the host sanitizers, into
the program ref_7z_check):

    python tests/golden/make_golden_szh.py

Per case: the SHA-256 of the generated archive (so generator drift is caught),
its tags, and -- unless the case is tagged ref_undefined and never handed to the
reference -- SzArEx_Open's result, per folder {NumCoders, unpack size,
UnpackCRCDefined, UnpackCRC, NumUnpackStreams}, per file {HasStream, IsDir,
CrcDefined, Crc, folder index, size, SzArEx_Extract's result}, and hashes of
the name buffer and of the extracted bytes.  Results only: no input is stored.

Every untagged archive first goes through ref_7z_check, one process each: the
file is written only if no run is ended by a sanitizer and each run's answers
equal the library's.  Prints the per-class counts and asserts the case table's
conditions (sz_handmade.check_table) on the reference's answers alone.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sz_handmade as H  # noqa: E402


def main():
    assert H.have_ref(), "build oracle/_ref first: make -f oracle/Makefile.ref"
    assert os.path.exists(H.CHECK_EXE), "oracle/_ref/ref_7z_check is not built"
    cs = H.all_cases()
    dirty = []
    for c in cs:
        if "ref_undefined" in c["tags"]:
            continue
        status, got, report = H.run_sanitized(c)
        if status != 0:
            dirty.append(c["name"])
            print(f"{c['name']}: ref_7z_check ended with {status}\n{report}", file=sys.stderr)
        elif got != H.ref_answers(c["data"], "ref_unset" in c["tags"]):
            dirty.append(c["name"])
            print(f"{c['name']}: the sanitized program and libref.so answer differently",
                  file=sys.stderr)
    assert not dirty, f"the reference's answer rests on undefined behaviour: {dirty}"
    rec = {c["name"]: H.record(c) for c in cs}
    stats = H.check_table(cs, rec)
    for cls, n in stats["classes"].items():
        print(f"{cls:12s} {n[0]:4d} cases, {n[1]:3d} with a refusal, {n[2]:2d} tagged code_differs")
    print(f"{len(cs)} cases, every untagged one clean under the sanitizers; {stats['refused']} "
          f"refused at open ({stats['failing']} with a refusal), {stats['tagged']} of them tagged code_differs; {stats['undefined']} tagged "
          f"ref_undefined")
    print("STRICTER (the reference accepts, this project refuses):")
    for name, why in H.STRICTER.items():
        print(f"  {name}: {why}")
    with open(H.GOLDEN, "w") as f:
        json.dump({"generator": "tests/golden/make_golden_szh.py",
                   "reference": "LZMA SDK 9.20 SzArEx_Open, SzArEx_Extract (7zIn.c, 7zDec.c) -- "
                                "oracle/Makefile.ref, oracle/ref_shim.c, oracle/ref_7z_check.c",
                   "cases": rec}, f, indent=0, sort_keys=True)
    print(f"wrote {os.path.relpath(H.GOLDEN)}: {os.path.getsize(H.GOLDEN)} bytes")


if __name__ == "__main__":
    main()

"""Generate tests/golden/ppmd7enc_cases.json + ppmd7enc_blob.bin: small plain
buffers and the streams the REFERENCE's PPMd7 encoder (Ppmd7.c, Ppmd7Enc.c)
makes of them, for the encoder tests.  Supplements ppmd7_cases.json, whose
streams are the same encoder's output but whose model sizes are all multiples
of 4 and whose plain text is not stored.

Run in the build container only:

    python tests/golden/make_golden_ppmd7enc.py

The reference is compiled in a temporary directory exactly as
make_golden_ppmd7.py does (its Ref class and driver are used as they are), and
every stream is decoded back by the reference's decoder before it is kept.
Only data is written to the tree.

The set: 56 streams of at most 4,096 plain bytes, walking three lists of
pairwise coprime length side by side --
  contents  empty, one byte, two equal bytes, 4,096 equal bytes, 0..255
            ascending twice, random bytes, text (word soup)
  orders    2, 7, 32, 63, 64
  mem_size  2,049 / 2,050 / 2,051 and eight more; nine of the eleven are no
            multiple of 4, so the model's alignment offset is 3, 2 or 1
"""
import hashlib
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ppmd7 as G  # noqa: E402

ORDERS = [2, 7, 32, 63, 64]
MEMS = [2049, 2050, 2051, 4097, 2048, 8194, 16387, 65537, 1 << 16, 70002, 32771]
COUNT = 56


def content(kind, k):
    if kind == 0:
        return "empty", b""
    if kind == 1:
        return "one byte", bytes([(37 * k + 1) & 0xFF])
    if kind == 2:
        return "two equal bytes", bytes([(91 * k + 7) & 0xFF]) * 2
    if kind == 3:
        return "4096 equal bytes", bytes([(53 * k) & 0xFF]) * 4096
    if kind == 4:
        return "0..255 ascending twice", bytes(range(256)) * 2
    if kind == 5:
        return "random bytes", G.random_bytes(300 + k, 1024 + (k * 97) % 1024)
    return "word soup", G.word_soup(300 + k, 4096 - (k * 131) % 1500)


def main():
    tmp = tempfile.mkdtemp(prefix="ppmd7enc_golden_")
    try:
        ref = G.Ref(tmp, False)
        blob = bytearray()

        def put(b):
            off = len(blob)
            blob.extend(b)
            return off

        cases = []
        for k in range(COUNT):
            order, mem = ORDERS[k % len(ORDERS)], MEMS[k % len(MEMS)]
            name, plain = content(k % 7, k)
            packed = ref.encode(order, mem, plain)
            res = ref.decode(order, mem, packed, len(plain))
            assert res == (0, len(plain), len(packed), plain), (k, res[:3])
            cases.append({"order": order, "mem_size": mem, "content": name,
                          "plain_off": put(plain), "plain_len": len(plain),
                          "off": put(packed), "len": len(packed),
                          "sha256": hashlib.sha256(plain).hexdigest()})

        # the conditions the set is made for
        assert len(cases) >= 48 and all(c["plain_len"] <= 4096 for c in cases)
        for r in (1, 2, 3):
            assert sum(c["mem_size"] & 3 == r for c in cases) >= 8
        assert {2049, 2050, 2051} <= {c["mem_size"] for c in cases}
        assert {c["order"] for c in cases} == set(ORDERS)
        assert len({c["content"] for c in cases}) == 7

        with open(os.path.join(HERE, "ppmd7enc_blob.bin"), "wb") as f:
            f.write(blob)
        meta = {"generator": "tests/golden/make_golden_ppmd7enc.py",
                "reference": "LZMA SDK 9.20 Ppmd7.c / Ppmd7Enc.c / Ppmd7Dec.c compiled where they "
                             "lie: Ppmd7_EncodeSymbol per byte, no end mark, then "
                             "Ppmd7z_RangeEnc_FlushData; decoded back by the rules of SzDecodePpmd",
                "blob": "ppmd7enc_blob.bin", "blob_sha256": hashlib.sha256(blob).hexdigest(),
                "cases": cases}
        text = json.dumps(meta, indent=0)
        with open(os.path.join(HERE, "ppmd7enc_cases.json"), "w") as f:
            f.write(text)
        assert len(blob) + len(text) < 512 << 10
        print(f"{len(cases)} cases, blob {len(blob)} B, json {len(text)} B")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

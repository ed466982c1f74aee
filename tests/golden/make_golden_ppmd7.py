"""Generate tests/golden/ppmd7_cases.json + ppmd7_blob.bin from the REFERENCE
PPMd7 codec (Ppmd7.c, Ppmd7Enc.c, Ppmd7Dec.c).

Run in the build container only:

    python tests/golden/make_golden_ppmd7.py

The reference's encoder is not part of oracle/_ref/libref.so, so this script
compiles the three reference files where they lie, together with the small
driver below (this project's own: the byte reader, loop and result rules of
SzDecodePpmd, 7zDec.c:66-122, over a memory buffer), into a temporary
directory, and removes it afterwards.  Only data is written to the tree.

Output:
  cases    the well-formed streams: order, mem_size, packed bytes (blob offset /
           length), plain length and sha256, how the plain text was made
  mutated  corrupt and cut variants of the cases of at most 30,000 symbols: the
           base case, the recipe (applied in order to the base's packed bytes /
           plain length) and the reference's {res, dest_len, src_len} with the
           sha256 of the bytes it wrote
  sevenz   streams the 7z tests wrap in folders (one over x86-BCJ-encoded text)
  bench    one order-6 / 16 MiB stream, 7-Zip's usual setting, for ppmd7_bench.py
  coverage the gcov line summary of Ppmd7.c and Ppmd7Dec.c after decoding the
           unmutated cases in a --coverage build: must be 100 % of both
"""
import hashlib
import json
import os
import random
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get("LZMA_REF", "/root/reference")

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "Ppmd7.h"

static void *a_alloc(void *p, size_t n) { (void)p; return malloc(n); }
static void a_free(void *p, void *a) { (void)p; free(a); }
static ISzAlloc g_alloc = { a_alloc, a_free };

typedef struct { IByteIn p; const Byte *cur, *end, *begin; int extra; } MemIn;
static Byte mem_read(void *pp) {
  MemIn *s = (MemIn *)pp;
  if (s->cur != s->end) return *s->cur++;
  s->extra = 1;
  return 0;
}
typedef struct { IByteOut p; FILE *f; } FileOut;
static void file_write(void *pp, Byte b) { fputc(b, ((FileOut *)pp)->f); }

static Byte *slurp(const char *path, size_t *n) {
  FILE *f = fopen(path, "rb");
  Byte *b;
  if (!f) exit(3);
  fseek(f, 0, SEEK_END); *n = (size_t)ftell(f); fseek(f, 0, SEEK_SET);
  b = (Byte *)malloc(*n + 1);
  if (fread(b, 1, *n, f) != *n) exit(3);
  fclose(f);
  return b;
}

int main(int argc, char **argv) {
  unsigned order; UInt32 mem; size_t n, i; Byte *in; CPpmd7 pp;
  if (argc < 6) return 2;
  order = (unsigned)atoi(argv[2]); mem = (UInt32)strtoul(argv[3], 0, 10);
  in = slurp(argv[4], &n);
  Ppmd7_Construct(&pp);
  if (!Ppmd7_Alloc(&pp, mem, &g_alloc)) return 4;
  Ppmd7_Init(&pp, order);
  if (!strcmp(argv[1], "enc")) {
    CPpmd7z_RangeEnc rc; FileOut o;
    o.p.Write = file_write; o.f = fopen(argv[5], "wb");
    rc.Stream = &o.p;
    Ppmd7z_RangeEnc_Init(&rc);
    for (i = 0; i < n; i++) Ppmd7_EncodeSymbol(&pp, &rc, in[i]);
    Ppmd7z_RangeEnc_FlushData(&rc);
    fclose(o.f);
  } else {
    /* dec ORDER MEM src out DSTLEN: the rules of SzDecodePpmd */
    size_t out_size = (size_t)strtoull(argv[6], 0, 10);
    Byte *out = (Byte *)malloc(out_size + 1);
    CPpmd7z_RangeDec rc; MemIn s; int res = 0; FILE *f;
    s.p.Read = mem_read; s.begin = s.cur = in; s.end = in + n; s.extra = 0;
    Ppmd7z_RangeDec_CreateVTable(&rc);
    rc.Stream = &s.p;
    i = 0;
    if (!Ppmd7z_RangeDec_Init(&rc)) res = 1;
    else if (s.extra) res = 1;
    else {
      for (i = 0; i < out_size; i++) {
        int sym = Ppmd7_DecodeSymbol(&pp, &rc.p);
        if (s.extra || sym < 0) break;
        out[i] = (Byte)sym;
      }
      if (i != out_size) res = 1;
      else if ((size_t)(s.cur - s.begin) != n || !Ppmd7z_RangeDec_IsFinishedOK(&rc)) res = 1;
    }
    f = fopen(argv[5], "wb"); fwrite(out, 1, i, f); fclose(f);
    printf("%d %lu %lu\n", res, (unsigned long)i, (unsigned long)(s.cur - s.begin));
  }
  Ppmd7_Free(&pp, &g_alloc);
  return 0;
}
"""

WORDS = ("the of and to in is that it was for on are as with his they at be this from have or "
         "by one had not but what all were when we there can an your which their said if do "
         "will each about how up out them then she many some so these would other into has more "
         "her two like him see time could no make than first been its who now people my made "
         "over did down only way find use may water long little very after words called just "
         "where most know").split()


def word_soup(seed, n):
    rng = random.Random(seed)
    out = []
    size = 0
    while size < n:
        w = rng.choice(WORDS)
        if rng.random() < 0.08:
            w = w.capitalize()
        w += rng.choice([" ", " ", " ", " ", ", ", ". ", "\n"])
        out.append(w)
        size += len(w)
    return "".join(out).encode()[:n]


def skewed8(seed, n):
    """An 8-letter source with a steep distribution, one byte in ten random."""
    rng = random.Random(seed)
    letters = b"etaoinsh"
    weights = [128, 64, 32, 16, 8, 4, 2, 1]
    body = rng.choices(letters, weights, k=n)
    return bytes(rng.randrange(256) if rng.random() < 0.1 else b for b in body)


def random_bytes(seed, n):
    return random.Random(seed).randbytes(n)


def a_with_noise(seed, n):
    rng = random.Random(seed)
    return bytes(rng.randrange(256) if i % 7 == 6 else 0x61 for i in range(n))


def broken_runs(seed, n):
    """A short phrase repeated 30-60 times, then one random byte, and again:
    one-symbol contexts grow old before a second symbol arrives."""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += rng.choice(WORDS).encode() * rng.randrange(30, 60) + bytes([rng.randrange(256)])
    return bytes(out[:n])


GEN = {"broken runs": broken_runs, "word soup": word_soup, "skewed 8-letter source, 10 % noise": skewed8,
       "random bytes": random_bytes, "'a' with a random byte every 7th": a_with_noise}

# (order, mem_size, plain size, content): the set that reaches every line of the
# reference's model and decoder; the three long ones reach Rescale's shrink path,
# the 2 KiB ones force restarts and GlueFreeBlocks (the order-2 one a failed
# CreateSuccessors at full order), the broken runs the frequency clamp of a
# one-symbol context that gets its second symbol
CASES = [
    (6, 2048, 8192, "word soup"),
    (64, 2048, 8192, "skewed 8-letter source, 10 % noise"),
    (2, 4096, 4096, "random bytes"),
    (16, 16 << 10, 20000, "'a' with a random byte every 7th"),
    (8, 64 << 10, 30000, "word soup"),
    (2, 1 << 20, 200000, "'a' with a random byte every 7th"),
    (3, 1 << 20, 200000, "skewed 8-letter source, 10 % noise"),
    (4, 256 << 10, 100000, "'a' with a random byte every 7th"),
    (4, 8192, 8192, "broken runs"),
    (2, 2048, 8192, "word soup"),
    (3, 2048, 8192, "skewed 8-letter source, 10 % noise"),
]
MUT_MAX_SYMBOLS = 30000


class Ref:
    def __init__(self, tmp, coverage):
        self.tmp = tmp
        self.exe = os.path.join(tmp, "drv_cov" if coverage else "drv")
        self.n = 0
        with open(os.path.join(tmp, "driver.c"), "w") as f:
            f.write(DRIVER)
        srcs = [os.path.join(REF, x) for x in ("Ppmd7.c", "Ppmd7Enc.c", "Ppmd7Dec.c")]
        flags = ["-O1", "--coverage"] if coverage else ["-O2"]
        subprocess.run(["gcc", "-w", *flags, "-I", REF, "-o", self.exe,
                        os.path.join(tmp, "driver.c"), *srcs], check=True, cwd=tmp)

    def _tmpfile(self, data):
        self.n += 1
        p = os.path.join(self.tmp, f"f{self.n}")
        with open(p, "wb") as f:
            f.write(data)
        return p

    def encode(self, order, mem, plain):
        src, out = self._tmpfile(plain), self._tmpfile(b"")
        subprocess.run([self.exe, "enc", str(order), str(mem), src, out], check=True, cwd=self.tmp)
        with open(out, "rb") as f:
            packed = f.read()
        os.unlink(src), os.unlink(out)
        return packed

    def decode(self, order, mem, packed, dst_len):
        src, out = self._tmpfile(packed), self._tmpfile(b"")
        r = subprocess.run([self.exe, "dec", str(order), str(mem), src, out, str(dst_len)],
                           check=True, cwd=self.tmp, capture_output=True, text=True)
        res, dest_len, src_len = (int(x) for x in r.stdout.split())
        with open(out, "rb") as f:
            written = f.read()
        os.unlink(src), os.unlink(out)
        assert len(written) == dest_len
        return res, dest_len, src_len, written


def recipes(rng, packed_len, plain_len):
    out = []
    for k in range(1, 9):
        out.append([["trunc", k]])
    for _ in range(12):
        out.append([["flip", rng.randrange(1, packed_len), 1 << rng.randrange(8)]])
    for _ in range(6):
        out.append([["flip", rng.randrange(1, min(packed_len, 12)), rng.randrange(1, 256)]])
    for _ in range(4):
        out.append([["flip", rng.randrange(1, packed_len), rng.randrange(1, 256)] for _ in range(3)])
    out.append([["append", "00"]])
    out.append([["append", "0000000000"]])
    out.append([["append", rng.randbytes(3).hex()]])
    out.append([["first", 1]])
    out.append([["first", 0xFF]])
    out.append([["flip", 1, 0xFF], ["flip", 2, 0xFF], ["flip", 3, 0xFF], ["flip", 4, 0xFF]])
    for n in (0, 1, plain_len - 1, plain_len // 2, plain_len + 1, plain_len + 100):
        out.append([["dst_len", n]])
    out.append([["trunc", packed_len - 4]])
    out.append([["trunc", packed_len - 5]])
    out.append([["trunc", packed_len]])
    out.append([["trunc", packed_len // 2], ["dst_len", plain_len // 2]])
    out.append([["flip", rng.randrange(1, packed_len), 0x10], ["trunc", 2]])
    return out


def main():
    import sevenzwrite as Z
    from ppmd7_golden import apply_recipe
    tmp = tempfile.mkdtemp(prefix="ppmd7_golden_")
    try:
        ref, cov = Ref(tmp, False), Ref(tmp, True)
        blob = bytearray()

        def put(b):
            off = len(blob)
            blob.extend(b)
            return off

        def make(order, mem, n, content, seed, plain=None):
            if plain is None:
                plain = GEN[content](seed, n)
            packed = ref.encode(order, mem, plain)
            res = ref.decode(order, mem, packed, len(plain))
            assert res == (0, len(plain), len(packed), plain), res[:3]
            return {"order": order, "mem_size": mem, "content": content, "seed": seed,
                    "off": put(packed), "len": len(packed), "plain_len": len(plain),
                    "sha256": hashlib.sha256(plain).hexdigest()}, packed, plain

        cases, packs = [], []
        for i, (order, mem, n, content) in enumerate(CASES):
            c, packed, plain = make(order, mem, n, content, 100 + i)
            cases.append(c)
            packs.append(packed)
            # the coverage condition: unmutated cases only, through the --coverage build
            assert cov.decode(order, mem, packed, n) == (0, n, len(packed), plain)

        coverage = {}
        gc = subprocess.run(["gcov", "-o", tmp] + [f"drv_cov-{x}.gcda" for x in ("Ppmd7", "Ppmd7Dec")],
                            cwd=tmp, capture_output=True, text=True).stdout
        print(gc)
        for m in re.finditer(r"File '([^']*)'\nLines executed:([0-9.]+)% of (\d+)", gc):
            name = os.path.basename(m.group(1))
            if name in ("Ppmd7.c", "Ppmd7Dec.c"):
                coverage[name] = {"percent": float(m.group(2)), "lines": int(m.group(3))}
        assert set(coverage) == {"Ppmd7.c", "Ppmd7Dec.c"}, gc
        for name in coverage:  # lines the cases do not reach (none, or the set needs more inputs)
            with open(os.path.join(tmp, name + ".gcov")) as f:
                for line in f:
                    if line.lstrip().startswith("#####"):
                        print(name, line.rstrip())
        assert all(v["percent"] == 100.0 for v in coverage.values()), coverage

        rng = random.Random(7)
        mutated = []
        for bi, c in enumerate(cases):
            if c["plain_len"] > MUT_MAX_SYMBOLS:
                continue
            for ops in recipes(rng, c["len"], c["plain_len"]):
                packed, dst_len = apply_recipe(packs[bi], c["plain_len"], ops)
                res, dest_len, src_len, written = ref.decode(c["order"], c["mem_size"], packed,
                                                             dst_len)
                mutated.append({"base": bi, "ops": ops, "res": res, "dest_len": dest_len,
                                "src_len": src_len,
                                "sha256": hashlib.sha256(written).hexdigest()})

        # 7z folders: text for plain PPMd folders, x86-flavoured bytes filtered
        # by the BCJ encoder first for the BCJ + PPMd folder
        import bcj2enc
        sevenz = []
        c, _, _ = make(6, 1 << 16, 12000, "word soup", 201)
        sevenz.append(dict(c, name="text"))
        c, _, _ = make(5, 1 << 18, 9000, "skewed 8-letter source, 10 % noise", 202)
        sevenz.append(dict(c, name="letters"))
        code = bcj2enc.x86_like(9, 6000, density=0.05)
        c, _, _ = make(4, 1 << 16, len(code), "x86-like bytes, BCJ-encoded before packing", 9,
                       plain=Z.x86_encode(code))
        sevenz.append(dict(c, name="bcj", unfiltered_sha256=hashlib.sha256(code).hexdigest(),
                           unfiltered_generator="bcj2enc.x86_like(9, 6000, density=0.05)"))

        c, _, _ = make(6, 16 << 20, 30000, "word soup", 104)  # case 4's text at 7-Zip's setting
        bench = [c]

        with open(os.path.join(HERE, "ppmd7_blob.bin"), "wb") as f:
            f.write(blob)
        meta = {"generator": "tests/golden/make_golden_ppmd7.py",
                "reference": "LZMA SDK 9.20 Ppmd7.c / Ppmd7Enc.c / Ppmd7Dec.c compiled where they "
                             "lie, driven by the rules of SzDecodePpmd (7zDec.c:66-122)",
                "blob": "ppmd7_blob.bin", "blob_sha256": hashlib.sha256(blob).hexdigest(),
                "coverage": coverage, "cases": cases, "mutated": mutated, "sevenz": sevenz,
                "bench": bench}
        with open(os.path.join(HERE, "ppmd7_cases.json"), "w") as f:
            json.dump(meta, f, indent=0)
        print(f"{len(cases)} cases, {len(mutated)} mutated "
              f"(results {sorted({m['res'] for m in mutated})}), blob {len(blob)} B, "
              f"coverage {coverage}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()

"""Encoder cases whose dictionary exceeds 64 KiB: a hash mask wider than 0xFFFF
(0x1FFFF from a 128 KiB + 1 dictionary on, 0x7FFFFF at 16 MiB), matches farther
than 64 KiB (pos slots from 32 up, 11 and more direct bits, the align prices at
those slots, a distTableSize above 32) and a ring that wraps beyond 64 KiB.
Shared by test_lzmaenc_bigdict_emu.py, test_lzmaenc_bigdict_gpu.py and
tests/golden/make_golden_lzmaenc_bigdict.py.

A case is lzmaenc_opt_cases.case's dict.  Expected results come from the live
reference where it is built, else from tests/golden/lzmaenc_bigdict_cases.json
(sizes, SHA-256, first 32 bytes, props; inputs are never stored).

The four parser and finder combinations, by the props that select them:
"opt_bt4" (level 5 as it is), "fast_bt4" (level 1, btMode 1), "opt_hc4"
(level 5, btMode 0) and "fast" (level 1: the fast path)."""
import json
import os
import random
import shutil
import subprocess

import lzma2enc_cases as C2
import lzmaenc_cases as C
import lzmaenc_opt_cases as O
import native

GOLDEN = os.path.join(native.ROOT, "tests", "golden", "lzmaenc_bigdict_cases.json")
key, data_of, check, sha = O.key, O.data_of, O.check, O.sha

MODES = {"opt_bt4": dict(level=5), "fast_bt4": dict(level=1, bt=1), "opt_hc4": dict(level=5, bt=0),
         "fast": dict(level=1)}
NORMAL_MODES = ("opt_bt4", "fast_bt4", "opt_hc4")
DICTS = ((1 << 16) + 1, (1 << 17) + 1, 3 << 16, 1 << 18, 1 << 20, 1 << 24)
BIG_DICT = 1 << 24      # 32 MiB of hash per stream: at most four of them in a device batch

FAR_KIND, FAR_N = "far:66000", 70000     # the block returns 67,024 bytes back: 11 direct bits
X_KIND, X_N = "far:1050000", 1100000     # above 1 MiB: 15 and more direct bits

# name -> (kind, seed, n, props); every shape but W, X and X_ctl exists in all four modes
SHAPES = {
    "F": (FAR_KIND, 41, FAR_N, dict(dict=1 << 18)),
    "F_ctl": (FAR_KIND, 41, FAR_N, dict(dict=1 << 16)),       # the far match is out of reach
    "M": ("copy", 43, 40000, dict(dict=1 << 18, mc=2)),       # the wide hash mask
    "M24": ("copy", 43, 40000, dict(dict=1 << 24, mc=2)),     # mask 0x7FFFFF
    "C80": ("copy", 42, 80000, dict(dict=1 << 18)),           # far matches at many distances
}
FAST_ONLY = {
    "W": ("copy", 31, 140000, dict(dict=(1 << 17) + 1)),      # the ring wraps with a wide mask
    "X": (X_KIND, 46, X_N, dict(dict=1 << 21)),
    "X_ctl": (X_KIND, 46, X_N, dict(dict=(1 << 20) + 1)),
}
# the product's defaults: the level's own dictionary (256 KiB, 1 MiB, 4 MiB, 16 MiB)
DEFAULTS = {"D%d" % level: (FAR_KIND, 41, FAR_N, dict(level=level, dict=0)) for level in (2, 3, 4, 5)}


def named(name, mode="fast"):
    """The named case in one of MODES (W, X, X_ctl: "fast" only; D2..D5: the
    level decides, `mode` is not looked at)."""
    if name in DEFAULTS:
        kind, seed, n, kw = DEFAULTS[name]
        return O.case(kind, seed, n, **kw)
    kind, seed, n, kw = SHAPES[name] if name in SHAPES else FAST_ONLY[name]
    assert name in SHAPES or mode == "fast", (name, mode)
    return O.case(kind, seed, n, **dict(kw, **MODES[mode]))


def named_cases():
    """[(name, mode, case)] of every named case."""
    out = [(name, mode, named(name, mode)) for name in SHAPES for mode in MODES]
    out += [(name, "fast", named(name)) for name in FAST_ONLY]
    out += [(name, "opt_bt4" if name == "D5" else "fast", named(name)) for name in DEFAULTS]
    return out


def random_cases(count=60, seed=20262):
    """Seeded shapes in the style of lzmaenc_opt_cases.random_cases over the
    large dictionaries: up to 90,000 bytes on the fast path (so that matches lie
    beyond 64 KiB), up to 30,000 in the normal modes (the wide mask alone)."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        mode = rng.choice(("fast", "fast", "fast", "opt_bt4", "fast_bt4", "opt_hc4"))
        max_n = 90000 if mode == "fast" else 30000
        n = rng.choice((rng.randrange(0, 600), rng.randrange(0, max_n + 1),
                        rng.randrange(max_n // 2, max_n + 1), rng.randrange(max_n // 2, max_n + 1)))
        kind = rng.choice(("copy", "far:%d" % rng.randrange(max(n, 1))))
        lc, lp, pb = rng.choice(((-1, -1, -1), (-1, -1, -1), (0, 0, 0), (3, 0, 2), (0, 4, 4),
                                 (8, 4, 4), (4, 2, 1)))
        cap = rng.choice((None, None, None, "full+0", "full-1"))
        out.append(O.case(kind, rng.randrange(1 << 30), n, dict=rng.choice(DICTS), lc=lc, lp=lp,
                          pb=pb, fb=rng.choice((-1, 5, 32, 64, 273)), mc=rng.choice((0, 0, 2, 4)),
                          end_mark=rng.randrange(2), cap=cap, **MODES[mode]))
    return out


def golden_cases():
    return [c for _, _, c in named_cases()] + random_cases()


def batches(cases, max_big=4):
    """The cases in order, cut so that no batch holds more than max_big streams
    with a 16 MiB dictionary (level 5 with dict 0 is one)."""
    out, big = [[]], 0
    for c in cases:
        is_big = c["dict"] == BIG_DICT or (c["dict"] == 0 and c["level"] >= 5)
        if is_big and big == max_big:
            out.append([])
            big = 0
        big += is_big
        out[-1].append(c)
    return out


# ---------------------------------------------------------------- LZMA2 and sessions

LZMA2_NAMES = ("F", "M", "C80", "F_ctl", "W")


def lzma2_case(name, level):
    """The named shape's bytes as one LZMA2 block (lc3 lp0 pb2, the level's mc)."""
    kind, seed, n, kw = SHAPES[name] if name in SHAPES else FAST_ONLY[name]
    return C2.case([(kind, seed, n)], level=level, dict=kw["dict"])


def lzma2_cases():
    """W at level 1 only (one normal-mode lane would need tens of seconds)."""
    return [lzma2_case(name, level) for name in LZMA2_NAMES
            for level in ((1,) if name == "W" else (1, 5))]


def lzma2_expect(c, golden=None):
    if native.have_ref():
        return C2.expect(c)
    return dict((golden or load_golden())["lzma2_by_key"][C2.key(c)], out=None)


SESSION_NAMES = ("F", "M", "W")
SESSION_SCHEDULES = ("p546", "random", "one", "p4096")


def pieces_of(name, n, seed=0):
    """lzmaenc_session_cases.pieces_of plus fixed 4,096-byte pieces."""
    import lzmaenc_session_cases as S
    if name == "p4096":
        return [4096] * (n // 4096) + ([n % 4096] if n % 4096 else [])
    return S.pieces_of(name, n, seed)


# ---------------------------------------------------------------- goldens

def load_golden():
    with open(GOLDEN) as f:
        d = json.load(f)
    d["by_key"] = {key(g["case"]): g for g in d["cases"]}
    d["lzma2_by_key"] = {C2.key(g["case"]): g for g in d["lzma2"]}
    return d


_want = {}


def expect(c, golden=None):
    """The reference's result for a case, computed once and shared: live where
    the library is built, else the golden (out is then None)."""
    k = key(c)
    if k not in _want:
        if native.have_ref():
            _want[k] = O.expect(c)
        else:
            _want[k] = O.golden_want((golden or load_golden())["by_key"][k])
    return _want[k]


# ---------------------------------------------------------------- mutants of the emulator

# textual replacements in csrc/lzmaenc_device.h, each of which a correct test
# of these cases must notice: (pattern, replacement)
MUTANT_NARROW_MASK = ("  if (hs > (1u << 24)) hs >>= 1;\n  return hs;\n",
                      "  if (hs > (1u << 24)) hs >>= 1;\n  return 0xFFFF;\n")
MUTANT_DIRECT_BIT_10 = (
    "  LZENC_FN void encode_direct_bits(uint32_t value, int numBits) {\n",
    "  LZENC_FN void encode_direct_bits(uint32_t value, int numBits) {\n"
    "    if (numBits > 10) value ^= 1u << 10;\n")


def build_mutant(out_dir, mutant):
    """The one-shot emulator built from a copy of lzmaenc_device.h with one
    replacement made (the copy sits beside a copy of the emulator's source, where
    the include finds it first).  Returns the loaded library."""
    pattern, replacement = mutant
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(C.CSRC, "lzmaenc_device.h")) as f:
        text = f.read()
    assert text.count(pattern) == 1, pattern
    with open(os.path.join(out_dir, "lzmaenc_device.h"), "w") as f:
        f.write(text.replace(pattern, replacement))
    src = shutil.copy(O.EMU_SRC, out_dir)
    so = os.path.join(out_dir, "liblzmaenc_opt_emu_mutant.so")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", C.CSRC, "-fPIC", "-shared", "-O2",
                    src, "-o", so], check=True)
    return O.load_emu(so)


def differs(lib, c, want):
    """Whether the library's stream of the case is not the expected one."""
    res, dl, _, out = O.emu_encode(lib, data_of(c), c, want["cap"])
    return (res, dl, sha(out)) != (want["res"], want["dest_len"], want["sha256"])

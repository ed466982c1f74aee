"""Cases and reference access for the normal-mode LZMA encoder tests (the
optimal parser and the Bt4 finder: test_lzmaenc_opt_emu.py,
test_lzmaenc_opt_gpu.py) and for tests/golden/make_golden_lzmaenc_opt.py.

A case is lzmaenc_cases' dict plus "nhb" (the props' numHashBytes, -1 = the
default).  Expected results come from the live reference's LzmaEncode with the
case's full CLzmaEncProps (single-threaded, as oracle/Makefile.ref builds it)
where it is built, else from tests/golden/lzmaenc_opt_cases.json (sizes,
SHA-256, first 32 bytes).  `expect` here differs from lzmaenc_cases.expect in
one thing: with both modes allowed, algo 1 and btMode 1 are encoded, and only
btMode 1 with numHashBytes below 4 (Bt2 / Bt3) is SZ_ERROR_UNSUPPORTED."""
import ctypes
import json
import os
import random
import struct
import subprocess

import lzmaenc_cases as C
import native

GOLDEN = os.path.join(native.ROOT, "tests", "golden", "lzmaenc_opt_cases.json")
EMU_SRC = os.path.join(native.ROOT, "tests", "emu_lzmaenc_opt", "lzmaenc_opt_emu.cpp")
OK, UNSUPPORTED, PARAM, OUTPUT_EOF = C.OK, C.UNSUPPORTED, C.PARAM, C.OUTPUT_EOF
MODE_OPTIMAL, MODE_BT4 = 1, 2
ALL_MODES = MODE_OPTIMAL | MODE_BT4
key, data_of, check, sha = C.key, C.data_of, C.check, C.sha


def case(kind, seed, n, level=5, nhb=-1, **kw):
    c = C.case(kind, seed, n, level=level, **kw)
    c["nhb"] = nhb
    return c


def edge_cases():
    """Every line of GetOptimum, Backward, the Bt4 finder and the price tables
    (the list was run on a coverage build of the reference)."""
    out = []
    for n in range(7):
        for em in (0, 1):
            out.append(case("text", 100 + n, n, dict=4096, end_mark=em))
    for n in (273, 274, 600):                # the repLens >= fb return
        for fb in (5, 32, 273):
            out.append(case("byte", 7, n, fb=fb))
    out.append(case("period2", 8, 1000))     # the mainLen >= fb return
    for n in (4095, 4096, 4097, 20000):      # ring wrap; text 20000: kNumOpts clamp, truncation
        out.append(case("text", 9, n, dict=4096))
        out.append(case("copy", 10, n, dict=4096))
    out.append(case("text", 20, 5001, dict=5000))            # the smallest shape at the clamp
    out.append(case("copy", 21, (3 << 11) + 1, dict=3 << 11))
    out.append(case("text", 22, 300, dict=1))
    out.append(case("distant", 11, 40 * 1024, dict=1 << 16))
    for lc, lp, pb in ((0, 0, 0), (3, 0, 2), (0, 4, 4), (8, 4, 4)):
        out.append(case("text", 13, 3000, lc=lc, lp=lp, pb=pb, end_mark=1))
        out.append(case("copy", 14, 3000, lc=lc, lp=lp, pb=pb))   # newLen >= fb inside the loop
    for mc in (1, 4, 48):                    # the tree's cut
        out.append(case("copy", 15, 6000, mc=mc))
        out.append(case("text", 16, 6000, mc=mc, fb=64))
    out.append(case("runs", 18, 20000, fb=273, dict=4096))
    out.append(case("text", 24, 20000, fb=273, dict=1 << 16))
    out.append(case("copy", 25, 20000, fb=273, dict=1 << 16))
    out.append(case("random", 26, 9000, dict=4096))
    out.append(case("text", 23, 9000, level=7, dict=1 << 16))
    out.append(case("text", 23, 9000, level=1, bt=1, dict=1 << 16))   # Bt4 + fast parser
    out.append(case("copy", 27, 9000, level=5, bt=0, dict=1 << 16))   # optimal + Hc4
    for cap in ("full+0", "full-1", 65536, 5, 0):
        out.append(case("random", 12, 70 * 1024, dict=1 << 16, cap=cap))
    out.append(case("text", 19, 500, bt=1, nhb=3, dict=4096))         # Bt3: unsupported
    out.append(case("text", 19, 500, lc=9, dict=4096))                # SZ_ERROR_PARAM first
    return out


def random_cases(count, seed, max_n=20000):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        lc, lp, pb = rng.choice(((-1, -1, -1), (0, 0, 0), (3, 0, 2), (0, 4, 4), (8, 4, 4),
                                 (8, 0, 0), (0, 4, 0), (0, 0, 4), (4, 2, 1)))
        n = rng.choice((rng.randrange(0, 40), rng.randrange(0, 600), rng.randrange(0, max_n + 1),
                        rng.randrange(0, max_n + 1)))
        cap = rng.choice((None, None, None, "full+0", "full-1", "full+3", 0, rng.randrange(0, 64),
                          "full-%d" % rng.randrange(1, 40)))
        algo, bt = rng.choice(((-1, -1), (-1, -1), (-1, -1), (1, 0), (0, 1)))
        out.append(case(rng.choice(C.KINDS), rng.randrange(1 << 30), n, level=rng.randrange(5, 10),
                        dict=rng.choice((4096, 5000, 3 << 11, 1 << 16)), lc=lc, lp=lp, pb=pb,
                        fb=rng.choice((-1, 5, 6, 32, 64, 273)), algo=algo, bt=bt,
                        end_mark=rng.randrange(2), cap=cap))
    return out


# the plain LZMA folder of the 7z test: a level-5 row with a 64 KiB dictionary
SEVENZ_CASE = case("text", 28, 9000, dict=1 << 16)


def golden_cases():
    """The cases the golden file is generated over."""
    return edge_cases() + [SEVENZ_CASE] + random_cases(120, 20261)


# ---------------------------------------------------------------- the live reference

def mode_of(c):
    """The descriptor's mode bits for the case, from the reference's own
    LzmaEncProps_Normalize."""
    nz = C.ref_normalize(c) if native.have_ref() else None
    if nz is None:
        level = 5 if c["level"] < 0 else c["level"]
        algo = c["algo"] if c["algo"] >= 0 else (0 if level < 5 else 1)
        bt = c["bt"] if c["bt"] >= 0 else (1 if algo else 0)
    else:
        algo, bt = nz["algo"], nz["btMode"]
    return (MODE_OPTIMAL if algo else 0) | (MODE_BT4 if bt else 0)


def ref_expect(c, data=None):
    """(res, dest_len, props5, out, cap, full_len) of the case by the live
    reference, Bt2 / Bt3 excepted."""
    data = data_of(c) if data is None else data
    nz = C.ref_normalize(c)
    if nz["lc"] > 8 or nz["lp"] > 4 or nz["pb"] > 4 or nz["dictSize"] > (1 << 30):
        assert C._ref_call(data, c, 64)[0] == PARAM
        return PARAM, 0, b"\0" * 5, b"", 64, 0
    if nz["btMode"] and 0 <= c["nhb"] < 4:
        return UNSUPPORTED, 0, b"\0" * 5, b"", 64, 0
    full_len = 0
    if isinstance(c["cap"], str):
        r0 = C._ref_call(data, c, C.ample(len(data)))
        assert r0[0] == OK
        full_len = r0[1]
    cap = C.resolve_cap(c, full_len)
    res, dl, props5, out = C._ref_call(data, c, cap)
    return res, dl, props5, out, cap, full_len


def load_golden():
    with open(GOLDEN) as f:
        d = json.load(f)
    d["by_key"] = {key(g["case"]): g for g in d["cases"]}
    d["lzma2_by_key"] = {key(g["case"]): g for g in d["lzma2"]}
    return d


def golden_want(g):
    return {"res": g["res"], "dest_len": g["dest_len"], "props5": bytes.fromhex(g["props5"]),
            "cap": g["cap"], "sha256": g["sha256"], "head": bytes.fromhex(g["head"]), "out": None}


def expect(c, data=None, golden=None):
    """What the reference gives for the case: live where the library is built,
    else from the golden file (out is then None; compare len / sha256 / head)."""
    if native.have_ref():
        res, dl, props5, out, cap, _ = ref_expect(c, data)
        return {"res": res, "dest_len": dl, "props5": props5, "cap": cap, "sha256": sha(out),
                "head": out[:32], "out": out}
    return golden_want((golden or load_golden())["by_key"][key(c)])


# ---------------------------------------------------------------- the emulator

def build_emu(out_dir, extra=(), main=False, name=None):
    out = os.path.join(str(out_dir),
                       name or ("lzmaenc_opt_emu_main" if main else "liblzmaenc_opt_emu.so"))
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", C.CSRC]
    cmd += (["-DLZMAENC_OPT_EMU_MAIN"] if main else ["-fPIC", "-shared"])
    cmd += list(extra) if extra else ["-O2"]
    subprocess.run(cmd + [EMU_SRC, "-o", out], check=True)
    return out


def load_emu(so):
    lib = ctypes.CDLL(so)
    f = lib.lzmaenc_opt_emu_encode
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int,
                  ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                  ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                  ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
    lib.lzmaenc_opt_emu_slice_bytes.restype = ctypes.c_uint64
    lib.lzmaenc_opt_emu_slice_bytes.argtypes = [ctypes.c_uint32] * 6 + [ctypes.c_uint64]
    lib.lzmaenc_opt_emu_prob_price.restype = ctypes.c_uint32
    lib.lzmaenc_opt_emu_prob_price.argtypes = [ctypes.c_uint32]
    return lib


def emu_encode(lib, data, c, cap, poison=0x3C, allowed=ALL_MODES):
    dst = ctypes.create_string_buffer(b"\xEE" * (cap + 8), cap + 8)
    props5 = ctypes.create_string_buffer(5)
    dl = ctypes.c_uint64(0)
    res = lib.lzmaenc_opt_emu_encode(data, len(data), dst, cap, c["level"], c["dict"], c["lc"],
                                     c["lp"], c["pb"], c["fb"], c["mc"], c["algo"], c["bt"],
                                     c["nhb"], c["end_mark"], allowed, poison, props5,
                                     ctypes.byref(dl))
    assert dst.raw[cap:] == b"\xEE" * 8, "write past dst_cap"
    return res, dl.value, props5.raw, dst.raw[:dl.value]


def write_case_file(path, cases, golden=None):
    """Records for the stand-alone build of lzmaenc_opt_emu.cpp.  Expected bytes
    come from the live reference where built, else from the library build of
    the emulator, which the golden test pins."""
    lib = None
    with open(path, "wb") as f:
        for c in cases:
            data = data_of(c)
            want = expect(c, data, golden)
            out = want["out"]
            if out is None:
                if lib is None:
                    lib = load_emu(build_emu(os.path.dirname(path),
                                             name="liblzmaenc_opt_emu_dump.so"))
                got = emu_encode(lib, data, c, want["cap"])
                check(got, want, key(c))
                out = got[3]
            f.write(struct.pack("<iIiiiiIiiiiI", c["level"], c["dict"], c["lc"], c["lp"], c["pb"],
                                c["fb"], c["mc"], c["algo"], c["bt"], c["nhb"], c["end_mark"],
                                ALL_MODES))
            f.write(struct.pack("<QQiQ", len(data), want["cap"], want["res"], want["dest_len"]))
            f.write(want["props5"] + data + out)

"""Shared by the encoder-session tests (test_lzmaenc_session_emu.py,
test_lzmaenc_session_gpu.py): the session record as ctypes, piece schedules,
the host emulator (tests/emu_lzmaenc_session/lzmaenc_session_emu.cpp) and the
expected one-shot streams.

The expected output of a session is always the one-shot stream of the
concatenated input: tests/golden/lzmaenc_cases.json or the live reference
through lzmaenc_cases.expect() where the case is there; for inputs that are in
neither, the live reference where it is built, else the one-shot host emulator
(tests/emu_lzmaenc, which the goldens pin)."""
import ctypes
import os
import random
import struct
import subprocess

import lzmaenc_cases as C
import native

EMU_SRC = os.path.join(native.ROOT, "tests", "emu_lzmaenc_session", "lzmaenc_session_emu.cpp")
HOLD = 546
NEEDS_INPUT, FINISHED, BUDGET = 0, 1, 2
SCHEDULES = ("ones", "p545", "p546", "p547", "random", "one")


class Session(ctypes.Structure):
    """LzmaEncGpuSession (include/lzma_gpu.h), 200 bytes."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("ws", ctypes.c_void_p),
                ("src_cap", ctypes.c_uint64), ("dst_cap", ctypes.c_uint64),
                ("src_len", ctypes.c_uint64), ("in_budget", ctypes.c_uint64),
                ("in_pos", ctypes.c_uint64), ("out_pos", ctypes.c_uint64),
                ("dict_size", ctypes.c_uint32), ("lc", ctypes.c_uint32), ("lp", ctypes.c_uint32),
                ("pb", ctypes.c_uint32), ("fb", ctypes.c_uint32), ("mc", ctypes.c_uint32),
                ("write_end_mark", ctypes.c_uint32), ("finish", ctypes.c_uint32),
                ("res", ctypes.c_int32), ("status", ctypes.c_int32),
                ("needs_init", ctypes.c_uint32), ("finished", ctypes.c_uint32),
                ("overflow", ctypes.c_uint32), ("off", ctypes.c_uint32),
                ("cyclic_pos", ctypes.c_uint32), ("longest_match_length", ctypes.c_uint32),
                ("num_pairs", ctypes.c_uint32), ("num_avail", ctypes.c_uint32),
                ("additional_offset", ctypes.c_uint32), ("reps", ctypes.c_uint32 * 4),
                ("state", ctypes.c_uint32), ("range", ctypes.c_uint32), ("cache", ctypes.c_uint32),
                ("cache_size", ctypes.c_uint32), ("_pad", ctypes.c_uint32),
                ("low", ctypes.c_uint64), ("out_total", ctypes.c_uint64)]


def pieces_of(name, n, seed=0):
    """Piece sizes that add up to n (the final call follows them with all n)."""
    if name == "ones":
        return [1] * n
    if name in ("p545", "p546", "p547"):
        p = int(name[1:])
        return [p] * (n // p) + ([n % p] if n % p else [])
    if name == "one":
        return [n]
    if name == "random":      # empty pieces, tiny ones, ones around the hold, large ones
        rng = random.Random(seed * 7919 + n)
        out, left = [], n
        while left:
            p = min(left, rng.choice((0, 0, 1, 2, rng.randrange(1, 40), rng.randrange(500, 600),
                                      rng.randrange(1, 5000), rng.randrange(1, 40000))))
            out.append(p)
            left -= p
        return out + [0]
    raise ValueError(name)


def is_mode0(want):
    return want["res"] in (C.OK, C.OUTPUT_EOF)


def mode0_cases(golden=None):
    """(case, data, want) of every golden and edge case the fast path encodes."""
    seen, out = set(), []
    for c in C.golden_cases() + C.edge_cases():
        if C.key(c) in seen:
            continue
        seen.add(C.key(c))
        data = C.data_of(c)
        want = C.expect(c, data, golden)
        if is_mode0(want):
            out.append((c, data, want))
    return out


def one_shot(c, data, cap, emu_one=None):
    """(res, dest_len, out) of the one-shot encoder for an input no golden holds."""
    if native.have_ref():
        res, dl, _, out, _, _ = C.ref_expect(dict(c, cap=cap), data)
        return res, dl, out
    res, dl, _, out = C.emu_encode(emu_one, data, c, cap)
    return res, dl, out


# ---------------------------------------------------------------- the emulator

def build_emu(out_dir, extra=(), main=False):
    out = os.path.join(str(out_dir), "lzmaenc_session_emu_main" if main else "liblzmaenc_session_emu.so")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", C.CSRC]
    cmd += (["-DLZMAENC_SESSION_EMU_MAIN"] if main else ["-fPIC", "-shared"])
    cmd += list(extra) if extra else ["-O2"]
    subprocess.run(cmd + [EMU_SRC, "-o", out], check=True)
    return out


def load_emu(so):
    lib = ctypes.CDLL(so)
    u64, u32, i32 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib.lzs_new.restype = ctypes.c_void_p
    lib.lzs_new.argtypes = [i32, u32, i32, i32, i32, i32, u32, i32, i32, i32, u64, u64, i32,
                            ctypes.c_char_p, ctypes.POINTER(i32)]
    lib.lzs_free.argtypes = [ctypes.c_void_p]
    lib.lzs_record.restype = ctypes.POINTER(Session)
    lib.lzs_record.argtypes = [ctypes.c_void_p]
    lib.lzs_dst.restype = ctypes.c_void_p
    lib.lzs_dst.argtypes = [ctypes.c_void_p]
    for f in (lib.lzs_slice_bytes, lib.lzs_slice_sum, lib.lzs_rounds_worked):
        f.restype = u64
        f.argtypes = [ctypes.c_void_p]
    lib.lzs_call.restype = i32
    lib.lzs_call.argtypes = [ctypes.c_void_p, ctypes.c_char_p, u64, i32, u64, u32, i32]
    lib.lzs_run.restype = i32
    lib.lzs_run.argtypes = [ctypes.c_void_p, ctypes.c_char_p, u64, ctypes.POINTER(u32), u32, u64,
                            u32, i32, ctypes.POINTER(i32), ctypes.POINTER(u64),
                            ctypes.POINTER(u64), ctypes.POINTER(u64)]
    lib.lzs_every_split.restype = ctypes.c_int64
    lib.lzs_every_split.argtypes = [ctypes.c_char_p, u64, i32, u32, i32, u32, ctypes.c_char_p, u64]
    return lib


def emu_new(lib, c, src_cap, dst_cap, poison=0x3C):
    """(handle or None, res, props5)"""
    props5 = ctypes.create_string_buffer(5)
    res = ctypes.c_int(0)
    h = lib.lzs_new(c["level"], c["dict"], c["lc"], c["lp"], c["pb"], c["fb"], c["mc"], c["algo"],
                    c["bt"], c["end_mark"], src_cap, dst_cap, poison, props5, ctypes.byref(res))
    return h, res.value, props5.raw


def emu_dst(lib, h, n):
    return ctypes.string_at(lib.lzs_dst(h), n) if n else b""


def emu_run(lib, data, c, cap, pieces, budget=0, hold=HOLD, poison=0x3C, fresh=0):
    """One stream through one emulated session by a piece schedule.  Returns
    dict(check, res, out_len, out, props5, calls, budget_calls); check is
    lzs_run's verdict on the published guarantees (0 = all held)."""
    h, res, props5 = emu_new(lib, c, len(data), cap, poison)
    assert h, (C.key(c), res)
    try:
        arr = (ctypes.c_uint32 * max(1, len(pieces)))(*pieces)
        r, ol, calls, bc = ctypes.c_int(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        check = lib.lzs_run(h, data, len(data), arr, len(pieces), budget, hold, fresh,
                            ctypes.byref(r), ctypes.byref(ol), ctypes.byref(calls), ctypes.byref(bc))
        return {"check": check, "res": r.value, "out_len": ol.value, "props5": props5,
                "out": emu_dst(lib, h, min(ol.value, cap)), "calls": calls.value,
                "budget_calls": bc.value}
    finally:
        lib.lzs_free(h)


def check_against(got, want, what):
    """emu_run's (or the GPU's) result against lzmaenc_cases.expect()'s dict."""
    assert got["check"] == 0, (what, got["check"])
    C.check((got["res"], got["out_len"], got["props5"], got["out"]), want, what)


def write_schedule_file(path, records):
    """records: (case, data, cap, pieces, budget, res, out) for the stand-alone
    build of the emulator."""
    with open(path, "wb") as f:
        for c, data, cap, pieces, budget, res, out in records:
            f.write(struct.pack("<iIiiiiIi", c["level"], c["dict"], c["lc"], c["lp"], c["pb"],
                                c["fb"], c["mc"], c["end_mark"]))
            f.write(struct.pack("<QQQIiQ", len(data), cap, budget, len(pieces), res, len(out)))
            f.write(struct.pack("<%dI" % len(pieces), *pieces))
            f.write(data + out)

"""Streams, cases and the composed expectation shared by the Lzma86 tests
(test_lzma86_gpu.py, test_lzma86_golden.py).

The expected bytes of an Lzma86 stream are composed on the spot from the
reference's own primitives -- ref_lzma_encode (oracle/_ref/libref_lzma.so) with
the capacity dst_cap - 14 and x86_Convert (oracle/_ref/libref.so) -- and the
choice rule of Lzma86_Encode (Lzma86Enc.c:59-104) written out in compose().
tests/golden/lzma86/ pins that composition against Lzma86Enc.c itself."""
import ctypes
import json
import os
import random
import struct

import native

GOLDEN_DIR = os.path.join(native.ROOT, "tests", "golden", "lzma86")
OK, UNSUPPORTED, PARAM, INPUT_EOF, OUTPUT_EOF = 0, 4, 5, 6, 7
NO, YES, AUTO = 0, 1, 2
HEADER = 14
_WORDS = ("the of and to in is that it was for on are as with his they at be this from have or by "
          "one had not but what all were when we there can an your which their said if do will "
          "each about how up out them then she many some so these would other into has more").split()


def have_refs():
    return native.have_ref() and os.path.exists(native.REF_CONT_SO)


# ---------------------------------------------------------------- the streams

def code(seed, n):
    """x86-like code: filler from a small alphabet without E8 / E9, and every
    9..16 bytes a CALL (E8 rel32) to one of six absolute targets, so the
    operand's top byte is 00 or FF.  Converted, the operands repeat: the filter
    must win."""
    rng = random.Random(seed)
    alphabet = bytes([0x55, 0x8B, 0xEC, 0x83, 0x45, 0x08, 0x89, 0x4D, 0xFC, 0x5D, 0xC3, 0x90, 0x33,
                      0xC0, 0x50, 0x51])
    targets = [rng.randrange(0, 3 * n + 64) for _ in range(6)]
    out = bytearray()
    while len(out) < n:
        out += bytes(rng.choice(alphabet) for _ in range(rng.randrange(4, 12)))
        rel = (rng.choice(targets) - (len(out) + 5)) & 0xFFFFFFFF
        out += b"\xE8" + struct.pack("<I", rel)
    return bytes(out[:n])


def text(seed, n):
    """Words: no E8, no E9.  Both candidates are the same bytes: the tie rule."""
    rng = random.Random(seed)
    return " ".join(rng.choices(_WORDS, k=n // 3 + 2)).encode()[:n]


def noise(seed, n):
    """Incompressible bytes without E8 / E9, salted every 24..40 bytes with the
    same five bytes E8 11 22 33 00.  As they stand the salts repeat; converted,
    each becomes another value: the filter must lose."""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes(b if b not in (0xE8, 0xE9) else 0x17
                     for b in rng.randbytes(rng.randrange(24, 41)))
        out += b"\xE8\x11\x22\x33\x00"
    return bytes(out[:n])


def tail(seed, n):
    """code() with an E8 among the last five bytes (x86_Convert stops before it)."""
    b = bytearray(code(seed, n))
    b[n - 3] = 0xE8
    return bytes(b)


GENERATORS = {"code": code, "text": text, "noise": noise, "tail": tail}
_data = {}


def data_of(kind, seed, n):
    k = (kind, seed, n)
    if k not in _data:
        _data[k] = GENERATORS[kind](seed, n) if n else b""
    return _data[k]


FIXED = ("code", 31, 6000)    # the filtered candidate is the smaller one
FIXED_U = ("noise", 33, 4000)  # the unfiltered one is


def stream_list():
    """(name, kind, seed, n): what every filter mode runs over."""
    out = [("code", ) + FIXED, ("text", "text", 32, 5000), ("noise", ) + FIXED_U]
    out += [("len%d" % n, "code", 34, n) for n in (0, 1, 4, 5, 6, 4097)]
    out.append(("tail", "tail", 35, 777))
    return out


def case(name, kind, seed, n, mode, cap=None, level=1, dict_size=0):
    return {"name": name, "kind": kind, "seed": seed, "n": n, "mode": mode, "cap": cap,
            "level": level, "dict": dict_size}


def ample(n):
    return HEADER + n + n // 2 + 1024


def mode_cases():
    return [case("%s/%d" % (name, mode), kind, seed, n, mode)
            for name, kind, seed, n in stream_list() for mode in (NO, YES, AUTO)]


def capacity_cases():
    """Capacities around the reference's two candidate sizes of the fixed streams
    (needs the live reference)."""
    out = []
    u, f = candidate_sizes(data_of(*FIXED), 1, 0)
    assert f < u, (u, f)
    for cap in (13, 14, HEADER + f - 1, HEADER + (f + u) // 2, None):
        out.append(case("cap/code/%s" % cap, *FIXED, AUTO, cap))
    u2, f2 = candidate_sizes(data_of(*FIXED_U), 1, 0)
    assert u2 < f2, (u2, f2)
    out.append(case("cap/noise/%d" % (HEADER + (u2 + f2) // 2), *FIXED_U, AUTO,
                    HEADER + (u2 + f2) // 2))
    return out


def cap_of(c):
    return ample(c["n"]) if c["cap"] is None else c["cap"]


def src_of(c):
    return data_of(c["kind"], c["seed"], c["n"])


# ---------------------------------------------------------------- the composed expectation

def ref_x86(data, encoding):
    """The reference's x86_Convert from ip 0 with a fresh state over the buffer."""
    lib = native.ref_cont()
    f = lib.ref_x86_convert
    f.restype = ctypes.c_size_t
    f.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint),
                  ctypes.c_int]
    buf = ctypes.create_string_buffer(bytes(data), max(len(data), 1))
    st = ctypes.c_uint(0)
    f(buf, len(data), 0, ctypes.byref(st), encoding)
    return buf.raw[:len(data)]


def ref_lzma(data, level, dict_size, room):
    """ref_lzma_encode into `room` bytes: (res, dest_len, props5, bytes)."""
    lib = native.ref()
    dst = ctypes.create_string_buffer(max(room, 1))
    dl = ctypes.c_size_t(room)
    props5 = ctypes.create_string_buffer(5)
    res = lib.ref_lzma_encode(dst, ctypes.byref(dl), data, len(data), level, dict_size, -1, -1, -1,
                              -1, 0, props5)
    return res, dl.value, props5.raw, dst.raw[:dl.value]


def candidate_sizes(data, level, dict_size):
    """(unfiltered, filtered) stream sizes with ample room."""
    room = len(data) + len(data) // 2 + 1024
    u = ref_lzma(data, level, dict_size, room)
    f = ref_lzma(ref_x86(data, 1), level, dict_size, room)
    assert u[0] == OK and f[0] == OK
    return u[1], f[1]


def compose(data, level, dict_size, mode, cap):
    """Lzma86_Encode's (res, destLen, the destLen bytes), from the primitives."""
    if cap < HEADER:
        return OUTPUT_EOF, 0, b""
    room = cap - HEADER
    u = ref_lzma(data, level, dict_size, room) if mode in (NO, AUTO) else None
    f = ref_lzma(ref_x86(data, 1), level, dict_size, room) if mode != NO else None
    props5 = (u or f)[2]
    u_ok, f_ok = u is not None and u[0] == OK, f is not None and f[0] == OK
    for c in (u, f):
        assert c is None or c[0] in (OK, OUTPUT_EOF), c[0]
    # the filtered candidate wins only when it fits and is strictly smaller; a
    # tie goes to the unfiltered one; a lone fitting candidate is taken
    if f_ok and (not u_ok or f[1] < u[1]):
        flag, best = 1, f
    elif u_ok:
        flag, best = 0, u
    else:
        flag, best = 0, None
    head = bytes([flag]) + props5 + struct.pack("<Q", len(data))
    if best is None:
        return OUTPUT_EOF, HEADER, head
    return OK, HEADER + best[1], head + best[3]


_want = {}


def expect(c):
    """compose() of a case, computed once and shared."""
    k = json.dumps(c, sort_keys=True)
    if k not in _want:
        _want[k] = compose(src_of(c), c["level"], c["dict"], c["mode"], cap_of(c))
    return _want[k]


# ---------------------------------------------------------------- goldens

def golden_cases():
    """The six inputs pinned against Lzma86Enc.c: code, text and salted noise,
    each under AUTO and YES."""
    return [case("%s_%s" % (name, "auto" if mode == AUTO else "yes"), kind, seed, n, mode)
            for name, kind, seed, n in stream_list()[:3] for mode in (AUTO, YES)]


def load_golden():
    with open(os.path.join(GOLDEN_DIR, "cases.json")) as f:
        rows = json.load(f)
    for r in rows:
        with open(os.path.join(GOLDEN_DIR, r["file"]), "rb") as f:
            r["bytes"] = f.read()
    return rows

"""What the PPMd7 encoder tests share: the supplementary fixtures
(tests/golden/ppmd7enc_cases.json + ppmd7enc_blob.bin, made by
tests/golden/make_golden_ppmd7enc.py from the reference's encoder, plain and
packed bytes both stored), the 15 streams of ppmd7_cases.json in one list, and
the host builds of csrc/ppmd7_device.h."""
import ctypes
import hashlib
import json
import os
import subprocess

import native
import ppmd7_golden as P

CSRC = os.path.join(native.ROOT, "lzma-sdk-zliblike_amd", "csrc")
ENC_SRC = os.path.join(native.ROOT, "tests", "emu_ppmd7", "ppmd7enc_emu.cpp")
DEC_SRC = os.path.join(native.ROOT, "tests", "emu_ppmd7", "ppmd7_emu.cpp")
OK, PARAM, OUTPUT_EOF = 0, 5, 7
POISON = 0xA5
_cache = {}


def load():
    if "d" not in _cache:
        with open(os.path.join(P.GOLD, "ppmd7enc_cases.json")) as f:
            d = json.load(f)
        with open(os.path.join(P.GOLD, d["blob"]), "rb") as f:
            d["_blob"] = f.read()
        assert hashlib.sha256(d["_blob"]).hexdigest() == d["blob_sha256"]
        _cache["d"] = d
    return _cache["d"]


def supplementary():
    """[(plain, packed, order, mem_size)] of the supplementary set."""
    d = load()
    b = d["_blob"]
    out = []
    for c in d["cases"]:
        plain = b[c["plain_off"]:c["plain_off"] + c["plain_len"]]
        assert P.sha(plain) == c["sha256"]
        out.append((plain, b[c["off"]:c["off"] + c["len"]], c["order"], c["mem_size"]))
    return out


def fixture_cases():
    """The 15 streams of ppmd7_cases.json: cases, then sevenz, then bench."""
    d = P.load()
    return d["cases"] + d["sevenz"] + d["bench"]


def build_emu(tmp, src=ENC_SRC, extra=("-O2",), main=None):
    """The host build of the encoder (or, with src=DEC_SRC, the decoder) in
    directory tmp: a shared library, or with main=<macro> a program."""
    out = os.path.join(str(tmp), os.path.basename(src)[:-4] + ("_main" if main else ".so"))
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-I", CSRC, src, "-o", out]
    cmd += ["-D" + main] if main else ["-fPIC", "-shared"]
    subprocess.run(cmd, check=True)
    return out


def load_enc(so):
    lib = ctypes.CDLL(so)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    lib.ppmd7_emu_encode.restype = ctypes.c_int
    lib.ppmd7_emu_encode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p,
                                     ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u64p, u64p,
                                     u64p]
    return lib


def load_dec(so):
    lib = ctypes.CDLL(so)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    lib.ppmd7_emu_decode.restype = ctypes.c_int
    lib.ppmd7_emu_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p,
                                     ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u64p, u64p]
    return lib


def emu_encode(lib, plain, order, mem, dst_cap):
    """(res, dest_len, packed_len, written bytes, [carries, pending 0xFF runs,
    carries through a run]); checks the poison behind the capacity."""
    tail = 32
    buf = ctypes.create_string_buffer(bytes([POISON]) * (dst_cap + tail), dst_cap + tail)
    dl, pl = ctypes.c_uint64(0), ctypes.c_uint64(0)
    cnt = (ctypes.c_uint64 * 3)()
    res = lib.ppmd7_emu_encode(plain, len(plain), buf, dst_cap, order, mem, ctypes.byref(dl),
                               ctypes.byref(pl), cnt)
    raw = buf.raw
    assert dl.value <= dst_cap
    assert raw[dl.value:] == bytes([POISON]) * (dst_cap + tail - dl.value)
    return res, dl.value, pl.value, raw[:dl.value], list(cnt)


def fixture_plain_cpu(dec, c):
    """A fixture's plain text: its packed bytes through the decoder's host build."""
    d = P.load()
    src = P.packed(d, c)
    dst = ctypes.create_string_buffer(max(c["plain_len"], 1))
    dl, sl = ctypes.c_uint64(0), ctypes.c_uint64(0)
    res = dec.ppmd7_emu_decode(src, len(src), dst, c["plain_len"], c["order"], c["mem_size"],
                               ctypes.byref(dl), ctypes.byref(sl))
    plain = dst.raw[:dl.value]
    assert (res, dl.value, sl.value) == (0, c["plain_len"], len(src))
    assert P.sha(plain) == c["sha256"]
    return plain

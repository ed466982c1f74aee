"""csrc/ppmd7_device.h on the host: the decoder the PPMd7 kernel runs, built with
g++ as lane 0 of 1 (tests/emu_ppmd7/ppmd7_emu.cpp), against every golden and
mutated case of tests/golden/ppmd7_cases.json (results recorded from the
reference's Ppmd7.c / Ppmd7Dec.c) and, where the reference library is built,
against 50 fresh random mutations decoded live by it (tests/ppmd7ref.py)."""
import ctypes
import os
import random
import struct
import subprocess

import pytest

import native
import ppmd7_golden as P

EMU_SRC = os.path.join(native.ROOT, "tests", "emu_ppmd7", "ppmd7_emu.cpp")
CSRC = os.path.join(native.ROOT, "lzma-sdk-zliblike_amd", "csrc")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ppmd7_emu") / "libppmd7_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", CSRC,
                    EMU_SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    f = lib.ppmd7_emu_decode
    f.restype = ctypes.c_int
    u64p = ctypes.POINTER(ctypes.c_uint64)
    f.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64,
                  ctypes.c_uint32, ctypes.c_uint32, u64p, u64p]
    return lib


def emu_decode(lib, packed, order, mem, dst_len):
    dst = ctypes.create_string_buffer(max(dst_len, 1))
    dl, sl = ctypes.c_uint64(0), ctypes.c_uint64(0)
    res = lib.ppmd7_emu_decode(packed, len(packed), dst, dst_len, order, mem, ctypes.byref(dl),
                               ctypes.byref(sl))
    return res, dl.value, sl.value, dst.raw[:dl.value]


def test_fixture_set_meets_its_conditions():
    d = P.load()
    assert d["coverage"]["Ppmd7.c"]["percent"] == 100.0
    assert d["coverage"]["Ppmd7Dec.c"]["percent"] == 100.0
    assert len(d["mutated"]) >= 200
    assert all(c["plain_len"] <= 200000 for c in d["cases"])
    assert all(d["cases"][m["base"]]["plain_len"] <= 30000 for m in d["mutated"])
    assert len(d["_blob"]) < (1 << 20)


def test_golden_cases(emu):
    d = P.load()
    for i, c in enumerate(d["cases"] + d["sevenz"] + d["bench"]):
        src = P.packed(d, c)
        res, dl, sl, out = emu_decode(emu, src, c["order"], c["mem_size"], c["plain_len"])
        assert (res, dl, sl) == (0, c["plain_len"], len(src)), (i, res, dl, sl)
        assert P.sha(out) == c["sha256"], i


def test_mutated_cases(emu):
    d = P.load()
    for i, m in enumerate(d["mutated"]):
        c = d["cases"][m["base"]]
        src, dst_len = P.mutated_input(d, m)
        res, dl, sl, out = emu_decode(emu, src, c["order"], c["mem_size"], dst_len)
        assert (res, dl, sl) == (m["res"], m["dest_len"], m["src_len"]), (i, m["ops"], res, dl, sl)
        assert P.sha(out) == m["sha256"], (i, m["ops"])


def test_parameter_checks_come_first(emu):
    for order, mem in ((1, 1 << 16), (65, 1 << 16), (6, (1 << 11) - 1), (6, 0xFFFFFFFF - 35)):
        assert emu_decode(emu, b"\1garbage", order, mem, 10) == (4, 0, 0, b"")
    assert emu_decode(emu, b"\0\0\0\0\0", 6, 1 << 16, 0) == (0, 0, 5, b"")
    assert emu_decode(emu, b"\0\0\0\0", 6, 1 << 16, 0)[:3] == (1, 0, 4)
    assert emu_decode(emu, b"\0\xff\xff\xff\xff", 6, 1 << 16, 3)[:3] == (1, 0, 5)
    assert emu_decode(emu, b"\5\0\0\0\0", 6, 1 << 16, 3)[:3] == (1, 0, 1)


@pytest.mark.skipif(not (native.have_ref() and os.path.exists(native.REF_CONT_SO)),
                    reason="reference library not built")
def test_fresh_mutations_against_the_live_reference(emu):
    import ppmd7ref
    d = P.load()
    rng = random.Random(int.from_bytes(os.urandom(8), "little"))
    small = [c for c in d["cases"] if c["plain_len"] <= 8192]
    for k in range(50):
        c = rng.choice(small)
        b = bytearray(P.packed(d, c))
        dst_len = c["plain_len"]
        for _ in range(rng.randrange(1, 4)):
            how = rng.randrange(5)
            if how == 0 and len(b) > 6:
                b[rng.randrange(1, len(b))] ^= 1 << rng.randrange(8)
            elif how == 1 and len(b) > 6:
                b[rng.randrange(1, len(b))] = rng.randrange(256)
            elif how == 2:
                del b[len(b) - rng.randrange(1, min(len(b), 64)):]
            elif how == 3:
                b += rng.randbytes(rng.randrange(1, 6))
            else:
                dst_len = rng.randrange(0, c["plain_len"] + 50)
        b = bytes(b)
        want = ppmd7ref.decode(b, c["order"], c["mem_size"], dst_len)
        got = emu_decode(emu, b, c["order"], c["mem_size"], dst_len)
        assert got == want, (k, c["order"], c["mem_size"], dst_len, b.hex(), got[:3], want[:3])


def write_case_file(path):
    """Every golden and mutated case as records for the stand-alone build of
    ppmd7_emu.cpp (-DPPMD7_EMU_MAIN; the sanitizer run): expected output bytes
    come from decoding with the library build, which the tests above pin."""
    d = P.load()
    so_dir = os.path.dirname(path)
    so = os.path.join(so_dir, "libppmd7_emu_dump.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, EMU_SRC, "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.ppmd7_emu_decode.restype = ctypes.c_int
    u64p = ctypes.POINTER(ctypes.c_uint64)
    lib.ppmd7_emu_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p,
                                     ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u64p, u64p]
    with open(path, "wb") as f:
        def rec(src, order, mem, dst_len, want):
            out = emu_decode(lib, src, order, mem, dst_len)
            assert out[:3] == want
            f.write(struct.pack("<IIQQiQQ", order, mem, len(src), dst_len, *want))
            f.write(src)
            f.write(out[3])
        for c in d["cases"]:
            rec(P.packed(d, c), c["order"], c["mem_size"], c["plain_len"],
                (0, c["plain_len"], c["len"]))
        for m in d["mutated"]:
            c = d["cases"][m["base"]]
            src, dst_len = P.mutated_input(d, m)
            rec(src, c["order"], c["mem_size"], dst_len, (m["res"], m["dest_len"], m["src_len"]))

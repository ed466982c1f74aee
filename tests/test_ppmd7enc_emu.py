"""csrc/ppmd7_device.h's encoder on the host: what ppmd7_encode_kernel runs,
built with g++ as lane 0 of 1 (tests/emu_ppmd7/ppmd7enc_emu.cpp), against the
reference encoder's own streams -- the 15 of tests/golden/ppmd7_cases.json
(their plain text recovered with the decoder's host build and checked by
sha256) and the 56 of ppmd7enc_cases.json.  Exact bytes and result triples,
every output capacity for two streams, the counters that show the carry and
pending-0xFF paths were taken, and a stand-alone sanitizer build over all of
it."""
import os
import struct
import subprocess

import pytest

import ppmd7enc_cases as C

OK, PARAM, OUTPUT_EOF = C.OK, C.PARAM, C.OUTPUT_EOF


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.load_enc(C.build_emu(tmp_path_factory.mktemp("ppmd7enc_emu")))


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    """[(plain, packed, order, mem_size)] of the 15 fixture streams."""
    dec = C.load_dec(C.build_emu(tmp_path_factory.mktemp("ppmd7_emu"), src=C.DEC_SRC))
    d = C.P.load()
    return [(C.fixture_plain_cpu(dec, c), C.P.packed(d, c), c["order"], c["mem_size"])
            for c in C.fixture_cases()]


def test_supplementary_set_meets_its_conditions():
    d = C.load()
    cases = d["cases"]
    assert len(cases) >= 48 and all(c["plain_len"] <= 4096 for c in cases)
    for r in (1, 2, 3):
        assert sum(c["mem_size"] & 3 == r for c in cases) >= 8
    assert {2049, 2050, 2051} <= {c["mem_size"] for c in cases}
    assert {2, 7, 32, 63, 64} <= {c["order"] for c in cases}
    assert {c["content"] for c in cases} >= {"empty", "one byte", "two equal bytes",
                                              "4096 equal bytes", "0..255 ascending twice",
                                              "random bytes", "word soup"}
    size =len(d["_blob"]) + os.path.getsize(os.path.join(C.P.GOLD, "ppmd7enc_cases.json"))
    assert size < 512 << 10


def test_fixture_streams_encode_exactly(emu, fixtures):
    assert len(fixtures) == 15
    for i, (plain, packed, order, mem) in enumerate(fixtures):
        res, dl, pl, out, _ = C.emu_encode(emu, plain, order, mem, len(packed))
        assert (res, dl, pl) == (OK, len(packed), len(packed)), (i, res, dl, pl)
        assert out == packed, i


def test_supplementary_streams_encode_exactly(emu):
    for i, (plain, packed, order, mem) in enumerate(C.supplementary()):
        res, dl, pl, out, _ = C.emu_encode(emu, plain, order, mem, len(packed) + 3)
        assert (res, dl, pl) == (OK, len(packed), len(packed)), (i, order, mem, res, dl, pl)
        assert out == packed, (i, order, mem)


@pytest.mark.parametrize("index", [8, 2])
def test_every_capacity(emu, fixtures, index):
    """Every dst_cap in 0..len+1: a cut anywhere, inside a pending 0xFF run
    included, leaves exactly the stream's prefix and the poison behind it
    (emu_encode checks the poison)."""
    plain, packed, order, mem = fixtures[index]
    n = len(packed)
    assert n == (352 if index == 8 else 4405)
    for cap in range(n + 2):
        res, dl, pl, out, _ = C.emu_encode(emu, plain, order, mem, cap)
        assert res == (OUTPUT_EOF if cap < n else OK), cap
        assert (dl, pl) == (min(cap, n), n), cap
        assert out == packed[:dl], cap


def test_carries_and_pending_runs_are_exercised(emu, fixtures):
    """The exact-bytes checks mean something only where the carry paths ran:
    every stream but the 352-byte one has a carry, a pending 0xFF run and a
    carry rippling through a run."""
    for i, (plain, packed, order, mem) in enumerate(fixtures):
        cnt = C.emu_encode(emu, plain, order, mem, len(packed))[4]
        assert cnt[0] >= 1, i
        if i != 8:
            assert cnt[1] >= 1 and cnt[2] >= 1, (i, cnt)
        if i == 2:  # the stream whose every capacity is tried: 18 runs, one rippling carry
            assert cnt[1:] == [18, 1]


def test_parameter_checks_come_first(emu):
    for order, mem in ((1, 1 << 16), (65, 1 << 16), (6, (1 << 11) - 1), (6, 0xFFFFFFFF - 35)):
        assert C.emu_encode(emu, b"garbage", order, mem, 10)[:4] == (PARAM, 0, 0, b"")


def test_empty_input_gives_the_five_flush_bytes(emu):
    assert C.emu_encode(emu, b"", 6, 1 << 16, 9)[:4] == (OK, 5, 5, b"\0" * 5)
    assert C.emu_encode(emu, b"", 64, 2049, 5)[:4] == (OK, 5, 5, b"\0" * 5)
    assert C.emu_encode(emu, b"", 2, 2048, 3)[:4] == (OUTPUT_EOF, 3, 5, b"\0" * 3)
    assert C.emu_encode(emu, b"", 2, 2048, 0)[:4] == (OUTPUT_EOF, 0, 5, b"")


def test_sanitizer_program_over_all_of_the_above(tmp_path, fixtures):
    """g++ -O1 -g -fsanitize=address,undefined, its own main, exact-size heap
    blocks for model, input and output: every fixture and supplementary stream,
    every capacity of streams 8 and 2, the bad parameters and the empty input."""
    exe = C.build_emu(tmp_path, extra=("-O1", "-g", "-fsanitize=address,undefined",
                                       "-fno-sanitize-recover=undefined"),
                      main="PPMD7ENC_EMU_MAIN")
    # the records are dealt over four case files, one child process each
    paths = [str(tmp_path / f"cases{k}.bin") for k in range(4)]
    files = [open(p, "wb") for p in paths]
    counts = [0] * len(files)

    def rec(plain, order, mem, cap, res, want):
        k = sum(counts) % len(files)
        files[k].write(struct.pack("<IIQQiQQ", order, mem, len(plain), cap, res,
                                   min(cap, len(want)), len(want)))
        files[k].write(plain)
        files[k].write(want[:cap])
        counts[k] += 1

    for plain, packed, order, mem in fixtures + C.supplementary():
        rec(plain, order, mem, len(packed), OK, packed)
    for index in (8, 2):
        plain, packed, order, mem = fixtures[index]
        for cap in range(len(packed) + 2):
            rec(plain, order, mem, cap, OUTPUT_EOF if cap < len(packed) else OK, packed)
    for order, mem in ((1, 1 << 16), (65, 1 << 16), (6, (1 << 11) - 1), (6, 0xFFFFFFFF - 35)):
        rec(b"garbage", order, mem, 10, PARAM, b"")
    rec(b"", 6, 1 << 16, 5, OK, b"\0" * 5)
    rec(b"", 6, 2051, 2, OUTPUT_EOF, b"\0" * 5)
    for f in files:
        f.close()
    assert sum(counts) == 15 + 56 + 354 + 4407 + 6
    runs = [subprocess.Popen([exe, p], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for p in paths]
    for k, r in enumerate(runs):
        out, err = r.communicate()
        assert r.returncode == 0, (out[-2000:], err[-4000:])
        assert "%d cases, 0 mismatches" % counts[k] in out

"""Encoder sessions on the host: LzmaEnc::session_call (csrc/lzmaenc_device.h)
on the public LzmaEncGpuSession record, driven round by round as the session
kernels drive it (tests/emu_lzmaenc_session/lzmaenc_session_emu.cpp, g++ -Wall
-Werror).  Whatever the piece sizes, the bytes, res and length are the one-shot
encoder's: the goldens, the live reference where it is built.  Nothing has a
tolerance.  The emulator itself checks the published guarantees after every call
(lzs_run's codes)."""
import ctypes
import subprocess

import pytest

import lzmaenc_cases as C
import lzmaenc_session_cases as S


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return S.load_emu(S.build_emu(tmp_path_factory.mktemp("lzmaenc_session_emu")))


@pytest.fixture(scope="module")
def emu_one(tmp_path_factory):
    return C.load_emu(C.build_emu(tmp_path_factory.mktemp("lzmaenc_one_emu")))


@pytest.fixture(scope="module")
def cases():
    return S.mode0_cases(C.load_golden())


# text; byte runs up to 700 (longer than the 273 a match can take); random bytes
# with copied spans under a 1 KiB dictionary, so that the ring wraps
SPLIT_INPUTS = (("text", 41, 2700, 0), ("runs", 42, 2900, 0), ("copy", 43, 2600, 1024))


def split_differences(emu, emu_one, kind, seed, n, dict_size, fb, hold):
    c = C.case(kind, seed, n, dict=dict_size, fb=fb)
    data = C.data_of(c)
    res, dl, out = S.one_shot(c, data, C.ample(n), emu_one)
    assert res == C.OK
    return emu.lzs_every_split(data, n, c["level"], dict_size, fb, hold, out, dl)


def test_record_layout():
    assert ctypes.sizeof(S.Session) == 200
    assert (S.Session.res.offset, S.Session.low.offset) == (104, 184)


@pytest.mark.parametrize("kind,seed,n,dict_size", SPLIT_INPUTS)
def test_every_split_into_two_calls(emu, emu_one, kind, seed, n, dict_size):
    """k bytes not final, then all bytes final, for every k in 0..n."""
    for fb in (5, 32, 273):
        assert split_differences(emu, emu_one, kind, seed, n, dict_size, fb, S.HOLD) == 0, fb


def test_every_split_notices_a_shortened_hold(emu, emu_one):
    """The same harness with the hold at 100 must see other bytes on the input
    with long runs: if it does not, the test above is not looking."""
    kind, seed, n, dict_size = SPLIT_INPUTS[1]
    for fb in (5, 32, 273):
        assert split_differences(emu, emu_one, kind, seed, n, dict_size, fb, 100) > 0, fb


@pytest.mark.parametrize("schedule", S.SCHEDULES)
def test_piece_schedules_over_the_mode0_cases(emu, cases, schedule):
    seen = set()
    for i, (c, data, want) in enumerate(cases):
        got = S.emu_run(emu, data, c, want["cap"], S.pieces_of(schedule, len(data), i))
        S.check_against(got, want, (schedule, C.key(c)))
        seen.add((want["res"], c["end_mark"], len(data) == 0, len(data) < S.HOLD,
                  0 < (c["dict"] or 1 << 16) < len(data)))
    # end mark on and off, the empty stream, streams shorter than the hold,
    # a dictionary smaller than the stream, overflow
    assert {s[0] for s in seen} == {C.OK, C.OUTPUT_EOF}
    assert {s[1] for s in seen} == {0, 1}
    assert {(s[1], s[2]) for s in seen} >= {(0, True), (1, True)}
    assert any(s[3] for s in seen) and any(s[4] for s in seen)


def test_a_stream_shorter_than_the_hold_waits_for_its_final_call(emu):
    c = C.case("text", 44, S.HOLD - 1)
    data = C.data_of(c)
    h, res, _ = S.emu_new(emu, c, len(data), 4096)
    assert h and res == C.OK
    try:
        rec = emu.lzs_record(h).contents
        poisoned = emu.lzs_slice_sum(h)
        for k in range(0, len(data) + 1, 7):
            assert emu.lzs_call(h, data, k, 0, 0, S.HOLD, 0) == 0
            assert (rec.in_pos, rec.out_pos, rec.status, rec.needs_init) == (0, 0, S.NEEDS_INPUT, 1)
        assert emu.lzs_slice_sum(h) == poisoned and emu.lzs_rounds_worked(h) == 0
        assert emu.lzs_call(h, data, len(data), 1, 0, S.HOLD, 0) == 1
        assert (rec.status, rec.res, rec.in_pos) == (S.FINISHED, C.OK, len(data))
    finally:
        emu.lzs_free(h)


@pytest.mark.parametrize("budget", (1, 40000))
def test_budget(emu, emu_one, budget):
    """The call ends at the first 32 KiB progress step at or after the budget;
    lzs_run checks each BUDGET call's advance (at least the budget, below
    budget + 32 KiB + 273).  The statuses walk BUDGET .. FINISHED."""
    c = C.case("text", 45, 100000)
    data = C.data_of(c)
    res, dl, out = S.one_shot(c, data, C.ample(len(data)), emu_one)
    assert res == C.OK
    for pieces in ([], [50000], S.pieces_of("p547", len(data))):
        got = S.emu_run(emu, data, c, C.ample(len(data)), pieces, budget=budget)
        assert (got["check"], got["res"], got["out_len"]) == (0, C.OK, dl), pieces[:3]
        assert got["out"] == out
        if not pieces:
            # one final call after the other: about n / 32 KiB of them with a
            # budget of 1, n / (40,000 rounded up to 64 KiB) with 40,000
            assert got["budget_calls"] == (3 if budget == 1 else 1), got
            assert got["calls"] == got["budget_calls"] + 1


def test_overflow(emu, emu_one):
    """SZ_ERROR_OUTPUT_EOF, out_pos == dst_cap, dst the first dst_cap bytes of
    the full stream; lzs_run checks that calls after the end change nothing."""
    for c in (C.case("text", 46, 30000), C.case("copy", 47, 5000, end_mark=1)):
        data = C.data_of(c)
        res, full, out = S.one_shot(c, data, C.ample(len(data)), emu_one)
        assert res == C.OK
        for cap in (0, 4, 5, full - 1, full):
            for schedule in ("p547", "random", "one"):
                got = S.emu_run(emu, data, c, cap, S.pieces_of(schedule, len(data), cap))
                want = (C.OK, full) if cap == full else (C.OUTPUT_EOF, cap)
                assert (got["check"], got["res"], got["out_len"]) == (0,) + want, (cap, schedule)
                assert got["out"] == out[:cap]


def test_workspace_and_record_poison_do_not_reach_the_output(emu, cases):
    for i, (c, data, want) in enumerate(cases[::3]):
        pieces = S.pieces_of("random", len(data), i)
        a = S.emu_run(emu, data, c, want["cap"], pieces, poison=0x3C)
        b = S.emu_run(emu, data, c, want["cap"], pieces, poison=0xA5)
        assert a == b, C.key(c)
        S.check_against(a, want, C.key(c))


def test_refused_at_init(emu):
    for kw, want in ((dict(level=5), C.UNSUPPORTED), (dict(algo=1), C.UNSUPPORTED),
                     (dict(bt=1), C.UNSUPPORTED), (dict(lc=9), C.PARAM),
                     (dict(dict=(1 << 30) + 1), C.PARAM)):
        h, res, _ = S.emu_new(emu, C.case("text", 1, 100, **kw), 100, 100)
        assert (h, res) == (None, want), kw
    h, res, _ = S.emu_new(emu, C.case("text", 1, 100), 1 << 31, 100)
    assert (h, res) == (None, C.UNSUPPORTED)


def test_a_record_the_encoder_did_not_save_is_refused(emu):
    """What indexes memory is checked on the way in: a tampered record ends the
    session with SZ_ERROR_PARAM before anything is read through it."""
    c = C.case("text", 48, 5000)
    data = C.data_of(c)
    for field, value in (("off", 4000), ("cyclic_pos", 1 << 20), ("state", 12),
                         ("additional_offset", 2), ("src_len", 6000)):
        h, _, _ = S.emu_new(emu, c, len(data), 8192)
        try:
            rec = emu.lzs_record(h).contents
            assert emu.lzs_call(h, data, 2000, 0, 0, S.HOLD, 0) == 1 and rec.in_pos > 0
            if field != "src_len":
                setattr(rec, field, value)
            emu.lzs_call(h, data, 6000 if field == "src_len" else 3000, 0, 0, S.HOLD, 0)
            assert (rec.finished, rec.res, rec.status) == (1, C.PARAM, S.FINISHED), field
        finally:
            emu.lzs_free(h)


def test_sanitizer_program_over_the_schedules(tmp_path, emu, cases):
    """g++ -O1 -fsanitize=address,undefined, own main, run as a child process:
    exact-size heap blocks for the slice, for dst and, for every call, a fresh
    copy of exactly the supplied prefix of the source, so a read past src_len is
    the sanitizer's to report.  Every record twice with two poison bytes."""
    exe = S.build_emu(tmp_path, extra=("-O1", "-g", "-fsanitize=address,undefined",
                                       "-fno-sanitize-recover=undefined"), main=True)
    records = []
    for i, (c, data, want) in enumerate(cases):
        # 1-byte pieces copy the prefix once per byte: short streams only
        names = [s for s in S.SCHEDULES if s != "ones" or len(data) <= 3000]
        name = names[i % len(names)]
        pieces = S.pieces_of(name, len(data), i)
        got = S.emu_run(emu, data, c, want["cap"], pieces)
        S.check_against(got, want, (name, C.key(c)))
        records.append((c, data, want["cap"], pieces, 0, got["res"], got["out"]))
    c = C.case("text", 45, 100000)
    data = C.data_of(c)
    got = S.emu_run(emu, data, c, C.ample(len(data)), [70000], budget=1)
    assert got["check"] == 0 and got["res"] == C.OK
    records.append((c, data, C.ample(len(data)), [70000], 1, got["res"], got["out"]))
    path = str(tmp_path / "schedules.bin")
    S.write_schedule_file(path, records)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "%d records, 0 mismatches" % len(records) in r.stdout

"""The encoders of csrc/lzmaenc_device.h and csrc/lzma2enc_device.h on the host
at dictionaries above 64 KiB (tests/lzmaenc_bigdict_cases.py): a hash mask wider
than 0xFFFF, matches farther than 64 KiB, a ring that wraps beyond 64 KiB, the
levels' own dictionaries.  Every stream against the reference's single-threaded
LzmaEncode / Lzma2Enc_Encode: live (oracle/_ref/libref_lzma.so) where it is
built, and the committed goldens (tests/golden/lzmaenc_bigdict_cases.json)
everywhere.  Nothing has a tolerance.

test_mutants_are_noticed is the test of these tests: two builds of the emulator
from a deliberately wrong copy of the header (a hash mask stuck at 0xFFFF; a
flipped direct bit above the tenth) must give other bytes on the cases that were
chosen for them."""
import os
import subprocess

import pytest

import lzma2enc_cases as C2
import lzma2enc_opt_cases as O2
import lzmaenc_bigdict_cases as B
import lzmaenc_opt_cases as O
import lzmaenc_session_cases as S
import native

SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return O.load_emu(O.build_emu(tmp_path_factory.mktemp("lzmaenc_bigdict_emu")))


@pytest.fixture(scope="module")
def emu2(tmp_path_factory):
    return O2.load_emu(O2.build_emu(tmp_path_factory.mktemp("lzma2enc_bigdict_emu")))


@pytest.fixture(scope="module")
def emu_session(tmp_path_factory):
    return S.load_emu(S.build_emu(tmp_path_factory.mktemp("lzmaenc_bigdict_session_emu")))


@pytest.fixture(scope="module")
def golden():
    return B.load_golden()


def test_golden_file_is_what_the_generators_cover(golden):
    assert os.path.getsize(B.GOLDEN) < (1 << 19)
    assert [B.key(g["case"]) for g in golden["cases"]] == [B.key(c) for c in B.golden_cases()]
    assert [C2.key(g["case"]) for g in golden["lzma2"]] == [C2.key(c) for c in B.lzma2_cases()]
    assert "out" not in golden["cases"][0] and "out" not in golden["lzma2"][0]
    rnd = golden["cases"][len(B.named_cases()):]
    assert len(rnd) == 60 and {g["case"]["dict"] for g in rnd} == set(B.DICTS)
    assert {(g["norm"]["algo"], g["norm"]["btMode"]) for g in rnd} == {(0, 0), (1, 1), (1, 0), (0, 1)}
    for g in rnd:
        assert g["case"]["n"] <= (90000 if g["norm"]["algo"] == g["norm"]["btMode"] == 0 else 30000)
    # every dictionary here is above 64 KiB, F_ctl's excepted
    by_name = {(name, mode): golden["by_key"][B.key(c)] for name, mode, c in B.named_cases()}
    assert all((g["norm"]["dictSize"] > 1 << 16) == (g["case"]["dict"] != 1 << 16)
               for g in golden["cases"])
    assert sum(g["case"]["dict"] == 1 << 16 for g in golden["cases"]) == len(B.MODES)
    # the levels' own dictionaries
    assert [by_name["D%d" % k, "opt_bt4" if k == 5 else "fast"]["norm"]["dictSize"]
            for k in (2, 3, 4, 5)] == [1 << 18, 1 << 20, 1 << 22, 1 << 24]


def test_the_far_matches_are_there(golden):
    """F and X against their controls in the reference itself: with the block
    out of the dictionary's reach the stream is about 1 KiB longer."""
    for name, ctl, modes in (("F", "F_ctl", B.MODES), ("X", "X_ctl", ("fast",))):
        for mode in modes:
            a = B.expect(B.named(name, mode), golden)
            b = B.expect(B.named(ctl, mode), golden)
            assert a["res"] == b["res"] == O.OK and a["sha256"] != b["sha256"]
            assert b["dest_len"] - a["dest_len"] > 1000, (name, mode)
    data = B.data_of(B.named("F"))
    assert data[:1024] == data[67024:68048] and data[100:900] == data[68560:69360]
    data = B.data_of(B.named("X"))
    assert data[:1024] == data[1051024:1052048]


def run_case(emu, c, golden):
    """The case through the one-shot emulator with two workspace poisons,
    against the golden and, where it is built, the live reference."""
    data = B.data_of(c)
    want = O.golden_want(golden["by_key"][B.key(c)])
    got = O.emu_encode(emu, data, c, want["cap"], 0x3C)
    B.check(got, want, B.key(c))
    assert O.emu_encode(emu, data, c, want["cap"], 0xA5) == got, B.key(c)
    if native.have_ref():
        live = B.expect(c)
        assert live["out"] is not None and live["cap"] == want["cap"]
        B.check(got, live, B.key(c))


def test_named_cases(emu, golden):
    seen = set()
    for name, mode, c in B.named_cases():
        assert O.mode_of(c) == {"opt_bt4": 3, "opt_hc4": 1, "fast_bt4": 2, "fast": 0}[mode], name
        run_case(emu, c, golden)
        seen.add(name)
    assert seen == {"F", "F_ctl", "M", "M24", "C80", "W", "X", "X_ctl", "D2", "D3", "D4", "D5"}
    # the issue's orientation figures, in the order opt_bt4, fast_bt4, opt_hc4, fast
    for name, lens in (("F", (69153, 69190, 69153, 69190)), ("M", (6749, 6875, 6835, 7005)),
                       ("M24", (6749, 6875, 6835, 7005)), ("C80", (12236, 12251, 12541, 12591))):
        assert tuple(golden["by_key"][B.key(B.named(name, m))]["dest_len"] for m in B.MODES) == lens
    assert [golden["by_key"][B.key(B.named(n))]["dest_len"] for n in ("W", "X", "X_ctl")] == [
        20831, 1114148, 1115173]


def test_random_cases(emu, golden):
    for c in B.random_cases():
        run_case(emu, c, golden)


def test_lzma2_blocks(emu2, golden):
    for c in B.lzma2_cases():
        data = C2.data_of(c)
        want = dict(golden["lzma2_by_key"][C2.key(c)], out=None)
        cap = C2.block_bound(len(data))
        got = O2.emu_encode(emu2, data, c, cap, 0x3C)
        C2.check_block(got, want, C2.key(c))
        assert O2.emu_encode(emu2, data, c, cap, 0xA5) == got, C2.key(c)
        assert C2.decode_raw(got[3] + b"\0", got[2]) == data
        if native.have_ref():
            C2.check_block(got, C2.expect(c, data), C2.key(c))
    # an LZMA2 block and the LZMA stream of the same name see the same bytes
    assert C2.data_of(B.lzma2_case("F", 1)) == B.data_of(B.named("F"))
    assert C2.data_of(B.lzma2_case("M", 1)) == B.data_of(B.named("M"))


@pytest.mark.parametrize("name", B.SESSION_NAMES)
def test_sessions(emu_session, golden, name):
    c = B.named(name)
    data = B.data_of(c)
    want = B.expect(c, golden)
    for i, schedule in enumerate(B.SESSION_SCHEDULES):
        got = S.emu_run(emu_session, data, c, want["cap"], B.pieces_of(schedule, len(data), i))
        S.check_against(got, want, (name, schedule))


def test_mutants_are_noticed(tmp_path, emu, golden):
    narrow = B.build_mutant(tmp_path / "narrow", B.MUTANT_NARROW_MASK)
    flipped = B.build_mutant(tmp_path / "flipped", B.MUTANT_DIRECT_BIT_10)

    def want(name, mode="fast"):
        c = B.named(name, mode)
        w = B.expect(c, golden)
        assert not B.differs(emu, c, w)         # the unchanged build is right
        return c, w
    for mode in B.MODES:
        assert B.differs(narrow, *want("M", mode)), mode
        assert B.differs(flipped, *want("F", mode)), mode
        assert B.differs(flipped, *want("C80", mode)), mode
    assert B.differs(narrow, *want("W"))
    assert B.differs(flipped, *want("X"))
    # and each mutant is otherwise the same encoder: at most ten direct bits,
    # a mask that is 0xFFFF anyway
    assert not B.differs(narrow, *want("F_ctl"))
    assert not B.differs(flipped, *want("F_ctl"))


def test_sanitizer_program_over_the_named_cases(tmp_path, golden):
    """g++ -O1 -fsanitize=address,undefined, own main, run as a child process,
    exact-size malloc'ed source and destination, poisoned exact-size workspace;
    every record twice with two poison bytes."""
    exe = O.build_emu(tmp_path, extra=SANITIZE, main=True)
    cases = [B.named(name, mode) for name in ("F", "M", "M24", "C80") for mode in B.MODES]
    cases.append(B.named("W"))
    path = str(tmp_path / "cases.bin")
    O.write_case_file(path, cases, golden)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "%d cases, 0 mismatches" % len(cases) in r.stdout

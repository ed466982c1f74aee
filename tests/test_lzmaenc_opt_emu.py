"""The normal-mode encoder of csrc/lzmaenc_device.h and csrc/lzma2enc_device.h
on the host (the optimal parser GetOptimum / Backward with its price tables, and
the Bt4 finder), built with g++ -Wall -Werror (tests/emu_lzmaenc_opt/), against
the reference's single-threaded LzmaEncode and Lzma2Enc_Encode at levels 5..9:
live (oracle/_ref/libref_lzma.so) over the edge lists and 2,000 seeded random
cases, and over the committed goldens (tests/golden/lzmaenc_opt_cases.json)
everywhere.  Output bytes, res, dest_len and the props bytes are compared;
nothing has a tolerance.  Every case runs twice with two workspace poison bytes:
a cell of `opt`, of a price table, of `son` or of `matches` that is read before
this call wrote it would make the two outputs differ.  Stand-alone sanitizer
builds run every golden and edge case as a child process."""
import os
import subprocess

import pytest

import lzma2enc_cases as C2
import lzma2enc_opt_cases as O2
import lzmaenc_opt_cases as O
import native

needs_ref = pytest.mark.skipif(not native.have_ref(), reason="reference library not built")
SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return O.load_emu(O.build_emu(tmp_path_factory.mktemp("lzmaenc_opt_emu")))


@pytest.fixture(scope="module")
def emu2(tmp_path_factory):
    return O2.load_emu(O2.build_emu(tmp_path_factory.mktemp("lzma2enc_opt_emu")))


@pytest.fixture(scope="module")
def golden():
    return O.load_golden()


def run_case(emu, c, want, data=None):
    data = O.data_of(c) if data is None else data
    got = O.emu_encode(emu, data, c, want["cap"], 0x3C)
    O.check(got, want, O.key(c))
    assert O.emu_encode(emu, data, c, want["cap"], 0xA5) == got, O.key(c)
    return got


def run_block(emu2, c, want, data=None):
    data = O2.data_of(c) if data is None else data
    cap = O2.block_bound(len(data))
    got = O2.emu_encode(emu2, data, c, cap, 0x3C)
    O2.check_block(got, want, O2.key(c))
    assert O2.emu_encode(emu2, data, c, cap, 0xA5) == got, O2.key(c)
    if got[0] == C2.OK:
        assert C2.decode_raw(got[3] + b"\0", got[2]) == data, O2.key(c)
    return got


def test_golden_file_is_what_the_generators_cover(golden):
    assert os.path.getsize(O.GOLDEN) < (1 << 19)
    assert [O.key(g["case"]) for g in golden["cases"]] == [O.key(c) for c in O.golden_cases()]
    assert [O2.key(g["case"]) for g in golden["lzma2"]] == [O2.key(c) for c in O2.golden_cases()]
    assert {g["res"] for g in golden["cases"]} == {O.OK, O.UNSUPPORTED, O.PARAM, O.OUTPUT_EOF}
    assert {g["case"]["mc"] for g in golden["cases"]} >= {0, 1, 4, 48}
    # all four combinations of the two mode bits, and levels 5..9
    assert {(g["norm"]["algo"], g["norm"]["btMode"]) for g in golden["cases"]} == {
        (1, 1), (1, 0), (0, 1)}
    assert {g["norm"]["level"] for g in golden["cases"]} >= {5, 6, 7, 8, 9}
    assert "out" not in golden["cases"][0] and "out" not in golden["lzma2"][0]


def test_golden_cases(emu, golden):
    for g in golden["cases"]:
        run_case(emu, g["case"], O.golden_want(g))


def test_lzma2_golden_cases(emu2, golden):
    for g in golden["lzma2"]:
        run_block(emu2, g["case"], dict(g, out=None))


def test_the_mixed_pieces_restore_state_in_front_of_rebuilt_prices(golden):
    """random 70 KiB + text 30 KiB: a stored chunk, then the restore, then a
    compressed chunk that sets state and props (0xC0); the long text: two full
    compressed chunks and a rest.  Saving cells, reps and state suffices because
    LzmaEnc_CodeOneMemBlock rebuilds every price table at each chunk's start:
    test_lzma2_golden_cases compares these bytes."""
    mixed = golden["lzma2_by_key"][O2.key(O2.MIXED_CASE)]["chunks"]
    assert [t[0] for t in mixed] == [1, 0xC0, 0] and mixed[0][1] + mixed[1][1] == 100 * 1024
    two = golden["lzma2_by_key"][O2.key(O2.TWO_CHUNK_CASE)]["chunks"]
    assert [t[0] for t in two] == [0xE0, 0x80, 0x80, 0] and sum(t[1] for t in two) == 400000


@needs_ref
def test_goldens_are_the_live_reference(golden):
    for g in golden["cases"]:
        res, dl, props5, out, cap, _ = O.ref_expect(g["case"])
        assert (res, dl, cap, O.sha(out), out[:32].hex()) == (
            g["res"], g["dest_len"], g["cap"], g["sha256"], g["head"]), O.key(g["case"])
        if res not in (O.PARAM, O.UNSUPPORTED):
            assert props5.hex() == g["props5"]
    for g in golden["lzma2"]:
        res, prop, out = C2.ref_stream(g["case"])
        assert C2.record(g["case"], res, prop, out) == g, O2.key(g["case"])


@needs_ref
def test_edge_cases_against_the_live_reference(emu, emu2):
    for c in O.edge_cases():
        run_case(emu, c, O.expect(c))
    for c in O2.edge_cases():
        run_block(emu2, c, O2.expect(c))


@needs_ref
@pytest.mark.parametrize("part", range(4))
def test_random_cases_against_the_live_reference(emu, part):
    cases = O.random_cases(500, 7100 + part)
    assert len(cases) * 4 >= 2000
    seen, modes = set(), set()
    for c in cases:
        want = O.expect(c)
        run_case(emu, c, want)
        seen.add(want["res"])
        modes.add(O.mode_of(c))
    assert seen >= {O.OK, O.OUTPUT_EOF} and modes == {1, 2, 3}


@needs_ref
def test_lzma2_random_cases_against_the_live_reference(emu2):
    for c in O2.random_cases(150, 7200, 200 * 1024):
        run_block(emu2, c, O2.expect(c))


def test_modes_are_refused_unless_allowed(emu, emu2):
    data = O.C.gen("text", 1, 100)
    refused = (O.UNSUPPORTED, 0, b"\0" * 5, b"")
    l5, bt4, opt_hc = O.case("text", 1, 100), O.case("text", 1, 100, level=1, bt=1), \
        O.case("text", 1, 100, bt=0)
    for allowed in (0, 1, 2):
        assert O.emu_encode(emu, data, l5, 200, allowed=allowed) == refused
    assert O.emu_encode(emu, data, bt4, 200, allowed=1) == refused
    assert O.emu_encode(emu, data, bt4, 200, allowed=2)[0] == O.OK
    assert O.emu_encode(emu, data, opt_hc, 200, allowed=2) == refused
    assert O.emu_encode(emu, data, opt_hc, 200, allowed=1)[0] == O.OK
    # Bt2 / Bt3 whatever the mask; numHashBytes above 4 is Bt4; the props checks come first
    for nhb in (0, 2, 3):
        assert O.emu_encode(emu, data, O.case("text", 1, 100, nhb=nhb), 200) == refused
    assert O.emu_encode(emu, data, O.case("text", 1, 100, nhb=5), 200) == \
        O.emu_encode(emu, data, l5, 200)
    assert O.emu_encode(emu, data, O.case("text", 1, 100, lc=9, nhb=3), 200, allowed=0) == (
        O.PARAM, 0, b"\0" * 5, b"")
    # a level-1 case with everything allowed is still the fast path
    c = O.case("text", 1, 100, level=1)
    assert O.mode_of(c) == 0 and O.emu_encode(emu, data, c, 200)[0] == O.OK
    # LZMA2: level 5 with the mask at 0 stays unsupported, lc + lp > 4 comes first
    c2 = O2.case([("text", 1, 100)], level=5)
    assert O2.emu_encode(emu2, data, c2, 200, allowed=0)[:2] == (C2.UNSUPPORTED, 0)
    assert O2.emu_encode(emu2, data, c2, 200, allowed=3)[0] == C2.OK
    assert O2.emu_encode(emu2, data, dict(c2, lc=4, lp=1), 200, allowed=3)[0] == C2.PARAM


def test_prob_prices(emu):
    """LzmaEnc_InitPriceTables: -log2(p) in sixteenths of a bit, by squaring."""
    p = [emu.lzmaenc_opt_emu_prob_price(i) for i in range(128)]
    # entry 0 is exact (8 / 2048 = 2^-8: 8 bits); the rest round -log2 up by
    # less than one sixteenth of a bit (the -15 in the reference's formula)
    assert p[0] == 128 and all(a >= b for a, b in zip(p, p[1:]))
    import math
    for i, v in enumerate(p):
        assert 0 <= v - 16 * -math.log2((i * 16 + 8) / 2048) < 1.0, i
    if native.have_ref():
        import ctypes
        t = (ctypes.c_uint32 * 128)()
        native.ref().LzmaEnc_InitPriceTables(t)
        assert list(t) == p


def test_slice_layout(emu, emu2):
    """What each mode adds to the fast path's slice: Bt4 doubles `son`; the
    optimal parser adds the price tables and the 4,096 opt cells."""
    f = emu.lzmaenc_opt_emu_slice_bytes
    fixed, cells = 1024 + 65536, 1846 + (0x300 << 3)

    def want(dict_size, src_len, mask, pb, algo, bt, cells=cells):
        raw = ((cells * 2 + 15) & ~15) + 552 * 4 + (fixed + mask + 1) * 4 + \
            ((min(dict_size, src_len) + 1) << bt) * 4
        if algo:
            raw = ((raw + 15) & ~15) + ((2 << pb) * 272 + 32 + 256 + 512 + 16 + 128) * 4 + 4096 * 48
        return (raw + 255) & ~255
    for dict_size, src_len, mask in ((4096, 100, 0xFFFF), (4096, 1 << 20, 0xFFFF),
                                     (5000, 5001, 0xFFFF), (1 << 24, 10, 0x7FFFFF)):
        for pb in (0, 2, 4):
            for algo in (0, 1):
                for bt in (0, 1):
                    assert f(dict_size, 3, 0, pb, algo, bt, src_len) == \
                        want(dict_size, src_len, mask, pb, algo, bt), (dict_size, pb, algo, bt)
    # mode 0 is the fast path's slice whatever pb is
    assert f(4096, 3, 0, 4, 0, 0, 100) == f(4096, 3, 0, 0, 0, 0, 100)
    # the optimal parser's additions: 192 KiB of opt, at most 38 KiB of prices
    add = f(4096, 3, 0, 4, 1, 0, 100) - f(4096, 3, 0, 4, 0, 0, 100)
    assert 192 * 1024 + 34 * 1024 < add <= 192 * 1024 + 39 * 1024
    import ctypes
    out2 = (ctypes.c_uint64 * 2)()
    emu2.lzma2enc_opt_emu_slice_bytes(4096, 3, 0, 2, 1, 1, 9000, out2)
    assert out2[0] == f(4096, 3, 0, 2, 1, 1, 9000)
    assert out2[1] == (out2[0] + ((cells * 2 + 15) & ~15) + 255) & ~255


def test_sanitizer_program_over_golden_and_edge_cases(tmp_path, golden):
    """g++ -O1 -fsanitize=address,undefined, own main, exact-size malloc'ed
    source and destination, poisoned exact-size workspace; every record twice
    with two poison bytes."""
    exe = O.build_emu(tmp_path, extra=SANITIZE, main=True)
    cases = {O.key(c): c for c in O.golden_cases() + O.edge_cases()}
    path = str(tmp_path / "cases.bin")
    O.write_case_file(path, list(cases.values()), golden)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "%d cases, 0 mismatches" % len(cases) in r.stdout


def test_lzma2_sanitizer_program_over_golden_and_edge_cases(tmp_path, golden):
    exe = O2.build_emu(tmp_path, extra=SANITIZE, main=True)
    cases = {O2.key(c): c for c in O2.golden_cases() + O2.edge_cases()}
    path = str(tmp_path / "cases2.bin")
    O2.write_case_file(path, list(cases.values()), golden)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "%d cases, 0 mismatches" % len(cases) in r.stdout

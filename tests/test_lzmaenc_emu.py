"""csrc/lzmaenc_device.h on the host: the encoder the LZMA encode kernel runs,
built with g++ -Wall -Werror (tests/emu_lzmaenc/lzmaenc_emu.cpp), against the
reference's LzmaEncode -- live (oracle/_ref/libref_lzma.so) over the edge list
and 2,000 seeded random cases, and over the committed goldens
(tests/golden/lzmaenc_cases.json) everywhere.  Output bytes, res, dest_len and
the 5 props bytes are compared; nothing has a tolerance.  A stand-alone
sanitizer build of the emulator runs every golden and edge case as a child
process, each with two workspace poison bytes."""
import os
import subprocess

import pytest

import lzmaenc_cases as C
import native

needs_ref = pytest.mark.skipif(not native.have_ref(), reason="reference library not built")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.load_emu(C.build_emu(tmp_path_factory.mktemp("lzmaenc_emu")))


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


def run_case(emu, c, want, data=None):
    data = C.data_of(c) if data is None else data
    got = C.emu_encode(emu, data, c, want["cap"], 0x3C)
    C.check(got, want, C.key(c))
    # a second workspace poison: no entry of `son` or `matches` is read before
    # it is written, or the two outputs would differ
    assert C.emu_encode(emu, data, c, want["cap"], 0xA5) == got, C.key(c)
    return got


def golden_want(g):
    return {"res": g["res"], "dest_len": g["dest_len"], "props5": bytes.fromhex(g["props5"]),
            "cap": g["cap"], "sha256": g["sha256"], "head": bytes.fromhex(g["head"]), "out": None}


def test_golden_file_is_what_the_generator_covers(golden):
    assert os.path.getsize(C.GOLDEN) < (1 << 19)
    assert [C.key(g["case"]) for g in golden["cases"]] == [C.key(c) for c in C.golden_cases()]
    assert {g["case"]["mc"] for g in golden["cases"]} >= {0, 1, 4, 48}
    assert {g["res"] for g in golden["cases"]} == {C.OK, C.UNSUPPORTED, C.PARAM, C.OUTPUT_EOF}


def test_golden_cases(emu, golden):
    for g in golden["cases"]:
        run_case(emu, g["case"], golden_want(g))


@needs_ref
def test_goldens_are_the_live_reference(golden):
    for g in golden["cases"]:
        res, dl, props5, out, cap, _ = C.ref_expect(g["case"])
        assert (res, dl, cap, C.sha(out), out[:32].hex()) == (
            g["res"], g["dest_len"], g["cap"], g["sha256"], g["head"]), C.key(g["case"])
        if res not in (C.PARAM, C.UNSUPPORTED):
            assert props5.hex() == g["props5"]


@needs_ref
def test_edge_cases_against_the_live_reference(emu):
    for c in C.edge_cases():
        run_case(emu, c, C.expect(c))


@needs_ref
def test_overflow_is_a_prefix_of_the_full_stream(emu):
    """The reading of MyWrite this encoder relies on, confirmed on the live
    reference: SZ_ERROR_OUTPUT_EOF, dest_len == cap, dst = the first cap bytes."""
    for c in (C.case("random", 31, 70 * 1024, dict=1 << 16), C.case("text", 32, 30000),
              C.case("text", 33, 0, end_mark=1)):
        data = C.data_of(c)
        full = C.ref_expect(c, data)
        assert full[0] == C.OK
        for cap in sorted(k for k in {0, 1, 4, 5, 65535, 65536, full[1] - 1} if k < full[1]):
            cc = dict(c, cap=cap)
            res, dl, _, out, _, _ = C.ref_expect(cc, data)
            assert (res, dl, out) == (C.OUTPUT_EOF, cap, full[3][:cap]), (C.key(cc), res, dl)
        cc = dict(c, cap=full[1])
        assert C.ref_expect(cc, data)[:2] == (C.OK, full[1])


@needs_ref
@pytest.mark.parametrize("part", range(4))
def test_random_cases_against_the_live_reference(emu, part):
    cases = C.random_cases(500, 7000 + part)
    assert len(cases) * 4 >= 2000
    seen = set()
    for c in cases:
        want = C.expect(c)
        run_case(emu, c, want)
        seen.add(want["res"])
    assert seen >= {C.OK, C.OUTPUT_EOF}


def test_props_checks_come_first(emu):
    data = C.gen("text", 1, 100)
    for kw in (dict(lc=9), dict(lp=5), dict(pb=5), dict(dict=(1 << 30) + 1), dict(lc=9, level=5)):
        got = C.emu_encode(emu, data, C.case("text", 1, 100, **kw), 64)
        assert got == (C.PARAM, 0, b"\0" * 5, b""), kw
    for kw in (dict(level=5), dict(level=9), dict(algo=1), dict(bt=1), dict(level=-1)):
        got = C.emu_encode(emu, data, C.case("text", 1, 100, **kw), 64)
        assert got == (C.UNSUPPORTED, 0, b"\0" * 5, b""), kw


def test_slice_layout(emu):
    """The hash geometry of MatchFinder_Create and the ring sized by the source."""
    f = emu.lzmaenc_emu_slice_bytes
    fixed = 1024 + 65536
    cells = 1846 + (0x300 << 3)

    def want(dict_size, src_len, mask, cells=cells):
        raw = ((cells * 2 + 15) & ~15) + 552 * 4 + (fixed + mask + 1) * 4 + \
            (min(dict_size, src_len) + 1) * 4
        return (raw + 255) & ~255
    assert f(4096, 3, 0, 100) == want(4096, 100, 0xFFFF)
    assert f(4096, 3, 0, 4096) == want(4096, 4096, 0xFFFF) == f(4096, 3, 0, 1 << 20)
    assert f(1 << 16, 3, 0, 1 << 20) == want(1 << 16, 1 << 20, 0xFFFF)
    assert f(1 << 20, 3, 0, 10) == want(1 << 20, 10, 0x7FFFF)
    assert f(1 << 24, 3, 0, 10) == want(1 << 24, 10, 0x7FFFFF)
    assert f(1 << 26, 3, 0, 10) == want(1 << 26, 10, 0xFFFFFF)   # the halving above 1 << 24
    assert f(4096, 8, 4, 10) == want(4096, 10, 0xFFFF, 1846 + (0x300 << 12))


def test_sanitizer_program_over_golden_and_edge_cases(tmp_path, golden):
    """g++ -O1 -fsanitize=address,undefined, own main, exact-size malloc'ed
    source and destination, poisoned exact-size workspace; every record twice
    with two poison bytes."""
    exe = C.build_emu(tmp_path, extra=("-O1", "-g", "-fsanitize=address,undefined",
                                       "-fno-sanitize-recover=undefined"), main=True)
    cases = {C.key(c): c for c in C.golden_cases() + C.edge_cases()}
    path = str(tmp_path / "cases.bin")
    C.write_case_file(path, list(cases.values()), golden)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "%d cases, 0 mismatches" % len(cases) in r.stdout

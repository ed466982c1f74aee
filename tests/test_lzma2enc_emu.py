"""csrc/lzma2enc_device.h on the host: the LZMA2 block encoder the kernel runs,
built with g++ -Wall -Werror (tests/emu_lzma2enc/lzma2enc_emu.cpp), against the
reference's single-threaded Lzma2Enc_Encode of the block alone -- live
(oracle/_ref/libref_lzma.so) over the edge list and 2,000 seeded random cases,
and over the committed goldens (tests/golden/lzma2enc_cases.json) everywhere.
With dst_cap = the block bound the block's bytes are the reference's minus its
final 0x00; res, the prop byte and the parsed chunk list are compared as well,
every output is decoded by Python's lzma, and nothing has a tolerance.  A
stand-alone sanitizer build of the emulator runs every golden and edge case as a
child process, each with two workspace poison bytes."""
import ctypes
import os
import subprocess

import pytest

import lzma2enc_cases as C
import native
import xzwrite

needs_ref = pytest.mark.skipif(not native.have_ref(), reason="reference library not built")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.load_emu(C.build_emu(tmp_path_factory.mktemp("lzma2enc_emu")))


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


def run_case(emu, c, want, data=None):
    data = C.data_of(c) if data is None else data
    cap = C.block_bound(len(data))
    got = C.emu_encode(emu, data, c, cap, 0x3C)
    C.check_block(got, want, C.key(c))
    # a second workspace poison: no entry of `son`, `matches` or the saved table
    # is read before it is written, or the two outputs would differ
    assert C.emu_encode(emu, data, c, cap, 0xA5) == got, C.key(c)
    if got[0] == C.OK:
        assert C.decode_raw(got[3] + b"\0", got[2]) == data, C.key(c)
    return got


def test_golden_file_is_what_the_generator_covers(golden):
    assert os.path.getsize(C.GOLDEN) < (1 << 18)
    assert [C.key(g["case"]) for g in golden["cases"]] == [C.key(c) for c in C.golden_cases()]
    assert {g["res"] for g in golden["cases"]} == {C.OK, C.PARAM}
    assert "segs" in golden["cases"][0]["case"] and "out" not in golden["cases"][0]


def test_the_patterns_the_shapes_were_chosen_for(golden):
    """(control & 0xE0 or copy control, unpack, pack) of the issue's table."""
    want = [
        [[0, 0, 0]],
        [[1, 1, 1], [0, 0, 0]],
        [[0xE0, 160396, 57348], [0x80, 139604, 48595], [0, 0, 0]],
        [[1, 56523, 56523], [2, 3477, 3477], [0, 0, 0]],
        [[1, 56527, 56527], [0xC0, 41473, 16872], [0, 0, 0]],
        [[0xE0, 81567, 57348], [2, 28433, 28433], [0, 0, 0]],
        [[0xE0, 160339, 57348], [2, 56448, 56448], [0x80, 40213, 15257], [0, 0, 0]],
    ]
    for c, chunks in zip(C.PATTERN_CASES, want):
        assert golden["by_key"][C.key(c)]["chunks"] == chunks, C.key(c)
    big = golden["by_key"][C.key(C.UNPACK_LIMIT_CASE)]["chunks"]
    assert big[0] == [0xE0, 2092927, 12211] and big[1][0] == 0x80 and len(big) == 3


def test_golden_cases(emu, golden):
    for g in golden["cases"]:
        run_case(emu, g["case"], dict(g, out=None))


@needs_ref
def test_goldens_are_the_live_reference(golden):
    for g in golden["cases"]:
        res, prop, out = C.ref_stream(g["case"])
        assert C.record(g["case"], res, prop, out) == {k: g[k] for k in g if k != "out"}, \
            C.key(g["case"])


@needs_ref
def test_edge_cases_against_the_live_reference(emu):
    for c in C.edge_cases():
        run_case(emu, c, C.expect(c))


@needs_ref
@pytest.mark.parametrize("part", range(4))
def test_random_cases_against_the_live_reference(emu, part):
    cases = C.random_cases(500, 9000 + part)
    assert len(cases) * 4 >= 2000
    controls = set()
    for c in cases:
        want = C.expect(c)
        run_case(emu, c, want)
        controls |= {t[0] for t in want["chunks"]}
    assert controls >= {0, 1, 2, 0x80, 0xC0, 0xE0}


def test_capacities(emu, golden):
    """dst_cap 0, 5, full - 1 and full: the full bytes with SZ_OK, or
    SZ_ERROR_OUTPUT_EOF with dest_len a whole-chunk prefix of them; nothing at
    or beyond dst_cap is written (emu_encode's guard)."""
    cases = [c for c in C.edge_cases() + C.random_cases(60, 9100) if C.size_of(c)]
    seen = set()
    for c in cases:
        data = C.data_of(c)
        want = C.expect(c, data, golden) if C.key(c) in golden["by_key"] or native.have_ref() \
            else None
        full = C.emu_encode(emu, data, c, C.block_bound(len(data)))
        if want is not None:
            C.check_block(full, want, C.key(c))
        if full[0] != C.OK:
            continue
        body = full[3]
        sizes = C.chunk_sizes(body)
        prefixes = {0}
        for s in sizes:
            prefixes.add(max(prefixes) + s)
        for cap in sorted({0, 5, len(body) - 1, len(body)}):
            res, dl, _, out = C.emu_encode(emu, data, c, cap)
            seen.add((res, cap == len(body)))
            if res == C.OK:
                assert cap == len(body) and out == body, (C.key(c), cap)
            else:
                assert res == C.OUTPUT_EOF, (C.key(c), cap, res)
                assert dl in prefixes and dl <= cap and out == body[:dl], (C.key(c), cap, dl)
                # the reference refuses a chunk before it tries when the room is below an
                # LZMA chunk header (Lzma2Enc.c:83-84): a last copy chunk shorter than
                # that header fails even at full
                assert cap < len(body) or sizes[-1] < 6, (C.key(c), cap)
    assert seen >= {(C.OK, True), (C.OUTPUT_EOF, False), (C.OUTPUT_EOF, True)}


def test_props_checks_come_first(emu):
    data = native.gen("text", 1, 100)
    for kw in (dict(lc=4, lp=1), dict(lc=0, lp=5), dict(lc=9, lp=0), dict(pb=5),
               dict(dict=(1 << 30) + 1), dict(lc=4, lp=1, level=5)):
        got = C.emu_encode(emu, data, C.case([("text", 1, 100)], **kw), 200)
        assert got == (C.PARAM, 0, 0, b""), kw
    for kw in (dict(level=5), dict(level=9), dict(level=-1)):
        got = C.emu_encode(emu, data, C.case([("text", 1, 100)], **kw), 200)
        assert got == (C.UNSUPPORTED, 0, 0, b""), kw


def test_slice_layout(emu):
    """The LZMA slice as it is, then the saved cells rounded up to 16 bytes."""
    out = (ctypes.c_uint64 * 2)()
    for dict_size, lc, lp, n in ((4096, 3, 0, 100), (1 << 16, 3, 0, 1 << 20), (1 << 20, 0, 4, 10),
                                 (1 << 16, 0, 0, 70000), (4096, 4, 0, 5)):
        emu.lzma2enc_emu_slice_bytes(dict_size, lc, lp, n, out)
        cells = 1846 + (0x300 << (lc + lp))
        saved = (cells * 2 + 15) & ~15
        assert out[0] % 256 == 0 and out[1] == out[0] + ((saved + 255) & ~255)


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


# ---------------------------------------------------------------- framing, host only

def test_props_init_and_normalize(emu):
    p = C.CLzma2EncProps()
    emu.lzma2enc_emu_props_init(ctypes.byref(p))
    assert (p.lzmaProps.level, p.lzmaProps.dictSize, p.lzmaProps.numThreads, p.blockSize,
            p.numBlockThreads, p.numTotalThreads) == (5, 0, -1, 0, -1, -1)
    assert ctypes.sizeof(p) == 64 and C.CLzma2EncProps.blockSize.offset == 48
    for given, want in C.NORMALIZE:
        emu.lzma2enc_emu_props_init(ctypes.byref(p))
        (p.lzmaProps.level, p.lzmaProps.dictSize, p.blockSize, p.numBlockThreads,
         p.numTotalThreads, p.lzmaProps.numThreads) = given
        emu.lzma2enc_emu_props_normalize(ctypes.byref(p))
        got = (p.lzmaProps.numThreads, p.numBlockThreads, p.numTotalThreads, p.blockSize,
               p.lzmaProps.dictSize)
        assert got == want, (given, got, want)


def test_prop_byte(emu):
    for d in (1, 4095, 4096, 4097, 6144, 6145, 8192, 1 << 16, (1 << 16) + 1, 3 << 15, C.MIB,
              C.MIB + 1, 3 << 19, 1 << 24, 1 << 30, (1 << 30) + 1, 3 << 30, (3 << 30) + 1,
              0xFFFFFFFF):
        assert emu.lzma2enc_emu_prop_byte(d) == xzwrite.lzma2_prop(d), d
    assert emu.lzma2enc_emu_prop_byte(4096) == 0 and emu.lzma2enc_emu_prop_byte(0xFFFFFFFF) == 40

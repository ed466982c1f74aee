"""The library's own LZMA2 streaming walker (Lzma2Dec_DecodeToBuf,
Lzma2Dec_DecodeToDic, Lzma2Dec_Allocate in dropin_capi.hip), call by call
against the reference's Lzma2Dec.c.

tests/lzma2_stream.py drives either library through the same two loops;
tests/golden/lzma2_stream_cases.json holds what the reference answered for
every cell of the grid (call count, SHA-256 of trace and of output).  The CPU
tests pin the file to the grid, to the live reference where it is built, and
to the coverage conditions the grid is there for; the GPU tests run the grid
through liblzmagpu.so from a 24-thread pool, so concurrent walkers share
session launches."""
import ctypes
import hashlib
import time
from concurrent.futures import ThreadPoolExecutor

import pytest

import lzma2_stream as S
import native

STEP_LIMIT_S = 60     # the launch-bearing step limit of tests/test_ppmd7.py
MAX_CALLS = 20_000    # per GPU test, by the recorded call counts
# name prefixes (lzma2_stream.cases()) and loops of each GPU test
PARTS = {"hand buf": ("hand", ("buf",)), "hand dic": ("hand", ("dic",)),
         "golden buf": ("golden", ("buf",)), "golden dic": ("golden", ("dic",)),
         "long": ("long", S.LOOPS)}


def _cells(part):
    prefix, loops = PARTS[part]
    return [c for c in S.grid(prefix) if c[2] in loops]


# ------------------------------------------------------------------ CPU

def test_file_grid_is_the_modules_grid():
    g = S.golden()
    keys = [S.key(*c) for c in S.grid()]
    assert len(set(keys)) == len(keys) and set(keys) == set(g["runs"])
    assert sorted(keys) == sorted(k for p in PARTS for k in (S.key(*c) for c in _cells(p)))
    hand = [c for c in S.cases() if c["name"].startswith("hand")]
    assert len(hand) == 24 and sum(c["cap"] <= S.SMALL_CAP for c in hand) == 22
    assert len([c for c in S.cases() if c["name"].startswith("golden")]) == 20
    # the liblzma-made inputs are the ones the file was recorded for
    assert g["streams"] == {c["name"]: hashlib.sha256(c["src"]).hexdigest()
                            for c in S.cases() if "plain" in c}
    for p in PARTS:
        n = sum(g["runs"][S.key(*c)]["calls"] for c in _cells(p))
        assert 0 < n < MAX_CALLS, (p, n)


def test_long_streams_begin_with_a_stored_chunk_longer_than_the_ring():
    """liblzma stores the random block as one chunk of many rings and copies
    from it in the LZMA chunk that follows (no dictionary reset in between)."""
    long_ = [c for c in S.cases() if "plain" in c]
    assert len(long_) == 2
    for c in long_:
        ch = S.lzma2_chunks(c["src"])
        assert S.well_formed(c) and sum(x[2] for x in ch) == len(c["plain"]) == c["cap"]
        assert [x[1] for x in ch] == [1, 0xC0], [hex(x[1]) for x in ch]
        assert ch[0][2] > 10 * S.RING0 and c["prop"] == 0
    src, cap = S.ring_straddle()
    ch = S.lzma2_chunks(src)
    assert [x[1] & 0xE0 for x in ch] == [0xE0, 0, 0x80] and ch[0][2] < S.RING0 < ch[0][2] + ch[1][2]


@pytest.mark.skipif(not native.have_ref(), reason="reference library not built")
def test_live_reference_equals_file():
    g, ref = S.golden()["runs"], native.ref()
    bad = [k for k, r in ((S.key(*c), S.record(S.run(ref, c))) for c in S.grid()) if g[k] != r]
    assert not bad, (len(bad), bad[:5])


def test_recorded_runs_cover_the_walkers_branches():
    """Every condition the grid is there for has a recorded witness (run and
    call); the live reference, where built, shows it at that very call."""
    g = S.golden()
    assert set(g["witness"]) == set(S.CONDITIONS)
    cells = {S.key(*c): c for c in S.grid()}
    for cond, (k, at) in g["witness"].items():
        assert k in cells and 0 <= at < g["runs"][k]["calls"], (cond, k, at)
        if native.have_ref():
            assert S.well_formed(cells[k][0])
            assert S.holds(cond, cells[k], S.run(native.ref(), cells[k])) == at, cond


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def _gpu(L):
    if L.device_count() <= 0:
        pytest.fail("no HIP device: " + L.last_error())


def _pool(L, cells, between=None):
    S._decl(L.lib)
    t0 = time.monotonic()
    with ThreadPoolExecutor(24) as ex:
        got = list(ex.map(lambda c: S.run(L.lib, c, between), cells))
    took = time.monotonic() - t0
    assert took < STEP_LIMIT_S, took
    return got, took


def _compare(cells, got):
    g = S.golden()["runs"]
    bad = [(S.key(*c), S.record(r)["calls"], g[S.key(*c)]["calls"], r[0][-2:])
           for c, r in zip(cells, got) if S.record(r) != g[S.key(*c)]]
    assert not bad, (len(bad), bad[:4])
    if native.have_ref():
        ref = native.ref()
        for c, r in zip(cells, got):
            w = S.run(ref, c)
            assert (r[0], r[1], r[2]) == (w[0], w[1], w[2]), S.key(*c)


@pytest.mark.gpu
@pytest.mark.parametrize("part", list(PARTS))
def test_gpu_lzma2_streaming_pool(L, part):
    """The grid through liblzmagpu.so's walker, 24 walkers at a time: every
    trace, output and input count equals the recorded reference's (and the
    live one's where it is built).  Every LZMA chunk piece is a launch."""
    _gpu(L)
    cells = _cells(part)
    calls = sum(S.golden()["runs"][S.key(*c)]["calls"] for c in cells)
    assert calls < MAX_CALLS
    L.path_stats(reset=True)
    got, took = _pool(L, cells)
    stats = L.path_stats()
    print(f"\n{part}: {len(cells)} runs, {calls} calls, {took:.1f} s, {stats}")
    _compare(cells, got)
    if part == "long":
        # the stored chunk of many rings reaches the first decoder call as a
        # whole-dictionary upload; the straddling stored chunk between two
        # decoder calls as a span in two pieces (buf loop) and in one (dic loop)
        assert stats["history_upload"] >= 1 and stats["span_two"] >= 1 and stats["span_one"] >= 1
    if part == "hand buf":
        assert stats["span_one"] >= 1  # "0xE0, stored 0x02, then 0x80"


@pytest.mark.gpu
def test_gpu_lzma2_streaming_mirror_dropped_every_7th_call(L):
    """LzmaGpu_DecoderRelease(&dec.decoder) after every 7th walker call: the
    next decoder call rebuilds its mirror from the host copies.  Nothing
    changes."""
    _gpu(L)
    cells = _cells("long") + [c for c in _cells("hand buf") if c[3:] == (5, 7)]
    calls = sum(S.golden()["runs"][S.key(*c)]["calls"] for c in cells)
    assert calls < MAX_CALLS

    def between(k, dec):
        if k % 7 == 0:
            L.lib.LzmaGpu_DecoderRelease(ctypes.byref(dec.decoder))

    L.path_stats(reset=True)
    got, took = _pool(L, cells, between)
    stats = L.path_stats()
    print(f"\nmirror dropped: {len(cells)} runs, {calls} calls, {took:.1f} s, {stats}")
    _compare(cells, got)
    assert stats["history_upload"] >= 1

"""The branches of dropin_capi.hip that a SIZE FIELD picks, each reached with a
small stream beside a large capacity and proved by LzmaGpu_DropinPathStats:

  B  tables wider than lc + lp = 4 through LzmaDec_DecodeToBuf / DecodeToDic:
     the cooperative session kernel at its widest LDS table (lc + lp = 5), the
     one-lane session kernel above it, and launches that carry both;
  C  the staging tiers: one-call batches through pageable memory and with
     per-call output downloads, session calls without pinned staging;
  D  mirror eviction (by count, by byte budget) and a decoder that starts on
     another decoder's retired, dirty device block.

Every expectation is the oracle's (tests/native.py: the restatement pinned to
the reference) or the recorded reference's (tests/handmade_cases.py).  The
thresholds are literals here on purpose: if a constant of the library moves,
the counters make the test fail instead of letting it check another tier."""
import ctypes
import json
import lzma
import os
import random
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import golden_cases as G
import handmade_cases as H
import lzmaenc_min as E
import native

STEP_LIMIT_S = 60           # the launch-bearing step limit of tests/test_ppmd7.py
CHILD_LIMIT_S = 120         # the child-process limit of tests/test_coalesce.py
MIB = 1 << 20
SET_PIN_MAX = 96 * MIB      # kSetPinMax: one-call batches above it stage pageable
BULK_OUT_MAX = 64 * MIB     # kBulkOutMax: outputs above it are downloaded per call
PINNED_STAGE_MAX = 8 * MIB  # kPinnedStageMax: session calls above it go unpinned
COOP_MAX_CELLS = 32768      # kSessCoopMaxCells: wider tables take the one-lane kernel
MIRROR_MAX_COUNT = 256      # kMirrorMaxCount
BIG = 1 << 20
CHUNKINGS = ((BIG, BIG), (1000, 3000), (100, 333), (1, 1))
BYTEWISE_CAP = 600          # (1, 1) runs stop after this many output bytes


def table_cells(lc, lp, pb):
    """The cells a decoder uses (the compact device layout, tests/test_abi.py)."""
    return 56 * (1 << pb) + 950 + (768 << (lc + lp))


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    if lzmagpu.device_count() <= 0:
        pytest.fail("no HIP device: " + lzmagpu.last_error())
    return lzmagpu


def _timed(fn):
    t0 = time.monotonic()
    r = fn()
    took = time.monotonic() - t0
    assert took < STEP_LIMIT_S, took
    return r


def _delta(L, fn):
    before = L.path_stats()
    r = _timed(fn)
    after = L.path_stats()
    return r, {k: after[k] - before[k] for k in after}


def _text_stream(seed, n, dict_size=1 << 16, lc=3, lp=0, pb=2):
    data = native.gen("text", seed, n)
    comp = lzma.compress(data, format=lzma.FORMAT_RAW, filters=[
        {"id": lzma.FILTER_LZMA1, "dict_size": dict_size, "lc": lc, "lp": lp, "pb": pb}])
    return data, comp, E.props(lc, lp, pb, dict_size)


# ------------------------------------------------------------------ B: wide tables

def _hand_wide(lc, lp, pb, seed):
    """About 6,000 bytes at lc + lp = 5: literals, then matches inside a 4 KiB
    dictionary with literals between them."""
    rng = random.Random(seed)
    e = E.Encoder(lc, lp, pb)
    for _ in range(1500):
        e.literal(rng.choice(H.ALPHA))
    while e.total < 6000:
        e.match(rng.randrange(1, min(e.total, 4096) + 1), rng.randrange(2, 60))
        for _ in range(rng.randrange(0, 4)):
            e.literal(rng.choice(H.ALPHA))
    return dict(name=f"hand lc{lc}lp{lp}pb{pb}", src=e.finish(), props=E.props(lc, lp, pb, 4096),
                plain=bytes(e.out), plp=(lc, lp, pb))


_W = {}


def wide_streams():
    if "w" in _W:
        return _W["w"]
    d, out = G.load(), []
    for plp, sizes in (((5, 1, 0), (300,)), ((7, 0, 1), (300,)), ((4, 4, 4), (300,)),
                       ((8, 0, 0), (0, 1))):
        pbyte = (plp[2] * 5 + plp[1]) * 9 + plp[0]
        for _, c in G.cases("lzma"):
            if bytes.fromhex(c["props"])[0] == pbyte and c["note"] == "exact END" and \
                    not c["flips"] and c["trunc"] is None and c["dest_cap"] in sizes and \
                    d["streams"][c["stream"]]["note"].startswith("text "):
                out.append(dict(name="golden " + d["streams"][c["stream"]]["note"],
                                src=G.case_input(d, c), props=bytes.fromhex(c["props"]),
                                plain=None, cap=c["dest_cap"], plp=plp))
    assert len(out) == 10, [s["name"] for s in out]  # with and without end mark
    for k, plp in enumerate(((5, 0, 2), (1, 4, 0), (3, 2, 4))):
        out.append(_hand_wide(*plp, seed=70 + k))
    rng = random.Random(80)
    e = E.Encoder(8, 4, 0)
    for _ in range(30):
        e.literal(rng.choice(H.ALPHA))
    e.match(7, 20)
    for _ in range(5):
        e.literal(rng.choice(H.ALPHA))
    out.append(dict(name="hand lc8lp4pb0", src=e.finish(), props=E.props(8, 4, 0, 4096),
                    plain=bytes(e.out), plp=(8, 4, 0)))
    for s in out:
        if s["plain"] is not None:
            s["cap"] = len(s["plain"])
    _W["w"] = out
    return out


def _wide_jobs():
    """(stream, loop, in_chunk, out_chunk, finish, capacity)."""
    jobs = []
    for s in wide_streams():
        for i, o in CHUNKINGS:
            cap = min(s["cap"], BYTEWISE_CAP) if (i, o) == (1, 1) else s["cap"]
            for fin in (0, 1):
                jobs.append((s, "buf", i, o, fin, cap))
            jobs.append((s, "dic", i, o, 1, cap))
    return jobs


def _run_gpu(L, j):
    s, loop, i, o, fin, cap = j
    if loop == "buf":
        return L.stream_decode(s["src"], s["props"], cap, i, o, fin, max_calls=20000)
    return L.dic_decode(s["src"], s["props"], cap, i, max_calls=20000)


def _run_orc(j):
    s, loop, i, o, fin, cap = j
    orc = native.oracle()
    if loop == "buf":
        return native.stream_decode(orc, "orc", s["src"], s["props"], cap, i, o, fin,
                                    max_calls=20000)
    return native.dic_decode(orc, "orc", s["src"], s["props"], cap, i, max_calls=20000)[:4]


def _same(g, w):
    return g[0] == w[0] and [tuple(r) for r in g[1]] == [tuple(r) for r in w[1]] and \
        g[2] == w[2] and g[3] == w[3]


def _want(jobs):
    key = lambda j: (j[0]["name"],) + j[1:]
    for j in jobs:
        if key(j) not in _W:
            _W[key(j)] = _run_orc(j)
    return [_W[key(j)] for j in jobs]


def test_oracle_decodes_the_hand_encoded_wide_streams():
    """The streams are what the encoder meant: the oracle's whole-stream loop
    gives the encoder's own output (runs beside the GPU tests: no device)."""
    for s in wide_streams():
        if s["plain"] is not None:
            w = _run_orc((s, "buf", BIG, BIG, 0, s["cap"]))
            assert w[2] == s["plain"] and w[1][-1][0] == 0, s["name"]
    cells = sorted({table_cells(*s["plp"]) for s in wide_streams()})
    assert 26422 in cells and cells[0] > 14134 and any(c > COOP_MAX_CELLS for c in cells)


@pytest.mark.gpu
def test_wide_tables_through_both_interfaces(L):
    """Every wide stream through LzmaDec_DecodeToBuf (both finish modes) and
    LzmaDec_DecodeToDic loops at the four chunkings, call by call against the
    oracle.  The 6,000-byte streams take (1, 1) over their first 600 bytes."""
    jobs = _wide_jobs()
    want = _want(jobs)
    assert sum(w[0] for w in want) < 20_000
    with ThreadPoolExecutor(24) as ex:
        got, stats = _delta(L, lambda: list(ex.map(lambda j: _run_gpu(L, j), jobs)))
    print(f"\nwide tables: {len(jobs)} runs, {sum(w[0] for w in want)} calls, {stats}")
    bad = [(j[0]["name"],) + j[1:] + (g[0], w[0], g[1][-1:], w[1][-1:])
           for j, g, w in zip(jobs, got, want) if not _same(g, w)]
    assert not bad, (len(bad), bad[:4])
    assert stats["sess_coop"] > 0 and stats["sess_global"] > 0


@pytest.mark.gpu
def test_wide_table_with_two_mib_input_goes_unpinned(L):
    """lc8 lp4: a 6.3 MB table and a 2 MiB input chunk need more than the 8 MiB
    pinned staging: table and input travel from the caller's memory."""
    s = next(x for x in wide_streams() if x["plp"] == (8, 4, 0))
    assert 2 * table_cells(8, 4, 0) + 2 * MIB > PINNED_STAGE_MAX > 2 * table_cells(8, 4, 0)
    padded = dict(s, src=s["src"] + bytes(2 * MIB - len(s["src"])))
    j = (padded, "buf", 2 * MIB, BIG, 0, s["cap"])
    w = _run_orc(j)
    g, stats = _delta(L, lambda: _run_gpu(L, j))
    assert _same(g, w) and g[2] == s["plain"], (g[:2], w[:2])
    assert stats["sess_unpinned"] == 1 and stats["sess_pinned"] == 0 and stats["sess_global"] == 1


@pytest.mark.gpu
def test_narrow_widest_lds_and_global_sessions_share_launches(L):
    """24 threads interleave narrow (3,0,2), widest-LDS (lc + lp = 5) and
    one-lane-kernel streams: every trace equals the oracle's and the counters
    show cooperative calls, one-lane calls and a launch that carried both
    (group commit makes the mix depend on timing: up to 5 passes)."""
    ws = wide_streams()
    data, comp, props = _text_stream(31, 3000)
    narrow = dict(name="narrow text", src=comp, props=props, cap=len(data), plp=(3, 0, 2))
    lds = [s for s in ws if s["plp"][0] + s["plp"][1] == 5]
    glob = [s for s in ws if COOP_MAX_CELLS < table_cells(*s["plp"]) < 10 ** 6 and s["cap"] >= 300]
    assert len(lds) == 3 and len(glob) == 6
    assert max(table_cells(*s["plp"]) for s in lds) == 26422  # the widest LDS table
    jobs = []
    for k in range(24):
        for s in (narrow, lds[k % 3], glob[k % 6]):
            jobs.append((s, "buf", 11, 13, k & 1, min(s["cap"], 400)))
    want = _want(jobs)
    total = dict(sess_coop=0, sess_global=0, sess_mixed=0)
    for _ in range(5):
        with ThreadPoolExecutor(24) as ex:
            got, stats = _delta(L, lambda: list(ex.map(lambda j: _run_gpu(L, j), jobs)))
        bad = [(j[0]["name"],) + j[1:] for j, g, w in zip(jobs, got, want) if not _same(g, w)]
        assert not bad, (len(bad), bad[:4])
        for k in total:
            total[k] += stats[k]
        if total["sess_mixed"]:
            break
    print(f"\nmixed launches: {total}")
    assert total["sess_coop"] > 0 and total["sess_global"] > 0 and total["sess_mixed"] >= 1


# ------------------------------------------------------------------ C: staging tiers

def _one_call(L, buf, in_size, props, cap, finish, dest=None):
    """LzmaDecode over a caller's ctypes buffer (no copies of a 97 MiB input)."""
    dest = dest if dest is not None else ctypes.create_string_buffer(max(cap, 1))
    dl, sl, st = ctypes.c_size_t(cap), ctypes.c_size_t(in_size), ctypes.c_int(-1)
    r = L.lib.LzmaDecode(dest, ctypes.byref(dl), buf, ctypes.byref(sl), bytes(props), len(props),
                         finish, ctypes.byref(st), ctypes.byref(L.g_alloc))
    return r, st.value, dl.value, sl.value, dest.raw[:dl.value]


def _orc_one_call(buf, in_size, props, cap, finish):
    orc = native.oracle()
    dst = ctypes.create_string_buffer(max(cap, 1))
    dl, sl, st = ctypes.c_size_t(cap), ctypes.c_size_t(in_size), ctypes.c_int(-1)
    r = orc.orc_lzma_decode(dst, ctypes.byref(dl), buf, ctypes.byref(sl), props, len(props),
                            finish, ctypes.byref(st))
    return r, st.value, dl.value, sl.value, dst.raw[:dl.value]


def _padded(comp, size):
    buf = ctypes.create_string_buffer(size)
    ctypes.memmove(buf, comp, len(comp))
    return buf


@pytest.mark.gpu
def test_one_call_pageable_alone_and_in_a_batch(L):
    """One LzmaDecode whose input is a small stream padded to 97 MiB: over the
    96 MiB pinned limit the batch uploads from and downloads to the callers'
    own buffers.  Alone, then from a pool beside 40 small calls -- six copies
    of the big call (one shared read-only input) go first, so that with every
    batch set busy the rest wait together and a pageable batch carries more
    than one call (fewer pageable batches than big calls shows it; group commit
    makes that depend on timing: up to 5 passes, reported, not required)."""
    data, comp, props = _text_stream(41, 5000)
    buf = _padded(comp, 97 * MIB)
    want = _orc_one_call(buf, 97 * MIB, props, len(data), 0)
    assert want[0] == 0 and want[2] == len(data) and want[4] == data
    got, stats = _delta(L, lambda: _one_call(L, buf, 97 * MIB, props, len(data), 0))
    assert got == want, (got[:4], want[:4])
    assert stats["one_pageable"] == 1 and stats["one_percall_out"] == 1 and stats["one_pinned"] == 0
    small = [_text_stream(4100 + k, 100 + 37 * k) for k in range(40)]
    wants = [want] * 6 + [native.decode(native.oracle(), "orc", c, p, len(d_), 1)
                          for d_, c, p in small]

    def run(k):
        if k < 6:
            return _one_call(L, buf, 97 * MIB, props, len(data), 0)
        d_, c, p = small[k - 6]
        return L.LzmaDecode(c, p, len(d_), 1)

    shared = False
    for _ in range(5):
        with ThreadPoolExecutor(24) as ex:
            gots, stats = _delta(L, lambda: list(ex.map(run, range(46))))
        bad = [(k, g[:4], w[:4]) for k, (g, w) in enumerate(zip(gots, wants)) if g != w]
        assert not bad, bad[:4]
        assert stats["one_pageable"] >= 1
        shared = shared or stats["one_pageable"] < 6
        if shared:
            break
    print(f"\npageable batch of several calls seen: {shared} {stats}")
    del buf


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["96 MiB pinned", "96 MiB + 16 pageable", "64 MiB bulk",
                                  "64 MiB + 16 per call"])
def test_one_call_size_boundaries(L, what):
    """Each side of the two size thresholds of run_batch, one call each.  The
    pinned need of a one-call batch is align16(in) + align16(out) + 160 (its
    descriptor, order word, result and slack)."""
    data, comp, props = _text_stream(42, 3000)
    if what.startswith("96"):
        cap = len(data)
        in_size = SET_PIN_MAX - 160 - ((cap + 15) & ~15) + (16 if "+" in what else 0)
        expect = dict(one_pinned=0, one_pageable=1, one_percall_out=1) if "+" in what else \
            dict(one_pinned=1, one_pageable=0, one_percall_out=0)
    else:
        cap = BULK_OUT_MAX + (16 if "+" in what else 0)
        in_size = len(comp)
        expect = dict(one_pinned=1, one_pageable=0, one_percall_out=1 if "+" in what else 0)
    buf = _padded(comp, in_size)
    want = _orc_one_call(buf, in_size, props, cap, 0)
    assert want[4] == data
    dest = ctypes.create_string_buffer(cap)
    got, stats = _delta(L, lambda: _one_call(L, buf, in_size, props, cap, 0, dest))
    assert got == want, (got[:4], want[:4])
    assert {k: stats[k] for k in expect} == expect
    del buf, dest


_S = {}


def _stream40k():
    if "s" not in _S:
        _S["s"] = _text_stream(43, 40_000)
    return _S["s"]


@pytest.mark.gpu
def test_session_dic_calls_with_a_nine_mib_dictionary_go_unpinned(L):
    """LzmaDec_DecodeToDic over a 9 MiB flat dictionary with dicLimit =
    dicBufSize: the room to download exceeds the pinned staging, so the bytes
    land in the caller's dictionary directly -- dic[0, dicPos) is the
    plaintext and the rest keeps its poison."""
    data, comp, props = _stream40k()
    size = 9 * MIB
    w = native.dic_decode(native.oracle(), "orc", comp, props, size, 4096, max_calls=1000)[:4]
    assert w[2] == data and w[0] >= 3
    dic = ctypes.create_string_buffer(size)
    ctypes.memset(dic, 0xA5, size)
    g, stats = _delta(L, lambda: L.dic_decode(comp, props, size, 4096, max_calls=1000, out=dic))
    assert _same(g, w), (g[:2], w[:2])
    assert stats["sess_unpinned"] == g[0] and stats["sess_pinned"] == 0
    arr = np.frombuffer(dic, dtype=np.uint8)
    assert arr[:len(data)].tobytes() == data and bool((arr[len(data):] == 0xA5).all())
    del arr, dic


@pytest.mark.gpu
def test_session_buf_calls_with_nine_mib_room_or_input_go_unpinned(L):
    """LzmaDec_DecodeToBuf with destLen = 9 MiB, and one call whose srcLen is
    9 MiB (the stream plus padding) with exact output room."""
    data, comp, props = _stream40k()
    size = 9 * MIB
    j = (dict(src=comp, props=props), "buf", 4096, size, 0, size)
    w = _run_orc(j)
    assert w[2] == data
    g, stats = _delta(L, lambda: _run_gpu(L, j))
    assert _same(g, w), (g[:2], w[:2])
    assert stats["sess_unpinned"] == g[0] and stats["sess_pinned"] == 0
    j = (dict(src=comp + bytes(size - len(comp)), props=props), "buf", size, BIG, 0, len(data))
    w = _run_orc(j)
    assert w[0] == 1 and w[2] == data
    g, stats = _delta(L, lambda: _run_gpu(L, j))
    assert _same(g, w), (g[:2], w[:2])
    assert stats["sess_unpinned"] == 1 and stats["sess_pinned"] == 0


@pytest.mark.gpu
def test_session_call_at_exactly_eight_mib_stays_pinned(L):
    """The staging need of a DecodeToBuf call is its table (padded to 16
    bytes) plus its output room: at 8 MiB exactly it is pinned, 16 bytes more
    and the first call is not (any later call has less room left)."""
    data, comp, props = _stream40k()
    tab_pad = (2 * table_cells(3, 0, 2) + 15) & ~15
    for extra, unpinned in ((0, 0), (16, 1)):
        room = PINNED_STAGE_MAX - tab_pad + extra
        j = (dict(src=comp, props=props), "buf", BIG, room, 0, room)
        w = _run_orc(j)
        assert w[2] == data and w[0] >= 1
        g, stats = _delta(L, lambda: _run_gpu(L, j))
        assert _same(g, w), (g[:2], w[:2])
        assert stats["sess_unpinned"] == unpinned and stats["sess_pinned"] == g[0] - unpinned, stats


# ------------------------------------------------------------------ D: mirrors and the pool

class _Dec:
    """A CLzmaDec over a caller-owned flat dictionary (LzmaDec_AllocateProbs)."""

    def __init__(self, L, props, size, poison=None, lib=None):
        self.L, self.d, self.lib = L, L.CLzmaDec(), lib or L.lib
        self.d.dic = None
        self.d.probs = None
        r = self.lib.LzmaDec_AllocateProbs(ctypes.byref(self.d), bytes(props), 5,
                                        ctypes.byref(L.g_alloc))
        assert r == 0, r
        self.dic = ctypes.create_string_buffer(max(size, 1))
        if poison is not None:
            ctypes.memset(self.dic, poison, max(size, 1))
        self.d.dic = ctypes.addressof(self.dic)
        self.d.dicBufSize = size
        self.lib.LzmaDec_Init(ctypes.byref(self.d))

    def to_dic(self, limit, src, finish):
        """(res, status, srcLen, dicPos) of one LzmaDec_DecodeToDic call."""
        sbuf = ctypes.create_string_buffer(bytes(src), max(len(src), 1))
        sl, st = ctypes.c_size_t(len(src)), ctypes.c_int(-1)
        r = self.lib.LzmaDec_DecodeToDic(ctypes.byref(self.d), limit, sbuf, ctypes.byref(sl),
                                           finish, ctypes.byref(st))
        return r, st.value, sl.value, self.d.dicPos

    def free(self):
        self.lib.LzmaDec_FreeProbs(ctypes.byref(self.d), ctypes.byref(self.L.g_alloc))


@pytest.mark.gpu
def test_more_decoders_than_mirrors(L):
    """300 decoders on one thread, advanced round-robin through 3 DecodeToDic
    calls each: beyond 256 mirrors every new one evicts the least recently
    used, and a decoder that comes back restarts from its host copy."""
    data, comp, props = _text_stream(51, 20_000)
    win = (len(comp) + 2) // 3
    w = native.dic_decode(native.oracle(), "orc", comp, props, len(data), win, max_calls=10)
    assert w[0] == 3 and w[2] == data
    want = [tuple(r) for r in w[1]]
    decs = [_Dec(L, props, len(data)) for _ in range(300)]
    try:
        before = L.path_stats()
        t0 = time.monotonic()
        for k in range(3):
            part = comp[k * win:(k + 1) * win]
            got = [d.to_dic(len(data), part, L.LZMA_FINISH_END) for d in decs]
            assert got == [want[k]] * 300, (k, [g for g in got if g != want[k]][:3], want[k])
            if k == 0:
                s = L.path_stats()
                assert s["mirror_evicted"] - before["mirror_evicted"] >= 300 - MIRROR_MAX_COUNT
        assert time.monotonic() - t0 < STEP_LIMIT_S
        s = L.path_stats()
        assert s["history_upload"] - before["history_upload"] > 0
        print(f"\n300 decoders: { {k: s[k] - before[k] for k in s} }")
        assert all(d.dic.raw[:len(data)] == data for d in decs[::37])
    finally:
        for d in decs:
            d.free()


CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin_budget_child.py")


@pytest.mark.gpu
def test_mirror_budget_of_one_mib_in_a_child_process():
    """LZGPU_MIRROR_BUDGET_MB=1 (read once per process: a fresh child): 16
    threads in DecodeToBuf loops over 64 KiB rings hold more than the budget at
    once.  Nothing spins or fails; every trace equals the oracle's."""
    import dropin_budget_child as C
    env = dict(os.environ, LZGPU_MIRROR_BUDGET_MB="1")
    p = subprocess.run([sys.executable, CHILD], env=env, timeout=CHILD_LIMIT_S,
                       capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    doc = json.loads(p.stdout.strip().splitlines()[-1])
    orc = native.oracle()
    for k, (data, comp, props) in enumerate(C.streams()):
        w = native.stream_decode(orc, "orc", comp, props, len(data), C.IN_CHUNK, C.OUT_CHUNK, 0,
                                 max_calls=5000)
        g = doc["runs"][k]
        assert g["calls"] == w[0] and [tuple(r) for r in g["trace"]] == [tuple(r) for r in w[1]]
        assert g["sha256"] == G.sha(w[2]) and g["used"] == w[3] and w[2] == data
    print(f"\nbudget child: {doc['stats']}")
    assert doc["stats"]["mirror_evicted"] > 0 and doc["stats"]["sess_coop"] > 0


def _dirty_cases():
    return [c for c in H.lzma_cases() if c["group"] in ("edge_unfilled", "rep_first")]


def _one_dic_call(new_dec, c, finish, size):
    """The case as one DecodeToDic call (dicLimit = its capacity) on a fresh
    decoder over a flat dictionary of `size` bytes: LzmaDecode's own sequence
    (LzmaDec.c:972-1002), so the answer is the recorded one-call answer, with
    SZ_ERROR_INPUT_EOF standing for SZ_OK + NEEDS_MORE_INPUT."""
    d = new_dec(c["props"], size)
    try:
        res, status, used, pos = d.to_dic(c["cap"], c["src"], finish)
        out = d.dic.raw[:pos]
    finally:
        d.free()
    if res == 0 and status == 3:
        res = 6
    return (res, status, pos, used), H.sha(out)


@pytest.mark.skipif(not native.have_ref(), reason="reference library not built")
def test_one_dic_call_on_the_reference_is_the_recorded_one_call_answer():
    """_one_dic_call through the reference's LzmaDec.c gives what
    handmade_cases.expected() holds for the one-call decode (no device)."""
    import lzmagpu as L
    ref = native.ref()
    vp = ctypes.c_void_p
    for name, args in (("LzmaDec_AllocateProbs", [vp, ctypes.c_char_p, ctypes.c_uint, vp]),
                       ("LzmaDec_Init", [vp]), ("LzmaDec_FreeProbs", [vp, vp]),
                       ("LzmaDec_DecodeToDic", [vp, ctypes.c_size_t, vp, vp, ctypes.c_int, vp])):
        getattr(ref, name).argtypes = args
    for c in _dirty_cases():
        for finish in (0, 1):
            got = _one_dic_call(lambda p, n: _Dec(L, p, n, poison=0x5A, lib=ref), c, finish, MIB)
            want = H.expected(c, finish)
            assert got == (tuple(want[0]), want[1]), (c["name"], finish, got, want)


@pytest.mark.gpu
def test_decoders_on_a_retired_dirty_block(L):
    """A decoder with a 1 MiB dictionary decodes 1 MiB of text and is freed: its
    device block goes to the pool full of data.  Fresh decoders over 1 MiB
    dictionaries then take a pooled block for their first call (the pool
    counter moves for each) and answer every edge_unfilled and rep_first case
    as recorded: a match that reaches before the stream's start is
    SZ_ERROR_DATA, never stale bytes."""
    data, comp, props = _text_stream(61, MIB, dict_size=MIB, lc=4, lp=0, pb=2)
    d = _Dec(L, props, MIB)
    try:
        r = _timed(lambda: d.to_dic(MIB, comp, L.LZMA_FINISH_ANY))
        assert r[0] == 0 and r[3] == MIB and d.dic.raw == data
    finally:
        d.free()
    cases = _dirty_cases()
    assert len(cases) == 21 and all(len(c["src"]) >= 5 and c["cap"] <= MIB for c in cases)
    bad = []
    t0 = time.monotonic()
    for c in cases:
        for finish in (0, 1):
            before = L.path_stats()["pool_reused"]
            got = _one_dic_call(lambda p, n: _Dec(L, p, n, poison=0x5A), c, finish, MIB)
            assert L.path_stats()["pool_reused"] > before, c["name"]
            want = H.expected(c, finish)
            if got != (tuple(want[0]), want[1]):
                bad.append((c["name"], finish, got, want))
    assert time.monotonic() - t0 < STEP_LIMIT_S
    assert not bad, (len(bad), bad[:4])
    assert any(H.expected(c, 1)[0][0] == 1 for c in cases)

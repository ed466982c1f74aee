"""The hand-made LZMA set (tests/handmade_cases.py) through the decoders that
resume in mid-stream, at cuts no encoder's output puts there: inside a
273-byte overlapping match, on the symbol before an end marker, on an edge
distance, inside a byte-hungry symbol, in the round before a data error, over
the ring's wrap and either side of the reference's 20-byte tempBuf threshold.

CPU: the reference's streaming loops over the chunk grid of
tests/handmade_stream.py as recorded digests (the oracle's loop and, where it
is built, the live reference equal them); the host builds of the lane code --
the time-sliced kernels' own sliced_step at every slice (emu_sliced_decode),
the session loops over the grid -- and the coverage conditions, read from the
encoders' records and the expected traces.

GPU: the time-sliced batch kernels (lane in both placements, cooperative,
global) at slices from 1 byte to one round; the whole grid as device sessions
in lockstep (lzgpu_session_kernel, one diverged lane per session); the
drop-in's DecodeToBuf loops from a thread pool (lzgpu_session_coop_kernel with
the LDS history window).  What the host builds cannot show is checked here:
the lane-strided copy-out, the cooperative window preload, the staging in and
out of LDS, the duplicate lanes of the sliced lane kernel."""
import collections
import ctypes
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import handmade_cases as H
import handmade_stream as S
import native
from test_emu import EMU_VARIANTS

POISON = 0xA5
ERROR_GROUPS = ("rep_first", "edge_unfilled", "edge_full")


# ------------------------------------------------------------------ recorded digests (CPU)

def test_grid_in_the_file_is_the_grid_here():
    g = S.golden()
    assert g["grid"] == {"in_chunks": list(S.IN_CHUNKS), "out_chunks": list(S.OUT_CHUNKS),
                         "small": S.SMALL, "large_min_in": 19, "large_min_out": 272}
    cs = S.cases()
    assert len(cs) == 336 and sum(S.is_small(c) for c in cs) == 246
    assert set(g["cases"]) == {H.key(c, f) for c in cs for f in (0, 1)}
    assert set(g["max_calls"]) == {f"{i},{o}" for i in S.IN_CHUNKS for o in S.OUT_CHUNKS}
    assert max(g["max_calls"].values()) <= S.MAX_ROUNDS


def test_oracle_stream_digests_equal_the_file():
    got, top = S.digests(S.oracle_fn())
    g = S.golden()
    bad = [k for k in g["cases"] if got.get(k) != g["cases"][k]]
    assert not bad, (len(bad), bad[:6])
    assert top == g["max_calls"]


@pytest.mark.skipif(not native.have_ref(), reason="oracle/_ref/libref_lzma.so not built")
def test_live_reference_stream_digests_equal_the_file():
    got, top = S.digests(S.reference_fn())
    g = S.golden()
    bad = [k for k in g["cases"] if got.get(k) != g["cases"][k]]
    assert not bad, (len(bad), bad[:6])
    assert top == g["max_calls"]


# ------------------------------------------------------------------ coverage, from the records

def _ends(c, finish, ic, oc):
    """Cumulative (input, output) position at the end of every call but the last."""
    tr = S.expected()[c["name"], finish, ic, oc][1]
    cum = np.cumsum(tr[:, 2:4], axis=0)[:-1]
    return cum[:, 0].tolist(), cum[:, 1].tolist()


def _case(name):
    return next(c for c in H.lzma_cases() if c["name"] == name)


def _long_overlap(c):
    """The record of the 273-byte match at distance 1 a case ends with."""
    r = c["records"][0][-1]
    assert (r["kind"], r["slot"], r["len_class"]) == ("MA", 0, 2)   # slot 0: distance 1
    assert H.expected(c, 0)[0][2] == c["cap"] == r["pos"] + 273     # the copy runs to the capacity
    return r


def test_cuts_fall_inside_a_273_byte_match_at_distance_1():
    for plp in H.PROPS:
        c = _case("copy distance 1 length 273 to the capacity lc%dlp%dpb%d" % plp)
        r = _long_overlap(c)
        inside = range(r["pos"] + 1, r["pos"] + 273)
        assert S.is_small(c)
        # time slices: a round ends at every multiple of the slice
        assert any(s * k in inside for s in S.slices(c) for k in range(1, c["cap"] // s + 1))
        assert {1, 2, 3, 7, 97, 272}.issubset(S.slices(c))
        # streaming: calls of the expected traces that end inside the copy
        # (272 / 273 / 274: one call that stops short of the copy's end)
        for oc in (1, 2, 13, 272, 273, 274):
            assert any(p in inside for p in _ends(c, 0, 1 << 20, oc)[1]), oc


def test_cuts_fall_on_the_byte_before_an_end_marker():
    late = []
    for plp in H.PROPS:
        c = _case("end marker length 273, three bytes behind, cap+5 lc%dlp%dpb%d" % plp)
        r = c["records"][0][-1]
        assert r["kind"] == "END" and r["pos"] == 20 and S.is_small(c)
        # a call (a round) that holds the last byte and the marker, one that
        # begins at the marker
        assert {r["pos"] - 1, r["pos"]} <= set(S.slices(c))
        outs = _ends(c, 0, 1 << 20, 1)[1]
        assert r["pos"] - 1 in outs and r["pos"] in outs
        assert r["pos"] in _ends(c, 0, 1 << 20, 2)[1]
        # (FINISH_END refuses a full output chunk that does not end the stream:
        # there the cuts come from the input, a byte a call, where the input
        # runs out before the chunk is full)
        outs = _ends(c, 1, 1, 1)[1]
        late.append(r["pos"] - 1 in outs and r["pos"] in outs)
    assert any(late)


def test_cuts_fall_inside_a_hungry_symbol():
    """The byte-hungry cases are large ones (their training prefix is long):
    the grid gives them in_chunk 19, 20 and 21.  An input chunk ends strictly
    inside the bytes the hungry symbol's decisions read at each of the three,
    and an output chunk / a slice ends inside its 273-byte copy and right
    before it; the emu runs below add in_chunk 1, which cuts at every byte."""
    hit_in, hit_out = collections.Counter(), 0
    cs = [c for c in S.cases() if c["group"] == "hungry"]
    assert len(cs) == 72 and not any(S.is_small(c) for c in cs)
    for c in cs:
        rec, k = c["records"][0], c["hungry"]
        first = H.reads_before(rec, k)
        reads = range(first + 1, first + sum(H.hungry_reads(rec, k)))
        for ic in (19, 20, 21):
            if any(p in reads for p in _ends(c, 0, ic, 1 << 20)[0]):
                hit_in[ic] += 1
        if rec[k]["kind"] != "SR":
            pos = rec[k]["pos"]
            assert rec[k + 1]["pos"] == pos + 273
            for oc in (272, 273, 274, 4096):
                hit_out += any(pos < p < pos + 273 for p in _ends(c, 0, 1 << 20, oc)[1])
            assert any(pos < s * (pos // s + 1) < pos + 273 for s in S.slices(c))
    assert min(hit_in[ic] for ic in (19, 20, 21)) >= 3, hit_in
    assert hit_out >= 3


def test_every_group_is_in_the_grid_and_the_ring_wraps():
    small = {c["group"] for c in S.cases() if S.is_small(c)}
    large = {c["group"] for c in S.cases() if not S.is_small(c)}
    # far_direct asks for a 4 GiB ring: time-sliced only (the dictionary is the output)
    assert small | large == set(H.LZMA_GROUPS) - {"far_direct"}
    assert {c["group"] for c in H.lzma_cases()} == set(H.LZMA_GROUPS)
    assert all(len(S.chunkings(c)) == (56 if S.is_small(c) else 20) for c in S.cases())
    wrap = [c for c in S.cases() if c["cap"] > H.DICT and H.expected(c, 0)[0][2] > H.DICT]
    assert {c["group"] for c in wrap} >= {"edge_full", "hungry"}


def _error_rounds(c, finish, slice_):
    """The round (from 0) a time-sliced decode meets the case's data error in."""
    row, _ = H.expected(c, finish)
    assert row[0] == 1
    at = c["records"][0][-1]["pos"]      # the output position of the symbol that fails
    return at // slice_


def test_data_errors_fall_in_later_rounds():
    """The decode-again path of sliced_step (pass 1) with the state of a later
    round: cases of the error groups whose failing symbol lies behind the first
    slice."""
    late = collections.Counter()
    for c in H.lzma_cases():
        if c["group"] in ERROR_GROUPS and c["want"][0] == H.ERR:
            for s in S.slices(c):
                late[c["group"]] += _error_rounds(c, 0, s) >= 1
    assert late["rep_first"] == 0          # its error is the first symbol
    assert late["edge_unfilled"] >= 3 * 49 and late["edge_full"] >= 3 * 2 * 10


# ------------------------------------------------------------------ host builds of the lane code

SLICED_BUILDS = ("default", "session_coop_window_4k", "session_coop_window_uniform_loop")
STREAM_BUILDS = ("default", "session_coop_window_4k")
_EMU = {}


def _emu(variant):
    if variant not in _EMU:
        vdir = os.path.join(tempfile.gettempdir(), "lzgpu_emu_variants")
        os.makedirs(vdir, exist_ok=True)
        out = os.path.join(vdir, f"liblane_emu_resume_{variant}.{os.getpid()}.so")
        subprocess.run(["make", "-s", "-f", "tests/emu/Makefile", f"EMU_OUT={out}",
                        f"EMU_FLAGS={EMU_VARIANTS[variant]}"], cwd=native.ROOT, check=True)
        lib = ctypes.CDLL(out)
        lib.emu_sliced_decode.restype = ctypes.c_int
        lib.emu_sliced_decode.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
                                          ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64,
                                          ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
        S.declare(lib.emu_stream_decode)
        S.declare(lib.emu_stream_decode_dic)
        _EMU[variant] = lib
    return _EMU[variant]


@pytest.mark.parametrize("variant", SLICED_BUILDS)
def test_emu_sliced_every_case_every_slice(variant):
    """sliced_step, the code the round kernels run, in a loop until the stream
    is done: the reference's one-call LzmaDecode result at every slice."""
    lib = _emu(variant)
    row = (ctypes.c_longlong * 4)()
    bad, runs, most = [], 0, 0
    for c in H.lzma_cases():
        src = ctypes.create_string_buffer(c["src"], len(c["src"]) + 32)
        for finish in (0, 1):
            want = H.expected(c, finish)
            for s in S.slices(c):
                dst = ctypes.create_string_buffer(c["cap"] + 1)
                rounds = lib.emu_sliced_decode(c["props"], src, len(c["src"]), dst, c["cap"], s,
                                               finish, row)
                got = tuple(row)
                runs += 1
                most = max(most, rounds)
                if got != want[0] or got[2] > c["cap"] or H.sha(dst.raw[:got[2]]) != want[1] \
                        or rounds > c["cap"] // s + 1 or dst.raw[c["cap"]] != 0:
                    bad.append((c["name"], finish, s, rounds, got, want[0]))
    assert not bad, (len(bad), bad[:6])
    assert runs > 50_000 and most > 5000     # slice 1 on the 5000-literal cases


@pytest.mark.parametrize("device_ring", [True, False])
@pytest.mark.parametrize("variant", STREAM_BUILDS)
def test_emu_streaming_grid(variant, device_ring):
    """The session's DecodeToBuf loop (mode 1, the device ring loop) and the host
    ring loop over DecodeToDic calls (mode 0) over the grid: the recorded
    reference digests.  The 4 KiB window of session_coop_window_4k is the
    smallest the kernel's contract allows."""
    lib = _emu(variant)
    got, top = S.digests(lib.emu_stream_decode if device_ring else lib.emu_stream_decode_dic)
    g = S.golden()
    bad = [k for k in g["cases"] if got.get(k) != g["cases"][k]]
    assert not bad, (len(bad), bad[:6])
    assert top == g["max_calls"]


@pytest.mark.parametrize("variant", STREAM_BUILDS)
def test_emu_streaming_hungry_byte_by_byte(variant):
    """in_chunk 1 on the byte-hungry cases (outside the grid: thousands of calls
    each): the input is cut at every byte of the hungry symbol, so every
    decision of it is met with 0, 1, 2 ... bytes of lookahead in tempBuf."""
    lib, orc = _emu(variant), S.oracle_fn()
    ref = S.reference_fn() if native.have_ref() else None
    bad = []
    for c in S.cases():
        if c["group"] != "hungry" or not any(f"window fill {k} " in c["name"] for k in (8, 3)):
            continue
        for finish, oc in ((0, 273), (1, 1 << 20)):
            want = S.run_bytes(S.run(orc, c, finish, 1, oc))
            if ref is not None:
                assert S.run_bytes(S.run(ref, c, finish, 1, oc)) == want
            for fn in (lib.emu_stream_decode, lib.emu_stream_decode_dic):
                if S.run_bytes(S.run(fn, c, finish, 1, oc)) != want:
                    bad.append((c["name"], finish, oc))
    assert not bad, (len(bad), bad[:6])


def test_form_1_on_a_session_table_does_not_compile():
    """lane_session decodes on a caller's CLzmaDec probabilities, where decision
    form 1's 16-bit update is not exact: a build that turns form 1 on for the
    cooperative kernels (LZGPU_BIT_FORM bit 2) must stop at lane_session's
    static_assert instead of decoding wrong on such tables."""
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-DLZGPU_HOST_EMU", "-DEMU_SESS_COOP_WIN",
           "-Wno-unknown-pragmas", "tests/emu/lane_emu.cpp"]
    ok = subprocess.run(cmd, cwd=native.ROOT, capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr[-2000:]
    r = subprocess.run(cmd + ["-DLZGPU_BIT_FORM=7"], cwd=native.ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "caller-owned probabilities" in r.stderr, r.stderr[-2000:]


# ------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def _gpu(L):
    if L.device_count() <= 0:
        pytest.fail("no HIP device visible: " + L.last_error())


def _dev(buf):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(buf), dtype=np.uint8).copy()).cuda()


def _sliced_run(L, its, slice_, kernel):
    """One time-sliced batch over raw device buffers with a poisoned output.
    Returns (plan, mismatches against the reference's rows)."""
    import torch
    items, src, dst_bytes = H.batch(its)
    descs = L.make_descs(items)
    plan, order = L.plan_sliced(descs, slice_, kernel)
    assert plan.rounds == max(1, -(-max(it["dst_cap"] for it in items) // slice_))
    n = len(items)
    t_src, t_desc, t_ord = _dev(src), _dev(descs), _dev(order)
    t_dst = torch.full((dst_bytes + 64,), POISON, dtype=torch.uint8, device="cuda")
    t_ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device="cuda")
    t_res = torch.full((n * 24,), 0xEE, dtype=torch.uint8, device="cuda")
    r = L.decode_batch_sliced_device(plan, t_desc.data_ptr(), t_ord.data_ptr(), t_src.data_ptr(),
                                     t_dst.data_ptr(), t_ws.data_ptr(), t_res.data_ptr())
    torch.cuda.synchronize()
    assert r == 0, L.last_error()
    res = (L.Result * n).from_buffer_copy(t_res.cpu().numpy().tobytes())
    dst = t_dst.cpu().numpy().tobytes()
    bad = H.mismatches(its, items, res, dst, poison=POISON)
    if dst[dst_bytes:] != bytes([POISON]) * 64:
        bad.append(("wrote behind the last stream",))
    return plan, bad


SLICES_SMALL = (1, 2, 3)                          # on the cases of at most 300 output bytes
SLICES_ALL = (7, 97, 272, 273, 274, 4096, 1 << 30)


def _sliced_sets(plp):
    tag = "lc%dlp%dpb%d" % plp
    cs = [c for c in H.lzma_cases() if c["name"].endswith(tag)]
    assert {c["group"] for c in cs} == set(H.LZMA_GROUPS)
    small = [c for c in cs if c["cap"] <= 300]
    return [(s, H.items(small)) for s in SLICES_SMALL] + [(s, H.items(cs)) for s in SLICES_ALL]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["lane", "coop", "global"])
def test_gpu_sliced_handmade(L, kernel):
    """Per props set and slice one batch of that set's cases (both finish modes,
    16 source alignments) on one round kernel: the reference's one-call rows
    and outputs, nothing written outside a stream's dest_len.  The lane kernel
    runs in both placements (the planner picks by table width)."""
    _gpu(L)
    masks, bad, late = set(), [], 0
    for plp in H.PROPS:
        for slice_, its in _sliced_sets(plp):
            assert max(c["cap"] for c, _, _ in its) <= 300 * slice_ or slice_ >= 7
            plan, b = _sliced_run(L, its, slice_, kernel)
            assert plan.kernel == L.SLICED_KERNELS[kernel]
            masks.add(plan.lds_mask)
            bad += [(plp, slice_) + tuple(x) for x in b]
            # the decode-again path with a later round's state
            late += sum(1 for c, f, _ in its if c["group"] in ERROR_GROUPS and
                        c["want"][f] == H.ERR and _error_rounds(c, f, slice_) >= 1)
    assert not bad, (kernel, len(bad), bad[:8])
    assert late >= 1
    if kernel == "lane":
        assert masks == {0x7FF, 0x200001BF}, [hex(m) for m in masks]


@pytest.mark.gpu
@pytest.mark.parametrize("slice_", [3, 273])
def test_gpu_sliced_handmade_mixed_auto(L, slice_):
    """All three props sets in one batch, the planner's own choice of kernel."""
    _gpu(L)
    cs = [c for c in H.lzma_cases() if slice_ >= 7 or c["cap"] <= 300]
    plan, bad = _sliced_run(L, H.items(cs), slice_, "auto")
    assert not bad, (len(bad), bad[:8])


class _DeviceSessions:
    """Buffers on the GPU (torch), calls through LzmaGpu_SessionDecodeBatch."""

    def __init__(self, L):
        import torch
        self.L, self.torch, self.arr = L, torch, None

    def alloc(self, host):
        t = self.torch.from_numpy(host).cuda()
        return t, t.data_ptr()

    def read(self, t):
        return t.cpu().numpy()

    def call(self, sess):
        torch, m = self.torch, len(sess)
        if self.arr is None:
            self.arr = torch.empty(m * 192, dtype=torch.uint8, device="cuda")   # the first round's
        d = self.arr[:m * 192]
        d.copy_(torch.from_numpy(sess.view(np.uint8)))
        assert self.L.session_decode_batch(d.data_ptr(), m) == 0, self.L.last_error()
        torch.cuda.synchronize()
        return d.cpu().numpy().view(sess.dtype)


class _HostSessions:
    """Buffers in host memory, calls through the emu's emu_session_batch."""

    def __init__(self, lib):
        self.lib = lib
        lib.emu_session_batch.restype = None
        lib.emu_session_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t]

    def alloc(self, host):
        return host, host.ctypes.data

    def read(self, t):
        return t

    def call(self, sess):
        sess = sess.copy()
        self.lib.emu_session_batch(sess.ctypes.data, len(sess))
        return sess


def _sessions_lockstep(L, be, cells, want):
    """Every cell (case, finish, in_chunk, out_chunk) as its own session in mode
    1, all advanced together, one call per session and round (be.call on the
    sessions still running: a session changes its place in the batch from round
    to round).  The probs, dic, src and out buffers are carved out of four
    allocations, the bookkeeping is numpy over a structured view of the session
    array.  Returns the rounds run and the list of sessions whose trace,
    output, input count or untouched output tail differ from `want`, and the
    runs by (case, finish) for the digests."""
    dt = np.dtype(L.Session)
    assert dt.itemsize == 192
    n = len(cells)
    probs_b = np.array([L.session_probs_bytes(c["props"]) for c, _, _, _ in cells], dtype=np.int64)
    assert probs_b.min() > 0
    probs_b = (probs_b + 15) // 16 * 16
    n_src = np.array([len(c["src"]) for c, _, _, _ in cells], dtype=np.int64)
    src_b = (n_src + 16 + 15) // 16 * 16          # the readers load whole 16-byte blocks
    cap = np.array([c["cap"] for c, _, _, _ in cells], dtype=np.int64)
    off = {k: np.concatenate(([0], np.cumsum(v)[:-1])) for k, v in
           (("probs", probs_b), ("src", src_b), ("out", cap))}
    src = np.zeros(int(src_b.sum()), dtype=np.uint8)
    for k, (c, _, _, _) in enumerate(cells):
        src[off["src"][k]:off["src"][k] + n_src[k]] = np.frombuffer(c["src"], dtype=np.uint8)
    t_probs, p_probs = be.alloc(np.zeros(int(probs_b.sum()), dtype=np.uint8))
    t_dic, p_dic = be.alloc(np.zeros(n * H.DICT, dtype=np.uint8))
    t_src, p_src = be.alloc(src)
    t_out, p_out = be.alloc(np.full(int(cap.sum()) + 64, POISON, dtype=np.uint8))
    # LzmaGpu_SessionInit once per props set; the pointers per session
    a, init = np.zeros(n, dtype=dt), {}
    for k, (c, f, _, _) in enumerate(cells):
        if c["props"] not in init:
            r, s = L.session_init(c["props"], 16, 16, H.DICT)
            assert r == 0
            init[c["props"]] = np.frombuffer(bytes(s), dtype=dt)[0]
        a[k] = init[c["props"]]
        a[k]["finish_mode"] = f
    a["probs"] = p_probs + off["probs"]
    a["dic"] = p_dic + np.arange(n, dtype=np.int64) * H.DICT
    a["mode"] = 1
    in_chunk = np.array([i for _, _, i, _ in cells], dtype=np.int64)
    out_chunk = np.array([o for _, _, _, o in cells], dtype=np.int64)
    src0, out0 = p_src + off["src"], p_out + off["out"]
    in_pos, out_pos = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    calls = np.zeros(n, dtype=np.int64)
    room = np.array([w[0] for w in want], dtype=np.int64) + 1    # a row past the expected trace
    row0 = np.concatenate(([0], np.cumsum(room)[:-1]))
    trace = np.full((int(room.sum()), 4), -99, dtype=np.int64)
    live = np.arange(n)
    rounds = 0
    while len(live) and rounds <= S.MAX_ROUNDS:
        q = a[live]
        q["in_"] = src0[live] + in_pos[live]
        q["in_len"] = np.minimum(n_src[live] - in_pos[live], in_chunk[live])
        q["out"] = out0[live] + out_pos[live]
        q["out_len"] = np.minimum(cap[live] - out_pos[live], out_chunk[live])
        got = be.call(q)
        a[live] = got
        rounds += 1
        res, st = got["res"].astype(np.int64), got["status"].astype(np.int64)
        used, made = got["in_used"].astype(np.int64), got["out_len"].astype(np.int64)
        trace[row0[live] + calls[live]] = np.stack([res, st, used, made], axis=1)
        calls[live] += 1
        in_pos[live] += used
        out_pos[live] += made
        done = (res != 0) | (st == 1) | (out_pos[live] == cap[live]) | ((used == 0) & (made == 0))
        live = live[~(done | (calls[live] >= room[live]))]
    out = be.read(t_out)
    bad, runs = [], {}
    for k, (c, f, i, o) in enumerate(cells):
        w = want[k]
        tr = trace[row0[k]:row0[k] + calls[k]]
        at = off["out"][k]
        data = out[at:at + out_pos[k]].tobytes()
        if calls[k] != w[0] or not np.array_equal(tr, w[1]) or data != w[2] or in_pos[k] != w[3]:
            bad.append((c["name"], f, i, o, int(calls[k]), w[0], tr[-2:].tolist(), w[1][-2:].tolist()))
        elif (out[at + out_pos[k]:at + cap[k]] != POISON).any():
            bad.append((c["name"], f, i, o, "wrote behind the output"))
        runs.setdefault(H.key(c, f), []).append((int(calls[k]), tr, data, int(in_pos[k])))
    if (out[int(cap.sum()):] != POISON).any():
        bad.append(("wrote behind the last session's output",))
    return rounds, bad, runs


def _grid_and_want():
    cells, exp = S.grid(), S.expected()
    want = [exp[c["name"], f, i, o] for c, f, i, o in cells]
    top = max(w[0] for w in want)
    assert top == max(S.golden()["max_calls"].values()) and top <= S.MAX_ROUNDS
    return cells, want, top


@pytest.mark.parametrize("variant", STREAM_BUILDS)
def test_emu_sessions_grid_lockstep(L, variant):
    """The lockstep driver of the GPU test below on the host build: the grid as
    sessions in host memory, emu_session_batch in place of the launch."""
    cells, want, top = _grid_and_want()
    rounds, bad, runs = _sessions_lockstep(L, _HostSessions(_emu(variant)), cells, want)
    assert not bad, (len(bad), bad[:6])
    assert rounds == top
    assert {k: S.digest(v) for k, v in runs.items()} == S.golden()["cases"]


@pytest.mark.gpu
def test_gpu_sessions_handmade_grid_lockstep(L):
    """Every (case, finish, in_chunk, out_chunk) of the grid as its own device
    session, all advanced together by LzmaGpu_SessionDecodeBatch in mode 1
    (lzgpu_session_kernel: one lane per session, 64 diverged lanes per
    workgroup).  Each session's trace, output and input count equal the
    oracle's loop, and their digests the recorded reference's; the number of
    rounds is the longest expected loop."""
    _gpu(L)
    cells, want, top = _grid_and_want()
    rounds, bad, runs = _sessions_lockstep(L, _DeviceSessions(L), cells, want)
    assert not bad, (len(bad), bad[:6])
    assert rounds == top and rounds <= S.MAX_ROUNDS
    assert {k: S.digest(v) for k, v in runs.items()} == S.golden()["cases"]


DROPIN_ALL = ((19, 272), (20, 273), (21, 274), (1 << 20, 4096))
DROPIN_SMALL = ((1, 1), (7, 13))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["every case", "small cases"])
def test_gpu_dropin_handmade_streaming_pool(L, which):
    """The drop-in's LzmaDec_DecodeToBuf loops (lzgpu_session_coop_kernel with the
    LDS history window) from 24 threads, whose calls share launches: every case
    and finish mode at the chunkings either side of the tempBuf threshold and
    of the longest match and at the ring's size -- the cases of more than
    4096 output bytes preload the window from a wrapped ring -- and the small
    cases at (1, 1) and (7, 13).  Against the oracle's loop.  Every call is a
    launch: each of the two parts stays under 40,000 calls (36,055 and 33,416
    by the expected traces)."""
    _gpu(L)
    exp, orc = S.expected(), S.oracle_fn()
    if which == "every case":
        jobs = [(c, f, i, o) for c in S.cases() for f in (0, 1) for i, o in DROPIN_ALL]
        assert len(jobs) == 336 * 2 * 4 and any(c["cap"] > H.DICT for c, _, _, _ in jobs)
    else:
        jobs = [(c, f, i, o) for c in S.cases() if S.is_small(c) for f in (0, 1)
                for i, o in DROPIN_SMALL]
        assert len(jobs) == 246 * 2 * 2
    want = [exp[c["name"], f, i, o] if (c["name"], f, i, o) in exp else S.run(orc, c, f, i, o)
            for c, f, i, o in jobs]
    assert sum(w[0] for w in want) <= 40_000

    def run(j):
        c, f, i, o = j
        return L.stream_decode(c["src"], c["props"], c["cap"], i, o, f)

    with ThreadPoolExecutor(24) as ex:
        got = list(ex.map(run, jobs))
    bad = []
    for (c, f, i, o), g, w in zip(jobs, got, want):
        if g[0] != w[0] or [tuple(r) for r in g[1]] != [tuple(r) for r in w[1].tolist()] or \
                g[2] != w[2] or g[3] != w[3]:
            bad.append((c["name"], f, i, o, g[0], w[0], g[1][-2:], w[1][-2:].tolist()))
    assert not bad, (len(bad), bad[:6])

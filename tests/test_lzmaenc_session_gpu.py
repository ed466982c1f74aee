"""LzmaEncGpu_SessionEncodeBatch and the LzmaEnc_* handle drop-ins on the device.
A session's bytes, res and length after its last call are the one-shot
encoder's over the concatenated input, whatever the pieces were: the one-shot
LzmaEncGpu_EncodeBatch of the same process, the live reference where it is
built, the goldens, and for the small special batches the host emulator's
answers (tests/emu_lzmaenc_session).  Nothing has a tolerance."""
import os
import random
import sys

import pytest

import lzmaenc_cases as C
import lzmaenc_opt_cases as O
import lzmaenc_session_cases as S
import native
import test_lzmaenc_gpu as T

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))

pytestmark = pytest.mark.gpu
POISON = 0x3C
N_BATCH = 200     # three full waves at 64 lanes and a partial one


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return S.load_emu(S.build_emu(tmp_path_factory.mktemp("lzmaenc_session_emu")))


def props_of(L, c):
    return L.enc_props(c["level"], c["dict"], c["lc"], c["lp"], c["pb"], c["fb"], c["mc"], c["algo"],
                       c["bt"])


def batch_cases():
    """200 streams of 0 .. 20,000 bytes: text, runs and random bytes with copied
    spans, with the variety of props the mode-0 goldens have."""
    rng = random.Random(20270)
    out = []
    for i in range(N_BATCH):
        lc, lp, pb = rng.choice(((-1, -1, -1), (0, 0, 0), (3, 0, 2), (0, 4, 4), (8, 4, 4), (4, 2, 1)))
        n = rng.choice((0, rng.randrange(0, 600), rng.randrange(0, 20001), rng.randrange(0, 20001)))
        out.append(C.case(rng.choice(("text", "runs", "copy", "random")), 9000 + i, n,
                          level=rng.randrange(5), dict=rng.choice((4096, 5000, 1 << 16)),
                          lc=lc, lp=lp, pb=pb, fb=rng.choice((5, 32, 64, 273)),
                          mc=rng.choice((0, 0, 4)), end_mark=rng.randrange(2)))
    return out


_shared = {}


def batch_reference(L):
    """The batch's inputs and their one-shot streams, computed once: the
    device's own LzmaEncGpu_EncodeBatch, checked against the live reference
    where that is built."""
    if not _shared:
        cases = batch_cases()
        datas = [C.data_of(c) for c in cases]
        items = []
        for c, data in zip(cases, datas):
            r, d, _ = T.desc_of(L, c)
            assert r == 0
            items.append((d, data, C.ample(len(data))))
        want = T.run_device(L, items)
        if native.have_ref():
            for c, data, w in zip(cases, datas, want):
                res, dl, _, out, _, _ = C.ref_expect(c, data)
                assert (res, dl, out) == tuple(w), C.key(c)
        _shared.update(cases=cases, datas=datas, want=want)
    return _shared["cases"], _shared["datas"], _shared["want"]


def slice_sum(sessions, i):
    """A position-weighted checksum of session i's workspace slice."""
    import torch
    lo = sessions.ws_off[i]
    s = sessions.ws[lo:lo + sessions.ws_bytes[i]].to(torch.int64)
    return int((s * (torch.arange(s.numel(), device=s.device) % 65521 + 1)).sum())


def has_work(rec, supplied, finish):
    return not rec.finished and (finish or supplied - rec.in_pos >= S.HOLD)


@pytest.mark.parametrize("lanes", (64, 16, 32))
def test_batch_of_sessions(L, lanes):
    cases, datas, want = batch_reference(L)
    n = len(cases)
    ss = L.LzmaEncSessions(n, 20000, C.ample(20000), end_mark=[c["end_mark"] for c in cases],
                           props=[props_of(L, c) for c in cases], poison=POISON)
    rng = random.Random(77 + lanes)
    out = [b""] * n
    done = [False] * n
    starved_rounds = finished_rounds = 0
    for rnd in range(60):
        finish = []
        for i in range(n):
            if done[i] or rng.random() < 0.3:      # no new bytes this round
                continue
            left = len(datas[i]) - ss.supplied[i]
            piece = min(left, rng.choice((0, 1, 300, 545, 546, 3000, 8000, 20000)))
            ss.append(i, datas[i][ss.supplied[i]:ss.supplied[i] + piece])
            if ss.supplied[i] == len(datas[i]) and rng.random() < 0.7:
                finish.append(i)
        idle = [i for i in range(n) if not has_work(ss.rec[i], ss.supplied[i], i in finish)]
        idle_set = set(idle)
        finished_rounds += sum(1 for i in idle if ss.rec[i].finished)
        starved_rounds += sum(1 for i in idle if not ss.rec[i].finished)
        watch = rng.sample(idle, min(6, len(idle)))
        before = {i: (ss.rec[i].in_pos, ss.rec[i].out_pos, ss.rec[i].needs_init, slice_sum(ss, i))
                  for i in watch}
        assert ss.round(finish=finish, lanes=lanes) == 0, L.last_error()
        assert ss.worked() == n - len(idle)
        for i in watch:                           # a session without work is not touched
            assert before[i] == (ss.rec[i].in_pos, ss.rec[i].out_pos, ss.rec[i].needs_init,
                                 slice_sum(ss, i)), i
        for i in range(n):
            rec = ss.rec[i]
            out[i] += ss.drain(i)
            if rec.finished:
                done[i] = True
            elif i not in idle_set:
                assert rec.status == S.NEEDS_INPUT and ss.supplied[i] - rec.in_pos < S.HOLD, i
        if all(done):
            break
    assert all(done) and starved_rounds > n and finished_rounds > n
    for i in range(n):
        rec = ss.rec[i]
        assert (rec.res, rec.out_pos, out[i]) == tuple(want[i]), (i, C.key(cases[i]))
        assert (rec.status, rec.in_pos) == (S.FINISHED, len(datas[i])), i


def test_sparse_round(L):
    """One session of 200 has work: the compacted count is 1, and so is the
    number of slices initialised."""
    cases, datas, want = batch_reference(L)
    idx = [i for i in range(len(cases)) if len(datas[i]) >= 2000][:N_BATCH]
    pick = idx[len(idx) // 2]
    ss = L.LzmaEncSessions(len(cases), 20000, C.ample(20000),
                           end_mark=[c["end_mark"] for c in cases],
                           props=[props_of(L, c) for c in cases], poison=POISON)
    for i in idx:
        ss.append(i, datas[i][:300])
    assert ss.round() == 0 and ss.worked() == 0
    assert all(ss.rec[i].needs_init == 1 and ss.rec[i].in_pos == 0 for i in range(len(cases)))
    other = next(i for i in idx if i != pick)
    untouched = slice_sum(ss, other)
    ss.append(pick, datas[pick][300:2000])
    assert ss.round() == 0 and ss.worked() == 1
    assert ss.rec[pick].needs_init == 0 and 2000 - S.HOLD < ss.rec[pick].in_pos <= 2000
    assert sum(ss.rec[i].needs_init for i in range(len(cases))) == len(cases) - 1
    assert slice_sum(ss, other) == untouched
    out = ss.drain(pick)
    ss.append(pick, datas[pick][2000:])
    assert ss.round(finish=[pick]) == 0 and ss.worked() == 1
    out += ss.drain(pick)
    assert (ss.rec[pick].res, ss.rec[pick].out_pos, out) == tuple(want[pick])


def run_like_the_emulator(L, emu, c, data, cap, pieces, budget=0):
    """One session on the device and in the emulator, call for call."""
    ss = L.LzmaEncSessions(1, max(len(data), 1), max(cap, 1), end_mark=c["end_mark"],
                           props=props_of(L, c), dst_caps=[cap], poison=POISON)
    h, res, props5 = S.emu_new(emu, c, max(len(data), 1), cap)
    assert h and res == 0 and props5 == ss.props5[0]
    try:
        rec = emu.lzs_record(h).contents
        supplied, out, statuses = 0, b"", []
        for k, piece in enumerate(list(pieces) + [None]):
            last = piece is None
            new = len(data) if last else min(len(data), supplied + piece)
            ss.append(0, data[supplied:new])
            supplied = new
            for _ in range(64):
                emu.lzs_call(h, data, supplied, 1 if last else 0, budget, S.HOLD, 0)
                assert ss.round(finish=[0] if last else [], in_budget=budget) == 0
                g = ss.rec[0]
                assert (g.res, g.status, g.in_pos, g.out_pos, g.finished) == (
                    rec.res, rec.status, rec.in_pos, rec.out_pos, rec.finished), (k, supplied)
                out += ss.drain(0)
                statuses.append(g.status)
                if g.status != S.BUDGET:
                    break
        assert ss.rec[0].finished == 1
        assert out == S.emu_dst(emu, h, min(rec.out_pos, cap))
        before = bytes(ss.rec[0])
        assert ss.round(finish=[0], in_budget=budget) == 0 and ss.worked() == 0
        assert bytes(ss.rec[0]) == before
        return ss.rec[0].res, ss.rec[0].out_pos, out, statuses
    finally:
        emu.lzs_free(h)


def test_overflow_empty_and_end_mark_against_the_emulator(L, emu):
    c = C.case("text", 46, 30000)
    data = C.data_of(c)
    full = L.LzmaEncode(data, props_of(L, c), C.ample(len(data)))
    assert full[0] == 0
    for cap in (0, 4, 5, full[1] - 1, full[1]):
        res, out_pos, out, _ = run_like_the_emulator(L, emu, c, data, cap, [547] * 20 + [12000])
        assert (res, out_pos) == ((0, full[1]) if cap == full[1] else (C.OUTPUT_EOF, cap)), cap
        assert out == full[3][:cap]
    for em in (0, 1):
        c = C.case("text", 100, 0, end_mark=em)            # the empty stream
        res, out_pos, out, _ = run_like_the_emulator(L, emu, c, b"", 64, [0, 0])
        C.check((res, out_pos, b"", out), dict(C.expect(c), props5=b""), C.key(c))
        c = C.case("copy", 14, 3000, lc=0, lp=4, pb=4, end_mark=em)
        data = C.data_of(c)
        res, out_pos, out, _ = run_like_the_emulator(L, emu, c, data, C.ample(3000), [1000, 1, 545])
        one = L.LzmaEncode(data, props_of(L, c), C.ample(3000), end_mark=bool(em))
        assert (res, out_pos, out) == (one[0], one[1], one[3])


@pytest.mark.parametrize("budget", (1, 40000))
def test_budget_against_the_emulator(L, emu, budget):
    c = C.case("text", 45, 100000)
    data = C.data_of(c)
    res, out_pos, out, statuses = run_like_the_emulator(L, emu, c, data, C.ample(len(data)), [],
                                                        budget=budget)
    assert statuses == [S.BUDGET] * (3 if budget == 1 else 1) + [S.FINISHED]
    one = L.LzmaEncode(data, props_of(L, c), C.ample(len(data)))
    assert (res, out_pos, out) == (one[0], one[1], one[3])


# ---------------------------------------------------------------- the LzmaEnc.h drop-ins

def reader(data, step):
    at = [0]

    def read(n):
        b = data[at[0]:at[0] + min(n, step)]
        at[0] += len(b)
        return b
    return read


def test_handle_dropins(L):
    c = C.case("text", 50, 50000)
    data = C.data_of(c)
    props = props_of(L, c)
    one = L.LzmaEncode(data, props, C.ample(len(data)))
    assert one[0] == 0
    for step in (1, 7, 65536):
        got, rounds = [], []
        r, props5 = L.LzmaEnc_Encode(reader(data, step), lambda b: got.append(b) or len(b), props,
                                     progress=lambda a, b: rounds.append((a, b)) or 0)
        assert (r, props5, b"".join(got)) == (0, one[2], one[3]), step
        assert rounds[-1] == (len(data), one[1]) and rounds == sorted(rounds)
        assert len(rounds) > 1 or step == 65536    # small reads are gathered into several rounds
    assert L.LzmaEnc_MemEncode(data, props, C.ample(len(data))) == (0, one[3])
    assert L.LzmaEnc_MemEncode(data, props, 100) == (C.OUTPUT_EOF, one[3][:100])
    # an out stream that takes fewer bytes than it is given; a progress that says stop
    r, _ = L.LzmaEnc_Encode(reader(data, 4096), lambda b: len(b) - 1, props)
    assert r == L.SZ_ERROR_WRITE
    r, _ = L.LzmaEnc_Encode(reader(data, 4096), lambda b: len(b), props, progress=lambda a, b: 1)
    assert r == L.SZ_ERROR_PROGRESS
    # the empty stream, with the end mark from the props
    p = props_of(L, C.case("text", 100, 0))
    p.writeEndMark = 1
    got = []
    assert L.LzmaEnc_Encode(lambda n: b"", lambda b: got.append(b) or len(b), p)[0] == 0
    assert b"".join(got) == L.LzmaEncode(b"", p, 64, end_mark=True)[3]


def test_write_properties_gives_the_goldens_bytes(L):
    golden = C.load_golden()
    seen = set()
    for g in golden["cases"]:
        if g["res"] in (C.PARAM, C.UNSUPPORTED) or g["props5"] in seen:
            continue
        seen.add(g["props5"])
        r, props5 = L.LzmaEnc_Encode(lambda n: b"", lambda b: len(b), props_of(L, g["case"]))
        assert (r, props5.hex()) == (0, g["props5"]), C.key(g["case"])
    assert len(seen) >= 5


def test_normal_mode_props_through_the_handle(L):
    c = O.case("text", 9, 4095, dict=4096)
    data = C.data_of(c)
    props = props_of(L, c)
    prev = L.enc_set_modes(0)
    try:
        got = []
        r, _ = L.LzmaEnc_Encode(reader(data, 1000), lambda b: got.append(b) or len(b), props)
        assert r == C.UNSUPPORTED and not got and "algo" in L.last_error()
        s = L.EncSession()
        L.enc_set_modes(3)        # sessions stay fast-path only whatever the mask says
        assert L.enc_session_init(s, props, 0, 4096, 0, 4096, 0)[0] == C.UNSUPPORTED
        assert "algo" in L.last_error()
        r, props5 = L.LzmaEnc_Encode(reader(data, 1000), lambda b: got.append(b) or len(b), props)
        want = O.expect(c, data, O.load_golden())
        O.check((r, len(b"".join(got)), props5, b"".join(got)), want, O.key(c))
    finally:
        L.enc_set_modes(prev)

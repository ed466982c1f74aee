"""The throughput placement's input reader (GlobalReaderP, lzma_device.h) on the
GPU.

The reader's block fetches and promotions are per lane and EXEC-masked, so the
smallest shape that can go wrong is one wave whose lanes start at every
alignment, end at every residue and promote at different checkpoints: 32
streams (one wave) and 33 (one wave plus one live lane) of <= 2 KiB each on
the throughput instantiation, lane-interleaved rows on and off, lc0/pb0 and
lc3/pb2, every output and result row against the oracle.

The streams are packed so that stream k starts at an offset = k (mod 16), and
their ends cover every residue mod 16.  Among them: plaintexts of 1..20 bytes
(a compressed input shorter than one block, and shorter than two),
incompressible data, 275-byte runs (promotions are rare), hand-written streams
(tests/lzmaenc_min.py) with a match at distance 1 and a short rep directly
after a literal, one whose literals go against trained cells at every level
(several input bytes per literal), a capacity that ends directly behind a literal
under FINISH_ANY, and inputs cut by 1..20 bytes.

Before the GPU run the test traces its inputs with test_fuse_gpu's small
Python decoder and asserts, as conditions, that some lane consumes >= 17 input
bytes inside one pass of the symbol loop and that at some literal of some pass
lanes of one wave cross into a new 16-byte block beside lanes that do not."""
import lzma
import random

import pytest

import lzmaenc_min as E
import native
from test_fuse_gpu import DICT, ILV, LANES, M_THR, _opts, _stream, passes, trace

CUTS = (1, 2, 5, 9, 16, 20)
TINY = (1, 2, 5, 11, 20)


def _raw(data, lc, pb, preset=6):
    return lzma.compress(data, format=lzma.FORMAT_RAW, filters=[
        {"id": lzma.FILTER_LZMA1, "dict_size": DICT, "lc": lc, "lp": 0, "pb": pb,
         "preset": preset}])


def _handmade(lc, pb, seed):
    """A hand-written stream: text literals; a literal, then a match at distance
    1; a literal, then a short rep, then a rep0-long; 300 zero literals, then
    eight 0xFF literals (the root cell against its training); text again.
    Returns (bytes, decoded length, positions directly behind a literal)."""
    rng = random.Random(seed)
    e = E.Encoder(lc, 0, pb)
    alpha = b"etaoinshrdlucmfw"
    for _ in range(40):
        e.literal(rng.choice(alpha))
    e.literal(0x51)
    e.match(1, 6)            # distance 1 directly behind a literal
    e.literal(0x52)
    e.literal(0x53)
    e.match(3, 4)
    e.literal(0x54)
    e.short_rep()            # rep0 = 3, directly behind a literal
    e.literal(0x55)
    e.match(1, 2)
    e.literal(0x56)
    e.rep(0, 3)              # rep0-long at distance 1 behind a literal
    for _ in range(300):
        e.literal(0)
    for _ in range(8):
        e.literal(0xFF)
    after_lit = []
    for _ in range(120):
        e.literal(rng.choice(alpha))
        after_lit.append(e.total)
    e.match(7, 9)
    for _ in range(60):
        e.literal(rng.choice(alpha))
    return e.finish(), e.total, after_lit


def _hungry(lc, pb, x=0xB4, reps=90):
    """Literals only: each node on x's path through the plain literal tree is
    trained against x's bit there -- the deepest first, by the byte that shares
    x's bits above the node and differs at it --, then x eight times in one
    literal run of the symbol loop (the run starts at the stream's start, the
    x's at a multiple of 8): several input bytes per literal."""
    e = E.Encoder(lc, 0, pb)
    keep = x ^ 1  # under lc > 0: a previous byte with x's top bits
    for k in reversed(range(8)):
        y = x ^ (1 << (7 - k))
        for _ in range(reps):
            if lc and k < lc:
                e.literal(keep)  # (its own context is y's, not x's)
            e.literal(y)
    if lc:
        e.literal(keep)
    while e.total % 8:
        e.literal(x ^ 0x80 if not lc else keep)
    assert e.total % 8 == 0
    for _ in range(8):
        e.literal(x)
    rng = random.Random(x)
    for _ in range(100):
        e.literal(rng.choice(b"etaoinshrdlucmfw"))
    return e.finish(), e.total


def _comps(lc, pb):
    """33 (compressed bytes, source bytes offered, capacity, finish mode)."""
    rng = random.Random(7100 + lc * 10 + pb)
    out = []
    # plaintexts of 1..20 bytes
    for n in TINY:
        data = bytes(rng.randrange(97, 123) for _ in range(n))
        raw = _raw(data, lc, pb)
        out.append((raw, len(raw), n, 1))
    # incompressible data
    for n in (600, 1100, 1500, 1800, 2000, 2048):
        data = bytes(rng.randrange(256) for _ in range(n))
        raw = _raw(data, lc, pb)
        out.append((raw, len(raw), n, 1))
    # 275-byte runs
    for k in range(4):
        data = b"".join(bytes([65 + (k * 5 + j) % 26]) * 275 + b"z " for j in range(3 + k))
        raw = _raw(data, lc, pb, preset=1)
        out.append((raw, len(raw), len(data), 1))
    # hand-written: whole, and with the capacity directly behind a literal
    raw, total, after_lit = _handmade(lc, pb, 50)
    out.append((raw, len(raw), total, 0))
    raw, total = _hungry(lc, pb)
    out.append((raw, len(raw), total, 0))
    for k in range(2):
        raw, total, after_lit = _handmade(lc, pb, 60 + k)
        out.append((raw, len(raw), after_lit[17 + 40 * k], 0))
    # inputs cut by 1..20 bytes
    for k, t in enumerate(CUTS):
        n = rng.randrange(1200, 2049)
        raw = _raw(_stream(9100 + 31 * k + lc, n, k == 3), lc, pb, preset=rng.choice([1, 6]))
        out.append((raw, len(raw) - t, n, k & 1))
    # text with planted repeats; the lengths are settled by batch()
    while len(out) < 33:
        k = len(out)
        out.append((None, rng.randrange(1300, 2000), 9200 + 17 * k + lc, k % 5 == 0))
    return out


_SETS = {}


def batch(lc, pb):
    """(items, src, dst bytes, oracle rows, traces) of the 33 streams, once."""
    if (lc, pb) in _SETS:
        return _SETS[lc, pb]
    props = bytes([pb * 45 + lc]) + DICT.to_bytes(4, "little")
    comps = _comps(lc, pb)
    # the text streams' plaintext lengths are chosen so that, with the others,
    # the inputs' ends cover every residue mod 16 within the first 32 streams
    items, chunks, off, doff = [], [], 0, 0
    want_ends = set(range(16))
    full = []
    for k, c in enumerate(comps):
        start = off + (k - off) % 16  # = k (mod 16)
        if c[0] is None:
            _, n, seed, long_run = c
            have = {(it["src_off"] + it["src_len"]) % 16 for it in items}
            missing = sorted(want_ends - have)
            for dn in range(64):
                raw = _raw(_stream(seed, n + dn, long_run), lc, pb)
                if not missing or (start + len(raw)) % 16 in missing:
                    break
            c = (raw, len(raw), n + dn, 1)
        raw, src_len, cap, fin = c
        chunks.append(b"\xA5" * (start - off) + raw)
        items.append(dict(src_off=start, src_len=src_len, dst_off=doff, dst_cap=cap, props=props,
                          finish=fin))
        full.append((raw[:src_len], cap, fin))
        off = start + len(raw)
        doff += cap
    src = b"".join(chunks) + b"\0" * 16
    orc = native.oracle()
    exp = [native.decode(orc, "orc", raw, props, cap, fin) for raw, cap, fin in full]
    traces = []
    for (raw, cap, fin), e in zip(full, exp):
        out, syms = trace(raw, lc, pb, cap, DICT)
        assert out[:e[2]] == e[4], len(traces)  # the tracer agrees with the oracle
        traces.append((syms, len(raw)))
    _SETS[lc, pb] = (items, src, doff, exp, traces)
    return _SETS[lc, pb]


def conditions(L, lc, pb, n, ilv):
    """What the inputs must be for the test to mean anything; all on the CPU."""
    items, src, dst_bytes, exp, traces = batch(lc, pb)
    items, exp, traces = items[:n], exp[:n], traces[:n]
    plan, order = L.plan_ex(L.make_descs(items), _opts(L, ilv))
    assert plan.n_lds == n and plan.n_classes == 1
    c = plan.classes[0]
    assert c.lds_mask == M_THR | (ILV if ilv else 0) and c.lanes_per_group == LANES
    # starts at every alignment, ends at every residue
    assert all(it["src_off"] % 16 == k % 16 for k, it in enumerate(items))
    assert {(it["src_off"] + it["src_len"]) % 16 for it in items[:32]} == set(range(16))
    # inputs shorter than one block and shorter than two
    lens = [it["src_len"] for it in items[:len(TINY)]]
    assert min(lens) < 16 and any(16 <= x < 32 for x in lens), lens
    # a match at distance 1, a short rep and a rep0-long directly behind a literal
    after = set()
    for syms, _ in traces:
        for a, b in zip(syms, syms[1:]):
            if a[0] in ("L", "ML"):
                after.add(("MA", b[2]) if b[0] == "MA" else b[0] if b[0] == "SR" else None)
    assert ("MA", 0) in after and "SR" in after, after
    # the capacity ends directly behind a literal under FINISH_ANY
    cut = [k for k, (it, (syms, _)) in enumerate(zip(items, traces))
           if it["finish"] == 0 and syms and syms[-1][0] == "L" and exp[k][2] == it["dst_cap"]
           and exp[k][1] == 2]
    assert len(cut) >= 2, cut
    # some lane consumes >= 17 input bytes inside one pass
    most = 0
    for syms, in_len in traces:
        ps = passes(syms, in_len)
        firsts = [(p[0][0] if p[0] else p[1])[-1] for p in ps]
        most = max([most] + [b - a for a, b in zip(firsts, firsts[1:])])
    assert most >= 17, most
    # some literal of some pass: lanes of one wave enter a new 16-byte block
    # beside lanes that stay in theirs
    mixed = 0
    order = list(order)
    for w in range(0, n, LANES):
        lanes = []
        for k in range(w, min(w + LANES, n)):
            i = order[k]
            syms, in_len = traces[i]
            at = [s[-1] for s in syms] + [in_len]
            nxt = {s[-1]: at[j + 1] for j, s in enumerate(syms)}
            lanes.append((items[i]["src_off"], passes(syms, in_len), nxt))
        for p in range(max(len(x[1]) for x in lanes)):
            for j in range(8):
                cross = set()
                for so, ps, nxt in lanes:
                    if p < len(ps) and j < len(ps[p][0]):
                        a = ps[p][0][j][-1]
                        cross.add((so + a) // 16 != (so + nxt[a]) // 16)
                mixed += cross == {True, False}
    assert mixed >= 10, mixed
    return True


@pytest.mark.parametrize("props", [(0, 0), (3, 2)])
def test_inputs_are_what_they_claim(props):
    """The conditions, on the CPU with the oracle and the planner alone."""
    import lzmagpu as L
    for n in (32, 33):
        for ilv in (True, False):
            assert conditions(L, props[0], props[1], n, ilv)
    # the cut inputs: the oracle's srcLen stays within what was offered
    items, src, dst_bytes, exp, traces = batch(*props)
    k0 = len(TINY) + 6 + 4 + 4
    for k in range(k0, k0 + len(CUTS)):
        assert exp[k][3] <= items[k]["src_len"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32, 33])
@pytest.mark.parametrize("ilv", [True, False])
@pytest.mark.parametrize("props", [(0, 0), (3, 2)])
def test_reader_bit_exact(props, ilv, n):
    import lzmagpu as L
    if L.device_count() <= 0:
        pytest.fail("no HIP device visible: " + L.last_error())
    lc, pb = props
    assert conditions(L, lc, pb, n, ilv)
    items, src, dst_bytes, exp, traces = batch(lc, pb)
    items, exp = items[:n], exp[:n]
    plan = L.Plan()
    r, res, dst = L.decode_batch_host(L.make_descs(items), src, dst_bytes, _opts(L, ilv), plan)
    assert r == 0, L.last_error()
    assert plan.n_classes == 1 and plan.classes[0].lds_mask == M_THR | (ILV if ilv else 0)
    assert plan.classes[0].lanes_per_group == LANES
    bad = []
    for k, e in enumerate(exp):
        got = (res[k].res, res[k].status, res[k].dest_len, res[k].src_len)
        out = dst[items[k]["dst_off"]:items[k]["dst_off"] + res[k].dest_len]
        if got != tuple(e[:4]) or out != e[4]:
            bad.append((k, got, e[:4]))
    assert not bad, (props, ilv, n, len(bad), bad[:6])

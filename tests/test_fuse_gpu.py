"""Fused tree walks (LZGPU_FUSE, lzma_device.h) on the GPU.

A fusion only does anything when lanes of one wave sit in different classes of
a pair at the same pass of the symbol loop (length low / mid, SpecPos / Align,
matched / plain literal), so the smallest shape that can go wrong is one wave
of streams that disagree.  Two waves (64 streams) and one wave plus a single
live lane (33 streams) of <= 2 KiB each run on the throughput instantiation,
lane-interleaved rows on and off, lc0/pb0 and lc3/pb2, and every stream's
output and result row is compared with the oracle.

Before the GPU run the test traces its own inputs with a small Python decoder
and asserts, as a condition, that the batch holds every class and that some
wave holds both classes of each pair in the same pass."""
import lzma
import random

import pytest

import golden_cases as G
import native

ILV, PLAN_NO_ILV = 0x40000000, 16
M_THR = 0x105
DICT = 1 << 22  # slots up to 43
LANES = 32


# ------------------------------------------------------------------ inputs

def _stream(seed, n, long_run=False):
    """Seeded text with planted repeats: copies of earlier spans at chosen
    distances and lengths (every length class, every distance-slot class a
    2 KiB stream reaches), some with one byte changed (a matched literal, then
    rep0 again), copies alternating between a few sources (rep1..rep3), and
    short-period runs (distances 1..4).  long_run: a run of 275 equal bytes --
    a literal, a match of the longest length (273) and one byte left over,
    which the encoder's fast mode writes as a literal: a matched literal that
    equals its match byte at every level."""
    rng = random.Random(seed)
    words = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randrange(2, 9)))
             for _ in range(40)]
    out = bytearray()
    while len(out) < 160:
        out += rng.choice(words) + b" "
    srcs = []  # recent copy distances, reused for rep1..rep3
    run_at = rng.randrange(300, 900) if long_run else n
    while len(out) < n:
        if len(out) >= run_at:
            out += b"Q" * 275 + b"z "
            run_at = n
        k = rng.randrange(10)
        if k < 2:
            for _ in range(rng.randrange(1, 6)):
                out += rng.choice(words) + b" "
        elif k == 2:
            out += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 5)))
        elif k == 3:
            per = rng.randrange(1, 5)
            unit = bytes(rng.randrange(97, 123) for _ in range(per))
            out += unit * rng.randrange(2, 12)
        else:
            if srcs and rng.random() < 0.45:
                dist = rng.choice(srcs)
            else:
                # distances spread over the slot classes: 5..127 (SpecPos, 1..5
                # bits) and 128.. (direct bits + Align)
                hi = len(out) - 1
                dist = rng.choice([rng.randrange(5, 9), rng.randrange(8, 16), rng.randrange(16, 32),
                                   rng.randrange(32, 64), rng.randrange(64, 128),
                                   rng.randrange(128, 256), rng.randrange(256, max(257, hi))])
            dist = min(dist, len(out))
            ln = rng.choice([2, 3, 4, 5, 7, 9, 10, 12, 15, 17, 18, 25, 40, 70])
            at = len(out) - dist
            # (a copy longer than its distance repeats the period)
            seg = bytearray((bytes(out[at:]) * (ln // dist + 1))[:ln])
            if ln >= 5 and rng.random() < 0.5:
                # one changed byte inside the copy: the bit flipped decides the
                # level at which the matched literal leaves the match byte
                seg[rng.randrange(1, ln - 1)] ^= 1 << rng.randrange(8)
            out += seg
            srcs = ([dist] + srcs)[:3]
    return bytes(out[:n])


def _inputs(lc, pb, n_streams):
    """(items, src bytes, dst bytes, per-stream compressed inputs, props)."""
    props = bytes([pb * 45 + lc]) + DICT.to_bytes(4, "little")
    comps = []
    rng = random.Random(4000 + lc * 10 + pb)
    for i in range(n_streams - 2):
        n = rng.randrange(1500, 2049)
        long_run = i % 8 == 3
        filt = [{"id": lzma.FILTER_LZMA1, "dict_size": DICT, "lc": lc, "lp": 0, "pb": pb,
                 "preset": 1 if long_run else rng.choice([1, 6, 6, 9])}]
        raw = lzma.compress(_stream(9000 + 97 * i + lc, n, long_run), format=lzma.FORMAT_RAW,
                            filters=filt)
        cap, fin = n, 1
        if i % 8 == 5:
            # liblzma's raw stream has no end marker: FINISH_ANY into a short
            # capacity stops inside a match
            cap, fin = n - rng.randrange(1, 40), 0
        comps.append((raw, props, cap, fin))
    # the end marker: the same kind of stream from the encoder's .lzma (alone)
    # container, which writes one when the size field says "unknown"
    alone = lzma.compress(_stream(8999, 1800), format=lzma.FORMAT_ALONE, filters=[
        {"id": lzma.FILTER_LZMA1, "dict_size": DICT, "lc": lc, "lp": 0, "pb": pb}])
    assert alone[5:13] == b"\xff" * 8
    comps.append((alone[13:], props, 1800 + 50, 1))
    # a stream ending in SZ_ERROR_DATA, distance beyond the dictionary: the
    # reference-recorded golden (lc3/pb2), else a far repeat under props that
    # declare a 4 KiB dictionary
    if (lc, pb) == (3, 2):
        d = G.load()
        c = next(c for i, c in G.cases("lzma") if c["note"] == "dict 4096 with far distances")
        assert c["expect"]["res"] == 1 and bytes.fromhex(c["props"])[0] == 0x5D
        comps.append((G.case_input(d, c), bytes.fromhex(c["props"]), c["dest_cap"], c["finish"]))
    else:
        rr = random.Random(5)
        head = bytes(rr.randrange(256) for _ in range(300))
        far = head + bytes(rr.randrange(97, 101) for _ in range(4400)) + head
        raw = lzma.compress(far, format=lzma.FORMAT_RAW, filters=[
            {"id": lzma.FILTER_LZMA1, "dict_size": DICT, "lc": lc, "lp": 0, "pb": pb}])
        comps.append((raw, bytes([pb * 45 + lc]) + (4096).to_bytes(4, "little"), len(far), 1))
    items, srcs, off, doff = [], [], 0, 0
    for raw, pr, cap, fin in comps:
        items.append(dict(src_off=off, src_len=len(raw), dst_off=doff, dst_cap=cap, props=pr,
                          finish=fin))
        srcs.append(raw)
        off += len(raw)
        doff += cap
    return items, b"".join(srcs) + b"\0" * 16, doff, comps


# ------------------------------------------------------------------ the tracer

def trace(buf, lc, pb, cap, dict_size):
    """Plain-Python LZMA decode of one stream (lp = 0): per symbol
    (kind, detail..., input bytes consumed before it), kinds
      L            plain literal
      ML  k        matched literal, first mismatch at level k (8: none)
      SR           short rep
      REP r c      rep r (0 = rep0-long, 1..3), length class c (0 low, 1 mid, 2 high)
      MA  c slot   match, length class c, distance slot
      END / ERR    end marker / data error (distance beyond what was written)"""
    pos = [5]
    st = [0xFFFFFFFF, int.from_bytes(buf[1:5], "big")]
    probs = {}

    def norm():
        if st[0] < (1 << 24):
            st[0] = (st[0] << 8) & 0xFFFFFFFF
            st[1] = ((st[1] << 8) | (buf[pos[0]] if pos[0] < len(buf) else 0)) & 0xFFFFFFFF
            pos[0] += 1

    def bit(key):
        p = probs.get(key, 1024)
        norm()
        b = (st[0] >> 11) * p
        if st[1] < b:
            st[0] = b
            probs[key] = p + ((2048 - p) >> 5)
            return 0
        st[0] -= b
        st[1] -= b
        probs[key] = p - (p >> 5)
        return 1

    def direct():
        norm()
        st[0] >>= 1
        if st[1] >= st[0]:
            st[1] -= st[0]
            return 1
        return 0

    def tree(pre, bits):
        m = 1
        for _ in range(bits):
            m = (m << 1) | bit((pre, m))
        return m - (1 << bits)

    out = bytearray()
    state, reps, syms = 0, [1, 1, 1, 1], []
    pbm = (1 << pb) - 1
    while len(out) < cap and pos[0] <= len(buf) + 4:
        at = pos[0]
        ps = len(out) & pbm
        if not bit(("M", state, ps)):
            ctx = (out[-1] >> (8 - lc)) if out else 0
            if state < 7:
                sym = 0x100 | tree(("L", ctx), 8)
                syms.append(("L", at))
            else:
                mb, offs, sym, lvl = out[-reps[0]], 0x100, 1, 8
                for k in range(8):
                    mb <<= 1
                    mbit = mb & offs
                    b = bit(("L", ctx, offs + mbit + sym)) if offs else bit((("L", ctx), sym))
                    sym = (sym << 1) | b
                    if offs and (mbit != 0) != (b != 0):
                        lvl = k
                    offs = (offs & mbit) if b else (offs & ~mbit)
                syms.append(("ML", lvl, at))
            out.append(sym & 0xFF)
            state = 0 if state < 4 else (state - 3 if state < 10 else state - 6)
            continue
        if bit(("R", state)):
            if not out:
                syms.append(("ERR", at))
                break
            rk = 0
            if not bit(("G0", state)):
                if not bit(("R0L", state, ps)):
                    state = 9 if state < 7 else 11
                    out.append(out[-reps[0]])
                    syms.append(("SR", at))
                    continue
            else:
                if not bit(("G1", state)):
                    d, rk = reps[1], 1
                else:
                    if not bit(("G2", state)):
                        d, rk = reps[2], 2
                    else:
                        d, rk = reps[3], 3
                        reps[3] = reps[2]
                    reps[2] = reps[1]
                reps[1] = reps[0]
                reps[0] = d
            lk, kind = "RL", "REP"
            state = 8 if state < 7 else 11
        else:
            lk, kind = "LL", "MA"
            state = 7 if state < 7 else 10
        if not bit((lk, "c")):
            ln, lcl = tree((lk, "lo", ps), 3), 0
        elif not bit((lk, "c2")):
            ln, lcl = 8 + tree((lk, "mid", ps), 3), 1
        else:
            ln, lcl = 16 + tree((lk, "hi"), 8), 2
        if kind == "MA":
            slot = tree(("S", min(ln, 3)), 6)
            if slot < 4:
                d = slot
            else:
                nb = (slot >> 1) - 1
                d = (2 | (slot & 1)) << nb
                if slot < 14:
                    m = 1
                    for k in range(nb):
                        b = bit(("SP", d - slot, m))
                        m = (m << 1) | b
                        d |= b << k
                else:
                    v = 0
                    for k in range(nb - 4):
                        v = (v << 1) | direct()
                    d += v << 4
                    m = 1
                    for k in range(4):
                        b = bit(("A", m))
                        m = (m << 1) | b
                        d |= b << k
                    if d == 0xFFFFFFFF:
                        syms.append(("END", at))
                        break
            reps[3], reps[2], reps[1], reps[0] = reps[2], reps[1], reps[0], d + 1
            if d >= len(out) or d >= dict_size:
                syms.append(("ERR", at))
                break
            syms.append(("MA", lcl, slot, at))
        else:
            syms.append(("REP", rk, lcl, at))
        for _ in range(ln + 2):
            if len(out) >= cap:
                break
            out.append(out[-reps[0]])
    return bytes(out), syms


def passes(syms, in_len):
    """The symbol loop's passes of one lane: up to 8 literals, then the match
    the literal run ended at.  A lane's progress per pass does not depend on
    its neighbours.  Only the bulk pass (input well before the last 20 bytes)."""
    res, i = [], 0
    while i < len(syms) and syms[i][-1] < in_len - 32:
        lits = []
        while i < len(syms) and len(lits) < 8 and syms[i][0] in ("L", "ML"):
            lits.append(syms[i])
            i += 1
        m = None
        if len(lits) < 8 and i < len(syms):
            m = syms[i]
            i += 1
        res.append((lits, m))
    return res


def coverage(traces, order, n):
    """Classes present in the batch, and class pairs that meet in one pass of
    one wave (lanes = consecutive streams of the planner's order)."""
    have, pairs = set(), set()
    for syms, _ in traces:
        for s in syms:
            if s[0] == "ML":
                have.add(("ML", s[1]))
            elif s[0] == "REP":
                have.add(("REP", s[1]))
                have.add(("LEN", s[2]))
            elif s[0] == "MA":
                have.add(("LEN", s[1]))
                sl = s[2]
                have.add(("SLOT", "lt4" if sl < 4 else ("ge14" if sl >= 14 else (sl >> 1) - 1)))
            else:
                have.add((s[0],))
    for w in range(0, n, LANES):
        lanes = [passes(*traces[order[k]]) for k in range(w, min(w + LANES, n))]
        for p in range(max(len(x) for x in lanes)):
            cur = [x[p] for x in lanes if p < len(x)]
            first = {x[0][0][0] for x in cur if x[0]}
            if {"L", "ML"} <= first:
                pairs.add("literal matched+plain")
            ms = [x[1] for x in cur if x[1] is not None]
            lens = {m[2] if m[0] == "REP" else m[1] for m in ms if m[0] in ("REP", "MA")}
            if {0, 1} <= lens:
                pairs.add("length low+mid")
            if {0, 1, 2} <= lens:
                pairs.add("length low+mid+high")
            tails = {("spec" if m[2] < 14 else "align") for m in ms if m[0] == "MA" and m[2] >= 4}
            if {"spec", "align"} <= tails:
                pairs.add("tail SpecPos+Align")
            nb = {(m[2] >> 1) - 1 for m in ms if m[0] == "MA" and 4 <= m[2] < 14}
            if len(nb) >= 2 and min(nb) < 3 <= max(nb):
                pairs.add("SpecPos bit counts below and from 3")
            if len({m[2] >> 1 for m in ms if m[0] == "MA" and m[2] >= 14}) >= 2:
                pairs.add("direct-bit counts differ")
            reps = {m[1] for m in ms if m[0] == "REP"} | {"SR" for m in ms if m[0] == "SR"}
            if (0 in reps or "SR" in reps) and reps & {1, 2, 3}:
                pairs.add("rep0 + rep1..3")
    return have, pairs


WANT = ({("L",), ("SR",), ("END",), ("ERR",)} | {("ML", k) for k in range(9)} |
        {("REP", r) for r in range(4)} | {("LEN", c) for c in range(3)} |
        {("SLOT", "lt4"), ("SLOT", "ge14")} | {("SLOT", b) for b in range(1, 6)})
WANT_PAIRS = {"literal matched+plain", "length low+mid", "length low+mid+high",
              "tail SpecPos+Align", "SpecPos bit counts below and from 3",
              "direct-bit counts differ", "rep0 + rep1..3"}

_SETS = {}


def batch(lc, pb, n):
    """Inputs, the oracle's results and the traces: once per (props, size)."""
    key = (lc, pb, n)
    if key not in _SETS:
        items, src, dst_bytes, comps = _inputs(lc, pb, n)
        orc = native.oracle()
        exp = [native.decode(orc, "orc", raw, pr, cap, fin) for raw, pr, cap, fin in comps]
        traces = []
        for (raw, pr, cap, fin), e in zip(comps, exp):
            out, syms = trace(raw, lc, pb, cap, int.from_bytes(pr[1:5], "little"))
            # the tracer agrees with the oracle on what was decoded
            assert out[:e[2]] == e[4], len(traces)
            traces.append((syms, len(raw)))
        _SETS[key] = (items, src, dst_bytes, exp, traces)
    return _SETS[key]


def _opts(L, ilv):
    return L.plan_options("throughput", cus=8, persistent=2, lanes_per_group=LANES,
                          flags=0 if ilv else PLAN_NO_ILV)


def check_coverage(L, lc, pb, n, ilv):
    items, src, dst_bytes, exp, traces = batch(lc, pb, n)
    plan, order = L.plan_ex(L.make_descs(items), _opts(L, ilv))
    assert plan.n_lds == n and plan.n_classes == 1
    c = plan.classes[0]
    assert c.lds_mask == M_THR | (ILV if ilv else 0) and c.lanes_per_group == LANES, \
        (hex(c.lds_mask), c.lanes_per_group)
    have, pairs = coverage(traces, list(order), n)
    return have, pairs


@pytest.mark.parametrize("props", [(0, 0), (3, 2)])
def test_inputs_cover_every_class_and_pair(props):
    """The coverage condition, on the CPU with the oracle alone: the planner
    (host code) gives the lane order, nothing runs on a device."""
    import lzmagpu as L
    for ilv in (True, False):
        have, pairs = check_coverage(L, props[0], props[1], 64, ilv)
        assert WANT <= have, sorted(WANT - have, key=str)
        assert WANT_PAIRS <= pairs, sorted(WANT_PAIRS - pairs)
    # the 33-stream batch: its second wave has one live lane
    batch(props[0], props[1], 33)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 33])
@pytest.mark.parametrize("ilv", [True, False])
@pytest.mark.parametrize("props", [(0, 0), (3, 2)])
def test_fused_walks_bit_exact(props, ilv, n):
    import lzmagpu as L
    if L.device_count() <= 0:
        pytest.fail("no HIP device visible: " + L.last_error())
    lc, pb = props
    items, src, dst_bytes, exp, traces = batch(lc, pb, n)
    if n == 64:
        have, pairs = check_coverage(L, lc, pb, n, ilv)
        assert WANT <= have and WANT_PAIRS <= pairs, (WANT - have, WANT_PAIRS - pairs)
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


# ------------------------------------------------------------------ hand-made neighbours

_HAND = {}


def handmade_wave(lc, pb, n):
    """n lanes made only of hand-made cases (tests/handmade_cases.py) under
    lc / lp0 / pb: lanes that decode 5,000 bytes beside lanes that end in a
    data error at once, at the dictionary edge or at the capacity, lanes that
    end at an end marker of each length, and symbols against fully trained
    contexts.  Returns (H, [(case, finish, None)], descs, src, dst bytes)."""
    if (lc, pb, n) not in _HAND:
        import handmade_cases as H
        tag = f" lc{lc}lp0pb{pb}"
        by = {c["name"]: c for c in H.lzma_cases()}
        pick = [(f"5000 literals, distance index {i}", 1) for i in (4094, 4095, 4096, 5000)]
        pick += [("5000 literals, index 4095 then rep0-long", 1)]
        pick += [(f"end marker length {ln}, three bytes behind, cap+0", f)
                 for ln in H.MARKER_LENS for f in (0, 1)]
        pick += [(f"first symbol {k}", 0) for k in ("rep0", "rep1", "rep2", "rep3", "short rep")]
        pick += [("50 literals, distance index 49", 1), ("50 literals, distance index 50", 1),
                 ("length 273 over the capacity", 0), ("length 273 over the capacity", 1),
                 ("matched literals, every state and level", 1), ("state walk", 0),
                 ("reps on initial values", 1), ("hungry rep3 at window fill 1", 1),
                 ("hungry match at window fill 4", 0), ("hungry short_rep at window fill 8", 1),
                 ("copy distance 1 length 273 to the capacity", 1),
                 ("copy distance 3 length 17 one over the capacity", 1),
                 ("copy distance 17 length 273 one over the capacity", 0),
                 ("copy distance 8 length 2 to the capacity", 0),
                 ("capacity 0, stream not empty", 1)]
        assert len(pick) == 33
        # the long lanes spread among the short ones
        pick = pick[5:5 + (n - 5) // 2] + pick[:5] + pick[5 + (n - 5) // 2:n]
        its = [(by[name + tag], f, None) for name, f in pick]
        _HAND[lc, pb, n] = (H, its) + H.batch(its)
    return _HAND[lc, pb, n]


@pytest.mark.parametrize("props", [(0, 0), (3, 2)])
def test_handmade_wave_is_what_it_claims(props):
    """On the CPU: one class of 32 lanes per group in both row layouts, and in
    it lanes of 5,000 bytes, error lanes and end-marker lanes."""
    import lzmagpu as L
    for n in (32, 33):
        H, its, items, src, dst_bytes = handmade_wave(props[0], props[1], n)
        assert len(its) == n
        rows = [H.expected(c, f)[0] for c, f, _ in its]
        assert sum(1 for r in rows if r[0] == 0 and r[2] >= 5000) >= 3
        assert sum(1 for r in rows if r[0] == 1) >= 10
        assert sum(1 for r in rows if r[:2] == (0, 1)) >= 4
        for ilv in (True, False):
            plan, order = L.plan_ex(L.make_descs(items), _opts(L, ilv))
            assert plan.n_lds == n and plan.n_classes == 1
            c = plan.classes[0]
            assert c.lds_mask == M_THR | (ILV if ilv else 0) and c.lanes_per_group == LANES


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32, 33])
@pytest.mark.parametrize("ilv", [True, False])
@pytest.mark.parametrize("props", [(0, 0), (3, 2)])
def test_fused_walks_handmade_neighbours(props, ilv, n):
    """One wave of 32 and a batch of 33 (a second wave with one live lane) of
    hand-made cases on the throughput instantiation: lanes that stop at once
    beside lanes that go on for 5,000 bytes, every row and byte against the
    reference's."""
    import lzmagpu as L
    if L.device_count() <= 0:
        pytest.fail("no HIP device visible: " + L.last_error())
    H, its, items, src, dst_bytes = handmade_wave(props[0], props[1], n)
    plan = L.Plan()
    r, res, dst = L.decode_batch_host(L.make_descs(items), src, dst_bytes, _opts(L, ilv), plan)
    assert r == 0, L.last_error()
    assert plan.n_classes == 1 and plan.classes[0].lds_mask == M_THR | (ILV if ilv else 0)
    assert plan.classes[0].lanes_per_group == LANES
    bad = H.mismatches(its, items, res, dst)
    assert not bad, (props, ilv, n, len(bad), bad[:6])

"""Inputs of the match-path tests (LZGPU_MP, lzma_device.h): streams written
symbol by symbol (tests/lzmaenc_min.py), so that every class the match path's
load batches tell apart stands in the batch and lanes of different classes meet
in one pass of a wave.

A stream is at most 2 KiB of input.  Most decode to under 2 KiB; the "far"
streams decode to 4.5 KiB of a four-letter alphabet, because a distance with
six or seven direct bits lies 2,049 to 8,192 bytes back.  (The format has no
slot with one direct bit: slots 14 and 15 have two, then one more per pair.)

The conditions (coverage) are asserted on a trace of the finished inputs by
the small Python decoder of tests/test_fuse_gpu.py, lengths taken from the
encoder's own record after the two were checked to agree symbol by symbol."""
import random

import lzmaenc_min as E
import native
from test_fuse_gpu import trace

DICT = 1 << 22
LANES = 32
# LenHigh symbols 0, 7 | 8, 63 | 64, 255: the first and the last leaf below
# tree8_g's three load batches
HIGH_EDGES = (18, 25, 26, 81, 82, 273)
SHORT_LENS = (2, 3, 4, 5, 6, 9)
MID_LENS = (10, 12, 17)
ALPHA = b"etaoinshrdlucmfw"


def _dist_of_class(rng, total):
    """A distance (1-based) of a random slot class that `total` bytes allow."""
    top = min(total, 2040)
    classes = [(1, 4), (5, 6), (7, 8), (9, 16), (17, 32), (33, 64), (65, 128), (129, 256),
               (257, 512), (513, 1024), (1025, 2048)]
    ok = [(a, min(b, top)) for a, b in classes if a <= top]
    a, b = rng.choice(ok)
    return rng.randrange(a, b + 1)


def _symbol(e, rng, lens, room):
    """One random symbol; lens: the lengths still to be planted, popped first."""
    k = rng.randrange(12)
    if k < 3 or e.total < 8:
        for _ in range(rng.randrange(1, 5)):
            e.literal(rng.choice(ALPHA))
            e.record[-1]["ln"] = 1
        return
    if k == 3:
        e.short_rep()
        e.record[-1]["ln"] = 1
        return
    if lens and rng.random() < 0.5:
        ln = lens.pop()
    else:
        ln = rng.choice(SHORT_LENS + SHORT_LENS + MID_LENS + (18, 30))
    ln = max(2, min(ln, room))
    if k < 7:
        e.rep(rng.randrange(4), ln)
    else:
        e.match(_dist_of_class(rng, e.total), ln)
    e.record[-1]["ln"] = ln


def _body(lc, pb, seed, target, lens=()):
    rng = random.Random(seed)
    e = E.Encoder(lc, 0, pb)
    for _ in range(rng.randrange(6, 14)):
        e.literal(rng.choice(ALPHA))
        e.record[-1]["ln"] = 1
    lens = list(lens)
    rng.shuffle(lens)
    while e.total < target or lens:
        _symbol(e, rng, lens, 273)
    return e, rng


def _far(lc, pb, seed):
    """4,400 literals of four letters, then matches and reps at distances whose
    slots have 1 to 7 direct bits (slots 14..24)."""
    rng = random.Random(seed)
    e = E.Encoder(lc, 0, pb)
    for _ in range(4400):
        e.literal(rng.choice(b"acgt"))
        e.record[-1]["ln"] = 1
    for slot in list(range(14, 25)) + [24, 23, 22]:
        nb = (slot >> 1) - 1
        lo = (2 | (slot & 1)) << nb
        idx = rng.randrange(lo, min(lo + (1 << nb), e.total - 1))
        ln = rng.choice((2, 3, 5, 11, 18))
        e.raw_match(idx, ln)
        e.record[-1]["ln"] = ln
        e.literal(rng.choice(b"acgt"))
        e.record[-1]["ln"] = 1
    return e, rng


def streams(lc, pb, n):
    """n streams as (src, props, cap, finish, record, tag); the last four are
    the far stream, the end-marker stream, the truncated one and the data
    error."""
    props = E.props(lc, 0, pb, DICT)
    out = []
    for i in range(n - 4):
        lens = []
        if i % 4 == 0:
            lens = list(HIGH_EDGES) + list(HIGH_EDGES)  # for matches and reps alike
        e, _ = _body(lc, pb, 7000 + 31 * i + lc, 700 + 90 * (i % 9), lens)
        out.append((e.finish(), props, e.total, 1, e.record, "body"))
    e, _ = _far(lc, pb, 7901)
    out.append((e.finish(), props, e.total, 1, e.record, "far"))
    # the end marker (Align all ones) with FINISH_END and room behind it
    e, _ = _body(lc, pb, 7902, 900)
    e.end_marker(3)
    e.record[-1]["ln"] = 3
    out.append((e.finish(), props, e.total + 50, 1, e.record, "end"))
    # cut inside a match's direct bits: the encoder's record says after which
    # decision it shifted a byte out, and the decoder reads that byte before
    # the next decision (it has read 5 + shifts bytes).  The input ends one
    # byte before a read that stands between two direct bits.
    e, _ = _far(lc, pb, 7903)
    src = e.finish()
    pick = None
    for k, r in enumerate(e.record):
        used = 0
        for j, (key, _b, sh) in enumerate(r["dec"]):
            used += sh
            if (r["kind"] == "MA" and sh and key == ("D",) and j + 1 < len(r["dec"])
                    and r["dec"][j + 1][0] == ("D",)):
                pick = (k, 5 + r["at"] + used - 1)
    assert pick is not None
    out.append((src[:pick[1]], props, e.total, 1, e.record[:pick[0]], "cut"))
    # a distance beyond the bytes written, seven direct bits
    e, rng = _body(lc, pb, 7904, 600)
    e.raw_match(4096 + 77, 5, model=False)
    e.record[-1]["ln"] = 5
    out.append((e.finish(), props, e.total + 20, 1, e.record, "error"))
    assert len(out) == n
    return out


def symbols(src, lc, pb, cap, record):
    """The decoder's view of one stream: trace() symbols with the length added
    from the encoder's record, ('MA', class, slot, len, at) / ('REP', r, class,
    len, at), checked kind by kind against it."""
    _, syms = trace(src, lc, pb, cap, DICT)
    res = []
    for s, r in zip(syms, record):
        kind = {"L": "L", "ML": "ML", "SR": "SR", "REP": "REP", "MA": "MA", "END": "END",
                "ERR": "MA"}[s[0]]
        assert kind == r["kind"], (s, r["kind"])
        if s[0] == "MA":
            assert (s[1], s[2]) == (r["len_class"], r["slot"])
            res.append(("MA", s[1], s[2], r["ln"], s[-1]))
        elif s[0] == "REP":
            assert (s[1], s[2]) == (r["rep"], r["len_class"])
            res.append(("REP", s[1], s[2], r["ln"], s[-1]))
        else:
            res.append(s)
    return res


def passes(syms, in_len):
    """A lane's passes of the symbol loop in the bulk pass (test_fuse_gpu)."""
    res, i = [], 0
    while i < len(syms) and syms[i][-1] < in_len - 32:
        lits = 0
        while i < len(syms) and lits < 8 and syms[i][0] in ("L", "ML"):
            lits += 1
            i += 1
        m = None
        if lits < 8 and i < len(syms):
            m = syms[i]
            i += 1
        res.append(m)
    return res


WANT = ({("END",), ("ERR",), ("SR",), ("SLOT", "lt4")} |
        {("MA", c) for c in range(3)} | {("REP", c) for c in range(3)} |
        {("HIGH", ln) for ln in HIGH_EDGES} | {("SPEC", b) for b in range(1, 6)} |
        {("DIRECT", b) for b in range(2, 8)})
WANT_PAIRS = {"choice 0+1", "LenHigh+short", "SpecPos+Align", "rep+match", "length <=4 + longer"}


def coverage(all_syms, in_lens, order):
    """(classes in the batch, class pairs met in one pass of one wave); lanes
    are consecutive streams of the planner's order."""
    have, pairs = set(), set()
    for syms in all_syms:
        for s in syms:
            if s[0] in ("MA", "REP"):
                have.add((s[0], s[2] if s[0] == "REP" else s[1]))
                if s[3] in HIGH_EDGES:
                    have.add(("HIGH", s[3]))
            if s[0] == "MA":
                sl = s[2]
                have.add(("SLOT", "lt4") if sl < 4 else
                         ("SPEC", (sl >> 1) - 1) if sl < 14 else ("DIRECT", (sl >> 1) - 5))
            elif s[0] in ("END", "ERR", "SR"):
                have.add((s[0],))
    n = len(order)
    for w in range(0, n, LANES):
        lanes = [passes(all_syms[order[k]], in_lens[order[k]]) for k in range(w, min(w + LANES, n))]
        for p in range(max(len(x) for x in lanes)):
            ms = [x[p] for x in lanes if p < len(x) and x[p] is not None and x[p][0] in ("MA", "REP")]
            cls = {m[1] if m[0] == "MA" else m[2] for m in ms}
            if 0 in cls and cls & {1, 2}:
                pairs.add("choice 0+1")
            if 2 in cls and cls & {0, 1}:
                pairs.add("LenHigh+short")
            slots = [m[2] for m in ms if m[0] == "MA"]
            if any(4 <= s < 14 for s in slots) and any(s >= 14 for s in slots):
                pairs.add("SpecPos+Align")
            if {m[0] for m in ms} == {"MA", "REP"}:
                pairs.add("rep+match")
            mlen = [m[3] for m in ms if m[0] == "MA"]
            if mlen and min(mlen) <= 4 < max(mlen):
                pairs.add("length <=4 + longer")
    return have, pairs


_SETS = {}


def batch(lc, pb, n):
    """(items, src, dst bytes, oracle results, symbols per stream, input
    lengths): once per (props, size)."""
    key = (lc, pb, n)
    if key not in _SETS:
        ss = streams(lc, pb, n)
        orc = native.oracle()
        items, srcs, exp, syms, off, doff = [], [], [], [], 0, 0
        for src, pr, cap, fin, rec, tag in ss:
            assert len(src) <= 2048, (tag, len(src))
            items.append(dict(src_off=off, src_len=len(src), dst_off=doff, dst_cap=cap, props=pr,
                              finish=fin))
            srcs.append(src)
            off += len(src)
            doff += cap
            exp.append(native.decode(orc, "orc", src, pr, cap, fin))
            syms.append(symbols(src, lc, pb, cap, rec))
        tags = [s[5] for s in ss]
        # the special streams end as they were built to
        e = {t: exp[tags.index(t)] for t in ("end", "cut", "error")}
        assert e["end"][:2] == (0, 1), e["end"][:4]       # FINISHED_WITH_MARK
        assert e["cut"][1] == 3, e["cut"][:4]             # NEEDS_MORE_INPUT
        assert e["error"][0] == 1, e["error"][:4]         # SZ_ERROR_DATA
        _SETS[key] = (items, b"".join(srcs) + b"\0" * 16, doff, exp, syms,
                      [len(s[0]) for s in ss])
    return _SETS[key]

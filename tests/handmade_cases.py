"""Hand-made LZMA and LZMA2 streams: the decoder corners no encoder emits.

Every other decoder test sees streams a well-behaved encoder wrote (the
reference's LzmaEnc, liblzma, the fast-mode encoder), cut or bit-flipped at
random.  The streams here are written symbol by symbol (tests/lzmaenc_min.py)
so that a chosen symbol stands at a chosen spot: a rep before any output, a
distance exactly at the dictionary edge, an end marker of any length with bytes
behind it, LZMA2 chunks that change lc / lp / pb, continue after a stored
chunk, pad their pack size, overrun their unpack size or hold an end marker,
and symbols that go against fully trained contexts at every decision they can.

The list is deterministic and seeded; nothing is stored but results.  A case
is a dict: name, kind ("lzma" / "lzma2"), group (the class of corner it was
built for), src, props (5 bytes) or prop (the LZMA2 property byte), cap, want
(per finish mode the class the reference's answer must fall in: "ok" decodes,
"error" a data error, "more" needs more input -- this guards the construction,
not the decoder), records (the encoders' own record of what they wrote: the
coverage conditions read it) and, for the byte-hungry set, hungry (the index of
the symbol in records[0]).  Every case runs with FINISH_ANY and FINISH_END.

Expected results come from the live reference (oracle/_ref/libref_lzma.so)
where it is built, else from tests/golden/handmade_cases.json, written by
tests/golden/make_golden_handmade.py."""
import hashlib
import json
import os
import random

import lzmaenc_min as E
import native

GOLDEN = os.path.join(native.ROOT, "tests", "golden", "handmade_cases.json")
PROPS = ((0, 0, 0), (3, 0, 2), (0, 4, 4))
DICT = 4096
ALPHA = b"etaoinshrdlucmfw"   # 16 letters: a literal costs about four bits
OVERLAP_DISTS = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17)
OVERLAP_LENS = (2, 17, 273)
MARKER_LENS = (2, 3, 18, 273)
# decisions that take a cell to one extreme from the other: 2017 * (31/32)^k
# falls below 64 after 109 of them, then by one a decision down to 31
TRAIN = 170
# Bytes the range coder shifts out over five consecutive decisions, at most:
# a decision against a cell at its extreme (31 / 2048) narrows the range by
# 6.05 bits and five of them by 30.2, which leaves room for four shifts of
# eight bits but not five (the first would need a range below 2^22.25 after
# normalisation).  Found on the generator alone (max_window over the hungry
# set) and asserted in tests/test_handmade.py.
HUNGRY_WINDOW = 4
LZMA_GROUPS = ("rep_first", "reps_initial", "edge_unfilled", "edge_full", "end_marker",
               "len273_over_cap", "far_direct", "matched_literals", "state_walk", "overlap",
               "empties", "hungry")
LZMA2_GROUPS = ("props_change", "after_stored", "missing_props", "bad_first", "stored_only",
                "bad_prop_byte", "padded_pack", "unpack_size", "marker_in_chunk",
                "edge_after_stored")
OK, ERR, MORE = "ok", "error", "more"


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def answer_class(res, status):
    """LzmaDecode reports an input that ends early as SZ_ERROR_INPUT_EOF (6)
    with NEEDS_MORE_INPUT; the LZMA2 loop as SZ_OK with it."""
    if status == 3 and res in (0, 6):
        return MORE
    return ERR if res != 0 else OK


def _case(name, group, e, cap, want, dict_size=DICT, tail=b"", src=None, **kw):
    lc, lp, pb = kw.pop("plp", (e.lc, e.lp, e.pb))
    c = dict(name=f"{name} lc{lc}lp{lp}pb{pb}", kind="lzma", group=group,
             src=(e.finish() if src is None else src) + tail,
             props=E.props(lc, lp, pb, dict_size), cap=cap,
             want=want if isinstance(want, dict) else {0: want, 1: want}, records=[e.record])
    c.update(kw)
    return c


def _lits(e, rng, n, alpha=ALPHA):
    for _ in range(n):
        e.literal(rng.choice(alpha))


# ------------------------------------------------------------------ LZMA cases

def _rep_first(plp):
    out = []
    for k in range(5):
        e = E.Encoder(*plp)
        if k < 4:
            e.rep(k, 2, model=False)
        else:
            e.short_rep(model=False)
        out.append(_case(f"first symbol {'rep%d' % k if k < 4 else 'short rep'}", "rep_first",
                         e, 10, ERR))
    return out


def _reps_initial(plp):
    rng = random.Random(11)
    e = E.Encoder(*plp)
    e.literal(0x41)
    e.short_rep()
    e.rep(1, 3)
    e.rep(3, 4)
    e.rep(2, 5)
    _lits(e, rng, 10)
    return [_case("reps on initial values", "reps_initial", e, e.total, OK)]


def _edge_unfilled(plp):
    out = []
    for idx, want in ((49, OK), (50, ERR)):
        rng = random.Random(12)
        e = E.Encoder(*plp)
        _lits(e, rng, 50)
        e.raw_match(idx, 5, model=want == OK)
        if want == OK:
            _lits(e, rng, 5)
        out.append(_case(f"50 literals, distance index {idx}", "edge_unfilled", e, 60, want))
    return out


def _edge_full(plp):
    rng = random.Random(13)
    base = E.Encoder(*plp)
    _lits(base, rng, 5000)
    out = []
    for idx, want in ((4094, OK), (4095, OK), (4096, ERR), (5000, ERR)):
        e = base.fork()
        e.raw_match(idx, 4, model=want == OK)
        if want == OK:
            _lits(e, rng, 6)
        out.append(_case(f"5000 literals, distance index {idx}", "edge_full", e, 5010, want))
    e = base.fork()
    e.match(4096, 3)
    e.literal(0x5A)
    e.rep(0, 5)
    _lits(e, rng, 4)
    out.append(_case("5000 literals, index 4095 then rep0-long", "edge_full", e, e.total, OK))
    return out


def _end_marker(plp):
    out = []
    for ln in MARKER_LENS:
        for extra in (0, 5):
            rng = random.Random(14)
            e = E.Encoder(*plp)
            _lits(e, rng, 20)
            e.end_marker(ln)
            out.append(_case(f"end marker length {ln}, three bytes behind, cap+{extra}",
                             "end_marker", e, 20 + extra, OK, tail=b"\x55\xaa\x33"))
    return out


def _len273_over_cap(plp):
    rng = random.Random(15)
    e = E.Encoder(*plp)
    _lits(e, rng, 10)
    e.match(1, 273)
    return [_case("length 273 over the capacity", "len273_over_cap", e, 100, {0: OK, 1: ERR})]


def _far_direct(plp):
    out = []
    for idx in (0x80000000, 0xFFFFFFFE, 0x4000005):
        rng = random.Random(16)
        e = E.Encoder(*plp)
        _lits(e, rng, 30)
        e.raw_match(idx, 4, model=False)
        out.append(_case(f"distance index {idx:#x}, 26 direct bits", "far_direct", e, 64, ERR,
                         dict_size=0xFFFFFFFF))
    return out


def _reach(e, rng, state):
    """From a literal state to `state` (7..11), by the shortest way."""
    d = rng.randrange(1, min(e.total, 30) + 1)
    if state in (7, 10, 11):
        e.match(d, 2)
    if state == 10:
        e.match(rng.randrange(1, min(e.total, 30) + 1), 3)
    if state in (8, 11):
        e.rep(0, 2)
    if state == 9:
        e.short_rep()
    assert e.state == state


def _matched_literals(plp):
    """In each of states 7 to 11 a literal that equals its match byte at all
    eight levels, and one that leaves it at each level 0 to 7."""
    rng = random.Random(17)
    e = E.Encoder(*plp)
    _lits(e, rng, 12, alpha=bytes(range(256)))
    for state in range(7, 12):
        for level in range(9):
            while e.state >= 7 or rng.random() < 0.5:
                e.literal(rng.randrange(256))
            _reach(e, rng, state)
            mb = e.back(e.reps[0])
            low = rng.randrange(0x80 >> level) if level < 8 else 0
            e.literal(mb if level == 8 else (mb ^ (0x80 >> level)) & ~((0x80 >> level) - 1) | low)
            assert e.record[-1]["level"] == level and e.record[-1]["state"] == state
    return [_case("matched literals, every state and level", "matched_literals", e, e.total, OK)]


def _state_walk(plp):
    """Every state 0..11 before a literal, a match, a rep and a short rep."""
    rng = random.Random(18)
    e = E.Encoder(*plp)
    _lits(e, rng, 8)
    seen = set()
    while len(seen) < 48:
        s = e.state
        todo = [k for k in "LMRS" if (s, k) not in seen]
        k = rng.choice(todo) if todo and rng.random() < 0.7 else rng.choice("LLMRS")
        seen.add((s, k))
        if k == "L":
            e.literal(rng.choice(ALPHA))
        elif k == "M":
            e.match(rng.randrange(1, min(e.total, 200) + 1), rng.choice((2, 3, 9, 12, 20)))
        elif k == "R":
            e.rep(rng.randrange(4), rng.choice((2, 5, 11, 19)))
        else:
            e.short_rep()
    _lits(e, rng, 3)
    return [_case("state walk", "state_walk", e, e.total, OK)]


def _overlap(plp):
    out = []
    for d in OVERLAP_DISTS:
        for ln in OVERLAP_LENS:
            rng = random.Random(19)
            e = E.Encoder(*plp)
            _lits(e, rng, 20)
            e.match(d, ln)
            src = e.finish()
            # the copy ends exactly at the capacity / runs one byte over it
            out.append(_case(f"copy distance {d} length {ln} to the capacity", "overlap", e,
                             20 + ln, OK, src=src))
            out.append(_case(f"copy distance {d} length {ln} one over the capacity", "overlap", e,
                             20 + ln - 1, {0: OK, 1: ERR}, src=src))
    return out


def _empties(plp):
    rng = random.Random(20)
    e = E.Encoder(*plp)
    _lits(e, rng, 5)
    src = e.finish()
    empty = E.Encoder(*plp)
    return [_case("capacity 0, stream not empty", "empties", e, 0, {0: OK, 1: ERR}, src=src),
            _case("empty stream, capacity 0", "empties", empty, 0, OK, src=bytes(5)),
            _case("empty stream, capacity 1", "empties", empty, 1, MORE, src=bytes(5)),
            _case("first byte not 0", "empties", e, 5, ERR, src=b"\x01" + src[1:])]


# -- byte-hungry symbols

def _train(e, period, n, sym):
    """n rounds: sym in state 0 at a multiple of `period` (posState 0 and the
    same literal position every time), then zero literals back to state 0."""
    for _ in range(n):
        assert e.state == 0 and e.total % period == 0
        sym(e)
        while e.total % period or e.state != 0:
            e.literal(0)


def decisions(record, first=0, last=None):
    """(key, bit, bytes shifted out) of symbols first..last-1, in order."""
    return [d for r in record[first:last] for d in r["dec"]]


def max_window(ns, width=5):
    return max((sum(ns[i:i + width]) for i in range(max(len(ns) - width + 1, 1))), default=0)


def reads_before(record, k):
    """Input bytes the DECODER has read when it begins symbol k: the five of
    the range coder's start and one per byte shifted out, less the byte the
    last decision shifted out (the decoder normalises before a decision, the
    encoder after it)."""
    prev = record[k - 1]["dec"][-1][2] if k else 0
    return 5 + record[k]["at"] - prev


def hungry_reads(record, k):
    """Bytes the decoder reads at each decision of symbol k."""
    prev = record[k - 1]["dec"][-1][2] if k else 0
    return [prev] + [d[2] for d in record[k]["dec"]][:-1]


def window_fill(record, k):
    """Bytes left in a reader's eight-byte window when symbol k begins, for a
    window that started full at the stream's first byte: 8 down to 1."""
    return 8 - reads_before(record, k) % 8


def _hungry_base(plp, variant):
    """The training prefix: every cell the hungry symbol will decide on is
    taken to the extreme the symbol goes against.  A cell below another in the
    decision order is trained first: training IsRepG1 also feeds IsRepG0 ones,
    which the next phase then takes back to zeros (a cell forgets at 1/32 per
    decision)."""
    rng = random.Random(21)
    # of the cells the symbols go against only IsMatch (retrained at every
    # posState by the literals at the end) and the short rep's IsRep0Long are
    # cells per posState: the short rep and its training stay at posState 0
    period = (1 << plp[2]) if variant == "short_rep" else 1
    e = E.Encoder(*plp)
    _lits(e, rng, 304)
    n = TRAIN
    if variant == "rep3":
        for d in (1, 2, 3, 5):              # four distances of their own
            _train(e, period, 1, lambda e, d=d: e.match(d, 2))
        for k in (2, 1, 0):                 # IsRepG2, IsRepG1 to 0; IsRepG0 to 0
            _train(e, period, n, lambda e, k=k: e.rep(k, 2))
        _train(e, period, n, lambda e: e.match(1, 2))           # IsRep to 0
    elif variant == "match":
        _train(e, period, n, lambda e: e.match(1, 18))          # LenHigh and slot paths to 0
        _train(e, period, n, lambda e: e.match(1, 10))          # LenChoice2 to 0
        _train(e, period, n, lambda e: e.match(1, 2))           # LenChoice to 0
        _train(e, period, n, lambda e: e.rep(0, 2))             # IsRep to 1
    else:
        _train(e, period, n, lambda e: e.rep(0, 2))             # IsRep0Long to 1
        _train(e, period, n, lambda e: e.rep(1, 2))             # IsRepG0 to 1
        _train(e, period, n, lambda e: e.match(1, 2))           # IsRep to 0
    for _ in range(n << plp[2]):                                # IsMatch to 0, every posState
        e.literal(0)
    return e


def _hungry_symbol(e, variant):
    if variant == "rep3":
        e.rep(3, 273)           # IsMatch, IsRep, IsRepG0, IsRepG1, IsRepG2, LenChoice against
    elif variant == "match":
        e.raw_match(293, 273)   # IsMatch, IsRep, LenChoice, LenChoice2, LenHigh, slot against
    else:
        e.short_rep()           # IsMatch, IsRep, IsRepG0, IsRep0Long against


def _hungry(plp):
    """For each variant one stream per window fill 8..1: zero literals (a fifth
    of a bit each) behind the training move the range and the input position
    until the hungry symbol begins at that fill and its decisions shift out
    HUNGRY_WINDOW bytes within five."""
    out = []
    for variant in ("rep3", "match", "short_rep"):
        e = _hungry_base(plp, variant)
        # (a short rep has four decisions: its window of five holds three bytes)
        need = HUNGRY_WINDOW - (variant == "short_rep")
        # IsRep0Long is a cell per posState, trained at posState 0 only
        step = (1 << plp[2]) if variant == "short_rep" else 1
        found = {}
        for _ in range(1200):
            t = e.fork(tail=512)     # a try-out: the symbol reaches back 294 bytes at most
            _hungry_symbol(t, variant)
            fill = window_fill(t.record, 1)
            if fill not in found and max_window(hungry_reads(t.record, 1)) == need:
                t = e.fork()
                _hungry_symbol(t, variant)
                k = len(t.record) - 1
                assert window_fill(t.record, k) == fill
                found[fill] = (t, k)
                if len(found) == 8:
                    break
            for _ in range(step):
                e.literal(0)
        for fill in sorted(found):
            t, k = found[fill]
            _lits(t, random.Random(22), 5)
            out.append(_case(f"hungry {variant} at window fill {fill}", "hungry", t, t.total, OK,
                             hungry=k))
    return out


_BUILDERS = (_rep_first, _reps_initial, _edge_unfilled, _edge_full, _end_marker, _len273_over_cap,
             _far_direct, _matched_literals, _state_walk, _overlap, _empties, _hungry)


# ------------------------------------------------------------------ LZMA2 cases

def prop_byte(lc, lp, pb):
    return (pb * 5 + lp) * 9 + lc


def _case2(name, group, src, cap, want, records=(), prop=0):
    return dict(name=name, kind="lzma2", group=group, src=bytes(src), prop=prop, cap=cap,
                want=want if isinstance(want, dict) else {0: want, 1: want},
                records=list(records))


def _props_change():
    rng = random.Random(31)
    e = E.Encoder(3, 0, 2)
    src, start = b"", 0
    for control, plp in ((0xE0, (3, 0, 2)), (0xC0, (0, 2, 0)), (0xC0, (4, 0, 4))):
        e.reset_state()
        e.set_props(*plp)
        if start:
            e.match(start - 3, 9)       # reaches back across the chunk border
        _lits(e, rng, 40)
        e.match(min(e.total, 45), 12)
        src += E.lz_chunk(control, e.restart_rc(), e.total - start, prop_byte(*plp))
        start = e.total
    src += b"\0"
    return [_case2("three chunks, three props, exact capacity", "props_change", src, e.total, OK,
                   [e.record]),
            _case2("three chunks, three props, capacity 5 short", "props_change", src,
                   e.total - 5, {0: OK, 1: ERR}, [e.record])]


def _after_stored():
    rng = random.Random(32)
    e = E.Encoder(3, 0, 2)
    _lits(e, rng, 30)
    e.match(7, 6)
    src = E.lz_chunk(0xE0, e.restart_rc(), e.total, prop_byte(3, 0, 2))
    raw = bytes(rng.choice(ALPHA) for _ in range(20))
    e.stored(raw)
    src += E.copy_chunk(2, raw)
    start = e.total
    e.rep(0, 5)                         # rep0 = 7, into the stored bytes; state and reps kept
    _lits(e, rng, 3)
    e.rep(1, 4)
    e.match(40, 8)
    _lits(e, rng, 4)
    src += E.lz_chunk(0x80, e.restart_rc(), e.total - start) + b"\0"
    return [_case2("0xE0, stored 0x02, then 0x80 beginning with rep0-long", "after_stored", src,
                   e.total, OK, [e.record])]


def _missing_props():
    rng = random.Random(33)
    raw = bytes(rng.choice(ALPHA) for _ in range(16))
    e = E.Encoder(3, 0, 2)
    e.stored(raw)
    _lits(e, rng, 10)
    src = E.copy_chunk(1, raw) + E.lz_chunk(0xA0, e.restart_rc(), 10) + b"\0"
    # the same behind a chunk that did bring props: the 0x01 chunk's dictionary
    # reset asks for new ones (without the first chunk a decoder that forgets
    # this still refuses, for want of any props at all)
    f = E.Encoder(3, 0, 2)
    _lits(f, rng, 12)
    first = E.lz_chunk(0xE0, f.restart_rc(), 12, prop_byte(3, 0, 2))
    f.reset_state()
    f.stored(raw)
    _lits(f, rng, 10)
    again = first + E.copy_chunk(1, raw) + E.lz_chunk(0xA0, f.restart_rc(), 10) + b"\0"
    return [_case2("stored 0x01 then 0xA0 without props", "missing_props", src, 26, ERR),
            _case2("0xE0, stored 0x01, then 0xA0 without props", "missing_props", again, 38, ERR,
                   [f.record])]


def _bad_first():
    rng = random.Random(34)
    out = []
    for control in (0x80, 0xC0):
        e = E.Encoder(3, 0, 2)
        _lits(e, rng, 10)
        src = E.lz_chunk(control, e.restart_rc(), 10,
                         prop_byte(3, 0, 2) if control == 0xC0 else None) + b"\0"
        out.append(_case2(f"first chunk {control:#x}", "bad_first", src, 10, ERR))
    raw = bytes(rng.choice(ALPHA) for _ in range(12))
    out.append(_case2("first chunk 0x02", "bad_first", E.copy_chunk(2, raw) + b"\0", 12, ERR))
    out.append(_case2("control byte 3", "bad_first", E.copy_chunk(3, raw) + b"\0", 12, ERR))
    return out


def _stored_only():
    rng = random.Random(35)
    a = bytes(rng.choice(ALPHA) for _ in range(33))
    b = bytes(rng.choice(ALPHA) for _ in range(17))
    two = E.copy_chunk(1, a) + E.copy_chunk(2, b)
    return [_case2("stored 0x01 then 0x02, end byte", "stored_only", two + b"\0", 50, OK),
            _case2("stored 0x01 then 0x02, no end byte", "stored_only", two, 50, {0: OK, 1: MORE}),
            _case2("stored chunk longer than the capacity", "stored_only", two + b"\0", 20,
                   {0: OK, 1: ERR}),
            _case2("stored chunk cut by the end of the input", "stored_only", two[:-6], 50, MORE)]


def _bad_prop_byte():
    rng = random.Random(36)
    out = []
    for pbyte, what in ((prop_byte(3, 2, 0), "lc + lp = 5"), (225, "225")):
        e = E.Encoder(3, 0, 2)
        _lits(e, rng, 10)
        src = E.lz_chunk(0xE0, e.restart_rc(), 10, pbyte) + b"\0"
        out.append(_case2(f"chunk props byte {what}", "bad_prop_byte", src, 10, ERR))
    return out


def _padded_pack():
    rng = random.Random(37)
    e = E.Encoder(3, 0, 2)
    _lits(e, rng, 30)
    e.match(7, 6)
    data = e.restart_rc()
    src = E.lz_chunk(0xE0, data + bytes(3), e.total, prop_byte(3, 0, 2)) + b"\0"
    # FINISH_ANY stops at an exact capacity before it looks at the padding
    return [_case2("pack size three bytes more than the coder used", "padded_pack", src, e.total,
                   {0: OK, 1: ERR}, [e.record]),
            _case2("pack size three bytes more than the coder used, cap+5", "padded_pack", src,
                   e.total + 5, ERR, [e.record])]


def _unpack_size():
    rng = random.Random(38)
    e = E.Encoder(3, 0, 2)
    _lits(e, rng, 30)
    e.match(7, 10)
    data = e.restart_rc()
    over = E.lz_chunk(0xE0, data, e.total - 3, prop_byte(3, 0, 2)) + b"\0"
    under = E.lz_chunk(0xE0, data, e.total + 5, prop_byte(3, 0, 2)) + b"\0"
    return [_case2("match overruns the chunk's unpack size", "unpack_size", over, e.total, ERR,
                   [e.record]),
            # the chunk's pack bytes run out first: the LZMA decoder asks for more
            _case2("unpack size larger than the data gives", "unpack_size", under, e.total + 5,
                   MORE, [e.record])]


def _marker_in_chunk():
    rng = random.Random(39)
    e = E.Encoder(3, 0, 2)
    _lits(e, rng, 30)
    e.end_marker()
    at_end = E.lz_chunk(0xE0, e.restart_rc(), e.total, prop_byte(3, 0, 2)) + b"\0"
    f = E.Encoder(3, 0, 2)
    _lits(f, rng, 15)
    f.end_marker()
    _lits(f, rng, 15)
    before = E.lz_chunk(0xE0, f.restart_rc(), f.total, prop_byte(3, 0, 2)) + b"\0"
    return [_case2("end marker at the chunk's end", "marker_in_chunk", at_end, 30,
                   {0: OK, 1: ERR}, [e.record]),
            _case2("end marker at the chunk's end, cap+5", "marker_in_chunk", at_end, 35, ERR,
                   [e.record]),
            _case2("end marker before the chunk's end", "marker_in_chunk", before, 30, ERR,
                   [f.record])]


def _edge_after_stored():
    rng = random.Random(40)
    raw = bytes(rng.choice(ALPHA) for _ in range(5000))
    out = []
    for idx, want in ((4095, OK), (4096, ERR)):
        e = E.Encoder(3, 0, 2)
        e.stored(raw)
        _lits(e, rng, 2)
        e.raw_match(idx, 6, model=want == OK)
        if want == OK:
            _lits(e, rng, 3)
        n = e.total - 5000 if want == OK else 8
        src = E.copy_chunk(1, raw) + E.lz_chunk(0xC0, e.restart_rc(), n,
                                                prop_byte(3, 0, 2)) + b"\0"
        out.append(_case2(f"5000 stored bytes, distance index {idx}", "edge_after_stored", src,
                          5000 + n, want, [e.record]))
    return out


_BUILDERS2 = (_props_change, _after_stored, _missing_props, _bad_first, _stored_only,
              _bad_prop_byte, _padded_pack, _unpack_size, _marker_in_chunk, _edge_after_stored)

_C = {}


def lzma_cases():
    if "lzma" not in _C:
        _C["lzma"] = [c for plp in PROPS for b in _BUILDERS for c in b(plp)]
    return _C["lzma"]


def lzma2_cases():
    if "lzma2" not in _C:
        _C["lzma2"] = [c for b in _BUILDERS2 for c in b()]
    return _C["lzma2"]


def cases():
    return lzma_cases() + lzma2_cases()


def key(c, finish):
    return f"{c['name']} | finish {finish}"


# ------------------------------------------------------------------ expected results

def _run(lib, prefix, c, finish):
    if c["kind"] == "lzma":
        r = native.decode(lib, prefix, c["src"], c["props"], c["cap"], finish)
    else:
        r = native.lzma2_decode(lib, prefix, c["src"], c["prop"], c["cap"], finish)
    return tuple(r[:4]), r[4]


def from_reference(c, finish):
    """((res, status, destLen, srcLen), output) from the live reference."""
    return _run(native.ref(), "ref", c, finish)


def from_oracle(c, finish):
    return _run(native.oracle(), "orc", c, finish)


def golden():
    if "golden" not in _C:
        with open(GOLDEN) as f:
            _C["golden"] = json.load(f)["cases"]
    return _C["golden"]


def expected(c, finish):
    """((res, status, destLen, srcLen), SHA-256 of the output): the live
    reference's where it is built, else the recorded one."""
    k = key(c, finish)
    if ("exp", k) not in _C:
        if native.have_ref():
            row, out = from_reference(c, finish)
            _C["exp", k] = (row, sha(out))
        else:
            g = golden()[k]
            _C["exp", k] = ((g["res"], g["status"], g["dest_len"], g["src_len"]), g["sha256"])
    return _C["exp", k]


# ------------------------------------------------------------------ batches

def items(cs=None, align=True):
    """(case, finish) for both finish modes of every case, and again at each of
    the 16 source alignments for the cases whose input is at most 64 bytes
    (align: the input's address modulo 16, None: wherever it falls)."""
    out = []
    for c in cases() if cs is None else cs:
        for finish in (0, 1):
            out.append((c, finish, None))
    if align:
        for c in cases() if cs is None else cs:
            if len(c["src"]) <= 64:
                for finish in (0, 1):
                    out.extend((c, finish, a) for a in range(16))
    return out


def batch(its):
    """Batch descriptors (lzmagpu.make_descs items), the source and the
    destination size for a list of (case, finish, align)."""
    descs, src, doff = [], bytearray(), 0
    for c, finish, align in its:
        if align is not None:
            src += bytes((align - len(src)) % 16)
        d = dict(src_off=len(src), src_len=len(c["src"]), dst_off=doff, dst_cap=c["cap"],
                 finish=finish)
        if c["kind"] == "lzma":
            d["props"] = c["props"]
        else:
            d["props"], d["kind"] = bytes([c["prop"]]), 1
        descs.append(d)
        src += c["src"]
        doff += c["cap"]
    return descs, bytes(src) + bytes(16), doff


def mismatches(its, descs, res, dst, poison=None):
    """Result rows and output bytes of a decoded batch against expected();
    with `poison` (the byte the destination was filled with) also that nothing
    was written behind a stream's dest_len."""
    bad = []
    for k, (c, finish, align) in enumerate(its):
        row, digest = expected(c, finish)
        got = (res[k].res, res[k].status, res[k].dest_len, res[k].src_len)
        at = descs[k]["dst_off"]
        if got != row or got[2] > c["cap"] or sha(dst[at:at + got[2]]) != digest:
            bad.append((c["name"], finish, align, got, row))
        elif poison is not None and dst[at + got[2]:at + c["cap"]].strip(bytes([poison])):
            bad.append((c["name"], finish, align, "wrote behind dest_len", got))
    return bad

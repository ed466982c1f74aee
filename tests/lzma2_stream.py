"""The LZMA2 streaming drop-ins (Lzma2Dec_DecodeToBuf, Lzma2Dec_DecodeToDic),
call by call, through any library that exports Lzma2Dec.h: liblzmagpu.so or
the reference's Lzma2Dec.c compiled in place (oracle/_ref/libref_lzma.so) --
TEST INFRASTRUCTURE, as lzmaenc_min.ring_decode / dic_calls are for LzmaDec.h.

Two loops, one signature: loop(lib, src, prop, cap, in_chunk, out_chunk,
finish, between=None) -> (trace, output, input used, finish mode per call).

  buf_loop  Lzma2Dec_Allocate (the decoder's own ring of the prop's dictionary
            size) + Lzma2Dec_Init, then Lzma2Dec_DecodeToBuf with at most
            in_chunk input and out_chunk output bytes per call;
            trace rows (res, status, srcLen, destLen).
  dic_loop  Lzma2Dec_AllocateProbs + a caller-owned flat dictionary of cap
            bytes, then Lzma2Dec_DecodeToDic with dicLimit advancing by
            out_chunk per call (0: the whole dictionary at once);
            trace rows (res, status, srcLen, dicPos).

`finish` is applied on the calls that reach the capacity, FINISH_ANY before.
A loop ends on an error, on FINISHED_WITH_MARK, or on a call that neither took
input nor gave output.

The inputs (cases()), their chunkings (grid()), the recorded reference results
(tests/golden/lzma2_stream_cases.json, written by
tests/golden/make_golden_lzma2_stream.py: per run the call count and SHA-256 of
trace and output) and the coverage conditions found in the recorded runs
(CONDITIONS, witness())."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np

import golden_cases as G
import handmade_cases as H
import native

GOLDEN = os.path.join(native.ROOT, "tests", "golden", "lzma2_stream_cases.json")
MAX_CALLS = 20000
BIG = 1 << 20
SMALL_CAP = 300
# hand-made cases: the small ones byte by byte, every one at the coarser pairs
# (5..7: inside headers; 19/20 and 272/273: LZMA_REQUIRED_INPUT_MAX and the
# longest match; 4096: the ring of prop 0)
HAND_SMALL = ((1, 1), (1, BIG), (BIG, 1), (2, 3))
HAND_ALL = ((5, 7), (6, 273), (19, 272), (20, 273), (4096, 4096), (BIG, BIG))
GOLDEN_CHUNKS = ((BIG, BIG), (777, 5000), (100, 333))
LONG_CHUNKS = ((BIG, BIG), (4096, 4096), (777, 5000), (100, 333), (BIG, 1000))
LONG_SEEDS = (1, 2)
LOOPS = ("buf", "dic")

_vp = ctypes.c_void_p
_declared = set()
_C = {}


def _decl(lib):
    if id(lib) in _declared:
        return
    for name, args in (("Lzma2Dec_Allocate", [_vp, ctypes.c_ubyte, _vp]),
                       ("Lzma2Dec_AllocateProbs", [_vp, ctypes.c_ubyte, _vp]),
                       ("Lzma2Dec_Init", [_vp]),
                       ("Lzma2Dec_DecodeToBuf", [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
                       ("Lzma2Dec_DecodeToDic", [_vp, ctypes.c_size_t, _vp, _vp, ctypes.c_int, _vp]),
                       ("LzmaDec_Free", [_vp, _vp]), ("LzmaDec_FreeProbs", [_vp, _vp])):
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = None if name in ("Lzma2Dec_Init", "LzmaDec_Free", "LzmaDec_FreeProbs") \
            else ctypes.c_int
    _declared.add(id(lib))


def _new_decoder():
    import lzmagpu as L
    d = L.CLzma2Dec()
    d.decoder.dic = None
    d.decoder.probs = None
    return d, ctypes.byref(L.g_alloc)


def buf_loop(lib, src, prop, cap, in_chunk, out_chunk, finish, between=None):
    _decl(lib)
    d, alloc = _new_decoder()
    r = lib.Lzma2Dec_Allocate(ctypes.byref(d), prop, alloc)
    if r != 0:
        return [(r, -1, 0, 0)], b"", 0, [finish]
    lib.Lzma2Dec_Init(ctypes.byref(d))
    sbuf = ctypes.create_string_buffer(bytes(src), max(len(src), 1))
    out = ctypes.create_string_buffer(max(cap, 1))
    trace, fins, ip, op = [], [], 0, 0
    try:
        while len(trace) < MAX_CALLS:
            sl = ctypes.c_size_t(min(in_chunk, len(src) - ip))
            n = min(out_chunk, cap - op)
            dl = ctypes.c_size_t(n)
            fin = finish if op + n == cap else 0
            st = ctypes.c_int(-1)
            r = lib.Lzma2Dec_DecodeToBuf(ctypes.byref(d), ctypes.addressof(out) + op,
                                         ctypes.byref(dl), ctypes.addressof(sbuf) + ip,
                                         ctypes.byref(sl), fin, ctypes.byref(st))
            trace.append((r, st.value, sl.value, dl.value))
            fins.append(fin)
            ip += sl.value
            op += dl.value
            if r != 0 or st.value == 1 or (sl.value == 0 and dl.value == 0):
                break
            if between:
                between(len(trace), d)
    finally:
        lib.LzmaDec_Free(ctypes.byref(d.decoder), alloc)
    return trace, out.raw[:op], ip, fins


def dic_loop(lib, src, prop, cap, in_chunk, dic_chunk, finish, between=None):
    _decl(lib)
    d, alloc = _new_decoder()
    r = lib.Lzma2Dec_AllocateProbs(ctypes.byref(d), prop, alloc)
    if r != 0:
        return [(r, -1, 0, 0)], b"", 0, [finish]
    dic = ctypes.create_string_buffer(max(cap, 1))
    d.decoder.dic = ctypes.addressof(dic)
    d.decoder.dicBufSize = cap
    lib.Lzma2Dec_Init(ctypes.byref(d))
    sbuf = ctypes.create_string_buffer(bytes(src), max(len(src), 1))
    trace, fins, ip = [], [], 0
    try:
        while len(trace) < MAX_CALLS:
            sl = ctypes.c_size_t(min(in_chunk, len(src) - ip))
            pos0 = d.decoder.dicPos
            limit = cap if dic_chunk == 0 else min(pos0 + dic_chunk, cap)
            fin = finish if limit == cap else 0
            st = ctypes.c_int(-1)
            r = lib.Lzma2Dec_DecodeToDic(ctypes.byref(d), limit, ctypes.addressof(sbuf) + ip,
                                         ctypes.byref(sl), fin, ctypes.byref(st))
            trace.append((r, st.value, sl.value, d.decoder.dicPos))
            fins.append(fin)
            ip += sl.value
            if r != 0 or st.value == 1 or (sl.value == 0 and d.decoder.dicPos == pos0):
                break
            if between:
                between(len(trace), d)
        pos = d.decoder.dicPos
    finally:
        lib.LzmaDec_FreeProbs(ctypes.byref(d.decoder), alloc)
    return trace, dic.raw[:pos], ip, fins


LOOP_FN = {"buf": buf_loop, "dic": dic_loop}


# ------------------------------------------------------------------ inputs

def lzma2_chunks(comp):
    """(offset, control, unpacked size, header bytes, data bytes) per chunk of a
    well-formed LZMA2 stream, up to its end byte."""
    out, i = [], 0
    while i < len(comp) and comp[i] != 0:
        c = comp[i]
        if c & 0x80:
            un = ((c & 0x1F) << 16) + (comp[i + 1] << 8) + comp[i + 2] + 1
            head = 5 + (1 if (c >> 5) & 3 >= 2 else 0)
            n = (comp[i + 3] << 8) + comp[i + 4] + 1
        else:
            un = n = (comp[i + 1] << 8) + comp[i + 2] + 1
            head = 3
        out.append((i, c, un, head, n))
        i += head + n
    return out


def long_stored(seed):
    """(plaintext, LZMA2 stream, prop 0) from liblzma with a 4 KiB dictionary:
    70,000 random bytes, 30 rounds of (a 20..299-byte tail of that block + 40
    words of text), a 9,000-byte random block and the same 30 rounds after it.
    Its first chunk is stored and many times the ring; the LZMA chunk behind it
    copies from the stored bytes."""
    import lzma
    rng = random.Random(seed)
    parts = []
    for k, size in enumerate((70_000, 9_000)):
        blk = rng.randbytes(size)
        parts.append(blk)
        text = native.gen("text", seed * 10 + k, 4000).split(b" ")
        for _ in range(30):
            parts.append(blk[-rng.randrange(20, 300):])
            at = rng.randrange(max(1, len(text) - 40))
            parts.append(b" ".join(text[at:at + 40]))
    data = b"".join(parts)
    comp = lzma.compress(data, format=lzma.FORMAT_RAW,
                         filters=[{"id": lzma.FILTER_LZMA2, "dict_size": 4096}])
    return data, comp, 0


def ring_straddle():
    """(stream, capacity): an LZMA chunk up to 96 bytes before the end of the
    4 KiB ring of prop 0, a stored chunk of 200 bytes across the ring's end, and
    an LZMA chunk that copies from both sides of it -- between two decoder calls
    the walker writes a span that wraps."""
    import lzmaenc_min as E
    rng = random.Random(41)
    e = E.Encoder(3, 0, 2)
    H._lits(e, rng, 3990)
    e.match(7, 10)
    src = E.lz_chunk(0xE0, e.restart_rc(), e.total, H.prop_byte(3, 0, 2))
    raw = bytes(rng.choice(H.ALPHA) for _ in range(200))
    e.stored(raw)
    src += E.copy_chunk(2, raw)
    start = e.total
    e.match(150, 20)    # from before the ring's end
    e.match(100, 30)    # from behind it
    H._lits(e, rng, 5)
    src += E.lz_chunk(0x80, e.restart_rc(), e.total - start) + b"\0"
    return src, e.total


def cases():
    """Every input: dict(name, src, prop, cap, finishes, chunkings)."""
    if "cases" in _C:
        return _C["cases"]
    out = []
    for c in H.lzma2_cases():
        pairs = (HAND_SMALL if c["cap"] <= SMALL_CAP else ()) + HAND_ALL
        out.append(dict(name="hand: " + c["name"], src=c["src"], prop=c["prop"], cap=c["cap"],
                        finishes=(0, 1), chunkings=pairs))
    d = G.load()
    for i, c in G.cases("lzma2"):
        out.append(dict(name=f"golden {i}: {c['note']}", src=G.case_input(d, c), prop=c["prop"],
                        cap=c["dest_cap"], finishes=(c["finish"],), chunkings=GOLDEN_CHUNKS))
    for seed in LONG_SEEDS:
        data, comp, prop = long_stored(seed)
        out.append(dict(name=f"long stored chunk, seed {seed}", src=comp, prop=prop,
                        cap=len(data), finishes=(0, 1), chunkings=LONG_CHUNKS, plain=data))
    src, cap = ring_straddle()
    out.append(dict(name="long ring straddle", src=src, prop=0, cap=cap, finishes=(0, 1),
                    chunkings=LONG_CHUNKS[:4]))
    _C["cases"] = out
    return out


def key(c, finish, loop, i, o):
    return f"{c['name']} | finish {finish} | {loop} | {i},{o}"


def grid(prefix=""):
    """Every (case, finish, loop, in_chunk, out_chunk) of the cases whose name
    begins with prefix, in a fixed order."""
    return [(c, f, lp, i, o) for c in cases() if c["name"].startswith(prefix)
            for f in c["finishes"] for lp in LOOPS for i, o in c["chunkings"]]


def run(lib, cell, between=None):
    c, f, lp, i, o = cell
    return LOOP_FN[lp](lib, c["src"], c["prop"], c["cap"], i, o, f, between)


def record(r):
    """What the fixture keeps of one run."""
    trace, out, used, _ = r
    rows = np.asarray(trace, dtype="<i8").reshape(len(trace), 4)
    return dict(calls=len(trace),
                trace=hashlib.sha256(rows.tobytes() + used.to_bytes(8, "little")).hexdigest(),
                out=hashlib.sha256(out).hexdigest())


def golden():
    if "golden" not in _C:
        with open(GOLDEN) as f:
            _C["golden"] = json.load(f)
    return _C["golden"]


# ------------------------------------------------------------------ coverage conditions

HEADER_BYTES = ("control", "unpack0", "unpack1", "pack0", "pack1")
CONDITIONS = tuple("more input after " + h for h in HEADER_BYTES) + (
    "stored chunk continued across calls", "stored piece ends at the ring end",
    "dicLimit inside an LZMA chunk, FINISH_ANY", "dicLimit inside an LZMA chunk, FINISH_END",
    "SZ_ERROR_DATA after the first call")
RING0 = 4096  # the dictionary of prop 0


def holds(cond, cell, r):
    """The index of the first call of run r (of a well-formed case) at which the
    condition holds, else None.  Positions come from the chunk layout of the
    input and the running sums of the trace."""
    c, f, lp, _, _ = cell
    trace, _, _, fins = r
    chunks = lzma2_chunks(c["src"])
    plain, spans = 0, []
    for off, ctl, un, head, n in chunks:
        spans.append((off, ctl, head, n, plain, plain + un))
        plain += un
    ip = op = 0
    for k, (res, st, sl, dl) in enumerate(trace):
        op0 = op
        ip += sl
        op = op + dl if lp == "buf" else dl
        if cond == "SZ_ERROR_DATA after the first call":
            if res == 1 and k > 0:
                return k
            continue
        for off, ctl, head, n, a, b in spans:
            lz = bool(ctl & 0x80)
            if cond == "dicLimit inside an LZMA chunk, FINISH_END":
                # the capacity lies inside the chunk: whatever the call answers
                if lz and a < op < b and fins[k] == 1 and op == c["cap"]:
                    return k
                continue
            if res != 0:
                return None
            if cond.startswith("more input after "):
                # an LZMA chunk that brings props: the byte after pack1 is the prop byte
                j = HEADER_BYTES.index(cond[len("more input after "):]) + 1
                if lz and head == 6 and st == 3 and ip == off + j:
                    return k
            elif cond == "stored chunk continued across calls":
                if not lz and st in (2, 3) and off + head < ip < off + head + n and k + 1 < len(trace):
                    return k
            elif cond == "stored piece ends at the ring end":
                if not lz and lp == "buf" and c["prop"] == 0 and a < RING0 < b and op0 < RING0 <= op:
                    return k
            elif cond == "dicLimit inside an LZMA chunk, FINISH_ANY":
                # NOT_FINISHED with input left: the call stopped at its limit
                if lz and a < op < b and fins[k] == 0 and st == 2:
                    return k
    return None


def well_formed(c):
    """Cases whose chunk layout lzma2_chunks() can walk to the end byte."""
    try:
        ch = lzma2_chunks(c["src"])
    except IndexError:
        return False
    return bool(ch) and sum(x[3] + x[4] for x in ch) == len(c["src"]) - 1 and c["src"][-1] == 0

"""The hand-made LZMA set (tests/handmade_cases.py) through the decoders that
resume in mid-stream: the chunk grid of the LzmaDec_DecodeToBuf loops, the
slices of the time-sliced batches, and the recorded reference digests
(tests/golden/handmade_stream_cases.json, written by
tests/golden/make_golden_handmade_stream.py).

The streaming cases are the LZMA cases whose dictionary is H.DICT (the
far_direct cases ask for a 4 GiB ring).  A small case (at most 300 input and
300 output bytes) takes every pair of IN_CHUNKS x OUT_CHUNKS; the others take
only the pairs with in_chunk >= 19 and out_chunk >= 272, which keeps the
number of calls of one loop at a few hundred.  19, 20 and 21 straddle the
reference's tempBuf threshold (LZMA_REQUIRED_INPUT_MAX = 20), 272, 273 and 274
the longest match, 4096 is the ring's size.  No pair had to be dropped to keep
the lockstep rounds of the device sessions at most MAX_ROUNDS: the longest
loop of the grid is a small case at (1, 1).

A digest covers, in the order of chunkings(case), each run's
    calls (u64) | trace rows (4 x i64 each) | output | in_used (u64)
little-endian, as the stream-decode loops of the oracle, the reference shim
and the host emulation report them (one signature: run())."""
import ctypes
import hashlib
import json
import os

import numpy as np

import handmade_cases as H
import native

GOLDEN = os.path.join(native.ROOT, "tests", "golden", "handmade_stream_cases.json")
IN_CHUNKS = (1, 2, 5, 19, 20, 21, 1 << 20)
OUT_CHUNKS = (1, 2, 13, 272, 273, 274, 4096, 1 << 20)
SMALL = 300
MAX_ROUNDS = 700
MAX_CALLS = 8192
# time-sliced batches: every slice up to this capacity (+ 1), the listed ones above it
SLICE_ALL_UP_TO = 300
SLICES_LARGE = (1, 2, 3, 7, 97, 271, 272, 273, 274, 275, 1000, 4095, 4096, 4097)

_C = {}


def cases():
    if "cases" not in _C:
        _C["cases"] = [c for c in H.lzma_cases()
                       if int.from_bytes(c["props"][1:5], "little") == H.DICT]
    return _C["cases"]


def is_small(c):
    return len(c["src"]) <= SMALL and c["cap"] <= SMALL


def chunkings(c):
    """(in_chunk, out_chunk) pairs of a case, in digest order."""
    small = is_small(c)
    return [(i, o) for i in IN_CHUNKS for o in OUT_CHUNKS if small or (i >= 19 and o >= 272)]


def grid():
    """Every (case, finish, in_chunk, out_chunk) of the grid, in digest order."""
    return [(c, f, i, o) for c in cases() for f in (0, 1) for i, o in chunkings(c)]


def slices(c):
    cap = c["cap"]
    if cap <= SLICE_ALL_UP_TO:
        return list(range(1, cap + 2))
    return sorted(set(SLICES_LARGE) | {cap - 1, cap, cap + 1})


# ------------------------------------------------------------------ one loop

_TRACE = (ctypes.c_longlong * (4 * MAX_CALLS))()
_ARGS = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
         ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong),
         ctypes.c_int, native.size_t_p, native.size_t_p]


def declare(fn):
    fn.restype = ctypes.c_int
    fn.argtypes = _ARGS
    return fn


def _padded(c):
    # the lane code's readers load aligned 16-byte blocks around the input
    if "padded" not in c:
        c["padded"] = ctypes.create_string_buffer(c["src"], len(c["src"]) + 32)
    return c["padded"]


def run(fn, c, finish, in_chunk, out_chunk):
    """One DecodeToBuf loop through fn (orc_ / ref_lzma_stream_decode, the
    emu's emu_stream_decode / emu_stream_decode_dic).  Returns (calls, trace
    as (calls, 4) int64, output, in_used)."""
    out = ctypes.create_string_buffer(max(c["cap"], 1))
    ol, iu = ctypes.c_size_t(0), ctypes.c_size_t(0)
    calls = fn(c["props"], _padded(c), len(c["src"]), out, c["cap"], in_chunk, out_chunk, finish,
               _TRACE, MAX_CALLS, ctypes.byref(ol), ctypes.byref(iu))
    assert 0 < calls < MAX_CALLS, (c["name"], calls)
    trace = np.frombuffer(_TRACE, dtype="<i8", count=4 * calls).reshape(calls, 4).copy()
    return calls, trace, out.raw[:ol.value], iu.value


def run_bytes(r):
    calls, trace, out, used = r
    return (calls.to_bytes(8, "little") + np.ascontiguousarray(trace, dtype="<i8").tobytes() +
            bytes(out) + used.to_bytes(8, "little"))


def digest(runs):
    """SHA-256 over the runs of one (case, finish), in chunkings order."""
    h = hashlib.sha256()
    for r in runs:
        h.update(run_bytes(r))
    return h.hexdigest()


def digests(fn, cs=None):
    """{key: digest} and {"in,out": largest call count} through fn."""
    out, top = {}, {}
    for c in cases() if cs is None else cs:
        for finish in (0, 1):
            runs = []
            for i, o in chunkings(c):
                r = run(fn, c, finish, i, o)
                runs.append(r)
                k = f"{i},{o}"
                top[k] = max(top.get(k, 0), r[0])
            out[H.key(c, finish)] = digest(runs)
    return out, top


def oracle_fn():
    return declare(native.oracle().orc_lzma_stream_decode)


def reference_fn():
    return declare(native.ref().ref_lzma_stream_decode)


def expected():
    """{(case name, finish, in_chunk, out_chunk): run} from the oracle's loop
    (tests/test_handmade_resume.py pins it to the recorded reference digests)."""
    if "exp" not in _C:
        fn = oracle_fn()
        _C["exp"] = {(c["name"], f, i, o): run(fn, c, f, i, o) for c, f, i, o in grid()}
    return _C["exp"]


def golden():
    if "golden" not in _C:
        with open(GOLDEN) as f:
            _C["golden"] = json.load(f)
    return _C["golden"]

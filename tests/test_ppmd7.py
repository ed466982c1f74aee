"""Ppmd7Gpu_DecodeBatch / Ppmd7Gpu_DecodeBatchHost on the device against the
results recorded from the reference's Ppmd7.c / Ppmd7Dec.c
(tests/golden/ppmd7_cases.json): every well-formed case and every mutated one,
exact result triples and bytes, nothing written outside each stream's range,
workspace slices that do not disturb each other, the edge cases of the result
table, and the host call's launch splitting."""
import ctypes
import os
import sys
import time

import pytest

import native
import ppmd7_golden as P

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))

pytestmark = pytest.mark.gpu
POISON = 0xA5
OK, DATA, MEM, UNSUPPORTED = 0, 1, 2, 4
STEP_LIMIT_S = 60.0  # a decode step that takes longer is a failure, not a wait


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def run_device(L, items):
    """items: (packed, order, mem_size, dst_len).  One Ppmd7Gpu_DecodeBatch with
    byte-odd offsets and a poisoned output.  Returns [(res, dest_len, src_len,
    written bytes)], having checked that the poison outside each written range
    is intact."""
    import numpy as np
    import torch
    n = len(items)
    src, descs, ws = bytearray(b"\x5a"), [], 0
    dst_off = 1
    for packed, order, mem, dst_len in items:
        slice_bytes = L.ppmd7_workspace_bytes(mem)
        descs.append(dict(src_off=len(src), src_len=len(packed), dst_off=dst_off, dst_len=dst_len,
                          order=order, mem_size=mem, ws_off=ws))
        src += packed + b"\x5a" * (2 + len(packed) % 2)   # keeps the next offset odd
        dst_off += dst_len + 2 + dst_len % 2
        ws += slice_bytes
        assert slice_bytes % 256 == 0
    assert all(d["src_off"] % 2 == 1 and d["dst_off"] % 2 == 1 for d in descs)
    arr = L.ppmd7_make_descs(descs)
    d_desc = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).cuda()
    d_src = torch.from_numpy(np.frombuffer(bytes(src), dtype=np.uint8).copy()).cuda()
    d_dst = torch.full((dst_off + 64,), POISON, dtype=torch.uint8, device="cuda")
    d_ws = torch.empty((max(ws, 256),), dtype=torch.uint8, device="cuda")
    d_res = torch.full((max(n, 1) * 24,), 0xEE, dtype=torch.uint8, device="cuda")
    t0 = time.monotonic()
    r = L.ppmd7_decode_batch_device(d_desc.data_ptr(), n, d_src.data_ptr(), d_dst.data_ptr(),
                                    d_ws.data_ptr(), d_res.data_ptr())
    torch.cuda.synchronize()
    took = time.monotonic() - t0
    assert r == OK, L.last_error()
    assert took < STEP_LIMIT_S, took
    res = (L.Ppmd7Result * max(n, 1)).from_buffer_copy(d_res.cpu().numpy().tobytes())
    out = d_dst.cpu().numpy().tobytes()
    got, at = [], 0
    for k, d in enumerate(descs):
        q = res[k]
        assert out[at:d["dst_off"]] == bytes([POISON]) * (d["dst_off"] - at), k
        assert q.dest_len <= d["dst_len"]
        at = d["dst_off"] + q.dest_len
        got.append((q.res, q.dest_len, q.src_len, out[d["dst_off"]:at]))
    assert out[at:] == bytes([POISON]) * (len(out) - at)
    return got


def golden_items(d, which):
    return [(P.packed(d, c), c["order"], c["mem_size"], c["plain_len"]) for c in which]


def test_all_golden_cases_in_one_batch(L):
    d = P.load()
    cases = d["cases"] + d["sevenz"] + d["bench"]
    got = run_device(L, golden_items(d, cases))
    for k, c in enumerate(cases):
        res, dl, sl, out = got[k]
        assert (res, dl, sl) == (OK, c["plain_len"], c["len"]), (k, res, dl, sl)
        assert P.sha(out) == c["sha256"], k


def test_all_mutated_cases_beside_well_formed_neighbours(L):
    """Every mutated case in one launch; each well-formed base is repeated
    between corrupt neighbours and must still decode exactly (slices do not
    overlap, a failing stream disturbs nobody)."""
    d = P.load()
    items, want = [], []
    bases = sorted({m["base"] for m in d["mutated"]})
    for i, m in enumerate(d["mutated"]):
        c = d["cases"][m["base"]]
        src, dst_len = P.mutated_input(d, m)
        items.append((src, c["order"], c["mem_size"], dst_len))
        want.append((m["res"], m["dest_len"], m["src_len"], m["sha256"]))
        if i % 37 == 5:
            b = d["cases"][bases[(i // 37) % len(bases)]]
            items += golden_items(d, [b])
            want.append((OK, b["plain_len"], b["len"], b["sha256"]))
    assert len(d["mutated"]) >= 200 and len(items) >= len(d["mutated"]) + len(bases)
    got = run_device(L, items)
    for k, (res, dl, sl, out) in enumerate(got):
        assert (res, dl, sl, P.sha(out)) == want[k], (k, res, dl, sl, want[k][:3])


def test_edges_of_the_result_table(L):
    d = P.load()
    c = d["cases"][0]
    good = (P.packed(d, c), c["order"], c["mem_size"], c["plain_len"])
    assert run_device(L, []) == []
    (res, dl, sl, out), = run_device(L, [good])
    assert (res, dl, sl, P.sha(out)) == (OK, c["plain_len"], c["len"], c["sha256"])
    M = 1 << 16
    items = [(b"\0" * 5, 6, M, 0),                 # nothing to decode, a finished coder
             (b"\0" * 4, 6, M, 0),                 # the init bytes run out
             (b"", 6, M, 7),
             (b"\0\xff\xff\xff\xff", 6, M, 3),     # the all-ones code
             (b"\x01" + good[0][1:], c["order"], c["mem_size"], c["plain_len"]),
             (good[0], 1, c["mem_size"], c["plain_len"]),          # bad props: nothing read
             (good[0], 65, c["mem_size"], c["plain_len"]),
             (good[0], c["order"], (1 << 11) - 1, c["plain_len"]),
             (good[0], c["order"], 0xFFFFFFFF - 35, c["plain_len"]),
             good]
    got = run_device(L, items)
    assert [g[:3] for g in got[:5]] == [(OK, 0, 5), (DATA, 0, 4), (DATA, 0, 0), (DATA, 0, 5),
                                        (DATA, 0, 1)]
    assert [g[:3] for g in got[5:9]] == [(UNSUPPORTED, 0, 0)] * 4
    assert got[9][:3] == (OK, c["plain_len"], c["len"]) and P.sha(got[9][3]) == c["sha256"]
    assert L.ppmd7_workspace_bytes((1 << 11) - 1) == 0 == L.ppmd7_workspace_bytes(0xFFFFFFFF - 35)


def host_batch(L, d, cases, limit):
    src, descs, dst_off = bytearray(b"\x5a"), [], 3
    for c in cases:
        p = P.packed(d, c)
        descs.append(dict(src_off=len(src), src_len=len(p), dst_off=dst_off,
                          dst_len=c["plain_len"], order=c["order"], mem_size=c["mem_size"]))
        src += p
        dst_off += c["plain_len"] + 1
    t0 = time.monotonic()
    r, res, out = L.ppmd7_decode_batch_host(L.ppmd7_make_descs(descs), len(descs), bytes(src),
                                            bytes([POISON]) * (dst_off + 5), limit)
    assert time.monotonic() - t0 < STEP_LIMIT_S
    return r, [(q.res, q.dest_len, q.src_len) for q in list(res)[:len(descs)]], out, descs


def test_host_call_splits_launches_by_the_workspace_limit(L):
    d = P.load()
    cases = [c for c in d["cases"] if c["plain_len"] <= 30000]
    slices = [L.ppmd7_workspace_bytes(c["mem_size"]) for c in cases]
    limit = max(slices)
    assert sum(slices) > 2 * limit  # at least three launches
    r1, res1, out1, descs = host_batch(L, d, cases, 0)
    r3, res3, out3, _ = host_batch(L, d, cases, limit)
    assert r1 == OK and r3 == OK, L.last_error()
    assert res1 == res3 == [(OK, c["plain_len"], c["len"]) for c in cases]
    assert out1 == out3
    at = 0
    for c, q in zip(cases, descs):
        assert out1[at:q["dst_off"]] == bytes([POISON]) * (q["dst_off"] - at)
        at = q["dst_off"] + q["dst_len"]
        assert P.sha(out1[q["dst_off"]:at]) == c["sha256"]
    assert out1[at:] == bytes([POISON]) * (len(out1) - at)
    # one stream alone over the limit
    r, _, out, _ = host_batch(L, d, cases, min(slices) - 1)
    assert r == MEM and out == bytes([POISON]) * len(out)
    assert host_batch(L, d, [], 0)[0] == OK

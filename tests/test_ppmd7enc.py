"""Ppmd7Gpu_EncodeBatch / Ppmd7Gpu_EncodeBatchHost on the device against the
reference encoder's own streams: the 15 of tests/golden/ppmd7_cases.json (their
plain text recovered on the device with Ppmd7Gpu_DecodeBatch and checked by
sha256) and the 56 of ppmd7enc_cases.json.  Exact bytes and result triples,
nothing written outside each stream's range, every output capacity of one
stream as a batch larger than the device holds at once, the edge cases of the
result table, the host call's launch splitting, and a round trip through 7z
folders."""
import os
import struct
import sys
import time

import pytest

import native
import ppmd7enc_cases as C
import ppmd7_golden as P

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))

pytestmark = pytest.mark.gpu
POISON = C.POISON
OK, MEM, PARAM, OUTPUT_EOF = 0, 2, 5, 7
STEP_LIMIT_S = 60.0  # a step that takes longer is a failure, not a wait


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def to_device(b):
    import numpy as np
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def pack_odd(blocks):
    """The blocks in one buffer, each at an odd offset.  Returns (bytes, offsets)."""
    buf, offs = bytearray(b"\x5a"), []
    for b in blocks:
        offs.append(len(buf))
        buf += b + b"\x5a" * (2 + len(b) % 2)
    assert all(o % 2 == 1 for o in offs)
    return bytes(buf), offs


def run_encode(L, d_src, items):
    """items: (src_off, src_len, order, mem_size, dst_cap).  One
    Ppmd7Gpu_EncodeBatch over the plain bytes already in d_src, with byte-odd
    output offsets, a poisoned output, a result array pre-filled with 0xEE and
    one slice per stream.  Returns [(res, dest_len, packed_len, written
    bytes)], having checked that the poison outside each written range is
    intact."""
    import torch
    n = len(items)
    descs, ws, dst_off = [], 0, 1
    for src_off, src_len, order, mem, cap in items:
        slice_bytes = L.ppmd7_workspace_bytes(mem)
        assert slice_bytes % 256 == 0
        descs.append(dict(src_off=src_off, src_len=src_len, dst_off=dst_off, dst_cap=cap,
                          order=order, mem_size=mem, ws_off=ws))
        dst_off += cap + 2 + cap % 2
        ws += slice_bytes
    assert all(d["dst_off"] % 2 == 1 for d in descs)
    d_desc = to_device(bytes(L.ppmd7_make_enc_descs(descs)))
    d_dst = torch.full((dst_off + 64,), POISON, dtype=torch.uint8, device="cuda")
    d_ws = torch.empty((max(ws, 256),), dtype=torch.uint8, device="cuda")
    d_res = torch.full((max(n, 1) * 24,), 0xEE, dtype=torch.uint8, device="cuda")
    t0 = time.monotonic()
    r = L.ppmd7_encode_batch_device(d_desc.data_ptr(), n, d_src.data_ptr(), d_dst.data_ptr(),
                                    d_ws.data_ptr(), d_res.data_ptr())
    torch.cuda.synchronize()
    took = time.monotonic() - t0
    assert r == OK, L.last_error()
    assert took < STEP_LIMIT_S, took
    raw = d_res.cpu().numpy().tobytes()
    if n == 0:
        assert raw == b"\xee" * 24
    res = (L.Ppmd7EncResult * max(n, 1)).from_buffer_copy(raw)
    out = d_dst.cpu().numpy().tobytes()
    got, at = [], 0
    for k, d in enumerate(descs):
        q = res[k]
        assert out[at:d["dst_off"]] == bytes([POISON]) * (d["dst_off"] - at), k
        assert q.dest_len <= d["dst_cap"] and q._pad == 0, k
        at = d["dst_off"] + q.dest_len
        got.append((q.res, q.dest_len, q.packed_len, out[d["dst_off"]:at]))
    assert out[at:] == bytes([POISON]) * (len(out) - at)
    return got


def decode_fixtures(L):
    """The 15 fixture streams through one Ppmd7Gpu_DecodeBatch.  Returns the
    device buffer holding the plain texts and their (odd) offsets in it."""
    import torch
    d = P.load()
    cases = C.fixture_cases()
    src, src_offs = pack_odd([P.packed(d, c) for c in cases])
    descs, ws, dst_off = [], 0, 1
    for c, so in zip(cases, src_offs):
        descs.append(dict(src_off=so, src_len=c["len"], dst_off=dst_off, dst_len=c["plain_len"],
                          order=c["order"], mem_size=c["mem_size"], ws_off=ws))
        dst_off += c["plain_len"] + 2 + c["plain_len"] % 2
        ws += L.ppmd7_workspace_bytes(c["mem_size"])
    d_desc = to_device(bytes(L.ppmd7_make_descs(descs)))
    d_src = to_device(src)
    d_plain = torch.full((dst_off + 64,), POISON, dtype=torch.uint8, device="cuda")
    d_ws = torch.empty((ws,), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((len(cases) * 24,), dtype=torch.uint8, device="cuda")
    t0 = time.monotonic()
    r = L.ppmd7_decode_batch_device(d_desc.data_ptr(), len(cases), d_src.data_ptr(),
                                    d_plain.data_ptr(), d_ws.data_ptr(), d_res.data_ptr())
    torch.cuda.synchronize()
    assert r == OK and time.monotonic() - t0 < STEP_LIMIT_S
    res = (L.Ppmd7Result * len(cases)).from_buffer_copy(d_res.cpu().numpy().tobytes())
    assert all((q.res, q.dest_len, q.src_len) == (0, c["plain_len"], c["len"])
               for q, c in zip(res, cases))
    return d_plain, [q["dst_off"] for q in descs]


@pytest.fixture(scope="module")
def fx(L):
    """The fixture streams: their plain texts on the device (decoded there, no
    host copy between) and on the host (sha256 checked), computed once."""
    d = P.load()
    cases = C.fixture_cases()
    d_plain, offs = decode_fixtures(L)
    host = d_plain.cpu().numpy().tobytes()
    plains = [host[o:o + c["plain_len"]] for o, c in zip(offs, cases)]
    for c, p in zip(cases, plains):
        assert P.sha(p) == c["sha256"]
    return dict(cases=cases, d_plain=d_plain, offs=offs, plains=plains,
                packed=[P.packed(d, c) for c in cases])


def test_decoded_on_the_device_then_encoded_there(L, fx):
    """Device composition: the d_dst of the decode batch is the d_src of the
    encode batch, and the packed bytes come back equal."""
    items = [(o, c["plain_len"], c["order"], c["mem_size"], c["len"])
             for o, c in zip(fx["offs"], fx["cases"])]
    got = run_encode(L, fx["d_plain"], items)
    for k, (res, dl, pl, out) in enumerate(got):
        n = len(fx["packed"][k])
        assert (res, dl, pl) == (OK, n, n), (k, res, dl, pl)
        assert out == fx["packed"][k], k


def test_every_fixture_and_supplementary_stream_in_one_batch(L, fx):
    streams = [(p, q, c["order"], c["mem_size"])
               for p, q, c in zip(fx["plains"], fx["packed"], fx["cases"])] + C.supplementary()
    assert len(streams) == 15 + 56
    src, offs = pack_odd([s[0] for s in streams])
    # capacities: exact, and a few bytes to spare
    items = [(o, len(p), order, mem, len(q) + (k % 3)) for k, (o, (p, q, order, mem))
             in enumerate(zip(offs, streams))]
    got = run_encode(L, to_device(src), items)
    for k, (res, dl, pl, out) in enumerate(got):
        q = streams[k][1]
        assert (res, dl, pl) == (OK, len(q), len(q)), (k, streams[k][2:], res, dl, pl)
        assert out == q, (k, streams[k][2:])


def test_every_capacity_of_one_stream_as_one_batch(L, fx):
    """Case index 2 (18 pending 0xFF runs, one carry rippling through a run) at
    every dst_cap in 0..len+1: 4,407 streams, more than are resident at once,
    about 92 MB of slices."""
    c, packed = fx["cases"][2], fx["packed"][2]
    n = len(packed)
    assert n == 4405 and (c["order"], c["mem_size"], c["plain_len"]) == (2, 4096, 4096)
    src, (off,) = pack_odd([fx["plains"][2]])
    items = [(off, c["plain_len"], 2, 4096, cap) for cap in range(n + 2)]
    assert len(items) == 4407
    assert len(items) * L.ppmd7_workspace_bytes(4096) > 90e6
    got = run_encode(L, to_device(src), items)
    for cap, (res, dl, pl, out) in enumerate(got):
        assert res == (OUTPUT_EOF if cap < n else OK), cap
        assert (dl, pl) == (min(cap, n), n), cap
        assert out == packed[:dl], cap


def test_edges_of_the_result_table(L, fx):
    plain, packed, c = fx["plains"][0], fx["packed"][0], fx["cases"][0]
    src, (off,) = pack_odd([plain])
    d_src = to_device(src)
    assert run_encode(L, d_src, []) == []      # n == 0: nothing touched
    good = (off, len(plain), c["order"], c["mem_size"], len(packed))
    items = [good,
             (off, len(plain), 1, c["mem_size"], len(packed)),          # bad props: nothing read
             (off, len(plain), 65, c["mem_size"], len(packed)),
             good,
             (off, len(plain), c["order"], (1 << 11) - 1, len(packed)),
             (off, len(plain), c["order"], 0xFFFFFFFF - 35, len(packed)),
             (off, 0, 6, 1 << 16, 9),                                   # nothing to encode
             (off, 0, 64, 2049, 5),
             (off, 0, 2, 2048, 3),
             good]
    got = run_encode(L, d_src, items)
    for k in (0, 3, 9):
        assert got[k] == (OK, len(packed), len(packed), packed), k
    for k in (1, 2, 4, 5):
        assert got[k] == (PARAM, 0, 0, b""), k
    assert got[6] == (OK, 5, 5, b"\0" * 5) == got[7]
    assert got[8] == (OUTPUT_EOF, 3, 5, b"\0" * 3)


def host_batch(L, fx, which, limit):
    src, descs, dst_off = bytearray(b"\x5a"), [], 3
    for k in which:
        p, c = fx["plains"][k], fx["cases"][k]
        descs.append(dict(src_off=len(src), src_len=len(p), dst_off=dst_off, dst_cap=c["len"] + 7,
                          order=c["order"], mem_size=c["mem_size"]))
        src += p
        dst_off += c["len"] + 8
    t0 = time.monotonic()
    r, res, out = L.ppmd7_encode_batch_host(L.ppmd7_make_enc_descs(descs), len(descs), bytes(src),
                                            bytes([POISON]) * (dst_off + 5), limit)
    assert time.monotonic() - t0 < STEP_LIMIT_S
    return r, [(q.res, q.dest_len, q.packed_len) for q in list(res)[:len(descs)]], out, descs


def test_host_call_splits_launches_by_the_workspace_limit(L, fx):
    which = [k for k, c in enumerate(fx["cases"][:11]) if c["plain_len"] <= 30000]
    slices = [L.ppmd7_workspace_bytes(fx["cases"][k]["mem_size"]) for k in which]
    limit = max(slices)
    assert sum(slices) > 2 * limit  # at least three launches
    r1, res1, out1, descs = host_batch(L, fx, which, 0)
    r3, res3, out3, _ = host_batch(L, fx, which, limit)
    assert r1 == OK and r3 == OK, L.last_error()
    assert res1 == res3 == [(OK, fx["cases"][k]["len"], fx["cases"][k]["len"]) for k in which]
    assert out1 == out3
    at = 0
    for k, q in zip(which, descs):
        assert out1[at:q["dst_off"]] == bytes([POISON]) * (q["dst_off"] - at)
        at = q["dst_off"] + len(fx["packed"][k])
        assert out1[q["dst_off"]:at] == fx["packed"][k]
    assert out1[at:] == bytes([POISON]) * (len(out1) - at)
    # one stream alone over the limit
    r, _, out, _ = host_batch(L, fx, which, min(slices) - 1)
    assert r == MEM and out == bytes([POISON]) * len(out)
    assert host_batch(L, fx, [], 0)[0] == OK


def test_7z_round_trip(L, fx):
    """GPU-encoded streams as 7z PPMd folders (method 0x030401, props = order
    byte + mem LE32), extracted with LzmaGpu_7zExtractEx and LZMA_GPU_7Z_PPMD."""
    import sevenzwrite as Z
    supp = [s for s in C.supplementary() if len(s[0]) > 2000 and s[3] & 3][:2]
    streams = [(fx["plains"][k], fx["cases"][k]["order"], fx["cases"][k]["mem_size"])
               for k in (11, 12)] + [(p, order, mem) for p, _, order, mem in supp]
    assert len(streams) == 4
    src, offs = pack_odd([s[0] for s in streams])
    got = run_encode(L, to_device(src), [(o, len(p), order, mem, len(p) + 1024)
                                         for o, (p, order, mem) in zip(offs, streams)])
    folders = []
    for k, ((plain, order, mem), (res, dl, pl, packed)) in enumerate(zip(streams, got)):
        assert res == OK and dl == pl
        cutat = len(plain) // 3
        files = [(f"s{k}a.txt", plain[:cutat]), (f"s{k}b.txt", plain[cutat:])]
        folders.append(Z.Folder(files, method=0x030401, packed=packed,
                                props=bytes([order]) + struct.pack("<I", mem), crc=bool(k & 1)))
    arc = Z.archive(folders)
    r, fo, files, _, total = L.sz_open(arc, flags=L.SZ_PPMD)
    assert r == 0 and [f.supported for f in fo] == [0] * 4
    r, out, fres = L.SzExtract(arc, total, flags=L.SZ_PPMD)
    assert r == 0 and fres[:len(files)] == [0] * len(files)
    want = [d for f in folders for _, d in f.files]
    assert len(want) == len(files) == 8
    for i, w in enumerate(want):
        assert out[files[i].dst_off:files[i].dst_off + files[i].size] == w, i

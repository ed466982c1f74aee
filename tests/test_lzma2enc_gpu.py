"""The LZMA2 and xz writers on the device against the reference: the block
batch (Lzma2EncGpu_EncodeBatch) against its single-threaded Lzma2Enc_Encode of
each block -- live (oracle/_ref/libref_lzma.so) where it is built, else the
committed goldens -- the compaction alone on hand-made slots, one buffer as a
multi-block stream, the Lzma2Enc_* drop-ins through memory streams, and the xz
writer through four decoders.  Equality is the criterion everywhere, and every
byte outside a block's [dst_off, dst_off + dst_cap) keeps its poison."""
import ctypes
import lzma
import os
import struct
import sys
import time

import pytest

import lzma2enc_cases as C
import native
import xzwrite

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))

pytestmark = pytest.mark.gpu
POISON = 0xA5
STEP_LIMIT_S = 60.0  # an encode step that takes longer is a failure, not a wait


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


_want = {}


def want_of(c, golden):
    """The reference's record of a case, computed once and shared."""
    k = C.key(c)
    if k not in _want:
        _want[k] = C.expect(c, golden=golden)
    return _want[k]


def desc_of(L, c):
    return L.enc2_desc_from_props(L.enc2_props(c["level"], c["dict"], c["lc"], c["lp"], c["pb"]))


def raw_desc(L, **kw):
    """A descriptor written by hand (what DescFromProps would refuse)."""
    d = L.EncStreamDesc()
    d.dict_size, d.lc, d.lp, d.pb, d.fb, d.mc = 1 << 16, 3, 0, 2, 32, 16
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def dev(b):
    import numpy as np
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def run_device(L, items, lanes=0, planned_order=True):
    """items: (EncStreamDesc with props set, data, cap).  One
    Lzma2EncGpu_EncodeBatch with byte-odd offsets, a poisoned destination and a
    poisoned workspace.  Returns [(res, dest_len, dst[:dest_len])], having
    checked that the poison outside every block's capacity is intact."""
    import torch
    n = len(items)
    src = bytearray(b"\x5a")
    descs = (L.EncStreamDesc * max(n, 1))()
    dst_off = 1
    for i, (d, data, cap) in enumerate(items):
        ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(d), ctypes.sizeof(d))
        descs[i].src_off, descs[i].dst_off, descs[i].dst_cap = len(src), dst_off, cap
        if descs[i].src_len == 0:
            descs[i].src_len = len(data)
        src += data + b"\x5a" * (2 + len(data) % 2)   # keeps the next offset odd
        dst_off += cap + 2 + cap % 2
        assert descs[i].src_off % 2 == 1 and descs[i].dst_off % 2 == 1
    r, order, ws = L.enc2_plan(descs, n)
    assert r == 0 and sorted(order) == list(range(n))
    lens = [descs[k].src_len for k in order]
    assert lens == sorted(lens, reverse=True)
    d_desc = dev(bytes(descs))
    d_order = dev(bytes((ctypes.c_uint32 * max(n, 1))(*order)))
    d_src = dev(src)
    d_dst = torch.full((dst_off + 64,), POISON, dtype=torch.uint8, device="cuda")
    d_ws = torch.full((max(ws, 256),), 0x3C, dtype=torch.uint8, device="cuda")
    d_res = torch.full((max(n, 1) * 16,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.monotonic()
    r = L.lzma2_encode_batch_device(d_desc.data_ptr(), d_order.data_ptr() if planned_order else 0,
                                    n, d_src.data_ptr(), d_dst.data_ptr(), d_ws.data_ptr(),
                                    d_res.data_ptr(), lanes)
    torch.cuda.synchronize()
    took = time.monotonic() - t0
    assert r == 0, L.last_error()
    assert took < STEP_LIMIT_S, took
    res = (L.EncResult * max(n, 1)).from_buffer_copy(d_res.cpu().numpy().tobytes())
    out = d_dst.cpu().numpy().tobytes()
    got, at = [], 0
    for k in range(n):
        q, d = res[k], descs[k]
        assert out[at:d.dst_off] == bytes([POISON]) * (d.dst_off - at), k
        assert q.dest_len <= d.dst_cap, k
        if q.res in (C.PARAM, C.UNSUPPORTED):     # refused: nothing written at all
            assert out[d.dst_off:d.dst_off + d.dst_cap] == bytes([POISON]) * d.dst_cap, k
        at = d.dst_off + d.dst_cap
        got.append((q.res, q.dest_len, out[d.dst_off:d.dst_off + q.dest_len]))
    assert out[at:] == bytes([POISON]) * (len(out) - at)
    return got


def encode_cases(L, cases, golden, lanes=0, planned_order=True, extra=()):
    """Encodes the cases, each with its block bound for room (plus hand-made
    (position, desc, data, cap, check) extras), in one batch and checks each
    against the reference.  Returns [(prop, block bytes, data)] of the cases that
    ended SZ_OK, for the round trip."""
    items, wants = [], []
    for c in cases:
        w = want_of(c, golden)
        r, d, prop = desc_of(L, c)
        assert r == w["res"], C.key(c)
        if r != 0:
            continue            # refused on the host: nothing reaches the device
        data = C.data_of(c)
        items.append((d, data, C.block_bound(len(data))))
        wants.append((c, w, prop))
    for pos, d, data, cap, check in sorted(extra, key=lambda e: e[0]):
        items.insert(pos, (d, data, cap))
        wants.insert(pos, (None, check, 0))
    got = run_device(L, items, lanes, planned_order)
    back = []
    for k, ((c, w, prop), g) in enumerate(zip(wants, got)):
        if c is None:
            w(g)
            continue
        C.check_block((g[0], g[1], prop, g[2]), w, C.key(c))
        back.append((prop, g[2], items[k][1]))
    return back


def round_trip(L, back):
    """Every block, with the final 0x00 behind it, decodes through
    LzmaGpu_DecodeBatchHost as a kind = 1 item."""
    src, items, dst_off = bytearray(), [], 0
    for prop, packed, data in back:
        items.append(dict(src_off=len(src), src_len=len(packed) + 1, dst_off=dst_off,
                          dst_cap=len(data), props=bytes([prop]), kind=L.KIND_LZMA2))
        src += packed + b"\0"
        dst_off += len(data)
    r, res, out = L.decode_batch_host(L.make_descs(items), bytes(src), dst_off)
    assert r == 0, L.last_error()
    for k, (it, (_, _, data)) in enumerate(zip(items, back)):
        assert (res[k].res, res[k].dest_len) == (0, len(data)), (k, res[k].res, res[k].dest_len)
        assert out[it["dst_off"]:it["dst_off"] + len(data)] == data, k


def test_every_edge_case_in_one_planned_batch(L, golden):
    """The chunk patterns (pack limit, restore and retry, LZMA after copy, copy
    after LZMA, restore and go on), sources of 0..5 bytes, levels, dictionaries
    and the lc / lp / pb corners in the planner's longest-first order; then the
    round trip on the device."""
    cases = C.edge_cases()
    assert sum(C.size_of(c) > 100 * 1024 for c in cases) <= 8
    back = encode_cases(L, cases, golden)
    assert len(back) == len(cases) - 5          # lc + lp = 5 is refused on the host
    round_trip(L, back)


def mixed_cases(golden):
    """62 golden cases of at most 20,000 bytes: their records are committed."""
    pick = [g["case"] for g in golden["cases"]
            if g["res"] == C.OK and 0 < C.size_of(g["case"]) <= 20000]
    assert len(pick) >= 62
    return pick[:62]


@pytest.mark.parametrize("lanes", [64, 32, 16])
def test_mixed_batch_of_65_blocks_in_index_order(L, golden, lanes):
    """One full wave plus one block at lanes == 64, odd offsets; a rejected
    descriptor, an empty block and a block whose second chunk does not fit sit in
    the first 16 lanes of the first wave."""
    two_copies = C.PATTERN_CASES[3]             # copy-reset 56,523, then copy 3,477
    data = C.data_of(two_copies)
    first = b"\x01" + struct.pack(">H", 56523 - 1) + data[:56523]

    def rejected(g):
        assert g == (C.PARAM, 0, b""), g[:2]

    def empty(g):
        assert g == (C.OK, 0, b""), g[:2]

    def overflow(g):                            # room for the first chunk and 5 bytes more
        assert g == (C.OUTPUT_EOF, len(first), first), g[:2]
    extra = [(3, raw_desc(L, lc=3, lp=2), b"abcdefgh", 64, rejected),
             (5, desc_of(L, two_copies)[1], b"", 7, empty),
             (9, desc_of(L, two_copies)[1], data, len(first) + 5, overflow)]
    cases = mixed_cases(golden)
    assert len(cases) + len(extra) == 65
    back = encode_cases(L, cases, golden, lanes=lanes, planned_order=False, extra=extra)
    if lanes == 64:
        round_trip(L, back)


def fuzz_cases(golden):
    if native.have_ref():
        return C.random_cases(256, 515151, max_n=8192)
    cases = [g["case"] for g in golden["cases"]
             if g["res"] == C.OK and C.size_of(g["case"]) <= 8192]
    return (cases * (256 // len(cases) + 1))[:256]


def test_fuzz_256_blocks(L, golden):
    cases = fuzz_cases(golden)
    assert len(cases) == 256 and max(C.size_of(c) for c in cases) <= 8192
    round_trip(L, encode_cases(L, cases, golden))


def test_what_the_kernel_refuses_and_the_empty_batch(L):
    assert run_device(L, []) == []
    for kw, res in ((dict(lc=4, lp=1), C.PARAM), (dict(lc=0, lp=5), C.PARAM), (dict(pb=5), C.PARAM),
                    (dict(fb=4), C.PARAM), (dict(dict_size=0), C.PARAM),
                    (dict(src_len=1 << 31), C.UNSUPPORTED)):
        assert run_device(L, [(raw_desc(L, **kw), b"abcdefgh", 64)]) == [(res, 0, b"")], kw
    assert L.lib.Lzma2EncGpu_EncodeBatch(None, None, 0, None, None, None, None, 0, None) == 0
    assert L.lib.Lzma2EncGpu_EncodeBatch(None, None, 1, None, None, None, None, 48, None) == C.PARAM


def host_batch(L, cases, golden, limit):
    """Lzma2EncGpu_EncodeBatchHost over the cases, each with its block bound for
    room, a poison byte between the slots and around them."""
    src, dst_off = bytearray(b"\x5a"), 3
    descs = (L.EncStreamDesc * max(len(cases), 1))()
    for i, c in enumerate(cases):
        r, d, _ = desc_of(L, c)
        assert r == 0
        ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(d), ctypes.sizeof(d))
        data = C.data_of(c)
        descs[i].src_off, descs[i].src_len, descs[i].dst_off, descs[i].dst_cap = (
            len(src), len(data), dst_off, C.block_bound(len(data)))
        src += data
        dst_off += descs[i].dst_cap + 1
    t0 = time.monotonic()
    r, res, out = L.lzma2_encode_batch_host(descs, len(cases), bytes(src),
                                            bytes([POISON]) * (dst_off + 5), limit)
    assert time.monotonic() - t0 < STEP_LIMIT_S
    return r, [(q.res, q.dest_len) for q in list(res)[:len(cases)]], out, descs


def test_host_call_splits_launches_by_the_workspace_limit(L, golden):
    """The host call's launches take (first, count) over a device copy of the
    longest-first order and write results at the caller's index.  30 blocks of at
    most 6,000 bytes with dictionaries of 4 and 64 KiB from the committed records
    (the 13 of level 1, then other fast levels: the list has no 30 of level 1),
    once in one launch and once in three."""
    small = [g["case"] for g in golden["cases"] if g["res"] == C.OK
             and C.size_of(g["case"]) <= 6000 and g["case"]["dict"] in (4096, 1 << 16)]
    cases = sorted(small, key=lambda c: c["level"] != 1)[:30]
    assert len(cases) == 30 and sum(c["level"] == 1 for c in cases) == 13
    assert len({C.size_of(c) for c in cases}) > 20 and sum(C.size_of(c) == 0 for c in cases) == 3
    r, order, ws = L.enc2_plan(host_batch(L, cases, golden, 0)[3], len(cases))
    assert r == 0 and order != sorted(order)
    limit = ws // 3 + (1 << 20)             # three launches
    assert 2 * limit < ws < 3 * limit
    r1, res1, out1, descs = host_batch(L, cases, golden, 0)
    r3, res3, out3, _ = host_batch(L, cases, golden, limit)
    assert r1 == 0 and r3 == 0, L.last_error()
    assert res1 == res3 == [(C.OK, want_of(c, golden)["len"] - 1) for c in cases]
    assert out1 == out3
    at = 0
    for c, q, (_, dl) in zip(cases, descs, res1):
        assert out1[at:q.dst_off] == bytes([POISON]) * (q.dst_off - at)
        C.check_block((C.OK, dl, desc_of(L, c)[2], out1[q.dst_off:q.dst_off + dl]),
                      want_of(c, golden), C.key(c))
        at = q.dst_off + q.dst_cap          # a block may use all of its slot on the way
    assert out1[at:] == bytes([POISON]) * (len(out1) - at)
    # one block alone over the limit, a range outside the buffers, nothing to do
    r, _, out, _ = host_batch(L, cases, golden, 1 << 16)
    assert r == 2 and out == bytes([POISON]) * len(out)
    assert host_batch(L, [], golden, 0)[0] == 0
    assert host_batch(L, [], golden, limit)[0] == 0
    d = (L.EncStreamDesc * 1)(raw_desc(L, src_len=10, dst_cap=10))
    assert L.lzma2_encode_batch_host(d, 1, b"123456789", bytes(10))[0] == C.PARAM
    d = (L.EncStreamDesc * 1)(raw_desc(L, src_len=9, dst_off=1, dst_cap=10))
    assert L.lzma2_encode_batch_host(d, 1, b"123456789", bytes(10), limit)[0] == C.PARAM


def test_multi_block_buffer(L, golden):
    """LzmaGpu_Lzma2EncodeHost: 300,000 bytes of text and 70,000 random at
    blockSize 100,000 is the reference's multi-threaded layout."""
    c, block = C.MULTIBLOCK[0]
    data = C.data_of(c)
    m = C.expect_multiblock(c, block, golden)
    t0 = time.monotonic()
    r, prop, out = L.Lzma2EncodeHost(data, L.enc2_props(1, 1 << 16, block_size=block),
                                     len(data) + 4096)
    assert time.monotonic() - t0 < STEP_LIMIT_S
    assert r == 0, L.last_error()
    assert (prop, len(out), C.sha(out)) == (m["prop"], m["len"], m["sha256"])
    blocks = L.split_lzma2_blocks(out)
    assert [u for _, _, u in blocks] == [100000, 100000, 100000, 70000]
    assert [n for _, n, _ in blocks][:3] == [b["len"] for b in m["blocks"]][:3]
    assert [C.sha(out[o:o + b["len"]]) for (o, _, _), b in zip(blocks, m["blocks"])] == \
        [b["sha256"] for b in m["blocks"]]
    assert C.decode_raw(out, prop) == data
    items = [dict(src_off=0, src_len=len(out), dst_off=0, dst_cap=len(data), props=bytes([prop]),
                  kind=L.KIND_LZMA2)]
    r, res, back = L.decode_batch_host(L.make_descs(items), out, len(data))
    assert (r, res[0].res, res[0].dest_len) == (0, 0, len(data)) and back == data
    # the Python forms, a short destination, the empty source
    assert L.lzma2_compress(data, dict_size=1 << 16, block_size=block) == (prop, out)
    assert L.Lzma2EncodeHost(data, L.enc2_props(1, 1 << 16, block_size=block), len(out) - 1)[0] \
        == C.OUTPUT_EOF
    assert L.Lzma2EncodeHost(b"", L.enc2_props(1), 1) == (0, 8, b"\0")
    assert L.Lzma2EncodeHost(b"", L.enc2_props(1), 0)[0] == C.OUTPUT_EOF
    got = L.lzma2_encode_batch([data[:100000], b"", data[300000:]], dict_size=1 << 16)
    assert [(r, p, len(b), C.sha(b)) for r, p, b in got] == [
        (0, prop, m["blocks"][0]["len"], m["blocks"][0]["sha256"]), (0, prop, 0, C.sha(b"")),
        (0, prop, m["blocks"][3]["len"], m["blocks"][3]["sha256"])]


def compact(L, lens, slot_base, out_base, fail=None, short=0):
    """Lzma2EncGpu_Compact over hand-made slots at odd offsets; returns
    (total, offsets, the poisoned output buffer)."""
    import torch
    n = len(lens)
    slots = bytearray(b"\x11" * slot_base)
    descs = (L.EncStreamDesc * max(n, 1))()
    res = (L.EncResult * max(n, 1))()
    parts = []
    for i, ln in enumerate(lens):
        body = bytes((7 * i + 3 * k + (k >> 8)) & 0xFF for k in range(ln))
        descs[i].dst_off, descs[i].dst_cap = len(slots), ln + 3
        res[i].res, res[i].dest_len = (fail[1] if fail and fail[0] == i else 0), ln
        slots += body + b"\x22" * (3 + (ln + 1) % 2 + 2 * (i % 3))
        parts.append(body)
    want = b"".join(parts) + b"\0"
    cap = len(want) - short
    d_desc, d_res, d_slots = dev(bytes(descs)), dev(bytes(res)), dev(slots + b"\x33" * 64)
    d_out = torch.full((out_base + len(want) + 64,), POISON, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    d_tot = torch.full((16,), 0xEE, dtype=torch.uint8, device="cuda")
    r = L.lzma2_compact_device(d_desc.data_ptr(), d_res.data_ptr(), n, d_slots.data_ptr(),
                               d_out.data_ptr() + out_base, cap, d_off.data_ptr(),
                               d_tot.data_ptr())
    torch.cuda.synchronize()
    assert r == 0, L.last_error()
    tot = L.EncResult.from_buffer_copy(d_tot.cpu().numpy().tobytes())
    return tot, d_off.cpu().tolist(), d_out.cpu().numpy().tobytes(), want


def test_compaction_alone(L):
    lens = [0, 1, 15, 16, 17, 70001, 0, 33]
    starts = [sum(lens[:i]) for i in range(len(lens) + 1)]
    for slot_base, out_base in ((1, 1), (3, 8), (16, 5), (7, 16), (9, 15), (12, 2)):
        tot, offs, out, want = compact(L, lens, slot_base, out_base)
        assert (tot.res, tot.dest_len) == (0, len(want)) and offs == starts
        assert out[:out_base] == bytes([POISON]) * out_base
        assert out[out_base:out_base + len(want)] == want, (slot_base, out_base)
        assert out[out_base + len(want):] == bytes([POISON]) * 64
    # a failed block, a short destination: the verdict, and nothing written
    tot, offs, out, want = compact(L, lens, 1, 1, fail=(4, C.OUTPUT_EOF))
    assert (tot.res, tot._pad, tot.dest_len) == (C.OUTPUT_EOF, 4, len(want))
    assert out == bytes([POISON]) * len(out)
    tot, offs, out, want = compact(L, lens, 1, 1, short=1)
    assert (tot.res, tot.dest_len) == (C.OUTPUT_EOF, len(want)) and offs == starts
    assert out == bytes([POISON]) * len(out)
    tot, offs, out, want = compact(L, [], 1, 3)
    assert (tot.res, tot.dest_len, offs, want) == (0, 1, [0], b"\0")
    assert out[3:4] == b"\0" and out[:3] + out[4:] == bytes([POISON]) * (len(out) - 1)


class MemStreams:
    """ISeqInStream / ISeqOutStream / ICompressProgress over Python buffers."""

    def __init__(self, L, data, read_step=50000, fail_read_at=None, short_write_at=None,
                 refuse_progress_at=None):
        self.data, self.pos, self.out, self.progress, self.reads, self.writes = data, 0, [], [], 0, 0

        def read(p, buf, size):
            self.reads += 1
            if fail_read_at is not None and self.reads > fail_read_at:
                return 8
            n = min(size[0], read_step, len(self.data) - self.pos)
            ctypes.memmove(buf, self.data[self.pos:self.pos + n], n)
            self.pos += n
            size[0] = n
            return 0

        def write(p, buf, size):
            self.writes += 1
            if short_write_at is not None and self.writes > short_write_at:
                return size - 1 if size else 0
            self.out.append(ctypes.string_at(buf, size))
            return size

        def progress(p, in_size, out_size):
            self.progress.append((in_size, out_size))
            return 1 if refuse_progress_at is not None and len(self.progress) > refuse_progress_at \
                else 0
        self.keep = (L.SeqRead(read), L.SeqWrite(write), L.ProgressFn(progress))
        self.inp = L.ISeqInStream(self.keep[0])
        self.outp = L.ISeqOutStream(self.keep[1])
        self.prog = L.ICompressProgress(self.keep[2])


def dropin_encode(L, props, s, with_progress=True):
    h = L.lib.Lzma2Enc_Create(ctypes.byref(L.g_alloc), ctypes.byref(L.g_alloc))
    assert h
    try:
        assert L.lib.Lzma2Enc_SetProps(h, ctypes.byref(props)) == 0
        prop = L.lib.Lzma2Enc_WriteProperties(h)
        r = L.lib.Lzma2Enc_Encode(h, ctypes.byref(s.outp), ctypes.byref(s.inp),
                                  ctypes.byref(s.prog) if with_progress else None)
        return r, prop
    finally:
        L.lib.Lzma2Enc_Destroy(h)


def test_lzma2enc_dropins_through_memory_streams(L, golden):
    c, block = C.MULTIBLOCK[2]                  # 70,000 bytes of text, dict 4 KiB, 4 blocks
    assert c in C.edge_cases()
    data, w, m = C.data_of(c), want_of(c, golden), C.expect_multiblock(c, block, golden)
    # numBlockThreads 1: the whole input is one block, Lzma2Enc_EncodeMt1's stream
    s = MemStreams(L, data)
    r, prop = dropin_encode(L, L.enc2_props(1, 4096, block_size=block, block_threads=1), s)
    out = b"".join(s.out)
    assert (r, prop, len(out), C.sha(out)) == (0, w["prop"], w["len"], w["sha256"])
    assert s.progress == [(len(data), len(out) - 1)]
    # numBlockThreads 4: blocks of blockSize, whatever the thread count
    for threads in (4, 2):
        s = MemStreams(L, data, read_step=7777)
        r, prop = dropin_encode(L, L.enc2_props(1, 4096, block_size=block, block_threads=threads),
                                s)
        out = b"".join(s.out)
        assert (r, prop, len(out), C.sha(out)) == (0, m["prop"], m["len"], m["sha256"])
        ends, at = [], 0
        for b in m["blocks"]:
            at += b["len"]
            ends.append(at)
        assert s.progress == list(zip((20000, 40000, 60000, 70000), ends))
        assert C.decode_raw(out, prop) == data
    # an empty input: the byte 00, no progress call
    s = MemStreams(L, b"")
    assert dropin_encode(L, L.enc2_props(1, block_threads=4), s)[0] == 0
    assert b"".join(s.out) == b"\0" and s.progress == []
    # the stream errors
    p4 = L.enc2_props(1, 4096, block_size=block, block_threads=4)
    assert dropin_encode(L, p4, MemStreams(L, data, fail_read_at=1))[0] == 8        # READ
    assert dropin_encode(L, p4, MemStreams(L, data, short_write_at=2))[0] == 9      # WRITE
    s = MemStreams(L, data, short_write_at=4)   # the final 0x00
    assert dropin_encode(L, p4, s)[0] == 9 and len(s.out) == 4
    s = MemStreams(L, data, refuse_progress_at=1)
    assert dropin_encode(L, p4, s)[0] == 10 and len(s.out) == 2                     # PROGRESS
    assert dropin_encode(L, p4, MemStreams(L, data), with_progress=False)[0] == 0
    assert dropin_encode(L, L.enc2_props(5), MemStreams(L, data))[0] == C.UNSUPPORTED


def ref_xz_decode(data, cap):
    lib = native.ref_cont()
    f = lib.ref_xz_decode
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_char_p, native.size_t_p, ctypes.c_char_p, native.size_t_p,
                  native.int_p, native.int_p]
    out = ctypes.create_string_buffer(max(cap, 1))
    dl, sl = ctypes.c_size_t(cap), ctypes.c_size_t(len(data))
    st, done = ctypes.c_int(-1), ctypes.c_int(0)
    res = f(out, ctypes.byref(dl), data, ctypes.byref(sl), ctypes.byref(st), ctypes.byref(done))
    return res, out.raw[:dl.value], done.value


@pytest.mark.parametrize("check", [0, 1, 4, 10])
def test_xz_writer(L, golden, check):
    c, block = C.MULTIBLOCK[1]                  # 250,000 bytes of text, blocks of 65,536
    data, m = C.data_of(c), C.expect_multiblock(c, block, golden)
    props = L.enc2_props(1, 1 << 16, block_size=block)
    t0 = time.monotonic()
    r, xz = L.XzEncode(data, props, check, len(data) + 4096)
    assert time.monotonic() - t0 < STEP_LIMIT_S
    assert r == 0, L.last_error()
    r, blocks, total = L.xz_index(xz)
    assert (r, total, len(blocks)) == (0, len(data), 4)
    csize = xzwrite.CHECK_SIZE[check]
    at = 12
    for i, (b, want) in enumerate(zip(blocks, m["blocks"])):
        piece = data[i * block:(i + 1) * block]
        assert (b.header_off, b.data_off, b.unpack_size, b.dst_off) == (at, at + 12, len(piece),
                                                                        i * block)
        assert (b.check_type, b.check_size, b.lzma2_prop, b.num_filters) == (check, csize,
                                                                             m["prop"], 0)
        # the block's LZMA2 data: the reference's chunks of the slice, then 0x00
        assert b.pack_size == want["len"] + 1
        body = xz[b.data_off:b.data_off + b.pack_size]
        assert body[-1] == 0 and C.sha(body[:-1]) == want["sha256"]
        pad = -b.pack_size % 4
        assert xz[b.data_off + b.pack_size:b.check_off] == b"\0" * pad
        assert xz[b.check_off:b.check_off + csize] == xzwrite.check_value(check, piece)
        at = b.check_off + csize
    assert lzma.decompress(xz, format=lzma.FORMAT_XZ) == data
    assert L.XzDecode(xz, len(data)) == (0, data, -1)
    if os.path.exists(native.REF_CONT_SO):
        assert ref_xz_decode(xz, len(data) + 16) == (0, data, 1)
    assert L.xz_compress(data, check=check, dict_size=1 << 16, block_size=block) == xz
    assert L.XzEncode(data, props, check, len(xz) - 1)[0] == C.OUTPUT_EOF
    # the empty file: header, an index of no records, footer
    r, empty = L.XzEncode(b"", props, check, 32)
    assert r == 0 and empty == xzwrite.make_stream([], check) and len(empty) == 32
    assert lzma.decompress(empty, format=lzma.FORMAT_XZ) == b""
    assert L.XzDecode(empty, 16) == (0, b"", -1)
    assert L.XzEncode(b"", props, check, 31)[0] == C.OUTPUT_EOF
    assert L.XzEncode(data, props, 2, len(data) + 4096)[0] == C.UNSUPPORTED

"""LzmaEncGpu_EncodeBatch / EncodeBatchHost and the LzmaEncode / LzmaCompress
drop-ins on the device against the reference's LzmaEncode: live
(oracle/_ref/libref_lzma.so) where it is built, else the committed goldens.
Equality is the criterion everywhere: output bytes, res, dest_len, the 5 props
bytes, and every byte of the destination outside a stream's written range keeps
its poison.  Every stream that ends SZ_OK is decoded again on the GPU."""
import ctypes
import os
import sys
import time

import pytest

import lzmaenc_cases as C
import native

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
    """The reference's result for a case, computed once and shared."""
    k = C.key(c)
    if k not in _want:
        _want[k] = C.expect(c, golden=golden)
    return _want[k]


def desc_of(L, c):
    p = L.enc_props(c["level"], c["dict"], c["lc"], c["lp"], c["pb"], c["fb"], c["mc"], c["algo"],
                    c["bt"])
    return L.enc_desc_from_props(p, c["end_mark"])


def raw_desc(L, **kw):
    """A descriptor written by hand (what DescFromProps would refuse)."""
    d = L.EncStreamDesc()
    d.dict_size, d.lc, d.lp, d.pb, d.fb, d.mc = 1 << 16, 3, 0, 2, 32, 16
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def run_device(L, items, lanes=0, planned_order=True):
    """items: (EncStreamDesc with props set, data, cap).  One LzmaEncGpu_EncodeBatch
    with byte-odd offsets, a poisoned destination and a poisoned workspace.
    Returns [(res, dest_len, written bytes)], having checked that the poison
    outside each written range is intact."""
    import numpy as np
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
    r, order, ws = L.enc_plan(descs, n)
    assert r == 0 and sorted(order) == list(range(n))
    lens = [descs[k].src_len for k in order]
    assert lens == sorted(lens, reverse=True)
    assert all(descs[i].ws_off % 256 == 0 for i in range(n))

    def dev(b):
        return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()
    d_desc = dev(bytes(descs))
    d_order = dev(bytes((ctypes.c_uint32 * max(n, 1))(*order)))
    d_src = dev(src)
    d_dst = torch.full((dst_off + 64,), POISON, dtype=torch.uint8, device="cuda")
    d_ws = torch.full((max(ws, 256),), 0x3C, dtype=torch.uint8, device="cuda")
    d_res = torch.full((max(n, 1) * 16,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.monotonic()
    r = L.encode_batch_device(d_desc.data_ptr(), d_order.data_ptr() if planned_order else 0, n,
                              d_src.data_ptr(), d_dst.data_ptr(), d_ws.data_ptr(),
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
        at = d.dst_off + q.dest_len
        got.append((q.res, q.dest_len, out[d.dst_off:at]))
    assert out[at:] == bytes([POISON]) * (len(out) - at)
    return got


def encode_cases(L, cases, golden, lanes=0, planned_order=True, extra=()):
    """Encodes the cases (plus hand-made (desc, data, cap, want) extras) in one
    batch and checks each against the reference.  Returns the round-trip work:
    [(props5, packed, data)] of the streams that ended SZ_OK."""
    items, wants = [], []
    for c in cases:
        w = want_of(c, golden)
        r, d, props5 = desc_of(L, c)
        assert r == (w["res"] if w["res"] in (C.PARAM, C.UNSUPPORTED) else 0), C.key(c)
        if r != 0:
            continue            # refused on the host: nothing reaches the device
        assert props5 == w["props5"], C.key(c)
        items.append((d, C.data_of(c), w["cap"]))
        wants.append((c, w))
    at = {}
    for pos, d, data, cap, res in extra:
        at[pos] = (d, data, cap, res)
    for pos in sorted(at):
        d, data, cap, res = at[pos]
        items.insert(pos, (d, data, cap))
        wants.insert(pos, (None, res))
    got = run_device(L, items, lanes, planned_order)
    back = []
    for k, ((c, w), g) in enumerate(zip(wants, got)):
        if c is None:
            assert g == (w, 0, b""), (k, g[:2])
            continue
        C.check((g[0], g[1], w["props5"], g[2]), w, C.key(c))
        if g[0] == C.OK:
            back.append((w["props5"], g[2], items[k][1]))
    return back


def round_trip(L, back):
    """Every (props5, packed, data) decodes through LzmaGpu_DecodeBatchHost."""
    if not back:
        return
    src, items, dst_off = bytearray(), [], 0
    for props5, packed, data in back:
        items.append(dict(src_off=len(src), src_len=len(packed), dst_off=dst_off,
                          dst_cap=len(data), props=props5))
        src += packed
        dst_off += len(data)
    r, res, out = L.decode_batch_host(L.make_descs(items), bytes(src), dst_off)
    assert r == 0, L.last_error()
    for k, (it, (_, _, data)) in enumerate(zip(items, back)):
        assert (res[k].res, res[k].dest_len) == (0, len(data)), (k, res[k].res, res[k].dest_len)
        assert out[it["dst_off"]:it["dst_off"] + len(data)] == data, k


def test_distant_case_has_a_match_beyond_the_short_distance_slots(golden):
    """The 40 KiB case repeats a 2 KiB incompressible block 35 KiB back (a
    distance slot >= kEndPosModelIndex: direct bits and the align tree): with a
    different second block the reference needs about 2 KiB more."""
    c = C.case("distant", 11, 40 * 1024, dict=1 << 16)
    assert c in C.edge_cases()
    with_match = want_of(c, golden)["dest_len"]
    assert C.gen("distant", 11, 40 * 1024)[:2048] == C.gen("distant", 11, 40 * 1024)[35840:37888]
    if native.have_ref():
        ctl = C.ref_expect(dict(c, kind="distant_ctl"))[1]
        assert ctl - with_match > 1900, (ctl, with_match)


def test_every_edge_case_in_one_planned_batch(L, golden):
    """Short sources, repeated bytes, the dictionary wrap, the distant match, the
    incompressible source at six capacities, the props corners, mc 1 / 4 / 48,
    clamped fb, sources of dictSize and dictSize + 1 bytes -- in the planner's
    longest-first order at the default lanes; then the round trip."""
    back = encode_cases(L, C.edge_cases(), golden)
    assert len(back) == 59      # 71 cases: 7 refused on the host, 5 overflows
    round_trip(L, back)


def mixed_cases():
    ec = C.edge_cases()
    pick = [c for c in ec if c["n"] <= 20000 and c["level"] < 5 and c["algo"] < 0 and c["bt"] < 0
            and c["lc"] < 9 and c["lp"] < 5 and c["pb"] < 5 and c["dict"] <= 1 << 30]
    rnd = [C.case("random", 12, 70 * 1024, dict=1 << 16, cap=cap)
           for cap in (65535, "full+0", 5, 0)]
    far = C.case("distant", 11, 40 * 1024, dict=1 << 16)
    assert len(pick) == 57 and all(c in ec for c in rnd + [far])
    return pick[:2] + [rnd[0], C.case("text", 100, 0)] + pick[2:] + rnd[1:] + [far]


@pytest.mark.parametrize("lanes", [64, 32, 16])
def test_mixed_batch_of_65_streams_in_index_order(L, golden, lanes):
    """One full wave plus one stream at lanes == 64, different lengths and
    props, odd offsets; an overflow, an empty and two rejected items sit in the
    first 16 lanes of the first wave."""
    rejected = [(4, raw_desc(L, lc=9), b"abcdefgh", 64, C.PARAM),
                (5, raw_desc(L, src_len=1 << 31), b"", 64, C.UNSUPPORTED)]
    cases = mixed_cases()
    assert len(cases) + len(rejected) == 65
    back = encode_cases(L, cases, golden, lanes=lanes, planned_order=False, extra=rejected)
    if lanes == 64:
        round_trip(L, back)


def test_single_streams_and_the_empty_batch(L, golden):
    assert run_device(L, []) == []
    for c in (C.case("text", 13, 3000, lc=8, lp=4, pb=4, end_mark=1), C.case("text", 100, 0),
              C.case("copy", 10, 20000, dict=4096)):
        assert c in C.edge_cases()
        round_trip(L, encode_cases(L, [c], golden))
    # what the kernel itself refuses, alone
    for kw, res in ((dict(lc=9), C.PARAM), (dict(lp=5), C.PARAM), (dict(pb=5), C.PARAM),
                    (dict(fb=4), C.PARAM), (dict(fb=274), C.PARAM), (dict(dict_size=0), C.PARAM),
                    (dict(dict_size=(1 << 30) + 1), C.PARAM), (dict(src_len=1 << 31),
                                                               C.UNSUPPORTED)):
        assert run_device(L, [(raw_desc(L, **kw), b"abcdefgh", 64)]) == [(res, 0, b"")], kw
    assert L.lib.LzmaEncGpu_EncodeBatch(None, None, 0, None, None, None, None, 0, None) == 0
    assert L.lib.LzmaEncGpu_EncodeBatch(None, None, 1, None, None, None, None, 48, None) == C.PARAM


def fuzz_cases(golden):
    if native.have_ref():
        return C.random_cases(512, 424242, max_n=8192)
    cases = [g["case"] for g in golden["cases"] if g["case"]["n"] <= 8192]
    return (cases * (512 // len(cases) + 1))[:512]


def test_fuzz_512_streams(L, golden):
    cases = fuzz_cases(golden)
    assert len(cases) == 512 and max(c["n"] for c in cases) <= 8192
    round_trip(L, encode_cases(L, cases, golden))


def test_dropins_against_the_reference(L, golden):
    c = C.case("text", 9, 4097, dict=4096)
    assert c in C.edge_cases()
    w, data = want_of(c, golden), C.data_of(c)
    got = L.LzmaCompress(data, w["cap"], level=1, dict_size=4096)
    assert got == (C.OK, w["dest_len"], w["props5"], got[3]) and C.sha(got[3]) == w["sha256"]
    got = L.LzmaEncode(data, L.enc_props(1, 4096), w["cap"])
    assert got[:3] == (C.OK, w["dest_len"], w["props5"]) and C.sha(got[3]) == w["sha256"]
    c = C.case("text", 13, 3000, lc=0, lp=4, pb=4, end_mark=1)
    w, data = want_of(c, golden), C.data_of(c)
    got = L.LzmaEncode(data, L.enc_props(1, 0, 0, 4, 4), w["cap"], end_mark=True)
    assert got[:3] == (C.OK, w["dest_len"], w["props5"]) and C.sha(got[3]) == w["sha256"]
    # overflow: the first cap bytes, dest_len == cap
    c = C.case("random", 12, 70 * 1024, dict=1 << 16, cap=65535)
    w, data = want_of(c, golden), C.data_of(c)
    got = L.LzmaCompress(data, 65535, level=1, dict_size=1 << 16)
    assert got[:2] == (C.OUTPUT_EOF, 65535) and C.sha(got[3]) == w["sha256"]
    # the documented differences, and the reference's own refusals
    got = L.LzmaCompress(data[:500], 2000)                      # the default level 5
    assert got == (C.UNSUPPORTED, 2000, b"\0" * 5, b"")
    assert "optimal parser" in L.last_error()
    assert L.LzmaEncode(data[:500], L.enc_props(1, algo=1), 2000)[0] == C.UNSUPPORTED
    assert L.LzmaEncode(data[:500], L.enc_props(1, lc=9), 2000) == (C.PARAM, 2000, b"\0" * 5, b"")
    assert L.LzmaEncode(data[:500], L.enc_props(1), 2000, props_size=4)[0] == C.PARAM
    # encode_batch: the Python form of the host call
    items = [C.data_of(k) for k in (C.case("text", 9, 4097, dict=4096),
                                    C.case("copy", 10, 4095, dict=4096))]
    for (res, props5, packed), k in zip(L.encode_batch(items, level=1, dict_size=4096),
                                        (C.case("text", 9, 4097, dict=4096),
                                         C.case("copy", 10, 4095, dict=4096))):
        w = want_of(k, golden)
        assert (res, props5, len(packed), C.sha(packed)) == (C.OK, w["props5"], w["dest_len"],
                                                             w["sha256"])


def host_batch(L, cases, golden, limit):
    src, dst_off = bytearray(b"\x5a"), 3
    descs = (L.EncStreamDesc * len(cases))()
    for i, c in enumerate(cases):
        r, d, _ = desc_of(L, c)
        assert r == 0
        ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(d), ctypes.sizeof(d))
        data, cap = C.data_of(c), want_of(c, golden)["cap"]
        descs[i].src_off, descs[i].src_len, descs[i].dst_off, descs[i].dst_cap = (
            len(src), len(data), dst_off, cap)
        src += data
        dst_off += cap + 1
    t0 = time.monotonic()
    r, res, out = L.encode_batch_host(descs, len(cases), bytes(src),
                                      bytes([POISON]) * (dst_off + 5), limit)
    assert time.monotonic() - t0 < STEP_LIMIT_S
    return r, [(q.res, q.dest_len) for q in list(res)[:len(cases)]], out, descs


def test_host_call_splits_launches_by_the_workspace_limit(L, golden):
    cases = [c for c in C.edge_cases() if c["dict"] in (0, 4096) and c["n"] <= 6000
             and c["level"] == 1 and c["algo"] < 0 and c["bt"] < 0 and max(c["lc"], c["lp"]) < 4
             and c["pb"] < 5][:30]
    assert len(cases) == 30
    r, order, ws = L.enc_plan(host_batch(L, cases, golden, 0)[3], len(cases))
    limit = ws // 3 + (1 << 20)             # three launches
    assert 2 * limit < ws < 3 * limit
    r1, res1, out1, descs = host_batch(L, cases, golden, 0)
    r3, res3, out3, _ = host_batch(L, cases, golden, limit)
    assert r1 == 0 and r3 == 0, L.last_error()
    assert res1 == res3 == [(want_of(c, golden)["res"], want_of(c, golden)["dest_len"])
                            for c in cases]
    assert out1 == out3
    at = 0
    for c, q, (_, dl) in zip(cases, descs, res1):
        assert out1[at:q.dst_off] == bytes([POISON]) * (q.dst_off - at)
        at = q.dst_off + dl
        assert C.sha(out1[q.dst_off:at]) == want_of(c, golden)["sha256"]
    assert out1[at:] == bytes([POISON]) * (len(out1) - at)
    # one stream alone over the limit, a range outside the buffers, nothing to do
    r, _, out, _ = host_batch(L, cases, golden, 1 << 16)
    assert r == 2 and out == bytes([POISON]) * len(out)
    assert host_batch(L, [], golden, 0)[0] == 0
    d = (L.EncStreamDesc * 1)(raw_desc(L, src_len=10, dst_cap=10))
    assert L.encode_batch_host(d, 1, b"123456789", bytes(10))[0] == C.PARAM

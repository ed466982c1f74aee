"""Lzma86Gpu_EncodeBatch / EncodeBatchHost / DecodeBatch / DecodeBatchHost and
the Lzma86_Encode / Lzma86_Decode / Lzma86_GetUnpackSize drop-ins on the device
against the expectation lzma86_cases.compose() builds from the reference's own
primitives.  Equality is the criterion: res, dest_len, every byte of
[dst_off, dst_off + dest_len), and every byte of the destination outside it
keeps its poison."""
import ctypes
import os
import sys

import pytest

import lzma86_cases as C
import native

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))

pytestmark = pytest.mark.gpu
POISON = 0xA5


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


@pytest.fixture(scope="module")
def cases():
    """Every stream under every filter mode and the capacity cases: one batch."""
    return C.mode_cases() + C.capacity_cases()


def layout(L, cases):
    """Byte-odd offsets, two guard bytes at least between the slots."""
    src, items, dst_off = bytearray(b"\x5a"), [], 1
    for c in cases:
        data, cap = C.src_of(c), C.cap_of(c)
        items.append(dict(src_off=len(src), src_len=len(data), dst_off=dst_off, dst_cap=cap,
                          level=c["level"], dict_size=c["dict"], mode=c["mode"]))
        src += data + b"\x5a" * (2 + len(data) % 2)
        dst_off += cap + 2 + cap % 2
    return L.lzma86_descs(items), bytes(src), dst_off + 64


def check_encoded(cases, descs, res, out):
    """Results and bytes against compose(); the poison around every written range."""
    at = 0
    for k, c in enumerate(cases):
        want, q, d = C.expect(c), res[k], descs[k]
        assert (q.res, q.dest_len) == want[:2], (c["name"], q.res, q.dest_len, want[:2])
        assert out[at:d.dst_off] == bytes([POISON]) * (d.dst_off - at), c["name"]
        at = d.dst_off + q.dest_len
        assert out[d.dst_off:at] == want[2], c["name"]
        if q.dest_len:
            assert q.filter == want[2][0], c["name"]
    assert out[at:] == bytes([POISON]) * (len(out) - at)


def dev(b):
    import numpy as np
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def encode_device(L, cases):
    import torch
    n = len(cases)
    descs, src, dst_size = layout(L, cases)
    r, scratch = L.lzma86_encode_scratch(descs, n)
    assert r == 0 and scratch > 0
    d_src = dev(src)
    d_dst = torch.full((dst_size,), POISON, dtype=torch.uint8, device="cuda")
    d_scratch = torch.full((scratch,), 0x3C, dtype=torch.uint8, device="cuda")
    d_res = torch.full((n * 24,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = L.lzma86_encode_batch_device(descs, n, d_src.data_ptr(), d_dst.data_ptr(),
                                     d_scratch.data_ptr(), scratch, d_res.data_ptr())
    torch.cuda.synchronize()
    assert r == 0, L.last_error()
    res = (L.Lzma86Result * n).from_buffer_copy(d_res.cpu().numpy().tobytes())
    return descs, res, d_dst.cpu().numpy().tobytes()


_encoded = {}


def encoded(L, cases):
    """The device batch over all cases, run once and shared."""
    if "all" not in _encoded:
        _encoded["all"] = encode_device(L, cases)
    return _encoded["all"]


def test_the_streams_are_what_the_cases_say():
    """The filter wins on the code, ties on the text and loses on the noise, by
    the reference's own sizes."""
    u, f = C.candidate_sizes(C.data_of(*C.FIXED), 1, 0)
    assert f < u
    t = C.data_of("text", 32, 5000)
    assert b"\xE8" not in t and b"\xE9" not in t and C.ref_x86(t, 1) == t
    u, f = C.candidate_sizes(C.data_of(*C.FIXED_U), 1, 0)
    assert u < f
    tail = C.data_of("tail", 35, 777)
    assert 0xE8 in tail[-5:]
    by_name = {c["name"]: C.expect(c) for c in C.mode_cases()}
    assert by_name["code/2"][2][0] == 1 and by_name["text/2"][2][0] == 0
    assert by_name["noise/2"][2][0] == 0 and by_name["text/1"][2][0] == 1
    caps = {c["name"].split("/", 1)[1]: C.expect(c)[:2] for c in C.capacity_cases()}
    assert caps["code/13"] == (C.OUTPUT_EOF, 0) and caps["code/14"] == (C.OUTPUT_EOF, 14)
    assert sorted(v[0] for v in caps.values()) == [0, 0, 0, 7, 7, 7]


def test_every_case_in_one_device_batch(L, cases):
    """Mixed filter modes, lengths 0..4,097, an E8 in the last five bytes and six
    capacities in one Lzma86Gpu_EncodeBatch."""
    assert len(cases) == 36
    descs, res, out = encoded(L, cases)
    check_encoded(cases, descs, res, out)


def test_host_batch_and_the_workspace_limit(L, cases):
    """Lzma86Gpu_EncodeBatchHost in one launch and, under a workspace limit of
    about 40 % of the candidates' slices, in several: the same bytes."""
    n = len(cases)
    descs, src, dst_size = layout(L, cases)
    one = L.Lzma86Stats()
    r1, res1, out1 = L.lzma86_encode_batch_host(descs, n, src, bytes([POISON]) * dst_size, 0, one)
    assert r1 == 0, L.last_error()
    check_encoded(cases, descs, res1, out1)
    want_cands = sum((2 if c["mode"] == C.AUTO else 1) for c in cases if C.cap_of(c) >= 14)
    assert (one.candidates, one.encode_launches) == (want_cands, 1)
    assert one.filtered == sum(1 for c in cases if c["mode"] != C.NO and C.cap_of(c) >= 14)
    # the candidates' slices, by the LZMA encoder's own planner
    r, proto, _ = L.enc_desc_from_props(L.enc_props(1, 0))
    assert r == 0
    total = 0
    for c in cases:
        if C.cap_of(c) < 14:
            continue
        e = (L.EncStreamDesc * 1)()
        ctypes.memmove(e, ctypes.byref(proto), ctypes.sizeof(proto))
        e[0].src_len = c["n"]
        total += L.enc_plan(e, 1)[2] * (2 if c["mode"] == C.AUTO else 1)
    cut = L.Lzma86Stats()
    r2, res2, out2 = L.lzma86_encode_batch_host(descs, n, src, bytes([POISON]) * dst_size,
                                                total * 2 // 5, cut)
    assert r2 == 0, L.last_error()
    assert cut.encode_launches >= 2 and cut.candidates == want_cands
    assert out2 == out1
    assert [(q.res, q.dest_len, q.filter) for q in res2] == [(q.res, q.dest_len, q.filter)
                                                              for q in res1]
    # one stream's candidates alone over the limit; a range outside the buffers
    assert L.lzma86_encode_batch_host(descs, n, src, bytes(dst_size), 1 << 12)[0] == 2
    bad = L.lzma86_descs([dict(src_off=0, src_len=10, dst_off=0, dst_cap=100)])
    assert L.lzma86_encode_batch_host(bad, 1, b"123456789", bytes(100))[0] == C.PARAM
    assert L.lzma86_encode_batch_host(bad, 0, b"", b"")[0] == 0


def test_level_5_needs_the_modes_mask(L):
    """One 2 KiB stream at level 5 with a 64 KiB dictionary: with the mask at 3 the
    reference's bytes, with the default mask SZ_ERROR_UNSUPPORTED."""
    c = C.case("code5", "code", 36, 2048, C.AUTO, level=5, dict_size=1 << 16)
    descs, src, dst_size = layout(L, [c])
    assert L.enc_get_modes() == 0
    r, res, out = L.lzma86_encode_batch_host(descs, 1, src, bytes([POISON]) * dst_size)
    assert r == 0 and (res[0].res, res[0].dest_len) == (C.UNSUPPORTED, 0)
    assert out == bytes([POISON]) * dst_size
    prev = L.enc_set_modes(3)
    try:
        r, res, out = L.lzma86_encode_batch_host(descs, 1, src, bytes([POISON]) * dst_size)
    finally:
        L.enc_set_modes(prev)
    assert r == 0, L.last_error()
    check_encoded([c], descs, res, out)
    assert res[0].filter == 1


def decode_items(cases, descs, res, out, cut=None):
    """The streams that ended SZ_OK as decode items: (case, stream bytes, dest cap)."""
    items = []
    for k, c in enumerate(cases):
        if res[k].res == C.OK:
            items.append((c, out[descs[k].dst_off:descs[k].dst_off + res[k].dest_len], c["n"]))
    return items


def decode_device(L, items):
    """One Lzma86Gpu_DecodeBatch over (name, stream bytes, dest cap): results and
    the destination, having checked the poison between the slots."""
    import torch
    n = len(items)
    src, rows, dst_off = bytearray(b"\x5a"), [], 1
    for _, stream, cap in items:
        rows.append(dict(src_off=len(src), src_len=len(stream), dst_off=dst_off, dst_cap=cap))
        src += stream + b"\x5a"
        dst_off += cap + 3
    descs = L.lzma86_descs(rows)
    headers = L.lzma86_headers(descs, n, bytes(src))
    r, scratch = L.lzma86_decode_scratch(descs, n, headers)
    assert r == 0
    d_src = dev(src)
    d_dst = torch.full((dst_off + 16,), POISON, dtype=torch.uint8, device="cuda")
    d_scratch = torch.full((max(scratch, 256),), 0x3C, dtype=torch.uint8, device="cuda")
    d_res = torch.full((n * 24,), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = L.lzma86_decode_batch_device(descs, n, headers, d_src.data_ptr(), d_dst.data_ptr(),
                                     d_scratch.data_ptr(), scratch, d_res.data_ptr())
    torch.cuda.synchronize()
    assert r == 0, L.last_error()
    res = (L.Lzma86Result * n).from_buffer_copy(d_res.cpu().numpy().tobytes())
    out = d_dst.cpu().numpy().tobytes()
    at, got = 0, []
    for k in range(n):
        d = descs[k]
        assert out[at:d.dst_off] == bytes([POISON]) * (d.dst_off - at), k
        assert res[k].dest_len <= d.dst_cap
        at = d.dst_off + res[k].dest_len
        got.append((res[k].res, res[k].dest_len, res[k].src_len, out[d.dst_off:at]))
    assert out[at:] == bytes([POISON]) * (len(out) - at)
    return got


def test_every_encoded_case_decodes_and_the_bad_headers(L, cases):
    descs, res, out = encoded(L, cases)
    items = decode_items(cases, descs, res, out)
    assert len(items) == 33
    code_stream = next(s for c, s, _ in items if c["name"] == "code/2")
    data = C.data_of(*C.FIXED)
    assert code_stream[0] == 1
    short_cap = 1000
    extra = [("flag2", b"\x02" + code_stream[1:], len(data)),
             ("13 bytes", code_stream[:13], len(data)),
             ("cut payload", code_stream[:len(code_stream) // 2], len(data)),
             ("short dest", code_stream, short_cap)]
    got = decode_device(L, items + extra)
    for (c, stream, _), g in zip(items, got):
        assert g == (C.OK, c["n"], len(stream), C.src_of(c)), c["name"]
    flag2, short13, cut, short_dest = got[len(items):]
    assert flag2[:3] == (C.UNSUPPORTED, 0, 0)
    assert short13[:3] == (C.INPUT_EOF, 0, 0)
    # the payload cut short: LzmaDecode's own verdict and lengths over half the
    # payload; Lzma86_Decode returns before the filter
    half = len(code_stream) // 2 - C.HEADER
    want = native.decode(native.ref(), "ref", code_stream[C.HEADER:C.HEADER + half],
                         code_stream[1:6], len(data), 0)
    assert want[0] == C.INPUT_EOF and 0 < want[2] < len(data)
    assert cut == (C.INPUT_EOF, want[2], C.HEADER + want[3], want[4])
    assert cut[3] != data[:want[2]]     # still filtered bytes
    # a dest shorter than the stored size: SZ_OK, a short dest_len, filtered
    want = native.decode(native.ref(), "ref", code_stream[C.HEADER:], code_stream[1:6], short_cap, 0)
    assert want[0] == C.OK and want[2] == short_cap
    assert short_dest == (C.OK, short_cap, C.HEADER + want[3], C.ref_x86(want[4], 0))
    # the host form over the same streams
    src, rows, dst_off = bytearray(), [], 0
    for _, stream, cap in items + extra:
        rows.append(dict(src_off=len(src), src_len=len(stream), dst_off=dst_off, dst_cap=cap))
        src += stream
        dst_off += cap
    d = L.lzma86_descs(rows)
    r, hres, hout = L.lzma86_decode_batch_host(d, len(rows), bytes(src), bytes(dst_off))
    assert r == 0, L.last_error()
    for k, g in enumerate(got):
        assert (hres[k].res, hres[k].dest_len, hres[k].src_len) == g[:3], k
        assert hout[d[k].dst_off:d[k].dst_off + g[1]] == g[3], k


def test_dropins_on_the_code_stream(L):
    c = C.case("code/2", *C.FIXED, C.AUTO)
    want, data = C.expect(c), C.src_of(c)
    got = L.Lzma86_Encode(data, C.cap_of(c), 1, 0, C.AUTO)
    assert got == want
    assert L.Lzma86_Encode(data, 13) == (C.OUTPUT_EOF, 0, b"")
    assert L.Lzma86_Encode(data, want[1] - 1)[:2] == (C.OUTPUT_EOF, 14)
    assert L.Lzma86_GetUnpackSize(want[2]) == (C.OK, len(data))
    assert L.Lzma86_GetUnpackSize(want[2][:13])[0] == C.INPUT_EOF
    assert L.Lzma86_Decode(want[2], len(data)) == (C.OK, len(data), len(want[2]), data)
    assert L.Lzma86_Decode(want[2][:13], len(data))[0] == C.INPUT_EOF
    assert L.Lzma86_Decode(b"\x02" + want[2][1:], len(data))[:2] == (C.UNSUPPORTED, 0)


def test_long_candidates_take_the_split_gather(L, cases):
    """A chosen candidate above the split threshold is moved by several
    workgroups in a second launch: two streams whose payloads exceed the default
    32 KiB (one filtered, one not) beside a short one, and the whole case batch
    again with the threshold lowered to 1,000 bytes -- the same bytes."""
    big = [C.case("noise40k", "noise", 37, 40000, C.AUTO),
           C.case("code/2", *C.FIXED, C.AUTO),
           C.case("code70k", "code", 38, 70001, C.YES, level=0)]
    descs, res, out = encode_device(L, big)
    check_encoded(big, descs, res, out)
    assert res[0].dest_len > 32768 + 14 and res[2].dest_len > 32768 + 14
    assert (res[0].filter, res[2].filter) == (0, 1)
    old = os.environ.get("LZGPU_LZMA86_SPLIT")
    os.environ["LZGPU_LZMA86_SPLIT"] = "1000"
    try:
        descs, res, out = encode_device(L, cases)
    finally:
        if old is None:
            del os.environ["LZGPU_LZMA86_SPLIT"]
        else:
            os.environ["LZGPU_LZMA86_SPLIT"] = old
    check_encoded(cases, descs, res, out)

"""The normal-mode encoder on the device (the optimal parser and the Bt4 finder:
lzmaenc_encode_normal_kernel, lzma2enc_encode_normal_kernel) against the
reference's single-threaded LzmaEncode / Lzma2Enc_Encode at level 5 and up:
live (oracle/_ref/libref_lzma.so) where it is built, else the committed goldens
(tests/golden/lzmaenc_opt_cases.json).  Equality is the criterion everywhere.
The modes are opt-in: every test that sets the process-wide mask puts the
previous one back in a finaliser, and with the mask at 0 the same calls are
SZ_ERROR_UNSUPPORTED, as the older tests in this process expect."""
import ctypes
import lzma
import os
import sys
import time

import pytest

import lzma2enc_cases as C2
import lzma2enc_opt_cases as O2
import lzmaenc_cases as C
import lzmaenc_opt_cases as O
import native
import test_lzmaenc_gpu as T

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))

pytestmark = pytest.mark.gpu
POISON = T.POISON
STEP_LIMIT_S = 60.0  # an encode step that takes longer is a failure, not a wait
RANK = {3: 0, 1: 1, 2: 2, 0: 3}   # the planner's mode groups, in launch order


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


@pytest.fixture(scope="module")
def golden():
    return O.load_golden()


@pytest.fixture
def modes_on(L, request):
    prev = L.enc_set_modes(O.ALL_MODES)
    request.addfinalizer(lambda: L.enc_set_modes(prev))
    return prev


_want = {}


def want_of(c, golden):
    """The reference's result for a case, computed once and shared."""
    k = O.key(c)
    if k not in _want:
        _want[k] = O.expect(c, golden=golden) if "nhb" in c else C.expect(c)
    return _want[k]


def desc_of(L, c):
    p = L.enc_props(c["level"], c["dict"], c["lc"], c["lp"], c["pb"], c["fb"], c["mc"], c["algo"],
                    c["bt"])
    p.numHashBytes = c.get("nhb", -1)
    return L.enc_desc_from_props_ex(p, O.ALL_MODES, c["end_mark"])


def mode0_cases():
    """Level-1 streams of the fast-path list, mixed into the normal-mode batch."""
    pick = [C.case("text", 9, 4097, dict=4096), C.case("copy", 10, 20000, dict=4096),
            C.case("text", 100, 0), C.case("byte", 7, 600, fb=32),
            C.case("random", 12, 70 * 1024, dict=1 << 16, cap=5)]
    assert all(c in C.edge_cases() for c in pick)
    return pick


def run_device(L, items, lanes=0):
    """test_lzmaenc_gpu.run_device with the planner's grouped order checked
    instead of the plain longest-first one: odd offsets, a poisoned destination
    and workspace.  Returns ([(res, dest_len, bytes)], order, descs)."""
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
        src += data + b"\x5a" * (2 + len(data) % 2)
        dst_off += cap + 2 + cap % 2
    r, order, ws = L.enc_plan(descs, n)
    assert r == 0 and sorted(order) == list(range(n))
    keys = [(RANK.get(descs[k].mode, 3), -descs[k].src_len) for k in order]
    assert keys == sorted(keys), "order: grouped by mode, longest first within a mode"
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
    r = L.encode_batch_device(d_desc.data_ptr(), d_order.data_ptr(), n, d_src.data_ptr(),
                              d_dst.data_ptr(), d_ws.data_ptr(), d_res.data_ptr(), lanes)
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
    return got, order, descs


def encode_cases(L, cases, golden, lanes=0, extra=()):
    """One batch of the cases (refused ones stay on the host) plus hand-made
    (desc, data, cap, res) extras at the end; every result against the
    reference.  Returns the round-trip work of the SZ_OK streams."""
    items, wants = [], []
    for c in cases:
        w = want_of(c, golden)
        r, d, props5 = desc_of(L, c)
        assert r == (w["res"] if w["res"] in (O.PARAM, O.UNSUPPORTED) else 0), O.key(c)
        if r != 0:
            continue
        assert props5 == w["props5"], O.key(c)
        assert d.mode == (O.mode_of(c) if "nhb" in c else 0), O.key(c)
        items.append((d, O.data_of(c), w["cap"]))
        wants.append((c, w))
    for d, data, cap, res in extra:
        items.append((d, data, cap))
        wants.append((None, res))
    got, order, descs = run_device(L, items, lanes)
    back = []
    for k, ((c, w), g) in enumerate(zip(wants, got)):
        if c is None:
            assert g == (w, 0, b""), (k, g[:2])
            continue
        O.check((g[0], g[1], w["props5"], g[2]), w, O.key(c))
        if g[0] == O.OK:
            back.append((w["props5"], g[2], items[k][1]))
    return back, [descs[k].mode for k in order]


def test_every_edge_case_in_one_planned_batch(L, golden):
    """The whole edge list (all three normal modes) with level-1 streams mixed
    in and two descriptors the kernels refuse, in the planner's order; then the
    round trip through the GPU decoder."""
    bad_mode = T.raw_desc(L, mode=4)
    bad_lc = T.raw_desc(L, lc=9, mode=3)
    edge = O.edge_cases()
    cases = edge[:20] + mode0_cases() + edge[20:]
    back, modes = encode_cases(L, cases, golden,
                               extra=[(bad_mode, b"abcdefgh", 64, O.PARAM),
                                      (bad_lc, b"abcdefgh", 64, O.PARAM)])
    # 64 edge cases: 2 refused on the host, 4 overflows; 5 mode-0 streams: 1 overflow
    assert len(back) == 58 + 4
    assert set(modes) == {0, 1, 2, 3, 4}
    T.round_trip(L, back)
    # a refused descriptor takes no slice
    d = (L.EncStreamDesc * 2)(bad_mode, T.raw_desc(L, mode=3, src_len=100))
    r, order, ws = L.enc_plan(d, 2)
    assert r == 0 and d[0].ws_off == 0 and ws > 192 * 1024 and order == [1, 0]


@pytest.mark.parametrize("lanes", [16, 32, 64])
def test_lanes(L, golden, lanes):
    """70 streams, most of them short: more than one wave at every lanes value,
    all four modes in one batch."""
    cases = [c for c in O.edge_cases() if c["n"] <= 9000 and c["dict"] != 0] + mode0_cases()[:4]
    if native.have_ref():
        more = O.random_cases(60, 31337, max_n=6000)
    else:
        more = [g["case"] for g in golden["cases"] if g["case"]["n"] <= 6000
                and g["case"] not in cases]
    cases = (cases + more)[:70]
    assert len(cases) == 70 and {O.mode_of(c) for c in cases if "nhb" in c} == {1, 2, 3}
    back, _ = encode_cases(L, cases, golden, lanes=lanes)
    if lanes == 64:
        T.round_trip(L, back)


def test_lzma_compress_at_its_true_defaults(L, golden, modes_on):
    c = O.case("copy", 14, 3000, lc=3, lp=0, pb=2)
    assert c in O.edge_cases() and c["level"] == 5 and c["dict"] == 0
    w, data = want_of(c, golden), O.data_of(c)
    t0 = time.monotonic()
    got = L.LzmaCompress(data, w["cap"])          # level 5, dictSize 0, lc / lp / pb / fb -1
    assert time.monotonic() - t0 < STEP_LIMIT_S
    assert got[:3] == (O.OK, w["dest_len"], w["props5"]) and O.sha(got[3]) == w["sha256"]
    assert w["props5"][1:] == (1 << 24).to_bytes(4, "little")
    props = L.enc_props(5)
    got = L.LzmaEncode(data, props, w["cap"])
    assert got[:3] == (O.OK, w["dest_len"], w["props5"]) and O.sha(got[3]) == w["sha256"]
    r, d, props5 = L.enc_desc_from_props(props)
    assert (r, d.mode, props5) == (0, 3, w["props5"])
    # Bt3 stays unsupported, and the error names the field
    props.numHashBytes = 3
    assert L.LzmaEncode(data, props, w["cap"])[0] == O.UNSUPPORTED
    assert "numHashBytes" in L.last_error()


def pieces_data():
    return b"".join(O2.data_of(c) for c in O2.PIECES)


def check_blocks(L, stream, golden):
    """An LZMA2 stream of the PIECES buffer: every block is its piece's golden."""
    blocks = L.split_lzma2_blocks(stream)
    assert [u for _, _, u in blocks] == [C2.size_of(c) for c in O2.PIECES]
    for (o, n, _), c in zip(blocks, O2.PIECES):
        w = O2.expect(c, golden=golden)
        assert n == w["len"] - 1 and C2.sha(stream[o:o + n] + b"\0") == w["sha256"], O2.key(c)
    assert stream[-1] == 0 and len(stream) == sum(n for _, n, _ in blocks) + 1


def test_lzma2_host_and_xz_at_level_5(L, golden, modes_on):
    data = pieces_data()
    props = L.enc2_props(5, 1 << 16, block_size=O2.BLOCK)
    t0 = time.monotonic()
    r, prop, out = L.Lzma2EncodeHost(data, props, len(data) + 4096)
    assert time.monotonic() - t0 < STEP_LIMIT_S
    assert r == 0, L.last_error()
    assert prop == O2.expect(O2.PIECES[0], golden=golden)["prop"]
    check_blocks(L, out, golden)
    assert C2.decode_raw(out, prop) == data
    r, d, p = L.enc2_desc_from_props(props)
    assert (r, d.mode, p) == (0, 3, prop)
    # xz with CRC-64
    r, xz = L.XzEncode(data, props, 4, len(data) + 4096)
    assert r == 0, L.last_error()
    r, blocks, total = L.xz_index(xz)
    assert (r, total, len(blocks)) == (0, len(data), 3)
    for b, c in zip(blocks, O2.PIECES):
        w = O2.expect(c, golden=golden)
        body = xz[b.data_off:b.data_off + b.pack_size]
        assert (b.check_type, b.pack_size) == (4, w["len"]) and C2.sha(body) == w["sha256"]
    assert lzma.decompress(xz, format=lzma.FORMAT_XZ) == data
    assert L.XzDecode(xz, len(data)) == (0, data, -1)
    # the block batch: the mixed piece, where a stored chunk precedes the restore
    got = L.lzma2_encode_batch([O2.data_of(O2.MIXED_CASE)], level=5, dict_size=1 << 16)
    w = O2.expect(O2.MIXED_CASE, golden=golden)
    assert [(r, p, len(b), C2.sha(b + b"\0")) for r, p, b in got] == [
        (0, w["prop"], w["len"] - 1, w["sha256"])]


def sevenz_archive(L):
    import bcj2enc
    import sevenzenc_cases as S
    row = dict(level=5, dict_size=1 << 16, lc=3, lp=0, pb=2)
    methods = [L.sz_method(L.SZ_M_LZMA, **row),
               L.sz_method(L.SZ_M_LZMA2, block_size=O2.BLOCK, **row),
               L.sz_method(L.SZ_M_LZMA, filter=L.SZ_FILTER_BCJ2, **row)]
    a = S.Archive(L, methods)
    a.group(0, [("plain.txt", O.data_of(O.SEVENZ_CASE))])
    a.group(1, [("blocks.bin", pieces_data())])
    a.group(2, [("code.bin", bcj2enc.x86_like(961, 12000))])
    return a


def test_7z_archive_at_level_5(L, golden, modes_on):
    import sevenzenc_cases as S
    import sevenzwrite as W
    a = sevenz_archive(L)
    src, items, n, names, names_len = a.build()
    r, folders, n_pieces, cap = L.sz_write_plan(items, n, len(src), names_len, a.methods)
    assert r == S.OK, L.last_error()
    t0 = time.monotonic()
    r, size, dest, st = L.SzWrite(src, items, n, names, names_len, a.methods, cap, 0, fill=0xEE)
    assert time.monotonic() - t0 < STEP_LIMIT_S
    assert r == S.OK, L.last_error()
    arc = dest[:size]
    want = b"".join(a.data_files())
    r, fo, fi, nm, total = L.sz_open(arc)
    assert r == S.OK and total == len(want) and [f.num_coders for f in fo] == [1, 1, 4]
    r, out, fres = L.SzExtract(arc, len(want))
    assert r == S.OK and out == want
    # the plain LZMA folder and the LZMA2 folder are the reference's streams
    w = want_of(O.SEVENZ_CASE, golden)
    pack = arc[fo[0].pack_off:fo[0].pack_off + fo[0].pack_size]
    assert bytes(fo[0].props[:fo[0].props_size]) == w["props5"]
    assert (len(pack), O.sha(pack)) == (w["dest_len"], w["sha256"])
    check_blocks(L, arc[fo[1].pack_off:fo[1].pack_off + fo[1].pack_size], golden)
    if not S.have_ref_reader():
        return
    # the reference's reader, and the BCJ2 folder's three coders by the
    # reference's encoder at the same props
    r, fres, fsz, out, nm = S.ref_extract(arc)
    assert r == S.OK and out == want
    files = a.groups()[2][2]
    f = W.Bcj2Folder(files, methods=(W.M_COPY, W.M_COPY, W.M_COPY))
    f.methods = (W.M_LZMA, W.M_LZMA, W.M_LZMA)
    f.enc = []
    for k, raw in enumerate(f.raw):
        kw = dict(level=5, dict_size=1 << 16, lc=3, lp=0, pb=2) if k == 2 else \
            dict(level=5, dict_size=1 << 16, lc=0, lp=2, pb=2)
        props, packed = native.ref_encode(raw, **kw)
        f.enc.append((packed, props))
    f._packs = [f.enc[2][0], f.rc, f.enc[1][0], f.enc[0][0]]
    f.packed = b"".join(f._packs)
    helper = [S.helper_folder(L, a.methods[mi], fl, arc[q.pack_off:q.pack_off + q.pack_size],
                              bytes(q.props[:q.props_size]))
              for (_, mi, fl), q in list(zip(a.groups(), fo))[:2]] + [f]
    assert arc == W.archive(helper, a.empties())


def test_switch_off_the_same_calls_are_unsupported(L):
    assert L.enc_get_modes() == 0
    data = O.data_of(O.SEVENZ_CASE)
    assert L.LzmaCompress(data, 20000)[0] == O.UNSUPPORTED
    assert "optimal parser" in L.last_error()
    assert L.LzmaEncode(data, L.enc_props(5), 20000)[0] == O.UNSUPPORTED
    assert L.enc_desc_from_props(L.enc_props(5))[0] == O.UNSUPPORTED
    assert L.enc_desc_from_props_ex(L.enc_props(5), 0)[0] == O.UNSUPPORTED
    assert L.enc_desc_from_props_ex(L.enc_props(5), 1)[0] == O.UNSUPPORTED
    assert "btMode" in L.last_error()
    assert L.enc_desc_from_props_ex(L.enc_props(5), 3)[0] == 0
    props2 = L.enc2_props(5, 1 << 16, block_size=O2.BLOCK)
    assert L.enc2_desc_from_props(props2)[0] == O.UNSUPPORTED
    assert L.enc2_desc_from_props_ex(props2, 3)[:1] == (0,)
    assert L.Lzma2EncodeHost(data, props2, 20000)[0] == O.UNSUPPORTED
    assert L.XzEncode(data, props2, 4, 20000)[0] == O.UNSUPPORTED
    a = sevenz_archive(L)
    src, items, n, names, names_len = a.build()
    assert L.sz_write_plan(items, n, len(src), names_len, a.methods)[0] == O.UNSUPPORTED
    # the switch itself: returns the previous mask, drops unknown bits
    assert L.enc_set_modes(7) == 0 and L.enc_get_modes() == 3
    assert L.enc_set_modes(0) == 3 and L.enc_get_modes() == 0

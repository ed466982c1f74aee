"""BCJ2 folders in the 7z writer, without a device: the plan for BCJ2 rows and
its refusals, and LzmaGpu_7zWriteHeaderEx against the layout helper
(tests/sevenzwrite.py's Bcj2Folder beside one- and two-coder folders) around
Python-made pack streams, read back by LzmaGpu_7zOpen and, where built, by the
reference's own reader."""
import ctypes
import zlib

import pytest

import bcj2enc
import native
import sevenzenc_cases as S
import sevenzwrite as W

OK, UNSUPPORTED, PARAM = S.OK, S.UNSUPPORTED, S.PARAM
needs_ref = pytest.mark.skipif(not S.have_ref_reader(), reason="reference library not built")


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def plan(L, entries, methods, src_size=1 << 20):
    items, names, names_len = L.sz_items(entries)
    return L.sz_write_plan(items, len(entries), src_size, names_len, methods)


def test_constant_struct_and_exports(L):
    assert L.SZ_FILTER_BCJ2 == 0x1B and ctypes.sizeof(L.SzBcj2Info) == 72
    assert L.SzBcj2Info.unpack_size.offset == 32 and L.SzBcj2Info.call_props.offset == 56
    header = open(native.ROOT + "/include/lzma_gpu.h").read()
    assert "LzmaGpu_7zWriteHeaderEx(" in header and "LZMA_GPU_7Z_FILTER_BCJ2 0x1B" in header
    assert "LzmaGpu_7zWriteHeaderEx" in L.EXPORTED


def test_bcj2_is_for_lzma_rows_only(L):
    assert plan(L, [], [L.sz_method(L.SZ_M_LZMA, filter=L.SZ_FILTER_BCJ2)])[0] == OK
    for m in (L.sz_method(L.SZ_M_COPY, filter=L.SZ_FILTER_BCJ2),
              L.sz_method(L.SZ_M_LZMA2, filter=L.SZ_FILTER_BCJ2),
              L.sz_method(L.SZ_M_PPMD, filter=L.SZ_FILTER_BCJ2)):
        assert plan(L, [], [m])[0] == UNSUPPORTED
        assert "BCJ2" in L.last_error()
    # every other unknown filter value stays a parameter error
    for f in (5, 0x1A, 0x1C, 0x0303011B):
        assert plan(L, [], [L.sz_method(L.SZ_M_LZMA, filter=f)])[0] == PARAM
    # the encoder's own verdict on the row's props stands
    assert plan(L, [], [L.sz_method(L.SZ_M_LZMA, level=5, filter=L.SZ_FILTER_BCJ2)])[0] == UNSUPPORTED
    assert plan(L, [], [L.sz_method(L.SZ_M_LZMA, lc=9, filter=L.SZ_FILTER_BCJ2)])[0] == PARAM


def test_plan_counts_four_pieces_and_four_coders(L):
    methods = [L.sz_method(L.SZ_M_LZMA, level=1, filter=L.SZ_FILTER_BCJ2),
               L.sz_method(L.SZ_M_LZMA, level=1), L.sz_method(L.SZ_M_COPY)]
    entries = [("x/a", 0, 5000, 0, 0), ("x/b", 5000, 300, L.SZ_ITEM_JOIN, 0),
               ("plain", 5300, 100, 0, 1), ("y", 5400, 1, 0, 0), ("raw", 5401, 9, 0, 2)]
    r, folders, n_pieces, bound = plan(L, entries, methods, src_size=5410)
    assert r == OK
    assert [(f.num_coders, f.x86, f.num_files, f.unpack_size, f.method) for f in folders] == [
        (4, 0, 2, 5300, W.M_LZMA), (1, 0, 1, 100, W.M_LZMA), (4, 0, 1, 1, W.M_LZMA),
        (1, 0, 1, 9, 0)]
    assert [f.props_size for f in folders] == [5, 5, 5, 0]
    assert n_pieces == 4 + 1 + 4 + 1
    # the bound holds the four streams of every BCJ2 folder at their bounds
    # (main n, call and jump 4 (n / 5), rc 5 + n) however badly they compress
    assert bound > 32 + (5300 + 2 * 4 * (5300 // 5) + 5305) + 100 + (1 + 6) + 9
    # a BCJ2 folder's range may overlap another's: the split is out of place
    r2 = plan(L, [("a", 0, 100, 0, 0), ("b", 50, 100, 0, 0)], methods, src_size=200)
    assert r2[0] == OK and [f.num_coders for f in r2[1]] == [4, 4]


def mixed_archive(L):
    """A BCJ2 folder (solid), a plain LZMA folder, an x86-filtered folder, a BCJ2
    folder without any branch, a Copy folder; pack streams made in Python."""
    xd = bcj2enc.x86_like(931, 20000)
    text = native.gen("text", 932, 9000)
    methods = [L.sz_method(L.SZ_M_LZMA, level=1, dict_size=1 << 16, filter=L.SZ_FILTER_BCJ2),
               L.sz_method(L.SZ_M_LZMA, level=1, dict_size=1 << 16),
               L.sz_method(L.SZ_M_LZMA, level=1, dict_size=1 << 16, filter=L.SZ_FILTER_X86),
               L.sz_method(L.SZ_M_COPY)]
    a = S.Archive(L, methods)
    a.group(0, [("bcj2/code", xd[:12000]), ("bcj2/tail", xd[12000:15000])])
    a.group(1, [("plain.txt", text[:4000])])
    a.group(2, [("x86/code", xd[15000:])])
    a.group(0, [("bcj2/no-branch.txt", text[4000:6000])])
    a.group(3, [("raw", text[6000:6100])])
    a.empty("zero.txt").empty("a/dir", True)
    helper = []
    for _, mi, files in a.groups():
        m = methods[mi]
        if m.filter == L.SZ_FILTER_BCJ2:
            helper.append(W.Bcj2Folder(files))
        else:
            packed, props = W.encode(m.method, S.filtered(b"".join(d for _, d in files), m.filter))
            helper.append(S.helper_folder(L, m, files, packed, props))
    return a, helper


def header_inputs(L, a, helper):
    src, items, n, names, names_len = a.build()
    r, folders, _, _ = L.sz_write_plan(items, n, len(src), names_len, a.methods)
    assert r == OK and len(folders) == len(helper)
    infos = []
    for f, h in zip(folders, helper):
        four = isinstance(h, W.Bcj2Folder)
        assert f.num_coders == (4 if four else 2 if h.bcj else 1)
        props = h.enc[2][1] if four else h.props
        f.pack_size = len(h.packed)
        f.props_size = len(props)
        for k in range(8):
            f.props[k] = props[k] if k < len(props) else 0
        if four:
            i = L.SzBcj2Info()
            for k, p in enumerate(h.pack_streams()):
                i.pack_size[k] = len(p)
            for k, raw in enumerate(h.raw):
                i.unpack_size[k] = len(raw)
            for k in range(5):
                i.jump_props[k], i.call_props[k] = h.enc[0][1][k], h.enc[1][1][k]
            infos.append(i)
    crcs = [zlib.crc32(src[items[i].src_off:items[i].src_off + items[i].size]) for i in range(n)]
    return src, items, n, names, names_len, folders, crcs, infos


def test_header_ex_equals_the_layout_helper(L):
    a, helper = mixed_archive(L)
    src, items, n, names, names_len, folders, crcs, infos = header_inputs(L, a, helper)
    assert len(infos) == 2 and helper[3].raw[0] == helper[3].raw[1] == b""
    body = b"".join(h.packed for h in helper)
    r, hdr, sig = L.sz_write_header_ex(folders, items, n, crcs, names, names_len, infos, 0,
                                       len(body))
    assert r == OK
    assert hdr == W.header(helper, a.empties())
    assert sig + body + hdr == W.archive(helper, a.empties())
    # the old call is the new one without entries: a four-coder folder has none
    assert L.sz_write_header(folders, items, n, crcs, names, names_len)[0] == PARAM
    assert L.sz_write_header_ex(folders, items, n, crcs, names, names_len, infos[:1])[0] == PARAM
    # without four-coder folders the two calls agree
    a2 = S.Archive(L, a.methods).group(1, [("t", b"some text")])
    h2 = [S.helper_folder(L, a.methods[1], [("t", b"some text")], *W.encode(W.M_LZMA, b"some text"))]
    _, items2, n2, names2, nl2, folders2, crcs2, _ = header_inputs(L, a2, h2)
    assert L.sz_write_header_ex(folders2, items2, n2, crcs2, names2, nl2, []) == \
        L.sz_write_header(folders2, items2, n2, crcs2, names2, nl2)


def test_archive_is_read_back_by_7zopen(L):
    a, helper = mixed_archive(L)
    src, items, n, names, names_len, folders, crcs, infos = header_inputs(L, a, helper)
    body = b"".join(h.packed for h in helper)
    r, hdr, sig = L.sz_write_header_ex(folders, items, n, crcs, names, names_len, infos, 0,
                                       len(body))
    r, fo, fi, raw_names, total = L.sz_open(sig + body + hdr)
    assert r == OK and len(fo) == len(folders) and len(fi) == n
    assert raw_names == a.names_buffer()
    assert [(f.num_coders, f.supported, f.unpack_size, f.num_files) for f in fo] == [
        (w.num_coders, OK, w.unpack_size, w.num_files) for w in folders]
    assert total == sum(len(d) for d in a.data_files())
    assert [f.crc for f in fi if f.has_stream] == [c for c, f in zip(crcs, fi) if f.has_stream]


@needs_ref
def test_the_reference_reader_extracts_it(L):
    a, helper = mixed_archive(L)
    src, items, n, names, names_len, folders, crcs, infos = header_inputs(L, a, helper)
    body = b"".join(h.packed for h in helper)
    r, hdr, sig = L.sz_write_header_ex(folders, items, n, crcs, names, names_len, infos, 0,
                                       len(body))
    r, fres, fsz, out, rnames = S.ref_extract(sig + body + hdr)
    assert r == OK and fres == [OK] * len(a.item_names())
    assert out == b"".join(a.data_files()) and rnames == a.names_buffer()

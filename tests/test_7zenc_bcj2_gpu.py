"""BCJ2 folders written by LzmaGpu_7zWrite: one archive with BCJ2 folders (x86
code, a solid JOIN group, data without any branch, random bytes) beside LZMA,
LZMA2 and Copy folders; read back by LzmaGpu_7zExtract and the reference's own
reader, and equal, byte for byte, to the layout helper around Bcj2Folders whose
three coder streams are the reference's LzmaEncode of the model's streams
(tests/bcj2enc.py), with and without a packed header.

The folder of 3,000 random bytes fits its first slot (LZMA's fast mode turns
3,000 random bytes into about 3,050, the slot is 3,087); the folder of 12,000
random bytes beside it is the one whose main stream is encoded again."""
import struct
import zlib

import pytest

import bcj2enc
import native
import sevenzenc_cases as S
import sevenzwrite as W

pytestmark = pytest.mark.gpu
OK = S.OK
needs_ref = pytest.mark.skipif(not S.have_ref_reader(), reason="reference library not built")
ROW = dict(level=1, dict_size=1 << 16, lc=3, lp=0, pb=2)
TARGET = dict(level=1, dict_size=1 << 16, lc=0, lp=2, pb=2)   # the CALL and JMP coders


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def describe(L):
    xd = bcj2enc.x86_like(951, 24000)
    solid = bcj2enc.x86_like(952, 9000, 0.3)
    text = native.gen("text", 953, 30000)
    rnd = native.gen("random", 954, 15000)
    methods = [L.sz_method(L.SZ_M_LZMA, filter=L.SZ_FILTER_BCJ2, **ROW),
               L.sz_method(L.SZ_M_LZMA, **ROW),
               L.sz_method(L.SZ_M_LZMA2, block_size=4096, **ROW),
               L.sz_method(L.SZ_M_COPY)]
    a = S.Archive(L, methods)
    a.group(1, [("plain/a.txt", text[:9000])])
    a.group(0, [("bcj2/code.bin", xd)])
    a.group(0, [("bcj2/solid/%d.bin" % j, solid[3000 * j:3000 * (j + 1)]) for j in range(3)])
    a.group(3, [("copy/raw.bin", rnd[:777])])
    a.group(0, [("bcj2/no-branch.txt", text[9000:12000])])
    a.group(2, [("lzma2/blocks.txt", text[12000:22001])])
    a.group(0, [("bcj2/random-3000.bin", rnd[:3000])])
    a.group(0, [("bcj2/random-12000.bin", rnd[3000:15000])])
    a.group(1, [("plain/one-byte", text[22001:22002])])
    a.empty("empty.txt").empty("a/dir", True)
    return a


def write(L, a, flags=0):
    src, items, n, names, names_len = a.build()
    r, folders, n_pieces, cap = L.sz_write_plan(items, n, len(src), names_len, a.methods)
    assert r == OK
    r, size, dest, st = L.SzWrite(src, items, n, names, names_len, a.methods, cap, flags, fill=0xEE)
    assert r == OK, L.last_error()
    assert dest[size:] == b"\xee" * (len(dest) - size) and st.pieces == n_pieces
    return dest[:size], st


@pytest.fixture(scope="module")
def written(L):
    a = describe(L)
    arc, st = write(L, a)
    return a, arc, st


def test_7zextract_returns_the_sources(L, written):
    a, arc, st = written
    want = b"".join(a.data_files())
    r, fo, fi, names, total = L.sz_open(arc)
    assert r == OK and total == len(want) and names == a.names_buffer()
    assert [f.num_coders for f in fo] == [1, 4, 4, 1, 4, 1, 4, 4, 1]
    assert all(f.supported == OK for f in fo)
    r, out, fres = L.SzExtract(arc, len(want))
    assert r == OK and out == want
    assert fres[:len(a.item_names())] == [OK] * len(a.item_names())
    assert st.folders == 9 and st.pieces == 4 * 5 + 3 + 3     # LZMA2: three blocks
    assert st.reencoded >= 1


def test_the_archive_is_a_pure_function_of_its_inputs(L, written):
    a, arc, st = written
    again, st2 = write(L, a)
    assert again == arc and (st2.pieces, st2.reencoded) == (st.pieces, st.reencoded)


def ref_bcj2_folder(files):
    """The layout helper's BCJ2 folder around the reference's encoder: coders 0,
    1, 2 = jump, call, main."""
    f = W.Bcj2Folder(files, methods=(W.M_COPY, W.M_COPY, W.M_COPY))
    f.methods = (W.M_LZMA, W.M_LZMA, W.M_LZMA)
    f.enc = []
    for k, raw in enumerate(f.raw):
        props, packed = native.ref_encode(raw, **(ROW if k == 2 else TARGET))
        f.enc.append((packed, props))
    f._packs = [f.enc[2][0], f.rc, f.enc[1][0], f.enc[0][0]]
    f.packed = b"".join(f._packs)
    return f


def helper_folders(L, a, arc):
    """Bcj2Folders from the model and the reference; the other folders around
    the archive's own pack streams."""
    r, fo, fi, names, total = L.sz_open(arc)
    assert r == OK
    helper = []
    for (_, mi, files), f in zip(a.groups(), fo):
        m = a.methods[mi]
        if m.filter == L.SZ_FILTER_BCJ2:
            helper.append(ref_bcj2_folder(files))
        else:
            helper.append(S.helper_folder(L, m, files, arc[f.pack_off:f.pack_off + f.pack_size],
                                          bytes(f.props[:f.props_size])))
    return helper


@needs_ref
def test_the_reference_reader_extracts_it(L, written):
    a, arc, st = written
    r, fres, fsz, out, names = S.ref_extract(arc)
    assert r == OK and fres == [OK] * len(a.item_names())
    assert out == b"".join(a.data_files()) and names == a.names_buffer()


@needs_ref
def test_archive_equals_the_layout_helper_over_reference_streams(L, written):
    a, arc, st = written
    helper = helper_folders(L, a, arc)
    no_branch = helper[4]
    assert no_branch.raw[0] == no_branch.raw[1] == b""
    assert no_branch.enc[0] == (b"\0" * 5, bytes.fromhex("6c00000100"))
    assert arc == W.archive(helper, a.empties())
    assert st.pack_bytes == sum(len(h.packed) for h in helper)


@needs_ref
def test_the_same_with_a_packed_header(L, written):
    a, plain, _ = written
    arc, st = write(L, a, L.SZ_WRITE_ENCODE_HEADER)
    helper = helper_folders(L, a, plain)
    body = b"".join(h.packed for h in helper)
    hdr = W.header(helper, a.empties())
    dict_size = 1 << 12
    while dict_size < len(hdr):
        dict_size <<= 1
    props, packed = native.ref_encode(hdr, level=4, dict_size=dict_size)
    hf = W.Folder([("", hdr)], method=W.M_LZMA, packed=packed, props=props, crc=True)
    stub = bytes([W.ENCODED_HEADER]) + W.streams_info([hf], len(body), substreams=False)
    start = struct.pack("<QQI", len(body) + len(packed), len(stub), zlib.crc32(stub))
    sig = b"7z\xbc\xaf\x27\x1c\x00\x04" + struct.pack("<I", zlib.crc32(start)) + start
    assert arc == sig + body + packed + stub
    r, fres, fsz, out, names = S.ref_extract(arc)
    assert r == OK and out == b"".join(a.data_files())
    r, out, fres = L.SzExtract(arc, len(out))
    assert r == OK and out == b"".join(a.data_files())


def test_sevenz_compress_with_bcj2(L):
    data = bcj2enc.x86_like(955, 30000)
    files = [("a.bin", data[:20000]), ("d", None), ("b.bin", data[20000:])]
    for kw in (dict(), dict(solid=2, encode_header=True)):
        arc = L.sevenz_compress(files, filter=L.SZ_FILTER_BCJ2, **kw)
        r, out, fres = L.SzExtract(arc, len(data))
        assert r == OK and out == data and fres[:3] == [OK] * 3, kw
    with pytest.raises(RuntimeError):
        L.sevenz_compress(files, method=L.SZ_M_LZMA2, filter=L.SZ_FILTER_BCJ2)

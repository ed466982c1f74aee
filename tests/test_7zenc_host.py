"""The 7z writer without a device: the exported surface and its refusals, the
plan (items -> folders and pieces), the header writer against the layout
helper (tests/sevenzwrite.py) around Python-made pack streams -- read back by
LzmaGpu_7zOpen and by the reference's own reader -- and the pack stage
(csrc/sevenz_pack_device.h) on the host: g++ -Wall -Werror
(tests/emu_7zpack/pack_emu.cpp) against a plain model of scan and gather, once
more as a stand-alone sanitizer build run as a child process."""
import ctypes
import os
import subprocess
import zlib

import pytest

import native
import sevenzenc_cases as S
import sevenzpack_cases as P
import sevenzwrite as W

OK, UNSUPPORTED, PARAM, OUTPUT_EOF, FAIL = S.OK, S.UNSUPPORTED, S.PARAM, S.OUTPUT_EOF, S.FAIL
NAMES = {"LzmaGpu_7zWritePlan", "LzmaGpu_7zWriteHeader", "LzmaGpu_7zWrite", "SzGpu_PackBatch",
         "SzGpu_PackScratch"}
needs_ref = pytest.mark.skipif(not S.have_ref_reader(), reason="reference library not built")


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def test_struct_sizes_and_exports(L):
    assert (ctypes.sizeof(L.SzItem), ctypes.sizeof(L.SzMethod)) == (32, 88)
    assert L.SzMethod.props.offset == 24
    assert (ctypes.sizeof(L.SzWriteOptions), ctypes.sizeof(L.SzWriteStats)) == (16, 112)
    assert (ctypes.sizeof(L.SzPackPiece), ctypes.sizeof(L.SzPackArgs)) == (32, 152)
    assert L.SzPackArgs.d_out.offset == 104 and L.SzPackPiece.kind.offset == 24
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert NAMES <= exported and NAMES <= set(L.EXPORTED)
    header = open(os.path.join(native.ROOT, "include", "lzma_gpu.h")).read()
    assert all(n + "(" in header for n in NAMES)
    assert L.sz_pack_scratch(0) == 1 and L.sz_pack_scratch(257) == 257 + 2 + 1


def plan(L, entries, methods, src_size=1 << 20):
    items, names, names_len = L.sz_items(entries)
    return L.sz_write_plan(items, len(entries), src_size, names_len, methods)


def test_refusals_come_before_the_device(L):
    ok = [L.sz_method(L.SZ_M_LZMA)]
    assert plan(L, [("a", 0, 10, 0, 0)], ok)[0] == OK
    # JOIN: nothing before it, a gap, another method
    assert plan(L, [("a", 0, 10, L.SZ_ITEM_JOIN, 0)], ok)[0] == PARAM
    assert plan(L, [("a", 0, 10, 0, 0), ("b", 11, 5, L.SZ_ITEM_JOIN, 0)], ok)[0] == PARAM
    two = ok + [L.sz_method(L.SZ_M_COPY)]
    assert plan(L, [("a", 0, 10, 0, 0), ("b", 10, 5, L.SZ_ITEM_JOIN, 1)], two)[0] == PARAM
    assert plan(L, [("a", 0, 10, 0, 0), ("b", 10, 5, L.SZ_ITEM_JOIN, 0)], two)[0] == OK
    # a JOIN on an entry without data means nothing
    assert plan(L, [("d", 0, 0, L.SZ_ITEM_DIR | L.SZ_ITEM_JOIN, 0)], ok)[0] == OK
    # ranges, method indices, flags
    assert plan(L, [("a", 90, 11, 0, 0)], ok, src_size=100)[0] == PARAM
    assert plan(L, [("a", 90, 10, 0, 0)], ok, src_size=100)[0] == OK
    assert plan(L, [("a", 0, 10, 0, 1)], ok)[0] == PARAM
    assert plan(L, [("a", 0, 10, 4, 0)], ok)[0] == PARAM
    assert plan(L, [("a", 0, 10, L.SZ_ITEM_DIR, 0)], ok)[0] == PARAM
    # the method table: ids, filters, PPMd ranges, the encoders' own verdicts
    assert plan(L, [], [L.sz_method(0x030102)])[0] == PARAM
    assert plan(L, [], [L.sz_method(L.SZ_M_LZMA, filter=5)])[0] == PARAM
    assert plan(L, [], [L.sz_method(L.SZ_M_PPMD, order=1)])[0] == PARAM
    assert plan(L, [], [L.sz_method(L.SZ_M_PPMD, order=65)])[0] == PARAM
    assert plan(L, [], [L.sz_method(L.SZ_M_PPMD, mem_size=2047)])[0] == PARAM
    assert plan(L, [], [L.sz_method(L.SZ_M_PPMD, order=2, mem_size=2048)])[0] == OK
    assert plan(L, [], [L.sz_method(L.SZ_M_LZMA, level=5)])[0] == UNSUPPORTED
    assert plan(L, [], [L.sz_method(L.SZ_M_LZMA2, level=5)])[0] == UNSUPPORTED
    assert plan(L, [], [L.sz_method(L.SZ_M_LZMA, lc=9)])[0] == PARAM
    assert plan(L, [], [L.sz_method(L.SZ_M_LZMA2, lc=4, lp=1)])[0] == PARAM
    assert plan(L, [], ok + [L.sz_method(L.SZ_M_LZMA, level=5)])[0] == UNSUPPORTED


def write(L, entries, methods, src=bytes(100), cap=1 << 16):
    items, names, names_len = L.sz_items(entries)
    return L.SzWrite(src, items, len(entries), names, names_len, methods, cap, fill=0xEE)


def test_no_device_fails_loudly_after_the_refusals(L):
    ok = [L.sz_method(L.SZ_M_LZMA)]
    for entries, methods, want in (
            ([("a", 0, 10, L.SZ_ITEM_JOIN, 0)], ok, PARAM),
            ([("a", 95, 10, 0, 0)], ok, PARAM),
            ([("a", 0, 10, 0, 0)], [L.sz_method(7)], PARAM),
            ([("a", 0, 10, 0, 0)], [L.sz_method(L.SZ_M_LZMA, level=5)], UNSUPPORTED)):
        r, n, dest, st = write(L, entries, methods)
        assert r == want and dest == b"\xee" * len(dest), (entries, r)
    if L.device_count() > 0:
        pytest.skip("a HIP device is present")
    r, n, dest, st = write(L, [("a", 0, 10, 0, 0)], ok)
    assert r == FAIL and dest == b"\xee" * len(dest)
    assert "no HIP device" in L.last_error()
    args = L.SzPackArgs()
    assert L.sz_pack_batch_device(args) == FAIL


def test_plan_folders_and_pieces(L):
    methods = [L.sz_method(L.SZ_M_LZMA, level=1),
               L.sz_method(L.SZ_M_LZMA2, level=1, block_size=4096),
               L.sz_method(L.SZ_M_COPY),
               L.sz_method(L.SZ_M_PPMD, order=6, mem_size=1 << 20, filter=L.SZ_FILTER_X86),
               L.sz_method(L.SZ_M_LZMA, level=1, filter=L.SZ_FILTER_ARM)]
    entries, at = [], 0
    for j in range(12):                                   # items 0..11: one solid folder
        entries.append((f"solid/{j}", at, 100 + j, L.SZ_ITEM_JOIN if j else 0, 0))
        at += 100 + j
    entries.append(("empty.txt", 0, 0, 0, 0))             # 12
    entries.append(("dir", 0, 0, L.SZ_ITEM_DIR, 0))       # 13
    entries.append(("two/blocks", at, 10000, 0, 1))       # 14: 3 pieces
    at += 10000
    entries.append(("copy", at, 7, 0, 2))                 # 15
    at += 7
    entries.append(("ppmd", at, 50, 0, 3))                # 16
    at += 50
    entries.append(("arm", at, 64, 0, 4))                 # 17
    entries.append(("arm2", at + 64, 4, L.SZ_ITEM_JOIN, 4))  # 18
    at += 68
    entries.append(("exact", at, 8192, 0, 1))             # 19: 2 pieces
    at += 8192
    r, folders, n_pieces, bound = plan(L, entries, methods, src_size=at)
    assert r == OK and len(folders) == 6
    assert [(f.first_file, f.num_files) for f in folders] == [
        (0, 12), (14, 1), (15, 1), (16, 1), (17, 2), (19, 1)]
    assert [f.unpack_size for f in folders] == [sum(100 + j for j in range(12)), 10000, 7, 50, 68,
                                                8192]
    assert [f.dst_off for f in folders][:2] == [0, sum(100 + j for j in range(12))]
    assert [f.method for f in folders] == [0x030101, 0x21, 0, 0x030401, 0x030101, 0x21]
    assert [(f.num_coders, f.x86) for f in folders] == [(1, 0), (1, 0), (1, 0), (2, 1), (2, 0),
                                                         (1, 0)]
    assert [f.props_size for f in folders] == [5, 1, 0, 5, 5, 1]
    assert bytes(folders[3].props[:5]) == bytes([6]) + (1 << 20).to_bytes(4, "little")
    assert n_pieces == 1 + 3 + 1 + 1 + 1 + 2
    assert bound > at
    # a second, non-solid list: one folder and one piece per data item
    r, folders, n_pieces, _ = plan(L, [(f"f{j}", j * 10, 10, 0, 0) for j in range(300)], methods)
    assert (r, len(folders), n_pieces) == (OK, 300, 300)


# ---------------------------------------------------------------- the header writer

def header_archive(L):
    """An archive description and pack streams made in Python: the reference's
    encoder where it is built, liblzma else."""
    text = native.gen("text", 900, 60000)
    import bcj2enc
    xd = bcj2enc.x86_like(901, 20000)
    ad = S.arm_like(902, 12000)
    methods = [L.sz_method(L.SZ_M_LZMA, level=1, dict_size=1 << 16),
               L.sz_method(L.SZ_M_LZMA2, level=1, dict_size=1 << 16),
               L.sz_method(L.SZ_M_COPY),
               L.sz_method(L.SZ_M_LZMA, level=1, dict_size=1 << 16, filter=L.SZ_FILTER_X86),
               L.sz_method(L.SZ_M_LZMA2, level=1, dict_size=1 << 16, filter=L.SZ_FILTER_ARM)]
    a = S.Archive(L, methods)
    a.group(0, [("a/one.txt", text[:7000]), ("a/two.txt", text[7000:7001]),
                ("a/ü三.txt", text[7001:20000])])
    a.group(1, [("b.bin", text[20000:45000])])
    a.group(2, [("c/raw1", text[100:133]), ("c/raw2", text[5:6])])
    a.group(3, [("x86/code", xd[:15000]), ("x86/tail", xd[15000:])])
    a.group(4, [("arm/code", ad)])
    a.empty("zero.txt").empty("some/dir", True)
    helper = []
    for _, mi, files in a.groups():
        m = methods[mi]
        data = S.filtered(b"".join(d for _, d in files), m.filter)
        if m.method == L.SZ_M_LZMA and native.have_ref():
            props, packed = native.ref_encode(data, level=1, dict_size=1 << 16)
        else:
            packed, props = W.encode(m.method, data)
        helper.append(S.helper_folder(L, m, files, packed, props))
    return a, helper


def header_inputs(L, a, helper):
    src, items, n, names, names_len = a.build()
    r, folders, _, _ = L.sz_write_plan(items, n, len(src), names_len, a.methods)
    assert r == OK and len(folders) == len(helper)
    for f, h in zip(folders, helper):
        f.pack_size = len(h.packed)
        f.props_size = len(h.props)
        for k in range(8):
            f.props[k] = h.props[k] if k < len(h.props) else 0
    crcs = [zlib.crc32(src[items[i].src_off:items[i].src_off + items[i].size]) for i in range(n)]
    return src, items, n, names, names_len, folders, crcs


def test_header_equals_the_layout_helper(L):
    a, helper = header_archive(L)
    src, items, n, names, names_len, folders, crcs = header_inputs(L, a, helper)
    body = b"".join(h.packed for h in helper)
    r, hdr, sig = L.sz_write_header(folders, items, n, crcs, names, names_len, 0, len(body))
    assert r == OK
    assert hdr == W.header(helper, a.empties())
    arc = sig + body + hdr
    assert arc == W.archive(helper, a.empties())
    # the packed-header shape: the helper's header folder as a given pack stream
    hf = W.Folder([("", hdr)], method=W.M_LZMA, crc=True)
    f = L.SzFolder()
    f.pack_off, f.pack_size, f.unpack_size = len(body), len(hf.packed), len(hdr)
    f.method, f.num_coders, f.num_files, f.props_size = W.M_LZMA, 1, 1, 5
    f.crc_defined, f.crc = 1, zlib.crc32(hdr)
    for k in range(5):
        f.props[k] = hf.props[k]
    r, stub, sig2 = L.sz_write_header([f], None, 0, None, None, 0, L.SZ_HEADER_STUB,
                                      len(body) + len(hf.packed))
    assert r == OK
    packed_arc = sig2 + body + hf.packed + stub
    assert packed_arc == W.archive(helper, a.empties(), encode_header=True)
    # a short buffer: the length, nothing else
    out = ctypes.create_string_buffer(b"\xee" * len(hdr), len(hdr))
    hl = ctypes.c_size_t(0)
    farr = (L.SzFolder * len(folders))(*folders)
    carr = (ctypes.c_uint32 * n)(*crcs)
    r = L.lib.LzmaGpu_7zWriteHeader(farr, len(folders), items, n, carr, names, names_len, 0, out,
                                    len(hdr) - 1, ctypes.byref(hl), None, 0)
    assert (r, hl.value, out.raw) == (OUTPUT_EOF, len(hdr), b"\xee" * len(hdr))
    # folders that do not cover the data items
    folders[0].num_files -= 1
    assert L.sz_write_header(folders, items, n, crcs, names, names_len)[0] == PARAM


def test_header_is_read_back_by_7zopen(L):
    a, helper = header_archive(L)
    src, items, n, names, names_len, folders, crcs = header_inputs(L, a, helper)
    body = b"".join(h.packed for h in helper)
    r, hdr, sig = L.sz_write_header(folders, items, n, crcs, names, names_len, 0, len(body))
    r, fo, fi, raw_names, total = L.sz_open(sig + body + hdr)
    assert r == OK and len(fo) == len(folders) and len(fi) == n
    assert raw_names == a.names_buffer()
    at = 32
    for got, want in zip(fo, folders):
        assert (got.pack_off, got.pack_size, got.unpack_size) == (at, want.pack_size,
                                                                  want.unpack_size)
        assert (got.method, got.x86, got.num_coders, got.num_files, got.supported) == (
            want.method, want.x86, want.num_coders, want.num_files, OK)
        assert bytes(got.props[:got.props_size]) == bytes(want.props[:want.props_size])
        at += want.pack_size
    data_last = [f for f in fi if f.has_stream] + [f for f in fi if not f.has_stream]
    assert [f.name_off for f in fi] == [items[i].name_off for i in range(n)]
    assert [(f.size, f.has_stream, f.is_dir) for f in fi] == [
        (items[i].size, int(items[i].size != 0), int(items[i].flags & L.SZ_ITEM_DIR != 0))
        for i in range(n)]
    assert [f.crc for f in fi if f.has_stream] == [c for c, f in zip(crcs, fi) if f.has_stream]
    assert len(data_last) == n and total == sum(len(d) for d in a.data_files())


@needs_ref
def test_the_reference_reader_extracts_both_shapes(L):
    a, helper = header_archive(L)
    for encode_header in (False, True):
        arc = W.archive(helper, a.empties(), encode_header=encode_header)
        r, fres, fsz, out, names = S.ref_extract(arc)
        assert r == OK and fres == [OK] * len(a.item_names())
        assert out == b"".join(a.data_files())
        assert names == a.names_buffer()


@needs_ref
def test_data_less_entries_keep_the_callers_order(L):
    """An empty file and a directory between the folders: the helper cannot
    write this order; LzmaGpu_7zOpen and the reference's reader read it."""
    text = native.gen("text", 903, 9000)
    methods = [L.sz_method(L.SZ_M_COPY)]
    a = S.Archive(L, methods)
    a.empty("first", True).group(0, [("a", text[:4000])]).empty("middle.txt")
    a.group(0, [("b", text[4000:4001]), ("c", text[4001:])]).empty("last", True)
    src, items, n, names, names_len = a.build()
    r, folders, _, _ = L.sz_write_plan(items, n, len(src), names_len, methods)
    assert r == OK and [(f.first_file, f.num_files) for f in folders] == [(1, 1), (3, 2)]
    for f in folders:
        f.pack_size = f.unpack_size
    crcs = [zlib.crc32(src[items[i].src_off:items[i].src_off + items[i].size]) for i in range(n)]
    body = text
    r, hdr, sig = L.sz_write_header(folders, items, n, crcs, names, names_len, 0, len(body))
    assert r == OK
    arc = sig + body + hdr
    r, fres, fsz, out, names_out = S.ref_extract(arc)
    assert r == OK and fres == [OK] * 6 and out == text
    assert fsz == [0, 4000, 0, 1, 4999, 0] and names_out == a.names_buffer()
    r, fo, fi, _, _ = L.sz_open(arc)
    assert r == OK and [(f.has_stream, f.is_dir) for f in fi] == [
        (0, 1), (1, 0), (0, 0), (1, 0), (1, 0), (0, 1)]


# ---------------------------------------------------------------- the pack stage on the host

@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return P.load_emu(P.build_emu(tmp_path_factory.mktemp("pack_emu")))


@pytest.fixture(scope="module")
def pack_cases():
    return P.cases()


def test_pack_case_list_covers_what_it_should(emu, pack_cases):
    assert emu.szpack_emu_tile() == P.TILE
    counts = {len(c.pieces) for c in pack_cases}
    assert counts >= {0, 1, P.TILE - 1, P.TILE, P.TILE + 1, P.SECOND + 1}
    al = pack_cases[0]
    w = P.model(al)
    seen = set()
    for p, o in zip(al.pieces[1::2], w["offs"][1::2]):
        n, _ = P.length_of(al, p)
        seen.add((p["off"] % 16, o % 16, n))
    assert seen == {(s, d, n) for s in range(16) for d in range(16) for n in P.LENGTHS}
    for c in pack_cases[1:6]:
        if len(c.pieces) < 3:
            continue
        last = [p["folder"] for p in c.pieces if p["flags"] & P.LAST]
        assert 0 in last and c.n_folders - 1 in last and c.n_folders // 2 in last, c.name
    assert any(p["kind"] == P.COPY and p["base"] == 0 for c in pack_cases for p in c.pieces)
    totals = {P.model(c)["total"][0] for c in pack_cases}
    assert totals == {OK, PARAM, OUTPUT_EOF}


def test_pack_emulator_against_the_model(emu, pack_cases):
    for c in pack_cases:
        want = P.model(c)
        P.check(c, P.run_emu(emu, c, want), want)
        if want["total"][0] != OK:
            assert want["image"] == bytes([P.POISON]) * len(want["image"])


def test_pack_sanitizer_program_over_the_case_list(tmp_path, pack_cases):
    """g++ -O1 -fsanitize=address,undefined, own main, exact-size allocations."""
    exe = P.build_emu(tmp_path, extra=("-O1", "-g", "-fsanitize=address,undefined",
                                       "-fno-sanitize-recover=undefined"), main=True)
    path = str(tmp_path / "cases.bin")
    P.write_case_file(path, pack_cases)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "%d cases, 0 mismatches" % len(pack_cases) in r.stdout

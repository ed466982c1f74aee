"""The 7z writer on the device: SzGpu_PackBatch alone over the emulator's case
list, and LzmaGpu_7zWrite -- every folder's pack stream against the reference's
encoder (LZMA, LZMA2) or the PPMd7 batch encoder and the reference's PPMd7
decoder, the archive against the layout helper around those streams, read back
by the reference's own reader and by LzmaGpu_7zExtractEx; 3,000 folders in one
encode launch with a packed header; the re-encode path; a short dest."""
import ctypes

import pytest

import native
import ppmd7ref
import sevenzenc_cases as S
import sevenzpack_cases as P
import sevenzwrite as W

pytestmark = pytest.mark.gpu
OK, UNSUPPORTED, OUTPUT_EOF = S.OK, S.UNSUPPORTED, S.OUTPUT_EOF
needs_ref = pytest.mark.skipif(not S.have_ref_reader(), reason="reference library not built")


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def dev(b):
    import numpy as np
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b) or b"\0", dtype=np.uint8).copy()).cuda()


def run_device(L, case, want):
    """SzGpu_PackBatch over one case: (total, offs, sizes, image)."""
    import torch
    n = len(case.pieces)
    pieces, lz, l2, pp = P.tables(case)
    keep = [dev(bytes(pieces)), dev(bytes(lz)), dev(bytes(l2)), dev(bytes(pp))]
    a = L.SzPackArgs()
    a.d_pieces, a.n, a.n_folders = keep[0].data_ptr(), n, case.n_folders
    for k, b in enumerate(case.bases):
        if b is not None:
            t = dev(bytes(b) + bytes([P.POISON]) * 16)
            assert t.data_ptr() % 16 == 0
            keep.append(t)
            a.bases[k] = t.data_ptr()
    a.d_lzma, a.n_lzma = keep[1].data_ptr(), len(case.res[P.LZMA])
    a.d_lzma2, a.n_lzma2 = keep[2].data_ptr(), len(case.res[P.LZMA2])
    a.d_ppmd, a.n_ppmd = keep[3].data_ptr(), len(case.res[P.PPMD])
    image = want["out_cap"] + P.GUARD
    d_out = torch.full((case.out_mis + image,), P.POISON, dtype=torch.uint8, device="cuda")
    d_scr = torch.full((L.sz_pack_scratch(n),), -1, dtype=torch.int64, device="cuda")
    d_off = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    d_size = torch.full((max(case.n_folders, 1),), -1, dtype=torch.int64, device="cuda")
    d_tot = torch.full((16,), 0xEE, dtype=torch.uint8, device="cuda")
    a.d_out, a.out_cap = d_out.data_ptr() + case.out_mis, want["out_cap"]
    a.d_scratch, a.d_piece_off = d_scr.data_ptr(), d_off.data_ptr()
    a.d_folder_size, a.d_total = d_size.data_ptr(), d_tot.data_ptr()
    torch.cuda.synchronize()
    assert L.sz_pack_batch_device(a) == OK, L.last_error()
    torch.cuda.synchronize()
    tot = P.EncResult.from_buffer_copy(d_tot.cpu().numpy().tobytes())
    out = d_out.cpu().numpy().tobytes()
    assert out[:case.out_mis] == bytes([P.POISON]) * case.out_mis
    return ((tot.res, tot._pad, tot.dest_len), d_off.cpu().tolist()[:n],
            d_size.cpu().tolist()[:case.n_folders], out[case.out_mis:])


def test_pack_batch_alone_over_the_emulators_case_list(L):
    for c in P.cases():
        want = P.model(c)
        P.check(c, run_device(L, c, want), want)


# ---------------------------------------------------------------- archive A

LZ_A = dict(level=1, dict_size=1 << 12, lc=0, lp=0, pb=2)
LZ_B = dict(level=4, dict_size=1 << 16, lc=3, lp=0, pb=2)
LZ_C = dict(level=1, dict_size=1 << 16, lc=3, lp=0, pb=2)


def archive_a(L):
    import bcj2enc
    text = native.gen("text", 910, 200000)
    runs = native.gen("runs", 911, 20000)
    rnd = native.gen("random", 912, 3000)
    xd = bcj2enc.x86_like(913, 24000)
    ad = S.arm_like(914, 16000)
    methods = [L.sz_method(L.SZ_M_COPY),
               L.sz_method(L.SZ_M_LZMA, **LZ_A),
               L.sz_method(L.SZ_M_LZMA, **LZ_B),
               L.sz_method(L.SZ_M_LZMA2, block_size=4096, **LZ_C),
               L.sz_method(L.SZ_M_PPMD, order=2, mem_size=1 << 20),
               L.sz_method(L.SZ_M_PPMD, order=6, mem_size=1 << 22),
               L.sz_method(L.SZ_M_LZMA, filter=L.SZ_FILTER_X86, **LZ_C),
               L.sz_method(L.SZ_M_LZMA, filter=L.SZ_FILTER_ARM, **LZ_C)]
    enc = {1: LZ_A, 2: LZ_B, 3: LZ_C, 6: LZ_C, 7: LZ_C}
    a = S.Archive(L, methods)
    at = [0]

    def cut(n, src=text):
        at[0] += n
        return src[at[0] - n:at[0]]

    a.group(0, [("copy/raw.bin", rnd[:2999])]).group(0, [("copy/t.txt", cut(33))])
    for j, n in enumerate((16384, 4097, 255)):
        a.group(1, [(f"lc0/{j}.txt", cut(n))])
    for j, n in enumerate((16000, 8191, 17)):
        a.group(2, [(f"l4/{j}.txt", cut(n))])
    a.group(2, [("l4/runs.bin", runs[:16384])])
    a.group(3, [("lzma2/three-blocks.txt", cut(10000))])
    a.group(3, [("lzma2/exact.txt", cut(4096))])
    a.group(3, [("lzma2/solid-a.txt", cut(5000)), ("lzma2/solid-b.bin", rnd[:1200])])
    a.group(4, [("ppmd2/a.txt", cut(9000))]).group(4, [("ppmd2/b.bin", runs[:3000])])
    a.group(5, [("ppmd6/a.txt", cut(12000))]).group(5, [("ppmd6/b.txt", cut(1))])
    a.group(6, [("x86/code.bin", xd[:16001])]).group(6, [("x86/more.bin", xd[16001:])])
    a.group(7, [("arm/code.bin", ad[:10002])]).group(7, [("arm/more.bin", ad[10002:])])
    a.group(2, [(f"solid/{j:02d}.txt", cut(300 + 37 * j)) for j in range(12)])
    a.group(1, [("one-byte", cut(1))])
    a.group(0, [("copy/ü三.txt", cut(700))])
    a.empty("empty.txt").empty("a/dir", True)
    assert len(a.item_names()) == 37
    return a, enc


def write(L, a, flags=0, cap=None, workspace_limit=0):
    src, items, n, names, names_len = a.build()
    if cap is None:
        r, _, _, cap = L.sz_write_plan(items, n, len(src), names_len, a.methods)
        assert r == OK
    return L.SzWrite(src, items, n, names, names_len, a.methods, cap, flags, workspace_limit,
                     fill=0xEE)


@pytest.fixture(scope="module")
def written_a(L):
    a, enc = archive_a(L)
    r, n, dest, st = write(L, a)
    assert r == OK, L.last_error()
    assert dest[n:] == b"\xee" * (len(dest) - n)
    return a, enc, dest[:n], st


def pack_streams(L, arc):
    r, fo, fi, names, total = L.sz_open(arc, L.SZ_PPMD)
    assert r == OK
    return [arc[f.pack_off:f.pack_off + f.pack_size] for f in fo], fo


@needs_ref
def test_archive_a_pack_streams_are_the_references(L, written_a):
    a, enc, arc, st = written_a
    packs, fo = pack_streams(L, arc)
    groups = a.groups()
    assert len(packs) == len(groups) == st.folders
    pieces, ppmd_items = 0, []
    for (_, mi, files), got, f in zip(groups, packs, fo):
        m = a.methods[mi]
        data = S.filtered(b"".join(d for _, d in files), m.filter)
        if m.method == L.SZ_M_COPY:
            want, pieces = data, pieces + 1
        elif m.method == L.SZ_M_LZMA:
            e = enc[mi]
            props, want = native.ref_encode(data, level=e["level"], dict_size=e["dict_size"],
                                            lc=e["lc"], lp=e["lp"], pb=e["pb"])
            assert bytes(f.props[:5]) == props, files[0][0]
            pieces += 1
        elif m.method == L.SZ_M_LZMA2:
            e, want = enc[mi], b""
            for o in range(0, len(data), 4096):
                prop, s = native.ref_encode2(data[o:o + 4096], level=e["level"],
                                             dict_size=e["dict_size"], lc=e["lc"], lp=e["lp"],
                                             pb=e["pb"])
                assert s[-1] == 0 and f.props[0] == prop
                want += s[:-1]
                pieces += 1
            want += b"\0"
        else:
            ppmd_items.append((data, m.ppmd_order, m.ppmd_mem_size, got))
            pieces += 1
            continue
        assert got == want, (files[0][0], len(got), len(want))
    assert pieces == st.pieces and len(ppmd_items) == 4
    # PPMd: the batch encoder's stream, which the reference's decoder reads
    descs, src, at = [], b"", 0
    for data, order, mem, got in ppmd_items:
        cap = len(data) + len(data) // 2 + 64
        descs.append(dict(src_off=len(src), src_len=len(data), dst_off=at, dst_cap=cap,
                          order=order, mem_size=mem))
        src += data
        at += cap
    r, res, out = L.ppmd7_encode_batch_host(L.ppmd7_make_enc_descs(descs), len(descs), src,
                                            bytes(at))
    assert r == OK
    for k, (data, order, mem, got) in enumerate(ppmd_items):
        d = descs[k]
        assert res[k].res == OK and got == out[d["dst_off"]:d["dst_off"] + res[k].dest_len], k
        assert ppmd7ref.decode(got, order, mem, len(data)) == (0, len(data), len(got), data), k


def test_archive_a_equals_the_layout_helper_around_its_own_streams(L, written_a):
    a, enc, arc, st = written_a
    packs, fo = pack_streams(L, arc)
    helper = [S.helper_folder(L, a.methods[mi], files, got, bytes(f.props[:f.props_size]))
              for (_, mi, files), got, f in zip(a.groups(), packs, fo)]
    assert arc == W.archive(helper, a.empties())
    assert st.pack_bytes == sum(len(p) for p in packs)
    assert st.header_bytes == len(arc) - 32 - st.pack_bytes
    assert (st.encode_launches, st.reencoded) == (3, 0)   # one launch per kind


@needs_ref
def test_archive_a_through_the_reference_reader(L, written_a):
    a, enc, arc, st = written_a
    r, fres, fsz, out, names = S.ref_extract(arc)
    assert r == OK and names == a.names_buffer()
    want_res, want_out = [], b""
    for e in a.order:
        if e[0] == "empty":
            want_res.append(OK)
            continue
        ppmd = a.methods[e[1]].method == L.SZ_M_PPMD
        for _, d in e[2]:
            want_res.append(UNSUPPORTED if ppmd else OK)
            want_out += b"" if ppmd else d
    assert fres == want_res and out == want_out
    assert want_res.count(UNSUPPORTED) == 4


def test_archive_a_through_7zextract_with_ppmd(L, written_a):
    a, enc, arc, st = written_a
    want = b"".join(a.data_files())
    r, out, fres = L.SzExtract(arc, len(want), flags=L.SZ_PPMD)
    assert r == OK and out == want
    assert fres[:len(a.item_names())] == [OK] * len(a.item_names())


def test_two_calls_give_identical_bytes_whatever_the_workspace_limit(L, written_a):
    a, enc, arc, st = written_a
    r, n, dest, st2 = write(L, a)
    assert r == OK and dest[:n] == arc
    assert (st2.folders, st2.pieces, st2.reencoded) == (st.folders, st.pieces, st.reencoded)
    # a limit that cuts every batch into several launches
    r, n, dest, st3 = write(L, a, workspace_limit=6 << 20)
    assert r == OK and dest[:n] == arc and st3.encode_launches > st.encode_launches


def test_dest_one_byte_short(L, written_a):
    a, enc, arc, st = written_a
    r, n, dest, _ = write(L, a, cap=len(arc) - 1)
    assert (r, n) == (OUTPUT_EOF, len(arc)) and dest == b"\xee" * (len(arc) - 1)
    r, n, dest, _ = write(L, a, cap=len(arc) + 5)
    assert (r, n) == (OK, len(arc)) and dest == arc + b"\xee" * 5


# ---------------------------------------------------------------- archive B, re-encodes

@needs_ref
def test_archive_b_3000_folders_in_one_launch_with_a_packed_header(L):
    text = native.gen("text", 920, 3000 * 300)
    files = [(f"tree/{j // 100:02d}/file{j:04d}.txt", text[300 * j:300 * j + 100 + (j * 7) % 201])
             for j in range(3000)]
    a = S.Archive(L, [L.sz_method(L.SZ_M_LZMA, **LZ_C)])
    for f in files:
        a.group(0, [f])
    r, n, dest, st = write(L, a, flags=L.SZ_WRITE_ENCODE_HEADER)
    assert r == OK, L.last_error()
    assert (st.folders, st.pieces, st.encode_launches, st.reencoded) == (3000, 3000, 1, 0)
    arc = dest[:n]
    assert arc[32 + st.pack_bytes] == W.ENCODED_HEADER and st.header_bytes < 64
    r, fres, fsz, out, names = S.ref_extract(arc)
    assert r == OK and fres == [OK] * 3000 and fsz == [len(d) for _, d in files]
    assert out == b"".join(d for _, d in files) and names == a.names_buffer()
    r, out, fres = L.SzExtract(arc, len(out))
    assert r == OK and out == b"".join(d for _, d in files)


@needs_ref
def test_streams_that_outgrow_their_first_slot_are_encoded_again(L):
    """Random bytes grow under PPMd7 (about 7 % at order 2) and under LZMA
    (1.45 %: 16,384 bytes become 16,626): the first slot is len + len / 128 + 64,
    so the three LZMA and the three PPMd7 streams of random bytes come back."""
    rnd = native.gen("random", 930, 6 * 16384)
    text = native.gen("text", 931, 5000)
    a = S.Archive(L, [L.sz_method(L.SZ_M_LZMA, **LZ_C),
                      L.sz_method(L.SZ_M_PPMD, order=2, mem_size=1 << 20)])
    for j in range(3):
        a.group(0, [(f"lzma/rnd{j}", rnd[16384 * j:16384 * (j + 1)])])
        a.group(1, [(f"ppmd/rnd{j}", rnd[16384 * (3 + j):16384 * (3 + j) + 4096 * (j + 1)])])
    a.group(0, [("lzma/text", text)]).group(1, [("ppmd/text", text[:3000])])
    r, n, dest, st = write(L, a)
    assert r == OK, L.last_error()
    print("re-encoded streams:", st.reencoded, "launches:", st.encode_launches)
    # two first launches and one more per kind; nothing needed the third slot
    assert (st.reencoded, st.encode_launches) == (6, 4)
    arc = dest[:n]
    packs, fo = pack_streams(L, arc)
    for (_, mi, files), got in zip(a.groups(), packs):
        if mi == 0:
            e = LZ_C
            assert got == native.ref_encode(files[0][1], level=e["level"], dict_size=e["dict_size"],
                                            lc=e["lc"], lp=e["lp"], pb=e["pb"])[1], files[0][0]
    r, fres, fsz, out, names = S.ref_extract(arc)
    want_lzma = b"".join(d for e in a.groups() if e[1] == 0 for _, d in e[2])
    assert r == OK and out == want_lzma
    assert fres == [OK, UNSUPPORTED] * 4
    want = b"".join(a.data_files())
    r, out, fres = L.SzExtract(arc, len(want), flags=L.SZ_PPMD)
    assert r == OK and out == want and fres[:8] == [OK] * 8


def test_sevenz_compress(L):
    text = native.gen("text", 940, 30000)
    files = [("a.txt", text[:10000]), ("d", None), ("b.txt", text[10000:10001]), ("e.txt", b""),
             ("c.txt", text[10001:])]
    for kw in (dict(), dict(solid=2, encode_header=True), dict(method=L.SZ_M_LZMA2, block_size=4096),
               dict(method=L.SZ_M_PPMD, order=4), dict(method=L.SZ_M_COPY, filter=L.SZ_FILTER_X86)):
        arc = L.sevenz_compress(files, **kw)
        r, fo, fi, names, total = L.sz_open(arc, L.SZ_PPMD)
        assert r == OK and len(fi) == 5 and total == 30000, kw
        assert len(fo) == (2 if kw.get("solid") else 3), kw
        r, out, fres = L.SzExtract(arc, total, flags=L.SZ_PPMD)
        assert r == OK and out == text and fres[:5] == [OK] * 5, kw

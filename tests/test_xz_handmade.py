"""Hand-made xz files against the reference's two readers (tests/xz_handmade.py).

Reference: Xzs_ReadBackward (XzIn.c:141-306) and XzUnpacker_Code (XzDec.c:
604-870), compiled in place (oracle/ref_shim.c: ref_xz_index, ref_xz_decode)
and recorded in tests/golden/xzh_cases.json (tests/golden/make_golden_xzh.py);
the live reference is used where oracle/_ref is built, the golden file
otherwise.

CPU (no GPU): LzmaGpu_XzIndex is host code.  It restates the backward reader,
so its result code is the backward reader's wherever that one fails; where the
backward reader succeeds and a block header is bad, the code is the one the
forward reader gives for that header (XzBlock_Parse, XzDec_Init,
BraState_SetProps); where both succeed, the blocks, sizes, check types and the
total are the reference's and the blocks tile the output.  The two readers
read differently: the reference's forward reader trusts nothing in the index
until its hash at the end, the backward index is what this project acts on.
A case where the codes may differ for that reason carries code_differs in the
case table and only refusal is asserted for it; a file the reference accepts
is refused only from the STRICTER table.  Files whose unpack sizes sum past
2^63 are refused by the index and never reach a decode call.

GPU (-m gpu): LzmaGpu_XzDecode, one call per file whose index passes; and
every valid file concatenated into one batch.
"""
import hashlib
import os
import sys

import pytest

import native
import xz_handmade as H

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


@pytest.fixture(scope="module")
def table():
    """[(case, the reference's answers)], computed once."""
    return [(c, H.expect(c)) for c in H.all_cases()]


def test_case_table_conditions(table):
    """About 200 named cases in the eight classes; the share of code_differs
    and the STRICTER entries within their bounds (xz_handmade.check_table)."""
    cs = [c for c, _ in table]
    stats = H.check_table(cs, {c["name"]: e for c, e in table})
    assert len(cs) >= 200 and len(stats["classes"]) == 8
    assert 5 * stats["tagged"] <= stats["refused"]
    assert all(len(c["data"]) <= 1200 for c in cs)
    assert all(c["plain"] is None or len(c["plain"]) <= 4 * 64 for c in cs)


def test_golden_file_matches_generator(table):
    """The golden file holds every case under its name with the SHA-256 of the
    file generated now, and -- where the reference is built -- its answers."""
    import json
    with open(H.GOLDEN) as f:
        g = json.load(f)["cases"]
    assert sorted(g) == sorted(c["name"] for c, _ in table)
    for c, e in table:
        assert g[c["name"]]["sha256"] == hashlib.sha256(c["data"]).hexdigest(), c["name"]
        assert g[c["name"]]["liblzma"] == H.liblzma_accepts(c["data"]), c["name"]
        if H.have_ref():
            assert g[c["name"]] == e, c["name"]


def check_blocks(c, e, blocks, total):
    """An accepted index against the reference's: streams, blocks, sizes,
    check types, the total, and the tiling of the output."""
    i = e["index"]
    name = c["name"]
    assert len(blocks) == len(i["blocks"]), name
    assert (blocks[-1].stream + 1 if blocks else 0) <= len(i["streams"]), name
    assert total == i["unpack_total"] and total < 1 << 63, name
    off = 0
    for b, (stream, total_size, unpack_size) in zip(blocks, i["blocks"]):
        assert b.stream == stream, name
        assert b.data_off - b.header_off + b.pack_size + b.check_size == total_size, name
        assert b.unpack_size == unpack_size, name
        assert b.check_type == i["streams"][stream], name
        assert b.check_size == H.CHECK_BYTES[b.check_type], name
        # an LZMA2 stream has its end byte at least; the check follows the padded data
        assert b.pack_size >= 1, name
        assert b.check_off == b.data_off + (b.pack_size + (-(b.data_off + b.pack_size) % 4)), name
        assert b.check_off + b.check_size <= len(c["data"]), name
        assert b.dst_off == off and b.dst_off + b.unpack_size <= total, name
        off += b.unpack_size
    assert off == total, name


def test_index_matches_reference(L, table):
    seen = {"overflow": 0, "index": 0, "header": 0, "stricter": 0, "equal": 0, "differs": 0}
    for c, e in table:
        name = c["name"]
        r, blocks, total = L.xz_index(c["data"])
        i = e["index"]
        if H.overflows(e):
            # Xzs_GetUnpackSize overflows or the sum reaches 2^63: refused, with the
            # code the reference gives its own oversized sums (XzIn.c:208-211)
            assert (r, blocks, total) == (H.ARCHIVE, [], 0), name
            assert c["no_gpu"], name
            seen["overflow"] += 1
        elif i["res"] != H.OK:
            if c["code_differs"]:
                assert r != H.OK, name
                seen["differs"] += 1
            else:
                assert r == i["res"], (name, r, i["res"])
            assert (blocks, total) == ([], 0), name
            seen["index"] += 1
        elif H.header_code(e) is not None and not c["code_differs"]:
            assert r == H.header_code(e), (name, r, H.header_code(e))
            seen["header"] += 1
        elif name in H.STRICTER:
            assert H.valid(e) and r != H.OK, name
            assert not H.liblzma_accepts(c["data"]), name
            seen["stricter"] += 1
        elif c["code_differs"] and r != H.OK:
            assert not H.valid(e), name     # a lying index the header walk already refuses
            seen["differs"] += 1
        else:
            assert r == H.OK, (name, r)
            check_blocks(c, e, blocks, total)
            seen["equal"] += 1
    assert seen["overflow"] >= 3 and seen["stricter"] == len(H.STRICTER), seen
    assert min(seen.values()) > 0, seen


def test_index_overflow_boundary(L, table):
    """One byte below 2^63 the index is still the reference's; at 2^63 and past
    2^64 it is refused -- in one stream and across two."""
    by = {c["name"]: (c, e) for c, e in table}
    c, e = by["index/unpack_sum_2_63_minus_1"]
    r, blocks, total = L.xz_index(c["data"])
    assert (r, total) == (0, (1 << 63) - 1) and e["index"]["unpack_total"] == total
    assert blocks[1].dst_off == total - blocks[1].unpack_size - blocks[2].unpack_size
    c, e = by["index/unpack_sum_past_2_64"]
    assert e["index"]["res"] == 0 and e["index"]["unpack_total"] == (1 << 64) - 1
    for name in ("index/unpack_sum_past_2_64", "index/unpack_sum_2_63",
                 "index/unpack_sum_2_63_two_streams"):
        assert L.xz_index(by[name][0]["data"])[0] == H.ARCHIVE, name


def gpu_cases(L, table):
    """The cases whose index passes; the overflow files are not even indexed here."""
    out = []
    for c, e in table:
        if c["no_gpu"] or H.overflows(e):
            continue
        r, blocks, total = L.xz_index(c["data"])
        if r == 0:
            assert total <= H.DEST_CAP
            out.append((c, e, blocks))
    return out


@pytest.mark.gpu
def test_gpu_decode_matches_reference(L, table):
    n_ok = n_bad = 0
    for c, e, _ in gpu_cases(L, table):
        name = c["name"]
        r, out, bad = L.XzDecode(c["data"], H.DEST_CAP)
        d = e["decode"]
        if H.valid(e):
            assert r == 0, (name, r, bad, L.last_error())
            assert len(out) == d["dest_len"] and out == c["plain"], name
            assert hashlib.sha256(out).hexdigest() == d["sha256"], name
            assert bad == -1, name
            n_ok += 1
        else:
            assert r != 0 and out == b"", (name, r)
            assert bad == c["bad_block"], (name, bad)
            if not c["code_differs"]:
                assert d["res"] != 0 and r == d["res"], (name, r, d["res"])
            n_bad += 1
    # every file the reference finishes reached the GPU (but the STRICTER ones),
    # and every file that fails inside a block did
    assert n_ok == sum(H.valid(e) and c["name"] not in H.STRICTER for c, e in table)
    assert n_bad == sum(c["bad_block"] is not None for c, _ in table)
    assert n_ok >= 50 and n_bad >= 25


@pytest.mark.gpu
def test_gpu_batch_of_every_valid_stream(L, table):
    """Every valid hand-made file, concatenated with stream paddings of 0, 4,
    8 and 12 bytes, is one file: all check kinds and filter chains side by side
    in one batch.  A flipped check byte in the middle is reported at its block."""
    files, plain, n_blocks = b"", b"", 0
    for k, (c, e, blocks) in enumerate(gpu_cases(L, table)):
        if H.valid(e):
            files += c["data"] + b"\0" * (4 * (k % 4))
            plain += c["plain"]
            n_blocks += len(blocks)
    r, blocks, total = L.xz_index(files)
    assert r == 0 and total == len(plain) and len(blocks) == n_blocks >= 60
    assert {b.check_type for b in blocks} == set(range(16))
    assert {tuple(b.filter_id[:b.num_filters]) for b in blocks} >= {
        (), (3,), (4, 3), (3, 7, 3), (4,), (5,), (6,), (8,), (9,)}
    r, out, bad = L.XzDecode(files, total)
    assert (r, bad) == (0, -1), (r, bad, L.last_error())
    assert out == plain
    mid = [k for k, b in enumerate(blocks) if b.check_type in (1, 4, 10) and b.unpack_size]
    k = mid[len(mid) // 2]
    r, out, bad = L.XzDecode(H.flip(files, blocks[k].check_off + blocks[k].check_size - 1), total)
    assert (r, out, bad) == (H.CRC, b"", k)

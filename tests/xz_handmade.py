"""Hand-made xz files -- TEST INFRASTRUCTURE (tests/test_xz_handmade.py,
tests/golden/make_golden_xzh.py, tests/fuzz/seeds.py).

An xz file written field by field (stream header, block header, LZMA2 data,
block padding, check, index, footer, stream padding), every field with an
override, so a case can be wrong in exactly one place -- the corners no xz
writer emits, where the container code decides what the GPU is told to do.
Blocks hold at most 64 plain bytes; the LZMA2 data is written by hand: stored
chunks (lzmaenc_min.copy_chunk) or a few compressed chunks from the symbol
encoder (lzmaenc_min.Encoder).  Inputs are generated, never stored; the golden
file (tests/golden/xzh_cases.json) keeps each file's SHA-256 and the
reference's answers.

The answers come from the reference's two readers: the backward index
(Xzs_ReadBackward, XzIn.c:141-306; oracle ref_xz_index) and the forward decoder
(XzUnpacker_Code, XzDec.c:604-870; ref_xz_decode) -- live where oracle/_ref is
built, else from the golden file (expect()).

Xz_ReadBackward's padding scan reads tempBuf[j - 1] at j == 0 when a scanned
window holds only zeros (XzIn.c:170-171).  Every input here stays clear of that
line: stream padding of at most 64 bytes, never longer than the bytes before
it, and no file longer than the scan's 1 KiB window that ends in a window of
zeros.

The reference's MixCoder keeps a freed buffer when the filter chain changes
between two blocks of one XzUnpacker (XzDec_Init -> MixCoder_Free, XzDec.c:
329-341, 570-579), so filter chains appear in single-block files only.

A case is a dict: name, cls (the class of the issue's list), data (the file),
plain (the decoded bytes of a file that is valid, else None), bad_block (the
first block a forward reader fails at, where the file fails inside a block),
code_differs (a reason, where the two readers examine different fields and
only refusal is compared), no_gpu (files that never go to a decode call).
"""
import ctypes
import hashlib
import json
import lzma
import os
import struct
import zlib

import lzmaenc_min as M
import native
from xzwrite import check_value, varint

GOLDEN = os.path.join(native.ROOT, "tests", "golden", "xzh_cases.json")
MAGIC = b"\xfd7zXZ\0"
# XzFlags_GetCheckSize (Xz.c:40-44) as the xz file format lists it
CHECK_BYTES = [0, 4, 4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64]
VERIFIED = (0, 1, 4, 10)   # XzCheck_Final returns 0 for the others (XzDec.c:755)
OK, DATA, MEM, CRC, UNSUPPORTED, READ, ARCHIVE, NO_ARCHIVE = 0, 1, 2, 3, 4, 8, 16, 17
DEST_CAP = 4096
ID_DELTA, ID_X86, ID_PPC, ID_IA64, ID_ARM, ID_ARMT, ID_SPARC, ID_LZMA2 = 3, 4, 5, 6, 7, 8, 9, 0x21
BRA_ALIGN = {ID_X86: 1, ID_PPC: 4, ID_IA64: 16, ID_ARM: 4, ID_ARMT: 2, ID_SPARC: 4}


def crc32(b):
    return struct.pack("<I", zlib.crc32(bytes(b)))


def flip(b, at, mask=1):
    b = bytearray(b)
    b[at] ^= mask
    return bytes(b)


# ------------------------------------------------------------------ LZMA2 data

def stored(plain, control=1):
    """One stored chunk (control 1: dictionary reset) and the end byte."""
    return (M.copy_chunk(control, plain) if plain else b"") + b"\0"


def _symbols(e, plain, at=0):
    """plain[at:] as literals and the longest earlier match of 2 or more bytes."""
    i = at
    while i < len(plain):
        best, dist = 0, 0
        for d in range(1, i + 1):
            n = 0
            while i + n < len(plain) and plain[i + n - d] == plain[i + n] and n < 273:
                n += 1
            if n > best:
                best, dist = n, d
        if best >= 2:
            e.match(dist, best)
            i += best
        else:
            e.literal(plain[i])
            i += 1


def compressed(plain):
    """One LZMA chunk of mode 3 (dictionary, state and props reset), lc3 lp0 pb2."""
    e = M.Encoder()
    _symbols(e, plain)
    return M.lz_chunk(0xE0, e.finish(), len(plain), prop=0x5D) + b"\0"


def compressed3(plain):
    """Three chunks: stored with a dictionary reset, LZMA of mode 2 (new props,
    state reset) whose matches reach into the stored bytes, LZMA of mode 0 (the
    model goes on under a fresh range coder)."""
    a, b = len(plain) // 3, 2 * len(plain) // 3
    e = M.Encoder()
    e.stored(plain[:a])
    _symbols(e, plain[:b], a)
    c2 = e.restart_rc()
    _symbols(e, plain, b)
    return (M.copy_chunk(1, plain[:a]) + M.lz_chunk(0xC0, c2, b - a, prop=0x5D) +
            M.lz_chunk(0x80, e.finish(), len(plain) - b) + b"\0")


# ------------------------------------------------------------------ containers

def stream_header(check, flags0=0, magic=MAGIC, crc=None):
    fl = bytes([flags0, check])
    return magic + fl + (crc32(fl) if crc is None else crc)


def check_field(check, plain):
    """The stored check: the real value for the IDs anyone verifies, 4 to 64
    bytes nobody can verify for the reserved ones."""
    if check in VERIFIED:
        return check_value(check, plain)
    return hashlib.sha512(bytes(plain) + bytes([check])).digest()[:CHECK_BYTES[check]]


def filt(fid, props=b"", size=None):
    """A filter record: ID, props size (`size` where it shall lie), props."""
    return varint(fid) + varint(len(props) if size is None else size) + bytes(props)


LZMA2 = filt(ID_LZMA2, b"\0")  # dictionary of 4 KiB


def _field(v):
    return b"" if v is None else (v if isinstance(v, bytes) else varint(v))


def block_header(filters=(LZMA2,), pack=None, unpack=None, flags=0, size=None, pad=None, crc=None):
    """size byte, flags (filter count and the two size bits, `flags` or-ed in),
    the optional size fields (an int, or the bytes of a varint written some
    other way), the filter records, zero padding up to `size` bytes in all
    (the smallest multiple of 4 by default; `pad` where it shall not be zero),
    CRC-32."""
    fl = len(filters) - 1
    fl |= (0x40 if pack is not None else 0) | (0x80 if unpack is not None else 0)
    body = bytes([fl | flags]) + _field(pack) + _field(unpack) + b"".join(filters)
    if size is None:
        size = (1 + len(body) + 4 + 3) // 4 * 4
    room = size - 4 - 1 - len(body)
    assert room >= 0 and size % 4 == 0 and size <= 1024
    h = bytes([size // 4 - 1]) + body + (b"\0" * room if pad is None else pad)
    assert len(h) == size - 4
    return h + (crc32(h) if crc is None else crc)


def block(plain, check, data=None, header=None, pad=None, field=None):
    """(bytes, unpadded size, unpack size) of one block: LZMA2-only header and
    one stored chunk unless given; `pad` / `field` replace the block padding
    and the check field."""
    data = stored(plain) if data is None else data
    header = block_header() if header is None else header
    body = header + data
    body += b"\0" * (-len(body) % 4) if pad is None else pad
    field = check_field(check, plain) if field is None else field
    return body + field, len(header) + len(data) + len(field), len(plain)


def index(records, indicator=0, count=None, pad=None, crc=None):
    """Index of (unpadded, unpack) records; count as an int or the bytes of a varint."""
    ix = bytes([indicator]) + _field(len(records) if count is None else count)
    ix += b"".join(_field(u) + _field(n) for u, n in records)
    ix += b"\0" * (-len(ix) % 4) if pad is None else pad
    return ix + (crc32(ix) if crc is None else crc)


def footer(index_len, check, backward=None, flags0=0, crc=None, magic=b"YZ"):
    back = struct.pack("<I", index_len // 4 - 1 if backward is None else backward)
    back += bytes([flags0, check])
    return (crc32(back) if crc is None else crc) + back + magic


def stream(blocks, check, header=None, ix=None, foot=None, records=None):
    """Stream from block() triples; header / ix / foot replace those parts,
    records the (unpadded, unpack) list the index is written from."""
    out = stream_header(check) if header is None else header
    out += b"".join(b for b, _, _ in blocks)
    if ix is None:
        ix = index([(u, n) for _, u, n in blocks] if records is None else records)
    return out + ix + (footer(len(ix), check) if foot is None else foot)


def one(plain, check=1, **kw):
    """A stream of one block."""
    return stream([block(plain, check, **kw)], check)


def filtered(plain, chain):
    """plain as the encoding side of a filter chain leaves it, from liblzma:
    raw-encode through chain + LZMA2, raw-decode through LZMA2 alone."""
    l2 = {"id": lzma.FILTER_LZMA2, "preset": 0}
    raw = lzma.compress(plain, format=lzma.FORMAT_RAW, filters=list(chain) + [l2])
    return lzma.decompress(raw, format=lzma.FORMAT_RAW, filters=[l2])


# ------------------------------------------------------------------ plain bytes

def text(seed, n):
    """n bytes with repeats (so the compressed chunks hold matches)."""
    words = [b"batch ", b"lane ", b"block ", b"index ", b"xz ", b"check "]
    out, k = b"", seed
    while len(out) < n:
        k = (k * 1103515245 + 12345) & 0x7FFFFFFF
        out += words[(k >> 16) % len(words)]
    return out[:n]


def code_like(n=64):
    """Bytes every branch converter changes: x86 E8 calls, ARM BL (xx xx xx EB),
    PowerPC bl (48 xx xx x1), SPARC call (40 xx xx xx), Thumb BL pairs."""
    b = (b"\x55\x89\xe5\xe8\x10\x00\x00\x00" + b"\x04\x00\x00\xeb" + b"\x48\x00\x01\x01" +
         b"\x40\x00\x00\x20" + b"\x00\xf0\x08\xf8" + b"\xe8\xfc\xff\xff\xff\x90\x90\x90" +
         b"\x08\x00\x00\xeb" + b"\x48\x00\x02\x05" + b"\x7f\xff\xff\xf0" + b"\xff\xf7\xf0\xff")
    return (b * (n // len(b) + 1))[:n]


# ------------------------------------------------------------------ the cases

def _case(out, cls, name, data, plain=None, bad_block=None, code_differs=None, no_gpu=False):
    assert all(c["name"] != name for c in out), name
    out.append({"name": name, "cls": cls, "data": bytes(data), "plain": plain,
                "bad_block": bad_block, "code_differs": code_differs, "no_gpu": no_gpu})


# Files the reference accepts and this project refuses, each with its reason;
# liblzma refuses every one of them too (asserted live by the generator and
# the test).
STRICTER = {
    "block_header/pack_field_plus1": "the pack-size field contradicts the index (XzBlock_Parse "
                                     "stores it, nothing compares it); liblzma refuses",
    "block_header/pack_field_minus1": "as pack_field_plus1",
    "block_header/unpack_field_plus1": "the unpack-size field contradicts the index and the data",
    "block_header/unpack_field_minus1": "as unpack_field_plus1",
    "block_header/both_fields_unpack_wrong": "as unpack_field_plus1, with both fields present",
    "block_header/varint_9_bytes": "as unpack_field_plus1: nine bytes cannot hold less than 2^56",
    "block_header/lzma2_twice": "LZMA2 as a non-last filter: the format allows it only last",
}

INDEX_LIES = ("the forward reader hashes the index it derived and reports a different one as "
              "SZ_ERROR_CRC (XzDec.c:799-801); the backward reader acts on the index")
RUNS_ON = ("the forward reader takes the bytes behind the packed size for the LZMA2 stream's "
           "end and fails at the check; a lane ends at its packed size (SZ_ERROR_DATA)")
SEEK = ("the index points before the start of the file: the reference's seek fails "
        "(SZ_ERROR_READ), here the size comparison does (SZ_ERROR_ARCHIVE)")


def _stream_header_cases(out):
    c = "stream_header"
    p = text(1, 23)
    good = one(p)
    for i in range(6):
        _case(out, c, f"{c}/magic_byte{i}", flip(good, i, 0x40))
    _case(out, c, f"{c}/flags0_nonzero",
          stream([block(p, 1)], 1, header=stream_header(1, flags0=1)))
    _case(out, c, f"{c}/check_id_16",
          stream([block(p, 1)], 1, header=stream_header(0x10)))
    _case(out, c, f"{c}/flags_crc", flip(good, 8))
    for chk in range(16):
        q = text(10 + chk, 5 + 3 * chk)
        _case(out, c, f"{c}/check_id_{chk}", one(q, chk), plain=q)
    for chk in (1, 4, 10):
        q = text(30 + chk, 33)
        f = flip(check_field(chk, q), CHECK_BYTES[chk] - 1, 0x80)
        _case(out, c, f"{c}/check_{chk}_wrong_value", one(q, chk, field=f), bad_block=0)
    q = text(50, 17)
    _case(out, c, f"{c}/check_7_any_value", one(q, 7, field=b"\xa5" * 16), plain=q)


def _block_header_cases(out):
    c = "block_header"
    p = text(2, 40)
    d = stored(p)

    def hdr_case(name, header, ok=False, data=None, plain=None, **kw):
        plain = p if plain is None else plain
        _case(out, c, f"{c}/{name}", one(plain, header=header, data=data),
              plain=plain if ok else None, **kw)

    hdr_case("size_byte_255", block_header(size=1024), ok=True)
    hdr_case("pad_nonzero", block_header(size=16, pad=b"\0\0\0\0\0\1\0"))
    hdr_case("header_crc", flip(block_header(), 8))
    for bits in (0x04, 0x20, 0x3C):
        hdr_case(f"reserved_flags_{bits:02x}", block_header(flags=bits), ok=True)
    hdr_case("pack_field_right", block_header(pack=len(d)), ok=True)
    hdr_case("pack_field_plus1", block_header(pack=len(d) + 1), ok=True)
    hdr_case("pack_field_minus1", block_header(pack=len(d) - 1), ok=True)
    hdr_case("pack_field_zero", block_header(pack=0))
    hdr_case("unpack_field_right", block_header(unpack=len(p)), ok=True)
    hdr_case("unpack_field_plus1", block_header(unpack=len(p) + 1), ok=True)
    hdr_case("unpack_field_minus1", block_header(unpack=len(p) - 1), ok=True)
    hdr_case("both_fields_right", block_header(pack=len(d), unpack=len(p)), ok=True)
    hdr_case("both_fields_unpack_wrong", block_header(pack=len(d), unpack=len(p) + 2), ok=True)
    hdr_case("varint_non_minimal", block_header(unpack=b"\x80\x00"))
    # nine bytes hold 63 bits, the most a size has; a tenth byte is refused
    hdr_case("varint_9_bytes", block_header(unpack=bytes([0x80 | len(p)]) + b"\x80" * 7 + b"\x01"),
             ok=True)
    hdr_case("varint_10_bytes", block_header(unpack=bytes([0x80 | len(p)]) + b"\x80" * 8 + b"\x01"))
    # chains: the bytes stored in the block are what the encoding side leaves
    code = code_like(64)
    chains = {
        "chain_delta_lzma2": ([{"id": lzma.FILTER_DELTA, "dist": 3}],
                              [filt(ID_DELTA, b"\x02")]),
        "chain_x86_delta_lzma2": ([{"id": lzma.FILTER_X86}, {"id": lzma.FILTER_DELTA, "dist": 1}],
                                  [filt(ID_X86), filt(ID_DELTA, b"\x00")]),
        "chain_delta_arm_delta_lzma2": ([{"id": lzma.FILTER_DELTA, "dist": 4},
                                         {"id": lzma.FILTER_ARM},
                                         {"id": lzma.FILTER_DELTA, "dist": 256}],
                                        [filt(ID_DELTA, b"\x03"), filt(ID_ARM),
                                         filt(ID_DELTA, b"\xff")]),
        "chain_x86_start_1": ([{"id": lzma.FILTER_X86, "start_offset": 1}],
                              [filt(ID_X86, struct.pack("<I", 1))]),
        "chain_ppc_start_0x100": ([{"id": lzma.FILTER_POWERPC, "start_offset": 0x100}],
                                  [filt(ID_PPC, struct.pack("<I", 0x100))]),
        "chain_ia64": ([{"id": lzma.FILTER_IA64}], [filt(ID_IA64)]),
        "chain_armt_start_2": ([{"id": lzma.FILTER_ARMTHUMB, "start_offset": 2}],
                               [filt(ID_ARMT, struct.pack("<I", 2))]),
        "chain_sparc": ([{"id": lzma.FILTER_SPARC}], [filt(ID_SPARC)]),
    }
    for name, (lz, recs) in chains.items():
        hdr_case(name, block_header(filters=recs + [LZMA2]), ok=True,
                 data=stored(filtered(code, lz)), plain=code)
    hdr_case("lzma2_not_last", block_header(filters=[LZMA2, filt(ID_DELTA, b"\0")]))
    # the reference takes LZMA2 at any place in a chain (MixCoder_SetFromMethod,
    # XzDec.c:363-372); the format, liblzma and this project only as the last
    hdr_case("lzma2_twice", block_header(filters=[LZMA2, LZMA2]), ok=True, data=stored(stored(p)))
    for fid in (0x0A, 0x20, 1 << 62):
        hdr_case(f"unknown_id_{fid:x}_first", block_header(filters=[filt(fid), LZMA2]))
    hdr_case("unknown_id_20_last", block_header(filters=[filt(0x20, b"\0")]))
    for n in (0, 2):
        hdr_case(f"lzma2_props_{n}", block_header(filters=[filt(ID_LZMA2, b"\0" * n)]))
        hdr_case(f"delta_props_{n}", block_header(filters=[filt(ID_DELTA, b"\0" * n), LZMA2]))
    for fid in sorted(BRA_ALIGN):
        for n in (1, 2, 3, 5):
            hdr_case(f"bra_{fid}_props_{n}", block_header(filters=[filt(fid, b"\0" * n), LZMA2]))
        if BRA_ALIGN[fid] > 1:
            v = struct.pack("<I", BRA_ALIGN[fid] // 2)
            hdr_case(f"bra_{fid}_start_misaligned", block_header(filters=[filt(fid, v), LZMA2]))
    hdr_case("lzma2_prop_40", block_header(filters=[filt(ID_LZMA2, b"\x28")]), ok=True)
    hdr_case("lzma2_prop_41", block_header(filters=[filt(ID_LZMA2, b"\x29")]))
    hdr_case("props_size_20", block_header(filters=[filt(ID_LZMA2, b"\0" * 20)]))
    hdr_case("props_size_21", block_header(filters=[filt(ID_LZMA2, b"\0" * 21)]))
    hdr_case("props_past_header", block_header(filters=[filt(ID_LZMA2, b"\0", size=9)], size=12))
    # size byte 0 is the index indicator: the index below still counts a block
    h = block_header()
    _case(out, c, f"{c}/size_byte_0", one(p, header=b"\0" + h[1:]),
          code_differs="the forward reader takes size byte 0 for the index indicator")


def _block_data_cases(out):
    c = "block_data"
    p = text(3, 64)
    _case(out, c, f"{c}/stored", one(p), plain=p)
    _case(out, c, f"{c}/stored_64_check_none", one(p, 0), plain=p)
    _case(out, c, f"{c}/compressed", one(p, data=compressed(p)), plain=p)
    _case(out, c, f"{c}/compressed_3_chunks", one(p, 4, data=compressed3(p)), plain=p)
    _case(out, c, f"{c}/one_byte", one(b"x"), plain=b"x")
    _case(out, c, f"{c}/empty_block", one(b""), plain=b"")
    _case(out, c, f"{c}/empty_block_sha256", one(b"", 10), plain=b"")
    d = stored(p)
    _case(out, c, f"{c}/end_byte_missing", one(p, data=d[:-1]), bad_block=0, code_differs=RUNS_ON)
    # the LZMA2 stream ends before the packed size the index implies
    _case(out, c, f"{c}/ends_early_zero_tail", one(p, 0, data=d + b"\0" * 4), bad_block=0,
          code_differs=INDEX_LIES)
    _case(out, c, f"{c}/ends_early_nonzero_tail", one(p, data=d + b"\0\0\0\x01"), bad_block=0,
          code_differs=INDEX_LIES)
    # the data decodes to one byte more / fewer than the index and the check say
    for name, q in (("one_byte_more", p[:40] + b"!"), ("one_byte_fewer", p[:39])):
        b = block(p[:40], 1, data=stored(q))
        _case(out, c, f"{c}/{name}", stream([b], 1), bad_block=0, code_differs=INDEX_LIES)
    _case(out, c, f"{c}/no_dict_reset", one(p, data=stored(p, control=2)), bad_block=0)
    _case(out, c, f"{c}/lz_chunk_no_dict_reset",
          one(p, data=b"\xc0" + compressed(p)[1:]), bad_block=0)
    e = compressed(p)
    _case(out, c, f"{c}/compressed_byte_flipped", one(p, data=flip(e, 12, 0x10)), bad_block=0)
    _case(out, c, f"{c}/control_byte_3", one(p, data=b"\x03" + d[1:]), bad_block=0)


def _block_padding_cases(out):
    c = "block_padding"
    for n in (1, 2, 3):
        p = text(4, 4 * 9 + (4 - n))   # header 12 + chunk 3 + len + end byte 1
        b, _, _ = block(p, 1)
        assert (12 + len(stored(p))) % 4 == 4 - n, (n, len(p))
        for k in range(n):
            pad = bytearray(n)
            pad[k] = 0x80
            _case(out, c, f"{c}/pad{n}_byte{k}", one(p, pad=bytes(pad)), bad_block=0)
        _case(out, c, f"{c}/pad{n}_zero", one(p), plain=p)


def _ordering_cases(out):
    c = "ordering"
    p = text(5, 33)
    d = stored(p)
    n = -(12 + len(d)) % 4
    assert n == 3
    _case(out, c, f"{c}/bad_data_and_bad_padding",
          one(p, data=d[:-1] + b"\x03", pad=b"\0\1\0"), bad_block=0)
    _case(out, c, f"{c}/bad_padding_and_bad_check",
          one(p, pad=b"\0\0\1", field=b"\0\0\0\0"), bad_block=0)
    _case(out, c, f"{c}/bad_data_and_bad_check",
          one(p, data=d[:-1] + b"\x03", field=b"\0\0\0\0"), bad_block=0)
    q = [text(60 + i, 20 + i) for i in range(4)]
    good = [block(x, 1) for x in q]
    bad_check = block(q[1], 1, field=b"\1\2\3\4")
    bad_data = block(q[3], 1, data=stored(q[3])[:-1] + b"\x04")
    _case(out, c, f"{c}/check_in_1_data_in_3",
          stream([good[0], bad_check, good[2], bad_data], 1), bad_block=1)
    bad_data1 = block(q[1], 1, data=stored(q[1])[:-1] + b"\x04")
    bad_pad = block(q[2], 1, pad=b"\1" * (-(12 + len(stored(q[2]))) % 4))
    assert len(bad_pad[0]) == len(good[2][0]) and bad_pad[0] != good[2][0]
    _case(out, c, f"{c}/data_in_1_padding_in_2",
          stream([good[0], bad_data1, bad_pad, good[3]], 1), bad_block=1)
    _case(out, c, f"{c}/padding_in_2_check_in_1_reversed",
          stream([good[0], bad_check, bad_pad, good[3]], 1), bad_block=1)


def _index_cases(out):
    c = "index"
    q = [text(70 + i, 11 + 9 * i) for i in range(3)]
    bl = [block(x, 1) for x in q]
    rec = [(u, n) for _, u, n in bl]
    hdr = stream_header(1)

    def ix_case(name, ix, foot=None, **kw):
        _case(out, c, f"{c}/{name}", stream(bl, 1, ix=ix, foot=foot), **kw)

    _case(out, c, f"{c}/three_blocks", stream(bl, 1), plain=b"".join(q))
    ix_case("indicator_nonzero", index(rec, indicator=1))
    ix_case("count_plus1", index(rec, count=4))
    ix_case("count_minus1", index(rec, count=2))
    ix_case("count_non_minimal", index(rec, count=b"\x83\x00"))
    ix_case("count_2_63_minus_1", index(rec, count=b"\xff" * 8 + b"\x7f"))
    # a larger sum puts the stream's start before the file's, a smaller one
    # where no magic is; one byte fewer in the middle block leaves the
    # layout alone and takes the block's end byte away
    for k, delta, why in (("zero", None, None), ("plus1", 1, SEEK), ("minus1", -1, INDEX_LIES),
                          ("plus4", 4, SEEK), ("minus4", -4, None)):
        r = list(rec)
        r[1] = (0 if delta is None else r[1][0] + delta, r[1][1])
        ix_case(f"unpadded_{k}", index(r), code_differs=why, bad_block=1 if delta == -1 else None)
    for k, delta in (("plus1", 1), ("minus1", -1)):
        r = list(rec)
        r[1] = (r[1][0], r[1][1] + delta)
        ix_case(f"unpack_{k}", index(r), bad_block=1, code_differs=INDEX_LIES)
    ix_case("records_swapped", index([rec[1], rec[0], rec[2]]), code_differs=INDEX_LIES)
    for k in (0, 1):    # two records leave two bytes of index padding
        pad = bytearray(2)
        pad[k] = 1
        _case(out, c, f"{c}/padding_byte{k}_nonzero",
              stream(bl[:2], 1, ix=index(rec[:2], pad=bytes(pad))))
    assert len(index(rec[:2])) == 12
    ix = index(rec)
    ix_case("index_crc", flip(ix, len(ix) - 1))
    ix_case("record_varint_non_minimal",
            index([rec[0], (bytes([0x80 | rec[1][0]]) + b"\0", rec[1][1]), rec[2]]))
    ix_case("record_cut_by_index_size", index(rec[:2], count=3))
    # a block of header and check alone, the index honest about it: no LZMA2
    # stream has fewer bytes than its end byte (line 109's >=)
    nodata = (block_header() + check_field(1, b""), 16, 0)
    _case(out, c, f"{c}/unpadded_is_header_plus_check", stream([bl[0], nodata], 1),
          code_differs="a block without data: the forward reader decodes what follows the header")
    # padded sizes: 2^62 + 2^62 reaches the reference's own bound (XzIn.c:208-211)
    ix_case("padded_sum_2_63", index([(1 << 62, 5), (1 << 62, 5), rec[2]]))
    ix_case("padded_sum_2_62", index([(1 << 61, 5), (1 << 61, 5), rec[2]]), code_differs=SEEK)
    # unpack sizes whose sum wraps 2^64, or reaches 2^63: host calls only
    big = (1 << 63) - 1
    ix_case("unpack_sum_past_2_64", index([(rec[0][0], big), (rec[1][0], big), (rec[2][0], 3)]),
            no_gpu=True)
    ix_case("unpack_sum_2_63", index([(rec[0][0], big), (rec[1][0], 1), rec[2]]), no_gpu=True)
    ix_case("unpack_sum_2_63_minus_1", index([(rec[0][0], big - rec[1][1] - rec[2][1]),
                                               rec[1], rec[2]]), no_gpu=True)
    two = stream(bl[:2], 1, ix=index([(rec[0][0], 1 << 62), rec[1]]))
    _case(out, c, f"{c}/unpack_sum_2_63_two_streams",
          two + stream(bl[1:], 1, ix=index([(rec[1][0], 1 << 62), rec[2]])), no_gpu=True)
    assert hdr == two[:12]


def _footer_cases(out):
    c = "footer"
    q = [text(80 + i, 30 + i) for i in range(2)]
    bl = [block(x, 4) for x in q]
    ix = index([(u, n) for _, u, n in bl])

    def ft(name, foot, **kw):
        _case(out, c, f"{c}/{name}", stream(bl, 4, foot=foot), **kw)

    good = footer(len(ix), 4)
    ft("crc", flip(good, 0))
    ft("backward_plus1", footer(len(ix), 4, backward=len(ix) // 4))
    ft("backward_minus1", footer(len(ix), 4, backward=len(ix) // 4 - 2))
    ft("backward_past_start", footer(len(ix), 4, backward=0x1000), code_differs=SEEK)
    ft("flags_differ_from_header", footer(len(ix), 1))
    ft("flags_differ_check_none", footer(len(ix), 0))
    ft("magic_byte0", good[:10] + b"yZ")
    ft("magic_byte1", good[:10] + b"Y\x00")
    ft("flags_unsupported", footer(len(ix), 0x14))
    ft("flags0_nonzero", footer(len(ix), 4, flags0=0x80))
    ft("flags_unsupported_and_crc", flip(footer(len(ix), 0x14), 1))


def _streams_cases(out):
    c = "streams"
    q = [text(90 + i, 7 + 13 * i) for i in range(4)]
    checks = (1, 4, 10, 0)
    st = [stream([block(q[i], checks[i], data=compressed(q[i]) if i & 1 else None)], checks[i])
          for i in range(4)]
    empty = stream([], 1)
    for n in (2, 3, 4):
        _case(out, c, f"{c}/{n}_streams", b"".join(st[:n]), plain=b"".join(q[:n]))
    _case(out, c, f"{c}/empty_stream", empty, plain=b"")
    _case(out, c, f"{c}/empty_streams_between", empty + st[0] + empty + empty + st[1] + empty,
          plain=q[0] + q[1])
    two = stream([block(q[0], 4), block(q[1], 4)], 4)
    for n in (4, 8, 64):
        _case(out, c, f"{c}/padding_{n}", st[0] + b"\0" * n + st[1] + b"\0" * n,
              plain=q[0] + q[1])
    for n in (1, 2, 3, 5):
        _case(out, c, f"{c}/padding_{n}_between", st[0] + b"\0" * n + st[1])
        _case(out, c, f"{c}/padding_{n}_at_end", st[0] + st[1] + b"\0" * n)
    _case(out, c, f"{c}/zeros_before_first", b"\0" * 4 + st[0])
    _case(out, c, f"{c}/first_stream_footer_crc", flip(st[0], len(st[0]) - 12) + st[1])
    _case(out, c, f"{c}/first_stream_check", flip(st[0], len(st[0]) - 28) + st[1], bad_block=0)
    _case(out, c, f"{c}/first_stream_magic", flip(st[0], 1) + st[1])
    _case(out, c, f"{c}/last_stream_header_magic", st[0] + flip(st[1], 0))
    _case(out, c, f"{c}/last_stream_check", st[0] + flip(st[1], len(st[1]) - 28, 0x40),
          bad_block=1)
    _case(out, c, f"{c}/trailing_nonzero_4", st[0] + b"junk")
    _case(out, c, f"{c}/trailing_nonzero_after_padding", st[0] + b"\0\0\0\0" + b"\0\0\0\1")
    # a valid two-block file cut at every structural boundary, and at every short length
    parts = [6, 2, 4]                                   # magic, flags, CRC
    for x in q[:2]:
        parts += [8, 4, len(stored(x)), -(12 + len(stored(x))) % 4, 8]
    ixl = len(two) - 12 - sum(parts)
    parts += [1, 1, ixl - 6, 4, 4, 4, 2, 2]             # index, footer fields
    assert sum(parts) == len(two)
    at, cuts = 0, []
    for n in parts[:-1]:
        at += n
        if n and at > 40:
            cuts.append(at)
    for n in cuts:
        _case(out, c, f"{c}/cut_at_boundary_{n}", two[:n])
    for n in range(41):
        _case(out, c, f"{c}/cut_at_length_{n}", two[:n])
    _case(out, c, f"{c}/second_stream_cut_to_its_header", st[0] + st[1][:12])


def cases():
    out = []
    for f in (_stream_header_cases, _block_header_cases, _block_data_cases, _block_padding_cases,
              _ordering_cases, _index_cases, _footer_cases, _streams_cases):
        f(out)
    return out


_cases = None


def all_cases():
    global _cases
    if _cases is None:
        _cases = cases()
    return _cases


def classes(cs):
    out = {}
    for c in cs:
        out.setdefault(c["cls"], []).append(c)
    return out


# ------------------------------------------------------------------ the reference

_sp = ctypes.POINTER(ctypes.c_size_t)


def have_ref():
    return os.path.exists(native.REF_CONT_SO) and hasattr(native.ref_cont(), "ref_xz_index")


def _lib():
    lib = native.ref_cont()
    if not getattr(lib, "_xzh_declared", False):
        lib.ref_xz_decode.restype = ctypes.c_int
        lib.ref_xz_decode.argtypes = [ctypes.c_char_p, _sp, ctypes.c_char_p, _sp, native.int_p,
                                      native.int_p]
        lib.ref_xz_index.restype = ctypes.c_int
        lib.ref_xz_index.argtypes = [ctypes.c_char_p, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_uint), ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, _sp,
                                     ctypes.POINTER(ctypes.c_ulonglong)]
        lib._xzh_declared = True
    return lib


def ref_index(data, cap=64):
    """ref_xz_index: {res, streams: [flags], blocks: [[stream, totalSize, unpackSize]],
    unpack_total} in file order; unpack_total 2^64 - 1 is the reference's overflow value."""
    ns, nb, tot = ctypes.c_uint(0), ctypes.c_size_t(0), ctypes.c_ulonglong(0)
    fl = (ctypes.c_ushort * cap)()
    bl = (ctypes.c_ulonglong * (3 * cap))()
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    res = _lib().ref_xz_index(buf, len(data), ctypes.byref(ns), fl, cap, bl, cap,
                              ctypes.byref(nb), ctypes.byref(tot))
    assert ns.value <= cap and nb.value <= cap
    return {"res": res, "streams": list(fl)[:ns.value],
            "blocks": [list(bl[3 * i:3 * i + 3]) for i in range(nb.value)],
            "unpack_total": tot.value}


def ref_decode(data):
    """ref_xz_decode over the whole file: {res, status, dest_len, src_len, finished, sha256}."""
    out = ctypes.create_string_buffer(DEST_CAP)
    dl, sl = ctypes.c_size_t(DEST_CAP), ctypes.c_size_t(len(data))
    st, done = ctypes.c_int(-1), ctypes.c_int(0)
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    res = _lib().ref_xz_decode(out, ctypes.byref(dl), buf, ctypes.byref(sl), ctypes.byref(st),
                               ctypes.byref(done))
    return {"res": res, "status": st.value, "dest_len": dl.value, "src_len": sl.value,
            "finished": done.value, "sha256": hashlib.sha256(out.raw[:dl.value]).hexdigest()}


def liblzma_accepts(data):
    """Whether liblzma (Python's lzma) decodes the whole file."""
    try:
        lzma.decompress(data, format=lzma.FORMAT_XZ)
        return True
    except (lzma.LZMAError, EOFError):
        return False


def record(c):
    return {"sha256": hashlib.sha256(c["data"]).hexdigest(), "index": ref_index(c["data"]),
            "decode": ref_decode(c["data"]), "liblzma": liblzma_accepts(c["data"])}


_golden = None


def expect(c):
    """The reference's answers for a case: live where oracle/_ref is built, else
    the golden file's (whose SHA-256 of the input must match the generated file)."""
    global _golden
    if have_ref():
        return record(c)
    if _golden is None:
        with open(GOLDEN) as f:
            _golden = json.load(f)["cases"]
    g = _golden[c["name"]]
    assert g["sha256"] == hashlib.sha256(c["data"]).hexdigest(), c["name"]
    return g


def overflows(e):
    """The index's unpack sizes wrap 2^64 (the reference's overflow value) or reach 2^63."""
    return e["index"]["res"] == OK and e["index"]["unpack_total"] >= 1 << 63


def header_code(e):
    """Where the backward index succeeds and the forward reader fails with a
    code only a block header gives it (XzBlock_Parse: SZ_ERROR_ARCHIVE;
    XzDec_Init / *_SetProps: SZ_ERROR_UNSUPPORTED, SZ_ERROR_MEM), that code."""
    if e["index"]["res"] == OK and e["decode"]["res"] in (ARCHIVE, UNSUPPORTED, MEM):
        return e["decode"]["res"]
    return None


def valid(e):
    return e["decode"]["res"] == OK and e["decode"]["finished"] == 1


def refused(c, e):
    """A file this project has to refuse: the forward reader does not finish
    it, or it is in STRICTER."""
    return not valid(e) or c["name"] in STRICTER


def check_table(cs, answers):
    """The conditions on the case table, given the reference's answers by case
    name: plain bytes exactly where the reference finishes the file, and the
    bytes it wrote; a tag only on refused cases, on at most one in five of
    them, and on no class as a whole; every STRICTER entry a file the
    reference accepts and liblzma (live) refuses; every file whose unpack
    sizes overflow kept from the GPU.  Returns the counts."""
    per, n_refused, n_tagged = {}, 0, 0
    for c in cs:
        e = answers[c["name"]]
        k = per.setdefault(c["cls"], [0, 0, 0])
        k[0] += 1
        assert (c["plain"] is not None) == valid(e), c["name"]
        if valid(e):
            assert e["decode"]["sha256"] == hashlib.sha256(c["plain"]).hexdigest(), c["name"]
            assert e["decode"]["dest_len"] == len(c["plain"]), c["name"]
        if refused(c, e):
            k[1] += 1
            n_refused += 1
            if c["code_differs"]:
                k[2] += 1
                n_tagged += 1
        else:
            assert not c["code_differs"] and c["bad_block"] is None, c["name"]
        assert c["no_gpu"] or not overflows(e), c["name"]
    names = {c["name"]: c for c in cs}
    for name in STRICTER:
        assert valid(answers[name]) and not liblzma_accepts(names[name]["data"]), name
    for cls, k in per.items():
        assert k[2] < k[0], f"class {cls} consists only of tagged cases"
    assert 5 * n_tagged <= n_refused, (n_tagged, n_refused)
    return {"classes": per, "refused": n_refused, "tagged": n_tagged}

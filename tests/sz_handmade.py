"""Hand-made 7z headers -- TEST INFRASTRUCTURE (tests/test_7z_handmade.py,
tests/golden/make_golden_szh.py, tests/fuzz/seeds.py).

A 7z archive written property by property (start header, pack info, folders,
coders, bind pairs, unpack sizes, substreams, files info), every field with an
override and both CRCs re-signed, so a case can be odd in exactly one place --
the headers no 7z writer emits, where sevenz_capi.hip decides which byte ranges
the decode, filter and CRC kernels are given.  Archives are at most 2 KiB, a
folder's output at most 256 bytes.  The coder data
is written by hand: Copy, raw LZMA from the symbol encoder (lzmaenc_min.Encoder),
LZMA2 chunks (xz_handmade.compressed / stored), BCJ2 streams from
tests/bcj2enc.py -- nothing from an installed liblzma, so the archives are the
same bytes everywhere.  Inputs are generated, never stored; the golden file
(tests/golden/szh_cases.json) keeps each archive's SHA-256 and the reference's
answers.

The answers come from the reference's reader: SzArEx_Open (7zIn.c:1214-1320)
and SzArEx_Extract (7zIn.c:1322-1402) through oracle/ref_shim.c (ref_7z_info,
ref_7z_extract) -- live where oracle/_ref is built, else from the golden file
(expect()).

Some headers make the reference read outside its own arrays or through a null
pointer (files with streams and no SubStreamsInfo, more stream files than
substreams, a second substreams kCRC section, folders that need more pack sizes
than PackInfo gave, a packed header without PackInfo).  Such a case carries the tag ref_undefined and is
never handed to the reference: the project has to refuse it with
SZ_ERROR_ARCHIVE.  That no untagged case rests on undefined
behaviour is shown by the generator, which runs each through the reference
under the host sanitizers (oracle/_ref/ref_7z_check, run_sanitized()).

A case is a dict: name, cls (the class of the list below), data (the archive),
tags (a set: ref_undefined; ref_unset -- the reference opens the archive and
leaves file sizes unset, which are then not compared; code_differs -- only
refusal is compared, the reason in DIFFERS; packed -- the header is decoded on the device at open),
no_gpu (archives that never go to an extract call).  For a code_differs case
that opens, the files' extract results are compared as failing or not.
"""
import ctypes
import hashlib
import json
import os
import struct
import subprocess
import tempfile
import zlib

import bcj2enc
import lzmaenc_min as M
import native
import xz_handmade as X
from sevenzwrite import bools, coder, method_id, number

GOLDEN = os.path.join(native.ROOT, "tests", "golden", "szh_cases.json")
CHECK_EXE = os.path.join(native.ROOT, "oracle", "_ref", "ref_7z_check")
CLASSES = ("start", "numbers", "top", "packinfo", "coders", "unpackinfo", "substreams", "files",
           "packed", "extract")
(OK, DATA, MEM, CRC_ERR, UNSUPPORTED, PARAM, INPUT_EOF, OUTPUT_EOF, READ, FAIL, ARCHIVE,
 NO_ARCHIVE) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 16, 17
OUTSIDE = -1   # ref_shim.c REF_7Z_OUTSIDE: OK reported for a range outside the folder's buffer
NO_FOLDER = 0xFFFFFFFF
MAX_ARCHIVE, MAX_FOLDER_OUT = 2048, 256
# What the reference may ask of its allocator for a case: everything a header
# states stays below 1 MiB; the one larger request is the LZMA probability table
# of lc + lp = 12 (props byte 224, a case the list asks for): 2 * (1846 + (768 <<
# 12)) bytes, 6.3 MB, the format's maximum.
MAX_REF_ALLOC = 1 << 23

# property ids (7z.h:17-45)
(END, HEADER, ARCHIVE_PROPS, ADDITIONAL_STREAMS, MAIN_STREAMS, FILES, PACK_INFO, UNPACK_INFO,
 SUBSTREAMS, SIZE, CRC, FOLDER, CODERS_UNPACK_SIZE, NUM_UNPACK_STREAM, EMPTY_STREAM, EMPTY_FILE,
 ANTI, NAME, CTIME, ATIME, MTIME, WIN_ATTRIB, COMMENT, ENCODED_HEADER, START_POS, DUMMY) = range(26)
M_COPY, M_LZMA, M_LZMA2, M_BCJ, M_ARM, M_BCJ2 = 0, 0x030101, 0x21, 0x03030103, 0x03030501, 0x0303011B
M_PPC, M_ARMT, M_DELTA, M_PPMD = 0x03030205, 0x03030701, 3, 0x030401

# Cases the reference accepts and this project refuses, with the reason from
# DESIGN.md §3 (7z).  Everything else the reference accepts, the project accepts.
STRICTER = {
    "numbers/unpack_size_2_64_minus_1":
        "a folder size sum that wraps or reaches 2^63 ends the open with SZ_ERROR_MEM, what "
        "SzArEx_Extract returns for a folder it cannot allocate",
    "packed/unpack_size_one_long_lzma2":
        "an LZMA2 stream that ends one byte before the stated size fails with SZ_ERROR_DATA; the "
        "reference takes the header with an unset last byte",
}

# code_differs: why only refusal is compared
SHORT = ("DESIGN.md §3: the reference takes an end marker in front of the stated size as the end "
         "of the folder and leaves the rest of its buffer unset (then fails the CRC over it); "
         "here the folder fails with SZ_ERROR_DATA")
DIFFERS = {
    "packinfo/pos_2_63": "a pack position >= 2^63 is a negative seek in the shim: every file "
                         "fails there with SZ_ERROR_READ, here as for any position past the end",
    "unpackinfo/size_one_more_lzma": SHORT,
    "unpackinfo/size_one_more_lzma2": SHORT,
    "packed/unpack_size_one_long_lzma": SHORT,
    "numbers/folder_count_beyond_bytes": "DESIGN.md §3: a folder count the header bytes cannot "
                                         "describe is SZ_ERROR_ARCHIVE before any allocation",
}


def crc32(b):
    return zlib.crc32(bytes(b)) & 0xFFFFFFFF


def u32(v):
    return struct.pack("<I", v & 0xFFFFFFFF)


def N(v):
    """A 7z number; bytes pass through (a number written some other way)."""
    return v if isinstance(v, (bytes, bytearray)) else number(v)


def wide(v, n):
    """v in the form with n extra bytes (n = 8: the 9-byte form), minimal or not."""
    assert 0 <= n <= 8 and (n == 8 or (v >> (8 * n)) < (1 << (7 - n)))
    if n == 8:
        return b"\xff" + struct.pack("<Q", v)
    return bytes([((0xFF00 >> n) & 0xFF) | (v >> (8 * n))]) + (v & ((1 << (8 * n)) - 1)).to_bytes(n, "little")


# ------------------------------------------------------------------ the assembler

def sign(hdr, body=b"", off=None, size=None, hcrc=None, scrc=None, major=0, minor=4, tail=b"",
         sig=b"7z\xbc\xaf\x27\x1c"):
    """The archive: signature header (both CRCs re-signed unless given), body
    (pack streams and gaps), next header, tail."""
    start = struct.pack("<QQI", len(body) if off is None else off,
                        len(hdr) if size is None else size, crc32(hdr) if hcrc is None else hcrc)
    return (sig + bytes([major, minor]) + u32(crc32(start) if scrc is None else scrc) + start +
            body + hdr + tail)


def digests(vals):
    """A digest vector: allDefined = 1 where every value is given, else the bit vector."""
    if all(v is not None for v in vals):
        return b"\1" + b"".join(u32(v) for v in vals)
    return b"\0" + bools([v is not None for v in vals]) + b"".join(u32(v) for v in vals if v is not None)


def pack_info(sizes, pos=0, n=None, pre=b"", crc=None, post=b"", end=b"\0"):
    out = bytes([PACK_INFO]) + N(pos) + N(len(sizes) if n is None else n) + pre + bytes([SIZE])
    out += b"".join(N(s) for s in sizes)
    if crc is not None:
        out += bytes([CRC]) + crc
    return out + post + end


def cod(m, props=None, nin=None, nout=None, alt=(), idb=None, flags=0):
    """A coder record: main byte (id size | 0x10 stream counts | 0x20 properties |
    0x80 alternative methods follow), id, counts, properties, alternatives (each
    a record of its own; 0x80 is set on all but the last)."""
    idb = method_id(m) if idb is None else idb
    b = len(idb) | flags | (0x10 if nin is not None else 0) | (0x20 if props is not None else 0)
    out = bytes([b | (0x80 if alt else 0)]) + idb
    if nin is not None:
        out += N(nin) + N(nout)
    if props is not None:
        out += number(len(props)) + props
    for k, a in enumerate(alt):
        out += bytes([a[0] | 0x80 if k + 1 < len(alt) else a[0] & 0x7F]) + a[1:]
    return out


def folder_rec(coders, binds=(), packs=None, nc=None):
    out = N(len(coders) if nc is None else nc) + b"".join(coders)
    out += b"".join(N(i) + N(o) for i, o in binds)
    if packs is not None:
        out += b"".join(N(p) for p in packs)
    return out


def unpack_info(folders, usizes, crc=None, nf=None, external=0, pre=b"", mid=b"", post=b"",
                end=b"\0"):
    out = bytes([UNPACK_INFO]) + pre + bytes([FOLDER]) + N(len(folders) if nf is None else nf)
    out += bytes([external]) + b"".join(folders) + mid + bytes([CODERS_UNPACK_SIZE])
    out += b"".join(N(u) for u in usizes)
    if crc is not None:
        out += bytes([CRC]) + crc
    return out + post + end


def substreams(nums=None, sizes=None, crc=None, pre=b"", mid=b"", post=b"", end=b"\0"):
    out = bytes([SUBSTREAMS]) + pre
    if nums is not None:
        out += bytes([NUM_UNPACK_STREAM]) + b"".join(N(n) for n in nums)
    out += mid
    if sizes is not None:
        out += bytes([SIZE]) + b"".join(N(s) for s in sizes)
    if crc is not None:
        out += bytes([CRC]) + crc
    return out + post + end


def prop(t, payload, size=None):
    """A files-info property: id, size (`size` where it shall lie), payload."""
    return N(t) + N(len(payload) if size is None else size) + payload


def utf16(names):
    return b"".join(n.encode("utf-16-le") + b"\0\0" for n in names)


def names_prop(names, external=0, raw=None, size=None):
    return prop(NAME, bytes([external]) + (utf16(names) if raw is None else raw), size)


def files_info(n, props=(), end=b"\0"):
    return bytes([FILES]) + N(n) + b"".join(props) + end


def header(streams=None, files=b"", pre=b"", end=b"\0", first=HEADER):
    """kHeader [pre] [kMainStreamsInfo streams kEnd] files kEnd; `streams` is the
    concatenation of the StreamsInfo sections."""
    out = N(first) + pre
    if streams is not None:
        out += bytes([MAIN_STREAMS]) + streams + b"\0"
    return out + files + end


# ------------------------------------------------------------------ coder data

def text(n, seed=0):
    """n printable bytes, no two runs alike: identity under the x86 and ARM filters."""
    out = bytearray()
    k = seed * 7 + 1
    while len(out) < n:
        k = (k * 73 + 41) % 251
        out.append(0x20 + k % 0x5A)
        if k % 5 == 0:
            out += out[-3:]
    return bytes(out[:n])


# x86-flavoured bytes: E8 / E9 rel32 branches, near and far, a Jcc, stray E8 and 0F
X86 = (b"\x55\x89\xe5\xe8\x10\x00\x00\x00\x90\x90\xe9\xf0\xff\xff\xff\x0f\x84\x08\x00\x00\x00"
       b"\xe8\x00\x00\x00\x01\xc3\xe8\xe8\x20\x00\x00\x00\x0f\x0f\x85\xfc\xff\xff\xff\x31\xc0"
       b"\xe8\xff\xff\xff\xff\x5d\xc3\xe9\x00\x00\x00\x80\xe8\x04\x00\x00\x00\x90\xe8")
# ARM: BL instructions (0xEB in the fourth byte) between data words
ARM = (b"\x04\x00\x00\xeb\x00\x00\xa0\xe1\xfe\xff\xff\xeb\x01\x02\x03\x04\x10\x00\x00\xeb"
       b"\x1e\xff\x2f\xe1\x00\x00\x00\xeb\xeb\xeb")


def lzma_raw(plain, marker=True, lc=3, lp=0, pb=2):
    """A raw LZMA stream of `plain`, by hand: literals and the longest earlier
    matches, then the end marker (or none)."""
    e = M.Encoder(lc, lp, pb)
    X._symbols(e, plain)
    if marker:
        e.end_marker()
    return e.finish()


LZMA_PROPS = M.props(3, 0, 2, 4096)


class Fo:
    """One folder: its record (coders, bind pairs, pack stream indices), the
    coders' unpack sizes, its pack streams, the folder CRC (None: undefined),
    its files' sizes and CRCs (None: undefined), and the bytes it decodes to
    where the case knows them."""

    def __init__(self, rec, usizes, streams, data=None, crc=None, files=None, fcrcs=None):
        self.rec, self.usizes, self.streams, self.data, self.crc = rec, list(usizes), list(streams), data, crc
        self.files = [self.usizes[-1] if self.usizes else 0] if files is None else list(files)
        if fcrcs is None:
            fcrcs, at = [], 0
            for n in self.files:
                ok = data is not None and at + n <= len(data)
                fcrcs.append(crc32(data[at:at + n]) if ok else None)
                at += n
        self.fcrcs = list(fcrcs)

    def but(self, **kw):
        f = Fo(self.rec, self.usizes, self.streams, self.data, self.crc, self.files, self.fcrcs)
        for k, v in kw.items():
            setattr(f, k, v)
        return f


def split(data, sizes):
    return dict(files=list(sizes) + [len(data) - sum(sizes)])


def copy_fo(data, **kw):
    return Fo(folder_rec([coder(M_COPY, b"")]), [len(data)], [data], data, **kw)


def lzma_fo(plain, marker=True, props=LZMA_PROPS, **kw):
    return Fo(folder_rec([cod(M_LZMA, props)]), [len(plain)], [lzma_raw(plain, marker)], plain, **kw)


def lzma2_fo(plain, props=b"\0", comp=True, **kw):
    s = X.compressed(plain) if comp else X.stored(plain)
    return Fo(folder_rec([cod(M_LZMA2, props)]), [len(plain)], [s], plain, **kw)


def filt_fo(main, filt=M_BCJ, known=True, binds=((1, 0),), packs=None, fcoder=None, usize0=None, **kw):
    """Two coders: `main` (a one-coder Fo) and a filter bound to its output.
    known=False: the filter changes the bytes (no CRCs from this side)."""
    n = main.usizes[0]
    rec = folder_rec([main.rec[1:], coder(filt, b"") if fcoder is None else fcoder], binds, packs)
    return Fo(rec, [n if usize0 is None else usize0, n], main.streams,
              main.data if known else None, **kw)


def bcj2_fo(data, methods=(M_LZMA, M_LZMA, M_LZMA), binds=((5, 0), (4, 1), (3, 2)),
            packs=(2, 6, 1, 0), last=None, **kw):
    """A BCJ2 folder in the layout CheckSupportedFolder accepts: coders 0, 1, 2 =
    the JMP, CALL and main streams, coder 3 = BCJ2 (4 in, 1 out); pack streams
    main, rc, CALL, JMP."""
    m, c, j, r = bcj2enc.encode(data)
    recs, enc = [], []
    for meth, raw in zip(methods, (j, c, m)):
        if meth == M_COPY:
            recs.append(coder(M_COPY, b""))
            enc.append(raw)
        elif meth == M_LZMA:
            recs.append(cod(M_LZMA, LZMA_PROPS))
            enc.append(lzma_raw(raw))
        elif meth == M_LZMA2:
            recs.append(cod(M_LZMA2, b"\0"))
            enc.append(X.compressed(raw) if raw else X.stored(raw))
        else:
            recs.append(coder(meth, b""))
            enc.append(raw)
    recs.append(cod(M_BCJ2, None, 4, 1) if last is None else last)
    return Fo(folder_rec(recs, binds, packs), [len(j), len(c), len(m), len(data)],
              [enc[2], r, enc[1], enc[0]], data, **kw)


# ------------------------------------------------------------------ whole archives

def stream_sections(fos, pos=0, pack_kw=None, unpack_kw=None, sub_kw=None, subs=True, order="PUS"):
    """The StreamsInfo sections of a folder list: {P, U, S} -> bytes."""
    packs = [s for f in fos for s in f.streams]
    P = pack_info([len(s) for s in packs], pos, **(pack_kw or {}))
    fcrc = digests([f.crc for f in fos]) if any(f.crc is not None for f in fos) else None
    U = unpack_info([f.rec for f in fos], [u for f in fos for u in f.usizes], fcrc, **(unpack_kw or {}))
    S = b""
    if subs:
        kw = dict(sub_kw or {})
        many = any(len(f.files) != 1 for f in fos)
        if "nums" not in kw and many:
            kw["nums"] = [len(f.files) for f in fos]
        if "sizes" not in kw and many:
            kw["sizes"] = [n for f in fos for n in f.files[:-1]]
        if "crc" not in kw:
            d = [c for f in fos if not (len(f.files) == 1 and f.crc is not None) for c in f.fcrcs]
            if any(c is not None for c in d):
                kw["crc"] = digests(d)
        S = substreams(**kw)
    parts = {"P": P, "U": U, "S": S}
    return b"".join(parts[k] for k in order)


def std(fos, layout=None, names=True, gap=b"", pos=None, fprops=(), nfiles=None, hdr_kw=None,
        sign_kw=None, after_names=(), **skw):
    """An archive around a folder list.  layout: one letter per file -- s: the
    next substream, e: an empty file, d: a directory (empty stream, not an empty
    file); default: every substream, in order.  fprops: further files-info
    properties (before the names), after_names: behind them."""
    n_s = sum(len(f.files) for f in fos)
    layout = "s" * n_s if layout is None else layout
    body = gap + b"".join(s for f in fos for s in f.streams)
    sec = stream_sections(fos, len(gap) if pos is None else pos, **skw)
    props = []
    if set(layout) - {"s"}:
        v = bools([c != "s" for c in layout])
        props.append(prop(EMPTY_STREAM, v))
        if "e" in layout:
            props.append(prop(EMPTY_FILE, bools([c == "e" for c in layout if c != "s"])))
    props += list(fprops)
    if names:
        props.append(names_prop([f"f{i}" for i in range(len(layout))] if names is True else names))
    props += list(after_names)
    fi = files_info(len(layout) if nfiles is None else nfiles, props)
    return sign(header(sec, fi, **(hdr_kw or {})), body, **(sign_kw or {}))


def packed(hdr, fo=None, body=b"", crc="right", pos=None, n_folders=1, sign_kw=None, pack=True,
           usize=None, cut=0, first=ENCODED_HEADER, tail=b"\0"):
    """An archive whose next header is kEncodedHeader: `hdr` packed by the
    folder `fo` (default Copy) behind `body`.  cut: the pack streams lie behind
    the next header instead, at the end of the file, the last `cut` bytes
    missing."""
    fo = copy_fo(hdr) if fo is None else fo
    if usize is not None:
        fo = fo.but(usizes=fo.usizes[:-1] + [usize])
    streams = b"".join(fo.streams)
    c = {"right": crc32(hdr), "wrong": crc32(hdr) ^ 1, None: None}.get(crc, crc)
    sec = b""
    if pack:
        sec += pack_info([len(s) for s in fo.streams] * n_folders, len(body) if pos is None else pos)
    sec += unpack_info([fo.rec] * n_folders, fo.usizes * n_folders,
                       None if c is None else digests([c] * n_folders))
    if cut:
        assert pos is None and n_folders == 1
        enc = N(first) + sec + tail
        for _ in range(3):   # the pack position counts the next header in front of it
            enc = N(first) + pack_info([len(s) for s in fo.streams], len(body) + len(enc)) + sec[sec.index(bytes([UNPACK_INFO, FOLDER])):] + tail
        return sign(enc, body, tail=streams[:-cut], **(sign_kw or {}))
    return sign(N(first) + sec + tail, body + streams * max(n_folders, 1), **(sign_kw or {}))


def plain_header(fos, pos=0, **kw):
    """The plain next header of std(fos) alone (the content of a packed header)."""
    arc = std(fos, pos=pos, **kw)
    off, size = struct.unpack("<QQ", arc[12:28])
    return arc[32 + off:32 + off + size]


def case(out, cls, name, data, tags=(), no_gpu=False):
    assert cls in CLASSES
    tags = set(tags)
    name = f"{cls}/{name}"
    if name in DIFFERS:
        tags.add("code_differs")
    if is_packed(data):
        tags.add("packed")
    out.append({"name": name, "cls": cls, "data": bytes(data), "tags": tags, "no_gpu": no_gpu})


def is_packed(arc):
    """True when the archive's next header starts with kEncodedHeader."""
    if len(arc) < 32:
        return False
    off, size = struct.unpack("<QQ", arc[12:28])
    return size > 0 and 32 + off < len(arc) and arc[32 + off] == ENCODED_HEADER


A, B, C3 = text(40, 1), text(23, 2), text(31, 3)


def two():
    """The plain archive most cases vary: a Copy folder of two files and an LZMA folder of one."""
    return [copy_fo(A, **split(A, [15])), lzma_fo(B)]


# ------------------------------------------------------------------ class 1: start header

def _start_cases(out):
    def c(name, data, **kw):
        case(out, "start", name, data, **kw)
    fos = two()
    base = std(fos)
    off, size = struct.unpack("<QQ", base[12:28])
    hdr, body = base[32 + off:], base[32:32 + off]
    c("plain", base)
    c("gap_before_header", sign(hdr, body + b"\xaa" * 9))
    c("tail_after_header", sign(hdr, body, tail=b"\x55" * 7))
    c("minor_0", sign(hdr, body, minor=0))
    c("minor_255", sign(hdr, body, minor=255))
    c("major_1", sign(hdr, body, major=1))
    c("signature_wrong", sign(hdr, body, sig=b"7z\xbc\xaf\x27\x1d"))
    c("start_crc_wrong", sign(hdr, body, scrc=0x12345678))
    c("header_crc_wrong", sign(hdr, body, hcrc=crc32(hdr) ^ 0x80))
    c("size_0_bytes_after", sign(hdr, body, size=0, hcrc=0))
    c("size_0_crc_set", sign(hdr, body, size=0))
    c("size_one_short", sign(hdr, body, size=len(hdr) - 1, hcrc=crc32(hdr[:-1])))
    c("size_past_end", sign(hdr, body, size=len(hdr) + 1))
    c("offset_past_end", sign(hdr, body, off=len(body) + len(hdr) + 1))
    c("offset_at_end_size_1", sign(hdr, body, off=len(body) + len(hdr), size=1))
    c("offset_plus_size_wraps", sign(hdr, body, off=(1 << 64) - 4, size=8), no_gpu=True)
    c("offset_plus_size_plus_32_wraps", sign(hdr, body, off=(1 << 64) - 40, size=10), no_gpu=True)
    c("offset_2_63", sign(hdr, body, off=1 << 63, size=len(hdr)), no_gpu=True)
    c("offset_2_62", sign(hdr, body, off=1 << 62, size=len(hdr)), no_gpu=True)
    c("size_2_62", sign(hdr, body, size=1 << 62), no_gpu=True)
    c("short_31_bytes", base[:31])
    c("start_header_only", base[:32])
    for first, name in ((END, "end"), (MAIN_STREAMS, "main_streams"), (FILES, "files"),
                        (0x18, "unknown_24"), (wide(HEADER, 1), "header_two_bytes")):
        c(f"first_id_{name}", sign(N(first) + hdr[1:], body))
    c("first_id_byte_missing", sign(b"\x80", body))


# ------------------------------------------------------------------ class 2: numbers

def _number_cases(out):
    def c(name, data, **kw):
        case(out, "numbers", name, data, **kw)
    d = text(20, 4)
    for n in (1, 2, 4, 7, 8):
        # every small value of the header in the form with n extra bytes
        fo = copy_fo(d)
        fo.rec = wide(1, n) + fo.rec[1:]
        fo.usizes = [wide(len(d), n)]
        arc = sign(header(pack_info([wide(len(d), n)], wide(0, n), wide(1, n)) +
                          unpack_info([fo.rec], fo.usizes, nf=wide(1, n)) +
                          substreams(nums=[wide(1, n)]),
                          files_info(wide(1, n), [names_prop(["n"])])), d)
        c(f"non_minimal_{n + 1}_bytes", arc)
    c("ids_non_minimal", sign(wide(HEADER, 2) + wide(MAIN_STREAMS, 1) + stream_sections([copy_fo(d)])
                              + b"\0" + wide(FILES, 3) + N(1) + names_prop(["n"]) + b"\0\0", d))
    big = 0x80000000
    one = copy_fo(d)
    c("pack_count_2_31", sign(header(pack_info([len(d)], n=wide(big, 4)) + unpack_info([one.rec], one.usizes)), d))
    # (a count of 2^31 - 1 would pass SzReadNumber32 and size a 17 GB malloc: not used)
    c("pack_count_1000_in_5_bytes", sign(header(pack_info([len(d)], n=wide(1000, 4)) +
                                               unpack_info([one.rec], one.usizes)), d))
    c("folder_count_2_31", sign(header(pack_info([len(d)]) + unpack_info([one.rec], one.usizes, nf=wide(big, 8))), d))
    c("coder_count_2_31", sign(header(pack_info([len(d)]) +
                                      unpack_info([wide(big, 4) + one.rec[1:]], one.usizes)), d))
    c("coder_count_2_63", sign(header(pack_info([len(d)]) +
                                      unpack_info([wide(1 << 63, 8) + one.rec[1:]], one.usizes)), d))
    c("in_count_2_31", sign(header(pack_info([len(d)]) + unpack_info(
        [folder_rec([cod(M_COPY, None, wide(big, 4), 1)])], one.usizes)), d))
    c("bind_index_2_31", sign(header(pack_info([len(d)]) + unpack_info(
        [folder_rec([coder(M_COPY, b""), coder(M_BCJ, b"")], [(wide(big, 4), 0)])], [20, 20])), d))
    c("pack_stream_index_2_31", sign(header(pack_info([len(d), 0]) + unpack_info(
        [folder_rec([cod(M_COPY, None, 2, 1)], (), [0, wide(big, 4)])], one.usizes)), d))
    c("num_unpack_streams_2_31", sign(header(stream_sections([one], sub_kw=dict(nums=[wide(big, 4)])),
                                             files_info(1)), d))
    c("file_count_2_31", sign(header(stream_sections([one]), files_info(wide(big, 4))), d))
    c("streams_id_2_31", sign(header(wide(big, 4) + stream_sections([one]), files_info(1)), d))
    c("streams_id_2_31_minus_1", sign(header(wide(big - 1, 4) + stream_sections([one]), files_info(1)), d))
    c("streams_id_9_byte_small", sign(header(wide(PACK_INFO, 8) + stream_sections([one])[1:], files_info(1)), d))
    c("files_id_2_31_skipped", std([one], fprops=[prop(wide(big, 4), b"\1\2\3")]))
    c("files_id_2_63_skipped", std([one], fprops=[prop(wide(1 << 63, 8), b"")]))
    c("files_id_2_31_minus_1_skipped", std([one], fprops=[prop(wide(big - 1, 4), b"\1")]))
    c("unpack_size_9_byte_form", std([one.but(usizes=[wide(len(d), 8)])]))
    c("pack_size_2_62", sign(header(pack_info([1 << 62]) + unpack_info([one.rec], one.usizes) + substreams(),
                                    files_info(1)), d), no_gpu=True)
    c("unpack_size_2_62", sign(header(pack_info([len(d)]) + unpack_info([one.rec], [1 << 62]) + substreams(),
                                      files_info(1)), d), no_gpu=True)
    c("unpack_size_2_64_minus_1", sign(header(pack_info([len(d)]) + unpack_info([one.rec], [(1 << 64) - 1]) +
                                              substreams(), files_info(1)), d), no_gpu=True)
    c("number_cut_after_first_byte", sign(header(pack_info([len(d)]) + b"\x07\x0b\xc0"), d))
    c("folder_count_beyond_bytes", sign(header(pack_info([len(d)]) + bytes([UNPACK_INFO, FOLDER]) +
                                               N(100) + b"\0\0"), d))
    c("pack_count_beyond_bytes", sign(header(bytes([PACK_INFO, 0]) + N(50) + bytes([SIZE, 1, 2, 0xC0])), d))


# ------------------------------------------------------------------ class 3: top level

def _top_cases(out):
    def c(name, data, **kw):
        case(out, "top", name, data, **kw)
    fos = two()
    body = b"".join(s for f in fos for s in f.streams)
    sec = stream_sections(fos)
    fi = files_info(3, [names_prop(["a", "b", "c"])])
    ap = bytes([ARCHIVE_PROPS])
    c("archive_properties_empty", sign(header(sec, fi, pre=ap + b"\0"), body))
    c("archive_properties_two_entries", sign(header(sec, fi, pre=ap + b"\x30\x03abc\x31\x00\0"), body))
    c("archive_properties_skip_runs_out", sign(header(None, b"", pre=ap + b"\x30\x7f\x00\x00", end=b""), body))
    c("archive_properties_skip_runs_out_then_end", sign(N(HEADER) + ap + b"\x30\x09\x00" + b"\0", body))
    c("archive_properties_unterminated", sign(N(HEADER) + ap + b"\x30\x01\x00", body))
    c("archive_properties_twice", sign(header(sec, fi, pre=ap + b"\0" + ap + b"\0"), body))
    c("end_alone", sign(N(HEADER) + b"\0"))
    c("header_alone", sign(N(HEADER)))
    c("no_main_streams_empty_files", sign(header(None, files_info(2, [
        prop(EMPTY_STREAM, bools([1, 1])), prop(EMPTY_FILE, bools([1, 0])), names_prop(["e", "d"])]))))
    c("no_main_streams_no_files", sign(header(None, files_info(0))))
    c("no_files_info", sign(header(sec), body))
    c("additional_streams_info", sign(N(HEADER) + bytes([ADDITIONAL_STREAMS]) + sec + b"\0" + fi + b"\0", body))
    c("additional_then_main", sign(header(sec, fi, pre=bytes([ADDITIONAL_STREAMS, 0])), body))
    c("unknown_id_at_top", sign(header(sec, fi, pre=b"\x19\x00"), body))
    c("unknown_id_after_streams", sign(N(HEADER) + bytes([MAIN_STREAMS]) + sec + b"\0\x19\x00" + fi + b"\0", body))
    c("main_streams_twice", sign(N(HEADER) + (bytes([MAIN_STREAMS]) + sec + b"\0") * 2 + fi + b"\0", body))
    c("files_info_twice", sign(header(sec, fi + fi[:-1]), body))
    c("bytes_after_final_end", sign(header(sec, fi) + b"\x01\x02\x03", body))
    c("final_end_missing", sign(header(sec, fi, end=b""), body))
    c("files_end_missing", sign(header(sec, fi[:-1], end=b""), body))
    # StreamsInfo sections in another order, repeated, missing
    c("streams_order_UPS", std(fos, order="UPS"))
    c("streams_order_USP", std(fos, order="USP"))
    c("streams_pack_twice", std(fos, order="PPUS"))
    c("streams_unpack_twice", std(fos, order="PUUS"))
    c("streams_substreams_twice", std(fos, order="PUSS"))
    c("streams_substreams_first_no_files", sign(header(stream_sections(fos, order="SPU")), body))
    c("streams_no_substreams_no_files", sign(header(stream_sections(fos, order="PU")), body))
    c("streams_only_pack_info", sign(header(stream_sections(fos, order="P")), body))
    c("streams_only_unpack_info_no_files", sign(header(stream_sections(fos, order="U")), body))
    c("streams_empty", sign(header(b"", files_info(0)), body))
    c("streams_unknown_section", sign(header(bytes([SIZE]) + sec, fi), body))
    c("streams_files_id_inside", sign(header(sec[:-1] + bytes([FILES]), fi), body))
    c("streams_end_missing", sign(N(HEADER) + bytes([MAIN_STREAMS]) + sec, body))
    # the reference's UB: files with streams and no SubStreamsInfo at all
    c("streams_no_substreams_with_files", std(fos, subs=False), tags=["ref_undefined"])
    c("no_main_streams_stream_file", sign(header(None, files_info(1, [names_prop(["x"])]))),
      tags=["ref_undefined"])
    c("streams_substreams_before_unpack_with_files", std(fos, order="PSU"), tags=["ref_undefined"])


# ------------------------------------------------------------------ class 4: PackInfo

def _packinfo_cases(out):
    def c(name, data, **kw):
        case(out, "packinfo", name, data, **kw)
    fos = two()
    n_body = sum(len(s) for f in fos for s in f.streams)
    pcrc = [crc32(s) for f in fos for s in f.streams]
    c("pos_gap_5", std(fos, gap=b"\xee" * 5))
    c("pos_gap_300", std(fos, gap=bytes(range(256)) + b"\xee" * 44))
    c("pos_1_without_gap", std(fos, pos=1))
    c("pos_inside_header", std(fos, pos=n_body + 4))
    c("pos_at_end_of_file", std(fos, pos=n_body + 200))
    c("pos_far_past_end", std(fos, pos=1 << 40))
    c("pos_2_62", std(fos, pos=1 << 62))
    c("pos_2_63", std(fos, pos=1 << 63), no_gpu=True)
    c("pos_2_64_minus_1", std(fos, pos=(1 << 64) - 1), no_gpu=True)
    c("pos_2_64_minus_32", std(fos, pos=(1 << 64) - 32), no_gpu=True)
    c("crc_all_defined", std(fos, pack_kw=dict(crc=digests(pcrc))))
    c("crc_all_defined_wrong_values", std(fos, pack_kw=dict(crc=digests([1, 2]))))
    c("crc_bit_vector_first", std(fos, pack_kw=dict(crc=digests([pcrc[0], None]))))
    c("crc_bit_vector_second", std(fos, pack_kw=dict(crc=digests([None, pcrc[1]]))))
    c("crc_bit_vector_none", std(fos, pack_kw=dict(crc=digests([None, None]))))
    c("crc_bit_vector_spare_bits_set", std(fos, pack_kw=dict(crc=b"\0\x7f" + u32(pcrc[1]))))
    c("crc_twice", std(fos, pack_kw=dict(crc=digests(pcrc), post=bytes([CRC]) + digests([None, 7]))))
    c("crc_cut", std(fos, pack_kw=dict(crc=b"\1" + u32(1) + b"\0\0", end=b"")))
    c("crc_vector_byte_missing", sign(header(pack_info([3], crc=b"\0", end=b"")), b"abc"))
    c("unknown_attribute_before_size", std(fos, pack_kw=dict(pre=b"\x19\x02\xaa\xbb")))
    c("two_unknown_attributes_before_size", std(fos, pack_kw=dict(pre=b"\x19\x00\x0a\x01\x55")))
    c("end_before_size", std(fos, pack_kw=dict(pre=b"\0")))
    c("unknown_attribute_after_size", std(fos, pack_kw=dict(post=b"\x19\x03abc")))
    c("unknown_attribute_skip_runs_out", std(fos, pack_kw=dict(post=b"\x19\x7f")))
    c("size_section_cut", sign(header(bytes([PACK_INFO, 0, 3, SIZE, 1]), b"", end=b""), b"abc"))
    z = [copy_fo(b""), copy_fo(A), lzma_fo(B)]
    c("zero_length_pack_stream_first", std(z))
    c("zero_length_pack_stream_middle", std([z[1], z[0], z[2]]))
    c("zero_length_pack_stream_last", std([z[1], z[2], z[0]]))
    c("zero_pack_streams_zero_folders", sign(header(pack_info([]) + unpack_info([], []), files_info(0))))
    c("more_pack_sizes_than_folders_need", sign(header(pack_info([len(A), len(fos[1].streams[0]), 9]) +
                                                       stream_sections(fos, order="US"), files_info(3)),
                                                A + fos[1].streams[0] + b"123456789"))
    c("pack_sizes_sum_past_end", sign(header(pack_info([len(A), 500]) + stream_sections(fos, order="US"),
                                             files_info(3)), A + fos[1].streams[0]))
    # the reference's UB: a folder reads PackSizes past the array
    c("fewer_pack_sizes_than_folders_need", sign(header(pack_info([len(A)]) + stream_sections(fos, order="US"),
                                                        files_info(3)), A + fos[1].streams[0]),
      tags=["ref_undefined"])
    c("no_pack_info_with_folders", sign(header(stream_sections(fos, order="US"), files_info(3)),
                                        A + fos[1].streams[0]), tags=["ref_undefined"])


# ------------------------------------------------------------------ class 5: coders and folders

X86_LONG = X86 + text(60, 9)


def coder_specs(d=C3, x=X86_LONG):
    """(name, Fo): folder shapes of class 5, each with `d` as its pack data where
    it has one pack stream, the BCJ2 ones around `x`."""
    s = []

    def one(name, rec, usizes=None, streams=None, **kw):
        s.append((name, Fo(rec, [len(d)] if usizes is None else usizes,
                           [d] if streams is None else streams, **kw)))
    cp = coder(M_COPY, b"")
    one("counts_1_1", folder_rec([cod(M_COPY, None, 1, 1)]), data=d)
    one("counts_0_1", folder_rec([cod(M_COPY, None, 0, 1)]), streams=[])
    one("counts_33_1", folder_rec([cod(M_COPY, None, 33, 1)]))
    one("counts_1_33", folder_rec([cod(M_COPY, None, 1, 33)]))
    one("counts_1_0", folder_rec([cod(M_COPY, None, 1, 0)]), usizes=[])
    one("counts_2_1_two_pack_streams", folder_rec([cod(M_COPY, None, 2, 1)], (), [0, 1]), streams=[d, b"xy"])
    one("counts_1_2_bound_to_itself", folder_rec([cod(M_COPY, None, 1, 2)], [(0, 0)]), usizes=[len(d), len(d)],
        streams=[])
    one("empty_properties_flag", folder_rec([cod(M_COPY, b"")]), data=d)
    one("copy_with_properties", folder_rec([cod(M_COPY, b"\1\2\3")]), data=d)
    one("properties_size_runs_out", folder_rec([bytes([0x21, 0x00]) + N(200)]))
    one("one_alternative", folder_rec([cod(M_COPY, None, alt=[cod(M_LZMA, LZMA_PROPS)])]), data=d)
    one("two_alternatives", folder_rec([cod(M_COPY, None, alt=[cod(M_PPMD, b"\6\0\0\0\1", 1, 1),
                                                             cod(M_LZMA2, b"\x18")])]), data=d)
    one("alternative_with_long_id", folder_rec([cod(M_COPY, None, alt=[cod(0, None, idb=b"\1" * 15)])]), data=d)
    one("alternative_count_2_31", folder_rec([cod(M_COPY, None, alt=[cod(0, None, wide(1 << 31, 4), 1)])]))
    one("alternative_cut", folder_rec([bytes([0x81, 0x00, 0x2f])]))
    one("id_size_0", folder_rec([cod(0, None, idb=b"")]), data=d)
    one("id_size_2_zero", folder_rec([cod(0, None, idb=b"\0\0")]), data=d)
    one("id_size_8_above_32_bits", folder_rec([cod(0, None, idb=b"\1\0\0\0\0\0\0\0")]))
    one("id_size_8_value_0", folder_rec([cod(0, None, idb=b"\0" * 8)]), data=d)
    for k in range(9, 16):
        one(f"id_size_{k}", folder_rec([cod(0, None, idb=b"\0" * k)]))
    one("id_size_15_cut", folder_rec([bytes([0x0f, 0, 0])]))
    one("coders_0", folder_rec([]), usizes=[], streams=[])
    one("coders_3", folder_rec([cp, coder(M_BCJ, b""), coder(M_ARM, b"")], [(1, 0), (2, 1)]),
        usizes=[len(d)] * 3)
    one("coders_5", folder_rec([cp] * 5, [(k + 1, k) for k in range(4)]), usizes=[len(d)] * 5)
    one("coders_32", folder_rec([cp] * 32, [(k + 1, k) for k in range(31)]), usizes=[len(d)] * 32)
    one("coders_33", folder_rec([cp] * 33, [(k + 1, k) for k in range(32)]), usizes=[len(d)] * 33)
    one("unknown_main_method", folder_rec([coder(0x0401, b"")]))
    one("ppmd_main_method", folder_rec([cod(M_PPMD, b"\6\0\0\x10\0")]))
    one("bcj_alone", folder_rec([coder(M_BCJ, b"")]))
    # two coders
    two = lambda f, **kw: s.append((f, filt_fo(copy_fo(d), **kw)))
    two("bcj_identity", filt=M_BCJ)
    two("arm_identity", filt=M_ARM)
    s.append(("bcj_x86_bytes", filt_fo(copy_fo(X86), M_BCJ, known=False)))
    s.append(("arm_bl_words", filt_fo(copy_fo(ARM), M_ARM, known=False)))
    s.append(("bcj_after_lzma", filt_fo(lzma_fo(d), M_BCJ)))
    s.append(("arm_after_lzma2", filt_fo(lzma2_fo(d), M_ARM)))
    two("bind_pair_reversed", binds=[(0, 1)])
    two("bind_pair_in_0_out_0", binds=[(0, 0)])
    two("bind_pair_in_1_out_1", binds=[(1, 1)])
    two("bind_pair_in_2", binds=[(2, 0)])
    s.append(("filter_first", Fo(folder_rec([coder(M_BCJ, b""), cp], [(1, 0)]), [len(d)] * 2, [d])))
    s.append(("filter_first_bound_backwards", Fo(folder_rec([coder(M_BCJ, b""), cp], [(0, 1)]), [len(d)] * 2, [d])))
    for m, name in ((M_DELTA, "delta"), (M_PPC, "ppc"), (M_ARMT, "armt"), (0x03030401, "ia64"),
                    (0x0A0B0C0D, "unknown"), (M_LZMA, "lzma_as_filter"), (M_BCJ2, "bcj2_as_filter")):
        two(f"filter_{name}", filt=m)
    two("filter_id_above_32_bits", fcoder=cod(0, None, idb=b"\1\3\3\1\3"))
    two("bcj_with_properties", fcoder=cod(M_BCJ, b"\0"))
    two("bcj_with_empty_properties", fcoder=cod(M_BCJ, b""))
    two("bcj_counts_1_1", fcoder=cod(M_BCJ, None, 1, 1))
    s.append(("bcj_counts_2_1", filt_fo(copy_fo(d), fcoder=cod(M_BCJ, None, 2, 1), packs=[0, 2]).but(
        streams=[d, b"pq"])))
    s.append(("two_coders_unbound", Fo(folder_rec([cp, cod(M_BCJ, None, 1, 0)], (), [0, 1]), [len(d)], [d, b""])))
    # four coders
    s.append(("bcj2_lzma", bcj2_fo(x)))
    s.append(("bcj2_copy", bcj2_fo(x, (M_COPY, M_COPY, M_COPY))))
    s.append(("bcj2_mixed", bcj2_fo(x, (M_LZMA2, M_COPY, M_LZMA2))))
    good = (2, 6, 1, 0)
    for k in range(4):
        p = list(good)
        p[k] = (p[k] + 1) % 7
        s.append((f"bcj2_pack_stream_{k}_wrong", bcj2_fo(x, (M_COPY,) * 3, packs=p)))
    s.append(("bcj2_pack_streams_0_1_swapped", bcj2_fo(x, (M_COPY,) * 3, packs=(6, 2, 1, 0))))
    s.append(("bcj2_pack_streams_2_3_swapped", bcj2_fo(x, (M_COPY,) * 3, packs=(2, 6, 0, 1))))
    gb = [(5, 0), (4, 1), (3, 2)]
    for k in range(3):
        b = list(gb)
        b[k] = (b[k][0] + 1 if k else 3, b[k][1])
        s.append((f"bcj2_bind_pair_{k}_in_wrong", bcj2_fo(x, (M_COPY,) * 3, binds=b)))
        b = list(gb)
        b[k] = (b[k][0], (b[k][1] + 1) % 3)
        s.append((f"bcj2_bind_pair_{k}_out_wrong", bcj2_fo(x, (M_COPY,) * 3, binds=b)))
    s.append(("bcj2_bind_pairs_0_1_swapped", bcj2_fo(x, (M_COPY,) * 3, binds=[(4, 1), (5, 0), (3, 2)])))
    for k, m in ((0, M_BCJ), (1, M_PPMD), (2, 0x0401)):
        ms = [M_COPY] * 3
        ms[k] = m
        s.append((f"bcj2_coder_{k}_not_main", bcj2_fo(x, tuple(ms))))
    f = bcj2_fo(x, (M_COPY,) * 3, last=cod(M_BCJ2, None, 3, 1), packs=(2, 1, 0))
    s.append(("bcj2_3_inputs", f.but(streams=[f.streams[0], f.streams[2], f.streams[3]])))
    f = bcj2_fo(x, (M_COPY,) * 3, last=cod(M_BCJ2, None, 4, 2), binds=gb + [(6, 3)], packs=(2, 1, 0))
    s.append(("bcj2_2_outputs", f.but(usizes=f.usizes + [0], streams=f.streams[:3])))
    s.append(("bcj2_last_is_bcj", bcj2_fo(x, (M_COPY,) * 3, last=cod(M_BCJ, None, 4, 1))))
    s.append(("bcj2_without_counts", Fo(folder_rec([cp, cp, cp, coder(M_BCJ2, b"")], [(1, 0), (2, 1), (3, 2)]),
                                        [len(d)] * 4, [d])))
    s.append(("bcj2_first_coder", Fo(folder_rec([cod(M_BCJ2, None, 4, 1), cp, cp, cp], gb, good),
                                     [len(d)] * 4, [d, b"", b"", b""])))
    return s


def _coder_cases(out):
    for name, fo in coder_specs():
        case(out, "coders", name, std([fo, lzma_fo(B)]))


# ------------------------------------------------------------------ class 6: unpack info

def unpack_specs(d=C3):
    n = len(d)
    s = []
    s.append(("coder_0_size_smaller", filt_fo(copy_fo(d), M_BCJ, usize0=n - 4)))
    s.append(("coder_0_size_larger", filt_fo(copy_fo(d), M_BCJ, usize0=n + 4)))
    s.append(("coder_0_size_zero", filt_fo(lzma_fo(d), M_BCJ, usize0=0)))
    s.append(("coder_0_size_2_62", filt_fo(lzma2_fo(d), M_ARM, usize0=1 << 62)))
    s.append(("folder_size_smaller_than_coder_0", filt_fo(copy_fo(d), M_BCJ).but(usizes=[n, n - 4], files=[n - 4])))
    s.append(("size_zero_copy", copy_fo(b"")))
    s.append(("size_zero_lzma_marker_only", lzma_fo(b"")))
    s.append(("size_zero_lzma_no_marker", lzma_fo(b"", marker=False)))
    s.append(("size_zero_lzma2", lzma2_fo(b"", comp=False)))
    s.append(("size_zero_bcj", filt_fo(copy_fo(b""), M_BCJ)))
    s.append(("size_zero_copy_with_pack_bytes", copy_fo(b"").but(streams=[b"abc"])))
    s.append(("size_zero_but_lzma_has_bytes", lzma_fo(d).but(usizes=[0], files=[0])))
    s.append(("size_one_less_lzma", lzma_fo(d).but(usizes=[n - 1], files=[n - 1])))
    s.append(("size_one_more_lzma", lzma_fo(d).but(usizes=[n + 1], files=[n + 1])))
    s.append(("size_one_less_lzma2", lzma2_fo(d).but(usizes=[n - 1], files=[n - 1])))
    s.append(("size_one_more_lzma2", lzma2_fo(d).but(usizes=[n + 1], files=[n + 1])))
    s.append(("folder_crc_right", copy_fo(d, crc=crc32(d))))
    s.append(("folder_crc_wrong", lzma_fo(d, crc=crc32(d) ^ 0x100)))
    return s


def _unpackinfo_cases(out):
    def c(name, data, **kw):
        case(out, "unpackinfo", name, data, **kw)
    for name, fo in unpack_specs():
        c(name, std([lzma2_fo(B), fo]))
    d = [text(12, 20 + k) for k in range(9)]
    nine = [copy_fo(x) for x in d]
    for k, f in enumerate(nine):
        f.crc = crc32(f.data) if k in (0, 3, 8) else None
    c("folder_crc_vector_partial_9", std(nine))
    c("folder_crc_vector_partial_wrong_slot", std([f.but(crc=(crc32(d[4]) if k == 3 else f.crc))
                                                    for k, f in enumerate(nine)]))
    c("folder_crc_vector_all_defined_byte_2", std(
        two(), unpack_kw=dict(post=bytes([CRC, 2]) + u32(crc32(A)) + u32(crc32(B))),
        sub_kw=dict(crc=digests([crc32(A[:15]), crc32(A[15:])]))))
    c("folder_crc_vector_none_defined", std(two(), unpack_kw=dict(post=bytes([CRC, 0, 0]))))
    c("folder_crc_twice", std(two(), unpack_kw=dict(post=bytes([CRC]) + digests([1, None]) +
                                                    bytes([CRC]) + digests([None, crc32(B)])),
                              sub_kw=dict(crc=digests([crc32(A[:15]), crc32(A[15:])]))))
    c("folder_crc_cut", std(two(), unpack_kw=dict(post=bytes([CRC, 1]) + u32(1) + b"\0\0", end=b"")))
    c("unknown_attribute_before_folder", std(two(), unpack_kw=dict(pre=b"\x19\x01\x77")))
    c("unknown_attribute_before_sizes", std(two(), unpack_kw=dict(mid=b"\x19\x02\x77\x88\x0a\x00")))
    c("unknown_attribute_after_sizes", std(two(), unpack_kw=dict(post=b"\x19\x01\x77")))
    c("unknown_attribute_skip_runs_out", std(two(), unpack_kw=dict(post=b"\x19\x60")))
    c("end_before_folder", std(two(), unpack_kw=dict(pre=b"\0")))
    c("end_before_sizes", std(two(), unpack_kw=dict(mid=b"\0")))
    c("external_1", std(two(), unpack_kw=dict(external=1)))
    c("external_2", std(two(), unpack_kw=dict(external=2)))
    c("external_byte_missing", sign(header(pack_info([3]) + bytes([UNPACK_INFO, FOLDER, 1]), b"", end=b""), b"abc"))
    c("sizes_cut", sign(header(pack_info([3]) + bytes([UNPACK_INFO, FOLDER, 1, 0]) + copy_fo(b"abc").rec +
                  bytes([CODERS_UNPACK_SIZE]), b"", end=b""), b"abc"))
    c("zero_folders", sign(header(pack_info([]) + unpack_info([], []) + substreams(), files_info(0))))
    c("zero_folders_with_empty_file", sign(header(pack_info([]) + unpack_info([], []) + substreams(),
                                                  files_info(1, [prop(EMPTY_STREAM, b"\x80"), names_prop(["d"])]))))
    c("one_folder_more_than_records", std(two(), unpack_kw=dict(nf=3)))
    c("one_folder_fewer_than_records", std(two(), unpack_kw=dict(nf=1)))


# ------------------------------------------------------------------ class 7: substreams

def _substream_cases(out):
    def c(name, data, **kw):
        case(out, "substreams", name, data, **kw)
    a, b, d = text(30, 30), text(24, 31), text(18, 32)
    f3 = lambda: [copy_fo(a, **split(a, [10, 5])), lzma_fo(b, **split(b, [7])), lzma2_fo(d)]
    c("three_folders_plain", std(f3()))
    for k, name in ((0, "first"), (1, "middle"), (2, "last")):
        fos = f3()
        fos[k] = fos[k].but(files=[], fcrcs=[])
        c(f"num_unpack_stream_0_{name}", std(fos))
    fos = [f.but(files=[], fcrcs=[]) for f in f3()]
    c("num_unpack_stream_0_all_no_files", std(fos, names=False))
    c("num_unpack_stream_0_all_empty_file", std(fos, layout="ed"))
    c("num_unpack_stream_twice", std(f3(), sub_kw=dict(pre=bytes([NUM_UNPACK_STREAM, 1, 1, 1]))))
    c("num_unpack_stream_cut", sign(header(stream_sections(f3(), order="PU") +
                                           bytes([SUBSTREAMS, NUM_UNPACK_STREAM, 3]), b"", end=b""), a))
    # sizes whose sum exceeds the folder: the remainder wraps
    fos = f3()
    fos[0] = fos[0].but(files=[10, 25, (30 - 35) % (1 << 64)], fcrcs=[crc32(a[:10]), None, None])
    c("sizes_exceed_folder_middle_file_fails", std(fos))
    fos = f3()
    fos[1] = fos[1].but(files=[25, (24 - 25) % (1 << 64)], fcrcs=[None, None])
    c("sizes_exceed_folder_first_file_fails", std(fos))
    fos = f3()
    fos[0] = fos[0].but(files=[(1 << 32) + 10, 5, (30 - 15 - (1 << 32)) % (1 << 64)], fcrcs=[None] * 3)
    c("size_above_32_bits_offset_truncates", std(fos))
    fos = f3()
    fos[0] = fos[0].but(files=[30, 0, 0], fcrcs=[crc32(a), 0, 0])
    c("sizes_zero_after_whole_folder", std(fos))
    fos = f3()
    fos[0] = fos[0].but(files=[0, 0, 30], fcrcs=[0, 0, crc32(a)])
    c("sizes_zero_before_whole_folder", std(fos))
    # digests
    fos = f3()
    fos[0].fcrcs[1] = None
    fos[1].fcrcs[0] = None
    c("digests_partial", std(fos))
    fos = f3()
    fos[0].fcrcs = [fos[0].fcrcs[0], None, fos[0].fcrcs[1]]
    c("digests_partial_value_in_wrong_slot", std(fos))
    fos = f3()
    fos[1].fcrcs[1] ^= 1
    c("digest_wrong_one_file", std(fos))
    c("digests_none_defined", std(f3(), sub_kw=dict(crc=b"\0\0")))
    c("digests_vector_cut", std(f3(), sub_kw=dict(crc=b"\1" + u32(5), end=b"")))
    one = lambda **kw: [copy_fo(a, **kw), lzma_fo(b, **split(b, [7]))]
    c("one_stream_folder_crc_with_crc_section", std(one(crc=crc32(a))))
    c("one_stream_folder_crc_without_crc_section", std(one(crc=crc32(a)), sub_kw=dict(crc=None)))
    c("one_stream_folder_crc_wrong_with_crc_section", std(one(crc=crc32(a) ^ 4)))
    c("one_stream_folder_crc_and_file_digest_given", std(
        one(crc=crc32(a)), sub_kw=dict(crc=digests([crc32(a), crc32(b[:7]), crc32(b[7:])]))))
    c("one_stream_no_folder_crc_file_digest", std(one()))
    c("every_folder_one_stream_with_crc_empty_crc_section", std(
        [copy_fo(a, crc=crc32(a)), lzma_fo(b, crc=crc32(b))], sub_kw=dict(crc=b"\1")))
    c("every_folder_one_stream_with_crc_no_section", std(
        [copy_fo(a, crc=crc32(a)), lzma_fo(b, crc=crc32(b))]))
    c("two_streams_folder_crc_needs_digests", std([copy_fo(a, crc=crc32(a), **split(a, [11])), lzma_fo(b)]))
    c("unknown_attribute_first", std(f3(), sub_kw=dict(pre=b"\x19\x02ab")))
    c("unknown_attribute_before_size", std(f3(), sub_kw=dict(mid=b"\x19\x01a")))
    c("unknown_attribute_after_size", std(f3(), sub_kw=dict(crc=None, post=b"\x19\x01a")))
    c("unknown_attribute_after_crc", std(f3(), sub_kw=dict(post=b"\x19\x03abc")))
    c("unknown_attribute_after_crc_skip_runs_out", std(f3(), sub_kw=dict(post=b"\x19\x70")))
    c("size_section_after_crc", std(f3(), sub_kw=dict(post=bytes([SIZE, 0]))))
    # the reference sets one size per folder and leaves the others unset (7zIn.c:784-792)
    c("no_size_section_two_streams", std(f3(), sub_kw=dict(sizes=None, crc=None)), tags=["ref_unset"],
      no_gpu=True)
    c("no_size_section_two_streams_with_crc", std(f3(), sub_kw=dict(sizes=None)), tags=["ref_unset"],
      no_gpu=True)
    c("no_num_unpack_stream_size_section_present", std(f3(), sub_kw=dict(nums=None, sizes=[], crc=None),
                                                       layout="sss"))
    c("size_section_cut", std(f3(), sub_kw=dict(sizes=[10], crc=None, end=b""), hdr_kw=dict(end=b""),
                              names=False, nfiles=0))
    c("end_missing", sign(header(stream_sections(f3())[:-1], b"", end=b""), a))
    c("fewer_stream_files_than_substreams", std(f3(), layout="sss"))
    c("no_stream_files_at_all", std(f3(), layout="dd"))
    # the reference's UB
    c("more_stream_files_than_substreams", std(f3(), layout="sssssss"), tags=["ref_undefined"])
    c("crc_section_twice", std(f3(), sub_kw=dict(post=bytes([CRC]) + b"\0\0")), tags=["ref_undefined"])


# ------------------------------------------------------------------ class 8: files

def _file_cases(out):
    def c(name, data, **kw):
        case(out, "files", name, data, **kw)
    a, b = text(36, 40), text(20, 41)
    fos = lambda: [copy_fo(a, **split(a, [9, 9, 9])), lzma_fo(b, **split(b, [8]))]
    c("empty_at_start_of_folder", std(fos(), layout="essssss"))
    c("empty_in_middle_of_folder", std(fos(), layout="ssesdss" + "s"))
    c("empty_at_end_of_folder", std(fos(), layout="ssssess"))
    c("empty_between_folders_and_at_end", std(fos(), layout="ssssdssed"))
    c("dir_in_middle_of_second_folder", std(fos(), layout="sssssds"))
    c("nine_files_last_vector_byte_partly_used", std(fos(), layout="sesdsesds"))
    c("empty_stream_spare_bits_set", std(fos(), fprops=[prop(EMPTY_STREAM, b"\x03")], layout="ssssss"))
    c("empty_file_spare_bits_set", std(fos(), fprops=[prop(EMPTY_STREAM, b"\xc0"), prop(EMPTY_FILE, b"\x7f")],
                                        layout="ssssssss", names=False))
    c("empty_stream_without_empty_file", std(fos(), fprops=[prop(EMPTY_STREAM, b"\x81")], layout="s" * 8))
    c("empty_file_before_empty_stream", std(fos(), fprops=[prop(EMPTY_FILE, b""), prop(EMPTY_STREAM, b"\x81")],
                                            layout="s" * 8))
    c("empty_stream_vector_short", std(fos(), fprops=[prop(EMPTY_STREAM, b"")], layout="s" * 6))
    c("empty_stream_size_field_too_long", std(fos(), fprops=[prop(EMPTY_STREAM, b"\x80", size=2)], layout="s" * 7))
    c("empty_file_vector_runs_out", std(fos(), fprops=[prop(EMPTY_STREAM, b"\xff\xc0"), prop(EMPTY_FILE, b"\x80", size=1)],
                                        layout="s" * 16, names=False, after_names=[]))
    for t, name in ((ANTI, "anti"), (DUMMY, "dummy"), (CTIME, "ctime"), (ATIME, "atime"),
                    (START_POS, "start_pos"), (COMMENT, "comment"), (0x30, "unknown_48")):
        c(f"skipped_{name}", std(fos(), fprops=[prop(t, b"\x01\x00" + bytes(range(16)))]))
    c("skipped_dummy_size_0", std(fos(), fprops=[prop(DUMMY, b""), prop(DUMMY, b"")]))
    c("skipped_property_size_past_end", std(fos(), fprops=[prop(ANTI, b"\x80", size=0x3000)]))
    c("property_size_missing", sign(header(stream_sections(fos()), files_info(6, [N(ANTI)], end=b""), end=b""), a))
    attr = lambda defined: (digests([0x20 if x else None for x in defined])[:1 + (0 if all(defined) else 1)]
                            + b"\0" + b"".join(u32(0x20 + k) for k, x in enumerate(defined) if x))
    mtime = lambda defined: ((b"\1" if all(defined) else b"\0" + bools(defined)) + b"\0" +
                             b"".join(struct.pack("<Q", 0x01D0000000000000 + k) for k, x in enumerate(defined) if x))
    c("attributes_all_defined", std(fos(), fprops=[prop(WIN_ATTRIB, attr([1] * 6))]))
    c("attributes_partly_defined", std(fos(), fprops=[prop(WIN_ATTRIB, attr([1, 0, 0, 1, 0, 1]))]))
    c("attributes_none_defined", std(fos(), fprops=[prop(WIN_ATTRIB, attr([0] * 6))]))
    c("attributes_external_1", std(fos(), fprops=[prop(WIN_ATTRIB, b"\1\1" + u32(0x20) * 6)]))
    c("attributes_cut", sign(header(stream_sections(fos()), files_info(6, [N(WIN_ATTRIB) + N(22) + b"\1\0" + u32(0x20) * 5], end=b""),
                  end=b""), a + fos()[1].streams[0]))
    c("attributes_size_field_too_small", std(fos(), fprops=[prop(WIN_ATTRIB, attr([1] * 6), size=3)]))
    c("attributes_size_field_too_large", std(fos(), fprops=[prop(WIN_ATTRIB, attr([1] * 6), size=40)]))
    c("mtime_all_defined", std(fos(), fprops=[prop(MTIME, mtime([1] * 6))]))
    c("mtime_partly_defined", std(fos(), fprops=[prop(MTIME, mtime([0, 1, 1, 0, 0, 0]))]))
    c("mtime_external_1", std(fos(), fprops=[prop(MTIME, b"\1\1")]))
    c("mtime_size_field_disagrees", std(fos(), fprops=[prop(MTIME, mtime([1] * 6), size=9)]))
    c("attributes_and_mtime_behind_names", std(fos(), after_names=[prop(WIN_ATTRIB, attr([1, 0] * 3)),
                                                                   prop(MTIME, mtime([0, 1] * 3))]))
    six = [f"n{k}" for k in range(6)]
    raw = utf16(six)
    c("names_odd_byte_count", std(fos(), names=False, fprops=[names_prop(None, raw=raw + b"\0")]))
    c("names_no_final_terminator", std(fos(), names=False, fprops=[names_prop(None, raw=raw[:-2])]))
    c("names_one_too_few", std(fos(), names=False, fprops=[names_prop(six[:5])]))
    c("names_one_too_many", std(fos(), names=False, fprops=[names_prop(six + ["x"])]))
    c("names_all_empty", std(fos(), names=[""] * 6))
    c("names_lone_surrogates", std(fos(), names=False, fprops=[names_prop(
        None, raw=b"".join(struct.pack("<HH", 0xD800 + k, 0) for k in range(3)) +
        b"".join(struct.pack("<HHH", 0xDC00 + k, 0x41, 0) for k in range(3)))]))
    c("names_long", std(fos(), names=["x" * 90, "y" * 60] + six[2:]))
    c("names_external_1", std(fos(), names=False, fprops=[names_prop(six, external=1)]))
    c("names_size_0", std(fos(), names=False, fprops=[prop(NAME, b"")]))
    c("names_size_past_end", std(fos(), names=False, fprops=[names_prop(six, size=len(raw) + 40)]))
    c("names_size_field_short", std(fos(), names=False, fprops=[names_prop(six, size=len(raw) - 1)]))
    c("names_twice", std(fos(), fprops=[names_prop([f"m{k}" for k in range(6)])]))
    c("names_twice_second_bad", std(fos(), after_names=[names_prop(six[:4])]))
    c("names_missing", std(fos(), names=False))
    c("zero_files_with_folders", std(fos(), layout="", names=False))
    c("only_empty_files_with_folders", std(fos(), layout="ede"))
    c("fewer_stream_files_than_substreams", std(fos(), layout="ssds"))
    c("file_count_beyond_vector", std(fos(), nfiles=40, names=False, layout="ssssssd"))
    c("file_count_5000_beyond_bytes", std(fos(), nfiles=5000, names=False, layout="ssssssd"))
    c("more_stream_files_than_substreams", std(fos(), layout="s" * 7), tags=["ref_undefined"])


# ------------------------------------------------------------------ class 9: packed headers

def _packed_cases(out):
    def c(name, data, **kw):
        case(out, "packed", name, data, **kw)
    fos = two()
    body = b"".join(s for f in fos for s in f.streams)
    hdr = plain_header(fos)
    assert 0xE8 not in hdr and 0xE9 not in hdr   # the x86 filter leaves it alone
    c("copy", packed(hdr, None, body))
    c("copy_no_crc", packed(hdr, None, body, crc=None))
    c("copy_crc_wrong", packed(hdr, None, body, crc="wrong"))
    c("lzma", packed(hdr, lzma_fo(hdr), body))
    c("lzma_no_marker", packed(hdr, lzma_fo(hdr, marker=False), body))
    c("lzma_crc_wrong", packed(hdr, lzma_fo(hdr), body, crc="wrong"))
    c("lzma2", packed(hdr, lzma2_fo(hdr), body))
    c("lzma2_stored", packed(hdr, lzma2_fo(hdr, comp=False), body))
    c("lzma2_crc_wrong", packed(hdr, lzma2_fo(hdr), body, crc="wrong"))
    c("bcj_lzma", packed(hdr, filt_fo(lzma_fo(hdr), M_BCJ), body))
    c("arm_copy", packed(hdr, filt_fo(copy_fo(hdr), M_ARM), body))
    c("bcj2_copy", packed(hdr, bcj2_fo(hdr, (M_COPY,) * 3), body))
    c("bcj2_lzma", packed(hdr, bcj2_fo(hdr), body))
    c("bcj2_crc_wrong", packed(hdr, bcj2_fo(hdr, (M_COPY,) * 3), body, crc="wrong"))
    c("gap_before_pack_stream", packed(hdr, None, body + b"\xcc" * 6))
    c("pack_stream_before_data", _header_first(fos))
    c("two_folders", packed(hdr, None, body, n_folders=2))
    c("zero_folders", packed(hdr, None, body, n_folders=0))
    c("with_substreams_info", packed(hdr, None, body, tail=substreams() + b"\0"))
    inner = packed(hdr, None, body)
    off, size = struct.unpack("<QQ", inner[12:28])
    c("nested_packed_header", packed(inner[32 + off:32 + off + size], None, inner[32:32 + off]))
    c("unpack_size_one_short_copy", packed(hdr, None, body, usize=len(hdr) - 1))
    c("unpack_size_one_long_copy", packed(hdr, None, body, usize=len(hdr) + 1))
    c("unpack_size_one_short_lzma", packed(hdr, lzma_fo(hdr), body, usize=len(hdr) - 1))
    c("unpack_size_one_long_lzma", packed(hdr, lzma_fo(hdr), body, usize=len(hdr) + 1))
    c("unpack_size_one_short_lzma2", packed(hdr, lzma2_fo(hdr), body, usize=len(hdr) - 1, crc=None))
    c("unpack_size_one_long_lzma2", packed(hdr, lzma2_fo(hdr), body, usize=len(hdr) + 1, crc=None))
    c("unpack_size_zero", packed(b"", copy_fo(b""), body, crc=None))
    c("unsupported_coder_ppmd", packed(hdr, Fo(folder_rec([cod(M_PPMD, b"\6\0\0\x10\0")]), [len(hdr)], [hdr]), body))
    c("unsupported_filter_delta", packed(hdr, filt_fo(copy_fo(hdr), M_DELTA), body))
    c("unsupported_three_coders", packed(hdr, Fo(folder_rec(
        [coder(M_COPY, b""), coder(M_BCJ, b""), coder(M_ARM, b"")], [(1, 0), (2, 1)]), [len(hdr)] * 3, [hdr]), body))
    c("lzma_props_4_bytes", packed(hdr, lzma_fo(hdr, props=LZMA_PROPS[:4]), body))
    c("content_starts_with_end", packed(b"\0" + hdr[1:], None, body))
    c("content_starts_with_files_info", packed(bytes([FILES]) + hdr[1:], None, body))
    c("content_empty_header", packed(bytes([HEADER, END]), None, body))
    c("pack_stream_cut_copy", packed(hdr, None, body, cut=3))
    c("pack_stream_cut_lzma", packed(hdr, lzma_fo(hdr), body, cut=3))
    c("pack_stream_cut_lzma2", packed(hdr, lzma2_fo(hdr), body, cut=1))
    c("pack_position_past_end", packed(hdr, None, body, pos=5000))
    c("pack_position_2_62", packed(hdr, None, body, pos=1 << 62))
    c("streams_info_unknown_id", packed(hdr, None, body, tail=b"\x19\0"))
    c("streams_info_end_missing", packed(hdr, None, body, tail=b""))
    c("header_crc_over_packed_header_wrong", packed(hdr, None, body, sign_kw=dict(hcrc=0x1234)))
    c("lzma_data_corrupt", _flip_last_pack_byte(packed(hdr, lzma_fo(hdr), body), len(body) + 9))
    # the reference's UB: the packed header's folder reads PackSizes through a null pointer
    c("no_pack_info", packed(hdr, None, body, pack=False), tags=["ref_undefined"])


def _header_first(fos):
    """The Copy-packed header in front of the data it describes."""
    hdr = plain_header(fos)
    for _ in range(3):
        hdr = plain_header(fos, pos=len(hdr))
    fo = copy_fo(hdr)
    body = hdr + b"".join(s for f in fos for s in f.streams)
    sec = pack_info([len(hdr)], 0) + unpack_info([fo.rec], fo.usizes, digests([crc32(hdr)]))
    return sign(bytes([ENCODED_HEADER]) + sec + b"\0", body)


def _flip_last_pack_byte(arc, at):
    b = bytearray(arc)
    b[32 + at] ^= 0x55
    # the start header's CRCs cover only the next header: nothing to re-sign
    return bytes(b)


# ------------------------------------------------------------------ class 10: coder checks at extract

def extract_specs(d=C3, x=X86_LONG):
    n = len(d)
    s = []
    s.append(("copy_pack_shorter_than_unpack", copy_fo(d).but(streams=[d[:-1]])))
    s.append(("copy_pack_longer_than_unpack", copy_fo(d).but(streams=[d + b"!"])))
    s.append(("lzma_props_4_bytes", lzma_fo(d, props=LZMA_PROPS[:4])))
    s.append(("lzma_props_6_bytes", lzma_fo(d, props=LZMA_PROPS + b"\x77")))
    s.append(("lzma_props_0_bytes", lzma_fo(d, props=b"")))
    s.append(("lzma_prop_byte_224", Fo(folder_rec([cod(M_LZMA, bytes([224]) + LZMA_PROPS[1:])]), [n],
                                       [lzma_raw(d, True, 8, 4, 4)], d)))
    s.append(("lzma_prop_byte_225", lzma_fo(d, props=bytes([225]) + LZMA_PROPS[1:])))
    s.append(("lzma_dict_size_0", lzma_fo(d, props=LZMA_PROPS[:1] + u32(0))))
    s.append(("lzma2_props_size_0", lzma2_fo(d, props=b"")))
    s.append(("lzma2_props_size_2", lzma2_fo(d, props=b"\0\0")))
    s.append(("lzma2_prop_byte_40", lzma2_fo(d, props=b"\x28")))
    s.append(("lzma2_prop_byte_41", lzma2_fo(d, props=b"\x29")))
    full = lzma_raw(d, True)
    bare = lzma_raw(d, False)
    s.append(("lzma_ends_early", lzma_fo(d).but(streams=[full[:-6]])))
    s.append(("lzma_no_marker_exactly_at_size", lzma_fo(d, marker=False)))
    s.append(("lzma_marker_at_size", lzma_fo(d)))
    s.append(("lzma_one_byte_left_over", lzma_fo(d).but(streams=[full + b"\0"])))
    s.append(("lzma_no_marker_one_byte_left_over", lzma_fo(d).but(streams=[bare + b"\0"])))
    s.append(("lzma_first_byte_not_zero", lzma_fo(d).but(streams=[b"\1" + full[1:]])))
    s.append(("lzma_pack_size_zero", lzma_fo(d).but(streams=[b""])))
    l2 = X.compressed(d)
    s.append(("lzma2_without_end_byte", lzma2_fo(d).but(streams=[l2[:-1]])))
    s.append(("lzma2_one_byte_left_over", lzma2_fo(d).but(streams=[l2 + b"\0"])))
    s.append(("lzma2_stored_without_end_byte", lzma2_fo(d, comp=False).but(streams=[X.stored(d)[:-1]])))
    s.append(("lzma2_bad_control_byte", lzma2_fo(d).but(streams=[b"\x03" + l2[1:]])))
    s.append(("lzma2_three_chunks", Fo(folder_rec([cod(M_LZMA2, b"\0")]), [n], [X.compressed3(d)], d)))
    s.append(("folder_crc_wrong_file_crcs_right", lzma_fo(d, crc=crc32(d) ^ 1, **split(d, [n // 3]))))
    s.append(("folder_crc_right_file_crc_wrong", lzma2_fo(d, crc=crc32(d), **split(d, [n // 3])).but(
        fcrcs=[crc32(d[:n // 3]), crc32(d[n // 3:]) ^ 1])))
    s.append(("no_folder_crc_first_file_crc_wrong", copy_fo(d, **split(d, [n // 3])).but(
        fcrcs=[crc32(d[:n // 3]) ^ 1, crc32(d[n // 3:])])))
    # BCJ2 folders: failures planted in coder order
    good = bcj2_fo(x, (M_LZMA, M_LZMA2, M_LZMA))
    main, rc, call, jump = good.streams

    def b2(name, props0=None, call_s=call, usize2=None, main_s=main, rc_cut=0, jump_s=jump, **kw):
        f = bcj2_fo(x, (M_LZMA, M_LZMA2, M_LZMA), **kw)
        if props0 is not None:   # coder 0 (JMP): LZMA props the decoder refuses
            recs = [cod(M_LZMA, props0), cod(M_LZMA2, b"\0"), cod(M_LZMA, LZMA_PROPS), cod(M_BCJ2, None, 4, 1)]
            f.rec = folder_rec(recs, [(5, 0), (4, 1), (3, 2)], (2, 6, 1, 0))
        f.streams = [main_s, rc[:len(rc) - rc_cut], call_s, jump_s]
        if usize2 is not None:
            f.usizes[2] = usize2
        s.append((name, f))
    bad_props = bytes([225]) + LZMA_PROPS[1:]
    b2("bcj2_sound")
    b2("bcj2_fails_in_coders_0_1_2_and_rc", bad_props, call[:-1], len(x) + 1, main[:-3], 2)
    b2("bcj2_fails_in_coders_1_2_and_rc", None, call[:-1], len(x) + 1, main[:-3], 2)
    b2("bcj2_fails_in_coder_2_size_and_rc", None, call, len(x) + 1, main, 2)
    b2("bcj2_fails_in_coder_2_data_and_rc", None, call, None, main[:-3], 2)
    b2("bcj2_rc_first_byte_ignored", None, call, None, main, 0)
    s[-1][1].streams[1] = b"\x01" + rc[1:]
    b2("bcj2_rc_stream_corrupt", None, call, None, main, 0)
    s[-1][1].streams[1] = rc[:1] + bytes([rc[1] ^ 0xC0]) + rc[2:]
    b2("bcj2_jump_stream_one_byte_left_over", None, call, None, main, 0, jump + b"\0")
    b2("bcj2_call_stream_empty", None, b"", None, main, 0)
    b2("bcj2_folder_crc_wrong", crc=crc32(x) ^ 2)
    return s


def _extract_cases(out):
    def c(name, data, **kw):
        case(out, "extract", name, data, **kw)
    for name, fo in extract_specs():
        c(name, std([copy_fo(A), fo, lzma2_fo(B)]))
    c("lzma2_pack_stream_cut_by_end_of_file", _cut_data([copy_fo(A), lzma2_fo(C3)], 1))
    f = bcj2_fo(X86_LONG, (M_COPY,) * 3)
    c("bcj2_rc_stream_cut_by_end_of_file", _cut_data([copy_fo(A), f.but(
        streams=[f.streams[0], f.streams[2], f.streams[3], f.streams[1]], rec=folder_rec(
            [coder(M_COPY, b"")] * 3 + [cod(M_BCJ2, None, 4, 1)], [(5, 0), (4, 1), (3, 2)], (2, 6, 1, 0)))], 2))
    c("lzma_pack_stream_cut_by_end_of_file", _cut_data([copy_fo(A), lzma_fo(C3)], 4))
    c("copy_pack_stream_cut_by_end_of_file", _cut_data([lzma_fo(C3), copy_fo(A)], 4))
    for name, arc in matrix_archives():
        c(name, arc)


def _cut_data(fos, k):
    """std(fos) with the pack data behind the next header, at the end of the
    file, and its last k bytes missing: the last pack stream is cut by the end
    of the file."""
    hdr = plain_header(fos)
    for _ in range(3):
        hdr = plain_header(fos, pos=len(hdr))
    data = b"".join(s for f in fos for s in f.streams)
    return sign(hdr, b"", tail=data[:len(data) - k])


MATRIX_PAIRS = 24
# the failing folders, classes 10, 5 and 6 mixed (names of extract_specs,
# coder_specs and unpack_specs), and the sound ones between them
MATRIX_FAILING = (
    "copy_pack_shorter_than_unpack", "counts_2_1_two_pack_streams", "lzma_props_4_bytes",
    "id_size_8_above_32_bits", "folder_size_smaller_than_coder_0", "lzma_prop_byte_225", "coders_3",
    "lzma2_props_size_2", "bind_pair_reversed", "size_zero_but_lzma_has_bytes",
    "lzma2_prop_byte_41", "filter_first", "lzma_ends_early", "filter_delta", "size_one_less_lzma",
    "lzma_one_byte_left_over", "lzma2_without_end_byte", "bcj2_pack_stream_1_wrong",
    "folder_crc_wrong", "folder_crc_wrong_file_crcs_right", "folder_crc_right_file_crc_wrong",
    "bcj2_fails_in_coders_0_1_2_and_rc", "bcj2_fails_in_coder_2_size_and_rc",
    "bcj2_call_stream_empty")
MATRIX_SOUND = (
    "counts_1_1", "empty_properties_flag", "copy_with_properties", "one_alternative",
    "two_alternatives", "id_size_0", "id_size_8_value_0", "bcj_identity", "arm_identity",
    "bcj_x86_bytes", "arm_bl_words", "bcj_after_lzma", "arm_after_lzma2", "bcj2_lzma", "bcj2_copy",
    "bcj2_mixed", "size_zero_copy", "size_zero_lzma_marker_only", "size_zero_lzma2",
    "folder_crc_right", "lzma_props_6_bytes", "lzma_prop_byte_224", "lzma2_prop_byte_40",
    "lzma_no_marker_exactly_at_size", "lzma_marker_at_size", "lzma2_three_chunks", "bcj2_sound",
    "coder_0_size_smaller", "coder_0_size_larger")
assert len(MATRIX_FAILING) == MATRIX_PAIRS


def matrix_folders():
    """2 * MATRIX_PAIRS small folders from classes 5, 6 and 10, failing and sound
    ones in turn (as many as fit into 2 KiB with the header packed by Copy)."""
    d, x = text(6, 50), X86[:21]
    specs = dict(coder_specs(d, x) + unpack_specs(d) + extract_specs(d, x))
    failing = [specs[n] for pair in zip(MATRIX_FAILING[0::2], MATRIX_FAILING[1::2]) for n in pair]
    sound = [specs[n] for n in MATRIX_SOUND]
    out = []
    for k in range(MATRIX_PAIRS):
        out.append(failing[k])
        # file CRCs on every third sound folder only: the header stays small
        f = sound[(k * 7) % len(sound)]
        out.append(f if k % 3 == 0 else f.but(fcrcs=[None] * len(f.fcrcs)))
    return out


def matrix_archives():
    fos = matrix_folders()
    plain = std(fos, names=False)
    off, size = struct.unpack("<QQ", plain[12:28])
    hdr, body = plain[32 + off:32 + off + size], plain[32:32 + off]
    return [("matrix_plain_header", plain),
            ("matrix_lzma2_packed_header", packed(hdr, lzma2_fo(hdr), body)),
            ("matrix_copy_packed_header", packed(hdr, None, body))]


# ------------------------------------------------------------------ the case table

def cases():
    out = []
    for f in (_start_cases, _number_cases, _top_cases, _packinfo_cases, _coder_cases,
              _unpackinfo_cases, _substream_cases, _file_cases, _packed_cases, _extract_cases):
        f(out)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    for c in out:
        assert len(c["data"]) <= MAX_ARCHIVE, (c["name"], len(c["data"]))
    return out


_cases = None


def all_cases():
    global _cases
    if _cases is None:
        _cases = cases()
    return _cases


# ------------------------------------------------------------------ the reference

MAX_FILES, MAX_FOLDERS, OUT_CAP, NAMES_CAP = 512, 256, 1 << 16, 1 << 14
_sp = ctypes.POINTER(ctypes.c_size_t)
_up = ctypes.POINTER(ctypes.c_uint)


def have_ref():
    return os.path.exists(native.REF_CONT_SO) and hasattr(native.ref_cont(), "ref_7z_info")


def _lib():
    lib = native.ref_cont()
    if not getattr(lib, "_szh_declared", False):
        lib.ref_7z_extract.restype = ctypes.c_int
        lib.ref_7z_extract.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                       ctypes.c_size_t, _sp, native.int_p, ctypes.c_void_p, _up,
                                       ctypes.c_uint, ctypes.c_char_p, ctypes.c_size_t, _sp]
        lib.ref_7z_info.restype = ctypes.c_int
        lib.ref_7z_info.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                    _up, ctypes.c_void_p, ctypes.c_size_t, _up]
        lib.ref_shim_max_alloc.restype = ctypes.c_ulonglong
        lib.ref_shim_max_alloc.argtypes = [ctypes.c_int]
        lib._szh_declared = True
    return lib


def answers(open_res, folders, files, names, out, max_alloc, unset=False):
    """The recorded form: folders [[NumCoders, unpack size, UnpackCRCDefined,
    UnpackCRC, NumUnpackStreams]], files [[HasStream, IsDir, CrcDefined, Crc,
    folder index, size, extract result]], and hashes of the name buffer and of
    the bytes of the files that extract, in file order; max_alloc is the largest
    allocation the reference asked its allocator for in both calls.  unset (the tag
    ref_unset): the reference leaves file sizes unset, so sizes, extract
    results and bytes are not recorded."""
    if unset:
        files, out = [f[:5] + [None, None] for f in files], b""
    return {"open": open_res, "folders": folders, "files": files, "max_alloc": max_alloc,
            "names_len": len(names), "names_sha256": hashlib.sha256(names).hexdigest(),
            "out_len": len(out), "out_sha256": hashlib.sha256(out).hexdigest()}


def ref_answers(data, unset=False):
    lib = _lib()
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    out = ctypes.create_string_buffer(OUT_CAP)
    names = ctypes.create_string_buffer(NAMES_CAP)
    ol, nl = ctypes.c_size_t(0), ctypes.c_size_t(0)
    nf, nfo, nf2 = ctypes.c_uint(0), ctypes.c_uint(0), ctypes.c_uint(0)
    fres = (ctypes.c_int * MAX_FILES)()
    fsize = (ctypes.c_ulonglong * MAX_FILES)()
    lib.ref_shim_max_alloc(1)
    r = lib.ref_7z_extract(buf, len(data), out, OUT_CAP, ctypes.byref(ol), fres, fsize,
                           ctypes.byref(nf), MAX_FILES, names, NAMES_CAP, ctypes.byref(nl))
    fo = (ctypes.c_ulonglong * (5 * MAX_FOLDERS))()
    fi = (ctypes.c_uint * (5 * MAX_FILES))()
    r2 = lib.ref_7z_info(buf, len(data), fo, MAX_FOLDERS, ctypes.byref(nfo), fi, MAX_FILES,
                         ctypes.byref(nf2))
    assert r == r2 and nf.value == nf2.value <= MAX_FILES and nfo.value <= MAX_FOLDERS
    folders = [list(fo[5 * i:5 * i + 5]) for i in range(nfo.value)]
    files = [list(fi[5 * i:5 * i + 5]) + [fsize[i], fres[i]] for i in range(nf.value)]
    return answers(r, folders, files, names.raw[:nl.value], out.raw[:ol.value],
                   lib.ref_shim_max_alloc(0), unset)


def record(c):
    rec = {"sha256": hashlib.sha256(c["data"]).hexdigest(), "tags": sorted(c["tags"])}
    if "ref_undefined" not in c["tags"]:
        rec.update(ref_answers(c["data"], "ref_unset" in c["tags"]))
    return rec


_golden = None


def expect(c):
    """The reference's answers for a case: live where oracle/_ref is built, else
    the golden file's (whose SHA-256 of the input must match the generated
    archive).  A ref_undefined case has no answers."""
    global _golden
    if have_ref():
        return record(c)
    if _golden is None:
        with open(GOLDEN) as f:
            _golden = json.load(f)["cases"]
    g = _golden[c["name"]]
    assert g["sha256"] == hashlib.sha256(c["data"]).hexdigest(), c["name"]
    return g


def run_sanitized(c):
    """The case through oracle/_ref/ref_7z_check (the reference under the host
    sanitizers, a program of its own): (exit status, its answers or None,
    the sanitizer's report)."""
    with tempfile.NamedTemporaryFile(suffix=".7z") as f:
        f.write(c["data"])
        f.flush()
        p = subprocess.run([CHECK_EXE, f.name], capture_output=True, timeout=60)
    if p.returncode != 0:
        return p.returncode, None, p.stderr.decode(errors="replace")
    j = json.loads(p.stdout)
    return 0, answers(j["open"], j["folders"], j["files"], bytes.fromhex(j["names"]),
                      bytes.fromhex(j["out"]), j["max_alloc"], "ref_unset" in c["tags"]), ""


def accepted(e):
    return e.get("open") == OK


def refused(c, e):
    """A case the project has to refuse at open."""
    return "ref_undefined" in c["tags"] or not accepted(e) or c["name"] in STRICTER


def failing(c, e):
    """A case with anything to refuse: the open, or a file at extract."""
    return refused(c, e) or any(f[6] not in (OK, None) for f in e["files"])


def check_table(cs, ans):
    """The conditions on the case table, given the reference's answers by case
    name (no project code involved): at least 200 cases in the ten classes,
    ref_undefined on at most one case in eight, code_differs only on cases the
    reference refuses something of (the open, or a file at extract) and on at
    most one in five of the cases refused at open -- the smaller of the two
    denominators; every STRICTER entry a case the reference accepts; no answer
    that hangs on a huge allocation: every folder size below 1 MiB or at least
    2^62, and the largest request the reference made of its allocator (counts
    times element sizes, property and name buffers, folder outputs, BCJ2
    temporaries, probability tables) below MAX_REF_ALLOC or at least 2^62;
    every folder's output within MAX_FOLDER_OUT where it decodes.  Returns the
    counts."""
    per, n_refused, n_tagged, n_undef, n_open = {}, 0, 0, 0, 0
    for c in cs:
        e = ans[c["name"]]
        k = per.setdefault(c["cls"], [0, 0, 0])
        k[0] += 1
        assert c["tags"] <= {"ref_undefined", "ref_unset", "code_differs", "packed"}, c["name"]
        if "ref_undefined" in c["tags"]:
            n_undef += 1
            assert "open" not in e and "code_differs" not in c["tags"], c["name"]
        n_open += refused(c, e)
        if failing(c, e):
            k[1] += 1
            n_refused += 1
            if "code_differs" in c["tags"]:
                k[2] += 1
                n_tagged += 1
                assert c["name"] in DIFFERS, c["name"]
        else:
            assert "code_differs" not in c["tags"], c["name"]
        for f in e.get("folders", []):
            assert f[1] < 1 << 20 or f[1] >= 1 << 62, (c["name"], f)
        if "max_alloc" in e:
            assert e["max_alloc"] < MAX_REF_ALLOC or e["max_alloc"] >= 1 << 62, (c["name"], e["max_alloc"])
        for f in e.get("files", []):
            if f[6] == OK and f[4] != NO_FOLDER:
                assert e["folders"][f[4]][1] <= MAX_FOLDER_OUT, c["name"]
    for name in STRICTER:
        assert accepted(ans[name]), name
    for name in DIFFERS:
        assert name in ans, name
    assert len(cs) >= 200 and set(per) == set(CLASSES), (len(cs), sorted(per))
    assert 8 * n_undef <= len(cs), (n_undef, len(cs))
    assert 5 * n_tagged <= n_open <= n_refused, (n_tagged, n_open, n_refused)
    return {"classes": per, "refused": n_open, "failing": n_refused, "tagged": n_tagged, "undefined": n_undef}

"""Shared by tests/test_7zenc_host.py and tests/test_7zenc_gpu.py: archive
descriptions for the 7z writer, the layout helper's view of them
(tests/sevenzwrite.py) and the reference's own reader (ref_7z_extract in
oracle/_ref/libref.so)."""
import ctypes
import os
import random
import struct
import sys
import zlib

import native
import sevenzwrite as W

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))

OK, UNSUPPORTED, PARAM, OUTPUT_EOF, FAIL = 0, 4, 5, 7, 11
M_PPMD = 0x030401
_sp = ctypes.POINTER(ctypes.c_size_t)


def have_ref_reader():
    return native.have_ref() and os.path.exists(native.REF_CONT_SO)


def ref_extract(arc, max_files=4096):
    """The reference's SzArEx_Open + SzArEx_Extract of every file: (open res,
    [file res], [file size], the extracted bytes of the files that were OK,
    the raw UTF-16LE names buffer)."""
    lib = native.ref_cont()
    lib.ref_7z_extract.restype = ctypes.c_int
    lib.ref_7z_extract.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                   ctypes.c_size_t, _sp, ctypes.POINTER(ctypes.c_int),
                                   ctypes.POINTER(ctypes.c_uint64),
                                   ctypes.POINTER(ctypes.c_uint), ctypes.c_uint, ctypes.c_char_p,
                                   ctypes.c_size_t, _sp]
    cap = 16 << 20
    out = ctypes.create_string_buffer(cap)
    ol = ctypes.c_size_t(0)
    fres = (ctypes.c_int * max_files)()
    fsz = (ctypes.c_uint64 * max_files)()
    nf = ctypes.c_uint(0)
    names = ctypes.create_string_buffer(1 << 20)
    nl = ctypes.c_size_t(0)
    r = lib.ref_7z_extract(arc, len(arc), out, cap, ctypes.byref(ol), fres, fsz, ctypes.byref(nf),
                           max_files, names, len(names), ctypes.byref(nl))
    n = nf.value
    return r, [fres[i] for i in range(n)], [fsz[i] for i in range(n)], out.raw[:ol.value], \
        names.raw[:nl.value]


def arm_like(seed, n):
    """ARM-flavoured words: one in six is a BL (top byte 0xEB) with a near target."""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        if rng.random() < 1 / 6:
            out += struct.pack("<I", 0xEB000000 | (rng.randrange(-3000, 3000) & 0xFFFFFF))
        else:
            out += struct.pack("<I", rng.choice((0xE1A00000, 0xE59F0000, 0xE3A00000)) |
                               rng.randrange(1 << 12))
    return bytes(out[:n])


class Archive:
    """An archive description: groups (method index, [(name, bytes)]) are
    folders, loose entries (name, None | b"") have no data.  `order` lists them
    as the caller's item list has them."""

    def __init__(self, L, methods):
        self.L = L
        self.methods = methods
        self.order = []      # ("group", method index, files) | ("empty", name, is_dir)

    def group(self, method, files):
        assert all(len(d) for _, d in files)
        self.order.append(("group", method, files))
        return self

    def empty(self, name, is_dir=False):
        self.order.append(("empty", name, is_dir))
        return self

    def build(self):
        """(src bytes, SzItem array, n, names, names_len)."""
        L = self.L
        src, entries = bytearray(b"\x5a" * 3), []   # folders start at odd offsets
        for e in self.order:
            if e[0] == "empty":
                entries.append((e[1], 0, 0, L.SZ_ITEM_DIR if e[2] else 0, 0))
                continue
            for j, (name, data) in enumerate(e[2]):
                entries.append((name, len(src), len(data), L.SZ_ITEM_JOIN if j else 0, e[1]))
                src += data
            src += b"\x5a" * (1 + len(src) % 2)
        items, names, names_len = L.sz_items(entries)
        return bytes(src), items, len(entries), names, names_len

    def groups(self):
        return [e for e in self.order if e[0] == "group"]

    def empties(self):
        return [(e[1], e[2]) for e in self.order if e[0] == "empty"]

    def item_names(self):
        out = []
        for e in self.order:
            out += [e[1]] if e[0] == "empty" else [n for n, _ in e[2]]
        return out

    def data_files(self):
        return [d for e in self.groups() for _, d in e[2]]

    def names_buffer(self):
        return b"".join(n.encode("utf-16-le") + b"\0\0" for n in self.item_names())


def filtered(data, filter_id):
    """The folder's bytes after the x86 (4) or ARM (7) filter, by liblzma."""
    import lzma
    if not filter_id:
        return data
    return W.x86_encode(data, lzma.FILTER_X86 if filter_id == 4 else lzma.FILTER_ARM)


def helper_folder(L, method, files, packed, props):
    """The layout helper's folder for a method-table row and a pack stream."""
    return W.Folder(files, method=method.method, packed=packed, props=props,
                    bcj=method.filter == L.SZ_FILTER_X86, arm=method.filter == L.SZ_FILTER_ARM)


def crcs_of(arc_items):
    return [zlib.crc32(d) for d in arc_items]

"""The pack stage's case list (csrc/sevenz_pack_device.h): hand-made piece
tables over hand-made result arrays, a plain Python model of scan and gather,
the host emulator's build (tests/emu_7zpack/pack_emu.cpp) and the case file its
stand-alone sanitizer build reads.  tests/test_7zenc_host.py runs the list
through the emulator, tests/test_7zenc_gpu.py through SzGpu_PackBatch."""
import ctypes
import os
import random
import struct
import subprocess

import native

CSRC = os.path.join(native.ROOT, "lzma-sdk-zliblike_amd", "csrc")
EMU_SRC = os.path.join(native.ROOT, "tests", "emu_7zpack", "pack_emu.cpp")

OK, PARAM, OUTPUT_EOF = 0, 5, 7
COPY, LZMA, LZMA2, PPMD = 0, 1, 2, 3
LAST = 1
TILE = 256            # pieces per first-level tile
SECOND = TILE * TILE  # pieces one pass of the second level covers (one tile sum per thread)
POISON = 0xEE
GUARD = 48
LENGTHS = (0, 1, 15, 16, 17, 31, 33, 4097)
NULL = (1 << 64) - 1


class Piece(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64), ("slot", ctypes.c_uint32),
                ("folder", ctypes.c_uint32), ("kind", ctypes.c_uint16), ("base", ctypes.c_uint16),
                ("flags", ctypes.c_uint32)]


class EncResult(ctypes.Structure):
    _fields_ = [("res", ctypes.c_int32), ("_pad", ctypes.c_uint32), ("dest_len", ctypes.c_uint64)]


class PpmdResult(ctypes.Structure):
    _fields_ = [("res", ctypes.c_int32), ("_pad", ctypes.c_uint32), ("dest_len", ctypes.c_uint64),
                ("packed_len", ctypes.c_uint64)]


class Args(ctypes.Structure):
    _fields_ = [("d_pieces", ctypes.c_void_p), ("n", ctypes.c_uint64),
                ("n_folders", ctypes.c_uint64), ("bases", ctypes.c_void_p * 4),
                ("d_lzma", ctypes.c_void_p), ("n_lzma", ctypes.c_uint64),
                ("d_lzma2", ctypes.c_void_p), ("n_lzma2", ctypes.c_uint64),
                ("d_ppmd", ctypes.c_void_p), ("n_ppmd", ctypes.c_uint64),
                ("d_out", ctypes.c_void_p), ("out_cap", ctypes.c_uint64),
                ("d_scratch", ctypes.c_void_p), ("d_piece_off", ctypes.c_void_p),
                ("d_folder_size", ctypes.c_void_p), ("d_total", ctypes.c_void_p)]


assert ctypes.sizeof(Piece) == 32 and ctypes.sizeof(Args) == 152


class Case:
    """pieces: dicts (kind, base, off, len, slot, folder, flags); bases: four
    bytearrays or None; results: lists of (res, dest_len) per kind."""

    def __init__(self, name):
        self.name = name
        self.pieces = []
        self.bases = [bytearray(), bytearray(), None, None]
        self.res = {LZMA: [], LZMA2: [], PPMD: []}
        self.n_folders = 0
        self.out_mis = 0
        self.short = 0       # out_cap = the total - short

    def add(self, rng, kind, length, folder, src_mis=None, base=None, last=False, res=OK):
        """One piece of `length` fresh bytes; its source starts src_mis bytes
        into a 16-byte granule of its base (any when None)."""
        if base is None:
            base = 0 if kind == COPY else rng.choice((1, 1, 2, 3))
        if self.bases[base] is None:
            self.bases[base] = bytearray()
        b = self.bases[base]
        if src_mis is not None:
            b += bytes([0x5A]) * ((src_mis - len(b)) % 16)
        else:
            b += bytes([0x5A]) * rng.randrange(3)
        off = len(b)
        b += rng.randbytes(length)
        slot = 0
        if kind != COPY:
            slot = len(self.res[kind])
            # a failed stream's dest_len is not a length to gather
            self.res[kind].append((res, length if res == OK else length + 7))
        self.pieces.append(dict(kind=kind, base=base, off=off, len=length if kind == COPY else 0,
                                slot=slot, folder=folder, flags=LAST if last else 0))
        self.n_folders = max(self.n_folders, folder + 1)


def length_of(case, p):
    """(length, res) of a piece as the kernels see it."""
    if p["folder"] >= case.n_folders or p["base"] >= 4 or case.bases[p["base"]] is None or \
            p["flags"] & ~LAST:
        return 0, PARAM
    if p["kind"] == COPY:
        return p["len"], OK
    if p["kind"] not in case.res or p["slot"] >= len(case.res[p["kind"]]):
        return 0, PARAM
    res, n = case.res[p["kind"]][p["slot"]]
    return (n, OK) if res == OK else (0, res)


def model(case):
    """What the pack stage leaves: total (res, index, dest_len), piece offsets,
    folder sizes (None unless SZ_OK), the image of out_cap + GUARD bytes."""
    offs, at, bad = [], 0, None
    vals = []
    for i, p in enumerate(case.pieces):
        n, res = length_of(case, p)
        if res != OK and bad is None:
            bad = (res, i)
        offs.append(at)
        vals.append(n)
        at += n + (1 if p["flags"] & LAST else 0)
    out_cap = max(at - case.short, 0)
    image = bytearray([POISON]) * (out_cap + GUARD)
    if bad is not None:
        return dict(total=(bad[0], bad[1], at), offs=offs, sizes=None, image=bytes(image),
                    out_cap=out_cap)
    if at > out_cap:
        return dict(total=(OUTPUT_EOF, 0, at), offs=offs, sizes=None, image=bytes(image),
                    out_cap=out_cap)
    sizes = [0] * case.n_folders
    for p, o, n in zip(case.pieces, offs, vals):
        b = case.bases[p["base"]]
        image[o:o + n] = b[p["off"]:p["off"] + n]
        if p["flags"] & LAST:
            image[o + n] = 0
        sizes[p["folder"]] += n + (1 if p["flags"] & LAST else 0)
    return dict(total=(OK, 0, at), offs=offs, sizes=sizes, image=bytes(image), out_cap=out_cap)


def alignment_case():
    """Every source misalignment x destination misalignment x length of
    LENGTHS: a Copy filler before each piece brings the destination to the
    wanted misalignment."""
    rng = random.Random(7001)
    c = Case("alignments")
    at, folder, k = 0, 0, 0
    for dst_mis in range(16):
        for src_mis in range(16):
            for n in LENGTHS:
                fill = (dst_mis - at) % 16
                c.add(rng, COPY, fill, folder)
                at += fill
                kind = (COPY, LZMA, LZMA2, PPMD)[k % 4]
                c.add(rng, kind, n, folder + 1, src_mis=src_mis)
                at += n
                folder += 2
                k += 1
    return c


def mixed_case(n, seed, terminators=True):
    """n pieces of random kinds, bases and lengths in folders of 1..5 pieces;
    LZMA2 folders end in a 0x00: the first, a middle and the last folder are
    LZMA2 folders."""
    rng = random.Random(seed)
    c = Case(f"mixed {n}")
    c.out_mis = rng.randrange(16)
    groups, left = [], n
    while left:
        g = min(left, rng.randrange(1, 6))
        groups.append(g)
        left -= g
    forced = {0, len(groups) // 2, len(groups) - 1} if terminators else set()
    for f, g in enumerate(groups):
        kind = LZMA2 if f in forced else rng.choice((COPY, LZMA, LZMA2, PPMD))
        for j in range(g):
            c.add(rng, kind, rng.choice((0, 1, 5, 16, 33, 40)) if n > 300 else rng.randrange(70),
                  f, last=kind == LZMA2 and j == g - 1)
    return c


def cases():
    out = [alignment_case()]
    for k, n in enumerate((1, TILE - 1, TILE, TILE + 1, SECOND + 1)):
        out.append(mixed_case(n, 7100 + k))
    rng = random.Random(7200)
    c = Case("no pieces")
    out.append(c)
    c = mixed_case(300, 7201)
    c.name = "a failed piece"
    c.res[PPMD][len(c.res[PPMD]) // 2] = (OUTPUT_EOF, 9)
    out.append(c)
    c = mixed_case(300, 7202)
    c.name = "two failed pieces: the first is reported"
    c.res[LZMA][1] = (PARAM, 0)
    c.res[LZMA2][0] = (OUTPUT_EOF, 3)
    out.append(c)
    c = mixed_case(40, 7203)
    c.name = "a slot out of range"
    c.pieces[17]["kind"], c.pieces[17]["slot"] = LZMA, len(c.res[LZMA])
    out.append(c)
    c = mixed_case(40, 7204)
    c.name = "an unknown kind"
    c.pieces[3]["kind"] = 4
    out.append(c)
    c = mixed_case(40, 7205)
    c.name = "a folder out of range"
    c.pieces[39]["folder"] = c.n_folders
    out.append(c)
    c = mixed_case(40, 7206)
    c.name = "a base that is not given"
    c.bases[3] = None
    c.pieces[5]["base"] = 3
    out.append(c)
    c = mixed_case(300, 7207)
    c.name = "capacity one byte short"
    c.short = 1
    out.append(c)
    c = Case("one Copy piece of the source")
    c.add(rng, COPY, 1000, 0, src_mis=3)
    out.append(c)
    return out


# ---------------------------------------------------------------- marshalling

def tables(case):
    """ctypes arrays: pieces, the three result arrays."""
    n = len(case.pieces)
    pieces = (Piece * max(n, 1))()
    for i, p in enumerate(case.pieces):
        q = pieces[i]
        q.off, q.len, q.slot, q.folder = p["off"], p["len"], p["slot"], p["folder"]
        q.kind, q.base, q.flags = p["kind"], p["base"], p["flags"]
    lz = (EncResult * max(len(case.res[LZMA]), 1))()
    l2 = (EncResult * max(len(case.res[LZMA2]), 1))()
    pp = (PpmdResult * max(len(case.res[PPMD]), 1))()
    for arr, kind in ((lz, LZMA), (l2, LZMA2), (pp, PPMD)):
        for i, (res, dl) in enumerate(case.res[kind]):
            arr[i].res, arr[i].dest_len = res, dl
            if kind == PPMD:
                arr[i].packed_len = dl
    return pieces, lz, l2, pp


def build_emu(out_dir, extra=(), main=False):
    out = os.path.join(str(out_dir), "pack_emu_main" if main else "libpack_emu.so")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC]
    cmd += ["-DSZPACK_EMU_MAIN"] if main else ["-fPIC", "-shared"]
    cmd += list(extra) if extra else ["-O2"]
    subprocess.run(cmd + [EMU_SRC, "-o", out], check=True)
    return out


def load_emu(so):
    lib = ctypes.CDLL(so)
    lib.szpack_emu_run.restype = None
    lib.szpack_emu_run.argtypes = [ctypes.POINTER(Args)]
    lib.szpack_emu_scratch_words.restype = ctypes.c_uint64
    lib.szpack_emu_scratch_words.argtypes = [ctypes.c_uint64]
    lib.szpack_emu_tile.restype = ctypes.c_uint32
    return lib


def _aligned(data, mis=0, extra=0):
    """(keep-alive buffer, address with address % 16 == mis) holding data; the
    bytes around it are POISON."""
    size = len(data) + extra
    buf = ctypes.create_string_buffer(bytes([POISON]) * (size + 48), size + 48)
    addr = ctypes.addressof(buf)
    at = (-addr) % 16 + mis
    ctypes.memmove(addr + at, bytes(data), len(data))
    return buf, addr + at


def run_emu(lib, case, want):
    """The emulator's (total, offs, sizes, image) for a case."""
    n = len(case.pieces)
    pieces, lz, l2, pp = tables(case)
    keep, a = [], Args()
    a.d_pieces, a.n, a.n_folders = ctypes.addressof(pieces), n, case.n_folders
    for k, b in enumerate(case.bases):
        if b is not None:
            buf, addr = _aligned(b)
            keep.append(buf)
            a.bases[k] = addr
    a.d_lzma, a.n_lzma = ctypes.addressof(lz), len(case.res[LZMA])
    a.d_lzma2, a.n_lzma2 = ctypes.addressof(l2), len(case.res[LZMA2])
    a.d_ppmd, a.n_ppmd = ctypes.addressof(pp), len(case.res[PPMD])
    image = want["out_cap"] + GUARD
    obuf, oaddr = _aligned(bytes([POISON]) * image, case.out_mis)
    a.d_out, a.out_cap = oaddr, want["out_cap"]
    scratch = (ctypes.c_uint64 * lib.szpack_emu_scratch_words(n))()
    offs = (ctypes.c_uint64 * max(n, 1))()
    sizes = (ctypes.c_uint64 * max(case.n_folders, 1))()
    total = EncResult()
    a.d_scratch, a.d_piece_off = ctypes.addressof(scratch), ctypes.addressof(offs)
    a.d_folder_size, a.d_total = ctypes.addressof(sizes), ctypes.addressof(total)
    lib.szpack_emu_run(ctypes.byref(a))
    assert obuf.raw[:oaddr - ctypes.addressof(obuf)].count(POISON) == oaddr - ctypes.addressof(obuf)
    return ((total.res, total._pad, total.dest_len), list(offs)[:n], list(sizes)[:case.n_folders],
            ctypes.string_at(oaddr, image))


def check(case, got, want):
    total, offs, sizes, image = got
    assert total == want["total"], (case.name, total, want["total"])
    assert offs == want["offs"], case.name
    if want["sizes"] is not None:
        assert sizes == want["sizes"], case.name
    assert image == want["image"], case.name


def write_case_file(path, case_list):
    """The stand-alone emulator's input (the layout is in pack_emu.cpp)."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(case_list)))
        for c in case_list:
            w = model(c)
            pieces, lz, l2, pp = tables(c)
            n = len(c.pieces)
            nl, n2, np_ = len(c.res[LZMA]), len(c.res[LZMA2]), len(c.res[PPMD])
            f.write(struct.pack("<8Q", n, c.n_folders, nl, n2, np_, w["out_cap"], c.out_mis, GUARD))
            f.write(struct.pack("<4Q", *[NULL if b is None else len(b) for b in c.bases]))
            f.write(bytes(pieces)[:32 * n] + bytes(lz)[:16 * nl] + bytes(l2)[:16 * n2] +
                    bytes(pp)[:24 * np_])
            for b in c.bases:
                if b is not None:
                    f.write(bytes(b))
            f.write(struct.pack("<iIQ", *w["total"]))
            f.write(struct.pack(f"<{n}Q", *w["offs"]))
            f.write(struct.pack("<Q", 0 if w["sizes"] is None else 1))
            f.write(struct.pack(f"<{c.n_folders}Q", *(w["sizes"] or [0] * c.n_folders)))
            f.write(w["image"])

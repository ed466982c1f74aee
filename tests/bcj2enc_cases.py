"""Shared cases of the BCJ2 encoder tests (tests/test_bcj2enc_emu.py,
tests/test_bcj2enc_gpu.py): the generators, the case list, the model
(tests/bcj2enc.py's encode, the executable specification), batch layouts with
guard bytes, and the host build of csrc/bcj2enc_device.h
(tests/emu_bcj2enc/bcj2enc_emu.cpp)."""
import ctypes
import functools
import os
import random
import struct
import subprocess

import bcj2enc
import native

CSRC = os.path.join(native.ROOT, "lzma-sdk-zliblike_amd", "csrc")
EMU_SRC = os.path.join(native.ROOT, "tests", "emu_bcj2enc", "bcj2enc_emu.cpp")

OK, UNSUPPORTED, OUTPUT_EOF = 0, 4, 7
# the implementation's internal boundaries in bytes: a thread's run, a wave's
# segment, a workgroup's step (test_geometry pins them to the code's)
RUN, SEG, STEP = 16, 1024, 4096
SCAN = 64 * SEG     # the bytes of one step of the scan over a stream's segments
SIZES = list(range(0, 11)) + [63, 64, 65, 255, 256, 257, 4096, 20000]
GUARD = 0xEE


class Range(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint64), ("cap", ctypes.c_uint64)]


class Desc(ctypes.Structure):
    _fields_ = [("src_off", ctypes.c_uint64), ("src_len", ctypes.c_uint64), ("out", Range * 4)]


class Result(ctypes.Structure):
    _fields_ = [("res", ctypes.c_int32), ("_pad", ctypes.c_uint32), ("len", ctypes.c_uint64 * 4)]


# ---------------------------------------------------------------- generators

def nested(seed, n):
    """Branch opcodes whose operand bytes begin with another opcode; rel values
    small positive, small negative or wrapping, so that many convertible
    candidates sit inside the operand of an earlier converted one."""
    rng = random.Random(seed)
    out = bytearray()
    ops = [b"\xe8", b"\xe9", b"\x0f\x84", b"\x0f\x8f", b"\xe8"]
    while len(out) < n:
        r = rng.random()
        if r < 0.55:
            out += rng.choice(ops)
            inner = rng.choice([0xE8, 0xE9, 0xE8, 0x0F])
            kind = rng.random()
            if kind < 0.6:      # small positive, low byte an opcode
                rel = inner | (rng.randrange(0, max(1, min(n, 1 << 16)) >> 8 or 1) << 8)
            elif kind < 0.8:    # small negative
                rel = (-rng.randrange(1, 300)) & 0xFFFFFFFF
            elif kind < 0.9:    # wraps around: target = position + 5 + rel - 2^32
                rel = (0x100000000 - rng.randrange(0, 64)) & 0xFFFFFFFF
            else:
                rel = rng.randrange(1 << 32)
            out += struct.pack("<I", rel)
            if rng.random() < 0.7:
                out += rng.choice([b"\0", b"\0\0", b"\x80\0\0\0\0", b"\xff"])
        elif r < 0.7:
            out += rng.choice([b"\xe8\xe8\xe8", b"\x0f\x0f\x80", b"\xe9\xe8", b"\xe8\0\0\0\0\xe8"])
        else:
            out += bytes([rng.randrange(0x20, 0x7F)])
    return bytes(out[:n])


ALPHABET = bytes([0xE8, 0xE9, 0x0F, 0x80, 0x84, 0x8F, 0x00, 0xFF, 0x01, 0x10])


def small_alphabet(seed, n):
    rng = random.Random(seed)
    return bytes(rng.choice(ALPHABET) for _ in range(n))


def branch_at(n, pos, op=b"\xe8", target=0, fill=0x41):
    """n filler bytes with one branch whose opcode's last byte is at `pos` and
    whose absolute target is `target` (operand clipped at n)."""
    d = bytearray([fill]) * n
    at = pos - (len(op) - 1)
    rel = (target - (pos + 5)) & 0xFFFFFFFF
    ins = (op + struct.pack("<I", rel))[:max(0, n - at)]
    d[at:at + len(ins)] = ins
    return bytes(d[:n])


def hand_cases():
    c = []
    for op in (b"\xe8", b"\xe9", b"\x0f\x85"):
        c.append(("op last " + op.hex(), b"ab" + op))
        for tail in (1, 2, 3, 4):
            c.append(("op tail %d %s" % (tail, op.hex()), b"ab" + op + b"\0" * tail))
    c.append(("0f e8", b"\x0f\xe8\x10\0\0\0" + b"x" * 40))
    c.append(("0f e8 last", b"\x0f\xe8"))
    n = 100
    for name, t in (("target 0", 0), ("target n-1", n - 1), ("target n", n)):
        for op in (b"\xe8", b"\xe9", b"\x0f\x84"):
            c.append(("%s %s" % (name, op.hex()), branch_at(n, 40, op, t)))
    c.append(("rel wraps below zero", branch_at(n, 10, b"\xe8", -1 & 0xFFFFFFFF)))
    c.append(("rel below zero by a lot", branch_at(n, 10, b"\xe9", (-4000) & 0xFFFFFFFF)))
    # a convertible opcode at each of the ten positions around every internal
    # boundary, its operand straddling it
    for bound in (RUN, SEG, STEP, SCAN):
        for pos in range(bound - 5, bound + 5):
            op = (b"\xe8", b"\xe9", b"\x0f\x8c")[pos % 3]
            c.append(("bound %d pos %d" % (bound, pos), branch_at(bound + 40, pos, op, bound // 2)))
            # a second convertible opcode as the first's first operand byte
            # (dead), and a third right behind the operand (live)
            d = bytearray(b"\x41" * (bound + 300))
            d[pos:pos + 6] = b"\xe8\xe8\0\0\0\0"
            c.append(("bound %d pos %d dead pair" % (bound, pos), bytes(d)))
            d[pos + 5:pos + 10] = b"\xe9" + struct.pack("<I", (5 - (pos + 10)) & 0xFFFFFFFF)
            c.append(("bound %d pos %d live pair" % (bound, pos), bytes(d)))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, data)]"""
    c = []
    for k, n in enumerate(SIZES):
        c.append(("x86 0.06 n=%d" % n, bcj2enc.x86_like(100 + k, n, 0.06)))
        c.append(("x86 0.3 n=%d" % n, bcj2enc.x86_like(200 + k, n, 0.3)))
        c.append(("nested n=%d" % n, nested(300 + k, n)))
        c.append(("alphabet n=%d" % n, small_alphabet(400 + k, n)))
    c.append(("nested n=70001", nested(7, 70001)))  # more segments than one stream-scan step
    return tuple(c + hand_cases())


# ---------------------------------------------------------------- the model

@functools.lru_cache(maxsize=None)
def _model(data):
    return bcj2enc.encode(data)


def model(data):
    """(main, call, jump, rc) of tests/bcj2enc.py's encode."""
    return _model(bytes(data))


def decisions(data):
    """The restated rule, position by position: [(i, kind, conv, live)] for
    every candidate; kind 0 = E8, 1 = E9, 2 = Jcc."""
    n = len(data)
    out, s = [], 0
    for i in range(n):
        b, prev = data[i], data[i - 1] if i else 0
        isj = bcj2enc.is_j(prev, b)
        conv = False
        if isj and i + 5 <= n:
            rel = struct.unpack_from("<I", data, i + 1)[0]
            conv = (i + 5 + rel) % (1 << 32) < n
        live = s == 0
        if isj:
            out.append((i, 0 if b == 0xE8 else 1 if b == 0xE9 else 2, conv, live))
        s = s - 1 if s > 0 else (4 if conv else 0)
    return out


def bound(n):
    return [n, 4 * (n // 5), 4 * (n // 5), 5 + n]


# ---------------------------------------------------------------- batches

def lay_out(items, start=1):
    """items: [(data, caps or None)] -> (descs, src, dst_size).  Streams at odd
    offsets in src; every output range with GUARD bytes around it in dst."""
    descs = (Desc * len(items))()
    src = bytearray(b"\x5a" * start)
    at = 3
    for k, (data, caps) in enumerate(items):
        if len(src) % 2 == 0:
            src += b"\x5a"
        descs[k].src_off, descs[k].src_len = len(src), len(data)
        src += data + b"\x5a" * (1 + k % 3)
        caps = caps or [len(s) for s in model(data)]
        for j in range(4):
            descs[k].out[j].off, descs[k].out[j].cap = at, caps[j]
            at += caps[j] + 1 + (k + j) % 4
    return descs, bytes(src), at + 8


def expect(items, dst_size, descs):
    """The results and the dst image the model gives for a batch."""
    image = bytearray([GUARD]) * dst_size
    results = []
    for k, (data, caps) in enumerate(items):
        streams = model(data)
        lens = [len(s) for s in streams]
        res = OK
        for j in range(4):
            cap = descs[k].out[j].cap
            keep = min(lens[j], cap)
            if j in (1, 2):
                keep -= keep % 4   # a target is written whole or not at all
            if lens[j] > cap:
                res = OUTPUT_EOF
            o = descs[k].out[j].off
            image[o:o + keep] = streams[j][:keep]
        results.append((res, lens))
    return results, bytes(image)


def short_cap_items():
    """Exact capacities, and one short for each of the four streams."""
    items = []
    for name, data in cases():
        if len(data) not in (10, 65, 257, 4096) and not name.startswith("bound 16 "):
            continue
        lens = [len(s) for s in model(data)]
        items.append((data, list(lens)))
        for j in range(4):
            if lens[j]:
                caps = list(lens)
                caps[j] -= 1
                items.append((data, caps))
    return items


# ---------------------------------------------------------------- the host build

def build_emu(out_dir, extra=(), main=False):
    out = os.path.join(str(out_dir), "bcj2enc_emu_main" if main else "libbcj2enc_emu.so")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-DLZGPU_HOST_EMU", "-I", CSRC]
    cmd += (["-DBCJ2ENC_EMU_MAIN"] if main else ["-fPIC", "-shared"])
    cmd += list(extra) if extra else ["-O2"]
    subprocess.run(cmd + [EMU_SRC, "-o", out], check=True)
    return out


def load_emu(so):
    lib = ctypes.CDLL(so)
    lib.bcj2enc_emu_scratch.restype = ctypes.c_uint64
    lib.bcj2enc_emu_scratch.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    lib.bcj2enc_emu_geometry.argtypes = [ctypes.c_void_p]
    lib.bcj2enc_emu_run.restype = None
    lib.bcj2enc_emu_run.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_uint32]
    return lib


def emu_run(lib, descs, src, dst_size, grid=3, poison=0xA7):
    n = len(descs)
    dst = ctypes.create_string_buffer(bytes([GUARD]) * dst_size, dst_size)
    sbytes = lib.bcj2enc_emu_scratch(descs, n)
    scratch = ctypes.create_string_buffer(bytes([poison]) * sbytes, sbytes)
    res = (Result * n)()
    lib.bcj2enc_emu_run(descs, n, src, dst, scratch, res, grid)
    return [(r.res, list(r.len)) for r in res], dst.raw


def write_case_file(path, batches):
    """batches: [(items, grid)]; the records of the stand-alone emulator."""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(batches)))
        for items, grid in batches:
            descs, _, dst_size = lay_out(items)
            at = 0
            for k, (data, _) in enumerate(items):   # the source is exactly the streams
                descs[k].src_off = at
                at += len(data)
            results, image = expect(items, dst_size, descs)
            f.write(struct.pack("<QQQ", len(items), dst_size, grid))
            f.write(bytes(descs))
            for data, _ in items:
                f.write(data)
            for res, lens in results:
                f.write(struct.pack("<iI4Q", res, 0, *lens))
            f.write(image)

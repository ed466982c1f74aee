"""SHA-256 on the GPU: the per-block device code on the host (tests/emu_sha256/,
sha256_device.h under LZGPU_HOST_EMU) against hashlib and the reference's
Sha256.c traces (tests/golden/sha256_cases.json), then the same on the device:
the Sha256.h drop-ins call by call and Sha256Gpu_Batch with each kernel.
"""
import ctypes
import hashlib
import importlib.util
import json
import os
import random
import struct
import subprocess

import pytest

import native

EMU_DIR = os.path.join(native.ROOT, "tests", "emu_sha256")
GOLDEN = os.path.join(native.ROOT, "tests", "golden", "sha256_cases.json")

S = 4096  # bytes one pass of the wave kernel takes (64 lanes x 64-byte blocks)
EDGE_LENGTHS = list(range(131)) + [S - 1, S, S + 1, S + 55, S + 56, S + 63,
                                   2 * S - 1, 2 * S, 2 * S + 9]
FIPS_56 = b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq"
FIPS = [(b"", "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"),
        (b"abc", "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"),
        (FIPS_56, "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1"),
        (b"a" * 1000000, "cdc76e5c9914fb9281a1c7e284d73e67f1809a48a497200e046d39ccc7112cd0")]
POISON = 0xA5


def rand_bytes(seed, n):
    return random.Random(seed).randbytes(n)


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-s", "-f", "tests/emu_sha256/Makefile"], cwd=native.ROOT, check=True)
    lib = ctypes.CDLL(os.path.join(EMU_DIR, "libsha_emu.so"))
    for f in (lib.emu_sha256_lane, lib.emu_sha256_wave):
        f.restype = None
        f.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                      ctypes.c_int, ctypes.c_void_p]
    lib.emu_sha256_super_bytes.restype = ctypes.c_uint32
    assert lib.emu_sha256_super_bytes() == S
    return lib


PATHS = ("lane", "wave")


def emu_hash(emu, path, buf, at, n, init=None, prior=0, finalise=1, out=None, out_at=0):
    """One range buf[at, at + n) through an emulated path; the 32 output bytes."""
    f = emu.emu_sha256_lane if path == "lane" else emu.emu_sha256_wave
    out = out if out is not None else ctypes.create_string_buffer(32)
    st = (ctypes.c_uint32 * 8)(*init) if init is not None else None
    f(ctypes.addressof(buf) + at, n, st, prior, finalise, ctypes.addressof(out) + out_at)
    return out.raw[out_at:out_at + 32]


def one_shot(emu, path, data):
    return emu_hash(emu, path, ctypes.create_string_buffer(data, max(len(data), 1)), 0, len(data))


# ---------------------------------------------------------------- golden traces

def golden_cases():
    with open(GOLDEN) as f:
        d = json.load(f)
    spec = importlib.util.spec_from_file_location(
        "make_golden_sha256", os.path.join(os.path.dirname(GOLDEN), "make_golden_sha256.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = []
    for c in d["cases"]:
        c = dict(c)
        if isinstance(c["sizes"], dict):
            c["sizes"] = [c["sizes"]["repeat"][0]] * c["sizes"]["repeat"][1]
        c["msg"] = gen.message(c, c["seed"])
        out.append(c)
    return out


def state_at(case, call):
    """The reference's state words after call `call` (0 = Sha256_Init)."""
    cur = None
    for first, st in case["states"]:
        if first <= call:
            cur = st
    return struct.unpack("<8I", bytes.fromhex(cur))


IV = (0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
      0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19)


def test_golden_digests_match_hashlib():
    cases = golden_cases()
    assert len(cases) >= 20
    for c in cases:
        assert len(c["msg"]) == sum(c["sizes"])
        assert c["digest"] == hashlib.sha256(c["msg"]).hexdigest(), c["sizes"][:8]
        assert state_at(c, 0) == IV
        # Sha256_Final re-initialises: the IV, count 0, nothing buffered
        assert bytes.fromhex(c["final"]) == struct.pack("<8I", *IV) + bytes(8)


# ---------------------------------------------------------------- the device code on the host

@pytest.mark.parametrize("path", PATHS)
def test_emu_fips_vectors(emu, path):
    for msg, want in FIPS:
        assert one_shot(emu, path, msg).hex() == want, len(msg)


@pytest.mark.parametrize("path", PATHS)
def test_emu_edge_lengths(emu, path):
    data = rand_bytes(1, max(EDGE_LENGTHS))
    for n in EDGE_LENGTHS:
        assert one_shot(emu, path, data[:n]) == hashlib.sha256(data[:n]).digest(), n


@pytest.mark.parametrize("path", PATHS)
def test_emu_packed_alignments_with_poison(emu, path):
    """Ranges packed at every start alignment 0..15 with poison margins; the
    digests land in a poisoned buffer at odd offsets and nothing else changes."""
    lengths = [0, 1, 55, 56, 63, 64, 65, 119, 120, 130, S - 1, S, S + 56, 2 * S + 9]
    packed, ranges = bytearray(), []
    for k, n in enumerate(lengths * 16):
        packed += bytes([POISON]) * 16
        packed += bytes([POISON]) * ((k // len(lengths) - len(packed)) % 16)
        ranges.append((len(packed), n))
        packed += rand_bytes(100 + k, n)
    packed += bytes([POISON]) * 16
    assert {at % 16 for at, _ in ranges} == set(range(16))
    buf = ctypes.create_string_buffer(bytes(packed), len(packed))
    out = ctypes.create_string_buffer(bytes([POISON]) * (33 * len(ranges) + 64), 33 * len(ranges) + 64)
    for k, (at, n) in enumerate(ranges):
        got = emu_hash(emu, path, buf, at, n, out=out, out_at=32 + 33 * k)
        assert got == hashlib.sha256(bytes(packed[at:at + n])).digest(), (at, n)
    assert buf.raw == bytes(packed)
    o = out.raw
    assert o[:32] == bytes([POISON]) * 32 and o[32 + 33 * len(ranges):] == bytes([POISON]) * 32
    assert all(o[32 + 33 * k + 32] == POISON for k in range(len(ranges)))


@pytest.mark.parametrize("path", PATHS)
def test_emu_reproduces_reference_states(emu, path):
    """Sha256_Update's hand-over (buffered bytes + whole blocks, continued from
    the state) through the device code's state mode, against Sha256.c's states."""
    for c in golden_cases():
        msg, fed, st = c["msg"], 0, IV
        for call, n in enumerate(c["sizes"], 1):
            done = fed - (fed & 63)  # bytes already compressed
            fed += n
            whole = (fed - done) & ~63
            if whole:
                chunk = ctypes.create_string_buffer(msg[done:done + whole], whole)
                st = struct.unpack("<8I", emu_hash(emu, path, chunk, 0, whole, st, done, 0))
            assert st == state_at(c, call), (c["sizes"][:8], call)
        done = fed - (fed & 63)
        tail = ctypes.create_string_buffer(msg[done:], max(fed - done, 1))
        assert emu_hash(emu, path, tail, 0, fed - done, st, done, 1).hex() == c["digest"]


def test_sanitizer_edge_program_runs_clean(emu):
    """tests/emu_sha256/sha_edges (AddressSanitizer + UBSan, its own main): both
    paths over exactly-sized heap ranges at every alignment; an over-read trips."""
    r = subprocess.run([os.path.join(EMU_DIR, "sha_edges")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "16 alignments, 0 failures" in r.stdout and not r.stderr, r.stdout + r.stderr


def test_batch_parameter_errors_need_no_device():
    import lzmagpu as L
    assert L.sha256_batch_device(0, 0, 0, 1, 0, kernel=3) == L.SZ_ERROR_PARAM
    assert L.sha256_batch_device(0, 0, 0, 1 << 32, 0) == L.SZ_ERROR_PARAM


# ---------------------------------------------------------------- GPU: drop-ins

def defined_part(p):
    return (struct.pack("<8I", *p.state) + struct.pack("<Q", p.count)
            + bytes(p.buffer[:p.count & 63]))


@pytest.mark.gpu
def test_gpu_dropins_follow_reference_call_by_call():
    import lzmagpu as L
    for c in golden_cases():
        msg, fed = c["msg"], 0
        p = L.CSha256()
        ctypes.memset(ctypes.byref(p), POISON, ctypes.sizeof(p))
        L.Sha256_Init(p)
        trace = hashlib.sha256(defined_part(p))
        assert tuple(p.state) == IV and p.count == 0
        for call, n in enumerate(c["sizes"], 1):
            L.Sha256_Update(p, msg[fed:fed + n])
            fed += n
            assert tuple(p.state) == state_at(c, call), (c["sizes"][:8], call)
            assert p.count == fed
            assert bytes(p.buffer[:fed & 63]) == msg[fed - (fed & 63):fed], (c["sizes"][:8], call)
            trace.update(defined_part(p))
        assert trace.hexdigest() == c["trace"], c["sizes"][:8]
        assert L.Sha256_Final(p).hex() == c["digest"], c["sizes"][:8]
        assert defined_part(p).hex() == c["final"]  # re-initialised
        # ... and usable at once for the next message
        L.Sha256_Update(p, b"abc")
        assert L.Sha256_Final(p).hex() == FIPS[1][1]


@pytest.mark.gpu
def test_gpu_dropin_sub_block_update_only_buffers():
    import lzmagpu as L
    p = L.CSha256()
    L.Sha256_Init(p)
    L.Sha256_Update(p, rand_bytes(5, 64 + 10))  # one block compressed, 10 bytes buffered
    before_err = L.last_error()
    state, tail = tuple(p.state), bytes(p.buffer)
    more = rand_bytes(6, 53)  # 10 + 53 = 63: no block completes
    L.Sha256_Update(p, more)
    assert L.last_error() == before_err
    assert tuple(p.state) == state and p.count == 64 + 63
    assert bytes(p.buffer) == tail[:10] + more + tail[63:]
    # the next byte completes the block
    L.Sha256_Update(p, b"\x00")
    assert tuple(p.state) != state and p.count == 128
    for msg, want in FIPS:
        assert L.Sha256(msg).hex() == want, len(msg)


# ---------------------------------------------------------------- GPU: batch form

def pack_ranges(lengths, seed):
    """Ranges packed at mixed alignments with poison between them:
    (packed bytes, [(offset, length)...])."""
    rng = random.Random(seed)
    packed, ranges = bytearray(bytes([POISON]) * 32), []
    for k, n in enumerate(lengths):
        packed += bytes([POISON]) * (1 + (k * 7 + rng.randrange(16)) % 16)
        ranges.append((len(packed), n))
        packed += rng.randbytes(n)
    packed += bytes([POISON]) * 32
    return bytes(packed), ranges


@pytest.fixture(scope="module")
def ragged():
    """203 ragged ranges (not a multiple of 64): every boundary length, zeros,
    random lengths up to 40,000; reference digests computed once."""
    rng = random.Random(11)
    edge = [0, 0, 0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 130,
            S - 1, S, S + 1, S + 55, S + 56, S + 63, 2 * S - 1, 2 * S, 2 * S + 9]
    lengths = edge + [rng.randrange(40001) for _ in range(203 - len(edge))]
    rng.shuffle(lengths)
    packed, ranges = pack_ranges(lengths, 12)
    assert len(ranges) == 203 and len({at % 16 for at, _ in ranges}) == 16
    want = b"".join(hashlib.sha256(packed[at:at + n]).digest() for at, n in ranges)
    return packed, ranges, want


GUARD = 64


def run_batch(L, packed, ranges, kernel):
    """Sha256Gpu_Batch over packed ranges: (res, digests); asserts that the data
    and the guard areas around the digests are unchanged."""
    import numpy as np
    import torch
    n = len(ranges)
    data = torch.from_numpy(np.frombuffer(packed, dtype=np.uint8).copy()).cuda()
    d_off = torch.tensor([at for at, _ in ranges] or [0], dtype=torch.int64, device="cuda")
    d_len = torch.tensor([ln for _, ln in ranges] or [0], dtype=torch.int64, device="cuda")
    # digests at an odd address between two guard areas
    dig = torch.full((GUARD + 1 + 32 * n + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    r = L.sha256_batch_device(data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
                              dig.data_ptr() + GUARD + 1, kernel=kernel)
    torch.cuda.synchronize()
    assert bytes(data.cpu().numpy()) == packed
    got = bytes(dig.cpu().numpy())
    assert got[:GUARD + 1] == bytes([POISON]) * (GUARD + 1)
    assert got[GUARD + 1 + 32 * n:] == bytes([POISON]) * GUARD
    return r, got[GUARD + 1:GUARD + 1 + 32 * n]


KERNELS = {"auto": 0, "lane": 1, "wave": 2}


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_gpu_batch_ragged_ranges(ragged, kernel):
    import lzmagpu as L
    packed, ranges, want = ragged
    r, got = run_batch(L, packed, ranges, KERNELS[kernel])
    assert r == 0, L.last_error()
    bad = [(k, ranges[k]) for k in range(len(ranges)) if got[32 * k:32 * k + 32] != want[32 * k:32 * k + 32]]
    assert not bad, bad[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_gpu_batch_edge_counts(kernel):
    import lzmagpu as L
    k = KERNELS[kernel]
    # n = 0: a no-op that touches nothing
    r, got = run_batch(L, bytes([POISON]) * 64, [], k)
    assert r == 0 and got == b""
    # n = 1: the FIPS million-'a' message
    msg = b"a" * 1000000
    r, got = run_batch(L, bytes([POISON]) * 3 + msg + bytes([POISON]) * 5, [(3, len(msg))], k)
    assert r == 0 and got.hex() == FIPS[3][1]
    # n = 65 x 4 KiB: the second wave of the lane kernel has one lane
    packed, ranges = pack_ranges([4096] * 65, 13)
    r, got = run_batch(L, packed, ranges, k)
    assert r == 0
    assert got == b"".join(hashlib.sha256(packed[at:at + n]).digest() for at, n in ranges)


@pytest.mark.gpu
def test_gpu_batch_auto_many_short_ranges():
    """20,000 short ranges: AUTO is in the many-ranges regime (the lane kernel)."""
    import lzmagpu as L
    rng = random.Random(14)
    packed, ranges = pack_ranges([rng.randrange(200) for _ in range(20000)], 15)
    r, got = run_batch(L, packed, ranges, 0)
    assert r == 0
    assert got == b"".join(hashlib.sha256(packed[at:at + n]).digest() for at, n in ranges)


@pytest.mark.gpu
def test_gpu_batch_unknown_kernel_is_a_parameter_error():
    import lzmagpu as L
    r, got = run_batch(L, bytes([POISON]) * 64, [(8, 8)], 3)
    assert r == L.SZ_ERROR_PARAM and got == bytes([POISON]) * 32

"""xz blocks with the SHA-256 check (XZ_CHECK_SHA256, check id 10) decoded and
checked on the GPU: LzmaGpu_XzDecode hashes them with one Sha256Gpu_Batch over
the decode's own output, after the filters.  Files are written with
tests/xzwrite.py.
"""
import random
import struct

import pytest

import native
import xzwrite as M

SZ_ERROR_DATA, SZ_ERROR_CRC = 1, 3
SIZES = [1, 55, 64, 4097, 65536, 300000, 0]


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


@pytest.fixture(scope="module")
def seven():
    """A 7-block check-10 stream: (file, [block data...])."""
    datas = [native.gen("text", 9100 + i, n) if n else b"" for i, n in enumerate(SIZES)]
    return M.make_stream([(d, {}) for d in datas], 10), datas


def x86_code(seed, n):
    """Bytes dense in CALL / JMP opcodes with small relative targets."""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += rng.randbytes(rng.randrange(1, 12))
        out += bytes([rng.choice((0xE8, 0xE9))]) + struct.pack("<i", rng.randrange(-70000, 70000))
    return bytes(out[:n])


@pytest.mark.gpu
def test_gpu_xz_sha256_blocks_decode_bit_exact(L, seven):
    data, datas = seven
    r, blocks, total = L.xz_index(data)
    assert r == 0 and [b.unpack_size for b in blocks] == SIZES
    assert all(b.check_type == 10 and b.check_size == 32 for b in blocks)
    r, out, bad = L.XzDecode(data, total)
    assert (r, bad) == (0, -1), L.last_error()
    assert out == b"".join(datas)


@pytest.mark.gpu
def test_gpu_xz_mixed_checks_across_streams(L):
    """Concatenated streams with checks 1 / 4 / 10 / 0: one decode, each check
    kind in its own batch."""
    plain, files = [], b""
    for s, chk in enumerate((1, 4, 10, 0)):
        blocks = [(native.gen("text", 9200 + 10 * s + i, 777 + 4001 * i), {}) for i in range(5)]
        files += M.make_stream(blocks, chk) + b"\0" * 4
        plain += [b for b, _ in blocks]
    r, blocks, total = L.xz_index(files)
    assert r == 0 and [b.check_type for b in blocks] == [1] * 5 + [4] * 5 + [10] * 5 + [0] * 5
    r, out, bad = L.XzDecode(files, total)
    assert (r, bad) == (0, -1) and out == b"".join(plain)
    # a stored digest of the SHA-256 stream off by one bit: reported at its block
    b = blocks[12]
    broken = bytearray(files)
    broken[b.check_off + 31] ^= 0x80
    assert L.XzDecode(bytes(broken), total)[::2] == (SZ_ERROR_CRC, 12)


@pytest.mark.gpu
def test_gpu_xz_interleaved_check_kinds_fail_at_their_own_block(L):
    """Blocks of a few hundred bytes whose check kinds alternate (streams with
    checks 4 / 1 / 10 / 0 / 1 / 10 / 4): the k-th value of a kind's batch belongs
    to that kind's k-th block, not to block k.  One stored check corrupted at a
    time, in the first and in the last block of each kind: SZ_ERROR_CRC at that
    block, and every other block's check still holds."""
    kinds = (4, 1, 10, 0, 1, 10, 4)
    plain = [native.gen("text", 9400 + i, 200 + 97 * i) for i in range(len(kinds))]
    files = b"".join(M.make_stream([(d, {})], chk) for d, chk in zip(plain, kinds))
    r, blocks, total = L.xz_index(files)
    assert r == 0 and [b.check_type for b in blocks] == list(kinds)
    assert L.XzDecode(files, total) == (0, b"".join(plain), -1)
    for i, b in enumerate(blocks):
        for at in {0, b.check_size - 1} if b.check_size else ():
            broken = bytearray(files)
            broken[b.check_off + at] ^= 0x10
            assert L.XzDecode(bytes(broken), total) == (SZ_ERROR_CRC, b"", i), (i, at)
    # two kinds broken at once: the first block in file order is the one named
    broken = bytearray(files)
    broken[blocks[5].check_off + 7] ^= 1
    broken[blocks[4].check_off + 3] ^= 1
    assert L.XzDecode(bytes(broken), total)[::2] == (SZ_ERROR_CRC, 4)


@pytest.mark.gpu
def test_gpu_xz_sha256_after_x86_filter(L):
    """The digest is of the block's final bytes: it is taken after the BCJ filter."""
    datas = [x86_code(9300 + i, n) for i, n in enumerate((5000, 70001, 3))]
    data = M.make_stream([(d, {"x86": 0}) for d in datas], 10)
    r, blocks, total = L.xz_index(data)
    assert r == 0 and all(b.x86 == 1 and b.check_type == 10 for b in blocks)
    r, out, bad = L.XzDecode(data, total)
    assert (r, bad) == (0, -1) and out == b"".join(datas)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 3, 6])
def test_gpu_xz_sha256_failures_name_their_block(L, seven, which):
    data, datas = seven
    r, blocks, total = L.xz_index(data)
    assert r == 0
    b = blocks[which]
    # one bit of the stored digest: the check error, at that block
    broken = bytearray(data)
    broken[b.check_off + 5 * which] ^= 1 << which
    r, out, bad = L.XzDecode(bytes(broken), total)
    assert (r, bad, out) == (SZ_ERROR_CRC, which, b"")
    # one bit of the block's LZMA2 data (its first control byte, made invalid or
    # made to ask for bytes the block does not have): the data error, not the
    # check error
    broken = bytearray(data)
    c = broken[b.data_off]
    broken[b.data_off] = c ^ (0x80 if c >= 0x80 else (0x02 if c else 0x01))
    assert broken[b.data_off] not in (1, 2) or c == 0
    r, out, bad = L.XzDecode(bytes(broken), total)
    assert (r, bad, out) == (SZ_ERROR_DATA, which, b"")

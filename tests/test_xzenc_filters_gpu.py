"""LzmaGpu_XzEncodeEx: filter chains in front of LZMA2 on the encode side,
against the reference's xz reader, its own filters and ref_lzma2_encode, and
against this library's reader.  The parameter errors come back before any
device work, so those tests need no GPU."""
import ctypes
import lzma
import os
import sys

import pytest

import native
import xzenc_filter_cases as X

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def ref_xz_decode(data, cap):
    lib = native.ref_cont()
    f = lib.ref_xz_decode
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_char_p, native.size_t_p, ctypes.c_char_p, native.size_t_p,
                  native.int_p, native.int_p]
    out = ctypes.create_string_buffer(max(cap, 1))
    dl, sl = ctypes.c_size_t(cap), ctypes.c_size_t(len(data))
    st, done = ctypes.c_int(-1), ctypes.c_int(0)
    res = f(out, ctypes.byref(dl), data, ctypes.byref(sl), ctypes.byref(st), ctypes.byref(done))
    return res, out.raw[:dl.value], done.value


def props(L):
    return L.enc2_props(1, 1 << 16, block_size=X.BLOCK)


def test_parameter_errors_come_before_the_device(L):
    """Four filters, id 2, delta 0 and 257, an ARM start offset of 2: refused on
    the host (the same verdicts with and without a device)."""
    data = X.source([])
    for chain, want in (([(X.X86, 0)] * 4, X.PARAM), ([(2, 0)], X.UNSUPPORTED),
                        ([(0x21, 0)], X.UNSUPPORTED), ([(X.DELTA, 0)], X.PARAM),
                        ([(X.DELTA, 257)], X.PARAM), ([(X.ARM, 2)], X.PARAM),
                        ([(X.IA64, 8)], X.PARAM), ([(X.ARMT, 1)], X.PARAM),
                        ([(X.PPC, 0), (X.SPARC, 6)], X.PARAM)):
        assert L.XzEncodeEx(data, props(L), 1, len(data) + 4096, chain)[0] == want, chain


def test_the_sources_are_what_the_chains_need():
    """Every filter changes its source's first block; the x86 source has one E8
    whose operand straddles the first block boundary, which a per-block restart
    leaves alone and a run over the whole buffer converts."""
    for name, chain, _ in X.CHAINS:
        if not chain:
            continue
        first = X.pieces(X.source(chain))[0]
        step = first
        for fid, prop in chain:
            nxt = X.ref_filter(fid, prop, step)
            assert nxt != step, (name, fid)
            step = nxt
    src = X.source([(X.X86, 0)])
    assert len(src) == X.SIZE and len(X.pieces(src)) == 6 and len(X.pieces(src)[-1]) == 3
    assert src[X.BLOCK - 2] == 0xE8
    whole = X.ref_filter(X.X86, 0, src)
    assert whole[X.BLOCK - 2:X.BLOCK + 3] != src[X.BLOCK - 2:X.BLOCK + 3]
    per_block = b"".join(X.ref_filter(X.X86, 0, p) for p in X.pieces(src))
    assert per_block[X.BLOCK - 2:X.BLOCK + 3] == src[X.BLOCK - 2:X.BLOCK + 3]


@pytest.mark.gpu
@pytest.mark.parametrize("name,chain,check", X.CHAINS, ids=[c[0] for c in X.CHAINS])
def test_chain(L, name, chain, check):
    data = X.source(chain)
    r, xz = L.XzEncodeEx(data, props(L), check, len(data) + 4096, chain)
    assert r == 0, L.last_error()
    # the reference's reader, liblzma and this library's reader give the source
    assert ref_xz_decode(xz, len(data) + 16) == (0, data, 1)
    assert L.XzDecode(xz, len(data)) == (0, data, -1)
    assert lzma.decompress(xz, format=lzma.FORMAT_XZ) == data
    r, blocks, total = L.xz_index(xz)
    parts = X.pieces(data)
    assert (r, total, len(blocks)) == (0, len(data), len(parts))
    csize = {0: 0, 1: 4, 4: 8, 10: 32}[check]
    at = 12
    for i, (b, piece) in enumerate(zip(blocks, parts)):
        prop, want = X.ref_block_data(X.ref_chain(chain, piece))
        header = X.block_header(chain, prop)
        assert xz[at:at + len(header)] == header, (name, i)
        assert (b.header_off, b.data_off, b.unpack_size) == (at, at + len(header), len(piece))
        assert b.num_filters == len(chain)
        assert [(b.filter_id[k], b.filter_prop[k]) for k in range(len(chain))] == chain
        assert (b.check_type, b.check_size, b.lzma2_prop) == (check, csize, prop)
        assert xz[b.data_off:b.data_off + b.pack_size] == want, (name, i)
        assert xz[b.check_off:b.check_off + csize] == X.check_value(check, piece), (name, i)
        at = b.check_off + csize
    if not chain:
        assert L.XzEncode(data, props(L), check, len(data) + 4096) == (0, xz)
    assert L.xz_compress(data, check=check, dict_size=1 << 16, block_size=X.BLOCK, chain=chain) == xz

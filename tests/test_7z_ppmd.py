"""PPMd folders in 7z archives, opt-in (LZMA_GPU_7Z_PPMD): archives built by
tests/sevenzwrite.py around the reference-encoded PPMd7 streams of
tests/golden/ppmd7_cases.json ("sevenz"), mixed with LZMA / LZMA2 / Copy
folders and one BCJ + PPMd folder, behind a packed LZMA header.

CPU: the header walk with and without the flag (an unpacked-header twin of the
archive).  GPU (-m gpu): extraction with the flag, without it, with a corrupt
pack stream and with a wrong file CRC.
"""
import importlib.util
import os
import struct
import sys

import pytest

import native
import ppmd7_golden as P
import sevenzwrite as Z

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))

M_PPMD = 0x030401
UNSUPPORTED, DATA, CRC = 4, 1, 3


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_golden_ppmd7", os.path.join(P.GOLD, "make_golden_ppmd7.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


_cache = {}


def streams():
    """name -> (packed, props, plain text as the folder's files see it)."""
    if not _cache:
        import bcj2enc
        d, gen = P.load(), _generator()
        for c in d["sevenz"]:
            if c["name"] == "bcj":
                plain = bcj2enc.x86_like(9, 6000, density=0.05)
                assert P.sha(plain) == c["unfiltered_sha256"]
                assert P.sha(Z.x86_encode(plain)) == c["sha256"]
            else:
                plain = gen.GEN[c["content"]](c["seed"], c["plain_len"])
                assert P.sha(plain) == c["sha256"]
            props = bytes([c["order"]]) + struct.pack("<I", c["mem_size"])
            _cache[c["name"]] = (P.packed(d, c), props, plain)
    return _cache


def cut(name, data, parts):
    n = len(data)
    edges = [0] + [n * k // parts + (k * 7) % 5 for k in range(1, parts)] + [n]
    return [(f"{name}{k}.txt", data[edges[k]:edges[k + 1]]) for k in range(parts)]


def build(encode_header=True, spoil_pack=None, wrong_crc=None, short_props=False):
    """Folders: LZMA, PPMd (3 files), Copy, PPMd (1 file, folder CRC), LZMA2,
    BCJ + PPMd (2 files).  Returns (archive, folders)."""
    s = streams()
    text = native.gen("text", 5, 7000)

    def ppmd(name, parts, **kw):
        packed, props, plain = s[name]
        files = cut(name, plain, parts)
        if wrong_crc == name:  # the last file's recorded CRC belongs to other bytes
            files[-1] = (files[-1][0], bytes(b ^ 0x20 for b in files[-1][1]))
        if spoil_pack == name:
            b = bytearray(packed)
            b[len(b) // 2] ^= 0x40
            packed = bytes(b)
        if short_props and name == "text":
            props = props[:4]
        return Z.Folder(files, method=M_PPMD, packed=packed, props=props, **kw)

    folders = [Z.Folder(cut("lzma", text, 2), method=Z.M_LZMA),
               ppmd("text", 3),
               Z.Folder([("copy.bin", text[:1234])], method=Z.M_COPY, crc=True),
               ppmd("letters", 1, crc=True),
               Z.Folder(cut("lzma2_", text[::-1], 3), method=Z.M_LZMA2),
               ppmd("bcj", 2, bcj=True)]
    return Z.archive(folders, encode_header=encode_header), folders


PPMD_FOLDERS = (1, 3, 5)


def test_open_follows_the_flag(L):
    arc, folders = build(encode_header=False)
    r, fo, files, _, total = L.sz_open(arc)
    assert r == 0 and len(fo) == 6
    assert [f.supported for f in fo] == [0, UNSUPPORTED, 0, UNSUPPORTED, 0, UNSUPPORTED]
    assert [f.method for f in fo] == [Z.M_LZMA, M_PPMD, 0, M_PPMD, Z.M_LZMA2, M_PPMD]
    r, fo2, files2, _, total2 = L.sz_open(arc, flags=L.SZ_PPMD)
    assert r == 0 and [f.supported for f in fo2] == [0] * 6
    assert [f.x86 for f in fo2] == [0, 0, 0, 0, 0, 1]
    assert total2 == total == sum(len(f.data) for f in folders)
    assert [f.size for f in files2] == [f.size for f in files]
    assert bytes(fo2[1].props[:5]) == folders[1].props and fo2[1].props_size == 5
    # SzDecodePpmd's own checks: props size, then order and memSize
    arc4, _ = build(encode_header=False, short_props=True)
    r, fo4, _, _, _ = L.sz_open(arc4, flags=L.SZ_PPMD)
    assert r == 0 and [f.supported for f in fo4] == [0, UNSUPPORTED, 0, 0, 0, 0]
    _, props, plain = streams()["text"]
    for bad in (bytes([1]) + props[1:], bytes([65]) + props[1:], props[:1] + struct.pack("<I", 2047),
                props[:1] + struct.pack("<I", 0xFFFFFFFF - 35)):
        a = Z.archive([Z.Folder([("a", plain)], method=M_PPMD, packed=b"\0" * 5, props=bad)])
        r, fo, _, _, _ = L.sz_open(a, flags=L.SZ_PPMD)
        assert r == 0 and fo[0].supported == UNSUPPORTED, bad.hex()
    assert L.sz_open(arc, flags=2)[0] == 5  # an unknown flag bit: SZ_ERROR_PARAM


def test_ppmd_inside_bcj2_stays_unsupported(L):
    """The one deviation from the reference's compile-time switch."""
    import bcj2enc
    data = bcj2enc.x86_like(3, 3000, density=0.05)
    plain = Z.Bcj2Folder([("x.bin", data)])
    r, fo, _, _, _ = L.sz_open(Z.archive([plain]), flags=L.SZ_PPMD)
    assert r == 0 and fo[0].supported == 0
    hdr = Z.archive([plain])
    # the same folder with its main coder's method id rewritten to PPMd's
    # (both ids are three bytes: 03 01 01 -> 03 04 01)
    at = hdr.rfind(b"\x03\x01\x01")
    assert at > 0
    import zlib
    b = bytearray(hdr)
    b[at:at + 3] = b"\x03\x04\x01"
    off, size = struct.unpack("<QQ", bytes(b[12:28]))
    h = bytes(b[32 + off:32 + off + size])
    start = struct.pack("<QQI", off, size, zlib.crc32(h))
    b[8:32] = struct.pack("<I", zlib.crc32(start)) + start
    r, fo, _, _, _ = L.sz_open(bytes(b), flags=L.SZ_PPMD)
    assert r == 0 and fo[0].supported == UNSUPPORTED


def file_bytes(files, out, i):
    return out[files[i].dst_off:files[i].dst_off + files[i].size]


def expected_files(folders):
    return [d for f in folders for _, d in f.files]


@pytest.mark.gpu
def test_gpu_extract_with_the_flag(L):
    arc, folders = build()
    r, fo, files, _, total = L.sz_open(arc, flags=L.SZ_PPMD)
    assert r == 0 and [f.supported for f in fo] == [0] * 6
    r, out, fres = L.SzExtract(arc, total, flags=L.SZ_PPMD)
    assert r == 0 and fres[:len(files)] == [0] * len(files)
    want = expected_files(folders)
    assert len(want) == len(files) == 12
    for i, w in enumerate(want):
        assert file_bytes(files, out, i) == w, i


@pytest.mark.gpu
def test_gpu_extract_without_the_flag(L):
    arc, folders = build()
    r, fo, files, _, total = L.sz_open(arc)
    assert r == 0 and [f.supported for f in fo] == [0, UNSUPPORTED, 0, UNSUPPORTED, 0, UNSUPPORTED]
    r, out, fres = L.SzExtract(arc, total)
    assert r == UNSUPPORTED
    want = expected_files(folders)
    for i, w in enumerate(want):
        if files[i].folder in PPMD_FOLDERS:
            assert fres[i] == UNSUPPORTED, i
        else:
            assert fres[i] == 0 and file_bytes(files, out, i) == w, i


@pytest.mark.gpu
def test_gpu_corrupt_pack_stream_and_wrong_crc(L):
    want = None
    for kw, folder, code in ((dict(spoil_pack="text"), 1, DATA), (dict(wrong_crc="bcj"), 5, CRC)):
        arc, folders = build(**kw)
        r, fo, files, _, total = L.sz_open(arc, flags=L.SZ_PPMD)
        assert r == 0
        r, out, fres = L.SzExtract(arc, total, flags=L.SZ_PPMD)
        assert r == code
        want = expected_files(folders)
        for i, w in enumerate(want):
            if files[i].folder != folder:
                assert fres[i] == 0 and file_bytes(files, out, i) == w, (kw, i)
            elif code == DATA:
                assert fres[i] == DATA, (kw, i)  # exactly the folder's files
            else:
                last = i + 1 == len(want) or files[i + 1].folder != folder
                assert fres[i] == (CRC if last else 0), (kw, i)

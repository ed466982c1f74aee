"""Sources, chains and the reference's side of the xz writer's filter-chain
tests (test_xzenc_filters_gpu.py).

The source is 20 KiB + 3 bytes in blocks of 4,096 (the smallest block size the
LZMA2 writer tests use), so the last block is 3 bytes.  Per block the expected
data bytes are ref_lzma2_encode of the piece after the reference's own Convert /
Delta_Encode calls (oracle/_ref/libref.so) in chain order with a fresh state."""
import ctypes
import hashlib
import json
import os
import zlib

import lzma86_cases
import native
import xzwrite

BLOCK = 4096
SIZE = 20 * 1024 + 3
DELTA, X86, PPC, IA64, ARM, ARMT, SPARC = 3, 4, 5, 6, 7, 8, 9
BRA_NAMES = {PPC: "PPC", IA64: "IA64", ARM: "ARM", ARMT: "ARMT", SPARC: "SPARC"}
OK, UNSUPPORTED, PARAM = 0, 4, 5

# (name, chain, check): every id alone, x86 from a start offset, delta 1 and 256
# (the last block is shorter than 256), three filters, none
CHAINS = [
    ("delta4", [(DELTA, 4)], 1),
    ("x86", [(X86, 0)], 1),
    ("ppc", [(PPC, 0)], 4),
    ("ia64", [(IA64, 0)], 1),
    ("arm", [(ARM, 0)], 10),
    ("armt", [(ARMT, 0)], 1),
    ("sparc", [(SPARC, 0)], 1),
    ("x86@0x1000", [(X86, 0x1000)], 1),
    ("delta1", [(DELTA, 1)], 1),
    ("delta256", [(DELTA, 256)], 1),
    ("delta4+x86+arm", [(DELTA, 4), (X86, 0), (ARM, 0)], 4),
    ("none", [], 1),
]


def _bra_words(kind):
    """Bytes the kind's Convert changes: the inputs of tests/golden/bra_cases.json
    (the patterns of test_bra.py) for the encode direction, each padded to 16."""
    with open(os.path.join(native.ROOT, "tests", "golden", "bra_cases.json")) as f:
        d = json.load(f)
    with open(os.path.join(native.ROOT, "tests", "golden", "bra_blob.bin"), "rb") as f:
        blob = f.read()
    out = bytearray()
    for c in d["bra"]:
        a, b = blob[c["in"]:c["in"] + c["len"]], blob[c["out"]:c["out"] + c["len"]]
        if c["kind"] == kind and c["encoding"] == 1 and "chain" not in c and a != b:
            out += a[:2048] + bytes(-len(a[:2048]) % 16)
    assert len(out) >= 64, kind
    return bytes(out)


_src = {}


def source(chain):
    """The chain's source: by its first branch converter, else code-like bytes;
    for delta alone a ramp with a stride of 4."""
    ids = [fid for fid, _ in chain]
    key = next((f for f in ids if f in BRA_NAMES), X86 if X86 in ids or not ids else DELTA)
    if key not in _src:
        if key == DELTA:
            b = bytes((i // 4 * 3 + (i % 4) * 64) & 0xFF for i in range(SIZE))
        elif key == X86:
            b = bytearray(lzma86_cases.code(41, SIZE))
            # one CALL whose operand straddles the first block boundary: every
            # block restarts the filter, so this one stays as it is
            b[BLOCK - 8:BLOCK + 8] = b"\x90" * 6 + b"\xE8\x10\x20\x00\x00" + b"\x90" * 5
            b = bytes(b)
        else:
            w = _bra_words(BRA_NAMES[key])
            b = (w * (SIZE // len(w) + 1))[:SIZE]
        _src[key] = b
    return _src[key]


def pieces(data):
    return [data[at:at + BLOCK] for at in range(0, len(data), BLOCK)]


def ref_filter(fid, prop, piece):
    """One filter of the reference over one block, fresh state, encode direction."""
    lib = native.ref_cont()
    buf = ctypes.create_string_buffer(bytes(piece), max(len(piece), 1))
    if fid == DELTA:
        state = ctypes.create_string_buffer(256)
        lib.Delta_Init(state)
        lib.Delta_Encode.argtypes = [ctypes.c_char_p, ctypes.c_uint, ctypes.c_char_p,
                                     ctypes.c_size_t]
        lib.Delta_Encode.restype = None
        lib.Delta_Encode(state, prop, buf, len(piece))
    elif fid == X86:
        f = lib.ref_x86_convert
        f.restype = ctypes.c_size_t
        f.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint,
                      ctypes.POINTER(ctypes.c_uint), ctypes.c_int]
        st = ctypes.c_uint(0)
        f(buf, len(piece), prop, ctypes.byref(st), 1)
    else:
        f = getattr(lib, BRA_NAMES[fid] + "_Convert")
        f.restype = ctypes.c_size_t
        f.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int]
        f(buf, len(piece), prop, 1)
    return buf.raw[:len(piece)]


def ref_chain(chain, piece):
    for fid, prop in chain:
        piece = ref_filter(fid, prop, piece)
    return piece


def ref_block_data(piece, dict_size=1 << 16):
    """ref_lzma2_encode of one (filtered) piece: its chunks and the final 0x00."""
    lib = native.ref()
    cap = len(piece) + len(piece) // 2 + 4096
    dst = ctypes.create_string_buffer(cap)
    dl = ctypes.c_size_t(cap)
    prop = ctypes.c_ubyte(0)
    res = lib.ref_lzma2_encode(dst, ctypes.byref(dl), piece, len(piece), 1, dict_size, -1, -1, -1,
                               0, ctypes.byref(prop))
    assert res == OK
    return prop.value, dst.raw[:dl.value]


def header_filters(chain):
    """The filter records of a block header as the issue words them."""
    out = bytearray()
    for fid, prop in chain:
        out.append(fid)
        if fid == DELTA:
            out += bytes([1, prop - 1])
        elif prop == 0:
            out.append(0)
        else:
            out += bytes([4]) + prop.to_bytes(4, "little")
    return bytes(out)


def block_header(chain, lzma2_prop):
    body = bytes([len(chain)]) + header_filters(chain) + bytes([0x21, 1, lzma2_prop])
    body += bytes(-(len(body) + 1) % 4)
    body = bytes([(len(body) + 1 + 4) // 4 - 1]) + body
    return body + zlib.crc32(body).to_bytes(4, "little")


def check_value(kind, piece):
    return xzwrite.check_value(kind, piece)


def sha(b):
    return hashlib.sha256(b).hexdigest()

"""LZMA2 block cases for the normal-mode encoder (the optimal parser and Bt4):
lzma2enc_cases' edge list moved to level 5, the mixed pieces that exercise the
state restore in front of rebuilt price tables, and a seeded random list.
Cases, records and the reference access are lzma2enc_cases' (ref_lzma2_encode
takes the level); only the emulator differs, which has to be told which modes
are allowed.  Goldens: tests/golden/lzmaenc_opt_cases.json, key "lzma2"."""
import ctypes
import os
import random
import struct
import subprocess

import lzma2enc_cases as C2
import native

EMU_SRC = os.path.join(native.ROOT, "tests", "emu_lzmaenc_opt", "lzma2enc_opt_emu.cpp")
ALL_MODES = 3
case, key, data_of, check_block, block_bound = (C2.case, C2.key, C2.data_of, C2.check_block,
                                                C2.block_bound)

# a stored chunk, then the restore, then compressed chunks
MIXED_CASE = case([("random", 61, 70 * 1024), ("text", 62, 30 * 1024)], level=5)
# one piece of text long enough for two compressed chunks
TWO_CHUNK_CASE = case([("text", 63, 400000)], level=5)


# one buffer cut into blocks of BLOCK bytes (LzmaGpu_Lzma2EncodeHost,
# LzmaGpu_XzEncode, a 7z LZMA2 folder): the concatenation of these pieces, so
# that every block is a case of its own with a golden of its own
BLOCK = 20000
PIECES = [case([("text", 70, BLOCK)], level=5), case([("runs", 71, BLOCK)], level=5),
          case([("random", 72, 9000)], level=5)]


def edge_cases():
    out, seen = [], set()
    for c in C2.edge_cases():
        c = dict(c, level=5)
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    out += [MIXED_CASE, TWO_CHUNK_CASE]
    out.append(case([("text", 64, 30000), ("runs", 65, 9000)], level=7))
    out.append(case([("text", 66, 9000)], level=5, dict=5000))      # not a power of two
    return out


def random_cases(count, seed, max_n=None):
    rng = random.Random(seed)
    out = []
    for c in C2.random_cases(count, seed, max_n):
        out.append(dict(c, level=rng.randrange(5, 10),
                        dict=rng.choice((4096, 5000, 1 << 16, 1 << 16, C2.MIB))))
    return out


def golden_cases():
    return edge_cases() + PIECES + random_cases(40, 20262, 200 * 1024)


def expect(c, data=None, golden=None):
    if native.have_ref():
        return C2.expect(c, data)
    if golden is None:
        import lzmaenc_opt_cases
        golden = lzmaenc_opt_cases.load_golden()
    return dict(golden["lzma2_by_key"][key(c)], out=None)


def build_emu(out_dir, extra=(), main=False, name=None):
    out = os.path.join(str(out_dir),
                       name or ("lzma2enc_opt_emu_main" if main else "liblzma2enc_opt_emu.so"))
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", C2.CSRC]
    cmd += (["-DLZMA2ENC_OPT_EMU_MAIN"] if main else ["-fPIC", "-shared"])
    cmd += list(extra) if extra else ["-O2"]
    subprocess.run(cmd + [EMU_SRC, "-o", out], check=True)
    return out


def load_emu(so):
    lib = ctypes.CDLL(so)
    f = lib.lzma2enc_opt_emu_encode
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int,
                  ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
                  ctypes.c_int, ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_uint64)]
    lib.lzma2enc_opt_emu_slice_bytes.restype = None
    lib.lzma2enc_opt_emu_slice_bytes.argtypes = [ctypes.c_uint32] * 6 + [
        ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    return lib


def emu_encode(lib, data, c, cap, poison=0x3C, allowed=ALL_MODES):
    """(res, dest_len, prop, dst[:dest_len]); asserts the guard behind cap."""
    dst = ctypes.create_string_buffer(b"\xEE" * (cap + 8), cap + 8)
    prop = ctypes.c_ubyte(0)
    dl = ctypes.c_uint64(0)
    res = lib.lzma2enc_opt_emu_encode(data, len(data), dst, cap, c["level"], c["dict"], c["lc"],
                                      c["lp"], c["pb"], allowed, poison, ctypes.byref(prop),
                                      ctypes.byref(dl))
    assert dst.raw[cap:] == b"\xEE" * 8, "write past dst_cap"
    assert dl.value <= cap
    return res, dl.value, prop.value, dst.raw[:dl.value]


def write_case_file(path, cases, golden=None):
    """Records for the stand-alone build of lzma2enc_opt_emu.cpp, each with
    dst_cap = the block bound."""
    lib = None
    with open(path, "wb") as f:
        for c in cases:
            data = data_of(c)
            want = expect(c, data, golden)
            cap = block_bound(len(data))
            out = want["out"]
            if want["res"] != C2.OK:
                out = b""
            elif out is None:
                if lib is None:
                    lib = load_emu(build_emu(os.path.dirname(path),
                                             name="liblzma2enc_opt_emu_dump.so"))
                got = emu_encode(lib, data, c, cap)
                check_block(got, want, key(c))
                out = got[3]
            else:
                out = out[:-1]
            f.write(struct.pack("<iIiiiI", c["level"], c["dict"], c["lc"], c["lp"], c["pb"],
                                ALL_MODES))
            f.write(struct.pack("<QQiQ", len(data), cap, want["res"], len(out)))
            f.write(data + out)

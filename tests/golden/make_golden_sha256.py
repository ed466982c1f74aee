"""Generate tests/golden/sha256_cases.json from the REFERENCE SHA-256 (Sha256.c).

Run in the build container only (needs oracle/_ref/libref.so from
`make -f oracle/Makefile.ref`, which compiles Sha256.c in place):

    python tests/golden/make_golden_sha256.py

Each case is a sequence of Sha256_Update sizes over a deterministic message
(`pattern(seed, n)` below, or explicit hex).  After Sha256_Init and after every
Sha256_Update the reference's struct is read back.  Recorded per case:

  states   the eight state words (hex, as 32 little-endian bytes), run-length
           coded: [call, hex] where call 0 is Sha256_Init and call k the k-th
           update; a state holds until the next entry
  trace    sha256 over the concatenation, call by call, of
           state || count (8 bytes LE) || buffer[0 .. count & 63)
           -- the part of the struct the reference defines
  digest   what Sha256_Final wrote
  final    the same struct read-back after Sha256_Final (it re-initialises)

count and the buffer prefix follow from the sizes and the message (count = the
bytes fed so far, prefix = the last count & 63 of them); the generator asserts
that the reference holds exactly those, so a test can rebuild them.
"""
import ctypes
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import native  # noqa: E402

FIPS_56 = b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq"

SEQUENCES = [
    {"sizes": []},
    {"sizes": [0]},
    {"sizes": [3], "hex": b"abc".hex()},
    {"sizes": [56], "hex": FIPS_56.hex()},
    {"sizes": [1, 63, 64, 1]},
    {"sizes": [55]},
    {"sizes": [56]},
    {"sizes": [64]},
    {"sizes": [65]},
    {"sizes": [100, 100, 100]},
    {"sizes": [1] * 1000},
    {"sizes": [7, 10000]},
    {"sizes": [63, 1]},
    {"sizes": [63, 2]},
    {"sizes": [64, 64]},
    {"sizes": [128]},
    {"sizes": [119]},
    {"sizes": [120]},
    {"sizes": [0, 5, 0, 59, 0]},
    {"sizes": [4096, 4095, 1]},
    {"sizes": [1, 4096 + 63]},
    {"sizes": [100000]},
]


def pattern(seed, n):
    """The message of a case without explicit hex."""
    return bytes((i * 131 + (i >> 8) * 29 + seed * 7 + 1) & 0xFF for i in range(n))


def message(case, k):
    if "hex" in case:
        return bytes.fromhex(case["hex"])
    return pattern(k, sum(case["sizes"]))


class CSha256(ctypes.Structure):
    _fields_ = [("state", ctypes.c_uint32 * 8), ("count", ctypes.c_uint64),
                ("buffer", ctypes.c_ubyte * 64)]


def defined_part(p):
    return (struct.pack("<8I", *p.state) + struct.pack("<Q", p.count)
            + bytes(p.buffer[:p.count & 63]))


def main():
    lib = native.ref_cont()
    for f in (lib.Sha256_Init, lib.Sha256_Update, lib.Sha256_Final):
        f.restype = None
    lib.Sha256_Update.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    lib.Sha256_Final.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    cases = []
    for k, seq in enumerate(SEQUENCES):
        case = dict(seq)
        msg = message(case, k)
        p = CSha256()
        lib.Sha256_Init(ctypes.byref(p))
        states, trace, fed = [], hashlib.sha256(), 0

        def snap(call):
            st = struct.pack("<8I", *p.state).hex()
            if not states or states[-1][1] != st:
                states.append([call, st])
            assert p.count == fed
            assert bytes(p.buffer[:fed & 63]) == msg[fed - (fed & 63):fed]
            trace.update(defined_part(p))

        snap(0)
        for call, n in enumerate(case["sizes"], 1):
            lib.Sha256_Update(ctypes.byref(p), msg[fed:fed + n], n)
            fed += n
            snap(call)
        dig = ctypes.create_string_buffer(32)
        lib.Sha256_Final(ctypes.byref(p), dig)
        assert dig.raw == hashlib.sha256(msg).digest()
        if len(set(case["sizes"])) == 1 and len(case["sizes"]) > 8:
            case["sizes"] = {"repeat": [case["sizes"][0], len(case["sizes"])]}
        case.update(seed=k, states=states, trace=trace.hexdigest(), digest=dig.raw.hex(),
                    final=defined_part(p).hex())
        cases.append(case)
    with open(os.path.join(HERE, "sha256_cases.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_sha256.py",
                   "reference": "LZMA SDK 9.20 Sha256.c Sha256_Init / Sha256_Update / "
                                "Sha256_Final (oracle/Makefile.ref)",
                   "cases": cases}, f, indent=0)
    print(f"{len(cases)} SHA-256 update sequences")


if __name__ == "__main__":
    main()

"""Fused tree walks (LZGPU_FUSE, lzma_device.h) on the CPU: the host build of
the per-lane code with every fusion bit alone, all of them and none, in each
placement where the fusions compile (the throughput placement with per-lane
and lane-interleaved global rows, and two A/B placements of it), and in the
instantiations the gate keeps on the old path (one-stream, cooperative,
latency), against the golden vectors and the oracle.

A fusion moves where a lane's decision is issued, never which decisions the
lane makes: every result row and every output byte must equal the oracle's."""
import ctypes
import lzma
import os
import random
import subprocess
import tempfile

import pytest

import golden_cases as G
import native
from test_emu import run_batch

# every bit alone (4, the rep chain, compiles to nothing), all of them, none
FUSE_VALUES = [0, 1, 2, 4, 8, 15]
PLACEMENTS = {
    "default": "",
    "interleaved": "-DEMU_ILV",
    "all_global": "-DLZGPU_LDS_MASK=0",
    "hot_only_lds": "-DLZGPU_LDS_MASK=0x107",
}
VARIANTS = {f"{p}_fuse{v}": f"{pf} -DLZGPU_FUSE={v}"
            for p, pf in PLACEMENTS.items() for v in FUSE_VALUES}
# the emulation is one lane wide: a lane enters the fused literal walk on its
# own only for a matched literal.  LZGPU_FUSE_EMU_ALL sends every literal
# through it, as a plain-literal lane beside a matched one goes on the GPU.
VARIANTS["default_fuse15_all_literals"] = "-DLZGPU_FUSE=15 -DLZGPU_FUSE_EMU_ALL=1"
VARIANTS["interleaved_fuse15_all_literals"] = "-DEMU_ILV -DLZGPU_FUSE=15 -DLZGPU_FUSE_EMU_ALL=1"
# gated off: every lane of these kernels agrees (or the placement was not
# measured); all bits requested, the old path must be taken and stay exact
VARIANTS["gated_dup_fuse15"] = "-DEMU_DUP -DLZGPU_FUSE=15"
VARIANTS["gated_coop_fuse15"] = "-DEMU_COOP -DLZGPU_FUSE=15"
VARIANTS["gated_latency_fuse15"] = "-DEMU_LAT_MASK -DLZGPU_FUSE=15"


@pytest.fixture(scope="module", params=sorted(VARIANTS))
def emu(request):
    vdir = os.path.join(tempfile.gettempdir(), "lzgpu_emu_variants")
    os.makedirs(vdir, exist_ok=True)
    out = os.path.join(vdir, f"liblane_emu_fuse_{request.param}.{os.getpid()}.so")
    subprocess.run(["make", "-s", "-f", "tests/emu/Makefile", f"EMU_OUT={out}",
                    f"EMU_FLAGS={VARIANTS[request.param]}"], cwd=native.ROOT, check=True)
    lib = ctypes.CDLL(out)
    lib.emu_decode_batch_lds.restype = None
    lib.emu_decode_batch_lds.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_uint32]
    lib.emu_decode_batch.restype = None
    lib.emu_decode_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_fuse_emu_golden_lzma(emu):
    d = G.load()
    items, srcs, off, doff = [], [], 0, 0
    cs = G.cases("lzma")
    for i, c in cs:
        s = G.case_input(d, c)
        items.append(dict(src_off=off, src_len=len(s), dst_off=doff, dst_cap=c["dest_cap"],
                          props=bytes.fromhex(c["props"]), finish=c["finish"]))
        srcs.append(s)
        off += len(s)
        doff += c["dest_cap"]
    res, dst = run_batch(emu, items, b"".join(srcs) + b"\0" * 16, True)
    bad = []
    for k, (i, c) in enumerate(cs):
        e = c["expect"]
        got = (res[k].res, res[k].status, res[k].dest_len, res[k].src_len)
        out = dst[items[k]["dst_off"]:items[k]["dst_off"] + res[k].dest_len]
        if got != (e["res"], e["status"], e["dest_len"], e["src_len"]) or G.sha(out) != e["sha256"]:
            bad.append((i, c["note"], got, (e["res"], e["status"], e["dest_len"], e["src_len"])))
    assert not bad, bad[:10]


def test_fuse_emu_handmade_set(emu):
    """The hand-made streams (tests/handmade_cases.py) through every fusion
    build, against the reference's answers."""
    import handmade_cases as H
    its = H.items()
    descs, src, _ = H.batch(its)
    res, dst = run_batch(emu, descs, src, True)
    bad = H.mismatches(its, descs, res, dst)
    assert not bad, (len(bad), bad[:8])


_FUZZ = None


def fuzz_set():
    """Seeded streams with their oracle results, computed once for every build:
    whole, bit-flipped and truncated inputs, exact / short / long capacities,
    both finish modes (FINISH_ANY with a short capacity stops inside a match)."""
    global _FUZZ
    if _FUZZ is not None:
        return _FUZZ
    rng = random.Random(1907)
    orc = native.oracle()
    items, srcs, exp, off, doff = [], [], [], 0, 0
    for it in range(400):
        lc, pb = rng.choice([0, 0, 3, 4]), rng.choice([0, 0, 2, 4])
        dsz = rng.choice([4096, 1 << 16, 1 << 22])
        n = rng.choice([1, 2, 60, 700, 2048, 4096, 9000])
        data = native.gen(rng.choice(["text", "text", "random", "runs"]), 77_000 + it, n)
        f = [{"id": lzma.FILTER_LZMA1, "dict_size": dsz, "lc": lc, "lp": 0, "pb": pb,
              "preset": rng.choice([1, 6])}]
        comp = bytearray(lzma.compress(data, format=lzma.FORMAT_RAW, filters=f))
        props = bytes([pb * 5 * 9 + lc]) + dsz.to_bytes(4, "little")
        mode = rng.randrange(5)
        if mode == 1 and len(comp) > 6:
            comp[rng.randrange(5, len(comp))] ^= 1 << rng.randrange(8)
        elif mode == 2:
            comp = comp[:rng.randrange(len(comp) + 1)]
        cap = max(0, n + rng.choice([0, 0, 1, -1, 50, -50, -300]))
        fin = rng.randrange(2)
        comp = bytes(comp)
        items.append(dict(src_off=off, src_len=len(comp), dst_off=doff, dst_cap=cap, props=props,
                          finish=fin))
        srcs.append(comp)
        exp.append(native.decode(orc, "orc", comp, props, cap, fin))
        off += len(comp)
        doff += cap
    _FUZZ = (items, b"".join(srcs) + b"\0" * 16, exp)
    return _FUZZ


def test_fuse_emu_fuzz_vs_oracle(emu):
    items, src, exp = fuzz_set()
    res, dst = run_batch(emu, items, src, True)
    for k in range(len(items)):
        got = (res[k].res, res[k].status, res[k].dest_len, res[k].src_len)
        out = dst[items[k]["dst_off"]:items[k]["dst_off"] + res[k].dest_len]
        assert got == exp[k][:4] and out == exp[k][4], (k, got, exp[k][:4])

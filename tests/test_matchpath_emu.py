"""The match path's load batches (LZGPU_MP, lzma_device.h) on the CPU: the host
build of the per-lane code in the throughput placement, per-lane and
lane-interleaved global rows, with LZGPU_MP = 0, every bit alone and the
shipped mask, against the oracle over the match-path inputs
(tests/matchpath_cases.py), the hand-made streams and seeded fuzz streams.

A batch moves a load ahead of decisions that cannot store to its cells, never
a decision: every result row and every output byte must equal the oracle's.

tests/emu_matchpath/mp_emu.cpp is the same code as a stand-alone program built
with -fsanitize=address,undefined and run as a program (nothing sanitized is
loaded into this process): every table, row area and input has its exact size,
so a batch that reads outside them is a report."""
import ctypes
import os
import struct
import subprocess
import tempfile

import pytest

import matchpath_cases as C
import native
from test_emu import run_batch
from test_fuse_emu import fuzz_set

SHIPPED = 7
MP_VALUES = [0, 1, 2, 4, SHIPPED]
VARIANTS = {f"{p}_mp{v}": f"{pf} -DLZGPU_MP={v}"
            for p, pf in (("default", ""), ("interleaved", "-DEMU_ILV")) for v in MP_VALUES}
# the batches with F1's and F2's walks compiled out, and in kernels the gate
# keeps on the old path
VARIANTS["default_mp7_fuse0"] = f"-DLZGPU_MP={SHIPPED} -DLZGPU_FUSE=0"
VARIANTS["gated_dup_mp7"] = f"-DEMU_DUP -DLZGPU_MP={SHIPPED}"
VARIANTS["gated_coop_mp7"] = f"-DEMU_COOP -DLZGPU_MP={SHIPPED}"
VARIANTS["gated_latency_mp7"] = f"-DEMU_LAT_MASK -DLZGPU_MP={SHIPPED}"


@pytest.fixture(scope="module", params=sorted(VARIANTS))
def emu(request):
    vdir = os.path.join(tempfile.gettempdir(), "lzgpu_emu_variants")
    os.makedirs(vdir, exist_ok=True)
    out = os.path.join(vdir, f"liblane_emu_mp_{request.param}.{os.getpid()}.so")
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


def _bad_rows(items, exp, rows, dst):
    bad = []
    for k, e in enumerate(exp):
        got = tuple(rows[k])
        out = dst[items[k]["dst_off"]:items[k]["dst_off"] + got[2]]
        if got != tuple(e[:4]) or out != e[4]:
            bad.append((k, got, tuple(e[:4])))
    return bad


@pytest.mark.parametrize("props", [(0, 0), (3, 2)])
def test_inputs_hold_every_class(props):
    """The conditions on the inputs, in stream order (the GPU test asserts the
    pairs again in the planner's lane order)."""
    items, src, dst_bytes, exp, syms, in_lens = C.batch(props[0], props[1], 64)
    have, pairs = C.coverage(syms, in_lens, list(range(64)))
    assert C.WANT <= have, sorted(C.WANT - have, key=str)
    assert C.WANT_PAIRS <= pairs, sorted(C.WANT_PAIRS - pairs)
    C.batch(props[0], props[1], 33)


@pytest.mark.parametrize("props", [(0, 0), (3, 2)])
def test_matchpath_emu_inputs_vs_oracle(emu, props):
    items, src, dst_bytes, exp, syms, in_lens = C.batch(props[0], props[1], 64)
    res, dst = run_batch(emu, items, src, True)
    rows = [(r.res, r.status, r.dest_len, r.src_len) for r in res]
    bad = _bad_rows(items, exp, rows, dst)
    assert not bad, (len(bad), bad[:8])


def test_matchpath_emu_handmade_set(emu):
    import handmade_cases as H
    its = H.items()
    descs, src, _ = H.batch(its)
    res, dst = run_batch(emu, descs, src, True)
    bad = H.mismatches(its, descs, res, dst)
    assert not bad, (len(bad), bad[:8])


def test_matchpath_emu_fuzz_vs_oracle(emu):
    items, src, exp = fuzz_set()
    res, dst = run_batch(emu, items, src, True)
    rows = [(r.res, r.status, r.dest_len, r.src_len) for r in res]
    bad = _bad_rows(items, exp, rows, dst)
    assert not bad, (len(bad), bad[:8])


# ------------------------------------------------------------------ sanitizer program

SRC = os.path.join(native.ROOT, "tests", "emu_matchpath", "mp_emu.cpp")
BUILDS = {f"{p}_mp{v}": f"{pf} -DLZGPU_MP={v}".split()
          for p, pf in (("default", ""), ("interleaved", "-DEMU_ILV")) for v in (0, SHIPPED)}
_DIR = os.path.join(tempfile.gettempdir(), "lzgpu_mp_emu")


@pytest.fixture(scope="module")
def exes():
    """Every sanitizer build, compiled side by side."""
    os.makedirs(_DIR, exist_ok=True)
    jobs = {}
    for name, flags in BUILDS.items():
        exe = os.path.join(_DIR, f"mp_emu_{name}.{os.getpid()}")
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-Wno-unused-function",
               "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRC]
        jobs[name] = (exe, subprocess.Popen(cmd, cwd=native.ROOT))
    out = {}
    for name, (exe, p) in jobs.items():
        assert p.wait() == 0, name
        out[name] = exe
    return out


_JOBS = {}


def _job(props):
    """The match-path inputs of one props pair plus the fuzz streams the
    planner puts on the LDS kernel, as the program's job file."""
    if props in _JOBS:
        return _JOBS[props]
    import lzmagpu as L
    items, src, dst_bytes, exp, syms, in_lens = C.batch(props[0], props[1], 64)
    items, src, exp = list(items), src[:-16], list(exp)
    if props == (0, 0):
        f_items, f_src, f_exp = fuzz_set()
        descs = L.make_descs(f_items)
        order = (ctypes.c_uint32 * len(f_items))()
        plan = L.Plan()
        assert L.lib.LzmaGpu_PlanBatchEx(descs, len(f_items), order, ctypes.byref(plan)) == 0
        keep = sorted(order[k] for k in range(plan.n_lds))
        assert len(keep) >= 200, len(keep)
        for i in keep:
            it = dict(f_items[i])
            it["src_off"] += len(src)
            it["dst_off"] += dst_bytes
            items.append(it)
            exp.append(f_exp[i])
        src += f_src[:-16]
        dst_bytes += max(it["dst_off"] + it["dst_cap"] for it in f_items)
    descs = L.make_descs(items)
    n = len(items)
    order = (ctypes.c_uint32 * n)()
    plan = L.Plan()
    assert L.lib.LzmaGpu_PlanBatchEx(descs, n, order, ctypes.byref(plan)) == 0
    assert plan.n_lds == n, (plan.n_lds, n)
    stride = 0
    for i in range(n):
        pr = bytes(descs[i].props)
        lc, lp, pb = pr[0] % 9, (pr[0] // 9) % 5, pr[0] // 45
        stride = max(stride, (56 << pb) + 950 + (768 << (lc + lp)))
    stride = (stride + 3) // 4 * 4
    blob = struct.pack("<5Q", n, len(src), dst_bytes, max(plan.workspace_bytes, 16), stride)
    blob += b"".join(bytes(descs[i]) for i in range(n)) + src
    path = os.path.join(_DIR, f"job_{props[0]}_{props[1]}.{os.getpid()}.bin")
    with open(path, "wb") as f:
        f.write(blob)
    _JOBS[props] = (path, items, exp, dst_bytes)
    return _JOBS[props]


@pytest.mark.parametrize("props", [(0, 0), (3, 2)])
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_sanitizer_program_vs_oracle(exes, build, props):
    path, items, exp, dst_bytes = _job(props)
    out = os.path.join(_DIR, f"out_{build}_{props[0]}.{os.getpid()}.bin")
    r = subprocess.run([exes[build], path, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("lanes ok"), (r.stdout, r.stderr[-3000:])
    assert r.stdout.strip().endswith("LZGPU_MP %s" % build.rsplit("mp", 1)[1]), r.stdout
    with open(out, "rb") as f:
        raw = f.read()
    os.unlink(out)
    n = len(items)
    assert len(raw) == 32 * n + dst_bytes
    rows = [struct.unpack_from("<4q", raw, 32 * k) for k in range(n)]
    bad = _bad_rows(items, exp, rows, raw[32 * n:])
    assert not bad, (build, len(bad), bad[:8])

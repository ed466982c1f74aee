"""The throughput placement's input reader (GlobalReaderP, lzma_device.h) on the
CPU.

tests/emu_reader/reader_emu.cpp is a stand-alone program on the host build of
the per-lane code, compiled with -fsanitize=address,undefined and run as a
program (nothing is loaded into this process):

  readers  both checkpoint readers against a byte cursor for every start
           alignment 0..15 and every avail 0..80, the input in a heap buffer
           that ends with its last valid 16-byte block (an over-read is an
           AddressSanitizer report);
  lanes    the lane emulation of the throughput placement over the golden
           LZMA streams.  The reader (LZGPU_READER) is a compile-time switch,
           so the program is built once per reader -- and once more each with
           every literal sent through the fused walk -- and every build's
           result rows and output bytes must equal the golden vectors', hence
           each other.  (The late literal store the same work measured lost its
           A/B and is not in the tree: DESIGN.md section 4, round 8.)"""
import ctypes
import os
import struct
import subprocess
import tempfile

import pytest

import golden_cases as G
import native

SRC = os.path.join(native.ROOT, "tests", "emu_reader", "reader_emu.cpp")
BUILDS = {
    "q": "-DLZGPU_READER=0",
    "p": "-DLZGPU_READER=1",
    # the emulation is one lane wide: LZGPU_FUSE_EMU_ALL sends plain literals
    # through the fused walk too, as beside a matched-literal lane on the GPU
    "q_all_literals": "-DLZGPU_READER=0 -DLZGPU_FUSE_EMU_ALL=1",
    "p_all_literals": "-DLZGPU_READER=1 -DLZGPU_FUSE_EMU_ALL=1",
}
_DIR = os.path.join(tempfile.gettempdir(), "lzgpu_reader_emu")


def _build(name):
    os.makedirs(_DIR, exist_ok=True)
    exe = os.path.join(_DIR, f"reader_emu_{name}.{os.getpid()}")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-Wno-unused-function",
           "-Wno-unknown-pragmas"] + BUILDS[name].split() + ["-o", exe, SRC]
    return exe, subprocess.Popen(cmd, cwd=native.ROOT)


@pytest.fixture(scope="module")
def exes():
    """Every build, compiled side by side."""
    jobs = {n: _build(n) for n in BUILDS}
    out = {}
    for n, (exe, p) in jobs.items():
        assert p.wait() == 0, n
        out[n] = exe
    return out


def _run(args):
    return subprocess.run(args, capture_output=True, text=True, timeout=120)


def test_readers_against_byte_cursor(exes):
    r = _run([exes["p"], "readers"])
    assert r.returncode == 0 and r.stdout.strip() == "readers ok", (r.stdout, r.stderr[-3000:])


_JOB = {}


def golden_job():
    """The golden LZMA cases the planner puts on the LDS kernel, as the
    program's job file: (path, cases, descriptors' items)."""
    if _JOB:
        return _JOB["v"]
    import lzmagpu as L
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
    # (no padding behind the last input: the program's buffer ends with it)
    src = b"".join(srcs)
    descs = L.make_descs(items)
    n = len(items)
    order = (ctypes.c_uint32 * n)()
    plan = L.Plan()
    assert L.lib.LzmaGpu_PlanBatchEx(descs, n, order, ctypes.byref(plan)) == 0
    keep = sorted(order[k] for k in range(plan.n_lds))
    assert len(keep) >= 50, len(keep)
    stride = 0
    for i in keep:
        pr = bytes(descs[i].props)
        lc, lp, pb = pr[0] % 9, (pr[0] // 9) % 5, pr[0] // 45
        stride = max(stride, (56 << pb) + 950 + (768 << (lc + lp)))
    stride = (stride + 3) // 4 * 4
    assert ctypes.sizeof(L.StreamDesc) == 48
    blob = struct.pack("<5Q", len(keep), len(src), doff, max(plan.workspace_bytes, 16), stride)
    blob += b"".join(bytes(descs[i]) for i in keep) + src
    os.makedirs(_DIR, exist_ok=True)
    path = os.path.join(_DIR, f"job.{os.getpid()}.bin")
    with open(path, "wb") as f:
        f.write(blob)
    _JOB["v"] = (path, [cs[i] for i in keep], [items[i] for i in keep], doff)
    return _JOB["v"]


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_lanes_golden_equal_in_every_build(exes, build):
    path, cs, items, dst_bytes = golden_job()
    out = os.path.join(_DIR, f"out_{build}.{os.getpid()}.bin")
    r = _run([exes[build], "lanes", path, out])
    assert r.returncode == 0 and r.stdout.startswith("lanes ok"), (r.stdout, r.stderr[-3000:])
    assert ("reader 1" if build.startswith("p") else "reader 0") in r.stdout, r.stdout
    with open(out, "rb") as f:
        raw = f.read()
    os.unlink(out)
    n = len(cs)
    assert len(raw) == 32 * n + dst_bytes
    dst = raw[32 * n:]
    bad = []
    for k, (i, c) in enumerate(cs):
        e = c["expect"]
        got = struct.unpack_from("<4q", raw, 32 * k)
        o = dst[items[k]["dst_off"]:items[k]["dst_off"] + got[2]]
        if got != (e["res"], e["status"], e["dest_len"], e["src_len"]) or G.sha(o) != e["sha256"]:
            bad.append((i, c["note"], got, (e["res"], e["status"], e["dest_len"], e["src_len"])))
    assert not bad, (build, len(bad), bad[:8])

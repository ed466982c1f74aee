"""Throughput of Ppmd7Gpu_DecodeBatch (its own script; bench.py measures the
LZMA flagship and is not involved).

Golden PPMd7 streams (tests/golden/ppmd7_cases.json: the order-6 and order-8
text cases at their own model sizes, and the order-6 text re-encoded at 16 MiB,
7-Zip's usual setting) are replicated into batches of 64, 1,024 and 4,096
streams, every copy with its own input bytes, output range and workspace slice.
Timing: HIP events around the launch alone, after a warm-up launch, best of
--reps; every copy's result and bytes are verified after the timed region.
Replicated inputs flatter the source side: the copies' packed bytes are equal,
their reads fall in step and hit the same few cache lines' worth of patterns,
and all streams end together, so no tail of long streams is seen.

Beside each GPU line: the reference's own decoder (oracle/_ref/libref.so, its
exported Ppmd7_* functions looked up at run time by csrc/ppmd7_cpu_bench.c) on
1 and 16 host threads over the same copies.  One JSON line per measurement,
appended to --out (default profiles/ppmd7/bench.jsonl).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(ROOT, "tests", "golden")
LIBREF = os.path.join(ROOT, "oracle", "_ref", "libref.so")
CPU_SRC = os.path.join(HERE, "csrc", "ppmd7_cpu_bench.c")
CPU_EXE = os.path.join(HERE, "lib", "ppmd7_cpu_bench")


def load_cases():
    with open(os.path.join(GOLD, "ppmd7_cases.json")) as f:
        d = json.load(f)
    with open(os.path.join(GOLD, d["blob"]), "rb") as f:
        blob = f.read()
    pick = [c for c in d["cases"] if c["content"] == "word soup" and c["order"] in (6, 8)]
    pick += d["bench"]
    return [(c, blob[c["off"]:c["off"] + c["len"]]) for c in pick]


def build_cpu():
    if (not os.path.exists(CPU_EXE)
            or os.path.getmtime(CPU_EXE) < os.path.getmtime(CPU_SRC)):
        os.makedirs(os.path.dirname(CPU_EXE), exist_ok=True)
        subprocess.run(["gcc", "-O2", "-o", CPU_EXE, CPU_SRC, "-ldl", "-pthread"], check=True)
    return CPU_EXE


def cpu_leg(c, packed, copies, threads, reps):
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "packed"), os.path.join(tmp, "plain")
        with open(src, "wb") as f:
            f.write(packed)
        r = subprocess.run([build_cpu(), LIBREF, src, str(c["order"]), str(c["mem_size"]),
                            str(c["plain_len"]), str(copies), str(threads), str(reps), out],
                           check=True, capture_output=True, text=True)
        with open(out, "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == c["sha256"]
    return float(r.stdout.split()[0])


def gpu_leg(L, torch, np, c, packed, copies, reps):
    slice_bytes = L.ppmd7_workspace_bytes(c["mem_size"])
    free_b, _ = torch.cuda.mem_get_info()
    if slice_bytes * copies > free_b * 0.8:
        return None
    n = c["plain_len"]
    stride_src = (len(packed) + 15) & ~15
    descs = [dict(src_off=k * stride_src, src_len=len(packed), dst_off=k * n, dst_len=n,
                  order=c["order"], mem_size=c["mem_size"], ws_off=k * slice_bytes)
             for k in range(copies)]
    one = np.zeros(stride_src, dtype=np.uint8)
    one[:len(packed)] = np.frombuffer(packed, dtype=np.uint8)
    d_src = torch.from_numpy(np.tile(one, copies)).cuda()
    d_desc = torch.from_numpy(np.frombuffer(bytes(L.ppmd7_make_descs(descs)),
                                            dtype=np.uint8).copy()).cuda()
    d_dst = torch.zeros((copies * n,), dtype=torch.uint8, device="cuda")
    d_ws = torch.empty((slice_bytes * copies,), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((copies * 24,), dtype=torch.uint8, device="cuda")

    def launch():
        r = L.ppmd7_decode_batch_device(d_desc.data_ptr(), copies, d_src.data_ptr(),
                                        d_dst.data_ptr(), d_ws.data_ptr(), d_res.data_ptr())
        assert r == 0, L.last_error()

    launch()  # warm-up (code object load, first touch of the workspace)
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        d_dst.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None or ms < best else best
    # verification, after the timed region: every copy's result and bytes
    res = (L.Ppmd7Result * copies).from_buffer_copy(d_res.cpu().numpy().tobytes())
    assert all((q.res, q.dest_len, q.src_len) == (0, n, len(packed)) for q in res)
    rows = d_dst.view(copies, n)
    assert bool((rows == rows[0]).all())
    assert hashlib.sha256(rows[0].cpu().numpy().tobytes()).hexdigest() == c["sha256"]
    return best / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppmd7", "bench.jsonl"))
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, HERE)
    import lzmagpu as L
    if L.device_count() <= 0:
        raise SystemExit("ppmd7_bench: no HIP device: " + L.last_error())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as out:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        for c, packed in load_cases():
            tag = dict(order=c["order"], mem_size=c["mem_size"], plain_len=c["plain_len"],
                       packed_len=len(packed))
            for copies in (int(x) for x in a.batches.split(",")):
                mb = copies * c["plain_len"] / 1e6
                s = gpu_leg(L, torch, np, c, packed, copies, a.reps)
                if s is None:
                    emit(dict(tag, leg="gpu", batch=copies, skipped="workspace does not fit"))
                else:
                    emit(dict(tag, leg="gpu", batch=copies, seconds=round(s, 6),
                              mb_per_s=round(mb / s, 2)))
                if a.no_cpu or not os.path.exists(LIBREF):
                    continue
                for threads in (1, 16):
                    # the 1-thread leg decodes at most 64 copies: its rate does not depend on more
                    k = min(copies, 64) if threads == 1 else copies
                    s = cpu_leg(c, packed, k, threads, 1 if k > 256 else 2)
                    emit(dict(tag, leg="cpu_ref", batch=k, threads=threads, seconds=round(s, 6),
                              mb_per_s=round(k * c["plain_len"] / 1e6 / s, 2)))


if __name__ == "__main__":
    main()

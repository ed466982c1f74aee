"""Throughput of LzmaEncGpu_EncodeBatch (its own script; bench.py measures the
LZMA decode flagship and is not involved).

Level 1 with default props (64 KiB dictionary, lc3 lp0 pb2, fb 32, mc 16), or
--level N (5 and up: the optimal parser and Bt4, with the modes switched on for
the run and, unless --dict is given, a dictionary of the stream's size, since
the hash is sized by the dictionary) on
the synthetic generator's English-like text (csrc/synth.c), every stream with
its own seed: replicas would flatter the hash and L2 behaviour.  Shapes:
64 / 1,024 / 4,096 / 65,536 streams of 4 KiB, 4,096 of 64 KiB, one of 1 MiB.

Timing: HIP events around the device-pointer call (hash clear + encode), after
a warm-up call, best of --reps; the hash-clear launch is also timed alone, the
same way.  After the timed region every result is checked for SZ_OK and a
sample of streams is compared byte for byte with the reference's LzmaEncode
(oracle/_ref/libref_lzma.so, ref_lzma_encode).

Baseline: the same reference function over the same streams on 1 and on 16
host threads (Python threads; ctypes drops the interpreter lock for the call),
on a subset large enough to time (the rate does not depend on more streams).
One JSON line per measurement, appended to --out (default
profiles/lzmaenc/bench.jsonl); --ab runs every shape at 64, 32 and 16 streams
per wave, alternating, into profiles/lzmaenc/lanes_ab.jsonl instead.
"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHAPES = ((64, 4096), (1024, 4096), (4096, 4096), (65536, 4096), (4096, 65536), (1, 1 << 20))
LEVEL = 1
DICT = 0


def make_streams(n, length):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import native
    buf = ctypes.create_string_buffer(n * length)
    native.synth().synth_batch(0, 777000, buf, length, n, 16)
    return buf


def ref_encode_one(lib, base, length, dst, cap, props5):
    dl = ctypes.c_size_t(cap)
    res = lib.ref_lzma_encode(dst, ctypes.byref(dl), base, length, LEVEL, DICT, -1, -1, -1, -1, 0,
                              props5)
    assert res == 0, res
    return dl.value


def ref_lib():
    """The reference library with ref_lzma_encode taking raw addresses."""
    import native
    lib = native.ref()
    lib.ref_lzma_encode.argtypes = [ctypes.c_void_p, native.size_t_p, ctypes.c_void_p,
                                    ctypes.c_size_t] + list(lib.ref_lzma_encode.argtypes[4:])
    return lib


def cpu_leg(buf, n, length, threads):
    """Seconds per pass for the reference to encode streams [0, n) on `threads`
    threads: one warm-up pass, then passes until half a second has gone by."""
    lib = ref_lib()
    base = ctypes.addressof(buf)
    cap = length + length // 2 + 1024

    def work(t):
        dst = ctypes.create_string_buffer(cap)
        props5 = ctypes.create_string_buffer(5)
        for i in range(t, n, threads):
            ref_encode_one(lib, base + i * length, length, dst, cap, props5)

    pool = ThreadPoolExecutor(max_workers=threads)
    list(pool.map(work, range(threads)))               # warm-up
    passes, t0 = 0, time.perf_counter()
    while passes == 0 or time.perf_counter() - t0 < 0.5:
        list(pool.map(work, range(threads)))
        passes += 1
    s = (time.perf_counter() - t0) / passes
    pool.shutdown()
    return s


def gpu_setup(L, torch, np, buf, n, length):
    r, proto, props5 = L.enc_desc_from_props(L.enc_props(LEVEL, DICT))
    assert r == 0, L.last_error()
    cap = length + length // 2 + 1024
    descs = (L.EncStreamDesc * n)()
    for i in range(n):
        ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(proto), ctypes.sizeof(proto))
        descs[i].src_off, descs[i].src_len = i * length, length
        descs[i].dst_off, descs[i].dst_cap = i * cap, cap
    r, order, ws = L.enc_plan(descs, n)
    assert r == 0
    free_b, _ = torch.cuda.mem_get_info()
    if ws + n * (length + cap) > free_b * 0.8:
        return None
    g = dict(n=n, cap=cap, ws=ws, props5=props5)
    g["d_desc"] = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).cuda()
    g["d_src"] = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8, count=n * length).copy()).cuda()
    g["d_dst"] = torch.zeros((n * cap,), dtype=torch.uint8, device="cuda")
    g["d_ws"] = torch.empty((max(ws, 256),), dtype=torch.uint8, device="cuda")
    g["d_res"] = torch.zeros((n * 16,), dtype=torch.uint8, device="cuda")
    return g


def timed(torch, fn, reps):
    fn()                       # warm-up (code object load, first touch of the workspace)
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None or ms < best else best
    return best / 1e3


def gpu_encode(L, torch, g, lanes, reps):
    def launch():
        r = L.encode_batch_device(g["d_desc"].data_ptr(), 0, g["n"], g["d_src"].data_ptr(),
                                  g["d_dst"].data_ptr(), g["d_ws"].data_ptr(),
                                  g["d_res"].data_ptr(), lanes)
        assert r == 0, L.last_error()
    return timed(torch, launch, reps)


def gpu_clear(L, torch, g, reps):
    f = L.lib.lzmaencgpu_launch_init
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]

    def launch():
        assert f(g["d_desc"].data_ptr(), g["n"], g["d_ws"].data_ptr(), None) == 0
    return timed(torch, launch, reps)


def verify(L, g, buf, length, sample=32):
    """Every result SZ_OK; a sample of streams equal to the reference's bytes."""
    import native
    n, cap = g["n"], g["cap"]
    res = (L.EncResult * n).from_buffer_copy(g["d_res"].cpu().numpy().tobytes())
    assert all(q.res == 0 for q in res)
    packed = sum(q.dest_len for q in res)
    checked = 0
    if native.have_ref():
        lib = ref_lib()
        dst = ctypes.create_string_buffer(cap)
        props5 = ctypes.create_string_buffer(5)
        base = ctypes.addressof(buf)
        for i in sorted({(k * n) // sample for k in range(sample)} | {n - 1}):
            dl = ref_encode_one(lib, base + i * length, length, dst, cap, props5)
            got = g["d_dst"][i * cap:i * cap + res[i].dest_len].cpu().numpy().tobytes()
            assert (res[i].dest_len, got) == (dl, dst.raw[:dl]), i
            assert props5.raw == g["props5"]
            checked += 1
    return packed, checked


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join("%dx%d" % s for s in SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ab", action="store_true", help="streams-per-wave A/B instead of the table")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--dict", type=int, default=0,
                    help="dictSize; 0 = the level's default below level 5, the stream size from 5 up")
    a = ap.parse_args()
    global LEVEL, DICT
    LEVEL = a.level
    import numpy as np
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lzmagpu as L
    import native
    if L.device_count() <= 0:
        raise SystemExit("lzmaenc_bench: no HIP device: " + L.last_error())
    path = a.out or os.path.join(ROOT, "profiles", "lzmaenc",
                                 "lanes_ab.jsonl" if a.ab else "bench.jsonl")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if LEVEL >= 5:
        L.enc_set_modes(L.ENC_MODE_OPTIMAL | L.ENC_MODE_BT4)
    with open(path, "a") as out:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        for shape in a.shapes.split(","):
            n, length = (int(x) for x in shape.split("x"))
            DICT = a.dict or (max(length, 4096) if LEVEL >= 5 else 0)
            tag = dict(level=LEVEL, streams=n, stream_bytes=length)
            if DICT:
                tag["dict_size"] = DICT
            mb = n * length / 1e6
            buf = make_streams(n, length)
            g = gpu_setup(L, torch, np, buf, n, length)
            if g is None:
                emit(dict(tag, leg="gpu", skipped="workspace does not fit"))
                continue
            tag["workspace_mib"] = round(g["ws"] / 2**20, 1)
            if a.ab:
                for rnd in range(2):                      # alternating, twice
                    for lanes in (64, 32, 16):
                        s = gpu_encode(L, torch, g, lanes, a.reps)
                        verify(L, g, buf, length, sample=4)
                        emit(dict(tag, leg="gpu", lanes=lanes, round=rnd, seconds=round(s, 6),
                                  mb_per_s=round(mb / s, 2)))
                continue
            s = gpu_encode(L, torch, g, 0, a.reps)
            packed, checked = verify(L, g, buf, length)
            c = gpu_clear(L, torch, g, a.reps)
            emit(dict(tag, leg="gpu", lanes="default", seconds=round(s, 6),
                      mb_per_s=round(mb / s, 2), clear_seconds=round(c, 6),
                      packed_bytes=packed, verified_streams=checked))
            if a.no_cpu or not native.have_ref():
                continue
            for threads in (1, 16):
                if threads > n:
                    continue
                # enough streams to time; the rate does not depend on more
                k = min(n, max(threads, (8 << 20) * threads // length))
                s = cpu_leg(buf, k, length, threads)
                emit(dict(tag, leg="cpu_ref", streams_timed=k, threads=threads,
                          seconds=round(s, 6), mb_per_s=round(k * length / 1e6 / s, 2)))


if __name__ == "__main__":
    main()

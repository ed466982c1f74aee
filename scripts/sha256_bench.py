"""SHA-256 kernels and the xz SHA-256 block check on one MI355X.

    python scripts/sha256_bench.py kernels   [--repeat 7]
    python scripts/sha256_bench.py crossover [--repeat 5]
    python scripts/sha256_bench.py xz [--lib path/to/liblzmagpu.so] [--label name] [--repeat 9]

kernels    both kernels (lane per range, wave per range) at 65,536 x 4 KiB and
           at 1,024 x 1 MiB.
crossover  each kernel at n = 1, 64, 256, 1,024, 2,048, 3,072, 4,096 and 16,384 ranges of
           1 MiB: where AUTO should change from the wave to the lane kernel
           (kLzgpuSha256AutoLaneMin, csrc/lzma_gpu_internal.h).  Ranges beyond
           the first 1,024 alias the same 1 GiB of data: the kernels are
           issue-bound by two orders of magnitude, not bandwidth-bound.
xz         LzmaGpu_XzDecode wall time (host clock around the synchronous call)
           on a 256 x 1 MiB check-10 file and a one-block 16 MiB check-10 file.
           --lib names the library, so the same files can be timed against a
           build of another commit (run the two alternately, one process
           each); the files are cached in the temp directory between runs.

Kernel times are HIP events on the launch stream, warm (two untimed launches),
repeated; every line reports min / median / max of the repeats.  One JSON line
per measurement.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lzma-sdk-zliblike_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = {"lane": 1, "wave": 2}


def spread(ms):
    ms = sorted(ms)
    return {"min_ms": round(ms[0], 4), "median_ms": round(ms[len(ms) // 2], 4),
            "max_ms": round(ms[-1], 4), "repeats": len(ms)}


def time_batch(L, torch, data, n, size, kernel, repeat, alias=None):
    """Event times (ms) of Sha256Gpu_Batch over n ranges of `size` bytes."""
    dev = data.device
    stream = torch.cuda.current_stream()
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    off = (idx % alias if alias else idx) * size
    ln = torch.full((n,), size, dtype=torch.int64, device=dev)
    dig = torch.zeros(32 * n, dtype=torch.uint8, device=dev)

    def launch():
        r = L.sha256_batch_device(data.data_ptr(), off.data_ptr(), ln.data_ptr(), n,
                                  dig.data_ptr(), kernel=kernel, stream=stream.cuda_stream)
        assert r == 0, L.last_error()
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(repeat)]
    for s, e in ev:
        s.record(stream)
        launch()
        e.record(stream)
    torch.cuda.synchronize()
    # the first and the last range against hashlib: a wrong kernel is not timed
    host = bytes(dig[:32].cpu().numpy()), bytes(dig[-32:].cpu().numpy())
    first = bytes(data[:size].cpu().numpy())
    lo = int(off[-1])
    last = bytes(data[lo:lo + size].cpu().numpy())
    assert host == (hashlib.sha256(first).digest(), hashlib.sha256(last).digest())
    return [s.elapsed_time(e) for s, e in ev]


def report(part, name, n, size, ms):
    sp = spread(ms)
    print(json.dumps({"part": part, "kernel": name, "ranges": n, "range_bytes": size, **sp,
                      "GB_per_s_median": round(n * size / sp["median_ms"] / 1e6, 2)}), flush=True)


def run_kernels(a, part):
    import torch
    torch.zeros(1, device="cuda")
    import lzmagpu as L
    g = torch.Generator(device="cuda").manual_seed(5)
    data = torch.randint(0, 256, (1 << 30,), dtype=torch.uint8, device="cuda", generator=g)
    if part == "kernels":
        shapes = [(65536, 4096), (1024, 1 << 20)]
    else:
        shapes = [(n, 1 << 20) for n in (1, 64, 256, 1024, 2048, 3072, 4096, 16384)]
    for n, size in shapes:
        for name, k in KERNELS.items():
            ms = time_batch(L, torch, data, n, size, k, a.repeat, alias=1024 if n > 1024 else None)
            report(part, name, n, size, ms)


def xz_files():
    """(name, file bytes, plain sha256, plain size) of the two check-10 files,
    cached in the temp directory (writing them takes longer than timing them)."""
    import native
    import xzwrite as M
    out = []
    for name, nblk, bsz in (("256x1MiB", 256, 1 << 20), ("1x16MiB", 1, 16 << 20)):
        path = os.path.join(tempfile.gettempdir(), f"lzgpu_sha256_bench_{name}.xz")
        distinct = [native.gen("text", 4200 + i, bsz) for i in range(min(nblk, 16))]
        plain = [distinct[i % len(distinct)] for i in range(nblk)]
        if not os.path.exists(path):
            made = {}
            for i, d in enumerate(distinct):
                made[i] = M.make_block(d, 10, dict_size=1 << 20)
            # make_stream's layout around ready-made blocks
            import struct
            import zlib
            flags = bytes([0, 10])
            f = b"\xfd7zXZ\0" + flags + struct.pack("<I", zlib.crc32(flags))
            recs = []
            for i in range(nblk):
                b, unp, n = made[i % len(distinct)]
                f += b
                recs.append((unp, n))
            idx = b"\0" + M.varint(len(recs)) + b"".join(M.varint(u) + M.varint(n) for u, n in recs)
            idx += b"\0" * ((-len(idx)) % 4)
            idx += struct.pack("<I", zlib.crc32(idx))
            back = struct.pack("<I", len(idx) // 4 - 1) + flags
            f += idx + struct.pack("<I", zlib.crc32(back)) + back + b"YZ"
            with open(path + ".tmp", "wb") as fh:
                fh.write(f)
            os.replace(path + ".tmp", path)
        with open(path, "rb") as fh:
            f = fh.read()
        h = hashlib.sha256()
        for p in plain:
            h.update(p)
        out.append((name, f, h.digest(), nblk * bsz))
    return out


def run_xz(a):
    files = xz_files()
    lib = ctypes.CDLL(a.lib or os.path.join(ROOT, "lzma-sdk-zliblike_amd", "lib", "liblzmagpu.so"))
    lib.LzmaGpu_XzDecode.restype = ctypes.c_int
    lib.LzmaGpu_XzDecode.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t),
                                     ctypes.c_char_p, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_int64)]
    for name, f, want, total in files:
        out = ctypes.create_string_buffer(total)
        ms = []
        for it in range(2 + a.repeat):
            dl, bad = ctypes.c_size_t(total), ctypes.c_int64(-1)
            t0 = time.perf_counter()
            r = lib.LzmaGpu_XzDecode(out, ctypes.byref(dl), f, len(f), ctypes.byref(bad))
            t1 = time.perf_counter()
            assert (r, dl.value, bad.value) == (0, total, -1), (r, dl.value, bad.value)
            if it >= 2:
                ms.append((t1 - t0) * 1e3)
        assert hashlib.sha256(out.raw).digest() == want
        print(json.dumps({"part": "xz", "label": a.label, "file": name, "file_bytes": len(f),
                          "plain_bytes": total, **spread(ms)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=("kernels", "crossover", "xz"))
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--lib", default="")
    ap.add_argument("--label", default="this")
    a = ap.parse_args()
    if a.part == "xz":
        run_xz(a)
    else:
        run_kernels(a, a.part)


if __name__ == "__main__":
    main()

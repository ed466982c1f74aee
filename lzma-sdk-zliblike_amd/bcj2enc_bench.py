"""Throughput of the BCJ2 batch encoder (its own script; bench.py measures the
LZMA decode flagship and is not involved).

Data: the bytes of one x86 file (--file, by default the running Python
executable) repeated to 64 MiB and cut into 1 x 64 MiB, 64 x 1 MiB and
4,096 x 16 KiB streams.  Per shape, device buffers in place, best of --reps
after a warm-up, timed with events on the stream:
  bcj2_split   plan, classify, stream scan and scatter (the parallel phases)
  bcj2_code    the range coder over the bit lists (one lane per stream)
  bcj2_all     Bcj2EncGpu_EncodeBatch, all five launches
  x86_batch    BcjGpu_X86Batch, encoding, one lane per range, on a copy of the
               same buffers made afresh before every call, outside the clock
  cpu_ref_x86  the reference's x86_Convert on one host core (where
               oracle/_ref/libref.so is built)
One stream of every shape is decoded back with Bcj2_Decode and compared.

Then LzmaGpu_7zWrite over the file itself (at most --file-max bytes) as one
LZMA level-1 folder with every branch filter the writer has: time and archive
size.  One JSON line per measurement, appended to --out (default
profiles/bcj2enc/bench.jsonl).
"""
import argparse
import ctypes
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOTAL = 64 << 20
SHAPES = ((1, 64 << 20), (64, 1 << 20), (4096, 16 << 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file", default=sys.executable)
    ap.add_argument("--file-max", type=int, default=2 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import lzmagpu as L
    import native
    if L.device_count() <= 0:
        raise SystemExit("bcj2enc_bench: no HIP device: " + L.last_error())
    path = a.out or os.path.join(ROOT, "profiles", "bcj2enc", "bench.jsonl")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(os.path.realpath(a.file), "rb") as f:
        code = f.read()
    data = (code * (TOTAL // len(code) + 1))[:TOTAL]
    d_src = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    launch = L.lib.bcj2encgpu_launch
    launch.restype = ctypes.c_int
    launch.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4 + [
        ctypes.c_uint, ctypes.c_void_p]

    def timed(fn, reps, before=lambda: None):
        before()
        fn()
        torch.cuda.synchronize()
        best = None
        for _ in range(reps):
            before()    # outside the clock
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None or ms < best else best
        return best / 1e3

    with open(path, "a") as out:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        for n, length in SHAPES:
            tag = dict(streams=n, stream_bytes=length, file=os.path.basename(a.file))
            mb = n * length / 1e6
            bound = L.bcj2_bound(length)
            descs = (L.Bcj2EncDesc * n)()
            at = 0
            for i in range(n):
                descs[i].src_off, descs[i].src_len = i * length, length
                for k in range(4):
                    descs[i].out[k].off, descs[i].out[k].cap = at, bound[k]
                    at += bound[k]
            d_descs = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
            d_dst = torch.zeros(at, dtype=torch.uint8, device="cuda")
            d_ws = torch.empty(L.bcj2_scratch(descs, n), dtype=torch.uint8, device="cuda")
            d_res = torch.zeros(n * 40, dtype=torch.uint8, device="cuda")
            ptrs = (d_descs.data_ptr(), n, d_src.data_ptr(), d_dst.data_ptr(), d_ws.data_ptr(),
                    d_res.data_ptr())

            def phase(mask):
                # the library's launcher on the null stream, which torch's
                # default stream is
                assert launch(*ptrs, mask, None) == 0

            def whole():
                assert L.bcj2_encode_batch_device(*ptrs) == 0
            for leg, fn in (("bcj2_split", lambda: phase(1)), ("bcj2_code", lambda: phase(2)),
                            ("bcj2_all", whole)):
                s = timed(fn, a.reps)
                emit(dict(tag, leg=leg, seconds=round(s, 6), mb_per_s=round(mb / s, 1)))
            res = (L.Bcj2EncResult * n).from_buffer_copy(d_res.cpu().numpy().tobytes())
            assert all(r.res == 0 for r in res)
            # the last stream, decoded back
            o, r = descs[n - 1].out, res[n - 1]
            parts = [d_dst[o[k].off:o[k].off + r.len[k]].cpu().numpy().tobytes() for k in range(4)]
            if length <= 1 << 20:
                assert L.Bcj2_Decode(*parts, length) == (0, data[(n - 1) * length:n * length])
            emit(dict(tag, leg="bcj2_sizes", main=sum(r.len[0] for r in res),
                      call=sum(r.len[1] for r in res), jump=sum(r.len[2] for r in res),
                      rc=sum(r.len[3] for r in res), scratch_bytes=d_ws.numel(),
                      verified_stream_bytes=length if length <= 1 << 20 else 0))
            # the x86 filter of the parent commit, one lane per range, in place
            d_copy = d_src.clone()
            d_off = torch.arange(n, dtype=torch.int64, device="cuda") * length
            d_len = torch.full((n,), length, dtype=torch.int64, device="cuda")
            d_ip = torch.zeros(n, dtype=torch.int32, device="cuda")
            d_state = torch.zeros(n, dtype=torch.int32, device="cuda")
            d_done = torch.zeros(n, dtype=torch.int64, device="cuda")

            def fresh():     # every call on the same bytes as the BCJ2 legs
                d_copy.copy_(d_src)
                d_state.zero_()

            def x86():
                assert L.bcj_x86_batch_device(d_copy.data_ptr(), d_off.data_ptr(),
                                              d_len.data_ptr(), d_ip.data_ptr(),
                                              d_state.data_ptr(), d_done.data_ptr(), n, 1) == 0
            s = timed(x86, a.reps, fresh)
            emit(dict(tag, leg="x86_batch", seconds=round(s, 6), mb_per_s=round(mb / s, 1)))
            del d_copy, d_dst, d_ws
            if native.have_ref():
                ref = native.ref_cont()
                f = ref.x86_Convert
                f.restype = ctypes.c_size_t
                buf = ctypes.create_string_buffer(data, len(data))
                t0 = time.perf_counter()
                for i in range(n):
                    state = ctypes.c_uint32(0)
                    f(ctypes.byref(buf, i * length), ctypes.c_size_t(length), ctypes.c_uint32(0),
                      ctypes.byref(state), 1)
                s = time.perf_counter() - t0
                emit(dict(tag, leg="cpu_ref_x86", threads=1, seconds=round(s, 6),
                          mb_per_s=round(mb / s, 1)))
        # the 7z writer over the file itself
        src = code[:a.file_max]
        filters = [("none", 0), ("x86", L.SZ_FILTER_X86), ("bcj2", L.SZ_FILTER_BCJ2)]
        for name, filt in filters:
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                arc = L.sevenz_compress([("a.bin", src)], method=L.SZ_M_LZMA, filter=filt, level=1)
                s = time.perf_counter() - t0
                best = s if best is None or s < best else best
            r, got, fres = L.SzExtract(arc, len(src), max_files=1)
            assert r == 0 and got == src and fres[:1] == [0]
            emit(dict(leg="gpu_7zwrite", filter=name, file=os.path.basename(a.file),
                      file_bytes=len(src), level=1, seconds=round(best, 6),
                      archive_bytes=len(arc)))


if __name__ == "__main__":
    main()

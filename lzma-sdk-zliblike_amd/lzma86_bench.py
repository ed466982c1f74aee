"""Throughput of the Lzma86 batch encoder (its own script; bench.py measures the
LZMA decode flagship and is not involved).

Data: the bytes of one x86 file (--file, by default the running Python
executable), repeated where the file is shorter than the shape, cut into
4,096 x 4 KiB, 65,536 x 4 KiB and 4,096 x 64 KiB streams; level 1, default
dictionary, every stream with room for len + len / 2 + 1024 + 14 bytes.

Per shape:
  lzma86        Lzma86Gpu_EncodeBatch over device buffers under SZ_FILTER_NO,
                _YES and _AUTO: a host clock around the call and a synchronise
                (the call plans on the host and uploads its tables), one
                warm-up, then --reps runs: the least, the median and the largest
                time; the packed size (against mode NO) and the share of streams
                whose flag byte is 1
  stages        Lzma86Gpu_EncodeBatchHost with LZMA86_GPU_TIMINGS (a synchronise
                after every stage), a second set of calls: filter, encode,
                select and gather, under SZ_FILTER_AUTO
  split         the 64 KiB shape under AUTO with LZGPU_LZMA86_SPLIT at 4 KiB,
                32 KiB (the default) and 1 GiB (never split), alternating
  plain_2n      LzmaEncGpu_EncodeBatch over the same 2n candidate streams (the
                sources and their x86-filtered copies), in a child process per
                library: this build and, with --parent-lib, the parent commit's
                liblzmagpu.so, alternating --rounds times.  The claim to check
                is that AUTO costs about what this plain batch costs.
One JSON line per measurement, appended to --out (default
profiles/lzma86/bench.jsonl).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHAPES = ((4096, 4096), (65536, 4096), (4096, 65536))
MODES = (("no", 0), ("yes", 1), ("auto", 2))


def cap_of(length):
    return 14 + length + length // 2 + 1024


def load(path, n, length):
    with open(os.path.realpath(path), "rb") as f:
        code = f.read()
    total = n * length
    return (code * (total // len(code) + 1))[:total], len(code)


def timed(fn, sync, reps):
    fn()
    sync()
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return out


def spread(ts):
    return dict(seconds=round(min(ts), 6), median=round(statistics.median(ts), 6),
                worst=round(max(ts), 6), reps=len(ts))


def plain_leg(a):
    """The child: one plain LzmaEncGpu_EncodeBatch over 2n streams, one JSON line.
    LZGPU_LIB names the library; --binding the directory of the lzmagpu.py that
    goes with it (a parent commit's binding knows its own library's symbols)."""
    sys.path.insert(0, a.binding or HERE)
    import numpy as np
    import torch
    import lzmagpu as L
    n, length = a.plain
    data, _ = load(a.file, n, length)
    d_src = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    d_filt = d_src.clone()
    d_off = torch.arange(n, dtype=torch.int64, device="cuda") * length
    d_len = torch.full((n,), length, dtype=torch.int64, device="cuda")
    d_ip = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_state = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_done = torch.zeros(n, dtype=torch.int64, device="cuda")
    assert L.bcj_x86_batch_device(d_filt.data_ptr(), d_off.data_ptr(), d_len.data_ptr(),
                                  d_ip.data_ptr(), d_state.data_ptr(), d_done.data_ptr(), n, 1) == 0
    d_all = torch.cat([d_src, d_filt])
    del d_src, d_filt
    r, proto, _ = L.enc_desc_from_props(L.enc_props(1, 0))
    assert r == 0
    m, room = 2 * n, cap_of(length) - 14
    descs = (L.EncStreamDesc * m)()
    for i in range(m):
        ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(proto), ctypes.sizeof(proto))
        # a stream and its filtered copy side by side, as the Lzma86 batch has them
        src = (i // 2) * length + (n * length if i % 2 else 0)
        descs[i].src_off, descs[i].src_len = src, length
        descs[i].dst_off, descs[i].dst_cap = i * room, room
    r, order, ws = L.enc_plan(descs, m)
    assert r == 0
    d_desc = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
    d_order = torch.tensor(order, dtype=torch.int32, device="cuda")
    d_dst = torch.empty(m * room, dtype=torch.uint8, device="cuda")
    d_ws = torch.empty(max(ws, 256), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(m * 16, dtype=torch.uint8, device="cuda")

    def run():
        assert L.encode_batch_device(d_desc.data_ptr(), d_order.data_ptr(), m, d_all.data_ptr(),
                                     d_dst.data_ptr(), d_ws.data_ptr(), d_res.data_ptr()) == 0
    ts = timed(run, torch.cuda.synchronize, a.reps)
    res = (L.EncResult * m).from_buffer_copy(d_res.cpu().numpy().tobytes())
    assert all(q.res == 0 for q in res)
    print(json.dumps(dict(spread(ts), packed=sum(q.dest_len for q in res))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file", default=sys.executable)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=None,
                    help="the parent commit's liblzmagpu.so for the plain_2n leg")
    ap.add_argument("--shapes", default=None, help="indices into the shape list, e.g. 0,2")
    ap.add_argument("--parent-binding", default=None,
                    help="the directory of the parent commit's lzmagpu.py (default: beside "
                         "--parent-lib, else this one)")
    ap.add_argument("--plain", type=int, nargs=2, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--binding", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.plain:
        return plain_leg(a)
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import lzmagpu as L
    if L.device_count() <= 0:
        raise SystemExit("lzma86_bench: no HIP device: " + L.last_error())
    path = a.out or os.path.join(ROOT, "profiles", "lzma86", "bench.jsonl")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    shapes = [SHAPES[int(k)] for k in a.shapes.split(",")] if a.shapes else SHAPES
    sync = torch.cuda.synchronize
    with open(path, "a") as out:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        for n, length in shapes:
            data, file_bytes = load(a.file, n, length)
            tag = dict(streams=n, stream_bytes=length, file=os.path.basename(a.file),
                       file_bytes=file_bytes, level=1)
            mb = n * length / 1e6
            cap = cap_of(length)
            d_src = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
            d_dst = torch.empty(n * cap, dtype=torch.uint8, device="cuda")
            d_res = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
            base = None

            def descs_of(mode):
                return L.lzma86_descs([dict(src_off=i * length, src_len=length, dst_off=i * cap,
                                            dst_cap=cap, level=1, dict_size=0, mode=mode)
                                       for i in range(n)])

            def device_leg(descs, split=None):
                r, scratch = L.lzma86_encode_scratch(descs, n)
                assert r == 0
                free = torch.cuda.mem_get_info()[0]
                if scratch > free:
                    return None, scratch
                d_scratch = torch.empty(scratch, dtype=torch.uint8, device="cuda")

                def run():
                    assert L.lzma86_encode_batch_device(descs, n, d_src.data_ptr(),
                                                        d_dst.data_ptr(), d_scratch.data_ptr(),
                                                        scratch, d_res.data_ptr()) == 0
                ts = timed(run, sync, a.reps)
                res = (L.Lzma86Result * n).from_buffer_copy(d_res.cpu().numpy().tobytes())
                assert all(q.res == 0 for q in res)
                return (ts, res), scratch

            for name, mode in MODES:
                descs = descs_of(mode)
                got, scratch = device_leg(descs)
                if got is None:
                    emit(dict(tag, leg="lzma86", mode=name, skipped="scratch does not fit",
                              scratch_bytes=scratch))
                    continue
                ts, res = got
                packed = sum(q.dest_len for q in res)
                base = packed if mode == 0 else base
                emit(dict(tag, leg="lzma86", mode=name, **spread(ts),
                          mb_per_s=round(mb / min(ts), 1), packed_bytes=packed,
                          packed_vs_no=round(packed / base, 4) if base else None,
                          filter_share=round(sum(q.filter for q in res) / n, 4),
                          scratch_bytes=scratch))
            # the stages, each behind a synchronise: a second set of calls
            descs = descs_of(2)
            stats = L.Lzma86Stats()
            dst0 = bytes(n * cap)
            for k in range(2):
                stats.flags = L.LZMA86_TIMINGS
                r, _, _ = L.lzma86_encode_batch_host(descs, n, data, dst0, 0, stats)
                assert r == 0, L.last_error()
            emit(dict(tag, leg="stages", mode="auto", filter_s=round(stats.stage_ns[0] / 1e9, 6),
                      encode_s=round(stats.stage_ns[1] / 1e9, 6),
                      select_gather_s=round(stats.stage_ns[2] / 1e9, 6),
                      call_s=round(stats.stage_ns[3] / 1e9, 6), candidates=stats.candidates,
                      encode_launches=stats.encode_launches))
            del dst0
            if length > 32768:
                for rnd in range(a.rounds):
                    for split in (4096, 32768, 1 << 30):
                        os.environ["LZGPU_LZMA86_SPLIT"] = str(split)
                        got, _ = device_leg(descs)
                        del os.environ["LZGPU_LZMA86_SPLIT"]
                        if got:
                            emit(dict(tag, leg="split", mode="auto", split=split, round=rnd,
                                      **spread(got[0])))
            del d_src, d_dst, d_res
            torch.cuda.empty_cache()
            # the plain batch over the same 2n streams, a fresh process per library
            libs = [("this", None)] + ([("parent", a.parent_lib)] if a.parent_lib else [])
            for rnd in range(a.rounds):
                for who, lib in libs:
                    env = dict(os.environ)
                    binding = HERE
                    if lib:
                        env["LZGPU_LIB"] = os.path.abspath(lib)
                        beside = os.path.dirname(os.path.abspath(lib))
                        binding = a.parent_binding or (
                            beside if os.path.exists(os.path.join(beside, "lzmagpu.py")) else HERE)
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--file", a.file,
                                        "--reps", str(a.reps), "--plain", str(n), str(length),
                                        "--binding", os.path.abspath(binding)],
                                       env=env, capture_output=True, text=True, timeout=300)
                    if p.returncode != 0:
                        raise SystemExit("lzma86_bench: the plain leg failed: " + p.stderr[-2000:])
                    row = json.loads(p.stdout.strip().splitlines()[-1])
                    emit(dict(tag, leg="plain_2n", library=who, round=rnd, **row,
                              mb_per_s=round(mb / row["seconds"], 1)))


if __name__ == "__main__":
    main()

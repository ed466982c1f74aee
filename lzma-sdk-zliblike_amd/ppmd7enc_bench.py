"""Throughput of Ppmd7Gpu_EncodeBatch (its own script; bench.py measures the
LZMA flagship and is not involved).

The streams and batch sizes of ppmd7_bench.py: the golden order-6 and order-8
text streams at their own model sizes and the order-6 text at 16 MiB, their
plain text (recovered by decoding, sha256 checked) replicated into batches of
64, 1,024 and 4,096 buffers, every copy with its own input bytes, output range
and workspace slice.  Timing: HIP events around the launch alone, after a
warm-up launch, best of --reps; every copy's result and packed bytes are
compared with the fixture after the timed region.  Replicas flatter the cache
behaviour (equal bytes read in step, all streams ending together), so one more
leg encodes distinct synthetic texts and verifies them by decoding back on the
device.

Beside each encode line: the GPU decode rate of the same batch in the same run
(ppmd7_bench.py's own leg), and the reference's DECODER on 1 and 16 host
threads (csrc/ppmd7_cpu_bench.c over oracle/_ref/libref.so).  The reference's
encoder is not in that library, so there is no reference-encoder baseline here
and the CPU lines are labelled as the decoder.  All rates are plain bytes per
second.  One JSON line per measurement, appended to --out (default
profiles/ppmd7enc/bench.jsonl).
"""
import argparse
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ppmd7_bench as D  # noqa: E402


def timed(torch, launch, reps, before=None):
    launch()  # warm-up (code object load, first touch of the workspace)
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None or ms < best else best
    return best / 1e3


def encode_batch(L, torch, np, plains, order, mem, cap, reps):
    """Encode the equal-length buffers `plains` (a [copies, n] uint8 array).
    Returns (seconds, results, d_dst viewed [copies, cap]) or None when the
    workspace does not fit."""
    copies, n = plains.shape
    slice_bytes = L.ppmd7_workspace_bytes(mem)
    free_b, _ = torch.cuda.mem_get_info()
    if slice_bytes * copies > free_b * 0.8:
        return None
    descs = [dict(src_off=k * n, src_len=n, dst_off=k * cap, dst_cap=cap, order=order,
                  mem_size=mem, ws_off=k * slice_bytes) for k in range(copies)]
    d_src = torch.from_numpy(plains.reshape(-1)).cuda()
    d_desc = torch.from_numpy(np.frombuffer(bytes(L.ppmd7_make_enc_descs(descs)),
                                            dtype=np.uint8).copy()).cuda()
    d_dst = torch.zeros((copies * cap,), dtype=torch.uint8, device="cuda")
    d_ws = torch.empty((slice_bytes * copies,), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((copies * 24,), dtype=torch.uint8, device="cuda")

    def launch():
        r = L.ppmd7_encode_batch_device(d_desc.data_ptr(), copies, d_src.data_ptr(),
                                        d_dst.data_ptr(), d_ws.data_ptr(), d_res.data_ptr())
        assert r == 0, L.last_error()

    s = timed(torch, launch, reps, d_dst.zero_)
    res = (L.Ppmd7EncResult * copies).from_buffer_copy(d_res.cpu().numpy().tobytes())
    return s, res, d_dst.view(copies, cap)


def decode_back(L, torch, np, d_packed, lens, cap, n, order, mem):
    """Decode what encode_batch left in d_packed ([copies, cap]) on the device."""
    copies = len(lens)
    slice_bytes = L.ppmd7_workspace_bytes(mem)
    descs = [dict(src_off=k * cap, src_len=lens[k], dst_off=k * n, dst_len=n, order=order,
                  mem_size=mem, ws_off=k * slice_bytes) for k in range(copies)]
    d_desc = torch.from_numpy(np.frombuffer(bytes(L.ppmd7_make_descs(descs)),
                                            dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros((copies * n,), dtype=torch.uint8, device="cuda")
    d_ws = torch.empty((slice_bytes * copies,), dtype=torch.uint8, device="cuda")
    d_res = torch.zeros((copies * 24,), dtype=torch.uint8, device="cuda")
    r = L.ppmd7_decode_batch_device(d_desc.data_ptr(), copies, d_packed.data_ptr(),
                                    d_out.data_ptr(), d_ws.data_ptr(), d_res.data_ptr())
    torch.cuda.synchronize()
    assert r == 0, L.last_error()
    res = (L.Ppmd7Result * copies).from_buffer_copy(d_res.cpu().numpy().tobytes())
    assert all((q.res, q.dest_len, q.src_len) == (0, n, lens[k]) for k, q in enumerate(res))
    return d_out.view(copies, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppmd7enc", "bench.jsonl"))
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-decode", action="store_true", help="skip the GPU decode leg")
    ap.add_argument("--tag", default=None, help="copied into every row (variant runs)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import lzmagpu as L
    if L.device_count() <= 0:
        raise SystemExit("ppmd7enc_bench: no HIP device: " + L.last_error())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    batches = [int(x) for x in a.batches.split(",")]
    with open(a.out, "a") as out:
        def emit(row):
            if a.tag:
                row = dict(row, tag=a.tag)
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        for c, packed in D.load_cases():
            n, order, mem = c["plain_len"], c["order"], c["mem_size"]
            tag = dict(order=order, mem_size=mem, plain_len=n, packed_len=len(packed))
            # the fixture's plain text: one stream through the host call
            desc = L.ppmd7_make_descs([dict(src_off=0, src_len=len(packed), dst_off=0, dst_len=n,
                                            order=order, mem_size=mem)])
            r, res, plain = L.ppmd7_decode_batch_host(desc, 1, packed, bytes(n))
            assert r == 0 and res[0].res == 0
            assert hashlib.sha256(plain).hexdigest() == c["sha256"]
            one = np.frombuffer(plain, dtype=np.uint8)
            want = torch.from_numpy(np.frombuffer(packed, dtype=np.uint8).copy()).cuda()
            cap = (len(packed) + 64 + 15) & ~15
            for copies in batches:
                mb = copies * n / 1e6
                got = encode_batch(L, torch, np, np.tile(one, (copies, 1)), order, mem, cap, a.reps)
                if got is None:
                    emit(dict(tag, leg="gpu_encode", batch=copies, skipped="workspace does not fit"))
                    continue
                s, res, rows = got
                # verification, after the timed region: every copy against the fixture
                assert all((q.res, q.dest_len, q.packed_len) == (0, len(packed), len(packed))
                           for q in res)
                assert bool((rows[:, :len(packed)] == want).all())
                del rows, got
                emit(dict(tag, leg="gpu_encode", batch=copies, seconds=round(s, 6),
                          mb_per_s=round(mb / s, 2)))
                if not a.no_decode:
                    s = D.gpu_leg(L, torch, np, c, packed, copies, a.reps)
                    emit(dict(tag, leg="gpu_decode", batch=copies, seconds=round(s, 6),
                              mb_per_s=round(mb / s, 2)))
                if a.no_cpu or not os.path.exists(D.LIBREF):
                    continue
                for threads in (1, 16):
                    # the 1-thread leg decodes at most 64 copies: its rate does not depend on more
                    k = min(copies, 64) if threads == 1 else copies
                    s = D.cpu_leg(c, packed, k, threads, 1 if k > 256 else 2)
                    emit(dict(tag, leg="cpu_ref_decoder", batch=k, threads=threads,
                              seconds=round(s, 6), mb_per_s=round(k * n / 1e6 / s, 2)))

        # distinct texts: no two streams read the same bytes or end together
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import native
        order, mem = 6, 1 << 16
        for copies in batches:
            n = 30000
            plains = np.zeros((copies, n), dtype=np.uint8)
            for k in range(copies):
                plains[k] = np.frombuffer(native.gen("text", 1000 + k, n), dtype=np.uint8)
            # equal lengths keep the layout simple; the texts differ
            cap = n + 4096
            s, res, rows = encode_batch(L, torch, np, plains, order, mem, cap, a.reps)
            assert all(q.res == 0 and q.dest_len == q.packed_len for q in res)
            lens = [q.dest_len for q in res]
            back = decode_back(L, torch, np, rows, lens, cap, n, order, mem)
            assert bool((back.cpu() == torch.from_numpy(plains)).all())
            emit(dict(order=order, mem_size=mem, plain_len=n, leg="gpu_encode_distinct_texts",
                      batch=copies, packed_mean=round(sum(lens) / copies, 1),
                      seconds=round(s, 6), mb_per_s=round(copies * n / 1e6 / s, 2)))


if __name__ == "__main__":
    main()

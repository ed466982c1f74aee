"""Cost of feeding LZMA encoder sessions in pieces (LzmaEncGpu_SessionEncodeBatch)
against the one-shot batch (LzmaEncGpu_EncodeBatch) on the same data.  Its own
script; bench.py measures the LZMA decode flagship and is not involved.

Level 1 with default props on the synthetic generator's English-like text, every
stream with its own seed (as lzmaenc_bench.py).  Shapes: 4,096 and 65,536
sessions of 64 KiB.  The whole source is on the device before the timed region;
a piece "arrives" when the session's src_len is raised, so what is timed is the
device's work, not the host's copies.  Legs, one JSON line each, appended to
--out (default profiles/lzmaenc_session/bench.jsonl):

  oneshot   LzmaEncGpu_EncodeBatch (hash clear + encode), warm-up then best of
            --reps
  pieces    the same streams through sessions in pieces of 4 KiB, 16 KiB and
            64 KiB: every round raises every session's src_len by one piece, the
            last round sets finish.  HIP events around each round's call (list
            pass, init, encode); total and per-round seconds.  One pass per piece
            size (a session cannot be rewound), after a warm-up pass on 256
            sessions.  Every session's length and a sample of streams' bytes are
            compared with the one-shot leg's.
  listpass  the list pass alone over records that all have work and over records
            that are all finished: best of --reps
  sparse    one round in which 1 % of fresh sessions have 16 KiB and the rest
            nothing, against the first round of the 16 KiB leg (all have 16 KiB)
  lone      LzmaEnc_Encode of one 1 MiB stream through 64 KiB reads, wall time

Not measured: host-to-device copies of arriving pieces, uneven piece sizes
across sessions, lanes other than the default, budgets."""
import argparse
import ctypes
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import lzmaenc_bench as B  # noqa: E402

SHAPES = ((4096, 65536), (65536, 65536))
PIECES = (4096, 16384, 65536)


class Sessions:
    """n sessions over one packed source (already on the device), records
    edited in bulk through numpy."""

    def __init__(self, L, torch, np, d_src, n, length, cap):
        self.L, self.torch, self.np, self.n, self.length = L, torch, np, n, length
        props = L.enc_props(1, 0)
        self.ws_bytes = L.enc_session_workspace_bytes(props, length)
        self.d_dst = torch.zeros((n * cap,), dtype=torch.uint8, device="cuda")
        self.d_ws = torch.empty((n * self.ws_bytes,), dtype=torch.uint8, device="cuda")
        self.d_scratch = torch.zeros((L.enc_session_scratch_bytes(n),), dtype=torch.uint8,
                                     device="cuda")
        self.rec = (L.EncSession * n)()
        for i in range(n):
            r, _ = L.enc_session_init(self.rec[i], props, d_src.data_ptr() + i * length, length,
                                      self.d_dst.data_ptr() + i * cap, cap,
                                      self.d_ws.data_ptr() + i * self.ws_bytes)
            assert r == 0, L.last_error()
        size = ctypes.sizeof(L.EncSession)
        self.bytes = np.frombuffer(self.rec, dtype=np.uint8).reshape(n, size)
        self.d_rec = torch.empty((n * size,), dtype=torch.uint8, device="cuda")

    def field(self, name, dtype):
        f = getattr(self.L.EncSession, name)
        return self.bytes[:, f.offset:f.offset + f.size].view(dtype)[:, 0]

    def upload(self):
        self.d_rec.copy_(self.torch.from_numpy(self.bytes.reshape(-1)))

    def download(self):
        self.bytes.reshape(-1)[:] = self.d_rec.cpu().numpy()

    def round(self):
        r = self.L.enc_session_encode_batch(self.d_rec.data_ptr(), self.n,
                                            self.d_scratch.data_ptr(), 0,
                                            self.torch.cuda.current_stream().cuda_stream)
        assert r == 0, self.L.last_error()


def timed_once(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def pieces_leg(L, torch, np, g, n, length, piece):
    """(per-round seconds, Sessions) of n sessions fed `piece` bytes a round."""
    s = Sessions(L, torch, np, g["d_src"], n, length, g["cap"])
    rounds = (length + piece - 1) // piece
    secs = []
    for r in range(rounds):
        s.field("src_len", np.uint64)[:] = min(length, (r + 1) * piece)
        s.field("finish", np.uint32)[:] = 1 if r == rounds - 1 else 0
        s.upload()
        torch.cuda.synchronize()
        secs.append(timed_once(torch, s.round))
        s.download()
    return secs, s


def verify_against_oneshot(L, np, g, s, sample=32):
    n, cap = s.n, g["cap"]
    res = (L.EncResult * n).from_buffer_copy(g["d_res"].cpu().numpy().tobytes())
    want_len = np.array([q.dest_len for q in res], dtype=np.uint64)
    assert (s.field("res", np.int32) == 0).all() and (s.field("finished", np.uint32) == 1).all()
    assert (s.field("out_pos", np.uint64) == want_len).all()
    for i in sorted({(k * n) // sample for k in range(sample)} | {n - 1}):
        lo, hi = i * cap, i * cap + int(want_len[i])
        assert bool((s.d_dst[lo:hi] == g["d_dst"][lo:hi]).all()), i
    return int(want_len.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join("%dx%d" % s for s in SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lzmagpu as L
    if L.device_count() <= 0:
        raise SystemExit("lzmaenc_session_bench: no HIP device: " + L.last_error())
    path = a.out or os.path.join(ROOT, "profiles", "lzmaenc_session", "bench.jsonl")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as out:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        # warm-up: code objects loaded, every kernel run once
        buf = B.make_streams(256, 65536)
        g = B.gpu_setup(L, torch, np, buf, 256, 65536)
        B.gpu_encode(L, torch, g, 0, 1)
        pieces_leg(L, torch, np, g, 256, 65536, 16384)
        for shape in a.shapes.split(","):
            n, length = (int(x) for x in shape.split("x"))
            tag = dict(level=1, sessions=n, stream_bytes=length)
            mb = n * length / 1e6
            buf = B.make_streams(n, length)
            g = B.gpu_setup(L, torch, np, buf, n, length)
            if g is None:
                emit(dict(tag, leg="oneshot", skipped="workspace does not fit"))
                continue
            sec = B.gpu_encode(L, torch, g, 0, a.reps)
            B.verify(L, g, buf, length)
            emit(dict(tag, leg="oneshot", seconds=round(sec, 6), mb_per_s=round(mb / sec, 2)))
            first_16k = None
            for piece in PIECES:
                secs, s = pieces_leg(L, torch, np, g, n, length, piece)
                packed = verify_against_oneshot(L, np, g, s)
                total = sum(secs)
                if piece == 16384:
                    first_16k = secs[0]
                emit(dict(tag, leg="pieces", piece_bytes=piece, rounds=len(secs), reps=1,
                          seconds=round(total, 6), mb_per_s=round(mb / total, 2),
                          vs_oneshot=round(total / sec, 3),
                          round_seconds_min=round(min(secs), 6), round_seconds_max=round(max(secs), 6),
                          round_seconds_first=round(secs[0], 6), round_seconds_last=round(secs[-1], 6),
                          packed_bytes=packed))
                # the list pass alone: every session finished
                if piece == PIECES[-1]:
                    fin = B.timed(torch, lambda: L.enc_session_list_pass(
                        s.d_rec.data_ptr(), n, s.d_scratch.data_ptr(),
                        torch.cuda.current_stream().cuda_stream), a.reps)
                del s
                torch.cuda.empty_cache()
            s = Sessions(L, torch, np, g["d_src"], n, length, g["cap"])
            s.field("src_len", np.uint64)[:] = 16384
            s.upload()
            work = B.timed(torch, lambda: L.enc_session_list_pass(
                s.d_rec.data_ptr(), n, s.d_scratch.data_ptr(),
                torch.cuda.current_stream().cuda_stream), a.reps)
            emit(dict(tag, leg="listpass", seconds_all_have_work=round(work, 6),
                      seconds_all_finished=round(fin, 6)))
            # a sparse round: 1 % of fresh sessions have 16 KiB, the rest nothing
            s.field("src_len", np.uint64)[:] = 0
            s.field("src_len", np.uint64)[::100] = 16384
            s.upload()
            torch.cuda.synchronize()
            sparse = timed_once(torch, s.round)
            s.download()
            worked = int((s.field("in_pos", np.uint64) > 0).sum())
            assert worked == len(range(0, n, 100))
            emit(dict(tag, leg="sparse", piece_bytes=16384, sessions_with_input=worked,
                      seconds=round(sparse, 6), full_round_seconds=round(first_16k, 6),
                      vs_full_round=round(sparse / first_16k, 4)))
            del s, g
            torch.cuda.empty_cache()
        # one lone stream through the handle drop-in
        buf = B.make_streams(1, 1 << 20)
        data = buf.raw
        at, got = [0], []

        def read(k):
            b = data[at[0]:at[0] + min(k, 65536)]
            at[0] += len(b)
            return b
        t0 = time.perf_counter()
        r, _ = L.LzmaEnc_Encode(read, lambda b: got.append(b) or len(b), L.enc_props(1, 0))
        wall = time.perf_counter() - t0
        one = L.LzmaEncode(data, L.enc_props(1, 0), len(data) * 2)
        assert r == 0 and b"".join(got) == one[3]
        emit(dict(level=1, leg="lone", stream_bytes=len(data), read_bytes=65536,
                  seconds=round(wall, 4), mb_per_s=round(len(data) / 1e6 / wall, 3)))


if __name__ == "__main__":
    main()

"""End-to-end throughput of LzmaGpu_7zWrite (its own script; bench.py measures
the LZMA decode flagship and is not involved).

Distinct English-like text files (csrc/synth.c, every file its own seed), LZMA
level 1 with default props, one folder per file: 4,096 and 65,536 files of
4 KiB, 4,096 of 64 KiB; and one solid variant, JOIN groups of 16 files.  The
call goes from host memory to host memory: upload, CRC-32 batch, encode batch,
pack, download, header.

Timing: the host clock around the call, after a warm-up call, best of --reps.
A second set of calls with LZMA_GPU_7Z_WRITE_TIMINGS (a synchronisation after
every stage) gives the split; its total is reported next to the untimed one.
The pack stage's share is reported against the encode stage of the same call.
After the timed region the archive is opened with LzmaGpu_7zOpen and extracted
with LzmaGpu_7zExtract, and the bytes are compared with the source.

Baseline: the reference has no 7z writer, so there is no container baseline;
beside each shape stands the reference's LzmaEncode per file (oracle/_ref/
libref_lzma.so) on 1 and on 16 host threads, as in lzmaenc_bench.py.  One JSON
line per measurement, appended to --out (default profiles/7zenc/bench.jsonl).
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# (files, file bytes, files per folder)
SHAPES = ((4096, 4096, 1), (65536, 4096, 1), (4096, 65536, 1), (65536, 4096, 16))
LEVEL = 1


def describe(L, n, length, solid):
    entries = [("f/%02x/%05d.txt" % (i >> 8 & 0xFF, i), i * length, length,
                L.SZ_ITEM_JOIN if i % solid else 0, 0) for i in range(n)]
    items, names, names_len = L.sz_items(entries)
    return items, names, names_len


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join("%dx%dx%d" % s for s in SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lzmagpu as L
    import native
    import lzmaenc_bench as E
    if L.device_count() <= 0:
        raise SystemExit("sevenzenc_bench: no HIP device: " + L.last_error())
    path = a.out or os.path.join(ROOT, "profiles", "7zenc", "bench.jsonl")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    methods = [L.sz_method(L.SZ_M_LZMA, level=LEVEL)]
    with open(path, "a") as out:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        for shape in a.shapes.split(","):
            n, length, solid = (int(x) for x in shape.split("x"))
            tag = dict(level=LEVEL, files=n, file_bytes=length, files_per_folder=solid)
            mb = n * length / 1e6
            buf = E.make_streams(n, length)
            src = buf.raw[:n * length]
            items, names, names_len = describe(L, n, length, solid)
            r, folders, pieces, bound = L.sz_write_plan(items, n, len(src), names_len, methods)
            assert r == 0

            def call(flags):
                t0 = time.perf_counter()
                r, size, dest, st = L.SzWrite(src, items, n, names, names_len, methods, bound,
                                              flags)
                s = time.perf_counter() - t0
                assert r == 0, L.last_error()
                return s, size, dest, st

            call(0)                                   # warm-up
            best = None
            for _ in range(a.reps):
                # SzWrite's Python side (buffer creation, the copy out) is inside
                # the clock: the stats' total is the call itself
                s, size, dest, st = call(0)
                t = st.stage_ns[7] / 1e9
                best = t if best is None or t < best else best
            split = None
            for _ in range(a.reps):
                s, size, dest, st = call(L.SZ_WRITE_TIMINGS)
                if split is None or st.stage_ns[7] < split[7]:
                    split = list(st.stage_ns)
            arc = dest[:size]
            r, got, fres = L.SzExtract(arc, len(src), max_files=n)
            assert r == 0 and got == src and fres[:n] == [0] * n
            stages = {k: round(v / 1e9, 6) for k, v in zip(L.SZ_STAGES, split)}
            emit(dict(tag, leg="gpu_7zwrite", seconds=round(best, 6), mb_per_s=round(mb / best, 2),
                      folders=st.folders, pieces=st.pieces, reencoded=st.reencoded,
                      encode_launches=st.encode_launches, archive_bytes=size,
                      pack_bytes=st.pack_bytes, header_bytes=st.header_bytes, stages=stages,
                      pack_share_of_encode=round(split[4] / split[3], 5), verified_files=n))
            if a.no_cpu or not native.have_ref() or solid != 1:
                continue
            for threads in (1, 16):
                k = min(n, max(threads, (8 << 20) * threads // length))
                s = E.cpu_leg(buf, k, length, threads)
                emit(dict(tag, leg="cpu_ref_lzmaencode", streams_timed=k, threads=threads,
                          seconds=round(s, 6), mb_per_s=round(k * length / 1e6 / s, 2)))


if __name__ == "__main__":
    main()

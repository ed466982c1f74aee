"""Throughput of the LZMA2 and xz writers (its own script; bench.py measures the
LZMA decode flagship and is not involved).

One buffer of the synthetic generator's English-like text (csrc/synth.c, a seed
per MiB), 64 MiB and 256 MiB, level 1 with default props (64 KiB dictionary,
lc3 lp0 pb2), cut into blocks of 64 KiB, 256 KiB and 1 MiB.  Per buffer and
block size, one JSON line each for:

  gpu_encode    Lzma2EncGpu_EncodeBatch alone (hash clear + encode), HIP events
                around the device-pointer call after a warm-up call, best of
                --reps
  gpu_compact   the same plus Lzma2EncGpu_Compact
  host_lzma2    LzmaGpu_Lzma2EncodeHost from host memory to host memory (its
                allocations, copies and synchronisation included), host clock
  host_xz       LzmaGpu_XzEncode with CRC-64, the same way
  cpu_ref       the reference's Lzma2Enc_Encode per block
                (oracle/_ref/libref_lzma.so, ref_lzma2_encode) on 1 and on 16
                host threads over the same blocks, on a subset large enough to
                time

After the timed region every block's result is checked for SZ_OK, the compacted
stream's length against the sum, and a sample of blocks byte for byte against
the reference.  --chunk-cost instead runs 4,096 text streams of 64 KiB through
LzmaEncGpu_EncodeBatch and through the LZMA2 batch in alternating rounds and
counts the chunks.  --xz-filter FILE instead takes the bytes of an x86 file
repeated to the first buffer size and writes them with LzmaGpu_XzEncodeEx
(CRC-64, the first block size) without a filter and with the x86 filter,
alternating: time and file size of each (legs host_xz_exe and host_xz_exe_x86).
Lines are appended to --out (default profiles/lzma2enc/bench.jsonl,
chunk_cost.jsonl)."""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LEVEL = 1
DICT = 0   # --level 5 and up: the block size (the hash is sized by the dictionary)
MIB = 1 << 20


def make_text(n_bytes):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import native
    buf = ctypes.create_string_buffer(n_bytes)
    native.synth().synth_batch(0, 888000, buf, MIB, n_bytes // MIB, 16)
    return buf


def ref_lib():
    """The reference library with ref_lzma2_encode taking raw addresses."""
    import native
    lib = native.ref()
    lib.ref_lzma2_encode.argtypes = [ctypes.c_void_p, native.size_t_p, ctypes.c_void_p,
                                     ctypes.c_size_t] + list(lib.ref_lzma2_encode.argtypes[4:])
    return lib


def ref_block(lib, addr, length, dst, cap):
    dl = ctypes.c_size_t(cap)
    prop = ctypes.c_ubyte(0)
    res = lib.ref_lzma2_encode(dst, ctypes.byref(dl), addr, length, LEVEL, min(DICT, length) if DICT else 0, -1, -1, -1, 0,
                               ctypes.byref(prop))
    assert res == 0, res
    return dl.value


def cpu_leg(buf, n, block, threads):
    """Seconds per pass for the reference to encode blocks [0, n) on `threads`
    threads: one warm-up pass, then passes until half a second has gone by."""
    lib = ref_lib()
    base = ctypes.addressof(buf)
    cap = block + block // 2 + 4096

    def work(t):
        dst = ctypes.create_string_buffer(cap)
        for i in range(t, n, threads):
            ref_block(lib, base + i * block, block, dst, cap)

    pool = ThreadPoolExecutor(max_workers=threads)
    list(pool.map(work, range(threads)))               # warm-up
    passes, t0 = 0, time.perf_counter()
    while passes == 0 or time.perf_counter() - t0 < 0.5:
        list(pool.map(work, range(threads)))
        passes += 1
    s = (time.perf_counter() - t0) / passes
    pool.shutdown()
    return s


def timed(torch, fn, reps):
    t0 = time.perf_counter()
    fn()                       # warm-up (code object load, first touch of the workspace)
    torch.cuda.synchronize()
    if time.perf_counter() - t0 > 4.0:
        reps = 1               # seconds per launch: one timed repeat says enough
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


def gpu_setup(L, torch, np, buf, total, block):
    r, proto, prop = L.enc2_desc_from_props(L.enc2_props(LEVEL, DICT))
    assert r == 0
    n = (total + block - 1) // block
    cap = L.block_bound(block)
    descs = (L.EncStreamDesc * n)()
    for i in range(n):
        ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(proto), ctypes.sizeof(proto))
        descs[i].src_off, descs[i].src_len = i * block, min(block, total - i * block)
        descs[i].dst_off, descs[i].dst_cap = i * cap, cap
    r, order, ws = L.enc2_plan(descs, n)
    assert r == 0
    g = dict(n=n, cap=cap, ws=ws, prop=prop, out_cap=n * cap + 1)
    g["d_desc"] = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).cuda()
    g["d_src"] = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8, count=total).copy()).cuda()
    g["d_dst"] = torch.zeros((n * cap,), dtype=torch.uint8, device="cuda")
    g["d_out"] = torch.zeros((g["out_cap"],), dtype=torch.uint8, device="cuda")
    g["d_ws"] = torch.empty((max(ws, 256),), dtype=torch.uint8, device="cuda")
    g["d_res"] = torch.zeros((n * 16,), dtype=torch.uint8, device="cuda")
    g["d_off"] = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    g["d_tot"] = torch.zeros((16,), dtype=torch.uint8, device="cuda")
    return g


def launch_encode(L, g):
    r = L.lzma2_encode_batch_device(g["d_desc"].data_ptr(), 0, g["n"], g["d_src"].data_ptr(),
                                    g["d_dst"].data_ptr(), g["d_ws"].data_ptr(),
                                    g["d_res"].data_ptr(), 0)
    assert r == 0, L.last_error()


def launch_compact(L, g):
    r = L.lzma2_compact_device(g["d_desc"].data_ptr(), g["d_res"].data_ptr(), g["n"],
                               g["d_dst"].data_ptr(), g["d_out"].data_ptr(), g["out_cap"],
                               g["d_off"].data_ptr(), g["d_tot"].data_ptr())
    assert r == 0, L.last_error()


def verify(L, g, buf, total, block, sample=8):
    """Every block SZ_OK, the compacted length the sum plus one, a sample of
    blocks equal to the reference's bytes.  Returns (stream bytes, checked)."""
    import native
    n, cap = g["n"], g["cap"]
    res = (L.EncResult * n).from_buffer_copy(g["d_res"].cpu().numpy().tobytes())
    assert all(q.res == 0 for q in res)
    tot = L.EncResult.from_buffer_copy(g["d_tot"].cpu().numpy().tobytes())
    offs = g["d_off"].cpu().tolist()
    assert tot.res == 0 and tot.dest_len == sum(q.dest_len for q in res) + 1 == offs[n] + 1
    checked = 0
    if native.have_ref():
        lib = ref_lib()
        rcap = block + block // 2 + 4096
        dst = ctypes.create_string_buffer(rcap)
        base = ctypes.addressof(buf)
        for i in sorted({(k * n) // sample for k in range(sample)} | {n - 1}):
            length = min(block, total - i * block)
            dl = ref_block(lib, base + i * block, length, dst, rcap)
            got = g["d_out"][offs[i]:offs[i + 1]].cpu().numpy().tobytes()
            assert got == dst.raw[:dl - 1], i
            assert got == g["d_dst"][i * cap:i * cap + res[i].dest_len].cpu().numpy().tobytes()
            checked += 1
    return tot.dest_len, checked


def host_leg(fn, min_reps=1, budget_s=6.0):
    """Best wall time of fn() (it ends synchronised): one more repeat while the
    budget lasts, at most three."""
    best, spent, reps = None, 0.0, 0
    while reps < min_reps or (reps < 3 and spent < budget_s):
        t0 = time.perf_counter()
        fn()
        s = time.perf_counter() - t0
        best = s if best is None or s < best else best
        spent += s
        reps += 1
    return best, reps


def run_table(a, L, torch, np, native, emit):
    blocks = [int(x) for x in a.blocks.split(",")]
    # load the code objects and the runtime's pools before any host-call timing
    small = make_text(MIB)
    dl = ctypes.c_size_t(2 * MIB)
    warm = ctypes.create_string_buffer(2 * MIB)
    prop = ctypes.c_ubyte(0)
    assert L.lib.LzmaGpu_Lzma2EncodeHost(warm, ctypes.byref(dl), small, MIB,
                                         ctypes.byref(L.enc2_props(LEVEL, DICT, block_size=65536)),
                                         ctypes.byref(prop)) == 0, L.last_error()
    for mib in (int(x) for x in a.sizes.split(",")):
        total = mib * MIB
        buf = make_text(total)
        dest = ctypes.create_string_buffer(total + total // 512 + 4096)
        for block in blocks:
            tag = dict(level=LEVEL, buffer_mib=mib, block_bytes=block,
                       blocks=(total + block - 1) // block)
            mb = total / 1e6
            g = gpu_setup(L, torch, np, buf, total, block)
            tag["workspace_mib"] = round(g["ws"] / 2**20, 1)
            s = timed(torch, lambda: launch_encode(L, g), a.reps)
            emit(dict(tag, leg="gpu_encode", seconds=round(s, 6), mb_per_s=round(mb / s, 2)))

            def both():
                launch_encode(L, g)
                launch_compact(L, g)
            s2 = timed(torch, both, a.reps)
            c = timed(torch, lambda: launch_compact(L, g), a.reps)
            packed, checked = verify(L, g, buf, total, block)
            emit(dict(tag, leg="gpu_compact", seconds=round(s2, 6), mb_per_s=round(mb / s2, 2),
                      compact_seconds=round(c, 6), packed_bytes=packed,
                      ratio=round(packed / total, 4), verified_blocks=checked))
            del g
            torch.cuda.empty_cache()
            props = L.enc2_props(LEVEL, DICT, block_size=block)

            def host_lzma2():
                dl = ctypes.c_size_t(len(dest))
                r = L.lib.LzmaGpu_Lzma2EncodeHost(dest, ctypes.byref(dl), buf, total,
                                                  ctypes.byref(props), ctypes.byref(prop))
                assert (r, dl.value) == (0, packed), (r, dl.value, L.last_error())

            def host_xz():
                dl = ctypes.c_size_t(len(dest))
                r = L.lib.LzmaGpu_XzEncode(dest, ctypes.byref(dl), buf, total, ctypes.byref(props), 4)
                assert r == 0 and dl.value > packed, (r, L.last_error())
            for leg, fn in (("host_lzma2", host_lzma2), ("host_xz", host_xz)):
                s, reps = host_leg(fn)
                emit(dict(tag, leg=leg, seconds=round(s, 6), mb_per_s=round(mb / s, 2), reps=reps))
            if a.no_cpu or not native.have_ref() or mib != int(a.sizes.split(",")[0]):
                continue                # the per-block CPU rate does not depend on the buffer
            for threads in (1, 16):
                k = min(tag["blocks"], max(threads, (8 << 20) * threads // block))
                s = cpu_leg(buf, k, block, threads)
                emit(dict(tag, leg="cpu_ref", blocks_timed=k, threads=threads,
                          seconds=round(s, 6), mb_per_s=round(k * block / 1e6 / s, 2)))


def run_xz_filter(a, L, emit):
    total = int(a.sizes.split(",")[0]) * MIB
    block = int(a.blocks.split(",")[0])
    with open(os.path.realpath(a.xz_filter), "rb") as f:
        code = f.read()
    buf = (code * (total // len(code) + 1))[:total]
    cap = total + total // 256 + 65536
    props = L.enc2_props(LEVEL, DICT, block_size=block)
    tag = dict(level=LEVEL, buffer_mib=total // MIB, block_bytes=block,
               blocks=(total + block - 1) // block, file=os.path.basename(a.xz_filter),
               file_bytes=len(code))
    sizes = {}

    def leg(chain):
        r, xz = L.XzEncodeEx(buf, props, 4, cap, chain)
        assert r == 0, L.last_error()
        sizes[bool(chain)] = len(xz)
        return xz
    assert L.XzDecode(leg([(4, 0)]), total)[:2] == (0, buf)      # warm-up and round trip
    for rnd in range(max(a.reps, 2)):
        for name, chain in (("host_xz_exe", []), ("host_xz_exe_x86", [(4, 0)])):
            t0 = time.perf_counter()
            leg(chain)
            s = time.perf_counter() - t0
            emit(dict(tag, leg=name, round=rnd, seconds=round(s, 6),
                      mb_per_s=round(total / 1e6 / s, 2), xz_bytes=sizes[bool(chain)]))


def count_chunks(L, g):
    """LZMA2 chunk headers in every block's slot."""
    n, cap = g["n"], g["cap"]
    res = (L.EncResult * n).from_buffer_copy(g["d_res"].cpu().numpy().tobytes())
    out = g["d_dst"].cpu().numpy().tobytes()
    chunks = 0
    for i in range(n):
        at, end = i * cap, i * cap + res[i].dest_len
        while at < end:
            ctl = out[at]
            if ctl < 0x80:
                at += 3 + ((out[at + 1] << 8) | out[at + 2]) + 1
            else:
                at += 5 + (1 if ctl >= 0xC0 else 0) + ((out[at + 3] << 8) | out[at + 4]) + 1
            chunks += 1
        assert at == end
    return chunks, sum(q.dest_len for q in res)


def run_chunk_cost(a, L, torch, np, emit):
    import lzmaenc_bench as B
    n, length = 4096, 65536
    buf = B.make_streams(n, length)
    g1 = B.gpu_setup(L, torch, np, buf, n, length)
    g2 = gpu_setup(L, torch, np, buf, n * length, length)
    mb = n * length / 1e6
    tag = dict(level=LEVEL, streams=n, stream_bytes=length)
    for rnd in range(2):                              # alternating, twice
        s1 = B.gpu_encode(L, torch, g1, 0, a.reps)
        emit(dict(tag, leg="lzma", round=rnd, seconds=round(s1, 6), mb_per_s=round(mb / s1, 2)))
        s2 = timed(torch, lambda: launch_encode(L, g2), a.reps)
        emit(dict(tag, leg="lzma2", round=rnd, seconds=round(s2, 6), mb_per_s=round(mb / s2, 2)))
    packed1, _ = B.verify(L, g1, buf, length, sample=4)
    chunks, packed2 = count_chunks(L, g2)
    cells = 1846 + (0x300 << 3)
    emit(dict(tag, leg="chunks", chunks=chunks, lzma_packed=packed1, lzma2_packed=packed2,
              saved_table_bytes=(cells * 2 + 15) & ~15,
              save_moves_16b_per_chunk=((cells * 2 + 15) & ~15) // 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256", help="buffer sizes, MiB")
    ap.add_argument("--blocks", default="65536,262144,1048576")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--chunk-cost", action="store_true")
    ap.add_argument("--xz-filter", default=None, metavar="FILE",
                    help="the xz writer with and without the x86 filter over FILE's bytes")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--level", type=int, default=1,
                    help="5 and up: the optimal parser and Bt4, modes switched on for the run, "
                         "dictionary = the smallest block size")
    a = ap.parse_args()
    global LEVEL, DICT
    LEVEL = a.level
    if LEVEL >= 5:
        DICT = min(int(x) for x in a.blocks.split(","))
    import numpy as np
    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lzmagpu as L
    import native
    if L.device_count() <= 0:
        raise SystemExit("lzma2enc_bench: no HIP device: " + L.last_error())
    if LEVEL >= 5:
        L.enc_set_modes(L.ENC_MODE_OPTIMAL | L.ENC_MODE_BT4)
    path = a.out or os.path.join(ROOT, "profiles", "lzma2enc",
                                 "chunk_cost.jsonl" if a.chunk_cost else "bench.jsonl")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as out:
        def emit(row):
            line = json.dumps(row)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        if a.xz_filter:
            run_xz_filter(a, L, emit)
        elif a.chunk_cost:
            run_chunk_cost(a, L, torch, np, emit)
        else:
            run_table(a, L, torch, np, native, emit)


if __name__ == "__main__":
    main()

"""The planner matrix behind tests/golden/decode_plan_cases.json: which batches
and LzmaGpuPlanOptions the golden plans were recorded for.  Shared by the
generator (tests/golden/make_golden_decode_plan.py), tests/test_decode_plan.py
and, as a text file, the stand-alone program tests/emu_hostplan/
decode_plan_check.cpp, which builds the same items from the same formula."""
import ctypes
import zlib

import numpy as np

LZMA, LZMA2 = 0, 1


def _lzma(b0):
    return (LZMA, bytes([b0, 0, 0, 1, 0]))     # 64 KiB dictionary


# name -> (pattern cycled over the items, item appended behind them or None)
SETS = {
    "00": ([_lzma(0x00)], None),               # lc0/pb0
    "5d": ([_lzma(0x5d)], None),               # lc3/pb2
    "02": ([_lzma(0x02)], None),               # lc2
    "b8": ([_lzma(0xb8)], None),               # lc4/pb4
    "e0": ([_lzma(0xe0)], None),               # lc8/lp4/pb4: too wide for LDS
    "e1": ([_lzma(0xe1)], None),               # invalid
    "l2": ([(LZMA2, bytes([16]))], None),
    "l2bad": ([(LZMA2, bytes([41]))], None),   # invalid
    "mix4": ([_lzma(0x00), _lzma(0x5d), _lzma(0x02), _lzma(0xb8)], None),
    "mix21": ([_lzma(0x5d), _lzma(0x00), _lzma(0x00)], (LZMA2, bytes([16]))),
}
NS = (0, 1, 3, 300, 1024, 4096, 65536)
KERNELS = ("auto", "throughput", "latency", "coop", "global")
KNOWN_FLAG_BITS = (1, 2, 4, 8, 16, 32, 64, 256)
PLAN_MASKS = {0x105, 0x105 | 0x40000000, 0x1BF, 0x19F, 0x1BF | 0x80000000, 0x7FF | 0x80000000}


def cases():
    """[(set name, n, options dict)]: every set x n x cus x kernel with the other
    options at their defaults (the one- and no-stream batches on auto only), then
    every other option value alone on three sets at two sizes."""
    out = []
    for s in SETS:
        for n in NS:
            for cus in (4, 256):
                for k in range(len(KERNELS) if n >= 3 else 1):
                    out.append((s, n, dict(kernel=k, cus=cus)))
    alone = [dict(flags=f) for f in KNOWN_FLAG_BITS]
    alone += [dict(coop=v) for v in (1, 2)] + [dict(lanes_per_group=v) for v in (2, 64)]
    alone += [dict(groups_per_cu=v) for v in (6, 14)]
    alone += [dict(waves_per_simd=v) for v in (1, 2, 4, 6, 8)]
    alone += [dict(persistent=2), dict(one_class=1)]
    for s in ("00", "b8", "mix21"):
        for n in (300, 4096):
            for cus in (4, 256):
                for a in alone:
                    out.append((s, n, dict(kernel=0, cus=cus, **a)))
    # a forced kernel with an override: widened latency waves, narrow throughput
    # waves (slices, no interleaved rows), the register budget of each
    for s in ("00", "b8"):
        for k in (1, 2, 3):
            for a in (dict(lanes_per_group=2), dict(waves_per_simd=1), dict(waves_per_simd=4),
                      dict(flags=2)):
                out.append((s, 300, dict(kernel=k, cus=4, **a)))
    return out


def make_descs(L, name, n):
    """The set's StreamDesc array: item i has src_len 100 + 10 (37 i mod 97),
    dst_cap 256 (1 + i mod 5), dst_off 4096 i."""
    descs = (L.StreamDesc * max(n, 1))()
    if n == 0:
        return descs
    arr = np.frombuffer(descs, dtype=np.uint8).reshape(max(n, 1), 48)[:n]
    i = np.arange(n, dtype=np.uint64)
    u64 = arr[:, :40].view(np.uint64)
    u64[:, 0] = 0
    u64[:, 1] = 100 + 10 * (37 * i % 97)
    u64[:, 2] = 4096 * i
    u64[:, 3] = 256 * (1 + i % 5)
    # bytes 40..47 of a descriptor: props[5], props_size, finish_mode, kind
    pat, tail = SETS[name]
    table = np.zeros((len(pat) + 1, 8), dtype=np.uint8)
    for j, (kind, props) in enumerate(pat + [tail or pat[0]]):
        table[j, :len(props)] = np.frombuffer(props, dtype=np.uint8)
        table[j, 5:] = (len(props), 1, kind)
    which = (i % len(pat)).astype(np.int64)
    if tail:
        which[n - 1] = len(pat)
    arr[:, 40:48] = table[which]
    return descs


def options(L, o):
    po = L.PlanOptions()
    for k, v in o.items():
        setattr(po, k, v)
    return po


def plan_ints(p):
    """The whole LzmaGpuPlan as a flat list: 10 header fields, then the four
    classes' 10 fields each."""
    out = [p.workspace_bytes, p.n, p.n_lds, p.lanes_per_group, p.lds_cells_per_lane,
           p.groups_per_cu, p.waves_per_simd, p.queue_offset, p.persistent, p.n_classes]
    for c in p.classes:
        out += [c.n, c.lanes_per_group, c.lds_cells_per_lane, c.groups_per_cu, c.waves_per_simd,
                c.lds_mask, c.flags, c.slot_off, c.slot_cells, c.slot_groups]
    return [int(v) for v in out]


def run_case(L, descs, n, o):
    """Plans through LzmaGpu_PlanBatchOpt; {"res", "plan", "probs", "order"} with
    probs_off and the order as lists up to 64 items, as CRC-32 of the
    little-endian arrays above."""
    order = (ctypes.c_uint32 * max(n, 1))()
    p = L.Plan()
    res = L.lib.LzmaGpu_PlanBatchOpt(descs, n, order, ctypes.byref(p), ctypes.byref(options(L, o)))
    probs = np.frombuffer(descs, dtype=np.uint64).reshape(-1, 6)[:n, 4].astype("<u8")
    ordr = np.frombuffer(order, dtype=np.uint32)[:n].astype("<u4")
    small = n <= 64
    return dict(res=int(res), plan=plan_ints(p),
                probs=[int(v) for v in probs] if small else zlib.crc32(probs.tobytes()),
                order=[int(v) for v in ordr] if small else zlib.crc32(ordr.tobytes()))

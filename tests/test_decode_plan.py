"""csrc/decode_plan.h -- the batch decoder's planner and launch shape.

Without a GPU:
- the library plans every case of tests/golden/decode_plan_cases.json (recorded
  before the planner moved into the header) exactly as recorded;
- the launch shapes of the branches of the launcher, written out by hand from
  the template ladder the shape function replaced;
- the header as a stand-alone sanitizer program (tests/emu_hostplan/
  decode_plan_check.cpp: g++ -Wall -Werror -O1 -fsanitize=address,undefined, own
  main, run as a child process) over the same matrix, against the golden and
  the library's answers.  -Wno-unknown-pragmas is for lzma_device.h's
  `#pragma unroll`, which g++ does not know;
- the kernel table is the 42 builds the ladder instantiated.
On the GPU: every row of the table launched once, results against the oracle.
"""
import ctypes
import json
import lzma
import os
import subprocess
import zlib

import numpy as np
import pytest

import decode_plan_cases as C
import native

SRC = os.path.join(native.ROOT, "tests", "emu_hostplan", "decode_plan_check.cpp")
CSRC = os.path.join(native.ROOT, "lzma-sdk-zliblike_amd", "csrc")
GOLDEN = os.path.join(native.ROOT, "tests", "golden", "decode_plan_cases.json")

ILV, COOP, WIN = 0x40000000, 0x80000000, 0x08000000
M_THR, M_LAT, M_SG, M_ALL = 0x105, 0x1BF, 0x19F, 0x7FF
LDS, DUP, COOPK = 0, 1, 2      # kernel families
K2 = 1                         # LZMA_GPU_CLASS_HAS_LZMA2

# (family, W, mask, K2) of every build: the instantiations of the former ladder
TABLE = {(f, w, m, k2)
         for f, ws, ms in ((LDS, (1, 2, 4), (M_THR, M_THR | ILV, M_LAT)),
                           (DUP, (1, 2, 4), (M_LAT, M_SG)),
                           (COOPK, (2, 4), (M_LAT | COOP, M_ALL | COOP, M_ALL | COOP | WIN)))
         for w in ws for m in ms for k2 in (0, 1)}


class Env(ctypes.Structure):
    _fields_ = [("dup", ctypes.c_int32), ("win_off", ctypes.c_uint32)]


class Shape(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint32) for k in ("family", "w", "mask", "k2", "grid", "block",
                                               "win_bytes", "lanes_total")] + \
               [("lds_bytes", ctypes.c_uint64)]

    def astuple(self):
        return tuple(int(getattr(self, k)) for k, _ in self._fields_)


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


def cls(L, mask, lanes, stride, groups, waves, n, flags=0, slot_groups=0):
    c = L.LdsClass()
    c.lds_mask, c.lanes_per_group, c.lds_cells_per_lane = mask, lanes, stride
    c.groups_per_cu, c.waves_per_simd, c.n, c.flags = groups, waves, n, flags
    c.slot_cells, c.slot_groups = (1458, slot_groups) if mask & ILV else (0, 0)
    return c


def shape(L, c, max_groups, cus, dup=32, win_off=0, n=None):
    """(family, w, mask, k2, grid, block, win_bytes, lanes_total, lds_bytes) or None."""
    s, env = Shape(), Env(dup, win_off)
    ok = L.lib.lzgpu_decode_launch_shape(ctypes.byref(c), int(c.n) if n is None else n, max_groups,
                                         cus, ctypes.byref(env), ctypes.byref(s))
    return s.astuple() if ok else None


def session_shape(L, n, lds_cells, max_groups, cus, win_off=0):
    s, env = Shape(), Env(32, win_off)
    ok = L.lib.lzgpu_session_launch_shape(n, lds_cells, max_groups, cus, ctypes.byref(env),
                                          ctypes.byref(s))
    return s.astuple() if ok else None


# ---------------------------------------------------------------- plans

@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_is_the_matrix(golden):
    assert [(c["set"], c["n"], c["opt"]) for c in golden] == C.cases()
    assert all(c["res"] == 0 for c in golden)
    masks = {c["plan"][10 + 10 * k + 5] for c in golden for k in range(c["plan"][9])}
    assert masks == C.PLAN_MASKS


def test_library_reproduces_every_golden_plan(L, golden):
    descs = {}
    for c in golden:
        key = (c["set"], c["n"])
        if key not in descs:
            descs[key] = C.make_descs(L, *key)
        got = C.run_case(L, descs[key], c["n"], c["opt"])
        for k in ("res", "plan", "probs", "order"):
            assert got[k] == c[k], (c["set"], c["n"], c["opt"], k)


# ---------------------------------------------------------------- launch shapes by hand

def test_kernel_table_is_the_ladders_builds(L):
    rows = (ctypes.c_uint32 * (4 * 64))()
    n = L.lib.lzgpu_decode_kernel_rows(rows, 64)
    got = [tuple(rows[4 * i:4 * i + 4]) for i in range(n)]
    assert n == 42 and len(set(got)) == 42 and set(got) == TABLE


def test_throughput_interleaved(L):
    # config 3: 65,536 streams, 32 lanes x 8 workgroups per CU on 256 CUs.  The
    # slices take 32 * 318 * 2 = 20,352 B, a workgroup's share 16 blocks = 20,480
    c = cls(L, M_THR | ILV, 32, 318, 8, 2, 65536, slot_groups=2048)
    assert shape(L, c, 2048, 256) == (LDS, 2, M_THR | ILV, 0, 2048, 32, 0, 65536, 20480)
    # one launch round (no group cap): the grid covers the batch
    assert shape(L, c, 0, 256) == (LDS, 2, M_THR | ILV, 0, 2048, 32, 0, 65536, 20480)
    # persistent lanes over a smaller slot area: the grid is the slot area's
    c.slot_groups = 2047
    assert shape(L, c, 4096, 256) == (LDS, 2, M_THR | ILV, 0, 2047, 32, 0, 2047 * 32, 20480)
    # whole 32-lane rows: 33 lanes take two, 64 * 318 * 2 = 40,704 B
    c = cls(L, M_THR | ILV, 33, 318, 8, 2, 66, K2, slot_groups=2)
    assert shape(L, c, 0, 256) == (LDS, 2, M_THR | ILV, 1, 2, 33, 0, 66, 40704)


def test_interleaved_refusals(L):
    c = cls(L, M_THR | ILV, 32, 318, 8, 2, 65536, slot_groups=2047)
    assert shape(L, c, 0, 256) is None            # grid above the slot area, no queue refills
    c.slot_groups = 0
    assert shape(L, c, 2048, 256) is None
    c = cls(L, M_THR | ILV, 65, 318, 1, 1, 65, slot_groups=8)
    assert shape(L, c, 8, 256) is None            # 64 < lanes
    c.lanes_per_group = 64
    assert shape(L, c, 8, 256) == (LDS, 1, M_THR | ILV, 0, 2, 64, 0, 128, 163840)


def test_throughput_slices(L):
    # 4 lanes x 318 cells = 2,544 B, padded to the share of 16 workgroups (8 blocks)
    c = cls(L, M_THR, 4, 318, 16, 4, 300)
    assert shape(L, c, 0, 4) == (LDS, 4, M_THR, 0, 75, 4, 0, 300, 10240)
    assert shape(L, c, 64, 4) == (LDS, 4, M_THR, 0, 64, 4, 0, 256, 10240)
    # the register budget is the plan's, not clamped: 0 and 1 -> 1, 2, above 2 -> 4
    for waves, w in ((0, 1), (1, 1), (2, 2), (3, 4), (4, 4), (6, 4), (8, 4)):
        c.waves_per_simd = waves
        assert shape(L, c, 0, 256)[1] == w
    # one lane per workgroup is still the one-lane kernel on this placement
    c = cls(L, M_THR, 1, 318, 16, 4, 3)
    assert shape(L, c, 0, 256) == (LDS, 4, M_THR, 0, 3, 1, 0, 3, 10240)


def test_latency_one_lane(L):
    # lc0/pb0 at 0x1BF: 638 cells = 1,276 B, 16 workgroups per CU
    c = cls(L, M_LAT, 1, 638, 16, 4, 4096)
    # 16 resident per CU: W = min(4, 4)
    assert shape(L, c, 4096, 256) == (DUP, 4, M_LAT, 0, 4096, 32, 0, 4096, 10240)
    # 3 streams: one workgroup on a CU, W = min(4, 1); 5 per CU: 2
    assert shape(L, c, 4096, 256, n=3) == (DUP, 1, M_LAT, 0, 3, 32, 0, 3, 10240)
    assert shape(L, c, 4096, 256, n=1025) == (DUP, 2, M_LAT, 0, 1025, 32, 0, 1025, 10240)
    assert shape(L, c, 4096, 256, dup=64, n=3) == (DUP, 1, M_LAT, 0, 3, 64, 0, 3, 10240)
    # no duplicate lanes: the one-lane kernel, same register clamp
    for dup in (1, 65, 0, -1):
        assert shape(L, c, 4096, 256, dup=dup) == (LDS, 4, M_LAT, 0, 4096, 1, 0, 4096, 10240)
        assert shape(L, c, 4096, 256, dup=dup, n=3) == (LDS, 1, M_LAT, 0, 3, 1, 0, 3, 10240)
    c.waves_per_simd = 2
    assert shape(L, c, 4096, 256)[:2] == (DUP, 2)


def test_latency_two_lanes(L):
    # widened waves: the plan's W although one workgroup is resident
    c = cls(L, M_LAT, 2, 638, 16, 4, 3, K2)
    assert shape(L, c, 4096, 256) == (LDS, 4, M_LAT, 1, 2, 2, 0, 4, 10240)


def test_slot_global(L):
    # lc4/pb4 without the slot trees: 5,062 cells = 10,124 B, 8 blocks, 16 per CU
    c = cls(L, M_SG, 1, 5062, 16, 4, 4097)
    assert shape(L, c, 4096, 256) == (DUP, 4, M_SG, 0, 4096, 32, 0, 4096, 10240)
    assert shape(L, c, 4096, 256, n=15) == (DUP, 1, M_SG, 0, 15, 32, 0, 15, 10240)
    for dup in (1, 0, 65):
        assert shape(L, c, 4096, 256, dup=dup) is None
    c.lanes_per_group = 2
    assert shape(L, c, 4096, 256) is None


def test_cooperative_latency_placement(L):
    c = cls(L, M_LAT | COOP, 1, 638, 16, 4, 32)
    # 8 resident workgroups per CU: W 2; 9: W 4.  LDS padded to the share
    assert shape(L, c, 64, 4) == (COOPK, 2, M_LAT | COOP, 0, 32, 32, 0, 32, 10240)
    assert shape(L, c, 64, 4, n=33) == (COOPK, 4, M_LAT | COOP, 0, 33, 32, 0, 33, 10240)
    assert shape(L, c, 16, 4, n=33) == (COOPK, 4, M_LAT | COOP, 0, 16, 32, 0, 16, 10240)
    # the class's own W is not read
    c.waves_per_simd = 1
    assert shape(L, c, 64, 4)[1] == 2


def test_cooperative_whole_table_and_window(L):
    # an lc + lp = 4, pb = 4 slice: 5,316 cells as an odd dword count
    stride = 5318
    table, tb = stride * 2, (stride * 2 + 15) & ~15
    c = cls(L, M_ALL | COOP, 1, stride, 16, 4, 1, K2)
    # one stream: the CU's LDS to itself, the largest window
    assert shape(L, c, 4096, 256) == (COOPK, 2, M_ALL | COOP | WIN, 1, 1, 32, 131072, 1,
                                      tb + 131072)
    # 1,024 streams on 256 CUs: 4 per CU share 40,960 B each -> 16 KiB
    c = cls(L, M_ALL | COOP, 1, stride, 14, 4, 1024)
    assert shape(L, c, 14 * 256, 256) == (COOPK, 2, M_ALL | COOP | WIN, 0, 1024, 32, 16384, 1024,
                                          tb + 16384)
    # 11 per CU: the share, 11 blocks = 14,080 B, is within 4 KiB of the table
    c = cls(L, M_ALL | COOP, 1, stride, 11, 4, 11 * 256)
    assert shape(L, c, 11 * 256, 256) == (COOPK, 4, M_ALL | COOP, 0, 2816, 32, 0, 2816, 14080)
    # windows off: the plain build, the table (above the share of 16) unpadded
    c = cls(L, M_ALL | COOP, 1, stride, 16, 4, 1)
    assert shape(L, c, 4096, 256, win_off=1) == (COOPK, 2, M_ALL | COOP, 0, 1, 32, 0, 1, table)


def test_unknown_masks(L):
    for mask in (M_ALL, M_LAT | ILV, M_ALL | COOP | WIN, M_SG | COOP, 0):
        assert shape(L, cls(L, mask, 1, 638, 16, 4, 3, slot_groups=8), 4096, 256) is None
    # nothing to launch, and no lanes, are no shape either
    assert shape(L, cls(L, M_LAT, 1, 638, 16, 4, 0), 4096, 256) is None
    assert shape(L, cls(L, M_LAT, 0, 638, 16, 4, 3), 4096, 256) is None


def test_session_cooperative(L):
    SESS = M_ALL | COOP
    assert session_shape(L, 4, 0, 0, 256) is None
    assert session_shape(L, 4, 81921, 0, 256) is None          # above a CU's 160 KiB
    assert session_shape(L, 1, 81920, 0, 256) == (COOPK, 0, SESS, 0, 1, 32, 0, 1, 163840)
    # lc0/lp0/pb0 whole table: 1,774 cells = 3,548 B
    assert session_shape(L, 1, 1774, 0, 256) == (COOPK, 0, SESS | WIN, 0, 1, 32, 131072, 1,
                                                 3552 + 131072)
    assert session_shape(L, 10, 1774, 4, 256)[4] == 4          # grid capped
    # no cap on the workgroups per CU: 40 of them share 3 blocks each, no room
    # for a window and no padding -- a decode class of 16 per CU gets 4 KiB
    assert session_shape(L, 10240, 1774, 0, 256) == (COOPK, 0, SESS, 0, 10240, 32, 0, 10240, 3548)
    c = cls(L, M_ALL | COOP, 1, 1774, 16, 4, 10240)
    assert shape(L, c, 0, 256)[6] == 4096
    assert session_shape(L, 1, 1774, 0, 256, win_off=1) == (COOPK, 0, SESS, 0, 1, 32, 0, 1, 3548)


# ---------------------------------------------------------------- the header under sanitizers

@pytest.fixture(scope="module")
def program_lines(tmp_path_factory, golden):
    d = tmp_path_factory.mktemp("decodeplan")
    exe = str(d / "decode_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-O1", "-g",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-DLZGPU_HOST_EMU", "-I", CSRC, SRC, "-o", exe], check=True)

    def item(it):
        kind, props = it
        return "%d %d %s" % (kind, len(props), " ".join(str(b) for b in props.ljust(5, b"\0")))

    path = str(d / "cases.txt")
    with open(path, "w") as f:
        for c in golden:
            o = c["opt"]
            pat, tail = C.SETS[c["set"]]
            opts = " ".join(str(o.get(k, 0)) for k in
                            ("cus", "kernel", "lanes_per_group", "groups_per_cu", "waves_per_simd",
                             "persistent", "coop", "one_class", "flags"))
            items = pat + ([tail] if tail else [])
            f.write("%d %s %d %d %s\n" % (c["n"], opts, len(pat), len(items) - len(pat),
                                          " ".join(item(it) for it in items)))
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(golden)
    return lines


def _crc(v, dt):
    return v if isinstance(v, int) else zlib.crc32(np.asarray(v, dtype=dt).tobytes())


def test_program_plans_equal_the_golden(golden, program_lines):
    for c, line in zip(golden, program_lines):
        res, plan, crcs, _ = line.split("|")
        assert int(res) == c["res"] and [int(v) for v in plan.split()] == c["plan"], (c["set"], c["n"], c["opt"])
        assert [int(v) for v in crcs.split()] == [_crc(c["probs"], "<u8"), _crc(c["order"], "<u4")]


def test_program_shapes_equal_the_librarys(L, golden, program_lines):
    rows = set()
    for c, line in zip(golden, program_lines):
        p, cus = c["plan"], c["opt"]["cus"]
        shapes = [s.strip() for s in line.split("|")[3].split(";")][:-1]
        assert len(shapes) == p[9]
        for k, text in enumerate(shapes):
            f = p[10 + 10 * k:20 + 10 * k]
            lc = L.LdsClass()
            (lc.n, lc.lanes_per_group, lc.lds_cells_per_lane, lc.groups_per_cu, lc.waves_per_simd,
             lc.lds_mask, lc.flags, lc.slot_off, lc.slot_cells, lc.slot_groups) = f
            want = shape(L, lc, cus * f[3] if p[8] else 0, cus)
            assert want is not None                   # every planned class has a kernel
            assert tuple(int(v) for v in text.split()) == want, (c["set"], c["n"], c["opt"], k)
            rows.add(want[:4])
    assert rows <= TABLE
    # all seven placements the launcher knows, the window bit added at launch
    assert {r[2] for r in rows} == C.PLAN_MASKS | {M_ALL | COOP | WIN}


# ---------------------------------------------------------------- every row on the GPU

def _row_cases():
    """(row, props byte, streams as a function of the CU count, options): options
    that reach the row on a device of any CU count.  W of a one-stream launch
    follows the workgroups resident per CU: 1-4 -> 1, 5-8 -> 2, above -> 4."""
    def few(cus):
        return 3

    def per_cu(k):                        # k + 1 streams on the fullest CU
        return lambda cus: k * cus + 1

    out = []
    for k2 in (0, 1):
        fl = 2 if k2 else 0               # LZMA_GPU_PLAN_KERNEL_LZMA2
        for w in (1, 2, 4):
            out += [((LDS, w, M_THR | ILV, k2), 0x00, few,
                     dict(kernel=1, waves_per_simd=w, flags=fl)),
                    ((LDS, w, M_THR, k2), 0x00, few,
                     dict(kernel=1, waves_per_simd=w, flags=fl | 16)),       # NO_ILV
                    ((LDS, w, M_LAT, k2), 0x00, few,
                     dict(kernel=2, waves_per_simd=w, lanes_per_group=2, flags=fl))]
        # one-stream waves: lc0/pb0 keeps its slot trees in LDS (16 workgroups per
        # CU fit); lc4/pb4 planned for one CU puts them in the global rows
        for w, n in ((1, few), (2, per_cu(4)), (4, per_cu(8))):
            out += [((DUP, w, M_LAT, k2), 0x00, n, dict(kernel=2, flags=fl)),
                    ((DUP, w, M_SG, k2), 0xb8, n if w > 1 else (lambda cus: 15),
                     dict(kernel=2, cus=1, flags=fl))]
        out += [((COOPK, 2, M_LAT | COOP, k2), 0x00, few, dict(kernel=3, flags=fl | 4)),  # COOP_LAT
                ((COOPK, 4, M_LAT | COOP, k2), 0x00, per_cu(9), dict(kernel=3, flags=fl | 4)),
                # a narrow table always leaves room for a window ...
                ((COOPK, 2, M_ALL | COOP | WIN, k2), 0x00, few, dict(kernel=3, flags=fl)),
                ((COOPK, 4, M_ALL | COOP | WIN, k2), 0x00, per_cu(9), dict(kernel=3, flags=fl)),
                # ... lc4/pb4 (28,268 B, 5 per CU) and lc3 (14,300 B, 10 per CU) none
                # once their workgroups fill the CU
                ((COOPK, 2, M_ALL | COOP, k2), 0xb8, per_cu(4), dict(kernel=3, flags=fl)),
                ((COOPK, 4, M_ALL | COOP, k2), 0x03, per_cu(9), dict(kernel=3, flags=fl))]
    return out


ROW_CASES = _row_cases()


def test_row_cases_are_the_table():
    assert sorted(r for r, _, _, _ in ROW_CASES) == sorted(TABLE)


_STREAMS = {}


def _streams(b0):
    """Three streams of the props byte (256, 64 and 64 bytes of text) and what the
    oracle decodes them to."""
    if b0 not in _STREAMS:
        lc, lp, pb = b0 % 9, b0 // 9 % 5, b0 // 45
        props = bytes([b0, 0, 0, 1, 0])
        orc, out = native.oracle(), []
        for k, size in enumerate((256, 64, 64)):
            data = native.gen("text", 4200 + k, size)
            comp = lzma.compress(data, format=lzma.FORMAT_RAW,
                                 filters=[{"id": lzma.FILTER_LZMA1, "dict_size": 1 << 16, "lc": lc,
                                           "lp": lp, "pb": pb, "preset": 6}])
            want = native.decode(orc, "orc", comp, props, size, 1)
            assert want[4] == data
            out.append((comp, size, want))
        _STREAMS[b0] = (props, out)
    return _STREAMS[b0]


@pytest.mark.gpu
@pytest.mark.timeout(60)
@pytest.mark.parametrize("row,b0,count,opt", ROW_CASES,
                         ids=["%s-w%d-%x-k%d" % ("lds dup coop".split()[r[0]], r[1], r[2], r[3])
                              for r, _, _, _ in ROW_CASES])
def test_every_table_row_launches(L, row, b0, count, opt):
    import torch
    assert L.device_count() > 0, L.last_error()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = count(cus)
    props, pool = _streams(b0)
    # a few streams: all three; a large batch: the two 64-byte ones
    pick = [i % 3 if n <= 16 else 1 + i % 2 for i in range(n)]
    src_off = np.cumsum([0] + [len(c) for c, _, _ in pool])
    dst_off = np.cumsum([0] + [pool[k][1] for k in pick])
    descs = (L.StreamDesc * n)()
    arr = np.frombuffer(descs, dtype=np.uint8).reshape(n, 48)
    u64 = arr[:, :40].view(np.uint64)
    u64[:, 0] = src_off[pick]
    u64[:, 1] = [len(pool[k][0]) for k in pick]
    u64[:, 2] = dst_off[:-1]
    u64[:, 3] = [pool[k][1] for k in pick]
    arr[:, 40:48] = list(props) + [5, 1, 0]
    plan = L.Plan()
    r, res, dst = L.decode_batch_host(descs, b"".join(c for c, _, _ in pool), int(dst_off[-1]),
                                      C.options(L, opt), plan)
    assert r == 0, L.last_error()
    # the row this plan launched, by the launcher's own shape function (device
    # CUs, process environment)
    assert plan.n_classes == 1 and plan.n_lds == n
    c = plan.classes[0]
    s = Shape()
    assert L.lib.lzgpu_decode_launch_shape(ctypes.byref(c), n, cus * c.groups_per_cu
                                           if plan.persistent else 0, 0, None, ctypes.byref(s))
    assert s.astuple()[:4] == row, (s.astuple(), n, cus)
    got = np.frombuffer(res, dtype=np.dtype([("res", "<i4"), ("status", "<i4"),
                                             ("dest_len", "<u8"), ("src_len", "<u8")]))[:n]
    for k in range(3):
        want = pool[k][2]
        sel = np.flatnonzero(np.asarray(pick) == k)
        g = got[sel]
        assert ((g["res"] == want[0]) & (g["status"] == want[1]) & (g["dest_len"] == want[2]) &
                (g["src_len"] == want[3])).all(), (k, g[:4], want[:4])
    out = np.frombuffer(dst, dtype=np.uint8)
    for i in range(n):
        data = pool[pick[i]][2][4]
        assert out[dst_off[i]:dst_off[i + 1]].tobytes() == data, i

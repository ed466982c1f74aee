"""Recipes that put the hand-made decoder corners on every build of the kernel
table (tests/test_handmade_rows.py).

The batch decoder is 42 separately compiled kernels, (family, W, placement, K2)
in csrc/lzma_kernels.hip, and which one a class of a plan launches is decided
by csrc/decode_plan.h's decode_launch_shape: from the class's placement, its
planned waves_per_simd, LZMA_GPU_CLASS_HAS_LZMA2 and, for one-stream
workgroups, the workgroups resident per CU, min(groups_per_cu, ceil(n / CUs)).
tests/test_gpu_kernels.py forces placements; a recipe here forces a row: plan
options and how many streams a launch may hold, as multiples of the device's
CU count, for each class of inputs the planner can put on that row.

Classes of inputs: the hand-made LZMA cases of tests/handmade_cases.py by props
byte -- "00" (lc0 lp0 pb0), "5d" (lc3 lp0 pb2), "d8" (lc0 lp4 pb4) -- and "l2",
the hand-made LZMA2 cases as kind = 1 items; both finish modes, the short
inputs at the 16 source alignments.  The reference-decoded vectors of
tests/golden/cases.json with the same props byte ride with their class, the
LZMA2 ranges with a valid dictionary byte with "l2" (the range with byte 41 and
the two vectors with four props bytes are no LDS items: the planner sends them
to the generic kernel).

A class is cut into launches of the size its recipe allows; where the device
has so many CUs that a launch would be too small it is filled up by cycling
through its own hand-made items.
"""
import ctypes

import numpy as np

import golden_cases as G
import handmade_cases as H
from test_decode_plan import (COOP, COOPK, DUP, ILV, LDS, M_ALL, M_LAT, M_SG, M_THR, TABLE, WIN,
                              Env, Shape)

CLASSES = ("00", "5d", "d8", "l2")
# items of H.items() per class, golden riders per class
HANDMADE_COUNT = {"00": 2918, "5d": 2918, "d8": 2886, "l2": 656}
GOLDEN_COUNT = {"00": 81, "5d": 133, "d8": 0, "l2": 19}
LDS_BYTES_PER_CU = 160 * 1024

KERNEL_LZMA2, COOP_LAT, NO_ILV, ILV_ANY, NO_SLOTG = 2, 4, 16, 32, 256   # LZMA_GPU_PLAN_*
THROUGHPUT, LATENCY, COOPERATIVE = 1, 2, 3                               # LZMA_GPU_KERNEL_*


def row_id(row):
    return "%s-w%d-%x-k%d" % ("lds dup coop".split()[row[0]], row[1], row[2], row[3])


# The rows and the classes each is given, as decided by host planning (the
# recipes below are checked against it at 64, 104, 256 and 304 CUs).  K2 = 0
# builds refuse LZMA2 items; on K2 = 1 rows the LZMA classes run the build with
# the chunk walker under LZMA_GPU_PLAN_KERNEL_LZMA2.  Interleaved rows hold
# whole 32-lane groups only for the narrow "00" table; under
# LZMA_GPU_PLAN_ILV_ANY "5d" gets there with 4 lanes (a 32-lane row of its
# slices is 137,344 bytes of LDS), "d8" and "l2" do not: a row of theirs, 277,632
# bytes, is more than a CU has, and the planner keeps their per-lane slices.  So
# the three interleaved K2 = 1 builds see no real LZMA2 item.  The slot trees
# go global (0x19f) only for tables too wide for 16 workgroups per CU.
# With every section in LDS and no window, W = 2 is the five 28,268-byte tables
# a CU holds ("d8", "l2") and W = 4 the ten of 14,300 bytes ("5d"); the narrow
# table always leaves room for a window, and only it leaves room at W = 4.
ROW_CLASSES = {
    "lds-w1-105-k0": "00 5d d8",
    "lds-w2-105-k0": "00 5d d8",
    "lds-w4-105-k0": "00 5d d8",
    "lds-w1-105-k1": "00 5d d8 l2",
    "lds-w2-105-k1": "00 5d d8 l2",
    "lds-w4-105-k1": "00 5d d8 l2",
    "lds-w1-40000105-k0": "00 5d",
    "lds-w2-40000105-k0": "00 5d",
    "lds-w4-40000105-k0": "00 5d",
    "lds-w1-40000105-k1": "00 5d",
    "lds-w2-40000105-k1": "00 5d",
    "lds-w4-40000105-k1": "00 5d",
    "lds-w1-1bf-k0": "00 5d d8",
    "lds-w2-1bf-k0": "00 5d d8",
    "lds-w4-1bf-k0": "00 5d d8",
    "lds-w1-1bf-k1": "00 5d d8 l2",
    "lds-w2-1bf-k1": "00 5d d8 l2",
    "lds-w4-1bf-k1": "00 5d d8 l2",
    "dup-w1-1bf-k0": "00 5d d8",
    "dup-w2-1bf-k0": "00 5d d8",
    "dup-w4-1bf-k0": "00 5d d8",
    "dup-w1-1bf-k1": "00 5d d8 l2",
    "dup-w2-1bf-k1": "00 5d d8 l2",
    "dup-w4-1bf-k1": "00 5d d8 l2",
    "dup-w1-19f-k0": "d8",
    "dup-w2-19f-k0": "d8",
    "dup-w4-19f-k0": "d8",
    "dup-w1-19f-k1": "d8 l2",
    "dup-w2-19f-k1": "d8 l2",
    "dup-w4-19f-k1": "d8 l2",
    "coop-w2-800001bf-k0": "00 5d d8",
    "coop-w4-800001bf-k0": "00 5d d8",
    "coop-w2-800001bf-k1": "00 5d d8 l2",
    "coop-w4-800001bf-k1": "00 5d d8 l2",
    "coop-w2-880007ff-k0": "00 5d d8",
    "coop-w4-880007ff-k0": "00",
    "coop-w2-880007ff-k1": "00 5d d8 l2",
    "coop-w4-880007ff-k1": "00",
    "coop-w2-800007ff-k0": "d8",
    "coop-w4-800007ff-k0": "5d",
    "coop-w2-800007ff-k1": "d8 l2",
    "coop-w4-800007ff-k1": "5d",
}


def _recipes():
    """{(family, W, placement): {class: (options, more, most, least)}}: a launch
    of the class under the options runs the row when it holds more than
    more * CUs, at most most * CUs (0: no limit) and at least `least` streams."""
    def every(opt, more=0, most=0, names=CLASSES, least=1):
        return {c: (opt, more, most, least) for c in names}

    out = {}
    for w in (1, 2, 4):
        # the W of a many-lane workgroup is the plan's waves_per_simd
        out[LDS, w, M_THR | ILV] = dict(
            every(dict(kernel=THROUGHPUT, waves_per_simd=w), names=("00",)),
            **every(dict(kernel=THROUGHPUT, waves_per_simd=w, flags=ILV_ANY), names=("5d",)))
        out[LDS, w, M_THR] = every(dict(kernel=THROUGHPUT, waves_per_simd=w, flags=NO_ILV))
        out[LDS, w, M_LAT] = every(dict(kernel=LATENCY, waves_per_simd=w, lanes_per_group=2))
    # one-stream workgroups: W by the workgroups resident per CU, 1-4 -> 1,
    # 5-8 -> 2, above -> 4
    out[DUP, 1, M_LAT] = every(dict(kernel=LATENCY, groups_per_cu=4))
    out[DUP, 2, M_LAT] = every(dict(kernel=LATENCY, groups_per_cu=8), 4)
    out[DUP, 4, M_LAT] = every(dict(kernel=LATENCY, flags=NO_SLOTG), 8)
    # planned for one CU the wide tables have more streams than resident
    # workgroups (above 14), which is what sends the slot trees to the global rows
    for w, more, most in ((1, 0, 4), (2, 4, 8), (4, 8, 0)):
        out[DUP, w, M_SG] = every(dict(kernel=LATENCY, cus=1), more, most, ("d8", "l2"), least=15)
    out[COOPK, 2, M_LAT | COOP] = every(dict(kernel=COOPERATIVE, flags=COOP_LAT), 0, 8)
    out[COOPK, 4, M_LAT | COOP] = every(dict(kernel=COOPERATIVE, flags=COOP_LAT), 8)
    coop = dict(kernel=COOPERATIVE)
    # a window needs 4 KiB of the workgroup's LDS share behind the table
    out[COOPK, 2, M_ALL | COOP | WIN] = dict(every(coop, 0, 8, ("00", "5d")),
                                             **every(coop, 0, 4, ("d8", "l2")))
    out[COOPK, 4, M_ALL | COOP | WIN] = every(coop, 8, 0, ("00",))
    out[COOPK, 2, M_ALL | COOP] = every(coop, 4, 5, ("d8", "l2"))
    out[COOPK, 4, M_ALL | COOP] = every(coop, 9, 10, ("5d",))
    return out


RECIPES = _recipes()


def recipe(row, name):
    """(options, more, most, least) of class `name` on the row, or None.  An
    LZMA2 item is refused by the K2 = 0 builds and makes its class K2 = 1 by
    itself; the LZMA classes reach the K2 = 1 builds by the plan flag."""
    r = RECIPES[row[:3]].get(name)
    if r is None or (name == "l2" and not row[3]):
        return None
    opt = dict(r[0])
    if row[3] and name != "l2":
        opt["flags"] = opt.get("flags", 0) | KERNEL_LZMA2
    return (opt,) + r[1:]


def rows():
    return sorted(TABLE)


def classes_of(row):
    return [c for c in CLASSES if recipe(row, c) is not None]


def launch_sizes(total, cus, more, most, least=1):
    """[(items, streams)]: `total` items cut into the fewest launches of at most
    most * cus, evenly; a launch below the recipe's minimum is filled up to it."""
    lo, hi = max(more * cus + 1, least), most * cus
    assert hi == 0 or lo <= hi
    k = -(-total // hi) if hi else 1
    base, extra = divmod(total, k)
    return [(base + (i < extra), max(base + (i < extra), lo)) for i in range(k)]


# ---------------------------------------------------------------- the classes' items

_C = {}


def class_name(case):
    return "l2" if case["kind"] == "lzma2" else "%02x" % case["props"][0]


def handmade():
    """{class: [(case, finish, align)]} of H.items()."""
    if "hm" not in _C:
        out = {c: [] for c in CLASSES}
        for it in H.items():
            out[class_name(it[0])].append(it)
        _C["hm"] = out
    return _C["hm"]


def goldens():
    """{class: [golden]}: a rider is a dict of its descriptor fields (src, props,
    cap, finish, kind) and the reference's recorded (row, sha256, note)."""
    if "gold" not in _C:
        d = G.load()
        out = {c: [] for c in CLASSES}
        for _, c in G.cases("lzma"):
            name = c["props"][:2]
            if name in ("00", "5d", "d8") and len(c["props"]) == 10:
                out[name].append((c, bytes.fromhex(c["props"]), 0))
        for _, c in G.cases("lzma2"):
            if c["prop"] <= 40:
                out["l2"].append((c, bytes([c["prop"]]), 1))
        for name in out:
            out[name] = [dict(src=G.case_input(d, c), props=props, kind=kind, cap=c["dest_cap"],
                              finish=c["finish"], note=c["note"], sha256=c["expect"]["sha256"],
                              row=tuple(c["expect"][k] for k in ("res", "status", "dest_len",
                                                                 "src_len")))
                         for c, props, kind in out[name]]
        _C["gold"] = out
    return _C["gold"]


def launches(name, cus, more, most, least=1):
    """The class cut for a device of `cus` CUs: per launch (indices of hand-made
    items, the cycled ones behind the launch's own, indices of golden riders).
    The riders follow the hand-made items, so they end up in the last launches."""
    n_hm, n_gold = len(handmade()[name]), len(goldens()[name])
    out, at = [], 0
    for items, streams in launch_sizes(n_hm + n_gold, cus, more, most, least):
        hm = list(range(at, min(at + items, n_hm)))
        gold = list(range(max(at, n_hm) - n_hm, at + items - n_hm))
        assert hm, "a launch of riders alone has nothing small to be filled up with"
        hm += [hm[i % len(hm)] for i in range(streams - items)]
        out.append((hm, gold))
        at += items
    return out


def batch(name, hm, gold):
    """(hand-made items, riders, descriptor dicts, source, destination bytes) of a
    launch: H.batch of the hand-made items, the riders behind them."""
    its = [handmade()[name][i] for i in hm]
    riders = [goldens()[name][i] for i in gold]
    descs, src, doff = H.batch(its)
    src = bytearray(src)
    for g in riders:
        descs.append(dict(src_off=len(src), src_len=len(g["src"]), dst_off=doff, dst_cap=g["cap"],
                          props=g["props"], finish=g["finish"], kind=g["kind"]))
        src += g["src"]
        doff += g["cap"]
    return its, riders, descs, bytes(src) + bytes(16), doff


def rider_leaves_tail(g):
    """Riders for which [dest_len, cap) is not the poison's, by their recorded
    answer.  SZ_ERROR_DATA: the reference's own LzmaDecode has written the
    symbols before the bad one and reports the dicPos of the pass's start (28
    of the "5d" and 6 of the "00" vectors, seen with the live reference over a
    poisoned buffer).  NEEDS_MORE_INPUT: the one-shot decoders take the last
    < 20 input bytes in one bulk pass and decode a truncated end again exactly
    (lz_decode_to_dic's fast tail), so symbols the reference's probe refuses
    have been written inside the capacity.  The streams behind them in the
    batch are checked from their first byte, so nothing passes a capacity."""
    return g["row"][0] == 1 or g["row"][1] == 3


def rider_mismatches(riders, descs, res, dst, poison):
    """The riders' result rows and output against the recorded reference answers;
    descs and res are theirs alone."""
    bad = []
    for g, d, r in zip(riders, descs, res):
        got = (r.res, r.status, r.dest_len, r.src_len)
        at = d["dst_off"]
        if got != g["row"] or got[2] > g["cap"] or G.sha(dst[at:at + got[2]]) != g["sha256"]:
            bad.append((g["note"], g["finish"], got, g["row"]))
        elif not rider_leaves_tail(g) and dst[at + got[2]:at + g["cap"]].strip(bytes([poison])):
            bad.append((g["note"], g["finish"], "wrote behind dest_len", got))
    return bad


# ---------------------------------------------------------------- planning on the host

def plan_descs(L, name):
    """The class's descriptors, hand-made items then riders, as an (n, 48) byte
    array to pick a launch's rows from: all the planner reads of an item is its
    kind, props, src_len and dst_cap."""
    if ("descs", name) not in _C:
        n_hm, n_gold = len(handmade()[name]), len(goldens()[name])
        descs = batch(name, range(n_hm), range(n_gold))[2]
        _C["descs", name] = np.frombuffer(L.make_descs(descs), dtype=np.uint8).reshape(-1, 48).copy()
    return _C["descs", name]


def launched_row(L, plan, cus, env=None):
    """(family, W, placement, K2) and LDS bytes of each class of the plan by the
    launcher's own shape function and group cap, on a device of `cus` CUs: with
    the environment `env`, or (None) as the library itself reads the device's
    CUs and the process environment."""
    out = []
    for k in range(plan.n_classes):
        c = plan.classes[k]
        s = Shape()
        max_groups = cus * c.groups_per_cu if plan.persistent else 0
        ok = L.lib.lzgpu_decode_launch_shape(ctypes.byref(c), int(c.n), max_groups,
                                             cus if env is not None else 0,
                                             ctypes.byref(env) if env is not None else None,
                                             ctypes.byref(s))
        out.append((s.astuple()[:4], s.lds_bytes) if ok else (None, 0))
    return out


def host_env():
    """The launcher's defaults: 32 lanes per one-stream wave, windows on."""
    return Env(32, 0)

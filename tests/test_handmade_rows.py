"""The hand-made decoder corners through every build of the kernel table.

tests/test_gpu_kernels.py sends the hand-made streams (tests/handmade_cases.py)
and the golden vectors through each PLACEMENT; which of the 42 builds of
csrc/lzma_kernels.hip's table a class then launches follows its planned
waves_per_simd, its LZMA2 flag and, for one-stream workgroups, the batch size
against the device's CU count.  Planned on the host for a 256-CU device that
module's hand-made batch reaches 9 of the 42 rows (test_gpu_kernels_reach_nine_
rows below keeps the record); tests/test_decode_plan.py launches all 42, with
three streams of plain text each.  The builds are separate compilations -- W is
the register budget: a W = 4 cooperative build spills where W = 2 does not --
so here every row gets every hand-made class the planner can put on it
(tests/handmade_rows.py: ROW_CLASSES, the recipes), with the golden vectors of
the same props byte riding along.

Without a GPU: the recipes reach their rows when planned for 64, 104, 256 and
304 CUs, the rows are the whole table, the row-to-classes table is the
committed one, and the record of the finding.
On the GPU, per row: every launch's plan is one class whose shape, by the
launcher's own function with the device's CUs and the process environment, is
the row; every result row and output byte equals the reference's over a
destination filled with 0xA5, nothing written behind a stream's dest_len or
behind the batch; and the row has seen every item and every group of every
class it is given.
"""
import numpy as np
import pytest

import decode_plan_cases as C
import handmade_cases as H
import handmade_rows as R
import test_gpu_kernels as K
from test_decode_plan import COOP, COOPK, DUP, ILV, LDS, M_ALL, M_LAT, M_SG, M_THR, TABLE, WIN

ROWS = R.rows()
IDS = [R.row_id(r) for r in ROWS]


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


# ---------------------------------------------------------------- without a GPU

def test_row_table_is_the_committed_one():
    assert set(ROWS) == TABLE and len(ROWS) == 42
    assert {R.row_id(r): " ".join(R.classes_of(r)) for r in ROWS} == R.ROW_CLASSES
    # every row has a class, every K2 = 1 row its K2 = 0 twin's LZMA classes
    for r in ROWS:
        assert R.classes_of(r)
        if r[3]:
            assert [c for c in R.classes_of(r) if c != "l2"] == R.classes_of(r[:3] + (0,))
    # real LZMA2 items on the 16 K2 = 1 rows host planning gives them
    l2 = {r[:3] for r in ROWS if "l2" in R.classes_of(r)}
    assert l2 == ({(LDS, w, m) for w in (1, 2, 4) for m in (M_THR, M_LAT)} |
                  {(DUP, w, m) for w in (1, 2, 4) for m in (M_LAT, M_SG)} |
                  {(COOPK, 2, M_LAT | COOP), (COOPK, 4, M_LAT | COOP),
                   (COOPK, 2, M_ALL | COOP | WIN), (COOPK, 2, M_ALL | COOP)})


def test_classes_are_the_whole_handmade_set():
    hm, gold = R.handmade(), R.goldens()
    assert {c: len(v) for c, v in hm.items()} == R.HANDMADE_COUNT
    assert sum(R.HANDMADE_COUNT.values()) == len(H.items()) == 9378
    assert {c: len(v) for c, v in gold.items()} == R.GOLDEN_COUNT
    for name in R.CLASSES:
        want = H.LZMA2_GROUPS if name == "l2" else H.LZMA_GROUPS
        assert {it[0]["group"] for it in hm[name]} == set(want)


@pytest.mark.parametrize("cus", (64, 104, 256, 304))
def test_recipes_reach_their_rows(L, cus):
    """Every launch of every class of every row, planned for `cus` CUs (the
    0x19f recipes for one, as on the device) and resolved by the launcher's
    shape function for a device of that many."""
    env = R.host_env()
    reached = set()
    for row in ROWS:
        for name in R.classes_of(row):
            opt, more, most, least = R.recipe(row, name)
            po = C.options(L, dict(dict(cus=cus), **opt))
            arr = R.plan_descs(L, name)
            n_hm = R.HANDMADE_COUNT[name]
            seen = set()
            for hm, gold in R.launches(name, cus, more, most, least):
                idx = np.asarray(hm + [n_hm + g for g in gold])
                seen.update(idx.tolist())
                descs = (L.StreamDesc * len(idx)).from_buffer_copy(arr[idx].tobytes())
                plan, _ = L.plan_ex(descs, po)
                assert plan.n_classes == 1 and plan.n_lds == len(idx), (R.row_id(row), name, cus)
                (got, lds_bytes), = R.launched_row(L, plan, cus, env)
                assert got == row, (R.row_id(row), name, cus, len(idx), got)
                assert plan.classes[0].lds_mask == row[2] & ~WIN
                assert 0 < lds_bytes <= R.LDS_BYTES_PER_CU
            assert seen == set(range(len(arr)))       # no item left out
            reached.add(row)
    assert reached == TABLE


def test_ilv_any_keeps_slices_where_a_row_exceeds_lds(L):
    """Found by the recipes: interleaved LDS slices take whole 32-lane rows, and
    under LZMA_GPU_PLAN_ILV_ANY the planner gave the 2-lane workgroups of the
    lc + lp = 4 tables ("d8", every LZMA2 item) such rows, 32 x 8,676 = 277,632
    bytes of LDS per workgroup, which no launch can have.  They keep their
    per-lane slices; "5d" (4 lanes, 137,344 bytes) is interleaved."""
    for name, mask in (("00", M_THR | ILV), ("5d", M_THR | ILV), ("d8", M_THR), ("l2", M_THR)):
        arr = R.plan_descs(L, name)
        descs = (L.StreamDesc * len(arr)).from_buffer_copy(arr.tobytes())
        for cus in (64, 256):
            plan, _ = L.plan_ex(descs, C.options(L, dict(kernel=R.THROUGHPUT, cus=cus,
                                                         flags=R.ILV_ANY)))
            assert plan.n_classes == 1 and plan.classes[0].lds_mask == mask, name
            (got, lds_bytes), = R.launched_row(L, plan, cus, R.host_env())
            assert got is not None and got[2] == mask and lds_bytes <= R.LDS_BYTES_PER_CU


# the rows tests/test_gpu_kernels.py's hand-made batch reaches under each of its
# forced placements, planned as that module plans and launched on 256 CUs: the
# finding this module answers.  Computed on the host, as below.
NINE_ROWS = {
    (LDS, 2, M_THR | ILV, 0), (LDS, 1, M_THR | ILV, 0), (LDS, 2, M_THR, 0), (LDS, 2, M_THR, 1),
    (LDS, 1, M_THR, 1),
    (DUP, 4, M_SG, 1),
    (COOPK, 4, M_ALL | COOP | WIN, 0), (COOPK, 4, M_LAT | COOP, 0), (COOPK, 4, M_LAT | COOP, 1),
}


def test_gpu_kernels_reach_nine_rows(L):
    """If the planner or test_gpu_kernels._opts change, this record changes with
    them: say so where it is updated."""
    its = H.items()
    descs = L.make_descs(H.batch(its)[0])
    rows = set()
    for kernel in K.KERNELS:
        plan, _ = L.plan_ex(descs, K._opts(L, kernel))
        if kernel == "global":
            assert plan.n_classes == 0
            continue
        got = [r for r, _ in R.launched_row(L, plan, 256, R.host_env())]
        assert None not in got and plan.n_lds == len(its)
        rows.update(got)
    assert rows == NINE_ROWS and len(NINE_ROWS) == 9


# ---------------------------------------------------------------- every row on the GPU

@pytest.fixture(scope="module")
def expected():
    """The reference's answers for every hand-made item, looked up once."""
    for c, finish, _ in H.items():
        H.expected(c, finish)
    return R.handmade(), R.goldens()


@pytest.mark.gpu
@pytest.mark.timeout(60)
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_handmade_through_each_row(L, expected, row):
    import torch
    assert L.device_count() > 0, L.last_error()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    hm_all, gold_all = expected
    names = R.classes_of(row)
    assert " ".join(names) == R.ROW_CLASSES[R.row_id(row)]
    for name in names:
        opt, more, most, least = R.recipe(row, name)
        seen_hm, seen_gold = set(), set()
        for hm, gold in R.launches(name, cus, more, most, least):
            its, riders, items, src, dst_bytes = R.batch(name, hm, gold)
            n = len(items)
            plan, res, d_dst = K._device_decode(L, torch, L.make_descs(items),
                                                np.frombuffer(src, np.uint8), dst_bytes,
                                                C.options(L, opt), fill=0xA5)
            # the row this launch ran: one class, the launcher's own shape with
            # the device's CUs and the process environment
            assert plan.n_classes == 1 and plan.n_lds == n and plan.classes[0].n == n
            (got, _), = R.launched_row(L, plan, cus)
            assert got == row, (R.row_id(row), name, n, cus, got)
            out = d_dst.cpu().numpy().tobytes()
            rows = [L.Result(int(x["res"]), int(x["status"]), int(x["dest_len"]), int(x["src_len"]))
                    for x in res]
            bad = H.mismatches(its, items, rows, out, poison=0xA5)
            assert not bad, (R.row_id(row), name, len(bad), bad[:8])
            bad = R.rider_mismatches(riders, items[len(its):], rows[len(its):], out, 0xA5)
            assert not bad, (R.row_id(row), name, "golden", len(bad), bad[:8])
            assert out[dst_bytes:] == b"\xa5" * 16
            seen_hm.update(hm)
            seen_gold.update(gold)
        # no case left out: every item of the class, so every group, both finish
        # modes and the 16 source alignments
        assert len(seen_hm) == R.HANDMADE_COUNT[name] == len(hm_all[name])
        assert len(seen_gold) == R.GOLDEN_COUNT[name] == len(gold_all[name])
        through = [hm_all[name][i] for i in seen_hm]
        assert {it[0]["group"] for it in through} == \
            set(H.LZMA2_GROUPS if name == "l2" else H.LZMA_GROUPS)
        assert {it[1] for it in through} == {0, 1}
        assert {it[2] for it in through} == set(range(16)) | {None}

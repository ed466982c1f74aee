"""The match path's load batches (LZGPU_MP, lzma_device.h) on the GPU.

The batches differ per lane only where lanes of one wave sit in different
classes at the same pass -- another length coder (rep / match), another
posState row, choice 0 beside 1, LenHigh beside short lengths, SpecPos beside
Align, a cut or failing lane beside running ones -- so the smallest shape that
can go wrong is one wave of streams that disagree.  Two waves (64 streams) and
one wave plus a single live lane (33 streams), at most 2 KiB of input each
(tests/matchpath_cases.py), run on the throughput instantiation,
lane-interleaved rows on and off, lc0/pb0 and lc3/pb2 (with pb = 2 the lanes of
a wave sit in different posStates: the length front's rows differ per lane),
and every stream's output and result row is compared with the oracle.

Before the GPU run the test asserts, as conditions on a trace of its own
inputs, that the batch holds every class and that some wave holds the classes
of each pair in the same pass, in the planner's lane order."""
import pytest

import matchpath_cases as C
from test_fuse_gpu import ILV, LANES, M_THR, _opts


def check_coverage(L, lc, pb, n, ilv):
    items, src, dst_bytes, exp, syms, in_lens = C.batch(lc, pb, n)
    plan, order = L.plan_ex(L.make_descs(items), _opts(L, ilv))
    assert plan.n_lds == n and plan.n_classes == 1
    c = plan.classes[0]
    assert c.lds_mask == M_THR | (ILV if ilv else 0) and c.lanes_per_group == LANES, \
        (hex(c.lds_mask), c.lanes_per_group)
    return C.coverage(syms, in_lens, list(order)[:n])


@pytest.mark.parametrize("props", [(0, 0), (3, 2)])
def test_inputs_cover_every_class_and_pair(props):
    """The coverage condition on the CPU: the planner (host code) gives the
    lane order, nothing runs on a device."""
    import lzmagpu as L
    for ilv in (True, False):
        have, pairs = check_coverage(L, props[0], props[1], 64, ilv)
        assert C.WANT <= have, sorted(C.WANT - have, key=str)
        assert C.WANT_PAIRS <= pairs, sorted(C.WANT_PAIRS - pairs)
    C.batch(props[0], props[1], 33)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 33])
@pytest.mark.parametrize("ilv", [True, False])
@pytest.mark.parametrize("props", [(0, 0), (3, 2)])
def test_matchpath_bit_exact(props, ilv, n):
    import lzmagpu as L
    if L.device_count() <= 0:
        pytest.fail("no HIP device visible: " + L.last_error())
    lc, pb = props
    items, src, dst_bytes, exp, syms, in_lens = C.batch(lc, pb, n)
    if n == 64:
        have, pairs = check_coverage(L, lc, pb, n, ilv)
        assert C.WANT <= have and C.WANT_PAIRS <= pairs, (C.WANT - have, C.WANT_PAIRS - pairs)
    plan = L.Plan()
    r, res, dst = L.decode_batch_host(L.make_descs(items), src, dst_bytes, _opts(L, ilv), plan)
    assert r == 0, L.last_error()
    assert plan.n_classes == 1 and plan.classes[0].lds_mask == M_THR | (ILV if ilv else 0)
    assert plan.classes[0].lanes_per_group == LANES
    bad = []
    for k, e in enumerate(exp):
        got = (res[k].res, res[k].status, res[k].dest_len, res[k].src_len)
        out = dst[items[k]["dst_off"]:items[k]["dst_off"] + res[k].dest_len]
        if got != tuple(e[:4]) or out != e[4]:
            bad.append((k, got, e[:4]))
    assert not bad, (props, ilv, n, len(bad), bad[:6])

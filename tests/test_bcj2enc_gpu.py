"""The BCJ2 batch encoder on the GPU (Bcj2EncGpu_EncodeBatch and its host form)
against tests/bcj2enc.py's encode on the cases of tests/bcj2enc_cases.py: all
four streams, all lengths and every guard byte of the destination, byte for
byte.  Nothing has a tolerance."""
import ctypes

import numpy as np
import pytest

import bcj2enc_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import torch
    torch.zeros(1, device="cuda")
    import lzmagpu
    return lzmagpu


def as_lib(L, descs):
    return ctypes.cast(descs, ctypes.POINTER(L.Bcj2EncDesc))


def run_device(L, descs, src, dst_size, poison=0xA7):
    """One Bcj2EncGpu_EncodeBatch launch: ([(res, lens)], the dst image)."""
    import torch

    def dev(b):
        return torch.from_numpy(np.frombuffer(bytes(b) or b"\0", np.uint8).copy()).cuda()
    n = len(descs)
    d_descs, d_src = dev(bytes(descs)), dev(src)
    d_dst = torch.full((max(dst_size, 1),), C.GUARD, dtype=torch.uint8, device="cuda")
    d_scratch = torch.full((L.bcj2_scratch(as_lib(L, descs), n),), poison, dtype=torch.uint8,
                           device="cuda")
    d_res = torch.full((n * 40,), 0x77, dtype=torch.uint8, device="cuda")
    assert d_scratch.data_ptr() % 16 == 0
    r = L.bcj2_encode_batch_device(d_descs.data_ptr(), n, d_src.data_ptr(), d_dst.data_ptr(),
                                   d_scratch.data_ptr(), d_res.data_ptr())
    assert r == 0, L.last_error()
    torch.cuda.synchronize()
    res = (C.Result * n).from_buffer_copy(d_res.cpu().numpy().tobytes())
    return [(x.res, list(x.len)) for x in res], d_dst.cpu().numpy().tobytes()[:dst_size]


def check(got, want, names):
    for name, g, w in zip(names, got[0], want[0]):
        assert g == w, (name, g, w)
    assert got[1] == want[1]


def test_every_case_in_one_launch(L):
    names = [name for name, _ in C.cases()]
    items = [(data, None) for _, data in C.cases()]
    descs, src, dst_size = C.lay_out(items)
    assert all(d.src_off % 2 == 1 for d in descs)
    check(run_device(L, descs, src, dst_size), C.expect(items, dst_size, descs), names)


def test_short_capacities_write_nothing_past_them(L):
    items = C.short_cap_items()
    descs, src, dst_size = C.lay_out(items)
    want = C.expect(items, dst_size, descs)
    assert {r for r, _ in want[0]} == {C.OK, C.OUTPUT_EOF}
    check(run_device(L, descs, src, dst_size, poison=0x00), want, range(len(items)))


def test_one_stream_over_many_workgroups(L):
    """A nested stream of 300,001 bytes: 74 workgroup steps, five steps of the
    stream scan; beside it an empty stream and one the encoder refuses."""
    data = C.nested(11, 300001)
    assert 3 * C.STEP <= len(data) <= 1 << 20 and len(data) > 64 * C.SEG
    assert sum(1 for _, _, conv, live in C.decisions(data) if conv and not live) >= 1000
    items = [(b"", None), (data, None), (b"", [0, 0, 0, 0])]
    descs, src, dst_size = C.lay_out(items)
    want_res, want_image = C.expect(items, dst_size, descs)
    descs[2].src_len = 1 << 31      # refused: nothing of it is read
    want_res[2] = (C.UNSUPPORTED, [0, 0, 0, 0])
    check(run_device(L, descs, src, dst_size), (want_res, want_image), ["empty", "nested", "2^31"])


def test_host_call_cut_by_the_workspace_limit(L):
    picked = [(name, data) for name, data in C.cases() if len(data) in (9, 257, 4096, 20000)]
    items = [(data, None) for _, data in picked]
    descs, src, dst_size = C.lay_out(items)
    one = (C.Desc * 1)()
    slices = []
    for d in descs:
        one[0].src_len = d.src_len
        slices.append(L.bcj2_scratch(as_lib(L, one), 1) - L.bcj2_scratch(as_lib(L, one), 0))
    assert L.bcj2_scratch(as_lib(L, descs), len(descs)) == \
        L.bcj2_scratch(as_lib(L, one), 0) + sum(slices)
    limit = max(slices) + 4096
    assert sum(slices) > 3 * limit      # at least four launches
    want = C.expect(items, dst_size, descs)
    r, res, image = L.bcj2_encode_batch_host(as_lib(L, descs), len(descs), src,
                                             bytes([C.GUARD]) * dst_size, workspace_limit=limit)
    assert r == 0, L.last_error()
    check(([(x.res, list(x.len)) for x in res], image), want, [name for name, _ in picked])
    # one stream's slice above the limit: SZ_ERROR_MEM; a range outside dst: SZ_ERROR_PARAM
    assert L.bcj2_encode_batch_host(as_lib(L, descs), len(descs), src, bytes(dst_size),
                                    workspace_limit=max(slices) - 1)[0] == 2
    descs[0].out[3].cap = dst_size
    assert L.bcj2_encode_batch_host(as_lib(L, descs), len(descs), src, bytes(dst_size))[0] == 5


def test_bcj2_encode_and_decode_back(L):
    import bcj2enc
    data = bcj2enc.x86_like(3, 24000, 0.06)
    streams = L.bcj2_encode(data)
    assert streams == C.model(data)
    assert all(len(s) <= b for s, b in zip(streams, L.bcj2_bound(len(data))))
    assert L.bcj2_bound(len(data)) == C.bound(len(data))
    assert L.Bcj2_Decode(*streams, len(data)) == (0, data)
    assert L.bcj2_encode(b"") == (b"", b"", b"", b"\0" * 5)

"""csrc/bcj2enc_device.h on the host (tests/emu_bcj2enc/bcj2enc_emu.cpp, g++
-Wall -Werror): the BCJ2 encoder's phases run thread by thread against
tests/bcj2enc.py's encode, the executable specification, byte for byte on every
case of tests/bcj2enc_cases.py; every output decoded back through the lane
emulator's emu_bcj2 and, where built, the reference's Bcj2_Decode; short
capacities with guard bytes; the bounds; a stand-alone sanitizer build over the
same cases.  Nothing has a tolerance."""
import ctypes
import subprocess

import pytest

import bcj2enc
import bcj2enc_cases as C
import native


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return C.load_emu(C.build_emu(tmp_path_factory.mktemp("bcj2enc_emu")))


@pytest.fixture(scope="module")
def lane_emu():
    subprocess.run(["make", "-s", "-f", "tests/emu/Makefile"], cwd=native.ROOT, check=True)
    lib = ctypes.CDLL(native.ROOT + "/tests/emu/liblane_emu.so")
    lib.emu_bcj2.restype = ctypes.c_int
    lib.emu_bcj2.argtypes = [ctypes.c_char_p, ctypes.c_uint64] * 4 + [ctypes.c_char_p,
                                                                      ctypes.c_uint64]
    return lib


def test_case_set_covers_the_rule():
    """Asserted on the model, so a weak case set cannot pass."""
    dead_conv = 0
    seen = set()
    for _, data in C.cases():
        n = len(data)
        for i, kind, conv, live in C.decisions(data):
            if conv and not live:
                dead_conv += 1
            if live and i + 1 < n:
                seen.add((kind, conv))
    assert dead_conv >= 1000, dead_conv
    assert seen == {(k, c) for k in range(3) for c in (False, True)}


def test_restated_rule_is_the_model():
    """The position-wise rule the kernels implement, against encode()."""
    for name, data in C.cases():
        if len(data) > 5000:
            continue
        main = bytes(data[i] for i in _live_positions(data))
        assert main == C.model(data)[0], name


def _live_positions(data):
    dead = set()
    for i, _, conv, live in C.decisions(data):
        if conv and live:
            dead.update(range(i + 1, i + 5))
    return [i for i in range(len(data)) if i not in dead]


def test_geometry(emu):
    g = (ctypes.c_uint32 * 3)()
    emu.bcj2enc_emu_geometry(g)
    assert list(g) == [C.RUN, C.SEG, C.STEP] and C.SCAN == 64 * C.SEG


def test_every_case_equals_the_model(emu):
    """All cases as the streams of one batch, at odd offsets."""
    items = [(data, None) for _, data in C.cases()]
    descs, src, dst_size = C.lay_out(items)
    want_res, want_image = C.expect(items, dst_size, descs)
    for grid, poison in ((3, 0xA7), (1, 0x00), (64, 0xFF)):
        got_res, got_image = C.emu_run(emu, descs, src, dst_size, grid, poison)
        for (name, _), g, w in zip(C.cases(), got_res, want_res):
            assert g == w, (name, g, w)
        assert got_image == want_image, (grid, _first_diff(got_image, want_image, descs))


def _first_diff(a, b, descs):
    at = next(i for i in range(len(a)) if a[i] != b[i])
    for k, d in enumerate(descs):
        for j in range(4):
            if d.out[j].off - 4 <= at <= d.out[j].off + d.out[j].cap + 4:
                return (at, C.cases()[k][0] if k < len(C.cases()) else k, j, at - d.out[j].off)
    return at


def test_single_stream_batches(emu):
    for name, data in C.cases():
        if len(data) > 300:
            continue
        items = [(data, None)]
        descs, src, dst_size = C.lay_out(items)
        assert C.emu_run(emu, descs, src, dst_size) == C.expect(items, dst_size, descs), name


def test_outputs_decode_back(emu, lane_emu):
    items = [(data, None) for _, data in C.cases()]
    descs, src, dst_size = C.lay_out(items)
    _, image = C.emu_run(emu, descs, src, dst_size)
    ref = native.ref_cont() if native.have_ref() else None
    for k, (name, data) in enumerate(C.cases()):
        s = [image[d.off:d.off + d.cap] for d in descs[k].out]
        n = len(data)
        out = ctypes.create_string_buffer(b"\xa5" * max(n, 1), max(n, 1))
        assert lane_emu.emu_bcj2(s[0], len(s[0]), s[1], len(s[1]), s[2], len(s[2]), s[3],
                                 len(s[3]), out, n) == 0, name
        assert out.raw[:n] == data, name
        if ref is not None:
            f = ref.Bcj2_Decode
            f.restype = ctypes.c_int
            sz = ctypes.c_size_t
            out = ctypes.create_string_buffer(b"\xa5" * max(n, 1), max(n, 1))
            assert f(s[0], sz(len(s[0])), s[1], sz(len(s[1])), s[2], sz(len(s[2])), s[3],
                     sz(len(s[3])), out, sz(n)) == 0, name
            assert out.raw[:n] == data, name


def test_short_capacities(emu):
    items = C.short_cap_items()
    descs, src, dst_size = C.lay_out(items)
    want = C.expect(items, dst_size, descs)
    assert {r for r, _ in want[0]} == {C.OK, C.OUTPUT_EOF}
    got = C.emu_run(emu, descs, src, dst_size)
    assert got[0] == want[0]
    assert got[1] == want[1]


def test_bounds_hold():
    worst = bytes([0xE8]) * 1000            # a bit per byte, nothing convertible
    dense = b"\xe8\xfb\xff\xff\xff" * 200  # a target per five bytes (each its own opcode)
    for data in [d for _, d in C.cases()] + [worst, dense]:
        lens = [len(s) for s in C.model(data)]
        assert sum(lens[:3]) == len(data)
        assert all(got <= b for got, b in zip(lens, C.bound(len(data)))), len(data)
    assert len(C.model(dense)[1]) == C.bound(len(dense))[1]


def test_unsupported_length(emu):
    """A stream of 2^31 bytes is refused per stream, nothing read or written,
    beside streams that are encoded."""
    data = bcj2enc.x86_like(1, 500, 0.3)
    items = [(data, None), (b"", [0, 0, 0, 0]), (data, None)]
    descs, src, dst_size = C.lay_out(items)
    want_res, want_image = C.expect(items, dst_size, descs)
    descs[1].src_len = 1 << 31
    got_res, got_image = C.emu_run(emu, descs, src, dst_size)
    assert got_res == [want_res[0], (C.UNSUPPORTED, [0, 0, 0, 0]), want_res[2]]
    assert got_image == want_image


def test_sanitizer_program(tmp_path):
    """g++ -O1 -fsanitize=address,undefined, own main, exact-size source,
    descriptors and scratch."""
    exe = C.build_emu(tmp_path, extra=("-O1", "-g", "-fsanitize=address,undefined",
                                       "-fno-sanitize-recover=undefined"), main=True)
    batches = [([(data, None) for _, data in C.cases()], 3), (C.short_cap_items(), 2)]
    batches += [([(data, None)], 1) for _, data in C.cases() if len(data) <= 300]
    path = str(tmp_path / "cases.bin")
    C.write_case_file(path, batches)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "%d batches," % len(batches) in r.stdout and ", 0 mismatches" in r.stdout

"""Kernel logic on the CPU: the per-lane code of the HIP kernels
(lzma-sdk-zliblike_amd/csrc/lzma_lane.h) compiled for the host
(tests/emu/liblane_emu.so, test-only) against the golden vectors and the
oracle.  Catches logic bugs before a GPU run; the GPU suite
(test_gpu_parity.py) then checks the same vectors on the device."""
import ctypes
import os
import shutil
import random
import subprocess
import tempfile

import pytest

import golden_cases as G
import native

EMU_SO = os.path.join(native.ROOT, "tests", "emu", "liblane_emu.so")


# Builds of lzma_device.h the emulation covers: section placements (which
# tables live in the lane's LDS slice), literal batch sizes and the kernel
# instantiations (latency, lane-interleaved, cooperative).  The code shapes
# measured and rejected in rounds 1-2 were removed from the header in round 3
# (DESIGN.md §4 keeps their A/B evidence).
EMU_VARIANTS = {
    "default": "",
    "litm_global": "-DLZGPU_LDS_MASK=0x1FF",
    "hot_only_lds": "-DLZGPU_LDS_MASK=0x107",
    "full_lds": "-DLZGPU_LDS_MASK=0x3FF",
    "latency_mask": "-DLZGPU_LDS_MASK=0x1BF",
    "all_global_mask": "-DLZGPU_LDS_MASK=0",
    "lit_batch": "-DLZGPU_LIT_BATCH=3",
    "lit_batch_1_latency": "-DLZGPU_LIT_BATCH=1 -DLZGPU_LDS_MASK=0x1BF",
    "lit_batch_32": "-DLZGPU_LIT_BATCH=32",
    "match_fat_global_len": "-DLZGPU_LDS_MASK_LAT=0x105 -DLZGPU_LDS_MASK=0x107 -DEMU_LAT_MASK",
    "latency_instantiation": "-DEMU_LAT_MASK",
    # round 5: the latency placement with the slot trees global (the planner's
    # choice for classes whose widest slice would cost workgroups per CU)
    "latency_slot_global": "-DLZGPU_LDS_MASK_LAT=0x19F -DEMU_LAT_MASK",
    "interleaved_global_instantiation": "-DEMU_ILV",
    "coop_instantiation": "-DEMU_COOP",
    "coop_all_lds_instantiation": "-DEMU_COOP_ALL",
    # round 4: the LDS history window of the cooperative kernels (a 4 KiB window
    # falls back to the dictionary for longer distances and wraps; 64 KiB holds
    # most streams whole), batch items and device-resident sessions
    "coop_window_4k": "-DEMU_COOP_ALL_WIN -DEMU_WIN_BYTES=4096",
    "coop_window_64k": "-DEMU_COOP_ALL_WIN -DEMU_WIN_BYTES=65536",
    "session_coop_window_4k": "-DEMU_SESS_COOP_WIN -DEMU_WIN_BYTES=4096",
    "session_coop_window_64k": "-DEMU_SESS_COOP_WIN -DEMU_WIN_BYTES=65536",
    # round 6: the one-stream 32-lane kernel's instantiation, and the uniform
    # symbol loop (one symbol per pass, uniform kind / exit branches) in it and
    # in the cooperative kernels, with and without uniform symbol-kind branches
    "dup_instantiation": "-DEMU_DUP",
    "dup_uniform_loop": "-DLZGPU_UNI_LOOP=1 -DEMU_DUP",
    "dup_uniform_loop_slot_global": "-DLZGPU_UNI_LOOP=1 -DLZGPU_LDS_MASK_LAT=0x19F -DEMU_DUP",
    "coop_uniform_loop": "-DLZGPU_UNI_LOOP=2 -DEMU_COOP",
    "coop_window_uniform_loop": "-DLZGPU_UNI_LOOP=2 -DEMU_COOP_ALL_WIN -DEMU_WIN_BYTES=4096",
    "session_coop_window_uniform_loop": "-DLZGPU_UNI_LOOP=2 -DEMU_SESS_COOP_WIN -DEMU_WIN_BYTES=4096",
    # round 6: the decision as borrow + one multiply-add update (Rc::decide form 1)
    # (defaults since round 6: uniform loop 2, decision form 1; the A/B forms)
    "bit_form_0_dup": "-DLZGPU_BIT_FORM=0",
    "bit_form_0_dup_kernel": "-DLZGPU_BIT_FORM=0 -DEMU_DUP",
    "bit_form_0_latency": "-DLZGPU_BIT_FORM=0 -DEMU_LAT_MASK",
    "bit_form_all_coop_window": "-DLZGPU_BIT_FORM=7 -DEMU_COOP_ALL_WIN -DEMU_WIN_BYTES=4096",
    "bit_form_all_coop": "-DLZGPU_BIT_FORM=7 -DEMU_COOP",
    "dup_batch_loop": "-DLZGPU_UNI_LOOP=0 -DEMU_DUP",
    "coop_window_batch_loop": "-DLZGPU_UNI_LOOP=0 -DEMU_COOP_ALL_WIN -DEMU_WIN_BYTES=4096",
    # the plain literal tree walked by node instead of cell address (LZGPU_LIT_ADDR)
    "lit_node_walk": "-DLZGPU_LIT_ADDR=0",
    "lit_node_walk_dup": "-DLZGPU_LIT_ADDR=0 -DEMU_DUP",
    "lit_node_walk_coop_window": "-DLZGPU_LIT_ADDR=0 -DEMU_COOP_ALL_WIN -DEMU_WIN_BYTES=4096",
}


@pytest.fixture(scope="module", params=sorted(EMU_VARIANTS))
def emu(request):
    # variant builds go to the temp dir: only the default build stays in-tree
    # (the GPU suite's test_bra compares against it), the rest never ship
    vdir = os.path.join(tempfile.gettempdir(), "lzgpu_emu_variants")
    os.makedirs(vdir, exist_ok=True)
    # one build per process (pytest-xdist workers would otherwise rebuild a
    # variant another worker has loaded); the default one is then moved
    # into the tree atomically
    out = os.path.join(vdir, f"liblane_emu_{request.param}.{os.getpid()}.so")
    subprocess.run(["make", "-s", "-f", "tests/emu/Makefile", f"EMU_OUT={out}",
                    f"EMU_FLAGS={EMU_VARIANTS[request.param]} {os.environ.get('LZGPU_EMU_EXTRA', '')}"], cwd=native.ROOT, check=True)
    if request.param == "default":
        tmp = f"{EMU_SO}.{os.getpid()}"
        shutil.copyfile(out, tmp)
        os.replace(tmp, EMU_SO)
    lib = ctypes.CDLL(out)
    lib.emu_decode_batch_lds.restype = None
    lib.emu_decode_batch_lds.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_uint32]
    lib.emu_decode_batch.restype = None
    lib.emu_decode_batch.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    for f in (lib.emu_stream_decode, lib.emu_stream_decode_dic):
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                      ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                      ctypes.POINTER(ctypes.c_longlong), ctypes.c_int, native.size_t_p,
                      native.size_t_p]
    return lib


def run_batch(emu, items, src, lds=False):
    """The kernel bodies on the host.  lds=True follows the planner: items it puts
    on the LDS kernel run through lane_decode_lds, the rest through lane_decode."""
    import lzmagpu as L
    descs = L.make_descs(items)
    n = len(items)
    order = (ctypes.c_uint32 * max(n, 1))()
    plan = L.Plan()
    assert L.lib.LzmaGpu_PlanBatchEx(descs, n, order, ctypes.byref(plan)) == 0
    wsbuf = ctypes.create_string_buffer(max(plan.workspace_bytes, 16))
    dst_bytes = max((it["dst_off"] + it["dst_cap"] for it in items), default=0)
    dst = ctypes.create_string_buffer(max(dst_bytes, 1))
    res = (L.Result * max(n, 1))()
    if not lds:
        emu.emu_decode_batch(descs, n, src, dst, wsbuf, res)
        return res, dst.raw
    one = (L.StreamDesc * 1)()
    r1 = (L.Result * 1)()
    # LDS slice large enough for any placement variant: the whole table
    stride = 0
    for k in range(plan.n_lds):
        if descs[order[k]].kind == L.KIND_LZMA2:
            lc, lp, pb = 4, 0, 4  # chunks may switch props: widest layout
        else:
            pr = bytes(descs[order[k]].props)
            lc, lp, pb = pr[0] % 9, (pr[0] // 9) % 5, pr[0] // 45
        stride = max(stride, (56 << pb) + 950 + (768 << (lc + lp)))
    for k in range(n):
        i = order[k]
        one[0] = descs[i]
        if k < plan.n_lds:
            emu.emu_decode_batch_lds(one, 1, src, dst, wsbuf, r1, (stride + 3) // 4 * 4)
        else:
            emu.emu_decode_batch(one, 1, src, dst, wsbuf, r1)
        res[i] = r1[0]
    return res, dst.raw


@pytest.mark.parametrize("lds", [False, True])
def test_emu_golden_lzma_batch(emu, lds):
    d = G.load()
    items, srcs, off, doff = [], [], 0, 0
    cs = G.cases("lzma")
    for i, c in cs:
        s = G.case_input(d, c)
        items.append(dict(src_off=off, src_len=len(s), dst_off=doff, dst_cap=c["dest_cap"],
                          props=bytes.fromhex(c["props"]), finish=c["finish"]))
        srcs.append(s)
        off += len(s)
        doff += c["dest_cap"]
    res, dst = run_batch(emu, items, b"".join(srcs) + b"\0" * 16, lds)
    bad = []
    for k, (i, c) in enumerate(cs):
        e = c["expect"]
        got = (res[k].res, res[k].status, res[k].dest_len, res[k].src_len)
        out = dst[items[k]["dst_off"]:items[k]["dst_off"] + res[k].dest_len]
        if got != (e["res"], e["status"], e["dest_len"], e["src_len"]) or G.sha(out) != e["sha256"]:
            bad.append((i, c["note"], got, (e["res"], e["status"], e["dest_len"], e["src_len"])))
    assert not bad, bad[:10]


@pytest.mark.parametrize("lds", [False, True])
def test_emu_golden_lzma2_batch(emu, lds):
    import lzmagpu as L
    d = G.load()
    for i, c in G.cases("lzma2"):
        s = G.case_input(d, c)
        items = [dict(src_off=0, src_len=len(s), dst_off=0, dst_cap=c["dest_cap"],
                      props=bytes([c["prop"]]), finish=c["finish"], kind=L.KIND_LZMA2)]
        res, dst = run_batch(emu, items, s + b"\0" * 16, lds)
        e = c["expect"]
        got = (res[0].res, res[0].status, res[0].dest_len, res[0].src_len)
        assert got == (e["res"], e["status"], e["dest_len"], e["src_len"]), (i, c["note"])
        assert G.sha(dst[:res[0].dest_len]) == e["sha256"]


@pytest.mark.parametrize("device_ring", [True, False])
def test_emu_golden_streaming(emu, device_ring):
    """DecodeToBuf traces: the session's device ring loop (mode 1) and the
    host ring loop over DecodeToDic calls (mode 0)."""
    d = G.load()
    fn = emu.emu_stream_decode if device_ring else emu.emu_stream_decode_dic
    for i, c in G.cases("stream"):
        s = G.case_input(d, c)
        # the readers load aligned 16-byte blocks around the input (a device
        # buffer's block never leaves its allocation): a padded host copy
        sb = ctypes.create_string_buffer(s, len(s) + 32)
        out = ctypes.create_string_buffer(max(c["out_total"], 1))
        trace = (ctypes.c_longlong * 400000)()
        ol, iu = ctypes.c_size_t(0), ctypes.c_size_t(0)
        calls = fn(bytes.fromhex(c["props"]), sb, len(s), out, c["out_total"],
                                      c["in_chunk"], c["out_chunk"], c["finish"], trace, 100000,
                                      ctypes.byref(ol), ctypes.byref(iu))
        tr = [tuple(trace[4 * k:4 * k + 4]) for k in range(calls)]
        e = c["expect"]
        assert calls == e["calls"], (i, c["note"])
        assert G.trace_digest(tr) == e["trace_sha256"], (i, c["note"], tr[:3], e["trace_head"])
        assert (ol.value, iu.value) == (e["out_len"], e["in_used"])
        assert G.sha(out.raw[:ol.value]) == e["sha256"]


@pytest.mark.parametrize("lds", [False, True])
def test_emu_fuzz_vs_oracle(emu, lds):
    rng = random.Random(77)
    orc = native.oracle()
    items, srcs, exp, off, doff = [], [], [], 0, 0
    have_ref = os.path.exists(native.REF_SO)
    import lzma
    for it in range(600):
        lc, lp, pb = rng.randrange(9), rng.randrange(5), rng.randrange(5)
        dsz = rng.choice([4096, 1 << 14, 1 << 16])
        n = rng.choice([0, 1, 2, 60, 700, 4096, 9000])
        data = native.gen(rng.choice(["text", "random", "runs"]), 51_000 + it, n)
        if have_ref and rng.random() < 0.5:
            props, comp = native.ref_encode(data, level=rng.choice([0, 5]), dict_size=dsz, lc=lc,
                                            lp=lp, pb=pb, end_mark=rng.random() < 0.5)
        else:
            lc, lp = min(lc, 4), 0
            f = [{"id": lzma.FILTER_LZMA1, "dict_size": dsz, "lc": lc, "lp": lp, "pb": pb,
                  "preset": 6}]
            comp = lzma.compress(data, format=lzma.FORMAT_RAW, filters=f)
            props = bytes([(pb * 5 + lp) * 9 + lc]) + dsz.to_bytes(4, "little")
        comp = bytearray(comp)
        mode = rng.randrange(5)
        if mode == 1 and len(comp) > 6:
            comp[rng.randrange(5, len(comp))] ^= 1 << rng.randrange(8)
        elif mode == 2:
            comp = comp[:rng.randrange(len(comp) + 1)]
        cap = max(0, n + rng.choice([0, 0, 1, -1, 50, -50]))
        fin = rng.randrange(2)
        comp = bytes(comp)
        items.append(dict(src_off=off, src_len=len(comp), dst_off=doff, dst_cap=cap, props=props,
                          finish=fin))
        srcs.append(comp)
        exp.append(native.decode(orc, "orc", comp, props, cap, fin))
        off += len(comp)
        doff += cap
    res, dst = run_batch(emu, items, b"".join(srcs) + b"\0" * 16, lds)
    for k in range(len(items)):
        got = (res[k].res, res[k].status, res[k].dest_len, res[k].src_len)
        out = dst[items[k]["dst_off"]:items[k]["dst_off"] + res[k].dest_len]
        assert got == exp[k][:4] and out == exp[k][4], (k, got, exp[k][:4])


def test_emu_handmade_set(emu):
    """The hand-made streams (tests/handmade_cases.py: symbols and chunk
    sequences no encoder writes, both finish modes, 16 source alignments for
    the short ones) through this build, against the reference's answers."""
    import handmade_cases as H
    its = H.items()
    descs, src, _ = H.batch(its)
    res, dst = run_batch(emu, descs, src, lds=True)
    bad = H.mismatches(its, descs, res, dst)
    assert not bad, (len(bad), bad[:8])


def test_update_forms_agree_for_every_probability():
    """Rc::decide's two update forms equal the reference's UPDATE_0 / UPDATE_1
    (LzmaDec.c:12-16) for every probability a cell can hold (0..2048)."""
    for p in range(0, 2049):
        up0, up1 = p + ((2048 - p) >> 5), p - (p >> 5)
        assert p - ((p - 2017) >> 5) == up0 and p - (p >> 5) == up1  # form 0 (Python >> is arithmetic)
        assert (31 * p + 2048) >> 5 == up0 and (31 * p + 31) >> 5 == up1  # form 1


def test_direct_chunks_match_serial_direct_bits(tmp_path):
    """direct_coop decides up to five direct bits per step (closed form over the
    range's halvings, one ballot); it must leave range, code, the distance bits
    and the input position exactly where the reference's bit-serial loop
    (LzmaDec.c:323-344) does, for well-formed and corrupt states alike."""
    import subprocess
    src = os.path.join(native.ROOT, "tests", "emu", "direct_chunks.cpp")
    exe = str(tmp_path / "direct_chunks")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I",
                    os.path.join(native.ROOT, "lzma-sdk-zliblike_amd", "csrc"), "-I",
                    os.path.join(native.ROOT, "include"), src, "-o", exe], check=True)
    r = subprocess.run([exe, "400000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 mismatches" in r.stdout

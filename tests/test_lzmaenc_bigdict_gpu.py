"""The encoder kernels at dictionaries above 64 KiB (tests/lzmaenc_bigdict_cases.py)
against the reference's single-threaded LzmaEncode / Lzma2Enc_Encode: a hash mask
wider than 0xFFFF (up to 0x7FFFFF and 32 MiB of hash at the level-5 default),
matches farther than 64 KiB (pos slots from 32 up, 11 to 16 direct bits, the
align prices at those slots, FillDistancesPrices over more than 32 slots, the
far arms of ChangePair), a ring that wraps beyond 64 KiB, and the levels' own
dictionaries -- through the one-shot fast kernel, the normal-mode kernels, the
session kernels, LZMA2, xz and 7z.  Live reference where it is built, else the
committed goldens (tests/golden/lzmaenc_bigdict_cases.json).  Equality is the
criterion everywhere.  test_lzmaenc_bigdict_emu.py shows on the host that these
cases notice a narrow mask and a wrong direct bit."""
import lzma
import os
import sys
import time

import pytest

import lzma2enc_cases as C2
import lzmaenc_bigdict_cases as B
import lzmaenc_cases as C
import lzmaenc_opt_cases as O
import lzmaenc_session_cases as S
import native
import test_lzmaenc_gpu as T
import test_lzmaenc_opt_gpu as TO
import test_lzmaenc_session_gpu as TS

sys.path.insert(0, os.path.join(native.ROOT, "lzma-sdk-zliblike_amd"))

pytestmark = pytest.mark.gpu
STEP_LIMIT_S = TO.STEP_LIMIT_S   # an encode step that takes longer is a failure, not a wait
FAST_NAMES = ("F", "F_ctl", "M", "M24", "C80", "W", "D2", "D3", "D4")


@pytest.fixture(scope="module")
def L():
    import lzmagpu
    return lzmagpu


@pytest.fixture(scope="module")
def golden():
    return B.load_golden()


modes_on = TO.modes_on


def random_of(normal):
    return [c for c in B.random_cases() if (O.mode_of(c) != 0) == normal]


def encode_batches(L, cases, golden, lanes=0):
    """TO.encode_cases over the cases, cut so that no batch holds more than
    four 16 MiB dictionaries.  Returns the round-trip work and the modes seen."""
    back, modes = [], set()
    for batch in B.batches(cases):
        b, m = TO.encode_cases(L, batch, golden, lanes=lanes)
        back += b
        modes |= set(m)
    return back, modes


@pytest.mark.parametrize("lanes", [16, 32, 64])
def test_fast_batch(L, golden, lanes):
    """The named fast-path streams and the mode-0 random cases, in the
    planner's order with poisoned destinations and workspaces."""
    cases = [B.named(name) for name in FAST_NAMES] + random_of(False)
    assert len(cases) > 30 and {c["dict"] for c in cases} >= set(B.DICTS)
    assert sum(c["n"] > 1 << 16 for c in cases) >= 12
    back, modes = encode_batches(L, cases, golden, lanes)
    assert modes == {0}
    if lanes == 16:
        T.round_trip(L, back)


@pytest.mark.parametrize("name", ["X", "X_ctl"])
def test_a_match_beyond_one_mebibyte(L, golden, name):
    """1.1 MB alone in a batch: the block returns 1,051,024 bytes back (16
    direct bits with the 2 MiB dictionary, out of reach with 1 MiB + 1)."""
    back, _ = TO.encode_cases(L, [B.named(name)], golden)
    T.round_trip(L, back)


def normal_named():
    cases = [B.named(name, mode) for name in ("F", "M", "C80") for mode in B.NORMAL_MODES]
    return cases + [B.named("M24", "opt_bt4"), B.named("D5"), B.named("F_ctl", "opt_bt4")]


def test_normal_batch(L, golden):
    """F, M and C80 in the three normal modes, M24 and the level-5 default (two
    16 MiB dictionaries), the control, and level-1 streams mixed in."""
    cases = normal_named()
    cases = cases[:5] + TO.mode0_cases() + cases[5:]
    back, modes = TO.encode_cases(L, cases, golden)
    assert set(modes) == {0, 1, 2, 3} and len(back) == len(cases) - 1
    T.round_trip(L, back)


def test_normal_random_batch(L, golden):
    cases = random_of(True)
    assert len(cases) >= 20 and {O.mode_of(c) for c in cases} == {1, 2, 3}
    assert {c["dict"] for c in cases} == set(B.DICTS)
    back, _ = encode_batches(L, cases, golden)
    T.round_trip(L, back)


def test_dropins_at_the_levels_own_dictionaries(L, golden, modes_on):
    """LzmaCompress with no arguments and LzmaEncode with level-5 props: a
    16 MiB dictionary; LzmaCompress at levels 2, 3, 4: 256 KiB, 1 MiB, 4 MiB."""
    d5 = B.named("D5")
    w, data = B.expect(d5, golden), B.data_of(d5)
    assert w["props5"][1:] == (1 << 24).to_bytes(4, "little")
    t0 = time.monotonic()
    got = L.LzmaCompress(data, w["cap"])
    assert time.monotonic() - t0 < STEP_LIMIT_S
    B.check((got[0], got[1], got[2], got[3]), w, "LzmaCompress()")
    got = L.LzmaEncode(data, L.enc_props(5), w["cap"])
    B.check((got[0], got[1], got[2], got[3]), w, "LzmaEncode(level 5)")
    for level in (2, 3, 4):
        c = B.named("D%d" % level)
        w = B.expect(c, golden)
        assert w["props5"][1:] == (1 << (14 + 2 * level)).to_bytes(4, "little")
        got = L.LzmaCompress(data, w["cap"], level=level)
        B.check((got[0], got[1], got[2], got[3]), w, "LzmaCompress(level %d)" % level)


def lzma2_blocks(L, golden, level):
    """lzma2_encode_batch and Lzma2EncodeHost on F and M with a 256 KiB
    dictionary: the reference's one-block stream."""
    cases = [B.lzma2_case(name, level) for name in ("F", "M")]
    wants = [B.lzma2_expect(c, golden) for c in cases]
    datas = [C2.data_of(c) for c in cases]
    t0 = time.monotonic()
    got = L.lzma2_encode_batch(datas, level=level, dict_size=1 << 18, lc=3, lp=0, pb=2)
    assert time.monotonic() - t0 < STEP_LIMIT_S
    for c, w, (r, prop, body) in zip(cases, wants, got):
        C2.check_block((r, len(body), prop, body), w, C2.key(c))
    for c, w, data in zip(cases, wants, datas):
        r, prop, out = L.Lzma2EncodeHost(data, L.enc2_props(level, 1 << 18, 3, 0, 2),
                                         len(data) + 4096)
        assert r == 0, L.last_error()
        C2.check_block((r, len(out) - 1, prop, out[:-1]), w, C2.key(c))
        assert out[-1] == 0 and C2.decode_raw(out, prop) == data
    return cases[0], wants[0], datas[0]


def test_lzma2_xz_and_7z_at_level_1(L, golden):
    c, w, data = lzma2_blocks(L, golden, 1)
    # xz: one block, the reference's LZMA2 stream of F
    r, xz = L.XzEncode(data, L.enc2_props(1, 1 << 18, 3, 0, 2), 4, len(data) + 4096)
    assert r == 0, L.last_error()
    r, blocks, total = L.xz_index(xz)
    assert (r, total, len(blocks)) == (0, len(data), 1)
    b = blocks[0]
    body = xz[b.data_off:b.data_off + b.pack_size]
    assert (b.pack_size, b.lzma2_prop) == (w["len"], w["prop"]) and C2.sha(body) == w["sha256"]
    assert lzma.decompress(xz, format=lzma.FORMAT_XZ) == data
    assert L.XzDecode(xz, len(data)) == (0, data, -1)
    # 7z: an LZMA folder of F, the reference's LzmaEncode stream as its pack stream
    import sevenzenc_cases as Z
    a = Z.Archive(L, [L.sz_method(L.SZ_M_LZMA, level=1, dict_size=1 << 18, lc=3, lp=0, pb=2)])
    a.group(0, [("far.bin", data)])
    src, items, n, names, names_len = a.build()
    r, folders, n_pieces, cap = L.sz_write_plan(items, n, len(src), names_len, a.methods)
    assert r == Z.OK, L.last_error()
    r, size, dest, st = L.SzWrite(src, items, n, names, names_len, a.methods, cap, 0, fill=0xEE)
    assert r == Z.OK, L.last_error()
    arc = dest[:size]
    r, fo, fi, nm, total = L.sz_open(arc)
    assert r == Z.OK and total == len(data) and [f.num_coders for f in fo] == [1]
    w1 = B.expect(B.named("F"), golden)
    pack = arc[fo[0].pack_off:fo[0].pack_off + fo[0].pack_size]
    assert bytes(fo[0].props[:fo[0].props_size]) == w1["props5"]
    assert (len(pack), O.sha(pack), pack[:32]) == (w1["dest_len"], w1["sha256"], w1["head"])
    r, out, fres = L.SzExtract(arc, len(data))
    assert r == Z.OK and out == data
    if Z.have_ref_reader():
        r, fres, fsz, out, nm = Z.ref_extract(arc)
        assert r == Z.OK and out == data


def test_lzma2_at_level_5(L, golden, modes_on):
    lzma2_blocks(L, golden, 5)


# ---------------------------------------------------------------- sessions

_one_shot = {}


def one_shot(L):
    """F, M and W by the one-shot fast kernel in one batch, computed once."""
    if not _one_shot:
        cases = [B.named(name) for name in B.SESSION_NAMES]
        items = []
        for c in cases:
            r, d, _ = T.desc_of(L, c)
            assert r == 0
            items.append((d, B.data_of(c), C.ample(c["n"])))
        _one_shot.update(cases=cases, got=T.run_device(L, items))
    return _one_shot["cases"], _one_shot["got"]


@pytest.mark.parametrize("schedule", ["p4096", "p546", "random"])
def test_sessions(L, golden, schedule):
    """F, M and W as three sessions fed by one schedule, a round per piece:
    the one-shot kernel's bytes and the reference's."""
    cases, one = one_shot(L)
    datas = [B.data_of(c) for c in cases]
    n = len(cases)
    cap = max(len(d) for d in datas)
    ss = L.LzmaEncSessions(n, cap, C.ample(cap), props=[TS.props_of(L, c) for c in cases],
                           poison=TS.POISON)
    pieces = [B.pieces_of(schedule, len(d), i) for i, d in enumerate(datas)]
    out = [b""] * n
    t0 = time.monotonic()
    for k in range(max(len(p) for p in pieces) + 1):
        finish = []
        for i in range(n):
            if k < len(pieces[i]):
                ss.append(i, datas[i][ss.supplied[i]:ss.supplied[i] + pieces[i][k]])
            elif not ss.rec[i].finished:
                assert ss.supplied[i] == len(datas[i])
                finish.append(i)
        assert ss.round(finish=finish) == 0, L.last_error()
        for i in range(n):
            out[i] += ss.drain(i)
            if not ss.rec[i].finished:
                assert ss.rec[i].status == S.NEEDS_INPUT and ss.supplied[i] - ss.rec[i].in_pos < S.HOLD
    assert time.monotonic() - t0 < STEP_LIMIT_S
    for i, c in enumerate(cases):
        rec = ss.rec[i]
        assert (rec.finished, rec.status, rec.in_pos) == (1, S.FINISHED, len(datas[i])), i
        assert (rec.res, rec.out_pos, out[i]) == tuple(one[i]), (schedule, i)
        w = B.expect(c, golden)
        B.check((rec.res, rec.out_pos, ss.props5[i], out[i]), w, (schedule, B.key(c)))


def test_handle_at_level_3(L, golden):
    """F through LzmaEnc_Create .. LzmaEnc_Encode with level-3 props as they
    are: the level's 1 MiB dictionary."""
    c = B.named("D3")
    w, data = B.expect(c, golden), B.data_of(c)
    got = []
    r, props5 = L.LzmaEnc_Encode(TS.reader(data, 65536), lambda b: got.append(b) or len(b),
                                 L.enc_props(3))
    packed = b"".join(got)
    B.check((r, len(packed), props5, packed), w, "LzmaEnc_Encode(level 3)")
    assert props5[1:] == (1 << 20).to_bytes(4, "little")

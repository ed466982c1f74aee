"""The hand-made LZMA / LZMA2 set (tests/handmade_cases.py) on the CPU: the
construction is what it claims to be (the reference's answer falls in each
case's class; the coverage conditions hold on the encoder's own record), the
recorded results equal the live reference's, and the CPU restatement
(oracle/liboracle.so) equals the reference on every case.  The host builds of
the lane code take the set in tests/test_emu.py and tests/test_fuse_emu.py,
the GPU kernels in tests/test_gpu_kernels.py, tests/test_fuse_gpu.py and
tests/test_gpu_parity.py; the kernels that resume in mid-stream (time-sliced
rounds, device sessions, the drop-in's DecodeToBuf) in
tests/test_handmade_resume.py."""
import collections
import hashlib

import pytest

import handmade_cases as H
import lzmaenc_min as E
import native


def test_ring_reach_streams_unchanged():
    """The generator grew; the ring-reach streams of tests/test_oracle.py and
    tests/test_dropin_mirror.py (seeds 1 to 3) are byte for byte what they were."""
    want = {1: "749166d3b323f382ed1f053ca77fbec41b4a817af26bbb6945cb648738552921",
            2: "28e767a46b18aadce6a533f063f52d48b2093d0cfbbea451d4915d8ca6d2d9a1",
            3: "a955edd88750c1c0a16e8c010672a32b4baf03229955b9adf7ea1aeecd5e88e6"}
    for seed, digest in want.items():
        assert hashlib.sha256(E.ring_reach_stream(seed)[0]).hexdigest() == digest


def test_names_are_unique_and_inputs_small():
    cs = H.cases()
    assert len({c["name"] for c in cs}) == len(cs)
    assert max(len(c["src"]) for c in cs) <= 6 * 1024
    assert all(c["cap"] >= 0 for c in cs)


def test_every_class_is_present():
    n = collections.Counter((c["kind"], c["group"]) for c in H.cases())
    for g in H.LZMA_GROUPS:
        # each LZMA class under each of the three props sets
        assert n["lzma", g] >= 3 and n["lzma", g] % 3 == 0, g
    for g in H.LZMA2_GROUPS:
        assert n["lzma2", g] >= 1, g
    for plp in H.PROPS:
        tag = "lc%dlp%dpb%d" % plp
        assert {c["group"] for c in H.lzma_cases() if c["name"].endswith(tag)} == \
            set(H.LZMA_GROUPS)
    # the source alignments: cases of at most 64 input bytes, some of them
    # ending inside their first 16-byte block
    small = [c for c in H.cases() if len(c["src"]) <= 64]
    assert small and any(len(c["src"]) < 16 for c in small)
    its = H.items()
    for c in small[:3] + small[-3:]:
        assert {a for cc, f, a in its if cc is c and f == 1} == set(range(16)) | {None}
    descs, src, _ = H.batch(its)
    assert all(a is None or d["src_off"] % 16 == a for d, (_, _, a) in zip(descs, its))


def test_reference_answer_falls_in_the_class_of_each_case():
    bad = []
    for c in H.cases():
        for finish in (0, 1):
            row, _ = H.expected(c, finish)
            if H.answer_class(row[0], row[1]) != c["want"][finish]:
                bad.append((c["name"], finish, row, c["want"][finish]))
    assert not bad, bad[:10]


def test_recorded_results_cover_the_list_exactly():
    assert set(H.golden()) == {H.key(c, f) for c in H.cases() for f in (0, 1)}


@pytest.mark.skipif(not native.have_ref(), reason="oracle/_ref/libref_lzma.so not built")
def test_recorded_results_equal_the_live_reference():
    g = H.golden()
    bad = []
    for c in H.cases():
        for finish in (0, 1):
            row, out = H.from_reference(c, finish)
            r = g[H.key(c, finish)]
            if (r["res"], r["status"], r["dest_len"], r["src_len"]) != row or \
                    r["sha256"] != H.sha(out):
                bad.append((c["name"], finish, row))
    assert not bad, bad[:10]


def test_oracle_equals_reference_on_every_case():
    bad = []
    for c in H.cases():
        for finish in (0, 1):
            row, out = H.from_oracle(c, finish)
            want = H.expected(c, finish)
            if (row, H.sha(out)) != want:
                bad.append((c["name"], finish, row, want[0]))
    assert not bad, bad[:10]


def test_prototype_answers_of_the_issue():
    """The answers the issue quotes for lc3 lp0 pb2, as a guard on the list."""
    by = {c["name"]: c for c in H.cases()}
    tag = " lc3lp0pb2"
    for k in ("rep0", "rep1", "rep2", "rep3", "short rep"):
        for f in (0, 1):
            assert H.expected(by[f"first symbol {k}{tag}"], f)[0] == (1, 0, 0, 5)
    assert H.expected(by["50 literals, distance index 50" + tag], 1)[0][:3] == (1, 0, 50)
    assert H.expected(by["50 literals, distance index 49" + tag], 1)[0][0] == 0
    for idx in (4096, 5000):
        assert H.expected(by[f"5000 literals, distance index {idx}{tag}"], 0)[0][:3] == (1, 0, 5000)
    for ln in H.MARKER_LENS:
        c = by[f"end marker length {ln}, three bytes behind, cap+0{tag}"]
        any_, end = H.expected(c, 0)[0], H.expected(c, 1)[0]
        assert any_[:3] == (0, 2, 20) and end[:3] == (0, 1, 20)
        # FINISH_ANY leaves the marker unread; FINISH_END stops before the trailing bytes
        assert any_[3] < end[3] == len(c["src"]) - 3
    c = by["length 273 over the capacity" + tag]
    assert H.expected(c, 0)[0][:3] == (0, 2, 100) and H.expected(c, 1)[0][:3] == (1, 2, 100)
    c = by["three chunks, three props, capacity 5 short"]
    assert H.expected(c, 1)[0][:2] == (1, 2)


# ------------------------------------------------------------------ coverage, from the record

def _records(group):
    return [r for c in H.lzma_cases() if c["group"] == group for r in c["records"]]


@pytest.mark.parametrize("plp", H.PROPS)
def test_state_walk_is_complete(plp):
    tag = "lc%dlp%dpb%d" % plp
    c = next(c for c in H.lzma_cases() if c["name"] == "state walk " + tag)
    kinds = {"L": "lit", "ML": "lit", "MA": "match", "REP": "rep", "SR": "short rep"}
    seen = {(r["state"], kinds[r["kind"]]) for r in c["records"][0]}
    assert seen == {(s, k) for s in range(12) for k in set(kinds.values())}
    # every rep index and every length class on the way
    assert {r["rep"] for r in c["records"][0] if r["kind"] == "REP"} == {0, 1, 2, 3}
    assert {r["len_class"] for r in c["records"][0] if r["kind"] in ("MA", "REP")} == {0, 1, 2}


@pytest.mark.parametrize("plp", H.PROPS)
def test_matched_literal_levels_in_every_state(plp):
    tag = "lc%dlp%dpb%d" % plp
    c = next(c for c in H.lzma_cases() if c["name"].startswith("matched literals") and
             c["name"].endswith(tag))
    seen = {(r["state"], r["level"]) for r in c["records"][0] if r["kind"] == "ML"}
    assert seen >= {(s, lvl) for s in range(7, 12) for lvl in range(9)}


def test_symbols_no_encoder_writes_are_in_the_record():
    first = collections.Counter(c["records"][0][0]["kind"] + str(c["records"][0][0].get("rep", ""))
                                for c in H.lzma_cases() if c["group"] == "rep_first")
    assert first == {"REP0": 3, "REP1": 3, "REP2": 3, "REP3": 3, "SR": 3}
    ends = [r for rec in _records("end_marker") for r in rec if r["kind"] == "END"]
    assert {r["len_class"] for r in ends} == {0, 2} and {r["slot"] for r in ends} == {63}
    far = [rec[-1] for rec in _records("far_direct")]
    assert {r["slot"] for r in far} == {52, 62, 63}
    # 26 direct bits in slots 62 and 63
    assert all(sum(1 for d in r["dec"] if d[0] == ("D",)) == (r["slot"] >> 1) - 5 for r in far)
    # the LZMA2 continuation: the first symbol behind the stored chunk is a rep0-long
    c = next(c for c in H.lzma2_cases() if c["group"] == "after_stored")
    rec = c["records"][0]
    k = next(i for i in range(1, len(rec)) if rec[i]["at"] < rec[i - 1]["at"])  # the new coder
    assert rec[k]["kind"] == "REP" and rec[k]["rep"] == 0 and rec[k]["state"] == 7


@pytest.mark.parametrize("plp", H.PROPS)
def test_hungry_symbols_at_every_window_fill(plp):
    """On the generator alone: the most bytes shifted out over five consecutive
    decisions anywhere in the byte-hungry set is H.HUNGRY_WINDOW, and a hungry
    symbol whose own decisions read that many begins at every window fill
    8..1.  Its decisions go against cells at their extreme: each costs more
    than 5.9 bits (probability at most 34 / 2048 for the bit taken)."""
    tag = "lc%dlp%dpb%d" % plp
    cs = [c for c in H.lzma_cases() if c["group"] == "hungry" and c["name"].endswith(tag)]
    fills = collections.defaultdict(set)
    top = 0
    for c in cs:
        rec, k = c["records"][0], c["hungry"]
        top = max(top, H.max_window([d[2] for d in H.decisions(rec)]))
        fills[H.max_window(H.hungry_reads(rec, k))].add(H.window_fill(rec, k))
        assert f"window fill {H.window_fill(rec, k)} " in c["name"]
    assert top == H.HUNGRY_WINDOW
    assert fills[H.HUNGRY_WINDOW] == set(range(1, 9))
    # each variant at every fill
    for v in ("rep3", "match", "short_rep"):
        assert {H.window_fill(c["records"][0], c["hungry"]) for c in cs
                if f"hungry {v} " in c["name"]} == set(range(1, 9)), v


@pytest.mark.parametrize("plp", H.PROPS)
def test_hungry_decisions_go_against_trained_cells(plp):
    """Replay of the record's decisions over the cells: the probability each
    hungry decision met for the bit it took."""
    tag = "lc%dlp%dpb%d" % plp
    want = {"rep3": ["M", "R", "G0", "G1", "G2", "Rc"],
            "match": ["M", "R", "Lc", "Lc2", "Lhi"],
            "short_rep": ["M", "R", "G0", "R0L"]}
    for v, keys in want.items():
        c = next(c for c in H.lzma_cases() if c["name"] == f"hungry {v} at window fill 8 {tag}")
        rec, k = c["records"][0], c["hungry"]
        probs = {}
        for r in rec[:k]:
            for key, b, _ in r["dec"]:
                if key != ("D",):
                    p = probs.get(key, 1024)
                    probs[key] = p - (p >> 5) if b else p + ((2048 - p) >> 5)
        met = []
        for key, b, _ in rec[k]["dec"][:len(keys)]:
            p = probs.get(key, 1024)
            met.append((key[0] if isinstance(key[0], str) else key[0][0], 2048 - p if b else p))
        assert [m[0] for m in met] == keys, met
        assert all(m[1] <= 34 for m in met), met

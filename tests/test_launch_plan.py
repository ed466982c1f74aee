"""csrc/launch_plan.h -- how every host batch call lays its streams out under
a workspace limit -- as a stand-alone sanitizer program
(tests/emu_hostplan/launch_plan_check.cpp: g++ -Wall -Werror -O1
-fsanitize=address,undefined, own main, run as a child process), against the
algorithm restated here: a stable sort by descending work, then a greedy cut.
order, ws_off, cut and ws_max are compared exactly, and the properties the
callers rely on are asserted on their own."""
import os
import random
import subprocess

import pytest

import native

SRC = os.path.join(native.ROOT, "tests", "emu_hostplan", "launch_plan_check.cpp")
CSRC = os.path.join(native.ROOT, "lzma-sdk-zliblike_amd", "csrc")


def plan(limit, items):
    """items: (work, slice) per index.  None: one slice alone exceeds the limit."""
    order = sorted(range(len(items)), key=lambda i: -items[i][0])   # sorted() is stable
    ws_off, cut, cur, ws_max = [], [0], 0, 0
    for k, i in enumerate(order):
        need = items[i][1]
        if need > limit:
            return None
        if cur + need > limit:
            cut.append(k)
            cur = 0
        ws_off.append(cur)
        cur += need
        ws_max = max(ws_max, cur)
    return order, ws_off, cut + [len(items)], ws_max


def limits_of(items):
    s = [x[1] for x in items] or [1]
    return sorted({max(1, min(s)), max(1, max(s)), max(1, sum(s)), max(1, sum(s) - 1), 1,
                   max(s) + 1, sum(s) + 7})


def cases():
    rng = random.Random(20260)
    out = []
    fixed = [
        [],
        [(5, 0)],
        [(5, 16)],
        [(1, 16), (1, 16), (1, 16), (1, 16)],                  # equal keys: index order
        [(3, 0), (9, 0), (3, 0)],                              # refused descriptors only
        [(7, 32), (7, 0), (9, 32), (7, 32), (0, 32), (9, 0)],  # zero slices between full ones
        [(1, 10), (2, 20), (3, 30), (4, 40)],
        [(4, 40), (3, 30), (2, 20), (1, 10)],
        [(2, 1 << 40), (1, 1 << 40), (3, (1 << 40) + 16)],     # above 2^32
    ]
    for items in fixed:
        out += [(lim, items) for lim in limits_of(items)]
    while len(out) < 400:
        n = rng.randrange(0, 41)
        sizes = rng.choice([(0, 16, 32), (0, 256, 4096, 65536), tuple(range(0, 200, 8))])
        works = rng.choice([(1,), (0, 1, 2), tuple(range(50))])
        items = [(rng.choice(works), rng.choice(sizes)) for _ in range(n)]
        for lim in rng.sample(limits_of(items), min(3, len(limits_of(items)))):
            out.append((lim, items))
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostplan")
    exe = str(d / "launch_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    cs = cases()
    path = str(d / "cases.txt")
    with open(path, "w") as f:
        for lim, items in cs:
            f.write("%d %d %s\n" % (lim, len(items), " ".join("%d %d" % x for x in items)))
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cs)
    got = []
    for line in lines:
        if line == "over":
            got.append(None)
            continue
        head, order, ws_off, cut = (part.split() for part in line.split("|"))
        assert head[0] == "ok"
        got.append(([int(v) for v in order], [int(v) for v in ws_off], [int(v) for v in cut],
                    int(head[1])))
    return cs, got


def test_the_case_list_covers_what_it_claims():
    cs = cases()
    assert len(cs) >= 400
    assert {len(items) for _, items in cs} >= {0, 1, 2, 40}
    assert any(plan(lim, items) is None for lim, items in cs)
    assert any(lim == 1 for lim, _ in cs)
    assert any(any(s == lim for _, s in items) for lim, items in cs)          # slice == limit
    assert any(items and lim == sum(s for _, s in items) for lim, items in cs)
    assert any(items and lim == sum(s for _, s in items) - 1 for lim, items in cs)
    assert any(len({w for w, _ in items}) < len(items) for _, items in cs)    # equal keys
    assert any(any(s == 0 for _, s in items) for _, items in cs)
    assert any(p is not None and len(p[2]) > 3 for p in (plan(*c) for c in cs))


def test_program_equals_the_restated_algorithm(answers):
    cs, got = answers
    for (lim, items), g in zip(cs, got):
        assert g == plan(lim, items), (lim, items)


def test_properties_of_every_plan(answers):
    cs, got = answers
    for (lim, items), g in zip(cs, got):
        n = len(items)
        if any(s > lim for _, s in items):
            assert g is None, (lim, items)    # reported, nothing returned
            continue
        order, ws_off, cut, ws_max = g
        assert sorted(order) == list(range(n))
        works = [items[i][0] for i in order]
        assert works == sorted(works, reverse=True)
        assert all(a < b for a, b, wa, wb in zip(order, order[1:], works, works[1:]) if wa == wb)
        assert cut[0] == 0 and cut[-1] == n and len(ws_off) == n
        totals = []
        for lo, hi in zip(cut, cut[1:]):
            assert hi > lo or n == 0              # no empty launch
            at = 0
            for k in range(lo, hi):
                assert ws_off[k] == at            # restart at 0, contiguous inside
                at += items[order[k]][1]
            assert at <= lim
            totals.append(at)
            # greedy: the launch ended only because the next slice did not fit
            assert hi == n or at + items[order[hi]][1] > lim
        assert ws_max == max(totals)
        if lim >= sum(s for _, s in items):
            assert len(cut) == 2

# Analysis only (not product, not test): dependent global round trips per
# match-path entry of the throughput kernel on config-3 streams, as the code
# issued them before round 9 and under each switch of LZGPU_MP (lzma_device.h;
# DESIGN.md section 4, round 9).
#
#   python3 scripts/analysis/mp_replay.py [streams=256]
#
# Streams, trace and the 32-lane / 8-literal replay are fuse_replay.py's.  A
# round trip = one load batch whose address needs a decision made on the batch
# before it; a wave pays it whatever number of its lanes need it.  Chain of an
# entry (F1 + F2 fusions in, as shipped since round 7):
#   IsRep0Long (rep0 lanes), choice, choice2 (some lane behind choice = 1), the
#   fused low / mid walk, LenHigh level by level, the slot tree's two batches,
#   the tail's first batch (some lane with >= 3 reverse bits), the tail's last
#   levels one by one, the copy's load and the matched byte behind it.
# Switches:
#   1  length front: choice + choice2 + low / mid in one batch issued at IsRep
#      (IsRep0Long flies beside it: the chain pays the longer of the two, one)
#   2  LenHigh in 3 batches
#   4  tail: first batch issued before the direct bits -- counted as hidden
#      when some lane of the entry runs >= 4 direct bits (about one round trip
#      of wave time), else still paid -- and the last levels in one batch
#   8  slot top issued early: saves its trip only when every match lane's
#      lstate is known before the low tree ends (no match length <= 5)
import os
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_replay as F  # noqa: E402


def entry_trips(ms, sw):
    """Dependent round trips of one entry (ms: the lanes' match symbols)."""
    t = Counter()
    rep0 = any(m[0] == 'SR' or (m[0] == 'REP' and m[1] == 0) for m in ms)
    lens = [m[2] if m[0] == 'REP' else m[1] for m in ms if m[0] != 'SR']
    lo, mid, hi = 0 in lens, 1 in lens, 2 in lens
    if sw & 1:
        t['rep0long+front'] = 1 if (rep0 or lens) else 0
    else:
        t['rep0long'] = 1 if rep0 else 0
        if lens:
            t['choice'] = 1
            t['choice2'] = 1 if (mid or hi) else 0
            t['low/mid'] = 1 if (lo or mid) else 0
    if hi:
        t['lenhigh'] = 3 if sw & 2 else 8
    ma = [m for m in ms if m[0] == 'MA']
    if ma:
        early = (sw & 8) and all(m[3] > 5 for m in ma)
        t['slot'] = 1 if early else 2
        rb = [((m[2] >> 1) - 1 if m[2] < 14 else 4) for m in ma if m[2] >= 4]
        dbits = max([(m[2] >> 1) - 5 for m in ma if m[2] >= 14], default=0)
        if rb:
            first = 1 if max(rb) >= 3 else 0
            rest = max(n - 3 if n >= 3 else n for n in rb)
            if sw & 4:
                first = 0 if (first and dbits >= 4) else first
                rest = 1 if rest else 0
            t['tail first'] = first
            t['tail rest'] = rest
    if any(m[0] != 'SR' for m in ms) or ms:
        t['copy+matched byte'] = 2
    return t


def main():
    import lzma
    import numpy as np
    import native
    plain = np.zeros(F.COUNT * F.N, dtype=np.uint8)
    native.synth().synth_batch(0, 0, plain.ctypes.data, F.N, F.COUNT, 8)
    filt = [{"id": lzma.FILTER_LZMA1, "dict_size": 4096, "lc": 0, "lp": 0, "pb": 0, "preset": 6}]
    T = []
    for s in range(F.COUNT):
        p = plain[s * F.N:(s + 1) * F.N].tobytes()
        comp = lzma.compress(p, format=lzma.FORMAT_RAW, filters=filt)
        o, syms = F.trace(comp)
        assert o == p, s
        T.append((len(comp), syms))
    T.sort(key=lambda t: t[0])
    waves = [[t[1] for t in T[i:i + F.LANES]] for i in range(0, F.COUNT - F.LANES + 1, F.LANES)]
    cols = [('now', 0), ('1', 1), ('2', 2), ('4', 4), ('8', 8), ('1+2+4', 7), ('all', 15)]
    tot = {n: Counter() for n, _ in cols}
    cls = Counter()
    entries = 0
    for w in waves:
        lanes = [F.passes(s) for s in w]
        for p in range(max(len(x) for x in lanes)):
            ms = [x[p][1] for x in lanes if p < len(x) and x[p][1] is not None]
            if not ms:
                continue
            entries += 1
            for n, sw in cols:
                tot[n].update(entry_trips(ms, sw))
            lens = [m[2] if m[0] == 'REP' else m[1] for m in ms if m[0] != 'SR']
            cls['lanes'] += len(ms)
            cls['choice 0 and 1 together'] += 1 if 0 in lens and (1 in lens or 2 in lens) else 0
            cls['choice 1 only'] += 1 if lens and 0 not in lens else 0
            cls['LenHigh'] += 1 if 2 in lens else 0
            ma = [m for m in ms if m[0] == 'MA']
            cls['some match'] += 1 if ma else 0
            cls['SpecPos with 4-5 bits'] += 1 if any(10 <= m[2] < 14 for m in ma) else 0
            cls['Align (direct bits)'] += 1 if any(m[2] >= 14 for m in ma) else 0
            cls['>= 4 direct bits'] += 1 if any(m[2] >= 18 for m in ma) else 0
            cls['match <= 4 beside a longer one'] += 1 if ma and min(m[3] for m in ma) <= 4 < max(
                m[3] for m in ma) else 0
            cls['no match <= 4'] += 1 if ma and min(m[3] for m in ma) > 4 else 0
            cls['no match <= 5 (slot top early pays)'] += 1 if ma and min(m[3] for m in ma) > 5 else 0
    nw = len(waves)
    print('%d streams, %d waves, %.0f entries per wave, %.1f lanes per entry' % (
        F.COUNT, nw, entries / nw, cls['lanes'] / entries))
    keys = []
    for n, _ in cols:
        for k in tot[n]:
            if k not in keys:
                keys.append(k)
    print('dependent global round trips per entry' + ''.join('%9s' % n for n, _ in cols))
    for k in keys:
        print('%-38s' % k + ''.join('%9.2f' % (tot[n].get(k, 0) / entries) for n, _ in cols))
    s = {n: sum(tot[n].values()) / entries for n, _ in cols}
    print('%-38s' % 'total' + ''.join('%9.2f' % s[n] for n, _ in cols))
    print('%-38s' % 'against now' + ''.join('%9.2f' % (s[n] - s['now']) for n, _ in cols))
    print('share of entries that hold')
    for k, v in cls.items():
        if k != 'lanes':
            print('  %-38s %5.1f %%' % (k, 100.0 * v / entries))


if __name__ == '__main__':
    main()

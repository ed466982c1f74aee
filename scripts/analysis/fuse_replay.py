# Analysis only (not product, not test): wave-level decision slots of the
# throughput kernel's symbol loop on config-3 streams, as the code issues them
# now and with the fused walks of LZGPU_FUSE (lzma_device.h; DESIGN.md section 4,
# round 7).  One slot = one decision body the wave issues, whatever number of
# its lanes use it: lanes that need the same kind of walk over different cells
# pay one EXEC-masked region after the other unless the walk is fused.
#
#   python3 scripts/analysis/fuse_replay.py [streams=256]
#
# The streams are the bench's own (synth kind 0, 4 KiB, lc0/lp0/pb0, liblzma
# preset 6), traced by a plain-Python decode as symbol_trace.py does -- per
# match: rep kind, length class, slot, length; per matched literal: the level
# of its first mismatch -- sorted by compressed length as the planner orders
# them, and replayed as 32-lane waves with the 8-literal batch policy of
# wave_replay.py (a lane's progress per pass does not depend on its neighbours:
# up to 8 literals, then the match the run ended at).
import lzma
import os
import sys
from collections import Counter

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(R, 'tests'))
sys.path.insert(0, os.path.join(R, 'lzma-sdk-zliblike_amd'))
import native  # noqa: E402

N = 4096
COUNT = int(sys.argv[1]) if len(sys.argv) > 1 else 256
LANES, BATCH = 32, 8


def trace(buf):
    """Symbols of one lc0/lp0/pb0 stream: ('L',) | ('ML', first mismatch level
    or 8) | ('SR',) | ('REP', rep 0..3, length class, length) | ('MA', length
    class, slot, length)."""
    pos = [5]
    st = [0xFFFFFFFF, int.from_bytes(buf[1:5], 'big')]
    probs = {}

    def norm():
        if st[0] < (1 << 24):
            st[0] = (st[0] << 8) & 0xFFFFFFFF
            st[1] = ((st[1] << 8) | buf[pos[0]]) & 0xFFFFFFFF
            pos[0] += 1

    def bit(key):
        p = probs.get(key, 1024)
        norm()
        b = (st[0] >> 11) * p
        if st[1] < b:
            st[0] = b
            probs[key] = p + ((2048 - p) >> 5)
            return 0
        st[0] -= b
        st[1] -= b
        probs[key] = p - (p >> 5)
        return 1

    def direct():
        norm()
        st[0] >>= 1
        if st[1] >= st[0]:
            st[1] -= st[0]
            return 1
        return 0

    def tree(pre, bits):
        m = 1
        for _ in range(bits):
            m = (m << 1) | bit((pre, m))
        return m - (1 << bits)

    out = bytearray()
    state, reps, syms = 0, [1, 1, 1, 1], []
    while len(out) < N:
        if not bit(('M', state)):
            if state < 7:
                sym = 0x100 | tree('L', 8)
                syms.append(('L',))
            else:
                mb, offs, sym, lvl = out[-reps[0]], 0x100, 1, 8
                for k in range(8):
                    mb <<= 1
                    mbit = mb & offs
                    b = bit(('LM', offs + mbit + sym)) if offs else bit(('L', sym))
                    sym = (sym << 1) | b
                    if offs and (mbit != 0) != (b != 0):
                        lvl = k
                    offs = (offs & mbit) if b else (offs & ~mbit)
                syms.append(('ML', lvl))
            out.append(sym & 0xFF)
            state = 0 if state < 4 else (state - 3 if state < 10 else state - 6)
            continue
        if bit(('R', state)):
            rk = 0
            if not bit(('G0', state)):
                if not bit(('R0L', state)):
                    state = 9 if state < 7 else 11
                    out.append(out[-reps[0]])
                    syms.append(('SR',))
                    continue
            else:
                if not bit(('G1', state)):
                    d, rk = reps[1], 1
                else:
                    if not bit(('G2', state)):
                        d, rk = reps[2], 2
                    else:
                        d, rk = reps[3], 3
                        reps[3] = reps[2]
                    reps[2] = reps[1]
                reps[1] = reps[0]
                reps[0] = d
            lk, kind = 'RL', 'REP'
            state = 8 if state < 7 else 11
        else:
            lk, kind = 'LL', 'MA'
            state = 7 if state < 7 else 10
        if not bit((lk, 'c')):
            ln, lcl = tree((lk, 'lo'), 3), 0
        elif not bit((lk, 'c2')):
            ln, lcl = 8 + tree((lk, 'mid'), 3), 1
        else:
            ln, lcl = 16 + tree((lk, 'hi'), 8), 2
        if kind == 'MA':
            slot = tree(('S', min(ln, 3)), 6)
            if slot < 4:
                d = slot
            else:
                nb = (slot >> 1) - 1
                d = (2 | (slot & 1)) << nb
                if slot < 14:
                    m = 1
                    for k in range(nb):
                        b = bit(('SP', d - slot, m))
                        m = (m << 1) | b
                        d |= b << k
                else:
                    v = 0
                    for k in range(nb - 4):
                        v = (v << 1) | direct()
                    d += v << 4
                    m = 1
                    for k in range(4):
                        b = bit(('A', m))
                        m = (m << 1) | b
                        d |= b << k
            reps[3], reps[2], reps[1], reps[0] = reps[2], reps[1], reps[0], d + 1
            syms.append(('MA', lcl, slot, ln + 2))
        else:
            syms.append(('REP', rk, lcl, ln + 2))
        for _ in range(ln + 2):
            if len(out) >= N:
                break
            out.append(out[-reps[0]])
    return bytes(out), syms


def passes(syms):
    res, i = [], 0
    while i < len(syms):
        lits = []
        while i < len(syms) and len(lits) < BATCH and syms[i][0] in ('L', 'ML'):
            lits.append(syms[i])
            i += 1
        m = None
        if len(lits) < BATCH and i < len(syms):
            m = syms[i]
            i += 1
        res.append((lits, m))
    return res


def tail_now(ms):
    """(global-cell slots, direct-bit slots) of the distance tails as separate
    SpecPos and Align regions."""
    g = dbits = 0
    spec = [(m[2] >> 1) - 1 for m in ms if 4 <= m[2] < 14]
    if spec:
        g += (3 if max(spec) >= 3 else 0) + max(n - 3 if n >= 3 else n for n in spec)
    al = [(m[2] >> 1) - 5 for m in ms if m[2] >= 14]
    if al:
        dbits += max(al)
        g += 4
    return g, dbits


def tail_fused(ms):
    rb = [(m[2] >> 1) - 1 if m[2] < 14 else 4 for m in ms if m[2] >= 4]
    al = [(m[2] >> 1) - 5 for m in ms if m[2] >= 14]
    g = 0
    if rb:
        g = (3 if max(rb) >= 3 else 0) + max(n - 3 if n >= 3 else n for n in rb)
    return g, (max(al) if al else 0)


def replay(wave, f_match, f_rep, f_lit):
    """Slots of one wave: Counter of categories, plus coincidence counts."""
    c = Counter()
    lanes = [passes(s) for s in wave]
    for p in range(max(len(x) for x in lanes)):
        cur = [x[p] for x in lanes if p < len(x)]
        c['passes'] += 1
        for it in range(BATCH):
            on = [x for x in cur if len(x[0]) > it or (len(x[0]) == it and x[1] is not None)]
            if not on:
                break
            c['lds'] += 1  # IsMatch
            lits = [x[0][it] for x in cur if len(x[0]) > it]
            plain = [s for s in lits if s[0] == 'L']
            ml = [s for s in lits if s[0] == 'ML']
            if ml:
                c['ml_iters'] += 1
                c['ml_iters_with_plain'] += 1 if plain else 0
            if f_lit:
                if lits:
                    c['lds'] += 8
            else:
                if plain:
                    c['lds'] += 8
                for k in range(8):
                    # still on the matched cells at level k / already in the plain tree
                    if any(s[1] >= k for s in ml):
                        c['ml_glob'] += 1
                    if any(s[1] < k for s in ml):
                        c['ml_plain'] += 1
        ms = [x[1] for x in cur if x[1] is not None]
        if not ms:
            continue
        c['entries'] += 1
        c['entry_lanes'] += len(ms)
        c['lds'] += 1  # IsRep
        reps = [m for m in ms if m[0] in ('REP', 'SR')]
        if reps:
            c['lds'] += 1  # G0
            g0 = [m for m in reps if m[0] == 'SR' or m[1] == 0]
            g1 = [m for m in reps if m[0] == 'REP' and m[1] >= 1]
            if f_rep:
                c['glob'] += 1 if g0 or g1 else 0  # one third-level decision
                c['rep_fused_saved'] += 1 if g0 and g1 else 0
            else:
                c['glob'] += 1 if g0 else 0  # IsRep0Long (a global cell)
                c['lds'] += 1 if g1 else 0   # G1
            c['lds'] += 1 if any(m[1] >= 2 for m in g1) else 0  # G2
        lens = [m[2] if m[0] == 'REP' else m[1] for m in ms if m[0] != 'SR']
        if lens:
            c['glob'] += 1  # choice
            lo, mid, hi = 0 in lens, 1 in lens, 2 in lens
            c['glob'] += 1 if mid or hi else 0  # choice2
            c['len_low_mid'] += 1 if lo and mid else 0
            c['len_hi'] += 1 if hi else 0
            c['glob'] += (3 if lo or mid else 0) if f_match else (3 * lo + 3 * mid)
            c['glob'] += 8 if hi else 0
        ma = [m for m in ms if m[0] == 'MA']
        if ma:
            c['glob'] += 6  # slot
            c['spec_align'] += 1 if any(4 <= m[2] < 14 for m in ma) and any(m[2] >= 14 for m in ma) else 0
            g, d = (tail_fused if f_match else tail_now)(ma)
            c['glob'] += g
            c['direct'] += d
    return c


def main():
    plain = np.zeros(COUNT * N, dtype=np.uint8)
    native.synth().synth_batch(0, 0, plain.ctypes.data, N, COUNT, 8)
    filt = [{"id": lzma.FILTER_LZMA1, "dict_size": 4096, "lc": 0, "lp": 0, "pb": 0, "preset": 6}]
    T = []
    for s in range(COUNT):
        p = plain[s * N:(s + 1) * N].tobytes()
        comp = lzma.compress(p, format=lzma.FORMAT_RAW, filters=filt)
        o, syms = trace(b'\x00' * 0 + comp)
        assert o == p, s
        T.append((len(comp), syms))
    T.sort(key=lambda t: t[0])
    lens = [t[0] for t in T]
    print('streams %d, compressed length %.0f +- %.0f (min %d, max %d)' % (
        COUNT, np.mean(lens), np.std(lens), min(lens), max(lens)))
    waves = [[t[1] for t in T[i:i + LANES]] for i in range(0, COUNT - LANES + 1, LANES)]
    cols = [('now', (False, False, False)), ('F1+F2', (True, False, False)),
            ('F1+F2+F3', (True, True, False)), ('F1+F2+F4', (True, False, True)),
            ('all', (True, True, True))]
    res = {}
    for name, f in cols:
        tot = Counter()
        for w in waves:
            tot.update(replay(w, *f))
        res[name] = {k: v / len(waves) for k, v in tot.items()}
    rows = [('match-path decisions on global cells', 'glob'),
            ('matched literal: global-cell levels', 'ml_glob'),
            ('matched literal: plain-tree levels', 'ml_plain'),
            ('LDS decisions', 'lds'), ('direct bits', 'direct')]
    print('per wave of %d streams (%d waves)%s' % (LANES, len(waves), ''.join('%12s' % n for n, _ in cols)))
    for label, k in rows:
        print('%-44s' % label + ''.join('%12.0f' % res[n].get(k, 0) for n, _ in cols))
    tot = {n: sum(res[n].get(k, 0) for _, k in rows) for n, _ in cols}
    print('%-44s' % 'total slots' + ''.join('%12.0f' % tot[n] for n, _ in cols))
    print('%-44s' % 'against now' + ''.join('%11.1f%%' % (100 * (tot[n] / tot['now'] - 1)) for n, _ in cols))
    r = res['now']
    print('passes %.0f, match-path entries %.0f with %.1f lanes; low+mid together in %.0f, LenHigh in %.0f, '
          'SpecPos+Align together in %.0f; matched-literal iterations %.0f, %.0f with plain lanes beside' % (
              r['passes'], r['entries'], r['entry_lanes'] / r['entries'], r['len_low_mid'], r['len_hi'],
              r['spec_align'], r['ml_iters'], r['ml_iters_with_plain']))
    lane = sum(len(s) for _, s in T) / COUNT
    print('symbols per stream %.0f' % lane)


if __name__ == '__main__':
    main()

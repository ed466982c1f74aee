"""Symbol-level LZMA encoder -- TEST INFRASTRUCTURE (fixture generation only).

Writes an LZMA stream from an explicit list of symbols (literals and plain
matches with chosen distances and lengths), so a test can place a match
exactly where it wants one.  Its probability model is the decoder's
(LzmaDec.c:131-426: IsMatch / IsRep, the literal and matched-literal trees,
the length coder, slot / SpecPos / direct / align distance coding), and it
tracks the bytes a DECODER produces -- including a decoder whose dictionary
is a ring smaller than the distances it is asked to reach (LzmaDec_DecodeToBuf
over a caller-owned `dic` of `ring` bytes), where the reference reads the ring
slot `dicPos - rep0 + dicBufSize` (LzmaDec.c:176, :388-407) rather than the
true history byte.  Parity is pinned on the reference's own LzmaDec.c decoding
these streams (tests/test_dropin_mirror.py), never on this encoder.

For the hand-made decoder set (tests/handmade_cases.py) it also writes the
symbols no encoder emits where the decoder must deal with them: rep0-long,
rep1..3 and short rep at any point (Encoder.rep, Encoder.short_rep), a plain
match with any 32-bit distance index (Encoder.raw_match), an end marker of any
length (Encoder.end_marker), and the pieces of an LZMA2 stream: a fresh range
coder over the kept model (Encoder.restart_rc), a state reset
(Encoder.reset_state) and the chunk headers (lz_chunk, copy_chunk).  The
encoder keeps a record of what it wrote (Encoder.record): per symbol the kind,
the state before it, the length class, the distance slot, every decision as
(cell key, bit, bytes shifted out by it) and the bytes shifted out before it.
"""
import random

K_TOP = 1 << 24


class _Rc:
    def __init__(self):
        self.low, self.range, self.cache, self.cache_size = 0, 0xFFFFFFFF, 0, 1
        self.out = bytearray()
        self.probs = {}
        self.log = []    # decisions of the symbol being coded: (key, bit, bytes shifted out)
        self.shifts = 0  # bytes shifted out by normalisation: the decoder has read 5 + shifts

    def _shift_low(self):
        if self.low < 0xFF000000 or self.low >= (1 << 32):
            carry = self.low >> 32
            temp = self.cache
            while True:
                self.out.append((temp + carry) & 0xFF)
                temp = 0xFF
                self.cache_size -= 1
                if self.cache_size == 0:
                    break
            self.cache = (self.low >> 24) & 0xFF
        self.cache_size += 1
        self.low = (self.low & 0x00FFFFFF) << 8

    def bit(self, key, b):
        p = self.probs.get(key, 1024)
        bound = (self.range >> 11) * p
        if b == 0:
            self.range = bound
            self.probs[key] = p + ((2048 - p) >> 5)
        else:
            self.low += bound
            self.range -= bound
            self.probs[key] = p - (p >> 5)
        n = 0
        while self.range < K_TOP:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self._shift_low()
            n += 1
        self.shifts += n
        self.log.append((key, b, n))

    def direct(self, v, n):
        for i in reversed(range(n)):
            self.range >>= 1
            b = (v >> i) & 1
            if b:
                self.low += self.range
            k = 0
            while self.range < K_TOP:
                self.range = (self.range << 8) & 0xFFFFFFFF
                self._shift_low()
                k += 1
            self.shifts += k
            self.log.append((("D",), b, k))

    def tree(self, pre, v, bits):
        m = 1
        for i in reversed(range(bits)):
            b = (v >> i) & 1
            self.bit((pre, m), b)
            m = (m << 1) | b

    def rtree(self, pre, v, bits):
        m = 1
        for i in range(bits):
            b = (v >> i) & 1
            self.bit((pre, m), b)
            m = (m << 1) | b

    def flush(self):
        for _ in range(5):
            self._shift_low()
        return bytes(self.out)


class Encoder:
    """Encode symbols while modelling the decoder's output in a dictionary of
    `ring` bytes (0: a flat dictionary)."""

    def __init__(self, lc=3, lp=0, pb=2, ring=0):
        self.lc, self.lp, self.pb = lc, lp, pb
        self.ring = ring
        self.rc = _Rc()
        self.state = 0
        self.reps = [1, 1, 1, 1]
        self.total = 0          # processedPos
        self.out = bytearray()  # what the decoder outputs, in order
        self.dic = bytearray(ring) if ring else None
        self.record = []        # one dict per symbol written (see _begin)

    def _begin(self, kind, **kw):
        """Open a symbol's record: kind L / ML / MA / REP / SR / END, the state and
        the position before it, and the bytes the range coder had shifted out."""
        self.rc.log = []
        r = dict(kind=kind, state=self.state, pos=self.total, at=self.rc.shifts, len_class=None,
                 slot=None, dec=self.rc.log)
        r.update(kw)
        self.record.append(r)
        return r

    # the decoder's dictionary byte at distance d before the next position
    def back(self, d):
        if not self.ring:
            return self.out[-d]
        q = self.total % self.ring
        i = q - d + (self.ring if q < d else 0)
        if i < 0:
            raise ValueError("ring read out of range (the reference would read outside dic)")
        return self.dic[i]

    def _put(self, b):
        if self.ring:
            self.dic[self.total % self.ring] = b
        self.out.append(b)
        self.total += 1

    def literal(self, byte):
        ps = self.total & ((1 << self.pb) - 1)
        rec = self._begin("L" if self.state < 7 else "ML")
        self.rc.bit(("M", self.state, ps), 0)
        prev = self.back(1) if self.total else 0
        ctx = ((self.total & ((1 << self.lp) - 1)) << self.lc) + (prev >> (8 - self.lc))
        if self.state < 7:
            sym = 1
            for i in reversed(range(8)):  # the plain tree: cells ctx * 0x300 + sym
                b = (byte >> i) & 1
                self.rc.bit(("L", ctx, sym), b)
                sym = (sym << 1) | b
        else:
            mb = self.back(self.reps[0])
            # the level at which the literal leaves its match byte (8: never)
            rec["level"] = next((k for k in range(8) if ((mb ^ byte) >> (7 - k)) & 1), 8)
            offs, sym = 0x100, 1
            for i in reversed(range(8)):
                b = (byte >> i) & 1
                mb <<= 1
                mbit = mb & offs
                self.rc.bit(("L", ctx, offs + mbit + sym), b)
                sym = (sym << 1) | b
                offs = (offs & mbit) if b else (offs & ~mbit)
        self.state = 0 if self.state < 4 else (self.state - 3 if self.state < 10 else self.state - 6)
        self._put(byte)

    def _length(self, ln, ps, rep=False):
        """The length coder; the rep length coder (RepLenCoder) has cells of its own."""
        c = "R" if rep else "L"
        v = ln - 2
        if v < 8:
            self.rc.bit((c + "c",), 0)
            self.rc.tree((c + "lo", ps), v, 3)
        elif v < 16:
            self.rc.bit((c + "c",), 1)
            self.rc.bit((c + "c2",), 0)
            self.rc.tree((c + "mid", ps), v - 8, 3)
        else:
            self.rc.bit((c + "c",), 1)
            self.rc.bit((c + "c2",), 1)
            self.rc.tree((c + "hi",), v - 16, 8)
        return 0 if v < 8 else (1 if v < 16 else 2)

    def _copy(self, dist, ln):
        for _ in range(ln):
            self._put(self.back(dist))

    def _distance(self, d, ln):
        """Distance index d (rep0 - 1, any 32-bit value) after a length of ln."""
        slot = d if d < 4 else (d.bit_length() - 1) * 2 + ((d >> (d.bit_length() - 2)) & 1)
        self.rc.tree(("S", min(ln - 2, 3)), slot, 6)
        if slot >= 4:
            nb = (slot >> 1) - 1
            base = (2 | (slot & 1)) << nb
            rest = d - base
            if slot < 14:
                self.rc.rtree(("SP", base - slot), rest, nb)
            else:
                self.rc.direct(rest >> 4, nb - 4)
                self.rc.rtree(("A",), rest & 15, 4)
        return slot

    def match(self, dist, ln):
        """A plain match (IsRep = 0): rep0 = dist, ln bytes (2..273)."""
        assert 2 <= ln <= 273 and 1 <= dist <= self.total
        self.raw_match(dist - 1, ln)

    def raw_match(self, index, ln, model=True):
        """A plain match with any 32-bit distance index (rep0 = index + 1; slots
        up to 63 with their 26 direct bits).  model=False writes the symbol and
        leaves the modelled output alone: for a distance the decoder must refuse."""
        assert 2 <= ln <= 273 and 0 <= index < 0xFFFFFFFF
        ps = self.total & ((1 << self.pb) - 1)
        rec = self._begin("MA")
        self.rc.bit(("M", self.state, ps), 1)
        self.rc.bit(("R", self.state), 0)
        rec["len_class"] = self._length(ln, ps)
        rec["slot"] = self._distance(index, ln)
        self.reps = [index + 1] + self.reps[:3]
        self.state = 7 if self.state < 7 else 10
        if model:
            self._copy(index + 1, ln)

    def end_marker(self, ln=2):
        """Distance index 0xFFFFFFFF with a length of ln (2..273): the end of
        the stream whatever the length (LzmaDec.c:354-359; state and reps stay)."""
        assert 2 <= ln <= 273
        ps = self.total & ((1 << self.pb) - 1)
        rec = self._begin("END")
        self.rc.bit(("M", self.state, ps), 1)
        self.rc.bit(("R", self.state), 0)
        rec["len_class"] = self._length(ln, ps)
        rec["slot"] = self._distance(0xFFFFFFFF, ln)

    def rep(self, k, ln, model=True):
        """Rep k (0: rep0-long, 1..3) of ln bytes, in the reference's decision
        order: IsRep, IsRepG0, IsRep0Long / IsRepG1, IsRepG2, the rep length
        coder (LzmaDec.c:200-292)."""
        assert 0 <= k <= 3 and 2 <= ln <= 273
        ps = self.total & ((1 << self.pb) - 1)
        rec = self._begin("REP", rep=k)
        self.rc.bit(("M", self.state, ps), 1)
        self.rc.bit(("R", self.state), 1)
        if k == 0:
            self.rc.bit(("G0", self.state), 0)
            self.rc.bit(("R0L", self.state, ps), 1)
        else:
            self.rc.bit(("G0", self.state), 1)
            if k == 1:
                self.rc.bit(("G1", self.state), 0)
            else:
                self.rc.bit(("G1", self.state), 1)
                self.rc.bit(("G2", self.state), k - 2)
            r = self.reps
            self.reps = [r[k]] + r[:k] + r[k + 1:]
        self.state = 8 if self.state < 7 else 11
        rec["len_class"] = self._length(ln, ps, rep=True)
        if model:
            self._copy(self.reps[0], ln)

    def short_rep(self, model=True):
        """One byte at rep0 (IsRepG0 = 0, IsRep0Long = 0)."""
        ps = self.total & ((1 << self.pb) - 1)
        self._begin("SR")
        self.rc.bit(("M", self.state, ps), 1)
        self.rc.bit(("R", self.state), 1)
        self.rc.bit(("G0", self.state), 0)
        self.rc.bit(("R0L", self.state, ps), 0)
        self.state = 9 if self.state < 7 else 11
        if model:
            self._copy(self.reps[0], 1)

    def stored(self, data):
        """Bytes an LZMA2 stored chunk puts into the dictionary (no symbol)."""
        for b in data:
            self._put(b)

    def restart_rc(self):
        """End the range coder and begin a new one; probabilities, state and
        reps stay (what an LZMA2 chunk of mode 0 continues from).  Returns the
        bytes of the coder that ended."""
        done = self.rc.flush()
        rc = _Rc()
        rc.probs = self.rc.probs
        self.rc = rc
        return done

    def reset_state(self):
        """Fresh probabilities, state and reps (LZMA2 chunk modes 1 to 3)."""
        self.rc.probs = {}
        self.state = 0
        self.reps = [1, 1, 1, 1]

    def fork(self, tail=None):
        """A copy that goes its own way from here (a shared prefix, several ends).
        tail: keep only the last `tail` bytes of the modelled output and the
        last symbol's record -- a cheap copy for trying a symbol out."""
        e = Encoder(self.lc, self.lp, self.pb, self.ring)
        rc = e.rc
        rc.low, rc.range, rc.cache, rc.cache_size = (self.rc.low, self.rc.range, self.rc.cache,
                                                     self.rc.cache_size)
        rc.out, rc.probs, rc.shifts = bytearray(self.rc.out), dict(self.rc.probs), self.rc.shifts
        e.state, e.reps, e.total = self.state, list(self.reps), self.total
        e.out = bytearray(self.out if tail is None else self.out[-tail:])
        e.dic = bytearray(self.dic) if self.ring else None
        e.record = list(self.record if tail is None else self.record[-1:])
        return e

    def set_props(self, lc, lp, pb):
        """New lc / lp / pb (LZMA2 chunk modes 2 and 3, with reset_state)."""
        self.lc, self.lp, self.pb = lc, lp, pb

    def finish(self):
        return self.rc.flush()


def props(lc, lp, pb, dict_size):
    return bytes([(pb * 5 + lp) * 9 + lc]) + int(dict_size).to_bytes(4, "little")


def lz_chunk(control, data, unpack, prop=None, pack=None):
    """An LZMA2 chunk of compressed data: control byte 0x80 | mode << 5 (the
    unpack size's top five bits are added here), unpack size, pack size (`pack`
    where it shall differ from len(data)), the props byte for modes 2 and 3."""
    pack = len(data) if pack is None else pack
    assert control & 0x80 and 1 <= unpack <= 1 << 21 and 1 <= pack <= 1 << 16
    head = bytes([(control & 0xE0) | ((unpack - 1) >> 16), ((unpack - 1) >> 8) & 0xFF,
                  (unpack - 1) & 0xFF, (pack - 1) >> 8, (pack - 1) & 0xFF])
    if prop is not None:
        head += bytes([prop])
    return head + bytes(data)


def copy_chunk(control, data, size=None):
    """An LZMA2 stored chunk: control 1 (dictionary reset) or 2, its size
    (`size` where it shall differ from len(data)) and the bytes."""
    size = len(data) if size is None else size
    assert 1 <= size <= 1 << 16
    return bytes([control, (size - 1) >> 8, (size - 1) & 0xFF]) + bytes(data)


def ring_reach_stream(seed, ring=4096, far=5096, total=None, lc=3, lp=0, pb=2):
    """A stream whose matches at distance `far` > `ring` read, in a decoder with
    a `ring`-byte dictionary ring, the ring slot the reference reads (the byte
    at distance far - ring), never outside the ring: a far match starts at a
    ring position >= far - ring and ends inside the ring; a matched literal
    against rep0 = far comes only from such positions; elsewhere short matches
    (distance <= 8) reset rep0.  Returns (stream, props, the decoder's output)."""
    rng = random.Random(seed)
    total = total or 5 * ring
    e = Encoder(lc, lp, pb, ring)
    for _ in range(ring):  # fill the ring
        e.literal(rng.randrange(256))
    low = far - ring
    while e.total < total:
        q = e.total % ring
        left = total - e.total
        r0_ok = e.reps[0] <= ring or q >= e.reps[0] - ring
        if q >= low and ring - q >= 2 and left >= 2 and rng.random() < 0.5:
            e.match(far, min(rng.randrange(2, 40), ring - q, left, 273))
        elif e.state < 7 or r0_ok:
            e.literal(rng.randrange(256))
        elif left >= 2:
            # rep0 = far is out of reach from here: a short match resets it
            e.match(rng.randrange(1, 9), min(rng.randrange(2, 12), left))
        else:
            break
    return e.finish(), props(lc, lp, pb, 1 << 16), bytes(e.out)


def ring_decode(lib, comp, props, ring, out_total, in_chunk, out_chunk):
    """The fork's zlib-like loop (LzmaDec_DecodeToBuf, LzmaDec.c:840-878) over a
    caller-owned dictionary ring of `ring` bytes (LzmaDec_AllocateProbs + its
    own `dic`, as LzmaDec.h allows), through `lib`: liblzmagpu.so or the
    reference's LzmaDec.c compiled in place (oracle/_ref/libref_lzma.so).
    Returns (trace of (res, status, destLen, srcLen) per call, output)."""
    import ctypes
    import lzmagpu as L
    vp = ctypes.c_void_p
    for name, args in (("LzmaDec_AllocateProbs", [vp, ctypes.c_char_p, ctypes.c_uint, vp]),
                       ("LzmaDec_Init", [vp]),
                       ("LzmaDec_DecodeToBuf", [vp, vp, vp, vp, vp, ctypes.c_int, vp]),
                       ("LzmaDec_FreeProbs", [vp, vp])):
        getattr(lib, name).argtypes = args
    lib.LzmaDec_AllocateProbs.restype = ctypes.c_int
    lib.LzmaDec_DecodeToBuf.restype = ctypes.c_int
    d = L.CLzmaDec()
    d.dic = None
    d.probs = None
    r = lib.LzmaDec_AllocateProbs(ctypes.byref(d), bytes(props), len(props), ctypes.byref(L.g_alloc))
    if r != 0:
        return [(r, -1, 0, 0)], b""
    dic = ctypes.create_string_buffer(ring)
    d.dic = ctypes.addressof(dic)
    d.dicBufSize = ring
    lib.LzmaDec_Init(ctypes.byref(d))
    src = ctypes.create_string_buffer(bytes(comp), len(comp))
    out = ctypes.create_string_buffer(max(out_total, 1))
    trace, ip, op = [], 0, 0
    try:
        while True:
            sl = ctypes.c_size_t(min(in_chunk, len(comp) - ip))
            n = min(out_chunk, out_total - op)
            dl = ctypes.c_size_t(n)
            fin = 1 if op + n == out_total else 0
            st = ctypes.c_int(-1)
            r = lib.LzmaDec_DecodeToBuf(ctypes.byref(d), ctypes.addressof(out) + op, ctypes.byref(dl),
                                        ctypes.addressof(src) + ip, ctypes.byref(sl), fin,
                                        ctypes.byref(st))
            trace.append((r, st.value, dl.value, sl.value))
            ip += sl.value
            op += dl.value
            if r != 0 or op == out_total or (dl.value == 0 and sl.value == 0) or len(trace) > 100000:
                break
    finally:
        lib.LzmaDec_FreeProbs(ctypes.byref(d), ctypes.byref(L.g_alloc))
    return trace, out.raw[:op]


def dic_calls(lib, comp, props, out_total, win, edit=None, max_calls=100000):
    """LzmaDec_DecodeToDic calls over a caller-owned flat dictionary of
    `out_total` bytes (LzmaDec_AllocateProbs + own dic), input in windows of at
    most `win` bytes, FINISH_ANY, through `lib`; edit(k, dec) runs on the host
    CLzmaDec between calls k and k + 1 (a host-side change both libraries see
    alike).  Returns (trace of (res, status, srcLen, dicPos), dictionary)."""
    import ctypes
    import lzmagpu as L
    vp = ctypes.c_void_p
    for name, args in (("LzmaDec_AllocateProbs", [vp, ctypes.c_char_p, ctypes.c_uint, vp]),
                       ("LzmaDec_Init", [vp]),
                       ("LzmaDec_DecodeToDic", [vp, ctypes.c_size_t, vp, vp, ctypes.c_int, vp]),
                       ("LzmaDec_FreeProbs", [vp, vp])):
        getattr(lib, name).argtypes = args
    lib.LzmaDec_AllocateProbs.restype = ctypes.c_int
    lib.LzmaDec_DecodeToDic.restype = ctypes.c_int
    d = L.CLzmaDec()
    d.dic = None
    d.probs = None
    r = lib.LzmaDec_AllocateProbs(ctypes.byref(d), bytes(props), len(props), ctypes.byref(L.g_alloc))
    if r != 0:
        return [(r, -1, 0, 0)], b""
    dic = ctypes.create_string_buffer(max(out_total, 1))
    d.dic = ctypes.addressof(dic)
    d.dicBufSize = out_total
    lib.LzmaDec_Init(ctypes.byref(d))
    src = ctypes.create_string_buffer(bytes(comp), len(comp))
    trace, ip = [], 0
    try:
        for k in range(max_calls):
            sl = ctypes.c_size_t(min(win, len(comp) - ip))
            st = ctypes.c_int(-1)
            pos0 = d.dicPos
            r = lib.LzmaDec_DecodeToDic(ctypes.byref(d), out_total, ctypes.addressof(src) + ip,
                                        ctypes.byref(sl), 0, ctypes.byref(st))
            trace.append((r, st.value, sl.value, d.dicPos))
            ip += sl.value
            if r != 0 or d.dicPos == out_total or (sl.value == 0 and d.dicPos == pos0):
                break
            if edit:
                edit(k, d)
    finally:
        lib.LzmaDec_FreeProbs(ctypes.byref(d), ctypes.byref(L.g_alloc))
    return trace, dic.raw[:out_total]

"""The match path's global load batches in a kernel's ISA, and where each is
first waited for (round 9, LZGPU_MP).

  python scripts/analysis/isa_mp_waits.py KERN.s SYMBOL_SUBSTR [LZMA_DEVICE_H]

KERN.s is `hipcc -O3 --offload-arch=gfx950 -S -gline-tables-only` of
csrc/lzma_kernels.hip; LZMA_DEVICE_H the header it was compiled from (default:
this tree's).  For the first function whose symbol contains SYMBOL_SUBSTR,
prints one row per batch of 16-bit global loads (probability cells) that the
line tables attribute to lz_run's match path -- from the IsRep decision to the
end of the copy:

  site    the source line of lz_run that issued the batch
  loads   load instructions of the batch (a batch ends at a vmcnt wait, a
          label, or a load of another site)
  dist    instructions from the batch's last load to the first `s_waitcnt` in
          text order whose vmcnt covers it (as isa_fetch_waits.py counts)
  blocks  basic-block labels crossed on the way
  direct  instructions of the direct-bits loop (`do rc.direct(dist)`) between
          the batch and that wait: > 0 means the batch flies across the loop
  wait    "loop" when that wait belongs to the direct-bits loop itself (the
          reader's refill inside it, taken once per 16 input bytes): then
          `dist` / `blocks` / `direct` count on to the first covering wait
          behind the loop, and `refill` is the distance to the one inside

The scan follows the text, not the control flow: exact inside a block, a lower
bound across blocks.  Then the kernel's VGPRs, scratch and occupancy.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_fetch_waits import VMCNT, VMEM, header_text, load_function  # noqa: E402

CELL = re.compile(r"^global_load_(ushort|short_d16|short_d16_hi|sshort)\b")


def main():
    path, sym = sys.argv[1], sys.argv[2]
    hdr_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "..", "lzma-sdk-zliblike_amd", "csrc",
        "lzma_device.h")
    hdr = header_text(hdr_path)
    lo = next(i for i, l in enumerate(hdr) if "rc.bit(T.template at<S_REP>(st))" in l)
    hi = next(i for i, l in enumerate(hdr) if "LZ_PROF_MARK(s, 2, t_prof);" in l)
    direct = [i for i, l in enumerate(hdr) if "do rc.direct(dist); while" in l]
    rows, meta = load_function(path, sym)
    print("==", meta.get("symbol"))
    print("match path: header lines %d-%d" % (lo, hi))

    def site(ch):
        for f, n in ch:
            if f.startswith("lzma_device") and lo <= n <= hi:
                return n
        return None

    def in_direct(ch):
        return any(f.startswith("lzma_device") and n in direct for f, n in ch)

    batches = []  # [site line, first row, last row, loads]
    cur = None
    for i, (kind, text, ch) in enumerate(rows):
        if kind == "label" or (text.startswith("s_waitcnt") and VMCNT.search(text)):
            cur = None
            continue
        if CELL.match(text):
            s = site(ch)
            if s is None:
                cur = None
                continue
            if cur is not None and cur[0] == s:
                cur[2] = i
                cur[3] += 1
            else:
                cur = [s, i, i, 1]
                batches.append(cur)
    print("%-4s %-5s %-62s %5s %5s %6s %6s %s" % ("idx", "line", "site", "loads", "dist",
                                                   "blocks", "direct", "wait"))
    for k, (s, first, last, loads) in enumerate(batches):
        issued = dist = blocks = nd = 0
        found = False
        refill = None
        for j in range(last + 1, len(rows)):
            kd, t, ch = rows[j]
            if kd == "label":
                blocks += 1
                continue
            dist += 1
            nd += 1 if in_direct(ch) else 0
            if t.startswith("s_waitcnt"):
                m = VMCNT.search(t)
                if m and int(m.group(1)) <= issued:
                    if in_direct(ch):
                        refill = dist if refill is None else refill
                        continue
                    found = True
                    break
            elif VMEM.match(t):
                issued += 1
            if t.startswith("s_endpgm"):
                break
        print("%-4d %-5d %-62s %5d %5s %6d %6d %s" % (
            k, s, hdr[s].strip()[:62], loads, dist if found else "-", blocks, nd,
            "" if refill is None else "loop (refill %d)" % refill))
    print("vgprs %s  scratch %s  occupancy %s" % (meta.get("NumVgprs"), meta.get("ScratchSize"),
                                                  meta.get("Occupancy")))


if __name__ == "__main__":
    main()

"""Where the waits of the input reader's block fetches sit in a kernel's ISA.

  python scripts/analysis/isa_fetch_waits.py KERN.s SYMBOL_SUBSTR [LZMA_DEVICE_H]

KERN.s is `hipcc -O3 --offload-arch=gfx950 -S -gline-tables-only` of
csrc/lzma_kernels.hip (or of one instantiation of its kernel template);
LZMA_DEVICE_H the header it was compiled from (default: this tree's).  For the
first function whose symbol contains SYMBOL_SUBSTR, prints one row per reader
fetch -- a `global_load_dwordx4` attributed to lzma_device.h -- with

  site    the source text of the call sites that led to the fetch: the reader
          call (topup / topup_mid / fetch_pending / next / init) and its caller
  dist    instructions from the fetch to the first `s_waitcnt` in text order
          whose vmcnt leaves fewer operations outstanding than were issued
          since the fetch, i.e. the first wait that covers it
  blocks  basic-block labels crossed on the way (0: the wait is in the block
          that issued the load, inside the same checkpoint)
  copy    "sync" when that wait is in the fetch's own block and a v_mov from
          the load's destination registers follows within 4 instructions: a
          register copy of a block still in flight.  "later" for the same
          behind a wait in another block (the block's promotion at a later
          checkpoint, or init's first block)

and after the rows: the kernel's VGPRs, scratch and SGPR spills, the count of
vmcnt waits (and of vmcnt(0) among them), and for every inlined copy of the
plain literal walk (Rc::tree8_a) whether a vmcnt wait stands between its first
instruction and its first ds_read.

The scan follows the text, not the control flow: it is exact for a wait in the
fetch's own block and a lower bound on the distance otherwise.
"""
import os
import re
import sys

LOC = re.compile(r"^\s*\.loc\s+\d+\s+(\d+)\s+\d+.*?;\s*(.*)$")
INS = re.compile(r"^\s+([a-z_][a-z0-9_]*)(\s|$)")
LBL = re.compile(r"^(\.LBB\d+_\d+):")
VMCNT = re.compile(r"vmcnt\((\d+)\)")
TUPLE = re.compile(r"v\[(\d+):(\d+)\]")
VMEM = re.compile(r"^(global|buffer|flat|scratch)_(load|store|atomic)")


def chain(comment):
    parts = re.findall(r"([\w./-]+\.(?:h|hip)):(\d+)", comment)
    return [(p.rsplit("/", 1)[-1], int(n)) for p, n in parts]


def header_text(path):
    try:
        with open(path) as f:
            return [""] + [l.rstrip("\n") for l in f]
    except OSError:
        return [""]


def walk_range(hdr):
    """Line range of Rc::tree8_a's body in the header."""
    lo = hi = 0
    for i, l in enumerate(hdr):
        if not lo and re.search(r"uint32_t tree8_a\(P probs", l):
            lo = i
        if lo and not hi and "return uint32_t((a - base) / st);" in l:
            hi = i
    return lo, hi


def load_function(path, sym):
    rows = []  # (kind, text, chain)  kind: ins / label
    on = False
    cur = []
    meta = {}
    with open(path) as f:
        for raw in f:
            if not on:
                if raw.startswith("_Z") and sym in raw.split(":")[0]:
                    on = True
                    meta["symbol"] = raw.split(":")[0]
                continue
            if raw.startswith(".Lfunc_end"):
                on = "tail"
                continue
            if on == "tail":
                for k in ("NumVgprs", "ScratchSize", "Occupancy"):
                    m = re.match(r";\s*%s:\s*(\d+)" % k, raw)
                    if m and k not in meta:
                        meta[k] = int(m.group(1))
                if raw.startswith("_Z") or ("ScratchSize" in meta and "Occupancy" in meta
                                            and "NumVgprs" in meta):
                    if raw.startswith("_Z"):
                        break
                continue
            m = LOC.match(raw)
            if m:
                cur = chain(m.group(2))
                continue
            m = LBL.match(raw)
            if m:
                rows.append(("label", m.group(1), cur))
                continue
            m = INS.match(raw)
            if not m or raw.strip().startswith("."):
                continue
            rows.append(("ins", raw.strip().split(";")[0].strip(), cur))
    # SGPR spills of this kernel from the metadata block
    with open(path) as f:
        txt = f.read()
    blk = re.search(r"(\.sgpr_spill_count:\s+(\d+)\s*\n(?:.*\n){0,12}?\s*\.symbol:\s+%s\.kd)"
                    % re.escape(meta.get("symbol", "?")), txt)
    if blk:
        meta["sgpr_spill"] = int(blk.group(2))
    return rows, meta


def main():
    path, sym = sys.argv[1], sys.argv[2]
    hdr_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "..", "lzma-sdk-zliblike_amd", "csrc",
        "lzma_device.h")
    hdr = header_text(hdr_path)
    rows, meta = load_function(path, sym)
    print("==", meta.get("symbol"))
    n_wait = n_wait0 = 0
    for kind, text, _ in rows:
        if kind == "ins" and text.startswith("s_waitcnt"):
            m = VMCNT.search(text)
            if m:
                n_wait += 1
                n_wait0 += m.group(1) == "0"

    def src(n):
        return hdr[n].strip() if 0 < n < len(hdr) else str(n)

    print("%-4s %-58s %5s %6s %6s" % ("idx", "site", "dist", "blocks", "copy"))
    k = 0
    for i, (kind, text, ch) in enumerate(rows):
        if kind != "ins" or not text.startswith("global_load_dwordx4"):
            continue
        if not ch or not ch[0][0].startswith("lzma_device"):
            continue
        dst = TUPLE.search(text)
        lo, hi = (int(dst.group(1)), int(dst.group(2))) if dst else (-1, -1)
        dev = [n for f, n in ch if f.startswith("lzma_device")]
        call = next((j for j, n in enumerate(dev)
                     if re.search(r"topup|next\(\)|init\(|fetch_pending", src(n))), 1)
        site = " < ".join(src(n)[:27] for n in dev[call:call + 2])
        issued = dist = blocks = 0
        found = None
        for j in range(i + 1, len(rows)):
            kd, t, _ = rows[j]
            if kd == "label":
                blocks += 1
                continue
            dist += 1
            if t.startswith("s_waitcnt"):
                m = VMCNT.search(t)
                if m and int(m.group(1)) <= issued:
                    found = j
                    break
            elif VMEM.match(t):
                issued += 1
            if t.startswith("s_endpgm"):
                break
        copy = "no"
        if found is not None:
            seen = 0
            for j in range(found + 1, len(rows)):
                kd, t, _ = rows[j]
                if kd != "ins":
                    continue
                seen += 1
                if seen > 4:
                    break
                if t.startswith("v_mov"):
                    srcop = t.split(None, 1)[1].split(",")[-1].strip()
                    m = TUPLE.match(srcop)
                    a = b = None
                    if m:
                        a, b = int(m.group(1)), int(m.group(2))
                    elif re.match(r"v(\d+)$", srcop):
                        a = b = int(srcop[1:])
                    if a is not None and lo <= a and b <= hi:
                        copy = "sync" if blocks == 0 else "later"
        print("%-4d %-58s %5s %6d %6s" % (k, site, dist if found is not None else "-", blocks, copy))
        k += 1
    # every inlined copy of the plain literal walk: a vmcnt wait before its first ds_read?
    w_lo, w_hi = walk_range(hdr)
    inside = False
    heads = []
    for kind, text, ch in rows:
        if kind != "ins":
            continue
        in_walk = any(f.startswith("lzma_device") and w_lo <= n <= w_hi for f, n in ch)
        if in_walk and not inside:
            heads.append(None)  # a walk begins; None: its first ds_read not seen yet
        inside = in_walk
        if in_walk and heads and heads[-1] is None:
            if text.startswith("s_waitcnt") and VMCNT.search(text):
                heads[-1] = "vmcnt wait"
            elif text.startswith("ds_read"):
                heads[-1] = "none"
    heads = [h for h in heads if h is not None]
    print("plain literal walk (tree8_a, header lines %d-%d), wait before the first ds_read of "
          "each entry: %s" % (w_lo, w_hi, ", ".join(heads[:4]) if heads else "walk not found"))
    print("vgprs %s  scratch %s  sgpr_spill %s  occupancy %s" % (
        meta.get("NumVgprs"), meta.get("ScratchSize"), meta.get("sgpr_spill"), meta.get("Occupancy")))
    print("vmcnt waits %d, of them vmcnt(0) %d" % (n_wait, n_wait0))


if __name__ == "__main__":
    main()

"""Writes tests/golden/decode_plan_cases.json: what LzmaGpu_PlanBatchOpt answers
for the matrix of tests/decode_plan_cases.py -- the whole LzmaGpuPlan, every
probs_off and the lane order of each case (above 64 items the two arrays as
their CRC-32, so that the file stays small).

The file pins the planner across refactors: it was recorded from the library
built at the commit before the planner moved to csrc/decode_plan.h, and is to
be regenerated only by a change that means to alter plans.  Planning
initialises no device, so this runs anywhere the library is built:
    python tests/golden/make_golden_decode_plan.py [root of the tree whose library plans]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "lzma-sdk-zliblike_amd"))
sys.path.insert(0, os.path.dirname(HERE))

import decode_plan_cases as C  # noqa: E402
import lzmagpu as L  # noqa: E402


def main():
    out, masks, descs = [], set(), {}
    for name, n, o in C.cases():
        if (name, n) not in descs:
            descs[name, n] = C.make_descs(L, name, n)
        r = C.run_case(L, descs[name, n], n, o)
        assert r["res"] == 0, (name, n, o, r["res"])
        p = r["plan"]
        masks |= {p[10 + 10 * k + 5] for k in range(p[9])}
        out.append(dict(set=name, n=n, opt=o, **r))
    # every placement the planner can hand the launcher (the seventh mask the
    # launcher knows, 0x7FF | COOP with the window bit, is chosen at launch)
    assert masks == C.PLAN_MASKS, sorted(hex(m) for m in masks)
    path = os.path.join(HERE, "decode_plan_cases.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in out) + "\n]\n")
    print(f"{len(out)} cases, {os.path.getsize(path)} bytes, masks {sorted(hex(m) for m in masks)}")


if __name__ == "__main__":
    main()

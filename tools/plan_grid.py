#!/usr/bin/env python3
"""Write tests/golden/plan_names.json: the plan name gasalx_describe_plan gives for every row of
the grid of tests/test_capi.py (plan_grid_names), from the library GASALX_LIB names (default: this
tree's build).  No GPU needed.

usage: GASALX_LIB=/path/to/parent/libgasal.so plan_grid.py COMMIT [OUT.json]

The fixture pins the planner across host-side refactors, so it is written from a build of the
commit *before* the change under test (COMMIT, recorded in the file), never from the branch.
Names are stored once; rows are run-length encoded as a flat list: name index, count, name index, count, ...
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "genomics-gpu_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import test_capi as T  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "plan_names.json")
    rows = T.plan_grid_names(os.environ.__setitem__, lambda s: os.environ.pop(s, None))
    names = sorted(set(rows))
    index = {n: i for i, n in enumerate(names)}
    runs = []
    for r in rows:
        if runs and runs[-2] == index[r]:
            runs[-1] += 1
        else:
            runs += [index[r], 1]
    doc = {"commit": commit, "lens": list(T.PLAN_LENS), "scores": [list(s) for s in T.PLAN_SCORES],
           "envs": list(T.PLAN_ENVS), "rows": len(rows), "names": names, "runs": runs}
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(rows)} rows, {len(names)} names, {len(runs) // 2} runs, {os.path.getsize(out)} bytes -> {out}")


if __name__ == "__main__":
    main()

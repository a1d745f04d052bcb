#!/usr/bin/env python3
"""Write tests/golden/plan_names.json: the plan name gasalx_describe_plan gives for every row of
the grid of tests/test_capi.py (plan_grid_names), from the library GASALX_LIB names (default: this
tree's build).  No GPU needed.  With --nv: tests/golden/nv_plan_names.json, the names
gasalx_nv_describe_plan and gasalx_nv_describe_sinks_plan give over nv_plan_grid_names' grid.

With --semi-cigar: tests/golden/semi_cigar_plan_names.json, the names (or refusals)
gasalx_describe_semi_cigar_plan gives over the grid of tests/test_semi_cigar_model.py, one row per key.

With --semi-cigar-head: tests/golden/semi_cigar_head_plan_names.json, the same for
gasalx_describe_semi_cigar_head_plan over the four heads (tests/test_semi_cigar_head_model.py).

usage: GASALX_LIB=/path/to/parent/libgasal.so plan_grid.py [--nv | --semi-cigar | --semi-cigar-head] COMMIT [OUT.json]

A fixture pins its planner across host-side refactors, so it is written from a build of the
commit *before* the change under test (COMMIT, recorded in the file), never from the branch.
Names are stored once; rows are run-length encoded as a flat list: name index, count, name index, count, ...
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "genomics-gpu_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import test_capi as T  # noqa: E402


def semi_cigar(commit, out):
    import test_semi_cigar_model as S
    rows = S.semi_cigar_plan_rows(os.environ.__setitem__, lambda s: os.environ.pop(s, None))
    doc = {"commit": commit, "lens": list(S.PLAN_LENS), "scores": [list(s) for s in S.PLAN_SCORES],
           "envs": list(S.PLAN_ENVS), "rows": rows}
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rows)} rows -> {out}")


def semi_cigar_head(commit, out):
    import test_semi_cigar_head_model as S
    rows = S.semi_cigar_head_plan_rows(os.environ.__setitem__, lambda s: os.environ.pop(s, None))
    doc = {"commit": commit, "lens": list(S.PLAN_LENS), "scores": [list(s) for s in S.PLAN_SCORES],
           "envs": list(S.PLAN_ENVS), "heads": ["hn", "hq", "ht", "hb"], "rows": rows}
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rows)} rows -> {out}")


def main():
    nv = "--nv" in sys.argv
    args = [a for a in sys.argv[1:] if a not in ("--nv", "--semi-cigar", "--semi-cigar-head")]
    commit = args[0]
    if "--semi-cigar-head" in sys.argv:
        return semi_cigar_head(commit, args[1] if len(args) > 1 else
                               os.path.join(ROOT, "tests", "golden", "semi_cigar_head_plan_names.json"))
    if "--semi-cigar" in sys.argv:
        return semi_cigar(commit, args[1] if len(args) > 1 else
                          os.path.join(ROOT, "tests", "golden", "semi_cigar_plan_names.json"))
    out = args[1] if len(args) > 1 else os.path.join(ROOT, "tests", "golden",
                                                     "nv_plan_names.json" if nv else "plan_names.json")
    grid = T.nv_plan_grid_names if nv else T.plan_grid_names
    rows = grid(os.environ.__setitem__, lambda s: os.environ.pop(s, None))
    names = sorted(set(rows))
    index = {n: i for i, n in enumerate(names)}
    runs = []
    for r in rows:
        if runs and runs[-2] == index[r]:
            runs[-1] += 1
        else:
            runs += [index[r], 1]
    if nv:
        doc = {"commit": commit, "plens": list(T.NV_PLAN_PLENS), "tlens": list(T.NV_PLAN_TLENS),
               "scores": [list(s) for s in T.NV_PLAN_SCORES], "envs": list(T.NV_PLAN_ENVS)}
    else:
        doc = {"commit": commit, "lens": list(T.PLAN_LENS), "scores": [list(s) for s in T.PLAN_SCORES],
               "envs": list(T.PLAN_ENVS)}
    doc.update(rows=len(rows), names=names, runs=runs)
    with open(out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(rows)} rows, {len(names)} names, {len(runs) // 2} runs, {os.path.getsize(out)} bytes -> {out}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Throughput of the quality-aware banded Gotoh kernels (gasalx_nv_banded_qual_score_device and
gasalx_nv_banded_qual_traceback_device, csrc/nvbanded_qual.hpp) beside the plain entry points they
restate (gasalx_nv_banded_score_sinks_device, gasalx_nv_banded_traceback_device) on the same data in
the same process: reads of 150 symbols against genome windows of 181 (4-bit big-endian reads, 2-bit
little-endian windows, the shape of nv_banded_sinks_probe.py), Gotoh SEMI_GLOBAL, bands 7, 15 and 31,
inputs and outputs resident in HBM.  Per band, packed (two pairs per lane) and int32 (GASALX_NVB16=0):
  qual_default   the quality scorer with nvBowtie's default tables (match 0, mismatch -QualCost(2, 6))
  qual_const     the same kernel with constant tables (0, -6)
  plain          the plain scorer with sinks under the constant scheme (0, -6): the yardstick
then the quality traceback (default tables) beside the plain banded traceback (0, -6).  Gaps -8 / -3
throughout.  The calls alternate inside every repeat, each launch timed on its own with HIP events
after warm-up launches; the median and the spread (min, max) of the repeats are reported.  The constant
tables' outputs are compared with the plain calls' once.  Prints one JSON line per band and family.

usage: nv_qual_probe.py [pairs] [repeats]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomics-gpu_amd"))
import gasal_ffi as G  # noqa: E402


def timed(calls, stream, warmup, reps):
    """calls: name -> launch; the launches alternate, one event pair around each."""
    for _ in range(warmup):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in ms.items()}


def qual_cost(lo, hi):
    f = np.float32
    return [lo + int(f(f(min(q, 40)) / f(40.0)) * f(hi - lo)) for q in range(256)]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    m, tl = 150, 181
    rng = np.random.default_rng(0x5EED09A1)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    texts = rng.integers(0, 4, (n, tl))
    st = rng.integers(0, 16, n)
    pats = texts[np.arange(n)[:, None], st[:, None] + np.arange(m)[None, :]].copy()
    flip = rng.random(pats.shape) < 0.03
    pats[flip] = (pats[flip] + rng.integers(1, 4, int(flip.sum()))) % 4
    quals = rng.integers(2, 42, (n, m)).astype(np.uint8)
    P = G.PackedSet.pack(list(pats), 4, True)
    T = G.PackedSet.pack(list(texts), 2, False)
    keep = [t(P.words), t(P.offsets), t(T.words), t(T.offsets), torch.from_numpy(quals.reshape(-1)).to(dev)]
    pat = dict(words=keep[0].data_ptr(), offsets=keep[1].data_ptr(), bits=4, big_endian=True)
    txt = dict(words=keep[2].data_ptr(), offsets=keep[3].data_ptr(), bits=2, big_endian=False)
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)
    out = {k: (i32(n), i32(2 * n)) for k in ("qual_default", "qual_const", "plain")}
    stride = 2 * m + 32
    mk_tb = lambda: dict(score=i32(n), source=i32(2 * n), sink=i32(2 * n), n_ops=i32(n),
                         ops=torch.zeros(n * stride, dtype=torch.uint8, device=dev))
    tb_q, tb_p = mk_tb(), mk_tb()
    ptrs = lambda d: {k: v.data_ptr() for k, v in d.items()}
    eng = G.Engine(0)
    ts = torch.cuda.Stream()      # a real stream: the null stream's handle 0 would mean the engine's own
    s = ts.cuda_stream
    al = G.NvAligner(G.NV_GOTOH, G.NV_SEMI_GLOBAL, 0, -6, -8, -3)
    q_def = G.NvQuals(None, [0] * 256, [-v for v in qual_cost(2, 6)], quals_ptr=keep[4].data_ptr())
    q_const = G.NvQuals(None, [0] * 256, [-6] * 256, quals_ptr=keep[4].data_ptr())
    for band in (7, 15, 31):
        for family in ("packed", "int32"):
            if family == "int32":
                os.environ["GASALX_NVB16"] = "0"
            else:
                os.environ.pop("GASALX_NVB16", None)
            score = lambda key, q: lambda: eng.nv_banded_qual_score_device_ptrs(
                al, q, band, n, pat, txt, out[key][0].data_ptr(), out[key][1].data_ptr(), m, s)
            calls = {
                "qual_default": score("qual_default", q_def),
                "qual_const": score("qual_const", q_const),
                "plain": lambda: eng.nv_banded_score_sinks_device_ptrs(al, band, n, pat, txt, out["plain"][0].data_ptr(),
                                                                       out["plain"][1].data_ptr(), m, s),
            }
            r = timed(calls, ts, 3, reps)
            same = bool(torch.equal(out["qual_const"][0], out["plain"][0]) and torch.equal(out["qual_const"][1], out["plain"][1]))
            line = {"probe": "nv_qual", "band": band, "family": family, "pairs": n, "pattern": m, "text": tl, "repeats": reps,
                    "qual_kernel": G.nv_describe_banded_qual_plan(al, q_def, band, m),
                    "plain_kernel": G.nv_describe_banded_sinks_plan(al, band, m), "const_equals_plain": same}
            for k, (med, lo, hi) in r.items():
                line[k + "_ms"] = round(med, 4)
                line[k + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
            line["qual_default_over_plain"] = round(r["qual_default"][0] / r["plain"][0], 3)
            line["qual_const_over_plain"] = round(r["qual_const"][0] / r["plain"][0], 3)
            print(json.dumps(line), flush=True)
        os.environ.pop("GASALX_NVB16", None)
        calls = {
            "qual_traceback": lambda: eng.nv_banded_qual_traceback_device_ptrs(al, q_const, band, n, pat, txt, ptrs(tb_q),
                                                                               stride, m, s),
            "plain_traceback": lambda: eng.nv_banded_traceback_device_ptrs(al, band, n, pat, txt, ptrs(tb_p), stride, m, s),
        }
        r = timed(calls, ts, 2, max(reps // 2, 5))
        same = all(torch.equal(tb_q[k], tb_p[k]) for k in ("score", "source", "sink", "n_ops"))
        qd = timed({"qual_traceback_default": lambda: eng.nv_banded_qual_traceback_device_ptrs(
            al, q_def, band, n, pat, txt, ptrs(tb_q), stride, m, s)}, ts, 2, max(reps // 2, 5))
        r.update(qd)
        line = {"probe": "nv_qual_traceback", "band": band, "pairs": n, "pattern": m, "text": tl,
                "qual_kernel": G.nv_describe_banded_qual_plan(al, q_def, band, m, traceback=True), "const_equals_plain": same}
        for k, (med, lo, hi) in r.items():
            line[k + "_ms"] = round(med, 4)
            line[k + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
        line["qual_over_plain"] = round(r["qual_traceback"][0] / r["plain_traceback"][0], 3)
        print(json.dumps(line), flush=True)
    eng.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Throughput of the banded scorer with BestSink positions (gasalx_nv_banded_score_sinks_device,
csrc/nvbanded_sink.hpp) beside (a) the score-only banded scorer (gasalx_nv_banded_score_device) and
(c) the banded traceback (gasalx_nv_banded_traceback_device), the only route to the sink before it,
on the same data in the same process: reads of 150 symbols against genome windows of 181 (4-bit
big-endian reads, 2-bit little-endian windows), Gotoh, SEMI_GLOBAL and LOCAL, bands 15 and 31,
inputs and outputs resident in HBM.  The three calls alternate inside every repeat, each launch
timed on its own with HIP events after warm-up launches; the median and the spread (min, max) of
the repeats are reported.  Score and sink of (b) and (c) are compared once.  Prints one JSON line
per type and band.

usage: nv_banded_sinks_probe.py [pairs] [repeats]"""
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


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    m, tl = 150, 181
    rng = np.random.default_rng(0x5EED0B5D)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    # reads of m drawn at offsets 0..15 of their windows, 3 % substitutions
    texts = rng.integers(0, 4, (n, tl))
    st = rng.integers(0, 16, n)
    pats = texts[np.arange(n)[:, None], st[:, None] + np.arange(m)[None, :]].copy()
    flip = rng.random(pats.shape) < 0.03
    pats[flip] = (pats[flip] + rng.integers(1, 4, int(flip.sum()))) % 4
    P = G.PackedSet.pack(list(pats), 4, True)
    T = G.PackedSet.pack(list(texts), 2, False)
    keep = [t(P.words), t(P.offsets), t(T.words), t(T.offsets)]
    pat = dict(words=keep[0].data_ptr(), offsets=keep[1].data_ptr(), bits=4, big_endian=True)
    txt = dict(words=keep[2].data_ptr(), offsets=keep[3].data_ptr(), bits=2, big_endian=False)
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)
    sc_a, sc_b, sk_b = i32(n), i32(n), i32(2 * n)
    stride = 2 * m + 32
    tb = dict(score=i32(n), source=i32(2 * n), sink=i32(2 * n), n_ops=i32(n),
              ops=torch.zeros(n * stride, dtype=torch.uint8, device=dev))
    outs = {k: v.data_ptr() for k, v in tb.items()}
    eng = G.Engine(0)
    ts = torch.cuda.Stream()      # a real stream: the null stream's handle 0 would mean the engine's own
    s = ts.cuda_stream
    for type_, tn in ((G.NV_SEMI_GLOBAL, "semi"), (G.NV_LOCAL, "local")):
        al = G.NvAligner(G.NV_GOTOH, type_, 2, -1, -2, -1)
        for band in (15, 31):
            calls = {
                "score": lambda: eng.nv_banded_score_device_ptrs(al, band, n, pat, txt, sc_a.data_ptr(), s, m),
                "sinks": lambda: eng.nv_banded_score_sinks_device_ptrs(al, band, n, pat, txt, sc_b.data_ptr(),
                                                                       sk_b.data_ptr(), m, s),
                "traceback": lambda: eng.nv_banded_traceback_device_ptrs(al, band, n, pat, txt, outs, stride, m, s),
            }
            r = timed(calls, ts, 3, reps)
            same = bool(torch.equal(sc_b, tb["score"]) and torch.equal(sk_b, tb["sink"]) and torch.equal(sc_a, sc_b))
            cells = n * m * band                     # band cells
            line = {"probe": "nv_banded_sinks", "type": tn, "band": band, "pairs": n, "pattern": m, "text": tl,
                    "repeats": reps, "sinks_kernel": G.nv_describe_banded_sinks_plan(al, band, m),
                    "sinks_equal_traceback": same}
            for k, (med, lo, hi) in r.items():
                line[k + "_ms"] = round(med, 4)
                line[k + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
                line[k + "_band_gcups"] = round(cells / med / 1e6, 1)
            line["sinks_over_score"] = round(r["sinks"][0] / r["score"][0], 3)
            line["traceback_over_sinks"] = round(r["traceback"][0] / r["sinks"][0], 2)
            print(json.dumps(line), flush=True)
    eng.close()


if __name__ == "__main__":
    main()

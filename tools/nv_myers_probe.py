#!/usr/bin/env python3
"""Throughput of nvbio's banded Myers aligner (gasalx_nv_banded_myers_device, csrc/nvmyers.hpp)
beside the path a caller had before it, gasalx_nv_banded_score_device with the edit-distance
aligner (nvbanded.hpp), on the same data in the same process: qmap's shape, reads of 150 symbols
against genome windows of 181 (4-bit big-endian reads, 2-bit little-endian windows, the
sw-benchmark packing), at band 31 and band 15, inputs and outputs resident in HBM.  Each launch is
timed on its own with HIP events after warm-up launches; the median and the spread (min, max) of
the repeats are reported.  The two paths' outputs are not compared: they are different functions
(DESIGN.md section 6).  Prints one JSON line per band.

usage: nv_myers_probe.py [pairs] [repeats]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomics-gpu_amd"))
import gasal_ffi as G  # noqa: E402


def timed(call, stream, warmup, reps):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    m, tl = 150, 181
    rng = np.random.default_rng(0x5EED0A11)
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
    sc = torch.zeros(n, dtype=torch.int32, device=dev)
    sk = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    eng = G.Engine(0)
    ts = torch.cuda.Stream()      # a real stream: the null stream's handle 0 would mean the engine's own
    s = ts.cuda_stream
    ed = G.NvAligner(G.NV_ED, G.NV_SEMI_GLOBAL)
    for band in (31, 15):
        myers = lambda: eng.nv_banded_myers_device_ptrs(G.NV_SEMI_GLOBAL, 5, band, n, pat, txt, sc.data_ptr(),
                                                        sk.data_ptr(), m, s)
        dp = lambda: eng.nv_banded_score_device_ptrs(ed, band, n, pat, txt, sc.data_ptr(), s, m)
        my_ms, my_lo, my_hi = timed(myers, ts, 3, reps)
        dp_ms, dp_lo, dp_hi = timed(dp, ts, 3, reps)
        cells = n * m * band                     # band cells: what the DP band updates
        print(json.dumps({"probe": "nv_myers", "band": band, "pairs": n, "pattern": m, "text": tl, "repeats": reps,
                          "myers_kernel": G.nv_describe_myers_plan(G.NV_SEMI_GLOBAL, 5, band),
                          "myers_ms": round(my_ms, 4), "myers_ms_min_max": [round(my_lo, 4), round(my_hi, 4)],
                          "dp_ed_ms": round(dp_ms, 4), "dp_ed_ms_min_max": [round(dp_lo, 4), round(dp_hi, 4)],
                          "dp_over_myers": round(dp_ms / my_ms, 2),
                          "myers_band_gcups": round(cells / my_ms / 1e6, 1),
                          "dp_ed_band_gcups": round(cells / dp_ms / 1e6, 1)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()

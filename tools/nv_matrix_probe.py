#!/usr/bin/env python3
"""Throughput of the matrix-scored Gotoh kernels (gasalx_nv_matrix_score_device, csrc/nvmatrix.hpp) at
nvbio's proteinsw shape: n pairs of a 128-symbol pattern against its own 1024-symbol text, 8-bit
little-endian strings over 24 symbols, LOCAL, gaps -5 / -3, inputs and outputs resident in HBM.  The
table is seeded random, symmetric, entries -4..11 (no BLOSUM table is shipped; throughput does not
depend on the values).  The yardstick runs in the same process on the same strings: the int32 Gotoh
LOCAL kernel under SimpleGotohScheme(1, -1, -5, -3) (8-bit texts keep it off the packed kernel),
score only and with sinks.  The four calls alternate inside every repeat, each launch timed on its own
with HIP events after warm-up launches; the median and the spread (min, max) of the repeats are
reported.  Scores of the first pairs are checked against a numpy fill.  Prints one JSON line.

--traceback times the full-DP traceback instead (gasalx_nv_matrix_traceback_device, csrc/nvmatrix_trace.hpp)
against the Gotoh traceback under SimpleGotohScheme(1, -1, -5, -3) (gasalx_nv_traceback_device,
csrc/nvtrace.hpp) on the same strings, GLOBAL, LOCAL and SEMI_GLOBAL: the two alternate inside every
repeat with HIP events around each device call.  128 x 1024 takes 139 KB of workspace per pair, so a
4 GB chunk holds about 30 K pairs: the default is 16,384 pairs, one chunk.  The LOCAL scores are checked
against the matrix scorer's.  Prints one JSON line.

usage: nv_matrix_probe.py [--traceback] [pairs] [repeats]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomics-gpu_amd"))
import gasal_ffi as G  # noqa: E402

N_SYM, M, TL, GO, GE = 24, 128, 1024, -5, -3


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


def local_score(S, p, t):
    """LOCAL Gotoh score, rows vectorised over the text: E needs a scan, done as a running maximum."""
    H = np.zeros(len(t) + 1, np.int64)
    F = np.full(len(t) + 1, -(1 << 40), np.int64)
    best = 0
    k = np.arange(len(t) + 1)
    for pi in p:
        F = np.maximum(F + GE, H + GO)
        d = np.concatenate([[0], np.maximum(np.maximum(H[:-1] + S[pi, t], F[1:]), 0)])   # without E
        # E(c) = max_j<c (h(j) + GO + GE * (c - 1 - j)); h >= d, and a gap opened from a gap never beats extending
        a = np.maximum.accumulate(d - GE * k)
        e = np.concatenate([[-(1 << 40)], a[:-1] + GO + GE * (k[1:] - 1)])
        H = np.maximum(d, e)
        H[0] = 0
        best = max(best, int(H.max()))
    return best


def traceback_leg(args):
    n = int(args[0]) if len(args) > 0 else 16384
    reps = int(args[1]) if len(args) > 1 else 10
    rng = np.random.default_rng(0x5EED1024)
    tri = np.triu(rng.integers(-4, 12, (N_SYM, N_SYM)))
    mat = G.NvMatrix((tri + np.triu(tri, 1).T).astype(np.int8))
    dev = torch.device("cuda:0")
    pats = rng.integers(0, N_SYM, (n, M), dtype=np.uint8)
    texts = rng.integers(0, N_SYM, (n, TL), dtype=np.uint8)
    keep = [torch.from_numpy(pats.reshape(-1)).to(dev), torch.from_numpy(texts.reshape(-1)).to(dev),
            torch.arange(0, (n + 1) * M, M, dtype=torch.int32, device=dev),
            torch.arange(0, (n + 1) * TL, TL, dtype=torch.int32, device=dev)]
    pat = dict(words=keep[0].data_ptr(), offsets=keep[2].data_ptr(), bits=8, big_endian=False)
    txt = dict(words=keep[1].data_ptr(), offsets=keep[3].data_ptr(), bits=8, big_endian=False)
    stride = M + TL
    bufs = {k: dict(score=torch.zeros(n, dtype=torch.int32, device=dev),
                    source=torch.zeros(2 * n, dtype=torch.int32, device=dev),
                    sink=torch.zeros(2 * n, dtype=torch.int32, device=dev),
                    ops=torch.zeros(n * stride, dtype=torch.uint8, device=dev),
                    n_ops=torch.zeros(n, dtype=torch.int32, device=dev)) for k in ("matrix", "simple")}
    ptrs = {k: {f: t.data_ptr() for f, t in v.items()} for k, v in bufs.items()}
    eng = G.Engine(0)
    ts = torch.cuda.Stream()
    s = ts.cuda_stream
    workspace = G.nv_traceback_workspace(M, TL, n)
    line = {"probe": "nv_matrix_traceback", "pairs": n, "pattern": M, "text": TL, "symbols": N_SYM, "repeats": reps,
            "workspace_bytes": workspace, "one_chunk": workspace >= (G.nv_traceback_workspace(M, TL, 1) - 128) * n}
    ok = True
    cells = n * M * TL
    for name, type_ in (("global", G.NV_GLOBAL), ("local", G.NV_LOCAL), ("semi", G.NV_SEMI_GLOBAL)):
        al = G.NvAligner(G.NV_GOTOH, type_, 1, -1, GO, GE)
        calls = {
            "simple": lambda: eng.nv_traceback_device_ptrs(al, n, pat, txt, ptrs["simple"], stride, M, TL, s),
            "matrix": lambda: eng.nv_matrix_traceback_device_ptrs(al, mat, n, pat, txt, ptrs["matrix"], stride, M, TL, s),
        }
        r = timed(calls, ts, 2, reps)
        for k, (med, lo, hi) in r.items():
            line[f"{name}_{k}_ms"] = round(med, 3)
            line[f"{name}_{k}_ms_min_max"] = [round(lo, 3), round(hi, 3)]
            line[f"{name}_{k}_gcups"] = round(cells / med / 1e6, 1)
        line[f"{name}_matrix_over_simple"] = round(r["matrix"][0] / r["simple"][0], 3)
        line[f"{name}_mean_ops"] = {k: round(float(bufs[k]["n_ops"].float().mean()), 1) for k in bufs}
        if type_ == G.NV_LOCAL:
            want = torch.zeros(n, dtype=torch.int32, device=dev)
            eng.nv_matrix_score_device_ptrs(al, mat, n, pat, txt, want.data_ptr(), 0, M, TL, s)
            ts.synchronize()
            ok = ok and bool(torch.equal(want, bufs["matrix"]["score"]))
    line["scores_ok"] = ok
    print(json.dumps(line), flush=True)
    eng.close()
    return 0 if ok else 1


def main():
    if "--traceback" in sys.argv[1:]:
        return traceback_leg([a for a in sys.argv[1:] if a != "--traceback"])
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rng = np.random.default_rng(0x5EED1024)
    tri = np.triu(rng.integers(-4, 12, (N_SYM, N_SYM)))
    table = (tri + np.triu(tri, 1).T).astype(np.int8)
    mat = G.NvMatrix(table)
    dev = torch.device("cuda:0")
    pats = rng.integers(0, N_SYM, (n, M), dtype=np.uint8)
    texts = rng.integers(0, N_SYM, (n, TL), dtype=np.uint8)
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)
    keep = [torch.from_numpy(pats.reshape(-1)).to(dev), torch.from_numpy(texts.reshape(-1)).to(dev),
            torch.arange(0, (n + 1) * M, M, dtype=torch.int32, device=dev),
            torch.arange(0, (n + 1) * TL, TL, dtype=torch.int32, device=dev)]
    pat = dict(words=keep[0].data_ptr(), offsets=keep[2].data_ptr(), bits=8, big_endian=False)
    txt = dict(words=keep[1].data_ptr(), offsets=keep[3].data_ptr(), bits=8, big_endian=False)
    sc = {k: i32(n) for k in ("matrix", "matrix_sinks", "simple", "simple_sinks")}
    sk = {k: i32(2 * n) for k in ("matrix_sinks", "simple_sinks")}
    eng = G.Engine(0)
    ts = torch.cuda.Stream()      # a real stream: the null stream's handle 0 would mean the engine's own
    s = ts.cuda_stream
    al = G.NvAligner(G.NV_GOTOH, G.NV_LOCAL, 1, -1, GO, GE)
    calls = {
        "simple": lambda: eng.nv_score_device_ptrs(al, n, pat, txt, sc["simple"].data_ptr(), 0, M, TL, s),
        "matrix": lambda: eng.nv_matrix_score_device_ptrs(al, mat, n, pat, txt, sc["matrix"].data_ptr(), 0, M, TL, s),
        "simple_sinks": lambda: eng.nv_score_sinks_device_ptrs(al, n, pat, txt, sc["simple_sinks"].data_ptr(),
                                                               sk["simple_sinks"].data_ptr(), M, TL, s),
        "matrix_sinks": lambda: eng.nv_matrix_score_device_ptrs(al, mat, n, pat, txt, sc["matrix_sinks"].data_ptr(),
                                                                sk["matrix_sinks"].data_ptr(), M, TL, s),
    }
    r = timed(calls, ts, 3, reps)
    got = sc["matrix"].cpu().numpy()
    S = table.astype(np.int64)
    checked = min(n, 8)
    ok = all(local_score(S, pats[k], texts[k]) == got[k] for k in range(checked))
    ok = ok and bool(torch.equal(sc["matrix"], sc["matrix_sinks"]) and torch.equal(sc["simple"], sc["simple_sinks"]))
    cells = n * M * TL
    line = {"probe": "nv_matrix", "pairs": n, "pattern": M, "text": TL, "symbols": N_SYM, "repeats": reps,
            "matrix_kernel": G.nv_describe_matrix_plan(al, N_SYM, M, TL, per_pair_texts=True),
            "simple_kernel": G.nv_describe_plan(al, M, TL, per_pair_texts=True, text_bits=8),
            "lds_bytes_per_block": {"matrix": 1024 + 32 * TL, "simple": 32 * TL * 2},
            "scores_checked": checked, "scores_ok": ok}
    for k, (med, lo, hi) in r.items():
        line[k + "_ms"] = round(med, 4)
        line[k + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
        line[k + "_gcups"] = round(cells / med / 1e6, 1)
    line["matrix_over_simple"] = round(r["matrix"][0] / r["simple"][0], 3)
    line["matrix_sinks_over_simple_sinks"] = round(r["matrix_sinks"][0] / r["simple_sinks"][0], 3)
    print(json.dumps(line), flush=True)
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

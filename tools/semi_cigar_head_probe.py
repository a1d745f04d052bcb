#!/usr/bin/env python3
"""Wall time of gasalx_semi_cigar_device and of gasalx_semi_cigar_head_device per HEAD on the same data
in one process: config-4 synthetic pairs, inputs and outputs resident in HBM, the
method of profiles/semi_cigar/README.md -- the whole call between two device synchronisations, 1 s of
warm-up, 7 runs, median (min - max).  A library without the head calls (an older build loaded through
GASALX_LIB) gives the first line only.  Then the score launch alone per HEAD (gasalx_align_device).
Prints one JSON line per call.

usage: semi_cigar_head_probe.py [pairs]"""
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genomics-gpu_amd"))
import gasal_ffi as G  # noqa: E402


def timed(call, warm_s=1.0, reps=7):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        call()
        torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    b = G.Batch.synth(4, n, 0x5EED0004)
    cells = int((b.q_lens.astype(np.int64) * b.t_lens.astype(np.int64)).sum())
    mq, mt = int(b.q_lens.max()), int(b.t_lens.max())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = dict(q_batch=dev(b.q_data), q_offsets=dev(b.q_offsets.view(np.int32)), q_lens=dev(b.q_lens.view(np.int32)),
             t_batch=dev(b.t_data), t_offsets=dev(b.t_offsets.view(np.int32)), t_lens=dev(b.t_lens.view(np.int32)))
    o = {k: torch.zeros(n, dtype=torch.int32, device="cuda")
         for k in ("aln_score", "q_end", "t_end", "q_start", "t_start", "n_cigar_ops")}
    o["cigar"] = torch.zeros(b.q_bytes, dtype=torch.uint8, device="cuda")
    ptrs = {k: v.data_ptr() for k, v in {**d, **o}.items()}
    eng = G.Engine(0)
    sha = hashlib.sha256(open(G.LIB_PATH, "rb").read()).hexdigest()[:16]
    heads = hasattr(G.lib(), "gasalx_semi_cigar_head_device")
    calls = [("gasalx_semi_cigar_device", G.TARGET, eng.semi_cigar_device_ptrs)]
    if heads:
        calls += [(f"gasalx_semi_cigar_head_device HEAD={name}", h, eng.semi_cigar_head_device_ptrs)
                  for name, h in (("TARGET", G.TARGET), ("NONE", G.NONE), ("QUERY", G.QUERY), ("BOTH", G.BOTH))]
    for what, head, fn in calls:
        p = G.make_params(algo=G.SEMI_GLOBAL, head=head, tail=G.TARGET)
        med, lo, hi = timed(lambda: fn(p, ptrs, b.q_bytes, b.t_bytes, n, mq, mt))
        print(json.dumps({"call": what, "pairs": n, "ms_median": round(med, 3), "ms_min": round(lo, 3),
                          "ms_max": round(hi, 3), "gcups": round(cells / med / 1e6, 1), "packed_pairs": eng.packed_pairs(),
                          "q_start_gt0": int((o["q_start"] > 0).sum()), "lib_sha256": sha}), flush=True)
    # the score launch alone (gasalx_align_device, WITHOUT_START) per HEAD: what of a head's time is not
    # the flag launch and the walk
    sp = {k: v for k, v in ptrs.items() if k in d or k in ("aln_score", "q_end", "t_end")}
    for name, h in (("TARGET", G.TARGET), ("NONE", G.NONE), ("QUERY", G.QUERY), ("BOTH", G.BOTH)):
        p = G.make_params(algo=G.SEMI_GLOBAL, head=h, tail=G.TARGET)
        med, lo, hi = timed(lambda: eng.align_device_ptrs(p, sp, b.q_bytes, b.t_bytes, n, mq, mt))
        print(json.dumps({"call": f"gasalx_align_device score only HEAD={name}", "pairs": n, "ms_median": round(med, 3),
                          "ms_min": round(lo, 3), "ms_max": round(hi, 3), "lib_sha256": sha}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()

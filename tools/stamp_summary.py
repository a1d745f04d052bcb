#!/usr/bin/env python3
"""Phase shares of the packed LOCAL kernel's waves from a stamp probe run.

Input: the file a probe build of the library (make variants VARIANTS=stamp:-DGX_WF16_STAMP,
loaded through GASALX_LIB) writes when GASALX_STAMP_OUT is set: per wave six 64-bit words, the
wall clock (100 MHz) at entry, after the block's vote, after the sweep and at exit, then
HW_ID | XCC_ID << 32, then the clock on reaching the vote.  Prints one JSON line: the median
share of a wave's life in the prologue (entry to vote), the sweep and the epilogue, the median
times in microseconds with the prologue split at the vote (entry to reaching it, waiting at it),
and, per SIMD (XCC, SE, SH, CU, SIMD), the share of its busy time (first entry to last exit) with
exactly 0, 1, 2 and 3 or more waves inside their sweep: over the launch (all SIMDs' time
together) and the median and the 10th / 90th percentile of the SIMDs' own shares.
Usage: stamp_summary.py FILE
"""
import json
import sys

import numpy as np

WORDS = 6


def sweeper_time(t1, t2, lo, hi):
    """Time in [lo, hi] with 0, 1, 2, >= 3 of the intervals [t1, t2) open."""
    ev = np.concatenate([np.stack([t1, np.ones(len(t1), np.int64)], 1),
                         np.stack([t2, -np.ones(len(t2), np.int64)], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    depth = np.minimum(np.cumsum(ev[:, 1])[:-1], 3)
    dt = np.diff(ev[:, 0])
    by = np.array([dt[depth == k].sum() for k in range(4)], np.float64)
    by[0] += (ev[0, 0] - lo) + (hi - ev[-1, 0])                  # before the first sweep, after the last
    return by


def main(path):
    a = np.fromfile(path, dtype=np.uint64).reshape(-1, WORDS)
    a = a[(a[:, 0] != 0) & (a[:, 3] != 0)]                       # waves that stamped entry and exit
    t = a[:, [0, 1, 2, 3, 5]].astype(np.int64)
    life = (t[:, 3] - t[:, 0]).astype(np.float64)
    ok = life > 0
    t, life, hw = t[ok], life[ok], a[ok, 4]
    pro, swp, epi = (t[:, 1] - t[:, 0]) / life, (t[:, 2] - t[:, 1]) / life, (t[:, 3] - t[:, 2]) / life
    simd = ((hw >> np.uint64(32)) << np.uint64(16)) | (hw & np.uint64(0xFF30))   # XCC, SE/SH/CU, SIMD
    total = np.zeros(4)
    shares = []
    for s in np.unique(simd):
        m = simd == s
        by = sweeper_time(t[m, 1], t[m, 2], t[m, 0].min(), t[m, 3].max())
        total += by
        shares.append(by / by.sum())
    shares = np.array(shares)
    names = ("0", "1", "2", "3+")
    us = lambda x: float(np.median(x)) / 100
    print(json.dumps({
        "waves": int(len(life)), "simds": int(len(shares)),
        "median_share": {"prologue": float(np.median(pro)), "sweep": float(np.median(swp)),
                         "epilogue": float(np.median(epi))},
        "median_us": {"prologue": us(t[:, 1] - t[:, 0]), "to_vote": us(t[:, 4] - t[:, 0]),
                      "at_vote": us(t[:, 1] - t[:, 4]), "sweep": us(t[:, 2] - t[:, 1]),
                      "epilogue": us(t[:, 3] - t[:, 2]), "life": us(life)},
        "sweepers_share_of_busy_time": {
            "launch": {n: float(total[k] / total.sum()) for k, n in enumerate(names)},
            "simd_median": {n: float(np.median(shares[:, k])) for k, n in enumerate(names)},
            "simd_p10": {n: float(np.percentile(shares[:, k], 10)) for k, n in enumerate(names)},
            "simd_p90": {n: float(np.percentile(shares[:, k], 90)) for k, n in enumerate(names)}},
        "simd_time_under_3_sweeping": float(total[:3].sum() / total.sum()),
        "simd_time_at_most_1_sweeping": float(total[:2].sum() / total.sum())}))


if __name__ == "__main__":
    main(sys.argv[1])

#!/usr/bin/env python3
"""Phase shares of the packed LOCAL kernel's waves from a stamp probe run.

Input: the file a probe build of the library (make variants VARIANTS=stamp:-DGX_WF16_STAMP,
loaded through GASALX_LIB) writes when GASALX_STAMP_OUT is set: per wave five 64-bit words, the
wall clock (100 MHz) at entry, after the block's vote, after the sweep and at exit, then
HW_ID | XCC_ID << 32.  Prints one JSON line: the median share of a wave's life in the prologue
(entry to vote), the sweep and the epilogue, the median times in microseconds, and, per SIMD
(XCC, SE, SH, CU, SIMD), the share of its busy time with fewer than 3 waves inside their sweep.
Usage: stamp_summary.py FILE
"""
import json
import sys

import numpy as np


def main(path):
    a = np.fromfile(path, dtype=np.uint64).reshape(-1, 5)
    a = a[(a[:, 0] != 0) & (a[:, 3] != 0)]                       # waves that stamped entry and exit
    t = a[:, :4].astype(np.int64)
    life = (t[:, 3] - t[:, 0]).astype(np.float64)
    ok = life > 0
    t, life, hw = t[ok], life[ok], a[ok, 4]
    pro, swp, epi = (t[:, 1] - t[:, 0]) / life, (t[:, 2] - t[:, 1]) / life, (t[:, 3] - t[:, 2]) / life
    simd = ((hw >> np.uint64(32)) << np.uint64(16)) | (hw & np.uint64(0xFF30))   # XCC, SE/SH/CU, SIMD
    under = busy = 0
    for s in np.unique(simd):
        m = simd == s
        ev = np.concatenate([np.stack([t[m, 1], np.ones(m.sum(), np.int64)], 1),
                             np.stack([t[m, 2], -np.ones(m.sum(), np.int64)], 1)])
        ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
        depth = np.cumsum(ev[:, 1])[:-1]
        dt = np.diff(ev[:, 0])
        lo, hi = t[m, 0].min(), t[m, 3].max()
        busy += hi - lo
        under += (hi - lo) - dt[depth >= 3].sum()
    print(json.dumps({
        "waves": int(len(life)), "simds": int(len(np.unique(simd))),
        "median_share": {"prologue": float(np.median(pro)), "sweep": float(np.median(swp)),
                         "epilogue": float(np.median(epi))},
        "median_us": {"prologue": float(np.median(t[:, 1] - t[:, 0])) / 100, "sweep": float(np.median(t[:, 2] - t[:, 1])) / 100,
                      "epilogue": float(np.median(t[:, 3] - t[:, 2])) / 100, "life": float(np.median(life)) / 100},
        "simd_time_under_3_sweeping": float(under) / float(busy) if busy else None}))


if __name__ == "__main__":
    main(sys.argv[1])

#!/usr/bin/env python3
"""PairHMM float64 / log10 probe: a client of the C-ABI on the config-5 synthetic batch
(bench.py's synth_pairhmm generator, resident in device memory) that leaves bench.py as it is.

Legs, each the median of --steps timed steps (device events on a non-default stream) after
--warmup untimed ones:
  fp32    gasalx_pairhmm_device
  log10   gasalx_pairhmm_log10_device (fp32 pass + selection + float64 rescue), with the
          number of pairs it rescued
  f64     gasalx_pairhmm64_device over every pair

  tools/pairhmm64_probe.py [--pairs N] [--steps K] [--warmup W] [--legs fp32,log10,f64]
                           [--parent-lib PATH] [--rounds R]

--parent-lib PATH: the fp32 leg of another build of the library (the parent commit's) against
this build's, alternating, R rounds each, every run in a fresh child process (the library is
chosen at load time through GASALX_LIB).  Prints one JSON line per leg."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sha256_of(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return h.hexdigest()[:16]


def run_legs(args):
    import torch
    import bench
    G = bench.G
    n = args.pairs
    rl, hl = 250, 500              # config 5 (bench.py's workload table)
    h = bench.synth_pairhmm(0, n, bench.SEEDS[5], rl, hl)
    dev = "cuda:0"
    i32 = lambda a: np.ascontiguousarray(a, np.uint32).view(np.int32)
    u = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = {"reads": u(h["reads"]), "haps": u(h["haps"]), "read_offsets": u(i32(h["read_offsets"])),
         "read_lens": u(i32(h["read_lens"])), "hap_offsets": u(i32(h["hap_offsets"])),
         "hap_lens": u(i32(h["hap_lens"])), "qm": u(h["qm"]), "delta": u(h["delta"]), "xiksi": u(h["xiksi"]),
         "alpha": u(h["alpha"])}
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    r32 = torch.zeros(n, dtype=torch.float32, device=dev)
    r64 = torch.zeros(n, dtype=torch.float64, device=dev)
    used = torch.zeros(n, dtype=torch.uint8, device=dev)
    eng = G.Engine(0)
    stream = torch.cuda.Stream()
    rb, hb = len(h["reads"]), len(h["haps"])
    calls = {
        "fp32": lambda: eng.pairhmm_device_ptrs(ptrs, rb, hb, n, rl, hl, r32.data_ptr(), stream.cuda_stream),
        "log10": lambda: eng.pairhmm_log10_device_ptrs(ptrs, rb, hb, n, rl, hl, r64.data_ptr(), used.data_ptr(),
                                                       stream=stream.cuda_stream),
        "f64": lambda: eng.pairhmm64_device_ptrs(ptrs, rb, hb, n, rl, hl, r64.data_ptr(), stream.cuda_stream),
    }
    cells = n * rl * hl
    torch.cuda.synchronize()
    for leg in args.legs.split(","):
        call = calls[leg]
        with torch.cuda.stream(stream):
            for _ in range(args.warmup):
                call()
            stream.synchronize()
            ms = []
            for _ in range(args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        out = {"leg": leg, "label": args.label, "lib_sha256": sha256_of(G.LIB_PATH), "pairs": n, "read": rl, "hap": hl,
               "steps": args.steps, "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
               "ms_max": round(max(ms), 4), "gcups": round(cells / med / 1e6, 1)}
        if leg == "log10":
            out["rescued"] = int(used.sum().item())
            out["all_finite"] = bool(torch.isfinite(r64).all().item())
        if leg == "f64":
            v = r64.cpu().numpy()
            out["all_finite_positive"] = bool(np.all(np.isfinite(v) & (v > 0)))
        print(json.dumps(out), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="fp32,log10,f64")
    ap.add_argument("--label", default="this")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    if args.steps < 1 or any(l not in ("fp32", "log10", "f64") for l in args.legs.split(",")):
        ap.error("bad --steps or --legs")
    if args.parent_lib:
        # a fresh process per run: GASALX_LIB picks the library when gasal_ffi is imported
        base = [sys.executable, os.path.abspath(__file__), "--pairs", str(args.pairs), "--steps", str(args.steps),
                "--warmup", str(args.warmup), "--legs", "fp32"]
        for _ in range(args.rounds):
            for label, lib in (("parent", os.path.abspath(args.parent_lib)), ("this", None)):
                env = dict(os.environ)
                env.pop("GASALX_LIB", None)
                if lib:
                    env["GASALX_LIB"] = lib
                subprocess.run(base + ["--label", label], env=env, check=True, timeout=300)
        return
    run_legs(args)


if __name__ == "__main__":
    main()

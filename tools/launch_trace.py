#!/usr/bin/env python3
"""The library's launch sequence, path by path, for comparing two builds of it.

  launch_trace.py run            one small call per dispatcher path, per host form of the flat API and
                                 per branch of the nvbio launcher on device 0 (GASALX_LIB picks the
                                 library); meant to run under `rocprofv3 --kernel-trace --output-format csv`
  launch_trace.py list DIR OUT   the kernel-trace CSV(s) under DIR as an ordered list, one line per
                                 launch of the library's kernels: name, grid, block, LDS bytes

Two builds launch the same sequence when their lists are equal line for line
(profiles/dispatch_refactor/README.md, profiles/capi_refactor/README.md,
profiles/nv_launcher_refactor/README.md, profiles/planner_refactor/README.md,
profiles/nv_capi_refactor/README.md).
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "genomics-gpu_amd"), os.path.join(ROOT, "tests")]


def run():
    import numpy as np
    import torch
    import gasal_ffi as G
    import helpers

    eng = G.Engine(0)
    dev = torch.device("cuda", 0)

    def rand_batch(seed, n, qmin, qmax, tmin, tmax):
        rng = np.random.default_rng(seed)
        return G.Batch.from_pairs(*helpers.random_pairs(rng, n, qmin, qmax, tmin, tmax))

    def device_call(b, fields, **kw):
        """one gasalx_align_device call over the whole batch (the host pipeline would split it)"""
        u = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else a).to(dev)
        d = {"q_batch": u(b.q_data), "t_batch": u(b.t_data), "q_offsets": u(b.q_offsets), "t_offsets": u(b.t_offsets),
             "q_lens": u(b.q_lens), "t_lens": u(b.t_lens)}
        for f in fields:
            d[f] = torch.zeros(b.q_bytes, dtype=torch.uint8, device=dev) if f == "cigar" else \
                torch.zeros(b.n, dtype=torch.int32, device=dev)
        eng.align_device_ptrs(G.make_params(**kw), {k: v.data_ptr() for k, v in d.items()}, b.q_bytes, b.t_bytes,
                              b.n, int(b.q_lens.max()), int(b.t_lens.max()))
        torch.cuda.synchronize()

    ends = ("aln_score", "q_end", "t_end")
    device_call(G.Batch.synth(2, 120_000, 0x7A13), ends, algo=G.LOCAL)            # the tail shape is taken
    device_call(G.Batch.synth(2, 2_000, 0x7A14), ends, algo=G.LOCAL)
    small = G.Batch.synth(2, 2_000, 0x7A15)
    eng.align_host(small, G.make_params(algo=G.LOCAL, start_pos=G.WITH_START))
    eng.align_host(small, G.make_params(algo=G.LOCAL, start_pos=G.WITH_TB))
    os.environ["GASALX_TB_FBCAP"] = "4096"                                        # several fallback chunks
    device_call(G.Batch.synth(3, 60_000, 0x7A31), ("aln_score", "cigar", "n_cigar_ops"), algo=G.GLOBAL,
                start_pos=G.WITH_TB)
    del os.environ["GASALX_TB_FBCAP"]
    semi = rand_batch(0x51, 5_000, 100, 150, 150, 182)
    eng.align_host(semi, G.make_params(algo=G.SEMI_GLOBAL, start_pos=G.WITH_START, tail=G.TARGET))
    two = G.Batch.from_pairs(["ACGT" * 30] * 600, ["ACGT" * 40] * 300 + ["ACGT" * 20] * 300)   # two target classes
    eng.align_host(two, G.make_params(algo=G.SEMI_GLOBAL, tail=G.BOTH))
    uneven = rand_batch(0x52, 5_000, 60, 150, 60, 182)
    eng.align_host(uneven, G.make_params(algo=G.LOCAL, second_best=1))
    eng.align_host(uneven, G.make_params(algo=G.BANDED, k_band=16))
    for qlen in (60, 200):                                                        # KSW: registers, then the global array
        k = rand_batch(0x53 + qlen, 2_000, qlen - 20, qlen, qlen, qlen + 40)
        eng.align_host(k, G.make_params(algo=G.KSW), seed_scores=np.full(k.n, 20, np.uint32))
    pairs = helpers.hmm_unrelated(0x54, (40, 100, 150))
    eng.pairhmm_quals_host(G.HmmData.from_pairs(pairs))

    # the flat API's other host forms (profiles/capi_refactor/README.md)
    hmm = G.HmmData.from_pairs(pairs)
    eng.pairhmm_host(*helpers.hmm_args(pairs, G.pairhmm_params))
    eng.pairhmm64_quals_host(hmm)
    eng.pairhmm_quals_log10_host(hmm)
    rng = np.random.default_rng(0x55)
    plen = rng.integers(20, 101, 200)
    pats = [rng.integers(0, 4, int(k)) for k in plen]
    txts = [rng.integers(0, 4, int(k) + 20) for k in plen]
    P = G.PackedSet.pack(pats)
    T = G.PackedSet.pack(txts, bits=2, big_endian=False)
    al = G.NvAligner(G.NV_GOTOH, G.NV_SEMI_GLOBAL, 2, -1, -2, -1)
    eng.nv_score_host(al, P, T)
    eng.nv_banded_score_host(al, 16, P, T)
    max_p = int(plen.max())
    for per, call in ((G.nv_traceback_workspace(max_p, max_p + 20, 1), lambda: eng.nv_traceback_host(al, P, T)),
                      (G.nv_banded_traceback_workspace(max_p, 16, 1), lambda: eng.nv_banded_traceback_host(al, 16, P, T))):
        os.environ["GASALX_NV_TB_BUDGET"] = str(70 * per)                         # 200 pairs: chunks of 70, 70, 60
        call()
        del os.environ["GASALX_NV_TB_BUDGET"]
    eng.align_host(rand_batch(0x56, 40_000, 20, 40, 20, 40), G.make_params(algo=G.LOCAL))   # the two-stream pipeline

    # every branch of the nvbio launcher (profiles/nv_launcher_refactor/README.md); the packed score
    # and banded kernels, band 16, ran above
    T4 = G.PackedSet.pack(txts)                                                   # 4-bit texts: the int32 kernels
    eng.nv_score_host(al, P, G.PackedSet.pack([max(txts, key=len)], bits=2, big_endian=False, shared=True))
    eng.nv_score_host(al, P, T4)
    eng.nv_score_host(G.NvAligner(G.NV_GOTOH, G.NV_LOCAL, 2, 1, -2, -1), P, T)    # a positive mismatch: MASK
    eng.nv_score_sinks_host(al, P, T)
    eng.nv_score_sinks_host(al, P, T4)
    for band in (16, 12):                                                         # an EX instance and a plain one
        eng.nv_banded_score_host(al, band, P, T4)
    eng.nv_banded_score_host(al, 12, P, T)
    for band in (15, 16):
        eng.nv_banded_traceback_host(al, band, P, T)
    P199, T199 = G.PackedSet.pack(pats[:199]), G.PackedSet.pack(txts[:199], bits=2, big_endian=False)
    eng.nv_score_host(al, P199, T199)                                             # an odd n: the packed grids round up
    eng.nv_banded_score_host(al, 16, P199, T199)

    # the nv host forms no call above makes (profiles/nv_capi_refactor/README.md)
    mat = G.NvMatrix(np.where(np.eye(4, dtype=bool), 2, -1))
    eng.nv_matrix_score_host(al, mat, P, T)
    eng.nv_banded_score_sinks_host(al, 16, P, T)
    eng.nv_banded_myers_host(G.NV_SEMI_GLOBAL, 4, 16, P, T)
    os.environ["GASALX_NV_TB_BUDGET"] = str(70 * G.nv_traceback_workspace(max_p, max_p + 20, 1))   # three chunks
    eng.nv_matrix_traceback_host(al, mat, P, T)
    del os.environ["GASALX_NV_TB_BUDGET"]

    # planner branches the calls above miss (profiles/planner_refactor/README.md)
    device_call(G.Batch.synth(3, 60_000, 0x7A32), ("aln_score",), algo=G.GLOBAL)  # GLOBAL score: its tail shape
    eng.semi_cigar_host(rand_batch(0x57, 2_000, 100, 150, 150, 182),
                        G.make_params(algo=G.SEMI_GLOBAL, head=G.TARGET, tail=G.TARGET))
    os.environ["GASALX_GMIN"] = "32"                                              # a forced minimum G
    device_call(G.Batch.synth(2, 2_000, 0x7A16), ends, algo=G.LOCAL)
    del os.environ["GASALX_GMIN"]
    eng.close()


def listing(d, out):
    rows = []
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)):
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    lds = "LDS_Block_Size" if rows and "LDS_Block_Size" in rows[0] else "Group_Segment_Size"
    with open(out, "w") as f:
        for r in rows:
            name = r["Kernel_Name"]
            if "at::" in name:          # torch's fills and copies
                continue
            f.write("%s grid=%s,%s,%s block=%s,%s,%s lds=%s\n" % (
                name, r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"],
                r["Workgroup_Size_Y"], r["Workgroup_Size_Z"], r[lds]))
    print(len(rows), "dispatches ->", out)


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else listing(sys.argv[2], sys.argv[3])

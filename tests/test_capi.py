"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports
every symbol declared in include/gasalx.h, the reference-compatible C++ API
symbols are present, and host-side logic (batch layout, CIGAR decoding,
synthetic workloads) behaves like the reference.  No compute calls."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import gasal_ffi as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_c_functions():
    src = open(os.path.join(ROOT, "include", "gasalx.h")).read()
    return sorted(set(re.findall(r"^\s*(?:int|const char \*)\s*(gasalx_\w+)\s*\(", src, re.M)))


def test_lib_loads_and_exports_every_declared_symbol():
    lib = G.lib()
    declared = _declared_c_functions()
    assert len(declared) >= 12
    for name in declared:
        assert hasattr(lib, name), name
    assert set(declared) == set(G.EXPORTS)


def test_cpp_api_symbols_present():
    out = subprocess.run(["nm", "-DC", G.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("gasal_init_gpu_storage_v(int)", "gasal_init_streams(", "gasal_destroy_streams(",
                "gasal_destroy_gpu_storage_v(", "gasal_host_batch_fill(", "gasal_host_batch_add(",
                "gasal_host_batch_addbase(", "gasal_host_batch_new(", "gasal_host_batch_destroy(",
                "gasal_host_batch_reset(", "gasal_host_batch_getlast(", "gasal_host_batch_print(",
                "gasal_host_batch_printall(", "gasal_host_alns_resize(", "gasal_op_fill(", "gasal_set_device(",
                "gasal_copy_subst_scores(", "gasal_aln_async(", "gasal_is_aln_async_done(",
                "gasal_res_new_host(", "gasal_res_new_device(", "gasal_res_new_device_cpy(",
                "gasal_res_destroy_host(", "gasal_res_destroy_device(", "Parameters::Parameters(int, char**)",
                "Parameters::parse()", "gasal_gpu_mem_alloc(", "gasal_gpu_mem_free("):
        assert sym in out, sym


def test_abi_version():
    assert G.lib().gasalx_abi_version() == 1


def test_batch_layout_matches_host_batch_fill():
    # host_batch.cpp:100-102,137-150: pad with N_CODE to a multiple of 8
    b = G.Batch.from_pairs(["ACGTA", "ACGTACGT", "A"], ["GG", "T" * 9, "C" * 16])
    assert list(b.q_offsets) == [0, 8, 16] and list(b.q_lens) == [5, 8, 1]
    assert bytes(b.q_data[:8]) == b"ACGTANNN"
    assert list(b.t_offsets) == [0, 8, 24] and b.t_bytes == 40


def test_decode_cigar_merges_split_runs():
    # reversed bytes: count<<2|op; 63-runs of one op are merged when printed
    rev = np.array([(1 << 2) | 0, (63 << 2) | 0, (2 << 2) | 3, (5 << 2) | 0], np.uint8)
    assert G.decode_cigar(rev, 0, 4) == "5M2I64M"


def test_plan_selection_cpu_only():
    assert G.describe_plan(G.make_params(algo=G.LOCAL), 150, 150) == "wavefront16_local_G8R19"
    assert G.describe_plan(G.make_params(algo=G.LOCAL, match=2), 150, 150) == "wavefront16_local_u16_G8R19"
    # past the u16 range: f16 keys by 64-step segments (WF16_LOCAL_SEG); GASALX_KSEG=0: the int32 kernel
    assert G.describe_plan(G.make_params(algo=G.LOCAL, match=3), 150, 150) == "wavefront16_local_seg64_G8R19"
    assert G.describe_plan(G.make_params(algo=G.LOCAL), 300, 300) == "wavefront16_local_seg64_G16R20"
    assert G.describe_plan(G.make_params(algo=G.LOCAL, start_pos=G.WITH_TB), 150, 150) == "wavefront16_local_tb_dr_G8R20"
    assert G.describe_plan(G.make_params(algo=G.LOCAL, start_pos=G.WITH_TB, match=2), 150, 150) == \
        "wavefront_local_tb_keys_G8R20"
    assert G.describe_plan(G.make_params(algo=G.LOCAL, start_pos=G.WITH_START), 150, 150) == \
        "wavefront16_local_start_G8R19"
    assert G.describe_plan(G.make_params(algo=G.SEMI_GLOBAL, start_pos=G.WITH_START), 150, 182) == \
        "wavefront16_semi_start_G8R23"
    assert G.describe_plan(G.make_params(algo=G.SEMI_GLOBAL, start_pos=G.WITH_START, tail=G.QUERY), 150, 182) == \
        "generic_semi"
    assert G.describe_plan(G.make_params(algo=G.LOCAL, second_best=1), 150, 150) == "local16_second"
    assert G.describe_plan(G.make_params(algo=G.LOCAL, second_best=1, start_pos=G.WITH_START), 150, 150) == \
        "generic_local"
    assert G.describe_plan(G.make_params(algo=G.KSW), 150, 150) == "generic_ksw"
    assert G.describe_plan(G.make_params(algo=G.GLOBAL, start_pos=G.WITH_TB), 300, 300) == \
        "wavefront16_global_tbband_G16R20"
    assert G.describe_plan(G.make_params(algo=G.UNKNOWN), 10, 10) == "none"


# ---- the planner over a fixed grid (tests/golden/plan_names.json, written by tools/plan_grid.py
#      from the build of the commit it names) ----
PLAN_LENS = (8, 64, 150, 152, 182, 256, 257, 300, 512, 513, 1000, 4000)
# (match, mismatch, gap_open, gap_extend, n_penalty): match 1, 2, 3; a zero and a negative mismatch;
# an N penalty below and above the mismatch
PLAN_SCORES = ((1, 4, 6, 1, None), (2, 4, 6, 1, None), (3, 4, 6, 1, None), (1, 0, 6, 1, None), (2, -1, 4, 2, None),
               (1, 4, 6, 1, 2), (1, 4, 6, 1, 6))
PLAN_ENVS = (None, "GASALX_KF16=0", "GASALX_KSEG=0", "GASALX_KSEG=2", "GASALX_TB_BAND=0", "GASALX_PACKED16=0",
             "GASALX_BAND16=0", "GASALX_LOCAL16=0")
PLAN_SWITCHES = sorted({e.split("=")[0] for e in PLAN_ENVS if e} | {"GASALX_GMIN"})


def plan_length_pairs():
    """Every length with itself, with each neighbour in the list and with the read length 150, in
    both orientations."""
    out = []
    for i, a in enumerate(PLAN_LENS):
        for b in {a, PLAN_LENS[max(i - 1, 0)], PLAN_LENS[min(i + 1, len(PLAN_LENS) - 1)], 150}:
            out += [(a, b), (b, a)]
    return sorted(set(out))


def plan_param_sets():
    """Every algo x start_pos x second_best x score set, and every tail and head for SEMI (k_band 16
    for BANDED): one list per set, of its heads."""
    for algo in range(7):
        semi = algo == G.SEMI_GLOBAL
        for start in (0, 1, 2):
            for second in (0, 1):
                for tail in (range(4) if semi else (G.TARGET,)):
                    for m, x, o, e, npen in PLAN_SCORES:
                        yield [G.make_params(algo=algo, start_pos=start, second_best=second, head=head, tail=tail,
                                             match=m, mismatch=x, gap_open=o, gap_extend=e, n_penalty=npen,
                                             k_band=16 if algo == G.BANDED else 0)
                               for head in (range(4) if semi else (G.TARGET,))]


def plan_grid_names(setenv, delenv):
    """The plan name of every grid row, in the fixture's order: switch, parameter set, length pair, head."""
    lib, buf = G.lib(), ctypes.create_string_buffer(128)
    pairs = plan_length_pairs()
    params = list(plan_param_sets())
    names = []
    for env in PLAN_ENVS:
        for s in PLAN_SWITCHES:
            delenv(s)
        if env:
            setenv(*env.split("="))
        for heads in params:
            refs = [ctypes.byref(p) for p in heads]
            for q, t in pairs:
                for ref in refs:
                    assert lib.gasalx_describe_plan(ref, q, t, buf, 128) == 0
                    names.append(buf.value)
    return [n.decode() for n in names]


def test_plan_names_match_golden_grid(monkeypatch):
    """make_plan names the same kernel for every row of the grid as the build that wrote the fixture
    (rows run-length encoded: name index, count, name index, count, ... over plan_grid_names' order)."""
    import json
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_names.json")))
    assert gold["lens"] == list(PLAN_LENS) and gold["envs"] == list(PLAN_ENVS)
    assert gold["scores"] == [list(s) for s in PLAN_SCORES]
    want = [gold["names"][i] for i, c in zip(gold["runs"][0::2], gold["runs"][1::2]) for _ in range(c)]
    got = plan_grid_names(monkeypatch.setenv, lambda s: monkeypatch.delenv(s, raising=False))
    assert len(got) == len(want) == gold["rows"]
    bad = [k for k in range(len(got)) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:5], [(got[k], want[k]) for k in bad[:5]])


# ---- the nvbio launcher's planner over a fixed grid (tests/golden/nv_plan_names.json, written by
#      tools/plan_grid.py --nv from the build of the commit it names) ----
# every lane-group shape edge G*R of batched.hip's shape list, and the length past it
NV_PLAN_PLENS = (64, 65, 96, 97, 128, 129, 152, 153, 192, 193, 256, 257, 320, 321, 512, 513, 1024, 1025)
# Text lengths either side of: the packed kernel's per-pair tables leaving LDS at G = 8 (4-column
# tables x 64 pairs: 640 columns); the int32 kernel's per-pair slots leaving LDS at G = 8 (2,560
# codes, which moves the shape to G = 16; also the packed limit at G = 32) and at G = 64 (20,480: no
# plan); the f16 window of the plain score set in the GLOBAL / SEMI_GLOBAL Gotoh drift frame at the
# shortest pattern (1683 + 5 * 64 + 2 t <= 0x7BFF: 14,870); with a zero gap extension the drift
# frame admits any text, and one shared text's tables leave LDS at 40,952 columns (G = 8); its
# int32 slot at 81,920 (no plan).  The plain set's window outside the drift frame (1610 +
# 8 (p + t + 2) <= 0x7BFF) closes between 2,561 and 14,870 for every pattern length.
NV_PLAN_TLENS = (64, 640, 641, 2560, 2561, 14870, 14871, 20480, 20481, 40952, 40953, 81920, 81921)
# (match, mismatch, gap_open, gap_ext, deletion, insertion), one either side of each admission rule
# of the packed kernel, the sets fewest rules admit first (longer runs in the fixture): a positive
# mismatch; match - mismatch 256; a magnitude of 0x201; an edit-distance aligner's gap_open /
# gap_ext, which no ED kernel reads, closing the window; a magnitude of 0x200; match - mismatch
# 255; a positive gap for Gotoh only; plain; an ED aligner's gap_open / gap_ext moving the window;
# a zero extension; a positive gap for linear gaps only
NV_PLAN_SCORES = ((2, 1, -2, -1, -1, -1), (200, -56, -2, -1, -1, -1), (2, -1, -0x201, -1, -1, -1),
                  (0, 0, -300, -300, 0, 0), (2, -1, -0x200, -1, -1, -1), (200, -55, -2, -1, -1, -1),
                  (2, -1, 1, -1, -1, -1), (2, -1, -2, -1, -1, -1), (0, 0, -3, -3, 0, 0), (2, -1, -2, 0, -1, -1),
                  (2, -1, -2, -1, -1, 1))
NV_PLAN_ENVS = (None, "GASALX_NV16=0")


def nv_plan_grid_names(setenv, delenv):
    """The name of every grid row, in the fixture's order: switch, entry point (describe_plan, then
    describe_sinks_plan), aligner, type, shared / per-pair text, pattern length, text length, text
    bits, score set."""
    lib, buf = G.lib(), ctypes.create_string_buffer(128)
    names = []
    for env in NV_PLAN_ENVS:
        delenv("GASALX_NV16")
        if env:
            setenv(*env.split("="))
        for fn in (lib.gasalx_nv_describe_plan, lib.gasalx_nv_describe_sinks_plan):
            for aligner in (G.NV_ED, G.NV_SW, G.NV_GOTOH):
                for typ in (G.NV_GLOBAL, G.NV_LOCAL, G.NV_SEMI_GLOBAL):
                    refs = [ctypes.byref(G.NvAligner(aligner, typ, *s).cstruct()) for s in NV_PLAN_SCORES]
                    for per_pair in (0, 1):
                        for p in NV_PLAN_PLENS:
                            for t in NV_PLAN_TLENS:
                                for bits in (2, 4, 8):
                                    for ref in refs:
                                        assert fn(ref, p, t, per_pair, bits, buf, 128) == 0
                                        names.append(buf.value)
    return [n.decode() for n in names]


def test_nv_plan_names_match_golden_grid(monkeypatch):
    """The nvbio launcher names the same kernel for every row of the grid as the build that wrote the
    fixture (encoded as plan_names.json is)."""
    import json
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "nv_plan_names.json")))
    assert gold["plens"] == list(NV_PLAN_PLENS) and gold["tlens"] == list(NV_PLAN_TLENS)
    assert gold["scores"] == [list(s) for s in NV_PLAN_SCORES] and gold["envs"] == list(NV_PLAN_ENVS)
    want = [gold["names"][i] for i, c in zip(gold["runs"][0::2], gold["runs"][1::2]) for _ in range(c)]
    got = nv_plan_grid_names(monkeypatch.setenv, lambda s: monkeypatch.delenv(s, raising=False))
    assert len(got) == len(want) == gold["rows"]
    bad = [k for k in range(len(got)) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:5], [(got[k], want[k]) for k in bad[:5]])


def test_synthetic_workloads_deterministic():
    a = G.Batch.synth(2, 64, 0x5EED0002)
    b = G.Batch.synth(2, 64, 0x5EED0002)
    assert np.array_equal(a.q_data, b.q_data) and np.array_equal(a.t_data, b.t_data)
    assert set(a.q_lens) == {150} and set(a.t_lens) == {150} and a.q_bytes == 64 * 152
    c = G.Batch.synth(4, 32, 0x5EED0004)
    assert set(c.q_lens) == {150} and set(c.t_lens) == {182}


def test_pairhmm_params_match_oracle():
    import oracle as O
    bq = np.arange(0, 60, dtype=np.uint8)
    iq = np.full(60, 45, np.uint8)
    dq = np.full(60, 45, np.uint8)
    a = G.pairhmm_params(bq, iq, dq)
    b = O.pairhmm_params(bq, iq, dq)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_no_gpu_call_fails_loudly_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        G.Engine(0)


def test_synth_range_is_a_shard_of_the_global_batch():
    # pairs [start, start + n) generated alone equal the same pairs of the whole batch,
    # across a 65,536-pair block boundary (gasalx_synth_range: one generator per block)
    full = G.Batch.synth(1, 70000, 0x5EED0001)
    for start, n in ((0, 5), (65530, 12), (69990, 10)):
        part = G.Batch.synth(1, n, 0x5EED0001, start=start)
        sl = full.slice(start, start + n)
        assert np.array_equal(part.q_data, sl.q_data) and np.array_equal(part.t_data, sl.t_data)
        assert np.array_equal(part.q_offsets, sl.q_offsets) and np.array_equal(part.t_lens, sl.t_lens)
    assert G.synth_spec(4) == (150, 182) and G.synth_spec(1) == (64, 64)


def test_batch_slice_matches_subset():
    b = G.Batch.from_pairs(["ACGTA", "A" * 17, "CG", "T" * 8], ["GG", "C" * 9, "ACGTACGTA", "A"])
    for s, e in ((0, 4), (1, 3), (2, 2), (3, 4)):
        x, y = b.slice(s, e), b.subset(np.arange(s, e))
        assert x.n == y.n
        if x.n:
            assert np.array_equal(x.q_data, y.q_data) and np.array_equal(x.t_offsets, y.t_offsets)
            assert np.array_equal(x.q_lens, y.q_lens)


def test_pinned_host_lifetime_follows_its_arrays():
    # gasalx_host_alloc is exported; without a device it fails loudly, with one the
    # memory lives as long as any view (tests/test_gpu_parity.py covers the GPU side)
    import gc
    import weakref
    try:
        h = G.PinnedHost(64)
    except RuntimeError:
        pytest.skip("no HIP device for page-locked memory")
    view = h.array[8:16]
    ref = weakref.ref(h)
    h.close()
    del h
    gc.collect()
    assert ref() is not None          # the view still holds the owner
    view[:] = 7
    del view
    gc.collect()
    assert ref() is None


def test_reference_error_helpers_compile(tmp_path):
    # a caller written against the reference's gasal.h error helpers (gasal.h:15-34)
    # compiles unchanged against include/gasal_header.h
    src = tmp_path / "caller.cpp"
    src.write_text('#include "gasal_header.h"\n'
                   "int f() { hipError_t err; CHECKCUDAERROR(hipGetLastError());\n"
                   "          return CudaCheckKernelLaunch(); }\n")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "caller.o")], check=True, capture_output=True)


# ---- nvbio traceback workspace and its chunk budget (gasalx_nv_*traceback_workspace) ----
NV_TB_DEFAULT_BUDGET = 4 << 30


def _nv_tb_expected(max_p, max_t, n, budget=NV_TB_DEFAULT_BUDGET):
    # gasalx.h: pad8(pattern) x text flag bytes + 8 bytes per text symbol per pair, chunks within the budget
    per = (max_p + 7) // 8 * 8 * max_t + 8 * max_t
    return per * max(1, min(n, budget // max(per, 1))) + 128


def _nv_btb_expected(max_p, band, n, budget=NV_TB_DEFAULT_BUDGET):
    # gasalx.h: max pattern x pad4(band) flag bytes per pair
    per = max_p * ((band + 3) // 4 * 4)
    return per * max(1, min(n, budget // max(per, 1))) + 64


NV_TB_SHAPES = [(G.nv_traceback_workspace, _nv_tb_expected, a, b)
                for a, b in ((150, 182), (1, 1), (70, 96), (65, 7), (1024, 6000), (4000, 4000))] + \
               [(G.nv_banded_traceback_workspace, _nv_btb_expected, a, b)
                for a, b in ((150, 7), (160, 16), (1, 2), (1200, 31), (32000, 32))]
NV_TB_COUNTS = (0, 1, 2, 3, 7, 8, 64, 203, 4097, 150_000, 1_000_000, 2**31, 2**32 - 1)


@pytest.mark.parametrize("fn,expected,a,b", NV_TB_SHAPES, ids=lambda v: v.__name__.lstrip("_") if callable(v) else str(v))
def test_nv_traceback_workspace_default_budget(monkeypatch, fn, expected, a, b):
    # unset: the 4 GiB budget, the numbers of the documented formula (1 M 150 x 182 pairs: 147,492 per chunk)
    monkeypatch.delenv("GASALX_NV_TB_BUDGET", raising=False)
    got = [fn(a, b, n) for n in NV_TB_COUNTS]
    assert got == [expected(a, b, n) for n in NV_TB_COUNTS]
    assert got == sorted(got)
    assert G.nv_traceback_workspace(150, 182, 1_000_000) == 29120 * 147492 + 128


@pytest.mark.parametrize("fn,expected,a,b", NV_TB_SHAPES, ids=lambda v: v.__name__.lstrip("_") if callable(v) else str(v))
def test_nv_traceback_workspace_under_budget(monkeypatch, fn, expected, a, b):
    # with budget B: non-decreasing in n, at most one pair's workspace past B, and for large n the
    # chunk of B / per pairs, per the bytes one more pair adds
    one = expected(a, b, 1)
    per = expected(a, b, 2, 1 << 62) - one
    for budget in (1, per - 1, per, per + 1, 7 * per, 7 * per + per - 1, 7 * one, 64 * one, 1 << 20, (1 << 32) + 5,
                   2**64 - 1):
        monkeypatch.setenv("GASALX_NV_TB_BUDGET", str(budget))
        got = [fn(a, b, n) for n in NV_TB_COUNTS]
        assert got == [expected(a, b, n, budget) for n in NV_TB_COUNTS], budget
        assert got == sorted(got), budget                            # non-decreasing in n
        assert all(g <= budget + one for g in got), budget          # never more than one pair past the budget
        c = max(1, budget // per)
        if c < 2**32:
            assert fn(a, b, 2**32 - 1) == fn(a, b, c), budget        # large n: the chunk of budget / per pairs


@pytest.mark.parametrize("value", ["", "0", "000", "abc", "12abc", "-1", "+5", "0x1000", "1e9", " ", "4 096",
                                   "18446744073709551616", "99999999999999999999999999"])
def test_nv_traceback_budget_unparsable_is_unset(monkeypatch, value):
    monkeypatch.setenv("GASALX_NV_TB_BUDGET", value)
    assert G.nv_traceback_workspace(150, 182, 1_000_000) == _nv_tb_expected(150, 182, 1_000_000)
    assert G.nv_banded_traceback_workspace(1200, 31, 1_000_000) == _nv_btb_expected(1200, 31, 1_000_000)
    # and a value that parses is taken, read again on every call
    monkeypatch.setenv("GASALX_NV_TB_BUDGET", "2912000")
    assert G.nv_traceback_workspace(150, 182, 1_000_000) == 29120 * 100 + 128
    monkeypatch.delenv("GASALX_NV_TB_BUDGET")
    assert G.nv_traceback_workspace(150, 182, 1_000_000) == 29120 * 147492 + 128

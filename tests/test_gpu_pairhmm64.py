"""The float64 PairHMM kernel and the log10 rescue pipeline on the GPU, against the float64
references: tests/independent.py's pairhmm64 (initial constant 2^120) where it does not
underflow, test_pairhmm64_api.forward64 (initial constant as an argument) for long reads.

Tolerances.  Raw float64 values, rtol 1e-10: every term of the recurrence is non-negative
(no cancellation); a path has at most R + H <= 756 cell steps of at most 8 roundings each
plus a sum of <= 500 terms, about 7e3 * 2^-53 = 8e-13 per side.  1e-10 leaves about 60x over
both sides and is five orders tighter than one accidental float32 operation would pass.
log10 of a rescued pair, atol 1e-9: 1e-10 relative is 4.3e-11 in log10, plus the log's own
rounding at magnitude <= 330.  log10 of an accepted fp32 result, atol 1e-5: the fp32 contract
is rtol 1e-5 plus the oracle's own distance m <= 1e-5 from float64 (test_gpu_independent
asserts m), 2e-5 / ln 10 = 8.7e-6."""
import os
import subprocess

import numpy as np
import pytest

import gasal_ffi as G
import helpers
import independent as I
import oracle as O
from test_pairhmm64_api import forward64

pytestmark = pytest.mark.gpu

CAPS = [256, 255, 129, 128, 127, 64, 63, 33, 32, 31, 9, 8, 7]
LOG2 = np.log10(2.0)
THR = float(np.float32(1e-28))
FLT_MIN = np.finfo(np.float32).tiny
_C = {}


@pytest.fixture(scope="module", autouse=True)
def _build():
    O.build()


def _grid():
    """hmm_related_grid plus the pair with a leading N (test_gpu_independent._hmm_grid's set)
    and its float64 values (2^120 scale), computed once."""
    if "grid" not in _C:
        pairs = helpers.hmm_related_grid()
        odd = dict(pairs[40])
        odd["read"] = "N" + odd["read"][1:]
        pairs = pairs + [odd]
        f = I.pairhmm64(*helpers.hmm_args(pairs, O.pairhmm_params))
        assert f.min() >= 2e-220
        _C["grid"] = dict(pairs=pairs, f=f)
    return _C["grid"]


def _all498():
    """The related grid, the unrelated 129/256-row reads and the unrelated length sweep of
    test_pairhmm_underflow_class: 498 pairs, float64 values between 2e-220 and 1.2e36."""
    if "all" not in _C:
        pairs = (helpers.hmm_related_grid() + helpers.hmm_unrelated(0xF10, (129, 256) * 6)
                 + helpers.hmm_unrelated(0xDE0, tuple(range(24, 120)), hap_lens=(48, 64, 80, 96)))
        args = helpers.hmm_args(pairs, O.pairhmm_params)
        f = I.pairhmm64(*args)
        assert len(pairs) == 498 and f.min() >= 2e-220
        # no pair sits near the threshold: the fp32 pass cannot put one on the other side
        assert np.abs(f / THR - 1).min() > 0.29
        _C["all"] = dict(pairs=pairs, args=args, f=f)
    return _C["all"]


def _raw(engine, pairs):
    g = engine.pairhmm64_host(*helpers.hmm_args(pairs, O.pairhmm_params))
    assert g.dtype == np.float64
    return g


def _related(rng, R, H):
    hap = helpers.random_seq(rng, H).decode()
    return dict(read=helpers.hmm_related_read(rng, hap, R), hap=hap, bq=rng.integers(10, 41, R),
                iq=rng.integers(10, 26, R), dq=rng.integers(10, 60, R))


# ---------------------------------------------------------------- 1. raw kernel ----
def test_raw_grid(engine):
    h = _grid()
    g = _raw(engine, h["pairs"]) * 2.0 ** -900
    np.testing.assert_allclose(g, h["f"], rtol=1e-10, atol=0)


@pytest.mark.parametrize("cap", CAPS)
def test_raw_per_lane_group(engine, cap):
    """Reads of at most `cap` rows: every G instance with a full and a partly virtual top lane."""
    h = _grid()
    idx = [i for i, p in enumerate(h["pairs"]) if len(p["read"]) <= cap]
    g = _raw(engine, [h["pairs"][i] for i in idx]) * 2.0 ** -900
    np.testing.assert_allclose(g, h["f"][idx], rtol=1e-10, atol=0, err_msg=f"reads <= {cap}")


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cap", CAPS)
def test_raw_partial_block(engine, cap, n):
    """n pairs, the longest first: the last (only) block has empty slots."""
    h = _grid()
    idx = sorted((i for i, p in enumerate(h["pairs"]) if len(p["read"]) <= cap),
                 key=lambda i: (-len(h["pairs"][i]["read"]), -len(h["pairs"][i]["hap"])))[:n]
    g = _raw(engine, [h["pairs"][i] for i in idx]) * 2.0 ** -900
    np.testing.assert_allclose(g, h["f"][idx], rtol=1e-10, atol=0, err_msg=f"reads <= {cap}, n = {n}")


# ---------------------------------------------------------------- 2. long reads ----
def test_long_reads(engine):
    """Reads past 256 rows (8 rows per lane), where pairhmm64's 2^120 underflows to 0."""
    rng = np.random.default_rng(0x64A)
    pairs = [_related(rng, R, H) for R, H in ((257, 300), (511, 500), (512, 512), (512, 64), (300, 1))]
    pairs += helpers.hmm_unrelated(7, (400, 512))
    ref = np.array([forward64(p, 2.0 ** 1020) for p in pairs])
    g = _raw(engine, pairs)
    assert np.all(np.isfinite(g)) and np.all(g > 0)
    np.testing.assert_allclose(g, ref, rtol=1e-10, atol=0)
    # a 300-row launch alone: 8 rows per lane with the top lanes virtual
    g1 = _raw(engine, pairs[4:5])
    np.testing.assert_allclose(g1, ref[4:5], rtol=1e-10, atol=0)


def test_limits(engine):
    rng = np.random.default_rng(5)
    with pytest.raises(RuntimeError, match="longer than 512"):
        _raw(engine, [_related(rng, 513, 20)])
    # 16 pairs of 4 lanes per wave: 64 haplotype slots share the 160 KB of LDS
    with pytest.raises(RuntimeError, match="haplotype too long"):
        _raw(engine, [_related(rng, 8, 2600)])


# ------------------------------------------------- 3. quality form = parameter form ----
def test_quals_form_equals_params_form(engine):
    h = _grid()
    pairs = h["pairs"][::3] + h["pairs"][-1:]
    d = G.HmmData.from_pairs(pairs)
    q = engine.pairhmm64_quals_host(d)
    qm, de, xi, al = d.float_params()
    p = engine.pairhmm64_host(d.reads, d.read_offsets, d.read_lens, qm, de, xi, al, d.haps, d.hap_offsets, d.hap_lens)
    assert np.array_equal(q.view(np.uint64), p.view(np.uint64))
    idx = list(range(0, len(h["pairs"]), 3)) + [len(h["pairs"]) - 1]
    np.testing.assert_allclose(q * 2.0 ** -900, h["f"][idx], rtol=1e-10, atol=0)


# ------------------------------------------------------------- 4. log10 pipeline ----
def _check_log10(lg, used, f):
    """lg, used against the float64 values f (2^120 scale), at the module's tolerances."""
    assert np.all(np.isfinite(lg))
    ref = np.log10(f) - 120 * LOG2
    r = used.astype(bool)
    np.testing.assert_allclose(lg[r], ref[r], rtol=0, atol=1e-9)
    np.testing.assert_allclose(lg[~r], ref[~r], rtol=0, atol=1e-5)


def test_log10_pipeline(engine):
    h = _all498()
    lg, used = engine.pairhmm_log10_host(*h["args"])
    expect = h["f"] < THR
    print(f"rescued {int(used.sum())} of {len(used)} (float64 side: {int(expect.sum())}), n_rescued {engine.n_rescued}")
    assert np.array_equal(used.astype(bool), expect)
    assert expect.sum() == 221 and engine.n_rescued == 221
    _check_log10(lg, used, h["f"])


def test_log10_quals_form(engine):
    """The quality form: fp32 pass in sorted length classes, rescue in one launch."""
    h = _all498()
    d = G.HmmData.from_pairs(h["pairs"])
    lg, used = engine.pairhmm_quals_log10_host(d)
    assert np.array_equal(used.astype(bool), h["f"] < THR) and engine.n_rescued == int((h["f"] < THR).sum())
    _check_log10(lg, used, h["f"])


# ---------------------------------------------------------------- 5. thresholds ----
def test_threshold_rescues_all(engine):
    h = _grid()
    args = helpers.hmm_args(h["pairs"], O.pairhmm_params)
    lg, used = engine.pairhmm_log10_host(*args, min_accepted=3e38)
    assert used.all() and engine.n_rescued == len(used)
    np.testing.assert_allclose(lg, np.log10(h["f"]) - 120 * LOG2, rtol=0, atol=1e-9)


def test_threshold_smallest(engine):
    """min_accepted = 1e-45: exactly the pairs whose fp32 result is 0, denormal or non-finite."""
    h = _all498()
    r32 = engine.pairhmm_host(*h["args"])
    expect = ~(np.isfinite(r32) & (r32 >= FLT_MIN))
    assert ((r32 > 0) & (r32 < FLT_MIN)).any() and (r32 == 0).any()
    lg, used = engine.pairhmm_log10_host(*h["args"], min_accepted=1e-45)
    assert np.array_equal(used.astype(bool), expect) and engine.n_rescued == int(expect.sum())
    assert np.all(np.isfinite(lg))
    np.testing.assert_allclose(lg[expect], np.log10(h["f"][expect]) - 120 * LOG2, rtol=0, atol=1e-9)


def test_no_rescue(engine):
    h = _grid()
    idx = [i for i, p in enumerate(h["pairs"]) if len(p["read"]) <= 65 and h["f"][i] >= 1e-20]
    assert len(idx) >= 40
    args = helpers.hmm_args([h["pairs"][i] for i in idx], O.pairhmm_params)
    lg, used = engine.pairhmm_log10_host(*args)
    assert engine.n_rescued == 0 and not used.any()
    r32 = engine.pairhmm_host(*args).astype(np.float64)
    np.testing.assert_allclose(lg, np.log10(r32) - 120 * LOG2, rtol=0, atol=1e-12)


# -------------------------------------------------------------- 6. device entry ----
def test_log10_device_entry(engine):
    import torch
    h = _all498()
    reads, ro, rl, qm, de, xi, al, haps, ho, hl = h["args"]
    u = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")
    i32 = lambda a: np.ascontiguousarray(a, np.uint32).view(np.int32)
    t = {"reads": u(reads), "haps": u(haps), "read_offsets": u(i32(ro)), "read_lens": u(i32(rl)),
         "hap_offsets": u(i32(ho)), "hap_lens": u(i32(hl)), "qm": u(qm), "delta": u(de), "xiksi": u(xi),
         "alpha": u(al)}
    n = len(rl)
    out = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    used = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
    raw = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    with torch.cuda.stream(st):
        engine.pairhmm_log10_device_ptrs(ptrs, len(reads), len(haps), n, int(rl.max()), int(hl.max()),
                                         out.data_ptr(), used.data_ptr(), stream=st.cuda_stream)
        engine.pairhmm64_device_ptrs(ptrs, len(reads), len(haps), n, int(rl.max()), int(hl.max()),
                                     raw.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    lg, ud = engine.pairhmm_log10_host(*h["args"])
    assert np.array_equal(used.cpu().numpy(), ud)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), lg.view(np.uint64))
    np.testing.assert_allclose(raw.cpu().numpy() * 2.0 ** -900, h["f"], rtol=1e-10, atol=0)


# -------------------------------------------------------------------- 7. driver ----
def test_pairhmm_prog_log10(tmp_path):
    from test_hmm_io import _rand_pairs, _write_groups
    rng = np.random.default_rng(0x4D33)
    groups = [_rand_pairs(rng, 40), _rand_pairs(rng, 7)]
    # one read replaced by an unrelated one with high base qualities
    bad = helpers.hmm_unrelated(11, (100,), hap_lens=(64,))[0]
    bad["gcp"] = np.full(100, 10)
    groups[0][5] = bad
    path = tmp_path / "in.txt"
    _write_groups(path, groups)
    d = G.read_hmm_file(str(path))
    qm, de, xi, al = O.pairhmm_params(d.base_quals, d.ins_quals, d.del_quals)
    args = (d.reads, d.read_offsets, d.read_lens, qm, de, xi, al, d.haps, d.hap_offsets, d.hap_lens)
    f = I.pairhmm64(*args)
    o = O.pairhmm(*args)
    assert f.min() > 1e-290 and f[5] < THR
    # the fp32 side of every pair falls where float64 puts it (a pair near the threshold or in the
    # fp32 denormal range would make the expected count a matter of fp32 rounding)
    expect = f < THR
    assert np.array_equal(~(np.isfinite(o) & (o >= np.float32(1e-28))), expect)
    prog = os.path.join(os.path.dirname(helpers.GOLDEN), "..", "tools", "pairhmm_prog")
    out = subprocess.run([prog, "-log10", "-print", "all", str(path)], capture_output=True, text=True,
                         check=True).stdout
    vals = np.array([float(l.split()[1]) for l in out.splitlines() if l.startswith("  i=")])
    assert len(vals) == 47 and np.all(np.isfinite(vals))
    ref = np.log10(f) - 120 * LOG2
    # "%.9g" keeps 9 significant digits: half a unit of the ninth digit of each printed value
    # comes on top of the rescued pairs' 1e-9 (5e-7 at magnitude 100..330, where 1e-9 cannot be printed)
    half = 0.5 * 10.0 ** (np.floor(np.log10(np.abs(ref))) - 8)
    assert np.all(np.abs(vals - ref)[expect] <= 1e-9 + half[expect])
    np.testing.assert_allclose(vals[~expect], ref[~expect], rtol=0, atol=1e-5)
    assert out.splitlines()[-1] == f"rescued: {int(expect.sum())} of 47"
    # without the flag: the lines as before, against the oracle as test_pairhmm_prog_driver does
    out = subprocess.run([prog, "-print", "all", str(path)], capture_output=True, text=True, check=True).stdout
    lines = out.splitlines()
    vals = [float(l.split()[1]) for l in lines if l.startswith("  i=")]
    np.testing.assert_allclose(np.array(vals, np.float32), o, rtol=1e-5)
    assert len(lines) == 47 + 2 and lines[-1].startswith("GCUPS:") and lines[-2].startswith("read_time=")
    assert not any("rescued" in l for l in lines)
    assert all(l == "  i=%d  %e" % (i if i < 40 else i - 40, v) for i, (l, v) in enumerate(zip(lines[:47], vals)))

"""The HIP engine compared *directly* with the independent references of
tests/independent.py (numpy restatements written from the reference kernels, a float64
PairHMM, a CIGAR replay), without going through the C oracle: a misreading that the oracle
and a kernel share passes every test of test_gpu_parity.py and fails here.

Every test asserts through describe_plan which kernel family it ran, so a planner change
that reroutes its shapes fails loudly instead of passing on another kernel."""
import zlib

import numpy as np
import pytest

import gasal_ffi as G
import helpers
import independent as I
import oracle as O

pytestmark = pytest.mark.gpu

SCORES = [(1, 4, 6, 1), (2, 3, 5, 2)]
ALPHABETS = [b"ACGT", b"ACGTN"]
SMALL = (1, 40, 1, 40)            # the two halves of a packed register hold different lengths
LARGE = (140, 160, 140, 160)      # config-2 shape
SEMI_LARGE = (150, 150, 182, 182)
FLT_MIN = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module", autouse=True)
def _build():
    O.build()


def _batch(lens, alphabet, sc, n=300, tag=""):
    rng = np.random.default_rng(zlib.crc32(repr((lens, alphabet, sc, tag)).encode()) & 0xFFFF)
    qs, ts = helpers.random_pairs(rng, n, *lens, alphabet=alphabet)
    return qs, ts, G.Batch.from_pairs(qs, ts)


def _kw(sc):
    a, bb, o, e = sc
    return dict(match=a, mismatch=bb, gap_open=o, gap_extend=e)


def _exact(g, r, fields, what):
    for f in fields:
        bad = np.flatnonzero(g[f] != r[f])
        assert bad.size == 0, f"{what} {f}: {bad.size} differ, first #{bad[0]}: gpu={g[f][bad[0]]} independent={r[f][bad[0]]}"


def _plan(kw, lens, *families):
    plan = G.describe_plan(G.make_params(**kw), lens[1], lens[3])
    assert plan.startswith(families), f"{plan}: expected one of {families}"
    return plan


# combinations of (score set, alphabet); the large shapes take one each in turn, the small
# shape takes all four
COMBOS = [(sc, al) for sc in SCORES for al in ALPHABETS]
SHAPES = [(SMALL, c) for c in COMBOS]


def _cases(large, k):
    """All four combinations at the small shape, combination k (mod 4) at the large one."""
    return SHAPES + [(large, COMBOS[k % 4])]


# ------------------------------------------------------------ score kernels ----
@pytest.mark.parametrize("lens,combo", SHAPES + [(LARGE, c) for c in COMBOS])
def test_local_second_best(engine, lens, combo):
    sc, alphabet = combo
    _, _, b = _batch(lens, alphabet, sc)
    fields = ("score", "q_end", "t_end")
    kw = dict(algo=G.LOCAL, second_best=1, **_kw(sc))
    _plan(kw, lens, "local16_second")
    ref = I.local(b, *sc, second=True)
    _exact(engine.align_host(b, G.make_params(**kw)), ref, fields + ("score2", "q_end2", "t_end2"), "LOCAL second")
    kw = dict(algo=G.LOCAL, **_kw(sc))
    _plan(kw, lens, "wavefront16_local_G", "wavefront16_local_u16_G")
    _exact(engine.align_host(b, G.make_params(**kw)), ref, fields, "LOCAL")


@pytest.mark.parametrize("lens,combo", SHAPES + [(LARGE, c) for c in COMBOS])
def test_global(engine, lens, combo):
    sc, alphabet = combo
    _, _, b = _batch(lens, alphabet, sc)
    kw = dict(algo=G.GLOBAL, **_kw(sc))
    _plan(kw, lens, "wavefront16_global_G")
    _exact(engine.align_host(b, G.make_params(**kw)), I.global_(b, *sc), ("score",), "GLOBAL")


SEMI_FAMILY = {G.NONE: ("semi_tail_none",), G.TARGET: ("wavefront16_semi_G",),
               G.QUERY: ("wavefront16_semi_tq_G",), G.BOTH: ("wavefront16_semi_tq_G",)}


@pytest.mark.parametrize("head", [G.NONE, G.QUERY, G.TARGET, G.BOTH])
@pytest.mark.parametrize("tail", [G.NONE, G.QUERY, G.TARGET, G.BOTH])
def test_semiglobal(engine, head, tail):
    for lens, (sc, alphabet) in _cases(SEMI_LARGE, 4 * head + tail + head):
        _, _, b = _batch(lens, alphabet, sc, tag=(head, tail))
        kw = dict(algo=G.SEMI_GLOBAL, head=head, tail=tail, **_kw(sc))
        _plan(kw, lens, *SEMI_FAMILY[tail])
        _exact(engine.align_host(b, G.make_params(**kw)), I.semi(b, head, tail, *sc), ("score", "q_end", "t_end"),
               f"SEMI {head}/{tail} {lens} {sc} {alphabet}")


@pytest.mark.parametrize("k_band", [0, 4, 16, 400])
def test_banded(engine, k_band):
    for lens, (sc, alphabet) in _cases(LARGE, [0, 4, 16, 400].index(k_band)):
        _, _, b = _batch(lens, alphabet, sc, tag=k_band)
        kw = dict(algo=G.BANDED, k_band=k_band, **_kw(sc))
        _plan(kw, lens, "banded16")
        _exact(engine.align_host(b, G.make_params(**kw)), I.banded(b, k_band, *sc), ("score", "q_end", "t_end"),
               f"BANDED {k_band} {lens} {sc} {alphabet}")


# ------------------------------------------------------- GLOBAL+TB replay ----
@pytest.mark.parametrize("env", [{}, {"GASALX_TB_BAND_W": "0"}, {"GASALX_TB_BAND_W": "3", "GASALX_TB_FBCAP": "64"}],
                         ids=["default", "w0", "w3cap64"])
@pytest.mark.parametrize("n,lens", [(300, (20, 310, 20, 310)), (333, (1, 40, 1, 40))])
def test_global_tb_replay(engine, monkeypatch, n, lens, env):
    """The GPU's own GLOBAL+TB CIGARs replayed over the bases (rules G1-G3 of replay_cigar):
    lengths, labels, replayed score == GPU score == independent.global_().  Q14 overflow is
    decided from the GPU's own n_ops."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for sc in SCORES:
        qs, ts, b = _batch(lens, b"ACGT", sc, n=n, tag=sorted(env.items()))
        kw = dict(algo=G.GLOBAL, start_pos=G.WITH_TB, **_kw(sc))
        plan = _plan(kw, lens, "wavefront16_global_tb")
        assert "_tbband_" in plan
        g = engine.align_host(b, G.make_params(**kw))
        keep = helpers.cigar_slots_kept(b.q_offsets, b.q_lens, g["n_ops"])
        assert 1 - keep.mean() <= 0.02
        st = I.replay_batch(qs, ts, b, g, sc, I.GLOBAL_MODE, G.decode_cigar, keep)
        assert not st["failures"], (len(st["failures"]), st["failures"][:3])
        assert st["checked"] == keep.sum()
        _exact(g, I.global_(b, *sc), ("score",), "GLOBAL+TB")


# -------------------------------------------------------- LOCAL+TB replay ----
@pytest.mark.parametrize("sc,alphabet,family", [
    ((1, 4, 6, 1), b"ACGT", "wavefront16_local_tb"),
    ((1, 4, 6, 1), b"ACGTRY", "wavefront16_local_tb"),      # IUPAC: declined blocks take the int32 kernel
    ((1, 4, 6, 1), b"ACGTACGTACGTN", "wavefront16_local_tb"),
    ((2, 3, 5, 2), b"ACGT", "wavefront_local_tb_keys"),
])
def test_local_tb_replay_and_rectangle(engine, sc, alphabet, family):
    """The GPU's own LOCAL+TB output: CIGAR replay, the rectangle property of its start and
    end (global_textbook of the rectangle == score) and score == independent.local()."""
    lens = (1, 200, 1, 250)
    qs, ts, b = _batch(lens, alphabet, sc)
    kw = dict(algo=G.LOCAL, start_pos=G.WITH_TB, **_kw(sc))
    _plan(kw, lens, family)
    g = engine.align_host(b, G.make_params(**kw))
    keep = helpers.cigar_slots_kept(b.q_offsets, b.q_lens, g["n_ops"])
    assert 1 - keep.mean() <= 0.02
    st = I.replay_batch(qs, ts, b, g, sc, I.LOCAL_MODE, G.decode_cigar, keep)
    assert not st["failures"], (len(st["failures"]), st["failures"][:3])
    assert st["zero"] <= 0.02 * b.n and st["stepped"] == 0
    if b"N" not in alphabet:
        assert st["n_path"] == 0
    _exact(g, I.local(b, *sc), ("score", "q_end", "t_end"), "LOCAL+TB")


# -------------------------------------------------------------- WITH_START ----
@pytest.mark.parametrize("qr,tr,alphabet,sc", [
    ((1, 40), (1, 40), b"ACGT", (1, 4, 6, 1)),
    ((140, 160), (140, 160), b"ACGT", (1, 4, 6, 1)),
    ((1, 200), (1, 250), b"ACGTN", (1, 4, 6, 1)),
    ((50, 150), (50, 180), b"ACGTRYacgt", (1, 4, 6, 1)),
    ((60, 160), (60, 160), b"ACGT", (2, 3, 5, 2)),
    ((60, 160), (60, 160), b"ACGT", (3, 6, 0, 0)),
    ((200, 320), (150, 400), b"ACGT", (1, 4, 6, 1)),
])
def test_local_with_start(engine, qr, tr, alphabet, sc):
    """The GPU's q_start / t_start equal independent.local_start(), ends and
    score equal independent.local()."""
    lens = (*qr, *tr)
    rng = np.random.default_rng(zlib.crc32(repr((qr, tr, alphabet, sc)).encode()) & 0xFFFF)
    qs, ts = helpers.random_pairs(rng, 300, *lens, alphabet=alphabet, related=0.5)
    b = G.Batch.from_pairs(qs, ts)
    kw = dict(algo=G.LOCAL, start_pos=G.WITH_START, **_kw(sc))
    _plan(kw, lens, "wavefront16_local_start", "wavefront_local_start")
    g = engine.align_host(b, G.make_params(**kw))
    fwd = I.local(b, *sc)
    _exact(g, fwd, ("score", "q_end", "t_end"), "WITH_START")
    _exact(g, I.local_start(b, *sc, fwd=fwd), ("q_start", "t_start"), "WITH_START")


# ------------------------------------------------------------------ PairHMM ----
_HMM = {}


def _hmm_grid():
    """Related reads over the lane-boundary grid plus one pair with an N (its block takes the
    compare path, the others the prior table); float64 values and the oracle's own worst
    relative error against them, computed once."""
    if not _HMM:
        pairs = helpers.hmm_related_grid()
        odd = dict(pairs[40])
        odd["read"] = "N" + odd["read"][1:]
        pairs = pairs + [odd]
        args = helpers.hmm_args(pairs, O.pairhmm_params)
        f = I.pairhmm64(*args)
        forced = np.array([helpers.hmm_insertion_bound(len(p["read"]), len(p["hap"])) for p in pairs])
        assert np.all(f[~forced] >= 1e-30) and np.all(f[forced] < 1e-45)
        o = O.pairhmm(*args).astype(np.float64)
        m = float((np.abs(o[~forced] - f[~forced]) / f[~forced]).max())
        assert m <= 1e-5
        _HMM.update(pairs=pairs, f=f, forced=forced, m=m)
    return _HMM


def _hmm_check(engine, idx, what):
    h = _hmm_grid()
    pairs = [h["pairs"][i] for i in idx]
    f, forced = h["f"][idx], h["forced"][idx]
    g = engine.pairhmm_host(*helpers.hmm_args(pairs, O.pairhmm_params)).astype(np.float64)
    assert np.all(np.isfinite(g)), what
    # 1e-5 is the contract against the reference; m is the fp32 reference's own distance from float64
    np.testing.assert_allclose(g[~forced], f[~forced], rtol=1e-5 + h["m"], atol=0, err_msg=what)
    assert np.all((g[forced] >= 0) & (g[forced] < FLT_MIN)), what


def test_pairhmm_against_float64(engine):
    h = _hmm_grid()
    _hmm_check(engine, np.arange(len(h["pairs"])), "whole batch")


@pytest.mark.parametrize("cap", [256, 255, 129, 128, 127, 64, 63, 33, 32, 31, 9, 8, 7])
def test_pairhmm_against_float64_per_lane_group(engine, cap):
    h = _hmm_grid()
    idx = np.array([i for i, p in enumerate(h["pairs"]) if len(p["read"]) <= cap])
    _hmm_check(engine, idx, f"reads <= {cap}")


def test_pairhmm_underflow_class(engine):
    """Below the smallest fp32 denormal (float64 < 1e-45) the GPU returns 0 or a denormal,
    never NaN or inf.  Between 1e-44 and 1e-38, where a GPU may flush denormals and the
    reference does not, the contract does not say which: |gpu - float64| <= FLT_MIN.
    Measured on an MI355X: 19 pairs land there and the GPU flushes none of them (nor does the oracle)."""
    pairs = helpers.hmm_unrelated(0xF10, (129, 256) * 6)
    # read lengths swept until unrelated reads land in the denormal range
    sweep = helpers.hmm_unrelated(0xDE0, tuple(range(24, 120)), hap_lens=(48, 64, 80, 96))
    fs = I.pairhmm64(*helpers.hmm_args(sweep, O.pairhmm_params))
    mid = [p for p, v in zip(sweep, fs) if 1e-44 <= v <= 1e-38]
    assert len(mid) >= 12, len(mid)
    pairs = pairs + mid
    args = helpers.hmm_args(pairs, O.pairhmm_params)
    f = I.pairhmm64(*args)
    g = engine.pairhmm_host(*args).astype(np.float64)
    assert np.all(np.isfinite(g)) and np.all(g >= 0)
    under = f < 1e-45
    assert under.sum() >= 12
    assert np.all(g[under] < FLT_MIN)
    den = (f >= 1e-44) & (f <= 1e-38)
    assert den.sum() >= 12
    print(f"denormal range: {int(den.sum())} pairs, gpu returns 0 for {int((g[den] == 0).sum())}, "
          f"oracle for {int((O.pairhmm(*args)[den] == 0).sum())}")
    assert np.all(np.abs(g[den] - f[den]) <= FLT_MIN)


# ---------------------------------------------------------------------- KSW ----
# (query length range, seed range, environment, gap_open override, the form meant)
KSW_FORMS = {
    "ksw16_64": ((1, 40), (0, 41), {}, None),
    "ksw16_96": ((60, 90), (0, 41), {}, None),
    "ksw16_160": ((140, 158), (0, 41), {}, None),
    "ksw16_global": ((160, 254), (0, 2), {}, None),
    "level0_lds": ((1, 40), (0, 41), {"GASALX_KSW16": "0"}, None),
    "level0_global": ((1, 40), (0, 41), {"GASALX_KSW16": "0", "GASALX_KSW_LDS": "0"}, None),
    "level1": ((100, 200), (300, 60001), {}, None),
    "level2": ((100, 200), (65000, 66001), {}, None),
    "level2_negative_gap": ((100, 200), (0, 41), {}, -1),
}
KSW16_FORMS = ("ksw16_64", "ksw16_96", "ksw16_160", "ksw16_global")
_KSW_REF = {}


def _ksw_case(form, sc, alphabet):
    """The batch of one form and its independent.ksw() answer, computed once.  Queries are
    A/C/G/T only; an ACGTN case puts N into a third of the targets.  ksw16 takes a pair when
    seed + match * min(ql, tl) <= 255, so at match = 2 the targets of the long ksw16 forms
    are cut to (255 - largest seed) // 2 bases: the instance follows the queries alone."""
    key = (form, sc, alphabet)
    if key not in _KSW_REF:
        (qlo, qhi), srange, env, o_neg = KSW_FORMS[form]
        a, bb, o, e = sc
        if o_neg is not None:
            o = o_neg
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()) & 0xFFFF)
        tlo, thi = qlo, qhi
        if form in KSW16_FORMS:
            thi = min(thi, (255 - (srange[1] - 1)) // a)
            tlo = min(tlo, max(1, thi - 30))
        qs, ts = helpers.random_pairs(rng, 301, qlo, qhi, tlo, thi, related=0.6)
        if alphabet == b"ACGTN":
            ts = [bytes(ord("N") if (k % 3 == 0 and rng.random() < 0.1) else c for c in t) for k, t in enumerate(ts)]
            assert sum(b"N" in t for t in ts) >= 20
        b = G.Batch.from_pairs(qs, ts)
        seed = rng.integers(*srange, b.n).astype(np.uint32)
        _KSW_REF[key] = (qs, ts, b, seed, (a, bb, o, e), env, I.ksw(b, seed, a, bb, o, e))
    return _KSW_REF[key]


@pytest.mark.parametrize("sc", SCORES)
@pytest.mark.parametrize("form,alphabet", [(f, b"ACGT") for f in KSW_FORMS] + [(f, b"ACGTN") for f in KSW16_FORMS])
def test_ksw(engine, monkeypatch, form, alphabet, sc):
    """Every KSW kernel form against independent.ksw() directly.  describe_plan names the
    family only, so the form is asserted from the inputs by the dispatcher's documented rule
    (helpers.ksw_routing): the ksw16 instance from cols = (max_q + 3) & ~1, the entry level
    from every pair's bound seed + step * min(ql, tl) against 255 and 65535."""
    qs, ts, b, seed, sc, env, ref = _ksw_case(form, sc, alphabet)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(algo=G.KSW, **_kw(sc))
    assert G.describe_plan(G.make_params(**kw), int(b.q_lens.max()), int(b.t_lens.max())) == "generic_ksw"
    r = helpers.ksw_routing(qs, ts, seed, sc, env)
    cols = (r["max_q"] + 3) & ~1
    if form in KSW16_FORMS:
        assert r["taken"].all(), (form, int((~r["taken"]).sum()), int(r["bound"].max()))
        want = {"ksw16_64": 64, "ksw16_96": 96, "ksw16_160": 160, "ksw16_global": 0}[form]
        assert r["inst"] == want, (form, r["max_q"], cols)
        assert {"ksw16_64": cols <= 64, "ksw16_96": 64 < cols <= 96, "ksw16_160": 96 < cols <= 160,
                "ksw16_global": cols > 160 and r["max_q"] <= 254}[form]
    else:
        assert not r["taken"].any()
        if form.startswith("level0"):
            assert (r["level"] == 0).all() and r["inst"] is None
            assert r["tpb"] == (256 if form == "level0_lds" else 0)
        elif form == "level1":
            assert (r["level"] == 1).all() and r["bound"].min() > 255 and r["bound"].max() <= 65535
        elif form == "level2":
            # the seed range straddles 65535: no pair fits 8 bits, most need the int2 entries
            assert r["bound"].min() > 255 and (r["level"] == 2).sum() >= b.n // 2
        else:
            assert sc[2] < 0 and (r["level"] == 2).all()
    _exact(engine.align_host(b, G.make_params(**kw), seed_scores=seed), ref, ("score", "q_end", "t_end"),
           f"KSW {form} {sc} {alphabet}")


# ----------------------------------------------------- reverse / complement ----
# Per-pair q_ops / t_ops (0 forward, 1 reverse, 2 complement, 3 both) on every kernel path,
# against the independent functions run on independent.apply_ops(batch): the op model is
# written in base space from pack_rc_seqs.h, not from the engine's or the oracle's word-swap
# loop.  Ops also switch the 16-bit wavefront kernels to their packed-load form, which the
# plan name does not show; so every test runs its batch once more with all ops 0 passed as
# arrays (the packed path: has_ops tests the pointers), which must equal the run without op
# arrays on every field.  That tells a packed-load bug from an op bug.
OPS_EDGES_N = ("edges", b"ACGTN")
OPS_EDGES_ODD = ("edges", helpers.OPS_ODD_ALPHABET)
OPS_FLAG = ("flagship", b"ACGT")
OPS_FLAG_N = ("flagship", b"ACGTN")
END_FIELDS = ("score", "q_end", "t_end")


def _ops_plan(kw, c, *families):
    return _plan(kw, (0, int(c["b"].q_lens.max()), 0, int(c["b"].t_lens.max())), *families)


def _ops_run(engine, c, kw, ref, fields, what, tb=False, **extra):
    """The run with ops against ref, and the all-zero-ops run against the run without ops."""
    p = G.make_params(**kw)
    b = c["b"]
    g = engine.align_host(b, p, q_ops=c["qo"], t_ops=c["to"], **extra)
    _exact(g, ref, fields, what)
    zero = np.zeros(b.n, np.uint8)
    gz = engine.align_host(b, p, q_ops=zero, t_ops=zero, **extra)
    gn = engine.align_host(b, p, **extra)
    _exact(gz, gn, G.OUT_FIELDS + (("n_ops",) if tb else ()), what + ", ops all 0 against no ops:")
    if tb:
        # CIGAR bytes of the slots that hold their own CIGAR; a CIGAR longer than its slot runs
        # into the next one, where two threads write the same bytes in no fixed order (Q14)
        keep = helpers.cigar_slots_kept(b.q_offsets, b.q_lens, gn["n_ops"])
        for k in np.flatnonzero(keep):
            lo, m = int(b.q_offsets[k]), int(gn["n_ops"][k])
            assert np.array_equal(gz["cigar"][lo:lo + m], gn["cigar"][lo:lo + m]), f"{what}, ops all 0 against no ops: CIGAR of pair {k}"
    return g, gn


def _ops_ref(case, name, fn):
    return helpers.ops_ref(*case, name, fn)


@pytest.mark.parametrize("case", [OPS_EDGES_N, OPS_EDGES_ODD, OPS_FLAG, OPS_FLAG_N], ids=lambda c: c[0] + "-" + c[1].decode())
def test_ops_local_and_second_best(engine, case):
    c = helpers.ops_case(*case)
    for sc in SCORES:
        ref = _ops_ref(case, ("local2", sc), lambda c: I.local(c["ob"], *sc, second=True))
        kw = dict(algo=G.LOCAL, **_kw(sc))
        _ops_plan(kw, c, "wavefront16_local")
        _ops_run(engine, c, kw, ref, END_FIELDS, f"LOCAL ops {case} {sc}")
        kw["second_best"] = 1
        _ops_plan(kw, c, "local16_second")
        _ops_run(engine, c, kw, ref, END_FIELDS + ("score2", "q_end2", "t_end2"), f"LOCAL second ops {case} {sc}")


@pytest.mark.parametrize("case", [OPS_EDGES_N, OPS_EDGES_ODD, OPS_FLAG, OPS_FLAG_N], ids=lambda c: c[0] + "-" + c[1].decode())
def test_ops_global(engine, case):
    c = helpers.ops_case(*case)
    for sc in SCORES:
        kw = dict(algo=G.GLOBAL, **_kw(sc))
        _ops_plan(kw, c, "wavefront16_global_G")
        ref = _ops_ref(case, ("global", sc), lambda c: I.global_(c["ob"], *sc))
        _ops_run(engine, c, kw, ref, ("score",), f"GLOBAL ops {case} {sc}")


@pytest.mark.parametrize("head,tail", [(G.TARGET, G.TARGET), (G.NONE, G.TARGET), (G.QUERY, G.QUERY), (G.TARGET, G.QUERY),
                                       (G.TARGET, G.BOTH), (G.NONE, G.BOTH), (G.TARGET, G.NONE), (G.QUERY, G.NONE)])
def test_ops_semiglobal(engine, head, tail):
    """SEMI_GLOBAL (the kernel runs transposed: the op-transformed target is the lanes' side).
    Tail NONE is the constant answer: ops must neither change it nor fault."""
    for case in (OPS_EDGES_N, OPS_FLAG):
        c = helpers.ops_case(*case)
        for sc in SCORES:
            kw = dict(algo=G.SEMI_GLOBAL, head=head, tail=tail, **_kw(sc))
            _ops_plan(kw, c, *SEMI_FAMILY[tail])
            ref = _ops_ref(case, ("semi", head, tail, sc), lambda c: I.semi(c["ob"], head, tail, *sc))
            g, gn = _ops_run(engine, c, kw, ref, END_FIELDS, f"SEMI ops {head}/{tail} {case} {sc}")
            if tail == G.NONE:
                _exact(g, gn, G.OUT_FIELDS, "SEMI tail NONE with ops against no ops")


@pytest.mark.parametrize("head", [G.TARGET, G.NONE])
def test_ops_semiglobal_with_start(engine, head):
    """SEMI_GLOBAL WITH_START, tail TARGET: score and ends against independent.semi on the
    transformed batch; independent has no model of the SEMI reverse pass, so the two start
    fields are held against the oracle run with the same ops."""
    for case in (OPS_EDGES_N, OPS_FLAG):
        c = helpers.ops_case(*case)
        for sc in SCORES:
            kw = dict(algo=G.SEMI_GLOBAL, head=head, tail=G.TARGET, start_pos=G.WITH_START, **_kw(sc))
            _ops_plan(kw, c, "wavefront16_semi_start")
            ref = _ops_ref(case, ("semi", head, G.TARGET, sc), lambda c: I.semi(c["ob"], head, G.TARGET, *sc))
            g, _ = _ops_run(engine, c, kw, ref, END_FIELDS, f"SEMI WITH_START ops {head} {case} {sc}")
            _exact(g, O.align(c["b"], O.make_params(**kw), q_ops=c["qo"], t_ops=c["to"]), ("q_start", "t_start"),
                   f"SEMI WITH_START ops {head} {case} {sc} (oracle)")


@pytest.mark.parametrize("k_band", [4, 16])
def test_ops_banded(engine, k_band):
    for case in (OPS_EDGES_N, OPS_FLAG):
        c = helpers.ops_case(*case)
        for sc in SCORES:
            kw = dict(algo=G.BANDED, k_band=k_band, **_kw(sc))
            _ops_plan(kw, c, "banded16")
            ref = _ops_ref(case, ("banded", k_band, sc), lambda c: I.banded(c["ob"], k_band, *sc))
            _ops_run(engine, c, kw, ref, END_FIELDS, f"BANDED {k_band} ops {case} {sc}")


_CODE_LETTER = bytes(b"NANCTNNGNNNNNNNN")        # 1 A, 3 C, 4 T, 7 G; anything else stands as N


def _ops_seeds(n):
    return np.random.default_rng(0x5EED).integers(0, 41, n).astype(np.uint32)


@pytest.mark.parametrize("form,env", [("ksw16_64", {}), ("level0_lds", {"GASALX_KSW16": "0"})])
def test_ops_ksw(engine, monkeypatch, form, env):
    """KSW with ops on the 16-bit form and on the generic form, forced as test_ksw forces them.
    ksw16 takes a pair by its *op-transformed* query (A/C/G/T only): a reversed query whose
    length is no multiple of 8 begins with pads and stays with the generic kernel, so the
    routing is asserted from the transformed codes."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = ("edges", b"ACGT")
    c = helpers.ops_case(*case)
    b, ob = c["b"], c["ob"]
    seed = _ops_seeds(b.n)
    letters = lambda data, offs, lens: [bytes(data[int(o):int(o) + int(n)]).translate(_CODE_LETTER + bytes(240))
                                        for o, n in zip(offs, lens)]
    for sc in SCORES:
        kw = dict(algo=G.KSW, **_kw(sc))
        assert G.describe_plan(G.make_params(**kw), int(b.q_lens.max()), int(b.t_lens.max())) == "generic_ksw"
        r = helpers.ksw_routing(letters(ob.q_data, ob.q_offsets, ob.q_lens), letters(ob.t_data, ob.t_offsets, ob.t_lens),
                                seed, sc, env)
        if form == "ksw16_64":
            assert r["inst"] == 64 and b.n // 4 <= r["taken"].sum() < b.n, int(r["taken"].sum())
            assert r["taken"][(c["qo"] != 0) | (c["to"] != 0)].sum() >= b.n // 8
        else:
            assert not r["taken"].any() and (r["level"] == 0).all() and r["tpb"] == 256
        ref = _ops_ref(case, ("ksw", sc), lambda c: I.ksw(c["ob"], seed, *sc))
        _ops_run(engine, c, kw, ref, END_FIELDS, f"KSW {form} ops {sc}", seed_scores=seed)


@pytest.mark.parametrize("case", [OPS_EDGES_N, OPS_EDGES_ODD, OPS_FLAG, OPS_FLAG_N], ids=lambda c: c[0] + "-" + c[1].decode())
def test_ops_local_with_start(engine, case):
    """The WITH_START reverse pass: reversed loads of packed words that the op already reversed."""
    c = helpers.ops_case(*case)
    for sc in SCORES:
        kw = dict(algo=G.LOCAL, start_pos=G.WITH_START, **_kw(sc))
        _ops_plan(kw, c, "wavefront16_local_start")
        fwd = _ops_ref(case, ("local2", sc), lambda c: I.local(c["ob"], *sc, second=True))
        st = _ops_ref(case, ("local_start", sc), lambda c: I.local_start(c["ob"], *sc, fwd=fwd))
        ref = dict(fwd, **st)
        _ops_run(engine, c, kw, ref, END_FIELDS + ("q_start", "t_start"), f"LOCAL WITH_START ops {case} {sc}")


@pytest.mark.parametrize("case", [OPS_EDGES_N, OPS_EDGES_ODD, OPS_FLAG], ids=lambda c: c[0] + "-" + c[1].decode())
def test_ops_global_tb_replay(engine, case):
    """GLOBAL + traceback with ops: the GPU's CIGARs replayed over the op-transformed slots
    (independent.replay_global_slots: the walk starts at the pad cell, whose codes are real
    bases after a reverse), the score against independent.global_()."""
    c = helpers.ops_case(*case)
    b = c["b"]
    for sc in SCORES:
        kw = dict(algo=G.GLOBAL, start_pos=G.WITH_TB, **_kw(sc))
        _ops_plan(kw, c, "wavefront16_global_tb")
        ref = _ops_ref(case, ("global", sc), lambda c: I.global_(c["ob"], *sc))
        g, _ = _ops_run(engine, c, kw, ref, ("score",), f"GLOBAL+TB ops {case} {sc}", tb=True)
        keep = helpers.cigar_slots_kept(b.q_offsets, b.q_lens, g["n_ops"])
        assert 1 - keep.mean() <= 0.04
        st = I.replay_global_slots(c["ob"], g, sc, G.decode_cigar, keep)
        assert not st["failures"], (len(st["failures"]), st["failures"][:3])
        assert st["checked"] == keep.sum() and st["through"] >= keep.sum() // 2


@pytest.mark.parametrize("case,sc,family", [
    (OPS_EDGES_ODD, (1, 4, 6, 1), "wavefront16_local_tb"),
    (OPS_EDGES_N, (1, 4, 6, 1), "wavefront16_local_tb"),
    (OPS_FLAG, (1, 4, 6, 1), "wavefront16_local_tb"),
    (OPS_FLAG, (2, 3, 5, 2), "wavefront_local_tb_keys"),
], ids=["edges-odd", "edges-N", "flagship", "flagship-int32"])
def test_ops_local_tb_replay_and_rectangle(engine, case, sc, family):
    """LOCAL + traceback with ops: CIGAR replay over the transformed slots (lengths, M/X labels
    against the post-op codes, the moved pads included), path score == score ==
    independent.local(), and the rectangle from start to end worth `score` by global_textbook."""
    c = helpers.ops_case(*case)
    b = c["b"]
    kw = dict(algo=G.LOCAL, start_pos=G.WITH_TB, **_kw(sc))
    _ops_plan(kw, c, family)
    ref = _ops_ref(case, ("local2", sc), lambda c: I.local(c["ob"], *sc, second=True))
    g, _ = _ops_run(engine, c, kw, ref, END_FIELDS, f"LOCAL+TB ops {case} {sc}", tb=True)
    keep = helpers.cigar_slots_kept(b.q_offsets, b.q_lens, g["n_ops"])
    assert 1 - keep.mean() <= 0.02
    st = I.replay_batch(c["oq"], c["ot"], b, g, sc, I.LOCAL_MODE, G.decode_cigar, keep)
    assert not st["failures"], (len(st["failures"]), st["failures"][:3])
    assert st["stepped"] == 0 and st["checked"] >= keep.sum() * 9 // 10
    if case != OPS_EDGES_N:
        # the moved pads carry the N code: alignments that run into them are on the path
        assert st["n_path"] <= keep.sum() // 10


@pytest.mark.parametrize("algo", [G.LOCAL, G.GLOBAL, G.SEMI_GLOBAL])
def test_ops_int32_kernels(engine, monkeypatch, algo):
    """The int32 wavefront kernels (GASALX_PACKED16=0, read per call) on the packed workspace."""
    monkeypatch.setenv("GASALX_PACKED16", "0")
    for case in (OPS_EDGES_N, OPS_FLAG):
        c = helpers.ops_case(*case)
        for sc in SCORES:
            kw = dict(algo=algo, **_kw(sc))
            _ops_plan(kw, c, "wavefront_")
            if algo == G.LOCAL:
                ref = _ops_ref(case, ("local2", sc), lambda c: I.local(c["ob"], *sc, second=True))
            elif algo == G.GLOBAL:
                ref = _ops_ref(case, ("global", sc), lambda c: I.global_(c["ob"], *sc))
            else:
                ref = _ops_ref(case, ("semi", G.TARGET, G.TARGET, sc), lambda c: I.semi(c["ob"], G.TARGET, G.TARGET, *sc))
            _ops_run(engine, c, kw, ref, ("score",) if algo == G.GLOBAL else END_FIELDS, f"int32 {algo} ops {case} {sc}")


def test_ops_generic_thread_per_pair(engine):
    """One generic thread-per-pair plan: SEMI_GLOBAL with second_best = 1, its first-best
    fields against independent.semi."""
    case = OPS_EDGES_N
    c = helpers.ops_case(*case)
    for head, tail in ((G.TARGET, G.TARGET), (G.QUERY, G.BOTH)):
        for sc in SCORES:
            kw = dict(algo=G.SEMI_GLOBAL, head=head, tail=tail, second_best=1, **_kw(sc))
            _ops_plan(kw, c, "generic_semi")
            ref = _ops_ref(case, ("semi", head, tail, sc), lambda c: I.semi(c["ob"], head, tail, *sc))
            _ops_run(engine, c, kw, ref, END_FIELDS, f"generic SEMI ops {head}/{tail} {sc}")


def _pack_codes(codes):
    """4-bit codes, eight per word, first in bits 31:28, as the bytes of the words."""
    w = (codes.reshape(-1, 8).astype(np.uint32) << (28 - 4 * np.arange(8, dtype=np.uint32))).sum(axis=1, dtype=np.uint32)
    return w.view(np.uint8)


def test_ops_packed_input(engine):
    """is_packed = 1 together with ops: the input packed with orc_pack as test_packed_input
    does; scores and ends against independent on the ASCII batch.  With start_pos = WITH_TB
    and a CIGAR buffer the reference's packed buffer aliases the unpacked one, so the buffer
    begins with the op-transformed packed query words (SEMI_GLOBAL: no walk writes over them)."""
    import ctypes
    case = OPS_EDGES_N
    c = helpers.ops_case(*case)
    b, ob = c["b"], c["ob"]
    qd = np.zeros(b.q_bytes, np.uint8); td = np.zeros(b.t_bytes, np.uint8)
    pq = np.zeros(b.q_bytes // 8, np.uint32); pt = np.zeros(b.t_bytes // 8, np.uint32)
    O.lib().orc_pack(O._ptr(b.q_data), ctypes.c_uint32(b.q_bytes), O._ptr(pq))
    O.lib().orc_pack(O._ptr(b.t_data), ctypes.c_uint32(b.t_bytes), O._ptr(pt))
    qd[:b.q_bytes // 2] = pq.view(np.uint8); td[:b.t_bytes // 2] = pt.view(np.uint8)
    assert np.array_equal(qd[:b.q_bytes // 2], _pack_codes(b.q_data & 15))
    cp = dict(c, b=G.Batch(qd, b.q_offsets, b.q_lens, td, b.t_offsets, b.t_lens))
    sc = SCORES[0]
    kw = dict(algo=G.LOCAL, is_packed=1, **_kw(sc))
    _ops_plan(kw, c, "wavefront16_local")
    ref = _ops_ref(case, ("local2", sc), lambda c: I.local(c["ob"], *sc, second=True))
    _ops_run(engine, cp, kw, ref, END_FIELDS, "is_packed LOCAL ops")
    kw = dict(algo=G.GLOBAL, is_packed=1, **_kw(sc))
    _ops_run(engine, cp, kw, _ops_ref(case, ("global", sc), lambda c: I.global_(c["ob"], *sc)), ("score",), "is_packed GLOBAL ops")
    kw = dict(algo=G.SEMI_GLOBAL, start_pos=G.WITH_TB, is_packed=1, **_kw(sc))
    _ops_plan(kw, c, "wavefront_semi_keys_G")
    ref = _ops_ref(case, ("semi", G.TARGET, G.TARGET, sc), lambda c: I.semi(c["ob"], G.TARGET, G.TARGET, *sc))
    g = engine.align_host(cp["b"], G.make_params(**kw), q_ops=c["qo"], t_ops=c["to"])
    _exact(g, ref, END_FIELDS, "is_packed SEMI WITH_TB ops")
    want = _pack_codes(ob.q_data)
    assert not np.array_equal(want, qd[:b.q_bytes // 2])
    assert np.array_equal(g["cigar"][:b.q_bytes // 2], want), "the CIGAR buffer must begin with the op-transformed packed query"
    assert np.array_equal(g["cigar"][b.q_bytes // 2:], qd[b.q_bytes // 2:])
    assert np.array_equal(g["n_ops"], b.q_lens)

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

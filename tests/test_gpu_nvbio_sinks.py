"""GPU parity of the sink-tracking scoring path (gasalx_nv_score_sinks_*, nvbio_sink.hpp) through
the C ABI: scores and BestSink positions bit-exact against the plain-Python model of nvbio's
TextBlockingTag report order (tests/nvbio_sink_model.py, pinned by test_nvbio_sinks_ref.py).
Pattern lengths sit at the lane-group edges of the planned kernel (G lanes x R rows, read from
the plan name), text lengths at the stripe edges (8 columns for Gotoh, 16 for Smith-Waterman and
edit distance), and most inputs are built to tie: the rule (the last maximum in report order) is
only visible on ties.  The crossed-tie batches are the ones whose sink depends on the order itself
(test_nvbio_sinks_ref.py::test_inputs_tell_orders_apart counts on how many pairs)."""
import re

import numpy as np
import pytest

import gasal_ffi as G
import nvbio_sink_model as R

pytestmark = pytest.mark.gpu

CASES = [(b, t) for b in R.BASES for t in R.TYPES]
IDS = [f"{b}-{t}" for b, t in CASES]


def _shape(name):
    m = re.search(r"^nvbio(16)?_.*_G(\d+)R(\d+)_sink$", name)
    assert m, name
    return int(m.group(2)), int(m.group(3))


def _sink_plan(al, mp, mt, per_pair, text_bits, packed):
    """The sink call's own plan: the packed kernel inside its value window, else the int32 one --
    named as the score-only plan of the same bounds, with the "_sink" mark."""
    name = G.nv_describe_sinks_plan(al, mp, mt, per_pair_texts=per_pair, text_bits=text_bits)
    base = "ed" if al.aligner == G.NV_ED else "sw" if al.aligner == G.NV_SW else "gotoh"
    kind = {G.NV_GLOBAL: "global", G.NV_LOCAL: "local", G.NV_SEMI_GLOBAL: "semi"}[al.type]
    assert name.startswith(("nvbio16_" if packed else "nvbio_") + base + "_" + kind + ("_G" if per_pair else "_shared_G")), name
    assert name == G.nv_describe_plan(al, mp, mt, per_pair_texts=per_pair, text_bits=text_bits) + "_sink"
    return name


def _max_lens(pats, texts):
    return max(len(p) for p in pats), max(len(t) for t in texts)


def _compare(engine, al, pats, texts, P, T):
    sc, sk = engine.nv_score_sinks_host(al, P, T)
    rs, rk, n_max = R.batch(al, pats, texts)
    bad = np.nonzero((sc != rs) | (sk != rk).any(axis=1))[0]
    assert bad.size == 0, (f"{bad.size}/{len(sc)} differ, first #{bad[0]} (M={len(pats[bad[0]])}): gpu={sc[bad[0]]} "
                           f"{sk[bad[0]]} model={rs[bad[0]]} {rk[bad[0]]} {al}")
    # regression guard: the score-only entry point gives the same scores on the same inputs
    assert np.array_equal(engine.nv_score_host(al, P, T), sc)
    return n_max


def _tie_share(al, n_max):
    if al.type != G.NV_GLOBAL:
        share = float((n_max > 1).mean())
        assert share >= 0.5, share


@pytest.mark.parametrize("base,type_", CASES, ids=IDS)
def test_lane_group_and_stripe_edges(engine, base, type_):
    # per-pair texts; pattern lengths 1, 7, 8, 9, R, R + 1, G*R - 1, G*R of the planned shape
    # against text lengths 1, 7, 8, 9, 16, 17, 301 and the tie families of every pattern length
    al = R.aligner(base, type_)
    g, r = _shape(G.nv_describe_sinks_plan(al, 150, 340, per_pair_texts=True))
    lens = (1, 7, 8, 9, r, r + 1, g * r - 1, g * r)
    pats, texts, P, T = R.packed("edge", lens, 0xE0)
    mp, mt = _max_lens(pats, texts)
    assert mp == g * r
    # the call's own bounds plan the same shape: the lengths sit at this kernel's edges
    assert _shape(G.nv_describe_sinks_plan(al, mp, mt, per_pair_texts=True)) == (g, r)
    # 2-bit little-endian texts lie inside the packed kernel's value window: the sink call runs
    # the packed sink kernel
    _sink_plan(al, mp, mt, True, 2, packed=True)
    n_max = _compare(engine, al, pats, texts, P, T)
    _tie_share(al, n_max)
    # the same symbols as 4-bit big-endian texts: outside the packed window, the int32 sink kernel
    T4 = R.packed("edge", lens, 0xE0, 4, True)[3]
    _sink_plan(al, mp, mt, True, 4, packed=False)
    _compare(engine, al, pats, texts, P, T4)


@pytest.mark.parametrize("base,type_", CASES, ids=IDS)
def test_one_past_the_shape(engine, base, type_):
    # G*R + 1 rows no longer fit the shape: the next one runs, at its own R and R + 1 too
    al = R.aligner(base, type_)
    g, r = _shape(G.nv_describe_sinks_plan(al, 150, 340, per_pair_texts=True))
    g2, r2 = _shape(G.nv_describe_sinks_plan(al, g * r + 1, 340, per_pair_texts=True))
    assert g2 * r2 > g * r
    # fewer short texts here: against a long pattern they leave SEMI_GLOBAL untied (filler)
    pats, texts, P, T = R.packed("edge", (g * r + 1, r2, r2 + 1), 0xE1, text_lens=(9, 16, 301))
    mp, mt = _max_lens(pats, texts)
    assert _shape(_sink_plan(al, mp, mt, True, 2, packed=True)) == (g2, r2)
    _tie_share(al, _compare(engine, al, pats, texts, P, T))
    T4 = R.packed("edge", (g * r + 1, r2, r2 + 1), 0xE1, 4, True, text_lens=(9, 16, 301))[3]
    assert _shape(_sink_plan(al, mp, mt, True, 4, packed=False)) == (g2, r2)
    _compare(engine, al, pats, texts, P, T4)


@pytest.mark.parametrize("base,type_", CASES, ids=IDS)
def test_pattern_limit_1024(engine, base, type_):
    # the longest pattern: 64 lanes x 16 rows, every lane of the wave on one pair
    al = R.aligner(base, type_)
    rng = np.random.default_rng(0xE2)
    t = rng.integers(0, 4, 130).astype(np.uint32)
    p = np.concatenate([t, t, t, t, t, t, t, t])[:1024].astype(np.uint32)   # the text, repeated down the pattern
    pats = [p, np.array([2] * 1023, np.uint32), np.array([1, 3] * 8, np.uint32)]
    texts = [t, np.array([2] * 100, np.uint32), np.array([3, 1] * 20, np.uint32)]
    # both kernels at the limit: 2-bit texts take the packed one, 4-bit texts the int32 one
    P = G.PackedSet.pack(pats, 4, True)
    assert _shape(_sink_plan(al, 1024, 130, True, 2, packed=True)) == (64, 16)
    _compare(engine, al, pats, texts, P, G.PackedSet.pack(texts, 2, False))
    assert _shape(_sink_plan(al, 1024, 130, True, 4, packed=False)) == (64, 16)
    _compare(engine, al, pats, texts, P, G.PackedSet.pack(texts, 4, True))
    # a crossed pair at 2L = 1024: the maxima at (520, 1024) and (1040, 512), so the greatest row
    # (all ten row bits of the packed key, the largest M in the int32 key) against the later
    # stripe, whose index lies above the row bits
    pats, texts = [_CROSSED_1024[0]], [_CROSSED_1024[1]]
    P, T2, T4 = _pack_both(pats, texts)
    assert _shape(_sink_plan(al, 1024, 1041, True, 2, packed=True)) == (64, 16)
    _compare(engine, al, pats, texts, P, T2)
    assert _shape(_sink_plan(al, 1024, 1041, True, 4, packed=False)) == (64, 16)
    _compare(engine, al, pats, texts, P, T4)
    if type_ == "local" and base != "ed":
        assert R.pair(al, pats[0], texts[0]) == (2 * 512, 1040, 512, 2)


@pytest.mark.parametrize("base,type_", CASES, ids=IDS)
def test_shared_text(engine, base, type_):
    # one text for every pattern (sw-benchmark's layout), 2-bit little-endian and 4-bit big-endian
    al = R.aligner(base, type_)
    g, r = _shape(G.nv_describe_sinks_plan(al, 150, 301))
    lens = (1, 9, r, g * r)
    pats, texts, P, T = R.packed("shared", lens, 0xE3, n_text=301)
    assert _shape(_sink_plan(al, g * r, 301, False, 2, packed=True)) == (g, r)
    _tie_share(al, _compare(engine, al, pats, texts, P, T))
    T4 = R.packed("shared", lens, 0xE3, 4, True, n_text=301)[3]
    assert _shape(_sink_plan(al, g * r, 301, False, 4, packed=False)) == (g, r)
    _compare(engine, al, pats, texts, P, T4)


_CROSSED_1024 = R.crossed_pair(512, 520, 1040, 1041, np.random.default_rng(0xC9))


def _pack_both(pats, texts, shared=False):
    """(P, T2, T4): reads 4-bit big-endian; texts 2-bit little-endian (inside the packed kernel's
    window) and 4-bit big-endian (outside: the int32 kernel)."""
    return (G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, 2, False, shared=shared),
            G.PackedSet.pack(texts, 4, True, shared=shared))


@pytest.mark.parametrize("base,type_", CASES, ids=IDS)
def test_crossed_ties(engine, base, type_):
    # two equal maxima, one left and low, one right and high: which of them is the sink depends on
    # the stripe width, on the rows' place in the order and on first-or-last.  L = 3, R and R + 1
    # of the planned shape: the tied rows L - 1 and 2L - 1 on one lane, on two lanes, and across a
    # lane edge, where the lanes' (H << 32 | key) meet in the reduction.  Neighbouring pairs have
    # different winners (the two halves of a packed lane keep different keys) and the batch is odd
    al = R.aligner(base, type_)
    Ls = R.crossed_lens(al)
    r = Ls[1]
    pats, texts = R.crossed_batch(base, Ls)
    mp, mt = _max_lens(pats, texts)
    assert len(pats) % 2 == 1 and mp == 2 * (r + 1) and mt <= R.CROSS_MAX_TEXT
    P, T2, T4 = _pack_both(pats, texts)
    assert _shape(_sink_plan(al, mp, mt, True, 2, packed=True))[1] == r
    n_max = _compare(engine, al, pats, texts, P, T2)
    assert _shape(_sink_plan(al, mp, mt, True, 4, packed=False))[1] == r
    _compare(engine, al, pats, texts, P, T4)
    if type_ == "local" and base != "ed":
        assert (n_max > 1).mean() >= 0.8
    if type_ == "local" and base == "ed":     # every cell is 0: the last report, whatever the width
        sc, sk = engine.nv_score_sinks_host(al, P, T2)
        assert not sc.any() and [list(v) for v in sk] == [[len(t), len(p)] for p, t in zip(pats, texts)]
    # one shared text holding nested V and U copies, the patterns cut from it
    Ls = R.crossed_lens(al, per_pair=False)
    for L in Ls:
        for lead in R.CROSS_LEADS:
            pats, texts = R.crossed_shared(L, lead)
            P, T2, T4 = _pack_both(pats, texts, shared=True)
            assert _shape(_sink_plan(al, 2 * L, len(texts[0]), False, 2, packed=True))[1] == Ls[1]
            _compare(engine, al, pats, texts, P, T2)
            assert _shape(_sink_plan(al, 2 * L, len(texts[0]), False, 4, packed=False))[1] == Ls[1]
            _compare(engine, al, pats, texts, P, T4)


@pytest.mark.parametrize("al", [G.NvAligner(G.NV_SW, G.NV_LOCAL, 1, 2, 0, 0, 1, -1),
                                G.NvAligner(G.NV_GOTOH, G.NV_LOCAL, 1, -1, 1, 1),
                                G.NvAligner(G.NV_GOTOH, G.NV_SEMI_GLOBAL, 5, -4, -10, -1),
                                G.NvAligner(G.NV_GOTOH, G.NV_LOCAL, 5, -4, -10, -1)],
                         ids=["sw_positive", "gotoh_positive_gaps", "gotoh_b_semi", "gotoh_b_local"])
def test_other_schemes(engine, al):
    # schemes whose gaps or mismatches score > 0 (outside the packed window: int32, where pad rows
    # and columns would outscore real cells if the sink kernel did not mask them), and a second
    # Gotoh scheme inside it
    pats, texts, P, T = R.packed("edge", (1, 8, 9, 20), 0xE4)
    _sink_plan(al, *_max_lens(pats, texts), True, 2, packed=al.match == 5)
    _compare(engine, al, pats, texts, P, T)
    # the crossed batch: under the positive scores pad cells would outscore real ones, and the
    # real maxima tie in other cells than the builder's -- the model says which
    pats, texts = R.crossed_batch("sw" if al.aligner == G.NV_SW else "gotoh", R.crossed_lens(al))
    P, T2, _ = _pack_both(pats, texts)
    _sink_plan(al, *_max_lens(pats, texts), True, 2, packed=al.match == 5)
    _compare(engine, al, pats, texts, P, T2)


def test_null_outputs(engine):
    al = R.aligner("gotoh", "local")
    pats, texts, P, T = R.packed("edge", (1, 8, 9, 20), 0xE4)
    sc, sk = engine.nv_score_sinks_host(al, P, T)
    only_sc, none_sk = engine.nv_score_sinks_host(al, P, T, sinks=False)
    none_sc, only_sk = engine.nv_score_sinks_host(al, P, T, scores=False)
    assert none_sk is None and none_sc is None
    assert np.array_equal(only_sc, sc) and np.array_equal(only_sk, sk)
    with pytest.raises(RuntimeError, match="null argument"):
        engine.nv_score_sinks_host(al, P, T, scores=False, sinks=False)


def test_pairs_that_report_no_cell(engine):
    # the score path produces them: an empty text reports nothing, an empty pattern nothing under
    # LOCAL and the band initialisation H(-1, c) at y = 0 otherwise (nvbio_oracle.c:70-108)
    pats = [np.zeros(0, np.uint32), np.array([1, 2, 3], np.uint32), np.zeros(0, np.uint32), np.array([0, 1], np.uint32)]
    texts = [np.array([0, 1, 2, 3, 0, 1, 2, 3, 0], np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32),
             np.array([0, 1, 0, 1], np.uint32)]
    P, T = G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, 2, False)
    none = [R.INT32_MIN, R.NO_SINK, R.NO_SINK]
    for base, type_ in CASES:
        al = R.aligner(base, type_)
        _compare(engine, al, pats, texts, P, T)
        sc, sk = engine.nv_score_sinks_host(al, P, T)
        got = [[int(sc[k]), int(sk[k, 0]), int(sk[k, 1])] for k in range(4)]
        assert got[1] == none and got[2] == none, (base, type_, got)
        if type_ == "local":
            assert got[0] == none
        else:
            assert got[0][1:] == [9, 0]


@pytest.mark.parametrize("type_", list(R.TYPES))
def test_device_entry_point_agrees_with_host(engine, type_):
    import torch
    al = R.aligner("gotoh", type_)
    pats, texts, P, T = R.packed("edge", (1, 8, 9, 20), 0xE4)
    n = P.n
    sc, sk = engine.nv_score_sinks_host(al, P, T)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")
    keep = [dev(P.words), dev(P.offsets), dev(T.words), dev(T.offsets)]
    mk = lambda S, w, off: {"words": w.data_ptr(), "offsets": off.data_ptr(), "length": 0, "bits": S.bits,
                            "big_endian": S.big_endian}
    pat, txt = mk(P, keep[0], keep[1]), mk(T, keep[2], keep[3])
    mp, mt = _max_lens(pats, texts)
    for bounds in ((0, 0), (mp, mt)):          # lengths read back, and given
        dsc = torch.full((n,), -77, dtype=torch.int32, device="cuda:0")
        dsk = torch.full((2 * n,), -77, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        engine.nv_score_sinks_device_ptrs(al, n, pat, txt, dsc.data_ptr(), dsk.data_ptr(), *bounds)
        torch.cuda.synchronize()
        assert np.array_equal(dsc.cpu().numpy(), sc)
        assert np.array_equal(dsk.cpu().numpy().view(np.uint32).reshape(n, 2), sk)
    # one output only: the other stays untouched
    dsk = torch.full((2 * n,), -77, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    engine.nv_score_sinks_device_ptrs(al, n, pat, txt, 0, dsk.data_ptr(), mp, mt)
    torch.cuda.synchronize()
    assert np.array_equal(dsk.cpu().numpy().view(np.uint32).reshape(n, 2), sk)

"""The banded scorer's BestSink positions (gasalx_nv_banded_score_sinks_*), the parts that need no
GPU: the reference the GPU tests compare against (the oracle's banded score pass,
O.nv_banded_traceback's score and sink) checked by a second restatement written from the cited nvbio
lines (tests/nvbio_banded_sinks_model.py) on the GPU tests' own inputs; that those inputs hold tied
maxima, so an implementation that kept the first maximum could not pass; the kernel names the
describe call gives; and the exported symbols.

One pair by hand, SW (1, -1, -1, -1), band 3, pattern [0, 1], text [0, 1, 0, 1]:
  row 0 (q = 0), band slots read text 0, 1, 2 = 0, 1, 0:
    LOCAL  j=0: diag 0+1 = 1, top 0-1: h = 1 at (1, 1); j=1: diag -1, top -1, left 0: h = 0 at
           (2, 1); j=2: diag 0+1 = 1, left -1: h = 1 at (3, 1)
  row 1 (q = 1), slots read text 1, 2, 3 = 1, 0, 1:
    LOCAL  j=0: diag 1+1 = 2 at (2, 2); j=1: diag 0-1, top 1-1 = 0, left 2-1 = 1: h = 1 at (3, 2);
           j=2: diag 1+1 = 2, left 0: h = 2 at (4, 2)
  LOCAL: the maximum 2 is reported at (2, 2) and again at (4, 2); the last wins: (2, 4, 2).
  SEMI_GLOBAL runs the same rows unclamped: row 0 = [1, 0, 1], row 1 = [2, 1, 2];
  m = min(2 + 2, 4) - 1 = 3, so slots 0, 1, 2 are reported at (2, 2), (3, 2), (4, 2): (2, 4, 2).
  With the text cut to [0, 1, 0] m = 2: slots 0 and 1 only, and the band's last slot of row 1 reads
  255 past the text: row 1 = [2, 1, 0]; the answer is (2, 2, 2).
  GLOBAL starts from [0, -1, -2]: row 0 = [1, 0, -1] (j=2: diag -2+1, left 0-1), row 1 = [2, 1, 0]
  (j=2: diag -1+1, left 1-1); it reports slot 2 at (2 + 2, 2): (0, 4, 2)."""
import os

import numpy as np
import pytest

import gasal_ffi as G
import nvbio_banded_sinks_model as R
import oracle as O

GLOBAL, LOCAL, SEMI = G.NV_GLOBAL, G.NV_LOCAL, G.NV_SEMI_GLOBAL
TYPES = {"global": GLOBAL, "local": LOCAL, "semi": SEMI}
ALIGNERS = {"gotoh": G.NvAligner(G.NV_GOTOH, 0, 2, -1, -2, -1), "sw": G.NvAligner(G.NV_SW, 0, 2, -3, 0, 0, -2, -3),
            "ed": G.NvAligner(G.NV_ED, 0), "gotoh_b": G.NvAligner(G.NV_GOTOH, 0, 5, -4, -10, -1)}
BANDS = (2, 7, 8, 9, 15, 16, 17, 31, 32)
SEED = 0xBA5D
NEW_SYMBOLS = ("gasalx_nv_banded_score_sinks_device", "gasalx_nv_banded_score_sinks_host",
               "gasalx_nv_describe_banded_sinks_plan")


def al_of(base, type_):
    return G.NvAligner(base.aligner, type_, base.match, base.mismatch, base.gap_open, base.gap_ext, base.deletion,
                       base.insertion)


_inputs = {}


def inputs():
    """The GPU tests' pairs (R.tie_pairs), packed as the kernels' fast path takes them: 4-bit
    big-endian patterns (N among the symbols), 2-bit little-endian texts."""
    if not _inputs:
        pats, texts = R.tie_pairs(SEED, symbols=5)
        _inputs.update(pats=pats, texts=texts, P=G.PackedSet.pack(pats, 4, True), T=G.PackedSet.pack(texts, 2, False))
    return _inputs


@pytest.fixture(scope="module", autouse=True)
def _built():
    O.build()


def test_exports():
    # the feature's public surface: fails on a library without it
    for name in NEW_SYMBOLS:
        assert name in G.EXPORTS and hasattr(G.lib(), name), name
    for name in ("nv_banded_score_sinks_host", "nv_banded_score_sinks_device_ptrs"):
        assert hasattr(G.Engine, name), name
    assert hasattr(G, "nv_describe_banded_sinks_plan")


def test_hand_worked_pair():
    sw = G.NvAligner(G.NV_SW, 0, 1, -1, 0, 0, -1, -1)
    p, t = [np.array([0, 1])], [np.array([0, 1, 0, 1])]

    def one(type_, tx, pat=p, **kw):
        sc, sk = R.best_sinks(al_of(sw, type_), 3, pat, tx, **kw)
        return int(sc[0]), int(sk[0, 0]), int(sk[0, 1])

    assert one(LOCAL, t) == (2, 4, 2)
    assert one(LOCAL, t, keep_first=True) == (2, 2, 2)
    assert one(SEMI, t) == (2, 4, 2)
    assert one(SEMI, [np.array([0, 1, 0])]) == (2, 2, 2)
    assert one(GLOBAL, t) == (0, 4, 2)
    # a text shorter than its pattern; LOCAL with an empty pattern
    assert one(SEMI, [np.array([0])]) == (R.INT32_MIN, R.NO_SINK, R.NO_SINK)
    empty = [np.zeros(0, np.int64)]
    assert one(LOCAL, t, empty) == (R.INT32_MIN, R.NO_SINK, R.NO_SINK)
    # an empty pattern reports row zero: SEMI_GLOBAL m = min(B - 1, N) + 1 slots, all 0, the last at (2, 0)
    assert one(SEMI, t, empty) == (0, 2, 0)


def test_inputs_cover_the_edges():
    d = inputs()
    M = np.array([len(p) for p in d["pats"]])
    N = np.array([len(t) for t in d["texts"]])
    assert len(M) == 1500 and M.max() == 200 and (M == 0).sum() >= 10
    assert (N < M).sum() >= 50                                   # skipped pairs
    assert ((N >= M) & (N < M + 31)).sum() >= 200                # SEMI_GLOBAL's m clipped by the text at band 32
    assert any((p == 4).any() for p in d["pats"])                # N in patterns


@pytest.mark.parametrize("aname", list(ALIGNERS))
@pytest.mark.parametrize("tname", list(TYPES))
def test_model_agrees_with_the_oracle(aname, tname):
    """Score and sink of the oracle's banded score pass (what the GPU tests compare against) equal the
    second restatement's, on the GPU tests' inputs, at every band the GPU tests run; the score also
    equals O.nv_banded_score."""
    d = inputs()
    al = al_of(ALIGNERS[aname], TYPES[tname])
    for band in BANDS:
        o = O.nv_banded_traceback(al, band, d["P"], d["T"])
        ms, mk = R.best_sinks(al, band, d["pats"], d["texts"])
        bad = np.nonzero((o["score"] != ms) | (o["sink"] != mk).any(axis=1))[0]
        assert bad.size == 0, (f"band {band}: {bad.size} differ, first #{bad[0]}: oracle {o['score'][bad[0]]} "
                               f"{o['sink'][bad[0]]} model {ms[bad[0]]} {mk[bad[0]]}")
        assert np.array_equal(ms, O.nv_banded_score(al, band, d["P"], d["T"]))


@pytest.mark.parametrize("tname", ["local", "semi"])
def test_ties_are_present(tname):
    """Pairs whose first maximum in report order is not the last: an implementation keeping the first
    maximum (or any other) gets these wrong.  At least 50 at band 15 under every scheme."""
    d = inputs()
    for aname, base in ALIGNERS.items():
        al = al_of(base, TYPES[tname])
        _, last = R.best_sinks(al, 15, d["pats"], d["texts"])
        _, first = R.best_sinks(al, 15, d["pats"], d["texts"], keep_first=True)
        n_tied = int((first != last).any(axis=1).sum())
        print(f"{aname} {tname}: {n_tied} pairs with tied maxima")
        assert n_tied >= 50, (aname, n_tied)


def test_local_sinks_past_the_text():
    # LOCAL sinks whose x lies past the text's end are among the answers (cells reading 255)
    d = inputs()
    N = np.array([len(t) for t in d["texts"]])
    _, sk = R.best_sinks(al_of(ALIGNERS["gotoh"], LOCAL), 15, d["pats"], d["texts"])
    live = sk[:, 0] != R.NO_SINK
    assert (sk[live, 0].astype(np.int64) > N[live]).sum() >= 10


def _env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def test_describe_plan_names():
    g = ALIGNERS["gotoh"]
    name = G.nv_describe_banded_sinks_plan
    # 2-bit texts inside the 16-bit window: two pairs per lane
    assert name(al_of(g, LOCAL), 16, 150) == "nvbio_banded16_gotoh_local_b16_sink"
    assert name(al_of(g, LOCAL), 15, 150) == "nvbio_banded16_gotoh_local_b16_sink"
    assert name(al_of(g, GLOBAL), 7, 150) == "nvbio_banded16_gotoh_global_b8_sink"
    assert name(al_of(ALIGNERS["sw"], SEMI), 32, 150) == "nvbio_banded16_sw_semi_b32_sink"
    assert name(al_of(ALIGNERS["ed"], SEMI), 17, 150) == "nvbio_banded16_ed_semi_b32_sink"
    # 4- and 8-bit texts, a positive gap score, a window too small, the switch: the int32 kernel
    assert name(al_of(ALIGNERS["sw"], SEMI), 32, 150, text_bits=4) == "nvbio_banded_sw_semi_b32_sink"
    assert name(al_of(g, LOCAL), 16, 150, text_bits=8) == "nvbio_banded_gotoh_local_b16_sink"
    assert name(G.NvAligner(G.NV_GOTOH, LOCAL, 1, -1, 1, -1), 16, 150) == "nvbio_banded_gotoh_local_b16_sink"
    assert name(G.NvAligner(G.NV_SW, LOCAL, 1, -1, 0, 0, 1, -1), 16, 150) == "nvbio_banded_sw_local_b16_sink"
    assert name(al_of(ALIGNERS["gotoh_b"], LOCAL), 16, 1000) == "nvbio_banded_gotoh_local_b16_sink"
    assert name(al_of(g, LOCAL), 16, 0) == "nvbio_banded_gotoh_local_b16_sink"
    try:
        _env("GASALX_NVB16", "0")
        assert name(al_of(g, LOCAL), 16, 150) == "nvbio_banded_gotoh_local_b16_sink"
    finally:
        _env("GASALX_NVB16", None)
    for band in (1, 33):
        with pytest.raises(RuntimeError, match=r"\(-1\): .*band length must be 2\.\.32"):
            name(al_of(g, LOCAL), band, 150)
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad aligner"):
        name(G.NvAligner(3, LOCAL), 16, 150)

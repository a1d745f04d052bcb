"""CPU checks of the matrix-scored Gotoh path's definition (tests/nvbio_matrix_model.py) and of its
planner (gasalx_nv_describe_matrix_plan, which needs no GPU):
  1. with the table of S = p == t ? match : mismatch the model is nvbio_sink_model.pair, the model
     test_nvbio_sinks_ref.py pins to the C oracle;
  2. hand-worked pairs over an asymmetric table (t + p*n, not p + t*n);
  3. a second fill, written independently (numpy anti-diagonals, the report order as a sort key),
     agrees on seeded random pairs and tables;
  4. plan names."""
import re

import numpy as np
import pytest

import gasal_ffi as G
import nvbio_matrix_model as M
import nvbio_sink_model as R

TYPES = list(R.TYPES)


# ---- 1. the model against the sink model ----
def _edge_inputs():
    al = M.gotoh("local", R.GOTOH.gap_open, R.GOTOH.gap_ext)
    g, r = _shape(G.nv_describe_matrix_plan(al, 4, 150, 340, per_pair_texts=True, sinks=True))
    return R.packed("edge", M.edge_lens(g, r), M.EDGE_SEED)[:2]


def _shape(name):
    m = re.search(r"^nvbio_matrix_gotoh_(global|local|semi)(_shared)?_G(\d+)R(\d+)(_sink)?$", name)
    assert m, name
    return int(m.group(3)), int(m.group(4))


@pytest.mark.parametrize("type_", TYPES)
def test_simple_table_is_the_sink_model(type_):
    pats, texts = _edge_inputs()
    ref_al = R.aligner("gotoh", type_)
    al = M.gotoh(type_, ref_al.gap_open, ref_al.gap_ext)
    mat = M.simple_table(4, ref_al.match, ref_al.mismatch)
    got = M.batch(al, mat, 4, pats, texts)
    want = R.batch(ref_al, pats, texts)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # the tie-share condition of the GPU test, on its inputs: the tie rule must be visible
    if type_ != "global":
        assert M.tie_share(got[2]) >= 0.5


# ---- 2. hand-worked pairs ----
# n = 2, the table as mat[p][t] (C layout mat[t + p*n]):   t=0  t=1
#                                                    p=0     2    5
#                                                    p=1    -3    4
HAND = G.NvMatrix(np.array([[2, 5], [-3, 4]], np.int8))


def test_hand_local_asymmetric():
    """pattern [0], text [1]: S = mat[1 + 0*2] = 5; E and F come from zeros plus negative gaps, so
    H(0,0) = max(0, 5) = 5 at (x, y) = (1, 1)."""
    assert HAND.scores.reshape(-1)[1 + 0 * 2] == 5 and HAND.scores.reshape(-1)[0 + 1 * 2] == -3
    assert M.pair(M.gotoh("local", -5, -3), HAND, 2, [0], [1])[:3] == (5, 1, 1)


def test_hand_local_swapped():
    """pattern [1], text [0]: S = mat[0 + 1*2] = -3, so H(0,0) = max(0, -10, -10, -3) = 0; the one
    reported cell holds the maximum 0: BestSink (best <= h) takes it, (1, 1)."""
    assert M.pair(M.gotoh("local", -5, -3), HAND, 2, [1], [0])[:3] == (0, 1, 1)


def test_hand_global():
    """pattern [0, 1], text [1], Go = -5, Ge = -3.  Boundaries: H(-1,-1) = 0, H(-1,0) = -5,
    H(0,-1) = -5, H(1,-1) = -8.
      row 0: S = mat[p=0][t=1] = 5; F = H(-1,0) + Go = -10; E = H(0,-1) + Go = -10;
             H(0,0) = max(-10, -10, 0 + 5) = 5
      row 1: S = mat[1][1] = 4; F = max(F(0,0) + Ge = -13, H(0,0) + Go = 0) = 0; E = H(1,-1) + Go = -13;
             diagonal H(0,-1) + S = -1;  H(1,0) = 0
    GLOBAL reports H(M-1, N-1) = 0 at (1, 2).  (The transposed table would give -1.)"""
    assert M.pair(M.gotoh("global", -5, -3), HAND, 2, [0, 1], [1])[:3] == (0, 1, 2)


def test_hand_semi_global():
    """pattern [0], text [1, 0], Go = -5, Ge = -3.  H(-1,c) = 0, H(0,-1) = -5, E(0,-1) = -inf.
      c = 0: S = mat[0][1] = 5; F = 0 + Go = -5; E = -5 + Go = -10; H = max(-10, -5, 0 + 5) = 5
      c = 1: S = mat[0][0] = 2; F = -5; E = max(-10 + Ge, 5 + Go) = 0; H = max(0, -5, 0 + 2) = 2
    The last row's maximum: 5 at (1, 1).  (The transposed table would give 2 at (2, 1).)"""
    assert M.pair(M.gotoh("semi", -5, -3), HAND, 2, [0], [1, 0])[:3] == (5, 1, 1)


def test_clamp_reads_the_last_symbol():
    mat = M.random_table(5, 3)
    al = M.gotoh("local", -4, -2)
    assert M.pair(al, mat, 5, [1, 200, 7, 4], [9, 2, 5, 4, 0]) == M.pair(al, mat, 5, [1, 4, 4, 4], [4, 2, 4, 4, 0])


# ---- 3. a second fill: anti-diagonals in numpy, the report order as a sort key ----
def _second(type_, go, ge, S, p, t):
    """(score, x, y): cells (i, d - i) of anti-diagonal d at once, over arrays with the boundary
    row and column at index 0; S[p, t] the table as a 2-D array."""
    local, glob = type_ == "local", type_ == "global"
    n = S.shape[0]
    p, t = np.minimum(np.asarray(p, np.int64), n - 1), np.minimum(np.asarray(t, np.int64), n - 1)
    m, k = len(p), len(t)
    if k == 0 or (local and m == 0):
        return R.INT32_MIN, R.NO_SINK, R.NO_SINK
    neg = -(1 << 50)
    H = np.zeros((m + 1, k + 1), np.int64)
    E = np.full((m + 1, k + 1), neg, np.int64)
    F = np.full((m + 1, k + 1), neg, np.int64)
    if not local:
        H[1:, 0] = go + ge * np.arange(m)
    else:
        E[1:, 0] = 0
    if glob:
        H[0, 1:] = go + ge * np.arange(k)
    for d in range(m + k - 1):
        i = np.arange(max(0, d - k + 1), min(m - 1, d) + 1)
        c = d - i
        f = np.maximum(F[i, c + 1] + ge, H[i, c + 1] + go)
        e = np.maximum(E[i + 1, c] + ge, H[i + 1, c] + go)
        h = np.maximum(np.maximum(e, f), H[i, c] + S[p[i], t[c]])
        if local:
            h = np.maximum(h, 0)
        H[i + 1, c + 1], E[i + 1, c + 1], F[i + 1, c + 1] = h, e, f
    if glob:
        return int(H[m, k]), k, m
    if type_ == "semi":
        row = H[m, 1:]
        x = k - 1 - int(np.argmax(row[::-1]))        # the rightmost maximum
        return int(row[x]), x + 1, m
    body = H[1:, 1:]
    ii, cc = np.nonzero(body == body.max())
    last = np.lexsort((cc % 8, ii, cc // 8))[-1]      # the latest in (stripe, row, column in stripe)
    return int(body.max()), int(cc[last]) + 1, int(ii[last]) + 1


@pytest.mark.parametrize("type_", TYPES)
def test_second_fill_agrees(type_):
    rng = np.random.default_rng(0x5EC0 + TYPES.index(type_))
    for trial in range(120):
        n = int(rng.integers(2, 33))
        mat = G.NvMatrix(rng.integers(-9, 10, (n, n)).astype(np.int8))
        go, ge = -int(rng.integers(0, 12)), -int(rng.integers(0, 5))
        m, k = int(rng.integers(0 if trial % 10 == 0 else 1, 40)), int(rng.integers(0 if trial % 15 == 0 else 1, 60))
        hi = n + (3 if trial % 4 == 0 else 0)          # some symbols past the table: the clamp
        p, t = rng.integers(0, hi, m), rng.integers(0, hi, k)
        want = M.pair(M.gotoh(type_, go, ge), mat, n, p, t)[:3]
        assert _second(type_, go, ge, mat.scores.astype(np.int64), p, t) == want, (trial, n, go, ge, m, k)


def test_second_fill_agrees_on_ties():
    # small alphabets and flat tables tie often: the order, not only the score
    rng = np.random.default_rng(0x71E5)
    tied = 0
    for trial in range(120):
        mat = G.NvMatrix(rng.integers(0, 3, (2, 2)).astype(np.int8))
        p, t = rng.integers(0, 2, int(rng.integers(1, 12))), rng.integers(0, 2, int(rng.integers(1, 40)))
        for type_ in ("local", "semi"):
            want = M.pair(M.gotoh(type_, -2, -1), mat, 2, p, t)
            tied += want[3] > 1
            assert _second(type_, -2, -1, mat.scores.astype(np.int64), p, t) == want[:3], (trial, type_)
    assert tied >= 120


# ---- 4. plan names ----
PROT = M.gotoh("local", -5, -3)


def _name(al=PROT, n=24, mp=128, mt=1024, per_pair=True, sinks=False):
    return G.nv_describe_matrix_plan(al, n, mp, mt, per_pair_texts=per_pair, sinks=sinks)


def test_proteinsw_shape_plans():
    assert _name() == "nvbio_matrix_gotoh_local_G8R16"
    assert _name(sinks=True) == "nvbio_matrix_gotoh_local_G8R16_sink"
    assert _name(M.gotoh("global", -5, -3)) == "nvbio_matrix_gotoh_global_G8R16"
    assert _name(M.gotoh("semi", -5, -3), sinks=True) == "nvbio_matrix_gotoh_semi_G8R16_sink"


def test_shared_mark_and_shapes():
    assert _name(per_pair=False) == "nvbio_matrix_gotoh_local_shared_G8R16"
    assert _name(per_pair=False, sinks=True) == "nvbio_matrix_gotoh_local_shared_G8R16_sink"
    assert _name(mp=1) == "nvbio_matrix_gotoh_local_G8R8"
    assert _name(mp=129) == "nvbio_matrix_gotoh_local_G8R19"
    assert _name(mp=1024) == "nvbio_matrix_gotoh_local_G64R16"


def test_bounds_that_do_not_plan():
    assert _name(mp=1025) == "none"
    assert _name(mp=1025, per_pair=False, sinks=True) == "none"
    # the LDS budget: 160 KB = the 1 KB table + one byte per column (padded to 8) of every text slot;
    # 128 / G slots per block, so longer texts move to wider lane groups before they stop planning
    assert _name(mt=5088) == "nvbio_matrix_gotoh_local_G8R16"
    assert _name(mt=5089) == "nvbio_matrix_gotoh_local_G16R16"
    assert _name(mt=40704) == "nvbio_matrix_gotoh_local_G64R16"
    assert _name(mt=40705) == "none"
    assert _name(mt=162816, per_pair=False) == "nvbio_matrix_gotoh_local_shared_G8R16"
    assert _name(mt=162817, per_pair=False) == "none"


def test_describe_refuses_what_the_call_refuses():
    for aligner in (G.NV_SW, G.NV_ED):
        with pytest.raises(RuntimeError, match=r"\(-5\).*Gotoh"):
            _name(G.NvAligner(aligner, G.NV_LOCAL, 1, -1, -5, -3, -1, -1))
    for n in (0, 1, 33):
        with pytest.raises(RuntimeError, match=r"\(-1\).*2\.\.32"):
            _name(n=n)
    assert _name(n=2) == _name(n=32) == "nvbio_matrix_gotoh_local_G8R16"


def test_existing_plan_names_for_the_same_bounds():
    # the DNA planner is untouched: proteinsw's first two calls (SimpleGotohScheme(1, -1, -5, -3) over the
    # same 8-bit strings) keep their int32 kernel, and the packed kernel keeps its 2-bit cases
    al = G.NvAligner(G.NV_GOTOH, G.NV_LOCAL, 1, -1, -5, -3)
    assert G.nv_describe_plan(al, 128, 1024, per_pair_texts=True, text_bits=8) == "nvbio_gotoh_local_G8R16"
    assert G.nv_describe_sinks_plan(al, 128, 1024, per_pair_texts=True, text_bits=8) == "nvbio_gotoh_local_G8R16_sink"
    assert G.nv_describe_plan(al, 128, 1024, per_pair_texts=False, text_bits=2) == "nvbio16_gotoh_local_shared_G8R16"
    assert G.nv_describe_plan(al, 1025, 1024, per_pair_texts=True, text_bits=8) == "none"

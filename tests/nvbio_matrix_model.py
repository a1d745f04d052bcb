"""Plain-Python definition of the matrix-scored Gotoh call (gasalx_nv_matrix_score_*): nvbio's
GotohAligner over a scheme whose substitution(r_i, q_j, r, q, qq) reads a table, as the cell
update of NvB/nvbio/alignment/gotoh/gotoh_inl.h:1042 takes it (:534 in the banded-free striped
form): S(p, t) = mat[t + p * n] with t the text symbol and p the pattern symbol, both read as
n - 1 when they are >= n (the library's clamp; the reference indexes past its table there).

The fill is nvbio_sink_model.dp_matrix's Gotoh branch with that S and nothing else changed:
  F(i,c) = max(F(i-1,c) + Ge, H(i-1,c) + Go)     E(i,c) = max(E(i,c-1) + Ge, H(i,c-1) + Go)
  H(i,c) = max3(E, F, H(i-1,c-1) + S)             LOCAL: max(H, 0)
  H(i,-1) = LOCAL ? 0 : Go + Ge*i,  E(i,-1) = LOCAL ? 0 : -inf
  H(-1,c) = GLOBAL ? Go + Ge*c : 0,  F(-1,c) = -inf,  H(-1,-1) = 0
and the reports are replayed by nvbio_sink_model.best_sink (the TextBlockingTag order and
BestSink's `best <= h`), imported, not restated."""
import numpy as np

import gasal_ffi as G
import nvbio_sink_model as R

NEG = R.NEG


def flat(mat, n):
    """The table as the C ABI reads it: a list of n*n ints, entry [t + p*n]."""
    a = np.asarray(mat.scores if isinstance(mat, G.NvMatrix) else mat, np.int64).reshape(-1)
    assert a.size == n * n
    return [int(v) for v in a]


def dp_matrix(al, mat, n, p, t):
    """(top, H) as nvbio_sink_model.dp_matrix; mat: flat list, p / t: lists of ints (any value)."""
    local, glob = al.type == G.NV_LOCAL, al.type == G.NV_GLOBAL
    go, ge = al.gap_open, al.gap_ext
    M, N = len(p), len(t)
    p = [min(v, n - 1) for v in p]
    t = [min(v, n - 1) for v in t]
    top = [(go + ge * c) if glob else 0 for c in range(N)]
    left = [0 if local else go + ge * i for i in range(M)]
    H = []
    up, upF = top, [NEG] * N
    for i in range(M):
        row, rowF = [0] * N, [NEG] * N
        h_left = left[i]
        diag = left[i - 1] if i else 0
        e = 0 if local else NEG
        srow = mat[p[i] * n:(p[i] + 1) * n]      # S(p_i, .)
        for c in range(N):
            f = max(upF[c] + ge, up[c] + go)
            e = max(e + ge, h_left + go)
            rowF[c] = f
            h = max(e, f, diag + srow[t[c]])
            if local:
                h = max(h, 0)
            diag = up[c]
            row[c] = h_left = h
        H.append(row)
        up, upF = row, rowF
    return top, H


_cache = {}


def pair(al, mat, n, p, t):
    """(score, x, y, n_max) of one pair; cached on (type, gaps, table, strings)."""
    m = flat(mat, n)
    k = (al.type, al.gap_open, al.gap_ext, n, tuple(m), bytes(np.asarray(p, np.uint8)), bytes(np.asarray(t, np.uint8)))
    if k not in _cache:
        top, H = dp_matrix(al, m, n, [int(v) for v in p], [int(v) for v in t])
        _cache[k] = R.best_sink(al.type, top, H, len(t), R.stripe(al))   # a GotohAligner: stripes of 8
    return _cache[k]


def batch(al, mat, n, pats, texts):
    """scores int32[k], sinks uint32[k, 2], n_max int64[k]; texts: one per pattern, or one shared."""
    if len(texts) == 1 and len(pats) != 1:
        texts = list(texts) * len(pats)
    r = [pair(al, mat, n, p, t) for p, t in zip(pats, texts)]
    return (np.array([v[0] for v in r], np.int32), np.array([[v[1], v[2]] for v in r], np.uint32).reshape(-1, 2),
            np.array([v[3] for v in r], np.int64))


def simple_table(n, match, mismatch):
    """The table of S(p, t) = p == t ? match : mismatch."""
    a = np.full((n, n), mismatch, np.int8)
    np.fill_diagonal(a, match)
    return G.NvMatrix(a)


def random_table(n, seed, lo=-9, hi=9):
    """A seeded asymmetric table with entries in lo..hi."""
    return G.NvMatrix(np.random.default_rng(seed).integers(lo, hi + 1, (n, n)).astype(np.int8))


def gotoh(type_, gap_open, gap_ext):
    """The aligner of a matrix call: match / mismatch are not read (set to values no test's table holds)."""
    return G.NvAligner(G.NV_GOTOH, R.TYPES[type_] if isinstance(type_, str) else type_, 77, -77, gap_open, gap_ext)


EDGE_SEED = 0xE0   # test_gpu_nvbio_sinks.py's lane-group test: the same inputs


def edge_lens(g, r):
    return (1, 7, 8, 9, r, r + 1, g * r - 1, g * r)


def tie_share(n_max):
    """The share of pairs whose best score sits in more than one reported cell."""
    return float((np.asarray(n_max) > 1).mean())

"""The sink tests' reference (tests/nvbio_sink_model.py: a plain-Python DP and a literal replay of
nvbio's report order) pinned on the CPU: its scores against the C oracle's, its sinks against the
properties that define BestSink, and against the oracle's full-DP traceback where the two report
in the same order.  The entry points under test must exist: without them every test here fails."""
import numpy as np
import pytest

import gasal_ffi as G
import nvbio_sink_model as R
import oracle as O

CASES = [(b, t) for b in R.BASES for t in R.TYPES]
LENS = (1, 7, 8, 9, 19, 20, 33)


@pytest.fixture(scope="module", autouse=True)
def _built():
    O.build()
    # the feature's public surface: these tests pin its reference
    assert "gasalx_nv_score_sinks_host" in G.EXPORTS and hasattr(G.Engine, "nv_score_sinks_host")
    assert hasattr(G.lib(), "gasalx_nv_score_sinks_host") and hasattr(G.lib(), "gasalx_nv_describe_sinks_plan")


def _inputs():
    pats, texts, P, T = R.packed("edge", LENS, 0x51)
    # empty strings: the pairs that report no cell (or only the band initialisation)
    extra_p = [np.zeros(0, np.uint32), np.array([1, 2, 3], np.uint32), np.zeros(0, np.uint32)]
    extra_t = [np.array([0, 1, 2, 3, 0, 1, 2, 3, 0], np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32)]
    pats, texts = list(pats) + extra_p, list(texts) + extra_t
    return pats, texts, G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, 2, False)


@pytest.mark.parametrize("base,type_", CASES, ids=[f"{b}-{t}" for b, t in CASES])
def test_scores_equal_the_c_oracle(base, type_):
    al = R.aligner(base, type_)
    pats, texts, P, T = _inputs()
    sc, _, _ = R.batch(al, pats, texts)
    assert np.array_equal(sc, O.nv_score(al, P, T))


def test_scores_equal_the_c_oracle_shared_text():
    pats, texts = R.shared_batch((1, 8, 9, 20, 40), 70, 0x52)
    P = G.PackedSet.pack(pats, 4, True)
    T = G.PackedSet.pack(texts, 2, False, shared=True)
    for base, type_ in CASES:
        al = R.aligner(base, type_)
        assert np.array_equal(R.batch(al, pats, texts)[0], O.nv_score(al, P, T)), (base, type_)


def _later_in_report_order(M, N, x, y, w):
    """Mask [M, N] of the cells nvbio reports after (x, y) (one-based) in stripes of w columns: a
    later stripe, or the same stripe and a lower row, or the same row of the stripe and a column
    further right."""
    i, c = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    si, sc = y - 1, x - 1
    return (c // w > sc // w) | ((c // w == sc // w) & ((i > si) | ((i == si) & (c > sc))))


@pytest.mark.parametrize("base,type_", CASES, ids=[f"{b}-{t}" for b, t in CASES])
def test_sink_properties(base, type_):
    al = R.aligner(base, type_)
    pats, texts, _, _ = _inputs()
    for p, t in zip(pats, texts):
        M, N = len(p), len(t)
        score, x, y, n_max = R.pair(al, p, t)
        top, H = R.dp_matrix(al, [int(v) for v in p], [int(v) for v in t])
        if N == 0 or (M == 0 and al.type == G.NV_LOCAL):
            assert (score, x, y) == (R.INT32_MIN, R.NO_SINK, R.NO_SINK)
            continue
        if al.type == G.NV_GLOBAL:
            assert (x, y) == (N, M)
            assert score == (H[M - 1][N - 1] if M else top[N - 1])
            continue
        if M == 0:                       # SEMI_GLOBAL: the band initialisation, 0 in every column
            assert (score, x, y) == (0, N, 0)
            continue
        Hn = np.array(H, np.int64)
        assert Hn[y - 1, x - 1] == score
        if al.type == G.NV_SEMI_GLOBAL:
            assert y == M and score == Hn[M - 1].max() and not (Hn[M - 1, x:] >= score).any()
        else:
            assert score == Hn.max() and not (Hn[_later_in_report_order(M, N, x, y, R.stripe(al))] >= score).any()
            assert n_max == int((Hn == score).sum())


@pytest.mark.parametrize("base,type_", CASES, ids=[f"{b}-{t}" for b, t in CASES])
def test_sinks_against_the_traceback_oracle(base, type_):
    """orc_nv_traceback_batch restates nvbio's alignment_traceback, whose checkpoint pass is the
    PatternBlockingTag form (gotoh_inl.h:462-593, sw_inl.h:420-540): it reports LOCAL cells at
    (i + 1, block + j) per *pattern* stripe, then text position, then pattern column
    (gotoh_inl.h:575, :582; sw_inl.h:517, :524), so a tied LOCAL maximum may end elsewhere than
    under the TextBlockingTag order (gotoh_inl.h:1083, :1090).  LOCAL: untied pairs only.
    Both orders now take stripes of 16 for Smith-Waterman and edit distance, but one stripes the
    pattern and the other the text, so a tie may still end in another cell: the set that must
    agree is unchanged, the untied pairs (n_max counts cells, whatever the width).
    SEMI_GLOBAL (the last text position holding the row's maximum, utils_inl.h:273-300) and
    GLOBAL agree with the text-stripe order on every pair.  The traceback skips empty strings."""
    al = R.aligner(base, type_)
    pats, texts, P, T = _inputs()
    sc, sk, n_max = R.batch(al, pats, texts)
    tb = O.nv_traceback(al, P, T)
    keep = np.array([len(p) > 0 and len(t) > 0 for p, t in zip(pats, texts)])
    if al.type == G.NV_LOCAL:
        keep &= n_max == 1
        # edit distance scores 0 in every LOCAL cell: all of its pairs tie but the 1 x 1 ones
        assert keep.sum() >= (1 if base == "ed" else 5)
    assert np.array_equal(sc[keep], tb["score"][keep])
    assert np.array_equal(sk[keep], tb["sink"][keep])


def test_tie_share_of_the_inputs():
    # the rule is only visible on ties: at least half of the LOCAL and SEMI_GLOBAL pairs tie
    pats, texts, _, _ = R.packed("edge", LENS, 0x51)
    for base in R.BASES:
        for type_ in ("local", "semi"):
            n_max = R.batch(R.aligner(base, type_), pats, texts)[2]
            assert (n_max > 1).mean() >= 0.5, (base, type_, float((n_max > 1).mean()))


def test_stripe_widths():
    # gotoh_bandlen_selector 8 / DIM, sw_bandlen_selector 16 / DIM (edit distance takes it too), DIM = 1
    assert [R.stripe(R.BASES[b]) for b in ("gotoh", "sw", "ed")] == [8, 16, 16]


# Three crossed pairs worked out on paper, L = 2: the pattern is U + V = 0 1 + 2 3, the text
# 3^k 2 3 0 0 1 0 (V at columns k + 1, k + 2; U at k + 4, k + 5; N = k + 6).  Rows 1 and 2 (0, 1)
# score 0 left of column k + 3, since no text symbol there is theirs; row 3 (2) matches column k + 1
# alone, H(3, k + 1) = 2, and row 4 (3) continues it, H(4, k + 2) = 4; row 4 holds 2 in the columns
# <= k (a single match each, a gap from the one before gives 0).  Row 1 (0) matches columns k + 3 and
# k + 4 with H = 2 each (and k + 6), row 2 (1) continues the second, H(2, k + 5) = 4.  Every other
# cell lies below 4 under both schemes (Smith-Waterman 2, -3, gaps -2 and -3: at most 2; Gotoh 2, -1,
# -2, -1: at most 3, at (k + 6, 3) from the diagonal of H(2, k + 5) = 4), so the cells that tie are
#     H(4, k + 2) = 4  -- x = k + 2, y = 4, left and low --  and  H(2, k + 5) = 4  -- x = k + 5, y = 2.
# In one stripe row 4 is reported after row 2; in a later stripe column k + 5 is reported after
# every cell of the stripe of column k + 2.  Zero-based columns k + 1 and k + 4:
#   k = 1: columns 2 and 5, one stripe of 8 and of 16: (k + 2, 4) for both aligners
#   k = 5: columns 6 and 9, stripes 0 and 1 of 8, stripe 0 of 16: Gotoh (k + 5, 2), Smith-Waterman (k + 2, 4)
#   k = 13: columns 14 and 17, stripes 0 and 1 of 16 (1 and 2 of 8): (k + 5, 2) for both
# Edit distance, LOCAL: every cell is 0 and the last report is (N, M).
HAND = [  # k, Smith-Waterman (score, x, y), Gotoh, edit distance
    (1, (4, 3, 4), (4, 3, 4), (0, 7, 4)),
    (5, (4, 7, 4), (4, 10, 2), (0, 11, 4)),
    (13, (4, 18, 2), (4, 18, 2), (0, 19, 4)),
]


@pytest.mark.parametrize("k,sw,gotoh,ed", HAND, ids=["one_stripe_of_8", "8_boundary_inside_16", "16_boundary"])
def test_hand_worked_crossed_pairs(k, sw, gotoh, ed):
    p, t = [0, 1, 2, 3], [3] * k + [2, 3, 0, 0, 1, 0]
    assert len(t) <= 20
    for base, want in (("sw", sw), ("gotoh", gotoh), ("ed", ed)):
        score, x, y, n_max = R.pair(R.aligner(base, "local"), p, t)
        assert (score, x, y) == want, (base, k)
        assert n_max == (2 if base != "ed" else 4 * len(t)), (base, k)
    if k == 5:
        assert sw != gotoh           # the pair that tells the two selectors apart


def _rivals(al):
    """The report orders nvbio does not have: (width, first)."""
    w = R.stripe(al)
    return [(v, False) for v in (1, 4, 8, 16, 32, R.ROW_MAJOR) if v != w] + [(w, True)]


def _differing(al, pats, texts, width, first):
    if len(texts) == 1:
        texts = list(texts) * len(pats)
    return sum(R.rival(al, p, t, width, first)[:3] != R.pair(al, p, t)[:3] for p, t in zip(pats, texts))


@pytest.mark.parametrize("base", list(R.BASES))
def test_inputs_tell_orders_apart(base):
    """The crossed-tie batches of test_gpu_nvbio_sinks.py::test_crossed_ties, before any kernel
    runs: a kernel that reported in another order would give another sink on at least 8 pairs.
    Counts of the per-pair batch at L = 3, 8, 9 (133 pairs, all tied), pairs whose sink differs
    from nvbio's order:
      Smith-Waterman (16): width 1: 48, 4: 45, 8: 36, 32: 37, row-major: 73, first maximum: 133
      Gotoh (8):           width 1: 12, 4: 9, 16: 37, 32: 73, row-major: 109, first maximum: 133
    SEMI_GLOBAL, first against last on the last row: sw 133, ed 133, gotoh 65."""
    semi = R.aligner(base, "semi")
    pats, texts = R.crossed_batch(base, R.crossed_lens(semi))
    assert max(len(t) for t in texts) <= R.CROSS_MAX_TEXT
    n = _differing(semi, pats, texts, R.stripe(semi), True)
    print(base, "semi first-against-last", n, "of", len(pats))
    assert n >= 8
    al = R.aligner(base, "local")
    pats, texts = R.crossed_batch(base, R.crossed_lens(al))
    assert len(pats) % 2 == 1
    shared = [R.crossed_shared(L, lead) for L in R.crossed_lens(al, per_pair=False) for lead in R.CROSS_LEADS]
    if base == "ed":
        # match 0, clamp at 0, boundaries 0: every LOCAL cell is 0 and the last report is (N, M)
        # under every width; no order to tell apart
        for p, t in list(zip(pats, texts)) + [(p, ts[0]) for ps, ts in shared for p in ps]:
            assert R.pair(al, p, t)[:3] == (0, len(t), len(p))
            assert all(R.rival(al, p, t, w, False)[:3] == (0, len(t), len(p)) for w, _ in _rivals(al))
        return
    n_max = R.batch(al, pats, texts)[2]
    print(base, "local tie share", float((n_max > 1).mean()))
    assert (n_max > 1).mean() >= 0.8
    for width, first in _rivals(al):
        n = _differing(al, pats, texts, width, first)
        print(base, "local width", width or "row-major", "first" if first else "last", n, "of", len(pats))
        assert n >= 8, (width, first, n)
    # one shared text: nested copies, so a pattern's two columns lie 2 j (L + 1) + L + 1 apart and
    # all but the innermost are split by every width; every pair ties, and the row-major order
    # and the first maximum differ on at least 8 pairs over the texts
    assert all(R.pair(al, p, ts[0])[3] == 2 for ps, ts in shared for p in ps)
    for width, first in _rivals(al):
        n = sum(_differing(al, ps, ts, width, first) for ps, ts in shared)
        print(base, "local shared width", width or "row-major", "first" if first else "last", n)
        if first or width == R.ROW_MAJOR:
            assert n >= 8, (width, first, n)


def test_header_reaches_the_sinks_entry_point():
    # tools/nvbio_sinks_header_check (built by the tools Makefile): include/nvbio_batched.h against
    # stubs of the C API, host only -- set_sinks() reaches gasalx_nv_score_sinks_device, the same
    # enact without sinks makes the score-only call unchanged
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "nvbio_sinks_header_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_set_sinks_on_a_pattern_blocking_aligner_does_not_compile(tmp_path):
    # the same source with CHECK_PATTERN_TAG_REFUSED calls set_sinks() on a PatternBlockingTag
    # stream: the static_assert of include/nvbio_batched.h must stop the build, with its message
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-I", os.path.join(root, "include"), "-c",
           os.path.join(root, "tools", "nvbio_sinks_header_check.cpp"), "-o", str(tmp_path / "check.o")]
    subprocess.run(cmd, check=True, capture_output=True)             # as it stands: compiles
    r = subprocess.run(cmd + ["-DCHECK_PATTERN_TAG_REFUSED"], capture_output=True, text=True)
    assert r.returncode != 0
    assert "static assertion failed" in r.stderr and "TextBlockingTag aligners only" in r.stderr, r.stderr

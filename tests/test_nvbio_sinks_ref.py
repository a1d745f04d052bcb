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


def _later_in_report_order(M, N, x, y):
    """Mask [M, N] of the cells nvbio reports after (x, y) (one-based): a later stripe, or the same
    stripe and a lower row, or the same row of the stripe and a column further right."""
    i, c = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    si, sc = y - 1, x - 1
    return (c // 8 > sc // 8) | ((c // 8 == sc // 8) & ((i > si) | ((i == si) & (c > sc))))


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
            assert score == Hn.max() and not (Hn[_later_in_report_order(M, N, x, y)] >= score).any()
            assert n_max == int((Hn == score).sum())


@pytest.mark.parametrize("base,type_", CASES, ids=[f"{b}-{t}" for b, t in CASES])
def test_sinks_against_the_traceback_oracle(base, type_):
    """orc_nv_traceback_batch restates nvbio's alignment_traceback, whose checkpoint pass is the
    PatternBlockingTag form (gotoh_inl.h:462-593, sw_inl.h:420-540): it reports LOCAL cells at
    (i + 1, block + j) per *pattern* stripe, then text position, then pattern column
    (gotoh_inl.h:575, :582; sw_inl.h:517, :524), so a tied LOCAL maximum may end elsewhere than
    under the TextBlockingTag order (gotoh_inl.h:1083, :1090).  LOCAL: untied pairs only.
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

"""The Myers tests' reference (tests/nvbio_myers_model.py, a cited restatement of nvbio's
banded_myers<BAND_LEN, 0, TYPE, ALPHABET_SIZE>) pinned on the CPU by hand-worked cases, and measured
against the repository's banded edit-distance oracle (the DP a caller had to use before).  The entry
points under test must exist: without them every test here fails.

One case traced in full, band 4 (top bit 8), alphabet 4, pattern [2], text [1, 2, 0, 0, 0, 0]:
  last = min(N - 1, M) = 1.  Phase 1, column 0: B[2] = 8, Eq = B[1] = 0, so X = 0, D0 = 0 and
  dist = 0 - (1 - D0[3]) = -1; HN = 0, HP = ~VP = 0, VN = 0, VP = ~0.
  Phase 2 starts at s = 3 + 1 - 1 = 3.
  column 1: B[2] = 4, Eq = 4: X = 4, VP + 4 = 3 (mod 2^32), D0 = (3 ^ ~0) | 4 = ~3, HN = ~3, HP = 0;
            HN[3] = 1: dist = -1 + 1 = 0, reported at (2, 1); VN = 0, VP = ~3 | ~(~3 >> 1) = ~2.
  column 2: Eq = 0: D0 = 0, HN = 0, HP = ~VP = 2; s = 2, HP[2] = 0: dist = 0, reported at (3, 1);
            VN = 0, VP = ~2.
  column 3: the same column; s = 1, HP[1] = 1: dist = -1, reported at (4, 1).
  column 4: the same column; s = 0, HP[0] = 0: dist = -1, reported at (5, 1).  s = -1 ends the loop:
            text[5] is never read.
  SEMI_GLOBAL keeps the last maximum, 0 at (3, 1); GLOBAL reports dist = -1 at (N, M) = (6, 1).
The match at text column 2 is reported at x = 2 and again at x = 3, and the last maximum wins: these
are nvbio's Myers numbers and positions, not the banded DP's (which ends this pair at (2, 1)), which
is why the function has a kernel of its own."""
import numpy as np
import pytest

import gasal_ffi as G
import nvbio_myers_model as R
import oracle as O

SEMI, GLOBAL = G.NV_SEMI_GLOBAL, G.NV_GLOBAL
NONE = (R.INT32_MIN, R.NO_SINK, R.NO_SINK)


@pytest.fixture(scope="module", autouse=True)
def _built():
    O.build()
    # the feature's public surface: these tests pin its reference
    for name in ("gasalx_nv_banded_myers_device", "gasalx_nv_banded_myers_host", "gasalx_nv_describe_myers_plan"):
        assert name in G.EXPORTS and hasattr(G.lib(), name), name
    assert hasattr(G.Engine, "nv_banded_myers_host") and hasattr(G.Engine, "nv_banded_myers_device_ptrs")


# band 4, alphabet 4; (pattern, text, SEMI_GLOBAL result, GLOBAL result), results (score, x, y)
KATS = {
    # the case traced in the module docstring
    "one_symbol": ([2], [1, 2, 0, 0, 0, 0], (0, 3, 1), (-1, 6, 1)),
    # N == M == 1: last = min(0, 1) = 0, so no pattern symbol is ever loaded; the one phase-2 column
    # has Eq = 0, D0 = 0, HP = ~VP = 0, HN = 0: dist stays 0 whether the symbols match or not
    "text_equals_pattern_length_1": ([2], [2], (0, 1, 1), (0, 1, 1)),
    "text_equals_pattern_length_1_mismatch": ([2], [1], (0, 1, 1), (0, 1, 1)),
    # N == M: phase 1 runs M - 1 columns, phase 2 the single column M at s = band
    "text_equals_pattern_length": ([0, 1, 2, 3], [0, 1, 2, 3], (0, 4, 4), (0, 4, 4)),
    # an exact match from text column 1: phase 1 keeps dist = 0 down the diagonal, column M is not
    # reported (phase 1 reports nothing); the first report is column M + 1
    "exact_match": ([0, 1, 2, 3], [0, 1, 2, 3, 0], (0, 5, 4), (0, 5, 4)),
    # the same with the text running on: phase 2 ends when s reaches -1, after band columns
    # (5 .. 8), so GLOBAL's dist is the one of column 8 and text[8], text[9] are never read
    "exact_match_long_text": ([0, 1, 2, 3], [0, 1, 2, 3, 0, 0, 0, 0, 0, 0], (0, 5, 4), (-3, 10, 4)),
    # the match one column to the right
    "exact_match_shifted": ([0, 1, 2, 3], [3, 0, 1, 2, 3, 1], (0, 6, 4), (0, 6, 4)),
    "one_substitution": ([0, 1, 2, 3], [3, 0, 1, 1, 3, 1], (-1, 6, 4), (-1, 6, 4)),
    # the pattern holds a symbol the text lacks
    "one_insertion": ([0, 1, 2, 2, 3], [3, 0, 1, 2, 3, 1, 1], (-1, 6, 5), (-2, 7, 5)),
    # the text holds a symbol the pattern lacks
    "one_deletion": ([0, 1, 3], [3, 0, 1, 2, 3, 1], (-1, 6, 3), (-1, 6, 3)),
    "two_symbols": ([0, 1], [1, 0, 1, 1], (0, 4, 2), (0, 4, 2)),
    "six_symbols": ([0, 1, 2, 3, 0, 1], [2, 0, 1, 2, 3, 0, 1, 2, 2], (0, 8, 6), (-1, 9, 6)),
    # a text one shorter than its pattern is skipped (:245): nothing is reported
    "text_one_shorter": ([0, 1, 2, 3], [0, 1, 2], NONE, NONE),
}


@pytest.mark.parametrize("name", list(KATS))
def test_hand_worked_cases(name):
    p, t, semi, glob = KATS[name]
    assert R.banded_myers(SEMI, 4, 4, p, t) == semi
    assert R.banded_myers(GLOBAL, 4, 4, p, t) == glob


def test_alphabet_rules():
    # <2> masks with 1, <4> with 3 (:88, :127): 2 reads as 0 under <2>, 6 as 2 under <4>
    assert R.banded_myers(SEMI, 2, 4, [2, 1], [0, 1, 1]) == R.banded_myers(SEMI, 2, 4, [0, 1], [0, 1, 1])
    assert R.banded_myers(SEMI, 4, 4, [6, 1], [2, 1, 1]) == R.banded_myers(SEMI, 4, 4, [2, 1], [2, 1, 1])
    # <5>: a pattern symbol above 4 loads nothing (:170-174), a text symbol above 4 reads B[4] (:180-182)
    v = R.BitVectors(5)
    v.load(7, 8)
    assert v.B == [0, 0, 0, 0, 0]
    v.load(4, 8)
    assert v.get(9) == 8 and v.get(4) == 8 and v.get(3) == 0
    # so N in the text matches N in the pattern, and 7 in the text does too, but 7 in the pattern matches nothing
    assert R.banded_myers(SEMI, 5, 4, [0, 4, 2], [0, 7, 2, 0]) == R.banded_myers(SEMI, 5, 4, [0, 4, 2], [0, 4, 2, 0])
    assert R.banded_myers(SEMI, 5, 4, [0, 7, 2], [0, 7, 2, 0]) != R.banded_myers(SEMI, 5, 4, [0, 4, 2], [0, 4, 2, 0])


def test_band_32_shift_by_register_width():
    # N == M at band 32: s = 32, both report bits read as 0 (the model's docstring): dist stays
    # what phase 1 left, here 0 down an exact diagonal
    p = [0, 1, 2, 3, 0]
    assert R.banded_myers(SEMI, 4, 32, p, p) == (0, 5, 5)


def test_reads_the_packed_sets_the_api_takes():
    rng = np.random.default_rng(0x3A)
    seqs = [rng.integers(0, 4, n).astype(np.uint32) for n in (0, 1, 7, 8, 9, 16, 17, 33)]
    for bits in (2, 4, 8):
        for big in (False, True):
            S = G.PackedSet.pack(seqs, bits, big)
            for k, s in enumerate(seqs):
                assert np.array_equal(R.unpack(S, k), s)
            one = G.PackedSet.pack([seqs[-1]], bits, big, shared=True)
            assert np.array_equal(R.unpack(one), seqs[-1])


def _related_pairs(rng, n, m, band):
    """Reads cut from a text window with ~4% substitutions and an occasional one-symbol indel, the
    text running band symbols past the read (qmap's shape, scaled)."""
    pats, texts = [], []
    for _ in range(n):
        t = rng.integers(0, 4, m + band)
        st = int(rng.integers(0, band // 2 + 1))
        p = list(t[st:st + m])
        for k in range(len(p)):
            if rng.random() < 0.04:
                p[k] = int(rng.integers(0, 4))
        if rng.random() < 0.3:
            k = int(rng.integers(0, len(p)))
            if rng.random() < 0.5:
                del p[k]
            else:
                p.insert(k, int(rng.integers(0, 4)))
        pats.append(np.array(p, np.uint32))
        texts.append(t.astype(np.uint32))
    return pats, texts


@pytest.mark.parametrize("band", [7, 15, 31])
def test_agreement_with_the_banded_dp_oracle(band, capsys):
    """How often nvbio's Myers function and nvbio's banded edit-distance DP (the oracle's
    restatement of ed_banded_inl.h, what gasalx_nv_banded_score_* computes) give the same BestSink.
    A measurement: the shares are printed (profiles/nv_myers/README.md records them) and not
    asserted, because the two definitions differ on ordinary inputs.  The DP reports row M at the
    columns M .. M + band - 1 of its band; the Myers function reports nothing in phase 1, so never
    column M of a longer text, and its first report is (min(N - 1, M) + 1, M): an exact match at
    text column 1, pattern [0, 1, 2, 3] in text [0, 1, 2, 3, 0], ends at (4, 4) in the DP and at
    (5, 4) here, both with score 0.  On the related pairs below SEMI_GLOBAL scores agree and the
    sink's x is one greater; GLOBAL, reported at (N, M) after at most band phase-2 columns, rarely
    agrees at all.

    What both definitions state in so many words, and is asserted: a text shorter than its pattern
    is skipped before any cell is computed (myers_banded_inl.h:245-246; sw_banded_inl.h:365 for the
    DP), so both leave the BestSink untouched: INT32_MIN."""
    rng = np.random.default_rng(0xA9 + band)
    pats, texts = _related_pairs(rng, 200, 40, band)
    # every fifth text cut one short of its pattern: the skipped class
    for k in range(0, len(pats), 5):
        texts[k] = texts[k][:len(pats[k]) - 1]
    P, T = G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, 2, False)
    short = np.array([len(t) < len(p) for p, t in zip(pats, texts)])
    for type_, tn in ((SEMI, "semi"), (GLOBAL, "global")):
        al = G.NvAligner(G.NV_ED, type_)
        dp_score = O.nv_banded_score(al, band, P, T)
        dp_sink = O.nv_banded_traceback(al, band, P, T)["sink"]
        sc, sk = R.batch(type_, 4, band, P, T)
        assert (sc[short] == R.INT32_MIN).all() and (dp_score[short] == R.INT32_MIN).all()
        assert (sk[short] == R.NO_SINK).all()
        live = ~short
        same_score = sc[live] == dp_score[live]
        same_both = same_score & (sk[live] == dp_sink[live]).all(axis=1)
        with capsys.disabled():
            print(f"\nmyers vs banded DP, band {band} {tn}: {int(live.sum())} pairs, score equal "
                  f"{same_score.mean():.3f}, score and sink equal {same_both.mean():.3f}")

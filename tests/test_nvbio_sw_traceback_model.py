"""CPU checks of the Smith-Waterman / edit-distance traceback's second reference
(tests/nvbio_sw_traceback_model.py), no GPU:
  1. it reproduces every SW and ED CIGAR and score of tests/golden/nvbio_reference_kats.json;
  2. it is oracle.nv_traceback / oracle.nv_banded_traceback bit for bit on every input family;
  3. its pushes replay to the reported score, inside the band, GLOBAL over both strings;
  4. hand-worked pairs, one per rule, the cells in the docstrings;
  5. the tie families tie, the sink-tie family tells stripes of 16 from stripes of 8, and the pushes per
     pair cover every residue mod 4 (what the GPU tests rest on, counted on the model alone);
  6. empty strings: what the reference lines give, and where the front-end's contract differs."""
import json
import os

import numpy as np
import pytest

import gasal_ffi as G
import helpers
import nvbio_sw_traceback_model as S
import oracle as O

TYPES = list(S.TYPES)
# (scheme, type): every scheme under every type; the positive gap score under LOCAL only
CASES = [(s, t) for s in ("sym", "ed", "asym", "asym2") for t in TYPES] + [("positive", "local")]
TYPE_OF = {"GLOBAL": G.NV_GLOBAL, "LOCAL": G.NV_LOCAL, "SEMI_GLOBAL": G.NV_SEMI_GLOBAL}


def _kats():
    return json.load(open(os.path.join(helpers.GOLDEN, "nvbio_reference_kats.json")))


def _kat_aligner(c):
    s = c["scheme"]
    if c["aligner"] == "ed":
        return G.NvAligner(G.NV_ED, TYPE_OF[c["type"]])
    return G.NvAligner(G.NV_SW, TYPE_OF[c["type"]], match=s["match"], mismatch=s["mismatch"], deletion=s["deletion"],
                       insertion=s["insertion"])


# ---- 1. the reference's own vectors ----
def test_reference_cigars_and_scores():
    # alignment_test.cu:778-792 (SW x GLOBAL / LOCAL / SEMI_GLOBAL) and :828-904 (ED, 144 x 500)
    k = _kats()
    cases = [c for c in k["alignment"] + k["traceback_real"] if c["aligner"] in ("sw", "ed")]
    assert [c["aligner"] for c in cases] == ["sw", "sw", "sw", "ed"]
    for c in cases:
        p, t = G.dna_n_codes(c["pattern"]), G.ref2_codes(c["text"])
        r = S.full(_kat_aligner(c), p, t)
        assert r["score"] == c["score"], c["cigar"]
        assert O.nv_cigar_string(r["ops"], len(p), r["source"][1], r["sink"][1]) == c["cigar"]
        assert S.replay(_kat_aligner(c), p, t, r) == c["score"]


def test_reference_banded_edit_distance_scores():
    # alignment_test.cu:680-745: band 5, SEMI_GLOBAL edit distance
    cases = _kats()["edit_distance"]
    assert len(cases) == 6
    for c in cases:
        al = G.NvAligner(G.NV_ED, TYPE_OF[c["type"]])
        p, t = G.dna_n_codes(c["pattern"]), G.ref2_codes(c["text"])
        r = S.banded(al, c["band"], p, t)
        assert r["score"] == c["score"], c["test_id"]
        assert S.replay(al, p, t, r, c["band"]) == (c["score"], True)


# ---- 2. the model against the oracle ----
def _packed(name, pats, texts, shared=None):
    P = G.PackedSet.pack(pats, bits=4, big_endian=True)
    bits = S.text_bits(name)
    if shared is not None:
        return P, G.PackedSet.pack([shared], bits=bits, big_endian=False, shared=True)
    return P, G.PackedSet.pack(texts, bits=bits, big_endian=False)


@pytest.mark.parametrize("scheme,type_", CASES)
def test_full_is_the_oracle(scheme, type_):
    al = S.aligner(scheme, type_)
    for name, (pats, texts) in S.families().items():
        P, T = _packed(name, pats, texts)
        S.same(S.full_batch(al, pats, texts), O.nv_traceback(al, P, T), f"{name} {scheme} {type_}")
        shared = max(texts, key=len)                       # one shared text: the family's longest
        P, T = _packed(name, pats, texts, shared)
        S.same(S.full_batch(al, pats, [shared]), O.nv_traceback(al, P, T), f"{name} {scheme} {type_} shared")


@pytest.mark.parametrize("band", S.BANDS)
@pytest.mark.parametrize("scheme,type_", CASES)
def test_banded_is_the_oracle(scheme, type_, band):
    al = S.aligner(scheme, type_)
    for name, (pats, texts) in S.families(band).items():
        P, T = _packed(name, pats, texts)
        S.same(S.banded_batch(al, band, pats, texts), O.nv_banded_traceback(al, band, P, T),
               f"{name} {scheme} {type_} band {band}")
        shared = max(texts, key=len)                       # shorter than some patterns: those pairs are skipped
        P, T = _packed(name, pats, texts, shared)
        S.same(S.banded_batch(al, band, pats, [shared]), O.nv_banded_traceback(al, band, P, T),
               f"{name} {scheme} {type_} band {band} shared")


def test_unpack_is_the_packing():
    for bits, big in ((2, False), (4, True), (8, False)):
        seqs = [np.arange(k, dtype=np.uint32) % (1 << bits) for k in (0, 1, 7, 16, 17)]
        got = S.unpack(G.PackedSet.pack(seqs, bits=bits, big_endian=big))
        assert all(np.array_equal(a, b) for a, b in zip(got, seqs))
    one = S.unpack(G.PackedSet.pack([[3, 1, 2]], bits=2, big_endian=False, shared=True), 4)
    assert len(one) == 4 and list(one[3]) == [3, 1, 2]


# ---- 3. replay ----
@pytest.mark.parametrize("scheme,type_", CASES)
def test_replay_is_the_score(scheme, type_):
    al = S.aligner(scheme, type_)
    for name, (pats, texts) in S.families().items():
        res = S.full_batch(al, pats, texts)
        for k in range(len(pats)):
            if len(pats[k]) == 0 or len(texts[k]) == 0:
                assert res["score"][k] == S.INT32_MIN and len(res["ops"][k]) == 0
                continue
            r = S.one(res, k)
            assert S.replay(al, pats[k], texts[k], r) == r["score"], (name, k)
            if al.type == G.NV_GLOBAL:                     # both strings consumed
                assert r["source"] == (0, 0) and r["sink"] == (len(texts[k]), len(pats[k])), (name, k)
            if al.type == G.NV_SEMI_GLOBAL:                # the whole pattern
                assert r["source"][1] == 0 and r["sink"][1] == len(pats[k]), (name, k)
    for band in S.BANDS:
        for name, (pats, texts) in S.families(band).items():
            res = S.banded_batch(al, band, pats, texts)
            for k in range(len(pats)):
                r = S.one(res, k)
                if len(texts[k]) < len(pats[k]) or (al.type == G.NV_LOCAL and len(pats[k]) == 0):
                    assert r["score"] == S.INT32_MIN and r["sink"] == (S.NO_CELL,) * 2 and not r["ops"]
                    continue
                assert S.replay(al, pats[k], texts[k], r, band) == (r["score"], True), (name, band, k)
                if al.type != G.NV_LOCAL:
                    # the whole pattern; the band's GLOBAL corner is (M + B - 1, M) whatever the text length and
                    # its source stands on row -1 (no tails in the banded walk)
                    assert r["source"][1] == 0 and r["sink"][1] == len(pats[k]), (name, band, k)
                if al.type == G.NV_GLOBAL:
                    assert r["sink"][0] == len(pats[k]) + band - 1


# ---- 4. hand-worked pairs ----
def _sw(type_, match, mismatch, deletion, insertion):
    return G.NvAligner(G.NV_SW, S.TYPES[type_], match=match, mismatch=mismatch, deletion=deletion, insertion=insertion)


def _r(r):
    return r["score"], r["source"], r["sink"], r["ops"]


SYM = ("global", 2, -1, -1, -1)
M_, I_, D_ = S.SUB, S.INS, S.DEL


def test_hand_top_equals_left_above_the_diagonal():
    """Full DP, GLOBAL, match 2, mismatch -5, G = I = -1, pattern [0], text [1].  H(0,1) = I = -1, H(1,0) = G = -1.
      (1,1): top = H(0,1) + G = -2, left = H(1,0) + I = -2, diagonal = 0 - 5 = -5.
    sw_inl.h:497-499: top > left is false, so the second line decides: left > diagonal: INSERTION (with >= it
    would be the DELETION).  The walk pushes I and leaves the column; column 0 with one text row left: the
    first-column tail pushes D.
    The band (B = 3, text [1, 1, 1], rows = pattern): H(-1,-1..1) = 0, -1, -2.
      (0,0): diagonal = -5, top = H(-1,0) + G = -2: INSERTION (vertical), -2
      (0,1): diagonal = H(-1,0) - 5 = -6, top = H(-1,1) + G = -3, left = H(0,0) + I = -3: top > left false,
             left > diagonal: DELETION (horizontal), -3
      (0,2): diagonal = -7, left = -4: DELETION, -4
    GLOBAL reports (0, M+B-2) at (3, 1).  The walk: D, D, then I from (0,0) up to (-1,0): source (1, 0), which
    stands on H(-1,0) = -1: -1 + G (the pattern-only step) + 2 I = -4."""
    al = _sw("global", 2, -5, -1, -1)
    assert _r(S.full(al, [0], [1])) == (-2, (0, 0), (1, 1), [I_, D_])
    assert S.full(al, [0], [1])["ties"] == 1
    assert _r(S.banded(al, 3, [0], [1, 1, 1])) == (-4, (1, 0), (3, 1), [D_, D_, I_])
    assert S.banded(al, 3, [0], [1, 1, 1])["ties"] == 1
    assert S.replay(al, [0], [1, 1, 1], S.banded(al, 3, [0], [1, 1, 1]), 3) == (-4, True)


def test_hand_top_equals_the_diagonal_above_left():
    """Full DP, GLOBAL 2 / -1 / -1 / -1, pattern [0], text [0, 0].  H(0,1) = -1; H(1,0), H(2,0) = -1, -2.
      (1,1): top = -2, left = -2, diagonal = 0 + 2: SUBSTITUTION, 2
      (2,1): top = H(1,1) + G = 1, left = H(2,0) + I = -3, diagonal = H(1,0) + 2 = 1: top > left, but
             top > diagonal is false: SUBSTITUTION (with >= the DELETION, and the pushes D then M).
    The walk pushes M at (2,1) and stands in column 0 on row 1: the first-column tail pushes D."""
    al = _sw(*SYM)
    assert _r(S.full(al, [0], [0, 0])) == (1, (0, 0), (2, 1), [M_, D_])
    assert S.full(al, [0], [0, 0])["ties"] == 1


def test_hand_left_equals_the_diagonal_above_top():
    """Full DP, GLOBAL 2 / -1 / -1 / -1, pattern [0, 0], text [0].  H(0,1), H(0,2) = -1, -2; H(1,0) = -1.
      (1,1): diagonal = 2: SUBSTITUTION, 2
      (1,2): top = H(0,2) + G = -3, left = H(1,1) + I = 1, diagonal = H(0,1) + 2 = 1: top > left false,
             left > diagonal false: SUBSTITUTION (with >= the INSERTION, and the pushes I then M).
    The walk pushes M at (1,2) and stands on row 0 in column 1: the first-row tail pushes I."""
    al = _sw(*SYM)
    assert _r(S.full(al, [0, 0], [0])) == (1, (0, 0), (1, 2), [M_, I_])
    assert S.full(al, [0, 0], [0])["ties"] == 1


def test_hand_local_zero_cell_on_the_path():
    """LOCAL, match 2, mismatch -2, G = I = -3, pattern [0, 1, 2], text [0, 3, 2].
    Full DP (rows = text): (1,1) = 0 + 2 = 2; (2,2): diagonal = 2 - 2 = 0, top and left = -3: H = 0, stored as
    SINK (sw_inl.h:393-396); (3,3) = 0 + 2 = 2; every other cell 0.  Reports 2 at (1,1) and, later, at (3,3): the
    sink.  The walk pushes M at (3,3) and stops on the SINK at (2,2): source (2, 2).
    The band (B = 2, rows = pattern): (0,0) = 2; (1,1): diagonal = H(0,0) - 2 = 0, top = H(0,1) + G = -3: 0,
    SUBSTITUTION -- no SINK in the banded pass (sw_banded_inl.h:268-279); (2,2) = H(1,1) + 2 = 2, the last
    maximum ((2,3), past the text, is 0).  The walk pushes M three times, through the zero cell, to row -1."""
    al = _sw("local", 2, -2, -3, -3)
    p, t = [0, 1, 2], [0, 3, 2]
    assert _r(S.full(al, p, t)) == (2, (2, 2), (3, 3), [M_])
    assert _r(S.banded(al, 2, p, t)) == (2, (0, 0), (3, 3), [M_, M_, M_])
    assert S.replay(al, p, t, S.banded(al, 2, p, t), 2) == (2, True)       # 2, floor 0, 2


def test_hand_global_tails():
    """Full DP, GLOBAL 2 / -1 / -1 / -1.
    Pattern [0], text [1, 1, 0]: H(i,0) = -1, -2, -3; H(0,1) = -1.
      (1,1): top = -2, left = -2, diagonal = -1: M, -1;  (2,1): top = -2, left = -3, diagonal = H(1,0) - 1 = -2:
      top > diagonal false: M, -2;  (3,1): diagonal = H(2,0) + 2 = 0, top = -3, left = -4: M, 0.
    The walk pushes M at (3,1) and leaves the column on row 2: the first-column tail pushes D D (2 - 1 - 1 = 0).
    Pattern [1, 1, 0], text [0]: H(0,j) = -1, -2, -3; H(1,0) = -1.
      (1,1): M, -1;  (1,2): top = -3, left = -2, diagonal = H(0,1) - 1 = -2: M, -2;  (1,3): diagonal = H(0,2) + 2 = 0: M.
    The walk pushes M at (1,3) and leaves the row in column 2: the first-row tail pushes I I."""
    al = _sw(*SYM)
    assert _r(S.full(al, [0], [1, 1, 0])) == (0, (0, 0), (3, 1), [M_, D_, D_])
    assert _r(S.full(al, [1, 1, 0], [0])) == (0, (0, 0), (1, 3), [M_, I_, I_])


def test_hand_banded_sink_tie_in_the_last_row():
    """Band 3, SEMI_GLOBAL, edit distance, pattern [0].  Text [0, 0, 0]: every cell of row 0 is a match on its
    diagonal from row -1's zeros: (0,0) = (0,1) = (0,2) = 0.  m = min(M + B - 1, N) - (M - 1) = 3: the reports are
    0 at (1,1), (2,1), (3,1) and BestSink's <= keeps the last.  The walk pushes M from (0,2) to (-1,1): source
    (2, 0).  Text [0, 0]: m = 2, the entry past the text is not reported: sink (2, 1), source (1, 0)."""
    al = G.NvAligner(G.NV_ED, G.NV_SEMI_GLOBAL)
    assert _r(S.banded(al, 3, [0], [0, 0, 0])) == (0, (2, 0), (3, 1), [M_])
    assert _r(S.banded(al, 3, [0], [0, 0])) == (0, (1, 0), (2, 1), [M_])


def test_hand_local_sink_order_is_stripes_of_16():
    """Full DP, LOCAL 2 / -1 / -1 / -1, pattern u z v = [0,1,2,3] [0] [3,2,1,0] (M = 9), text v q u =
    [3,2,1,0] [3] [0,1,2,3].  v scores 8 at (4, 9) (text rows 1..4, pattern columns 6..9) and u scores 8 at
    (9, 4); no cell scores more: a longer diagonal would have to cross z or q.  Columns 4 and 9 lie in the
    same stripe of 16 (sw_inl.h:1330-1334), where rows come in order: (9, 4) is reported last.  Stripes of 8
    would report column 9 after every row of column 4 and keep (4, 9)."""
    al = _sw("local", 2, -1, -1, -1)
    p, t = [0, 1, 2, 3, 0, 3, 2, 1, 0], [3, 2, 1, 0, 3, 0, 1, 2, 3]
    assert _r(S.full(al, p, t)) == (8, (5, 0), (9, 4), [M_] * 4)
    assert _r(S.full(al, p, t, stripe=8)) == (8, (0, 5), (4, 9), [M_] * 4)


# ---- 5. what the families hold ----
@pytest.mark.parametrize("scheme", ["sym", "ed"])
@pytest.mark.parametrize("type_", TYPES)
def test_tie_families_tie(scheme, type_):
    # at least half of the pairs walk through a cell where a strict comparison decided
    al = S.aligner(scheme, type_)
    pats, texts = S.families()["ties"]
    share = S.tie_share(S.full_batch(al, pats, texts)["ties"])
    if scheme == "ed" and type_ == "local":
        # match 0: every cell of the LOCAL full DP is 0, hence SINK: no walk, nothing to tie (the band has no SINK)
        assert share == 0 and all(len(o) == 0 for o in S.full_batch(al, pats, texts)["ops"])
    else:
        assert share >= 0.5, share
    for band in S.BANDS:
        pats, texts = S.families(band)["ties"]
        share = S.tie_share(S.banded_batch(al, band, pats, texts)["ties"])
        assert share >= 0.5, (band, share)


def test_sink_tie_family_sees_the_stripe_width():
    pats, texts = S.families()["sink_ties"]
    for scheme in ("sym", "asym", "asym2"):
        al = S.aligner(scheme, "local")
        differ = sum(S.full(al, p, t)["sink"] != S.full(al, p, t, stripe=8)["sink"] for p, t in zip(pats, texts))
        assert differ >= len(pats) // 2, (scheme, differ)


def test_pushes_cover_every_residue_mod_4():
    # the kernels' walk stores single bytes up to a 4-byte boundary, then whole words
    for scheme, type_ in CASES:
        if scheme == "ed" and type_ == "local":
            continue
        al = S.aligner(scheme, type_)
        pats, texts = S.block(257)
        assert {len(o) % 4 for o in S.full_batch(al, pats, texts)["ops"]} == {0, 1, 2, 3}, (scheme, type_)
    for band in S.BANDS:
        pats, texts = S.block(257, band)
        for scheme, type_ in CASES:
            al = S.aligner(scheme, type_)
            assert {len(o) % 4 for o in S.banded_batch(al, band, pats, texts)["ops"]} == {0, 1, 2, 3}, (band, scheme, type_)


# ---- 6. empty strings ----
def test_empty_strings():
    for scheme, type_ in CASES:
        al = S.aligner(scheme, type_)
        for p, t in (([], [1, 2]), ([1, 2], []), ([], [])):
            assert _r(S.full(al, p, t)) == (S.INT32_MIN, (S.NO_CELL,) * 2, (S.NO_CELL,) * 2, [])
            P = G.PackedSet.pack([p]); T = G.PackedSet.pack([t], bits=2, big_endian=False)
            S.same(S.full_batch(al, [p], [t]), O.nv_traceback(al, P, T), "empty")
        g = S.scores(al)[2]
        for band in (2, 7, 32):
            # an empty pattern: row -1 is what the banded pass reports (sw_banded_inl.h:494-510)
            for t in ([], [1], [1, 2, 3] * 12):
                want = {G.NV_GLOBAL: ((band - 1) * g, (band - 1, 0), (band - 1, 0), []),
                        G.NV_SEMI_GLOBAL: (0, (min(band - 1, len(t)), 0), (min(band - 1, len(t)), 0), []),
                        G.NV_LOCAL: (S.INT32_MIN, (S.NO_CELL,) * 2, (S.NO_CELL,) * 2, [])}[al.type]
                assert _r(S.banded(al, band, [], t)) == want, (scheme, type_, band, len(t))
            assert _r(S.banded(al, band, [1, 2], [])) == (S.INT32_MIN, (S.NO_CELL,) * 2, (S.NO_CELL,) * 2, [])


def test_global_empty_text_is_where_the_front_end_differs():
    """nvbio's lines give a GLOBAL pair with an empty text its M insertions (the model's docstring); the
    front-end reports nothing for it, as DESIGN.md states.  Pinned here so that the difference is a stated one."""
    al = S.aligner("asym", "global")
    ref = S.reference_global_empty_text(al, 3)
    assert _r(ref) == (-9, (0, 0), (0, 3), [I_] * 3)
    assert S.replay(al, [0, 1, 2], [], ref) == -9
    assert S.full(al, [0, 1, 2], [])["score"] == S.INT32_MIN

"""CPU checks of the matrix-scored Gotoh traceback's definition (tests/nvbio_matrix_traceback_model.py)
and of its way up to the header (no GPU):
  1. under the table of S = p == t ? match : mismatch the model is oracle.nv_traceback, the C
     restatement the reference's CIGAR vectors pin (score, source, sink and every push);
  2. hand-worked pairs over a 2 x 2 asymmetric table, the cells in the docstrings;
  3. the tie family really ties: at least half of its pairs walk through a cell where the strict
     comparisons decide;
  4. replay: the pushes spell an alignment of exactly the reported spans and score, on every pair of
     every family the GPU tests run;
  5. include/nvbio_batched.h routes the matrix aligner to gasalx_nv_matrix_traceback_device, and the
     banded traceback still refuses it at compile time;
  6. the two entry points are exported."""
import json
import os
import subprocess

import numpy as np
import pytest

import gasal_ffi as G
import helpers
import nvbio_matrix_model as M
import nvbio_matrix_traceback_model as T
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = list(T.TYPES)


# ---- 1. the model against the oracle ----
def _same_as_oracle(ref_al, pats, texts, P, Tx):
    al = M.gotoh(ref_al.type, ref_al.gap_open, ref_al.gap_ext)
    mat = M.simple_table(4, ref_al.match, ref_al.mismatch)
    T.same(T.batch(al, mat, 4, pats, texts), O.nv_traceback(ref_al, P, Tx), f"type {ref_al.type}")


def test_reference_cigar_vectors():
    # alignment_test.cu:778-792 and :828-904 (tests/golden/nvbio_reference_kats.json): the Gotoh cases
    kats = json.load(open(os.path.join(helpers.GOLDEN, "nvbio_reference_kats.json")))
    cases = [c for c in kats["alignment"] + kats["traceback_real"] if c["aligner"] == "gotoh"]
    assert len(cases) == 4
    for c in cases:
        s = c["scheme"]
        type_ = {"GLOBAL": G.NV_GLOBAL, "LOCAL": G.NV_LOCAL, "SEMI_GLOBAL": G.NV_SEMI_GLOBAL}[c["type"]]
        ref_al = G.NvAligner(G.NV_GOTOH, type_, s["match"], s["mismatch"], s["gap_open"], s["gap_ext"])
        p, t = G.dna_n_codes(c["pattern"]), G.ref2_codes(c["text"])
        assert max(p) < 4 and max(t) < 4                       # no N: nothing for the clamp to change
        P, Tx = G.PackedSet.pack([p]), G.PackedSet.pack([t], bits=2, big_endian=False)
        _same_as_oracle(ref_al, [p], [t], P, Tx)
        r = T.pair(M.gotoh(type_, s["gap_open"], s["gap_ext"]), M.simple_table(4, s["match"], s["mismatch"]), 4, p, t)
        assert r["score"] == c["score"]
        assert O.nv_cigar_string(np.array(r["ops"], np.uint8), len(p), r["source"][1], r["sink"][1]) == c["cigar"]


@pytest.mark.parametrize("type_", TYPES)
def test_simple_table_is_the_oracle(type_):
    # 150 random related pairs; a third of them again under two more schemes (one with Ge < Go: the fill
    # and the walk do not care)
    pats, texts = [], []
    for seed in range(3):
        p, t = T.random_pairs(4, (1, 7, 8, 9, 16, 17, 33, 40, 63, 65), (1, 8, 9, 33, 70), 0x0C + 16 * seed + T.TYPES[type_])
        pats += p; texts += t
    pats3, texts3 = pats[::3], texts[::3]
    assert len(pats) == 150
    P, Tx = G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, 2, False)
    _same_as_oracle(G.NvAligner(G.NV_GOTOH, T.TYPES[type_], 2, -1, -2, -1), pats, texts, P, Tx)
    P3, T3 = G.PackedSet.pack(pats3, 4, True), G.PackedSet.pack(texts3, 2, False)
    _same_as_oracle(G.NvAligner(G.NV_GOTOH, T.TYPES[type_], 1, -1, -5, -3), pats3, texts3, P3, T3)
    _same_as_oracle(G.NvAligner(G.NV_GOTOH, T.TYPES[type_], 2, -3, -2, -4), pats3, texts3, P3, T3)


def test_empty_strings_report_nothing():
    al = M.gotoh("global", -5, -3)
    for p, t in (([], [1]), ([1], []), ([], [])):
        r = T.pair(al, HAND, 2, p, t)
        assert (r["score"], r["source"], r["sink"], r["ops"]) == (T.INT32_MIN, (T.NO_CELL,) * 2, (T.NO_CELL,) * 2, [])


# ---- 2. hand-worked pairs ----
# n = 2, the table as mat[p][t] (C layout mat[t + p*n]):   t=0  t=1
#                                                    p=0     2    5
#                                                    p=1    -3    4
# Cells are (i, j) = (text row, pattern column); S(i, j) = mat[p_j][t_i].
HAND = G.NvMatrix(np.array([[2, 5], [-3, 4]], np.int8))


def _hand(type_, go, ge, p, t):
    r = T.pair(M.gotoh(type_, go, ge), HAND, 2, p, t)
    return r["score"], r["source"], r["sink"], r["ops"]


def test_hand_local_needs_the_table_not_its_transpose():
    """LOCAL, Go = -5, Ge = -3, pattern [0, 1], text [1, 1].  All boundaries are 0 (E(i,-1) = 0 too).
      (0,0): S = mat[0][1] = 5; E = max(0 - 3, 0 - 5) = -3; F = max(inf, 0 - 5) = -5; diag = 0 + 5;  H = 5  SUB
      (0,1): S = mat[1][1] = 4; E = max(-3 - 3, 5 - 5) = 0;  F = -5;                  diag = 0 + 4;  H = 4  SUB
      (1,0): S = 5;             E = -3; F = max(-5 - 3, 5 - 5) = 0;                   diag = 0 + 5;  H = 5  SUB
      (1,1): S = 4;             E = max(-3 - 3, 5 - 5) = 0; F = max(-5 - 3, 4 - 5) = -1; diag = 5 + 4; H = 9  SUB
    Reports 5, 4, 5, 9: the sink is (2, 2), the walk two SUBSTITUTIONs to the source (0, 0).  The
    transposed table reads S(., 0) = mat[1][0] = -3: (0,0) and (1,0) become 0 (SINK), H(1,1) = 4."""
    assert _hand("local", -5, -3, [0, 1], [1, 1]) == (9, (0, 0), (2, 2), [0, 0])
    transposed = G.NvMatrix(np.ascontiguousarray(HAND.scores.T))
    r = T.pair(M.gotoh("local", -5, -3), transposed, 2, [0, 1], [1, 1])
    assert (r["score"], r["source"], r["sink"], r["ops"]) == (4, (1, 1), (2, 2), [0])


def test_hand_e_equals_f_above_the_diagonal_is_an_insertion():
    """GLOBAL, Go = -2, Ge = -1, pattern [1, 1], text [0, 0, 0]: S = mat[1][0] = -3 everywhere.
    H(-1,j) = -2, -3; H(i,-1) = -2, -3, -4; H(-1,-1) = 0.
      (0,0): E = H(0,-1) + Go = -4; F = H(-1,0) + Go = -4; diag = 0 - 3 = -3;   H = -3  SUB
      (0,1): E = max(-4 - 1, -3 - 2) = -5; F = -3 - 2 = -5; diag = -2 - 3 = -5; H = -5  SUB (all three tie)
      (1,0): E = -3 - 2 = -5; F = max(-4 - 1, -3 - 2) = -5; diag = -2 - 3 = -5; H = -5
      (1,1): E = max(-5 - 1, -5 - 2) = -6; F = max(-5 - 1, -5 - 2) = -6; diag = -3 - 3 = -6; H = -6
      (2,0): E = -4 - 2 = -6; F = max(-5 - 1, -5 - 2) = -6; diag = -3 - 3 = -6; H = -6
      (2,1): E = max(-6 - 1, -6 - 2) = -7 (the extension, strictly: INS_EXT); F = max(-6 - 1, -6 - 2) = -7;
             diag = -5 - 3 = -8;  H = -7: F > E is false, E > diag: INSERTION (with >= it would be a DELETION)
    GLOBAL reports (3, 2) = -7.  The walk: (2,1) H -> E state; (2,1) INS_EXT set, push I, stay; (2,0): E(2,-1) is
    the infimum, no INS_EXT, push I, back to H with the pattern used up; the first-column tail pushes D D D.
    Replayed: I I = -2 - 1, D D D = -2 - 1 - 1, together -7."""
    assert _hand("global", -2, -1, [1, 1], [0, 0, 0]) == (-7, (0, 0), (3, 2), [1, 1, 2, 2, 2])
    assert T.pair(M.gotoh("global", -2, -1), HAND, 2, [1, 1], [0, 0, 0])["ties"] >= 1


def test_hand_e_equals_the_diagonal_is_a_substitution():
    """SEMI_GLOBAL, Go = -2, Ge = -1, pattern [0, 0], text [0]: S = mat[0][0] = 2.
    H(-1,j) = -2, -3 (not LOCAL); H(0,-1) = 0 (not GLOBAL); E(0,-1) and F(-1,j) the infimum.
      (0,0): E = 0 - 2 = -2; F = -2 - 2 = -4; diag = 0 + 2 = 2;                H = 2  SUB
      (0,1): E = max(-2 - 1, 2 - 2) = 0; F = -3 - 2 = -5; diag = -2 + 2 = 0;   H = 0: E > diag is false: SUB
    SEMI_GLOBAL reports H(0, M-1) = 0 at (1, 2).  The walk: (0,1) SUB to row 0 with one pattern symbol left: the
    first-row tail pushes one INSERTION.  Replayed: S(p_1, t_0) = 2 and one I = -2, together 0."""
    assert _hand("semi", -2, -1, [0, 0], [0]) == (0, (0, 0), (1, 2), [0, 1])
    assert T.pair(M.gotoh("semi", -2, -1), HAND, 2, [0, 0], [0])["ties"] == 1


def test_hand_global_tails():
    """GLOBAL, Go = -5, Ge = -3.
    Pattern [1, 0], text [0]: H(-1,j) = -5, -8; H(0,-1) = -5.
      (0,0): S = mat[1][0] = -3; E = -5 - 5 = -10; F = -5 - 5 = -10; diag = 0 - 3 = -3;             H = -3  SUB
      (0,1): S = mat[0][0] = 2;  E = max(-10 - 3, -3 - 5) = -8; F = -8 - 5 = -13; diag = -5 + 2 = -3; H = -3  SUB
    The sink is (1, 2); (0,1) SUB leaves row 0 with one pattern symbol: the first-row tail pushes I
    (replayed: 2 - 5).
    Pattern [0], text [0, 1]: H(-1,0) = -5; H(i,-1) = -5, -8.
      (0,0): S = mat[0][0] = 2; E = -10; F = -10; diag = 2;                                           H = 2  SUB
      (1,0): S = mat[0][1] = 5; E = -8 - 5 = -13; F = max(-10 - 3, 2 - 5) = -3; diag = -5 + 5 = 0;   H = 0  SUB
    The sink is (2, 1); (1,0) SUB leaves column 0 with one text symbol: the first-column tail pushes D
    (replayed: 5 - 5)."""
    assert _hand("global", -5, -3, [1, 0], [0]) == (-3, (0, 0), (1, 2), [0, 1])
    assert _hand("global", -5, -3, [0], [0, 1]) == (0, (0, 0), (2, 1), [0, 2])


# ---- 3. ties are really present ----
@pytest.mark.parametrize("type_", TYPES)
def test_tie_family_ties(type_):
    # with at least half of the pairs walking through a tied cell, a kernel with >= in place of > in the
    # flags cannot pass test_gpu_nvbio_matrix_traceback.py's comparison on this family
    al, mat, n, pats, texts = T.family_block(type_)
    assert (al.gap_open, al.gap_ext) == T.TIE_GAPS == (-3, -1)
    assert mat.scores.min() == -2 and mat.scores.max() == 3 and not np.array_equal(mat.scores, mat.scores.T)
    assert len(pats) == 300
    share = T.tie_share(T.batch(al, mat, n, pats, texts)["ties"])
    assert share >= 0.5, share


# ---- 4. replay ----
_FAMILIES = T.families()


@pytest.mark.parametrize("name", list(_FAMILIES))
def test_replay_is_the_score(name):
    al, mat, n, pats, texts = _FAMILIES[name]
    assert al.gap_ext >= al.gap_open
    res = T.batch(al, mat, n, pats, texts)
    for k in range(len(pats)):
        assert T.replay(al, mat, n, pats[k], texts[k], T.one(res, k)) == res["score"][k], (name, k)
        # the spans are real cells
        assert res["sink"][k][0] <= len(texts[k]) and res["sink"][k][1] <= len(pats[k])


@pytest.mark.parametrize("type_", TYPES)
def test_replay_on_the_simple_table_strings(type_):
    # the strings of the GPU test against the existing kernel (4-bit patterns, 2-bit texts), per-pair and shared
    import nvbio_sink_model as R
    ref_al = R.aligner("gotoh", type_)
    al, mat = M.gotoh(type_, ref_al.gap_open, ref_al.gap_ext), M.simple_table(4, ref_al.match, ref_al.mismatch)
    for pats, texts in (R.packed("edge", T.SIMPLE_LENS, T.SIMPLE_SEED)[:2],
                        R.packed("shared", T.SIMPLE_LENS, T.SIMPLE_SEED, n_text=T.SIMPLE_SHARED_TEXT)[:2]):
        texts = list(texts) * len(pats) if len(texts) == 1 else texts
        res = T.batch(al, mat, 4, pats, texts)
        for k in range(len(pats)):
            assert T.replay(al, mat, 4, pats[k], texts[k], T.one(res, k)) == res["score"][k], k


# ---- 5. the header ----
def _hipcc(tmp_path, *extra):
    return ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
            os.path.join(ROOT, "tools", "nvbio_matrix_header_check.cpp"), "-o", str(tmp_path / "check"), *extra]


def test_header_routes_the_matrix_traceback(tmp_path):
    # host only, stubs of the C API: BatchedAlignmentTraceback over the matrix aligner reaches
    # gasalx_nv_matrix_traceback_device with the table, n, the gap scores and every output pointer; a
    # Simple-scheme stream still reaches gasalx_nv_traceback_device
    subprocess.run(_hipcc(tmp_path), check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(tmp_path / "check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_banded_traceback_over_a_matrix_does_not_compile(tmp_path):
    r = subprocess.run(_hipcc(tmp_path, "-DCHECK_BANDED_TRACEBACK_OVER_MATRIX_REFUSED"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0
    assert "static assertion failed" in r.stderr, r.stderr
    assert "the banded scorer and the banded traceback have no matrix kernels" in r.stderr, r.stderr


# ---- 6. exports ----
def test_entry_points_are_exported():
    for name in ("gasalx_nv_matrix_traceback_device", "gasalx_nv_matrix_traceback_host"):
        assert name in G.EXPORTS
        assert hasattr(G.lib(), name), name
    assert hasattr(G.Engine, "nv_matrix_traceback_host") and hasattr(G.Engine, "nv_matrix_traceback_device_ptrs")

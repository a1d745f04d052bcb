"""CPU checks of the semi-global CIGAR call (gasalx_semi_cigar_*): the model every GPU comparison
uses (tests/semi_cigar_model.py) against the matrix the kernels already compute (independent.semi),
a replay of its CIGARs that does not depend on tie rules, hand cases with the expected text, the
exported symbols and the planner's names over a small grid.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import gasal_ffi as G
import independent as I
import semi_cigar_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(M.named_batches())


# ---- the model computes the matrix the kernels compute ----
@pytest.mark.parametrize("name", NAMES)
def test_model_score_and_ends_equal_independent_semi(name):
    b, m = M.reference(name)
    sc = M.named_batches()[name][1]
    ref = I.semi(b, M.TARGET, M.TARGET, **sc)
    for f in ("score", "q_end", "t_end"):
        assert np.array_equal(m[f], ref[f]), (name, f, np.flatnonzero(m[f] != ref[f])[:5])


@pytest.mark.parametrize("sc", [dict(a=2, b=7, o=2, e=3), dict(a=3, b=3, o=1, e=1), dict(a=1, b=2, o=0, e=1),
                                dict(a=5, b=4, o=6, e=1, npen=8), dict(a=1, b=4, o=6, e=1, npen=1),
                                dict(a=1, b=9, o=1, e=1), dict(a=2, b=30, o=0, e=0)])
def test_model_equals_independent_semi_where_gaps_open_from_gaps(sc):
    # cheap gaps against dear substitutions: insertion runs next to deletion runs, which a matrix
    # whose gaps open from the diagonal candidate (GLOBAL's) cannot hold
    rng = M._rng("edge", sorted(sc.items()))
    qs = [M._dna(rng, int(rng.integers(1, 40)), b"ACGTN" if "npen" in sc else b"ACGT") for _ in range(200)]
    ts = [M._dna(rng, int(rng.integers(1, 48)), b"ACGTN" if "npen" in sc else b"ACGT") for _ in range(200)]
    b = M.ModelBatch.from_pairs(qs, ts)
    m, ref = M.semi_cigar(b, **sc), I.semi(b, M.TARGET, M.TARGET, **sc)
    for f in ("score", "q_end", "t_end"):
        assert np.array_equal(m[f], ref[f]), f


# ---- replay: what the CIGAR consumes and what it is worth ----
def _seq(data, offs, lens, p):
    return bytes(data[int(offs[p]):int(offs[p]) + int(lens[p])])


def replay(q, t, text, t_start, t_end, a, b, o, e):
    """(query bases consumed, target bases consumed, score) of a forward CIGAR over t[t_start:].  M / X
    by the bases; a run of k D or I costs o + e*k.  The one exception: a leading I run at t_start = 0
    sits in the left boundary, which the kernels price H(r, -1) = -(o + e*r): k bases for o + e*(k-1),
    one base for nothing (semiglobal_kernel_template.h:94-98)."""
    qi, ti, score, first = 0, t_start, 0, True
    for cnt, op in re.findall(r"(\d+)([MXDI])", text):
        k = int(cnt)
        if op in "MX":
            for _ in range(k):
                score += a if q[qi] == t[ti] else -b
                qi += 1; ti += 1
        elif op == "D":
            score -= o + e * k; ti += k
        elif first and t_start == 0:
            score -= 0 if k == 1 else o + e * (k - 1); qi += k
        else:
            score -= o + e * k; qi += k
        first = False
    return qi, ti - t_start, score


REPLAY = [n for n in NAMES if n not in ("n_targets", "ops")]   # no N on a path: those two match the model exactly


@pytest.mark.parametrize("name", REPLAY)
def test_replay_closes_for_every_pair(name):
    b, m = M.reference(name)
    sc = M.named_batches()[name][1]
    for p in range(b.n):
        q, t = _seq(b.q_data, b.q_offsets, b.q_lens, p), _seq(b.t_data, b.t_offsets, b.t_lens, p)
        ts, te = int(m["t_start"][p]), int(m["t_end"][p])
        nq, nt, s = replay(q, t, m["text"][p], ts, te, sc["a"], sc["b"], sc["o"], sc["e"])
        assert nq == len(q), (name, p, m["text"][p])
        assert nt == te - ts + 1, (name, p, m["text"][p], ts, te)
        assert s == int(m["score"][p]), (name, p, m["text"][p], s, int(m["score"][p]))


# ---- hand cases ----
T0 = b"GATTACAGGCTTAGCCATGCAAGTCCGATAGCTTGACCGTAAGCTTACGGATCA"


def one(q, t, **sc):
    m = M.semi_cigar(M.ModelBatch.from_pairs([q], [t]), **(sc or M.DEFAULT))
    return m["text"][0], int(m["t_start"][0]), int(m["t_end"][0]), int(m["score"][0])


def test_hand_exact_substring():
    assert one(T0[7:27], T0) == ("20M", 7, 26, 20)


def test_hand_one_deletion():
    q = T0[5:17] + T0[18:32]          # target base 17 missing from the read
    assert one(q, T0) == ("12M1D14M", 5, 31, 26 - 7)


def test_hand_one_insertion():
    q = T0[5:17] + b"T" + T0[17:31]   # T0[17] is A: the inserted T matches neither neighbour
    assert one(q, T0) == ("12M1I14M", 5, 30, 26 - 7)


def test_hand_mismatch():
    q = bytearray(T0[10:30]); q[8] = ord("A") if q[8] != ord("A") else ord("C")
    assert one(bytes(q), T0) == ("8M1X11M", 10, 29, 19 - 4)


def test_hand_leading_insertion():
    # the read hangs over the window's left edge by three bases: the left boundary's insertions
    # (three bases for o + 2e = 8), t_start = 0
    q = b"CCC" + T0[:20]
    assert one(q, T0) == ("3I20M", 0, 19, 20 - 8)


def test_hand_all_insertions():
    # nothing matches and a substitution costs more than staying in the gap: the query is one insertion
    # run from the top boundary at column 0 (the first maximum), which consumes no target base
    text, ts, te, s = one(b"AAAA", b"CCCC", a=1, b=9, o=1, e=4)
    assert (text, ts, te) == ("4I", 1, 0) and s == -(1 + 4 * 4)


def test_hand_homopolymer_tie():
    # six A against ten: every window scores 6; the first maximum of the last row is column 5, and
    # the diagonal wins every tie (H == tmp is tested first)
    assert one(b"AAAAAA", b"AAAAAAAAAA") == ("6M", 0, 5, 6)
    # one base more in the read than in the run: the walk, coming from the end, stays on the diagonal
    # while H == tmp holds, so the insertion lands on the run's first base
    text, ts, te, s = one(b"CAAAAAG", b"TTCAAAAGTT")
    assert (ts, te, s) == (2, 7, 6 - 7) and text == "1M1I5M"


# ---- the interface exists ----
def test_symbols_exported_and_declared():
    src = open(os.path.join(ROOT, "include", "gasalx.h")).read()
    lib = G.lib()
    for name in ("gasalx_semi_cigar_device", "gasalx_semi_cigar_host", "gasalx_describe_semi_cigar_plan"):
        assert re.search(r"^\s*int\s+" + name + r"\s*\(", src, re.M), name
        assert hasattr(lib, name), name
        assert name in G.EXPORTS
    assert hasattr(G.Engine, "semi_cigar_host") and hasattr(G.Engine, "semi_cigar_device_ptrs")


# ---- the planner over a small grid (tests/golden/semi_cigar_plan_names.json, tools/plan_grid.py --semi-cigar) ----
PLAN_SCORES = ((1, 4, 6, 1), (200, 56, 6, 1))   # the second: match + table offset past a byte, never packed
PLAN_LENS = (8, 150, 152, 300)
PLAN_ENVS = ("", "GASALX_PACKED16=0")


def semi_cigar_plan_rows(setenv, unsetenv):
    rows = {}
    for env in PLAN_ENVS:
        if env:
            setenv(*env.split("="))
        try:
            for sc in PLAN_SCORES:
                for ql in PLAN_LENS:
                    for tl in (ql, ql + 32):
                        p = G.make_params(algo=G.SEMI_GLOBAL, head=G.TARGET, tail=G.TARGET, match=sc[0],
                                          mismatch=sc[1], gap_open=sc[2], gap_extend=sc[3])
                        try:
                            name = G.describe_semi_cigar_plan(p, ql, tl)
                        except RuntimeError as ex:
                            name = "error: " + str(ex).split("): ", 1)[-1]
                        rows[f"{env or 'default'}|{'/'.join(map(str, sc))}|{ql}x{tl}"] = name
        finally:
            if env:
                unsetenv(env.split("=")[0])
    return rows


def test_plan_names_over_the_grid(monkeypatch):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "semi_cigar_plan_names.json")))
    rows = semi_cigar_plan_rows(monkeypatch.setenv, monkeypatch.delenv)
    assert rows == gold["rows"]
    # both families and the refusal appear in it
    assert rows["default|1/4/6/1|150x182"] == "wavefront16_semi_tb_G8R20"
    assert rows["GASALX_PACKED16=0|1/4/6/1|150x182"] == "wavefront_semi_tb_G8R20"
    assert rows["default|200/56/6/1|8x8"].startswith("wavefront_semi_tb_")
    assert rows["default|200/56/6/1|300x332"].startswith("error: semi_cigar: lengths x scores")


def test_describe_refuses_other_heads_and_tails():
    for head in (G.NONE, G.QUERY, G.TARGET, G.BOTH):
        for tail in (G.NONE, G.QUERY, G.TARGET, G.BOTH):
            if (head, tail) == (G.TARGET, G.TARGET):
                continue
            p = G.make_params(algo=G.SEMI_GLOBAL, head=head, tail=tail)
            with pytest.raises(RuntimeError, match=r"\(-5\): semi_cigar: HEAD=\w+ TAIL=\w+ is not supported"):
                G.describe_semi_cigar_plan(p, 150, 182)
    with pytest.raises(RuntimeError, match=r"\(-5\): semi_cigar: negative gap_open or gap_extend"):
        G.describe_semi_cigar_plan(G.make_params(algo=G.SEMI_GLOBAL, gap_extend=-1), 150, 182)
    with pytest.raises(RuntimeError, match=r"\(-2\): semi_cigar: padded query of 1288 over the largest"):
        G.describe_semi_cigar_plan(G.make_params(algo=G.SEMI_GLOBAL), 1281, 100)

"""CPU checks of the semi-global CIGAR call for every HEAD (gasalx_semi_cigar_head_*): the model the GPU
comparison uses (tests/semi_cigar_head_model.py) against the matrix the kernels already compute
(independent.semi), against the HEAD = TARGET model, a re-scoring of every path with the boundary
prices, what the ops consume, hand cases with the expected text, the exported symbols, the refusals
and the planner's names over a small grid.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import gasal_ffi as G
import independent as I
import semi_cigar_head_model as H
import semi_cigar_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(H.named_batches())
HEAD_IDS = [H.HEAD_NAME[h] for h in H.HEADS]


# ---- 1: the model computes the matrix the kernels compute ----
@pytest.mark.parametrize("head", H.HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_score_and_ends_equal_independent_semi(name, head):
    b, m = H.reference(name, head)
    ref = I.semi(b, head, H.TARGET, **H.named_batches()[name][1])
    for f in ("score", "q_end", "t_end"):
        assert np.array_equal(m[f], ref[f]), (name, f, np.flatnonzero(m[f] != ref[f])[:5])


@pytest.mark.parametrize("head", H.HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("sc", [dict(a=2, b=7, o=2, e=3), dict(a=3, b=3, o=1, e=1), dict(a=1, b=2, o=0, e=1),
                                dict(a=5, b=4, o=6, e=1, npen=8), dict(a=1, b=9, o=1, e=1), dict(a=2, b=30, o=0, e=0)])
def test_score_and_ends_with_cheap_gaps(sc, head):
    rng = M._rng("head_edge", sorted(sc.items()))
    qs = [M._dna(rng, int(rng.integers(1, 40)), b"ACGTN" if "npen" in sc else b"ACGT") for _ in range(200)]
    ts = [M._dna(rng, int(rng.integers(1, 48)), b"ACGTN" if "npen" in sc else b"ACGT") for _ in range(200)]
    b = M.ModelBatch.from_pairs(qs, ts)
    m, ref = H.semi_cigar_head(b, head, **sc), I.semi(b, head, H.TARGET, **sc)
    for f in ("score", "q_end", "t_end"):
        assert np.array_equal(m[f], ref[f]), f


# ---- 2: HEAD = TARGET is the existing model ----
@pytest.mark.parametrize("name", [n for n in NAMES if n != "overhang_q"])
def test_head_target_equals_the_semi_cigar_model(name):
    b, m = H.reference(name, H.TARGET)
    old = M.reference(name)[1]
    for f in ("score", "q_end", "t_end", "q_start", "t_start", "n_ops", "cigar"):
        assert np.array_equal(m[f], old[f]), (name, f)
    assert m["text"] == old["text"] and m["ops"] == old["ops"]


# ---- 3 and 4: every path re-scored with the boundary prices; what the ops consume ----
def _seq(data, offs, lens, p):
    return bytes(data[int(offs[p]):int(offs[p]) + int(lens[p])])


REPLAY = [n for n in NAMES if n not in ("n_targets", "ops")]   # no N on a path


@pytest.mark.parametrize("head", H.HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("name", REPLAY)
def test_paths_rescore_and_consume(name, head):
    b, m = H.reference(name, head)
    sc = H.named_batches()[name][1]
    for p in range(b.n):
        q, t = _seq(b.q_data, b.q_offsets, b.q_lens, p), _seq(b.t_data, b.t_offsets, b.t_lens, p)
        qs, ts, te = int(m["q_start"][p]), int(m["t_start"][p]), int(m["t_end"][p])
        nq, nt, s = H.rescore(q, t, m["text"][p], head, qs, ts, sc["a"], sc["b"], sc["o"], sc["e"])
        assert nq == len(q) - qs, (name, p, m["text"][p], qs)
        assert nt == te - ts + 1, (name, p, m["text"][p], ts, te)
        assert s == int(m["score"][p]), (name, p, m["text"][p], s, int(m["score"][p]))
        if head in (H.NONE, H.TARGET):
            assert qs == 0
        if head in (H.NONE, H.QUERY):
            assert ts == 0


def test_the_new_endings_occur():
    # HEAD = QUERY really leaves a free query head on overhang_q, HEAD = NONE really pays boundary
    # deletions on overhang
    _, m = H.reference("overhang_q", H.QUERY)
    assert (m["q_start"] > 0).sum() * 2 >= len(m["q_start"]), int((m["q_start"] > 0).sum())
    _, m = H.reference("overhang", H.NONE)
    assert sum(x == "D" for x in m["bound"]) * 4 >= len(m["bound"]), sum(x == "D" for x in m["bound"])
    _, m = H.reference("overhang_q", H.BOTH)
    assert (m["q_start"] > 0).any()


# ---- hand cases: (text, q_start, t_start, t_end, score) ----
def one(q, t, head, **sc):
    m = H.semi_cigar_head(M.ModelBatch.from_pairs([q], [t]), head, **(sc or M.DEFAULT))
    return m["text"][0], int(m["q_start"][0]), int(m["t_start"][0]), int(m["t_end"][0]), int(m["score"][0])


def test_hand_none_pays_the_top_boundary():
    # anchored at (0, 0): the two target bases before the match are the top boundary's deletions, the
    # diagonal into (0, 2) holds -(o + 2e) = -3
    assert one(b"GTAC", b"AAGTAC", H.NONE, a=5, b=4, o=1, e=1) == ("2D4M", 0, 0, 5, 20 - 3)


def test_hand_query_skips_the_query_prefix():
    # CC is the free query head: the diagonal into (2, 0) is H(1, -1) = 0
    assert one(b"CCAGTA", b"AGTAC", H.QUERY) == ("4M", 2, 0, 3, 4)


def test_hand_query_deletion_out_of_the_free_boundary_costs_e():
    # G stands at target column 1: the deletion of column 0 leaves the free boundary at row 1 for e = 1,
    # not o + e = 7 (E(1, -1) = 0)
    assert one(b"CCGTA", b"AGTA", H.QUERY, a=5, b=4, o=6, e=1) == ("1D3M", 2, 0, 3, 15 - 1)


def test_hand_target_skips_the_target_prefix():
    assert one(b"GTAC", b"AAGTACAA", H.TARGET) == ("4M", 0, 2, 5, 4)


def test_hand_both_skips_either_prefix():
    assert one(b"CCGTA", b"GTACC", H.BOTH) == ("3M", 2, 0, 2, 3)
    assert one(b"GTA", b"CCGTA", H.BOTH) == ("3M", 0, 2, 4, 3)


def test_hand_none_top_row_price_before_an_insertion():
    # Q3: the value above (0, 0) is -o, so one target base deleted before an insertion run costs o, not
    # o + e.  Nothing matches and substitutions are dear: the first maximum of the last row is column 0,
    # reached by the insertion run from above it: -o - (o + 2e) = -1 - 3
    text, qs, ts, te, s = one(b"AA", b"CC", H.NONE, a=1, b=9, o=1, e=1)
    assert (text, qs, ts, te, s) == ("1D2I", 0, 0, 0, -4)


# ---- the interface ----
NEW = ("gasalx_semi_cigar_head_device", "gasalx_semi_cigar_head_host", "gasalx_describe_semi_cigar_head_plan")


def test_symbols_exported_and_declared():
    src = open(os.path.join(ROOT, "include", "gasalx.h")).read()
    lib = G.lib()
    for name in NEW:
        assert re.search(r"^\s*int\s+" + name + r"\s*\(", src, re.M), name
        assert hasattr(lib, name), name
        assert name in G.EXPORTS
    assert hasattr(G.Engine, "semi_cigar_head_host") and hasattr(G.Engine, "semi_cigar_head_device_ptrs")


def test_refusals():
    for head in (G.NONE, G.QUERY, G.TARGET, G.BOTH):
        for tail, tname in ((G.NONE, "NONE"), (G.QUERY, "QUERY"), (G.BOTH, "BOTH")):
            p = G.make_params(algo=G.SEMI_GLOBAL, head=head, tail=tail)
            with pytest.raises(RuntimeError, match=r"\(-5\): semi_cigar_head: HEAD=\w+ TAIL=" + tname +
                               r" is not supported \(TAIL=TARGET only\)"):
                G.describe_semi_cigar_head_plan(p, 150, 182)
        with pytest.raises(RuntimeError, match=r"\(-5\): semi_cigar_head: second_best is not supported"):
            G.describe_semi_cigar_head_plan(G.make_params(algo=G.SEMI_GLOBAL, head=head, second_best=1), 150, 182)
        with pytest.raises(RuntimeError, match=r"\(-1\): semi_cigar_head: algo must be SEMI_GLOBAL"):
            G.describe_semi_cigar_head_plan(G.make_params(algo=G.LOCAL, head=head), 150, 182)
        for gap in (dict(gap_open=-1), dict(gap_extend=-1)):
            with pytest.raises(RuntimeError, match=r"\(-5\): semi_cigar_head: negative gap_open or gap_extend"):
                G.describe_semi_cigar_head_plan(G.make_params(algo=G.SEMI_GLOBAL, head=head, **gap), 150, 182)
        with pytest.raises(RuntimeError, match=r"\(-2\): semi_cigar_head: padded query of 1288 over the largest"):
            G.describe_semi_cigar_head_plan(G.make_params(algo=G.SEMI_GLOBAL, head=head), 1281, 100)
    # the first call still refuses the other heads, in its own words
    with pytest.raises(RuntimeError, match=r"\(-5\): semi_cigar: HEAD=QUERY TAIL=TARGET is not supported"):
        G.describe_semi_cigar_plan(G.make_params(algo=G.SEMI_GLOBAL, head=G.QUERY), 150, 182)


# ---- the planner over a small grid (tests/golden/semi_cigar_head_plan_names.json) ----
PLAN_SCORES = ((1, 4, 6, 1), (200, 56, 6, 1))   # the second: match + table offset past a byte, never packed
PLAN_LENS = (8, 150, 152, 300)
PLAN_ENVS = ("", "GASALX_PACKED16=0")
SUFFIX = {G.NONE: "_hn", G.QUERY: "_hq", G.TARGET: "_ht", G.BOTH: "_hb"}


def semi_cigar_head_plan_rows(setenv, unsetenv):
    rows = {}
    for env in PLAN_ENVS:
        if env:
            setenv(*env.split("="))
        try:
            for head in (G.NONE, G.QUERY, G.TARGET, G.BOTH):
                for sc in PLAN_SCORES:
                    for ql in PLAN_LENS:
                        for tl in (ql, ql + 32):
                            p = G.make_params(algo=G.SEMI_GLOBAL, head=head, tail=G.TARGET, match=sc[0],
                                              mismatch=sc[1], gap_open=sc[2], gap_extend=sc[3])
                            try:
                                name = G.describe_semi_cigar_head_plan(p, ql, tl)
                            except RuntimeError as ex:
                                name = "error: " + str(ex).split("): ", 1)[-1]
                            rows[f"{env or 'default'}|{SUFFIX[head][1:]}|{'/'.join(map(str, sc))}|{ql}x{tl}"] = name
        finally:
            if env:
                unsetenv(env.split("=")[0])
    return rows


def test_plan_names_over_the_grid(monkeypatch):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "semi_cigar_head_plan_names.json")))
    rows = semi_cigar_head_plan_rows(monkeypatch.setenv, monkeypatch.delenv)
    assert rows == gold["rows"]
    assert rows["default|hq|1/4/6/1|150x182"] == "wavefront16_semi_tb_G8R20_hq"
    assert rows["GASALX_PACKED16=0|hn|1/4/6/1|150x182"] == "wavefront_semi_tb_G8R20_hn"
    assert rows["default|hb|200/56/6/1|8x8"].startswith("wavefront_semi_tb_")
    assert rows["default|hn|200/56/6/1|300x332"].startswith("error: semi_cigar_head: lengths x scores")
    # a head changes the suffix and nothing else: the same shapes as gasalx_semi_cigar_*'s golden rows
    first = json.load(open(os.path.join(ROOT, "tests", "golden", "semi_cigar_plan_names.json")))["rows"]
    for key, name in rows.items():
        env, h, sc, lens = key.split("|")
        want = first[f"{env}|{sc}|{lens}"]
        if want.startswith("error: "):
            assert name == want.replace("semi_cigar:", "semi_cigar_head:"), key
        else:
            assert name == want + "_" + h, key

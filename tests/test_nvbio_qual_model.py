"""Quality-aware Gotoh scoring for the banded aligners (gasalx_nv_banded_qual_*), the parts that need
no GPU: the definition the GPU tests compare against (tests/nvbio_qual_model.py, written from the cited
nvbio and nvBowtie lines) on pairs worked by hand; its reduction to the verified oracle under constant
tables; a replay of its alignments by an independent function; the table builders; a condition on the
GPU tests' inputs under which a kernel that ignored the qualities could not pass; the kernel names; the
order of the entry points' checks; the header's routing and compile-time refusals.

The pairs worked by hand, band 3, scheme S2: two levels, match (2, 2), mismatch (-1, -9), gap open -3,
gap extension -1.
  A. pattern 0 1 2 3 0 1 against text 0 1 3 3 0 1 2 2, SEMI_GLOBAL.  Pattern symbol 2 (a 2 against the
     text's 3) is the only disagreement on the main diagonal.
       quality level 0 there: the mismatch costs 1: six diagonal steps, 5 x 2 - 1 = 9, ending at (6, 6),
         ops M M M M M M.
       quality level 1: the mismatch costs 9, and leaving the diagonal and coming back (one pattern gap,
         one text gap, each opened at -3) costs 6: 5 x 2 - 3 - 3 = 4 at (6, 6); walking back from the
         sink the pushes are M M M (symbols 5, 4, 3), I (pattern symbol 2 unmatched), D (text symbol 2
         unmatched), M M.
  B. pattern 0 1 2 3 0 1 against text 0 1 2 2 0 1 3 3, LOCAL.  Three matches reach 6 at (3, 3); symbol 3
     disagrees; two more matches follow.
       level 0: 6 - 1 + 2 + 2 = 9 at (6, 6), source (0, 0).
       level 1: 6 - 9 clamps to 0, the tail reaches 4 only: the best stays 6 and the sink moves to (3, 3).
  C. pattern 0 1 against text 0 1 0 1, SEMI_GLOBAL: row 1 holds 4 in slot 0 (0 1 against text 0 1) and
     again in slot 2 (against text 2 3 = 0 1); slot 1 holds less; m = min(2 + 2, 4) - 1 = 3 slots are
     reported at (2, 2), (3, 2), (4, 2) and the last maximum wins: (4, 4, 2), source (2, 0).
  D. pair A with the quality byte 200 on symbol 2: 200 >= levels = 2 reads level 1: A's second answer."""
import os
import subprocess

import numpy as np
import pytest

import gasal_ffi as G
import nvbio_banded_sinks_model as R
import nvbio_qual_model as Q
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLOBAL, LOCAL, SEMI = G.NV_GLOBAL, G.NV_LOCAL, G.NV_SEMI_GLOBAL
TYPES = {"global": GLOBAL, "local": LOCAL, "semi": SEMI}
BANDS = (2, 3, 7, 8, 15, 16, 17, 31, 32)                 # the GPU tests' bands
REDUCTION_BANDS = (3, 7, 15, 31, 5, 12, 20)              # the exact instances, one inexact band per register size
SEED = 0x9A1B
N_PAIRS = 600
EINVAL, ERANGE, EUNSUPPORTED = -1, -2, -5
NEW_SYMBOLS = ("gasalx_nv_banded_qual_score_device", "gasalx_nv_banded_qual_score_host",
               "gasalx_nv_banded_qual_traceback_device", "gasalx_nv_banded_qual_traceback_host",
               "gasalx_nv_describe_banded_qual_plan")

S2 = Q.Scheme([2, 2], [-1, -9], -3, -1)
# nvBowtie's default (end-to-end: match 0) and its --local flavour (bowtie2's --ma 2): under match 0 every
# LOCAL cell is 0, so LOCAL cases that must see the qualities use the second
DEFAULT = Q.nvbowtie_default()
LOCAL_DEFAULT = Q.Scheme(Q.constant_cost(2), DEFAULT.mismatch_t, -8, -3)


def gotoh(type_, sc):
    return G.NvAligner(G.NV_GOTOH, type_, 0, 0, sc.gap_open, sc.gap_ext)


def nv_quals(sc, quals, **kw):
    return G.NvQuals(quals, sc.match_t, sc.mismatch_t, **kw)


_inputs = {}


def inputs():
    """The GPU tests' pairs: R.tie_pairs with N among the pattern symbols and a 12% substitution rate
    laid over it (tie_pairs' own 6% leaves too few pairs whose score depends on a quality), qualities
    from Q.attach_quals; 4-bit big-endian patterns, 2-bit little-endian texts."""
    if not _inputs:
        pats, texts = R.tie_pairs(SEED, n=N_PAIRS, symbols=5)
        rng = np.random.default_rng(SEED + 7)
        for k, p in enumerate(pats):
            if k % 4 != 1 and k % 8 != 7:                 # the tied and the disjoint pairs stay as they are
                sub = rng.random(len(p)) < 0.12
                p[sub] = rng.integers(0, 4, int(sub.sum()))
        quals = Q.attach_quals(SEED, pats)
        _inputs.update(pats=pats, texts=texts, quals=quals, flat=Q.flat_quals(quals), P=G.PackedSet.pack(pats, 4, True),
                       T=G.PackedSet.pack(texts, 2, False))
    return _inputs


_wants = {}


def want(sc_name, type_, band):
    """The model's traceback of the GPU tests' pairs, computed once per (scheme, type, band)."""
    key = (sc_name, type_, band)
    if key not in _wants:
        d = inputs()
        sc = {"default": DEFAULT, "local_default": LOCAL_DEFAULT}[sc_name]
        _wants[key] = Q.traceback(sc, type_, band, d["pats"], d["quals"], d["texts"])
    return _wants[key]


def replay(sc, type_, pattern, quals, text, source, sink, ops):
    """The score of an alignment's ops walked forwards from source to sink under the scheme: an
    independent few lines, not the model's walk.  Row zero of GLOBAL is the boundary G_o + (x - 1) G_e."""
    x, y = int(source[0]), int(source[1])
    s = sc.gap_open + (x - 1) * sc.gap_ext if type_ == GLOBAL and x > 0 else 0
    prev = 0
    for op in list(ops)[::-1]:
        if op == 0:
            r = int(text[x]) if x < len(text) else 255
            lvl = min(int(quals[y]), sc.levels - 1)
            s += sc.match_t[lvl] if r == int(pattern[y]) else sc.mismatch_t[lvl]
            x, y = x + 1, y + 1
        else:
            s += sc.gap_ext if op == prev else sc.gap_open
            x, y = (x, y + 1) if op == 1 else (x + 1, y)
        prev = op
    assert (x, y) == (int(sink[0]), int(sink[1]))
    return s


@pytest.fixture(scope="module", autouse=True)
def _built():
    O.build()


def test_exports():
    # the feature's public surface: fails on a library without it
    for name in NEW_SYMBOLS:
        assert name in G.EXPORTS and hasattr(G.lib(), name), name
    for name in ("nv_banded_qual_score_host", "nv_banded_qual_score_device_ptrs", "nv_banded_qual_traceback_host",
                 "nv_banded_qual_traceback_device_ptrs"):
        assert hasattr(G.Engine, name), name
    assert hasattr(G, "nv_describe_banded_qual_plan") and hasattr(G, "NvQuals")


# ---- 1. by hand ----
def test_hand_worked_pairs():
    pa, ta = [0, 1, 2, 3, 0, 1], [0, 1, 3, 3, 0, 1, 2, 2]
    low, high = [0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0]
    assert Q.traceback_one(S2, SEMI, 3, pa, low, ta) == (9, (0, 0), (6, 6), [0, 0, 0, 0, 0, 0])
    assert Q.traceback_one(S2, SEMI, 3, pa, high, ta) == (4, (0, 0), (6, 6), [0, 0, 0, 1, 2, 0, 0])
    pb, tb = [0, 1, 2, 3, 0, 1], [0, 1, 2, 2, 0, 1, 3, 3]
    assert Q.traceback_one(S2, LOCAL, 3, pb, [0, 0, 0, 0, 0, 0], tb) == (9, (0, 0), (6, 6), [0, 0, 0, 0, 0, 0])
    assert Q.traceback_one(S2, LOCAL, 3, pb, [0, 0, 0, 1, 0, 0], tb) == (6, (0, 0), (3, 3), [0, 0, 0])
    assert Q.traceback_one(S2, SEMI, 3, [0, 1], [0, 0], [0, 1, 0, 1]) == (4, (2, 0), (4, 2), [0, 0])
    assert Q.traceback_one(S2, SEMI, 3, pa, [0, 0, 200, 0, 0, 0], ta) == (4, (0, 0), (6, 6), [0, 0, 0, 1, 2, 0, 0])
    assert Q.score_one(S2, SEMI, 3, pa, [0, 0, 200, 0, 0, 0], ta) == (4, 6, 6)
    # a text shorter than its pattern; LOCAL with an empty pattern
    assert Q.traceback_one(S2, SEMI, 3, [0, 1], [0, 0], [0]) == (Q.INT32_MIN, (Q.NO_SINK,) * 2, (Q.NO_SINK,) * 2, [])
    assert Q.score_one(S2, LOCAL, 3, [], [], ta) == (Q.INT32_MIN, Q.NO_SINK, Q.NO_SINK)


def test_batch_form_equals_the_pair_form():
    d = inputs()
    sel = list(range(0, N_PAIRS, 5))
    pats, quals, texts = ([d[k][i] for i in sel] for k in ("pats", "quals", "texts"))
    for type_ in TYPES.values():
        for band in (2, 3, 16):
            b = Q.traceback(LOCAL_DEFAULT, type_, band, pats, quals, texts)
            for i in range(len(sel)):
                s, src, snk, ops = Q.traceback_one(LOCAL_DEFAULT, type_, band, pats[i], quals[i], texts[i])
                assert (s, src, snk, ops) == (int(b["score"][i]), tuple(int(v) for v in b["source"][i]),
                                              tuple(int(v) for v in b["sink"][i]), list(b["ops"][i])), (type_, band, i)


# ---- 2. constant tables reduce to what is already verified ----
@pytest.mark.parametrize("tname", list(TYPES))
def test_constant_tables_equal_the_oracle(tname):
    d = inputs()
    type_ = TYPES[tname]
    for a, b, go, ge, levels in ((2, -1, -2, -1, 1), (5, -4, -10, -1, 41)):
        al = G.NvAligner(G.NV_GOTOH, type_, a, b, go, ge)
        sc = Q.constant_scheme(a, b, go, ge, levels)
        for band in REDUCTION_BANDS:
            o = O.nv_banded_traceback(al, band, d["P"], d["T"])
            m = Q.traceback(sc, type_, band, d["pats"], d["quals"], d["texts"])
            for f in ("score", "source", "sink"):
                assert np.array_equal(o[f], m[f]), (band, f)
            assert all(np.array_equal(x, y) for x, y in zip(o["ops"], m["ops"])), band
            ms, mk = Q.best_sinks(sc, type_, band, d["pats"], d["quals"], d["texts"])
            assert np.array_equal(ms, o["score"]) and np.array_equal(mk, o["sink"]), band


# ---- 3. replay ----
@pytest.mark.parametrize("tname", list(TYPES))
def test_replay_gives_the_reported_score(tname):
    d = inputs()
    type_ = TYPES[tname]
    for name, sc in (("default", DEFAULT), ("local_default", LOCAL_DEFAULT)):
        for band in (3, 15, 32):
            res = want(name, type_, band)
            for k in range(N_PAIRS):
                if res["score"][k] == Q.INT32_MIN:
                    continue
                got = replay(sc, type_, d["pats"][k], d["quals"][k], d["texts"][k], res["source"][k], res["sink"][k],
                             res["ops"][k])
                assert got == res["score"][k], (name, band, k)


# ---- 4. the table builders, by hand from the cited formulas ----
def test_table_builders():
    # QualCost(2, 6) = 2 + int(min(q, 40) / 40.0f * 4): 9 -> int(0.9), 10 -> int(1.0), 39 -> int(3.9)
    t = Q.qual_cost(2, 6)
    assert [t[q] for q in (0, 9, 10, 39, 40, 41, 255)] == [2, 2, 3, 5, 6, 6, 6]
    assert Q.constant_cost(7, 3) == [7, 7, 7]
    r = Q.rounded_qual_cost()
    assert [r[q] for q in (0, 4, 5, 14, 15, 24, 25, 40, 255)] == [0, 0, 10, 10, 20, 20, 30, 30, 30]
    assert DEFAULT.match_t == [0] * 256 and DEFAULT.mismatch_t[:11] == [-2] * 10 + [-3]
    assert (DEFAULT.gap_open, DEFAULT.gap_ext, DEFAULT.levels) == (-8, -3, 256)


# ---- 5. the GPU tests' inputs: a kernel that ignores the qualities cannot pass ----
def test_inputs_depend_on_the_qualities():
    d = inputs()
    flat = d["flat"]
    assert len(d["pats"]) == N_PAIRS and (flat > 40).sum() >= 100 and (flat > 41).sum() >= 100 and flat.max() == 255
    assert sum(len(p) == 0 for p in d["pats"]) >= 5 and sum(len(p) == 1 for p in d["pats"]) >= 5
    assert sum(len(t) < len(p) for p, t in zip(d["pats"], d["texts"])) >= 20
    for type_ in (GLOBAL, SEMI):
        got = want("default", type_, 15)["score"]
        for mm in (-2, -6):
            const, _ = Q.best_sinks(Q.constant_scheme(0, mm, -8, -3), type_, 15, d["pats"], d["quals"], d["texts"])
            n_diff = int((const != got).sum())
            print(f"type {type_} mismatch {mm}: {n_diff} of {N_PAIRS} scores differ")
            assert n_diff * 10 >= N_PAIRS, (type_, mm, n_diff)
    got = want("local_default", LOCAL, 15)
    for mm in (-2, -6):
        cs, ck = Q.best_sinks(Q.constant_scheme(2, mm, -8, -3), LOCAL, 15, d["pats"], d["quals"], d["texts"])
        assert int((cs != got["score"]).sum()) * 10 >= N_PAIRS
        assert (ck != got["sink"]).any(axis=1).sum() >= 1


# ---- 6. plan names ----
def _env(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def test_plan_names_match_the_golden_file():
    import json
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "nv_qual_plan_names.json")))
    q = nv_quals(DEFAULT, None)
    for row in gold["names"]:
        got = G.nv_describe_banded_qual_plan(gotoh(TYPES[row["type"]], DEFAULT), q, row["band"], row["max_p"],
                                             row["text_bits"], row["traceback"])
        assert got == row["name"], row


def test_plan_family():
    name = G.nv_describe_banded_qual_plan
    q = nv_quals(DEFAULT, None)
    al = gotoh(LOCAL, DEFAULT)
    assert name(al, q, 16, 150) == "nvbio_banded16_qual_gotoh_local_b16_sink"
    assert name(gotoh(SEMI, DEFAULT), q, 32, 150) == "nvbio_banded16_qual_gotoh_semi_b32_sink"
    assert name(al, nv_quals(S2, None), 7, 150) == "nvbio_banded16_qual_gotoh_local_b8_sink"
    # the aligner's own match / mismatch are not read: values outside every window change nothing
    assert name(G.NvAligner(G.NV_GOTOH, LOCAL, 30000, -30000, -8, -3), q, 16, 150) == \
        "nvbio_banded16_qual_gotoh_local_b16_sink"
    for bits in (4, 8):
        assert name(al, q, 16, 150, text_bits=bits) == "nvbio_banded_qual_gotoh_local_b16_sink"
    wide = G.NvQuals(None, [2, 250], [-1, -6])            # a level with match - mismatch > 255
    assert name(al, wide, 16, 150) == "nvbio_banded_qual_gotoh_local_b16_sink"
    crossed = G.NvQuals(None, [2, -3], [-1, -2])          # a level with match < mismatch
    assert name(al, crossed, 16, 150) == "nvbio_banded_qual_gotoh_local_b16_sink"
    assert name(al, q, 16, 0) == "nvbio_banded_qual_gotoh_local_b16_sink"
    assert name(al, q, 16, 3000) == "nvbio_banded_qual_gotoh_local_b16_sink"      # outside the 16-bit window
    try:
        _env("GASALX_NVB16", "0")
        assert name(al, q, 16, 150) == "nvbio_banded_qual_gotoh_local_b16_sink"
    finally:
        _env("GASALX_NVB16", None)
    assert name(al, q, 15, 150, traceback=True) == "nvbio_banded_qual_traceback_gotoh_local_b15"
    assert name(al, q, 14, 150, traceback=True) == "nvbio_banded_qual_traceback_gotoh_local_b16"


# ---- 7. the order of the checks: each case fails one step, everything before it passes ----
def test_check_order():
    name = G.nv_describe_banded_qual_plan
    ok_q = nv_quals(DEFAULT, None)
    al = gotoh(LOCAL, DEFAULT)

    class NoTable(G.NvQuals):
        def cstruct(self):
            c = super().cstruct()
            c.mismatch = None
            return c

    bad_levels = G.NvQuals(None, [0], [0])
    bad_levels.levels = 0
    sw = G.NvAligner(G.NV_SW, LOCAL, 1, -1, 0, 0, -1, -1)
    # 1. a NULL table, with everything after it wrong too
    with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): .*null argument"):
        name(G.NvAligner(7, LOCAL), NoTable(None, [0], [0]), 99, 150, text_bits=3)
    # 2. a bad aligner (then: levels 0, band 99, bits 3)
    with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): .*bad aligner"):
        name(G.NvAligner(7, LOCAL), bad_levels, 99, 150, text_bits=3)
    with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): .*bad aligner"):
        name(G.NvAligner(G.NV_SW, 5), bad_levels, 99, 150, text_bits=3)
    # 3. not the Gotoh aligner
    for other in (sw, G.NvAligner(G.NV_ED, LOCAL)):
        with pytest.raises(RuntimeError, match=rf"\({EUNSUPPORTED}\): .*edit distance has no scheme.*Smith-Waterman"):
            name(other, bad_levels, 99, 150, text_bits=3)
    # 4. levels
    with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): .*quality levels must be 1\.\.256"):
        name(al, bad_levels, 99, 150, text_bits=3)
    with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): .*quality levels must be 1\.\.256"):
        name(al, G.NvQuals(None, [0] * 257, [0] * 257), 99, 150, text_bits=3)
    # 5. the band
    for band in (1, 33):
        with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): .*band length must be 2\.\.32"):
            name(al, ok_q, band, 150, text_bits=3)
    # 6. the symbol bits
    with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): .*symbol bits must be 2, 4 or 8"):
        name(al, ok_q, 16, 150, text_bits=3)
    assert name(al, ok_q, 16, 150)


# ---- 8. the header: routing against stubs, and the refusals ----
def _hipcc(tmp_path, *extra):
    return ["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
            os.path.join(ROOT, "tools", "nvbio_qual_header_check.cpp"), "-o", str(tmp_path / "check"), *extra]


def test_header_builds_the_tables_and_routes_the_calls(tmp_path):
    subprocess.run(_hipcc(tmp_path), check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(tmp_path / "check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("macro,message", [
    ("CHECK_SW_OVER_QUALS_REFUSED", "nothing in the tree drives Smith-Waterman with qualities"),
    ("CHECK_FULL_SCORE_OVER_QUALS_REFUSED", "the full-DP scorer and traceback have no quality kernels"),
    ("CHECK_FREE_SCORE_OVER_QUALS_REFUSED", "the full-DP scorer and traceback have no quality kernels"),
    ("CHECK_FULL_TRACEBACK_OVER_QUALS_REFUSED", "the full-DP scorer and traceback have no quality kernels")])
def test_refusals_do_not_compile(tmp_path, macro, message):
    r = subprocess.run(_hipcc(tmp_path, "-fsyntax-only", "-D" + macro), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "static assertion failed" in r.stderr and message in r.stderr, r.stderr

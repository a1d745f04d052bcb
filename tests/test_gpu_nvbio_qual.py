"""GPU parity of the quality-aware banded Gotoh kernels (gasalx_nv_banded_qual_*,
csrc/nvbanded_qual.hpp): the scorer's scores and sinks, packed and int32, and the traceback's five
outputs, bit-exact against tests/nvbio_qual_model.py (itself tied to the oracle under constant tables
and replayed in test_nvbio_qual_model.py), on inputs whose answers depend on the qualities
(test_inputs_depend_on_the_qualities there)."""
import os
import subprocess

import numpy as np
import pytest

import gasal_ffi as G
import nvbio_banded_sinks_model as R
import nvbio_qual_model as Q
import oracle as O
from test_nvbio_qual_model import (BANDS, DEFAULT, EINVAL, ERANGE, LOCAL_DEFAULT, N_PAIRS, TYPES, _env, gotoh, inputs,
                                   nv_quals, want)

pytestmark = pytest.mark.gpu

GLOBAL, LOCAL, SEMI = G.NV_GLOBAL, G.NV_LOCAL, G.NV_SEMI_GLOBAL
# inside the packed window with patterns past 1,000 symbols: every magnitude <= 6
MIXED = Q.Scheme(Q.constant_cost(2), [-v for v in Q.qual_cost(2, 6)], -5, -3)


def scheme_of(type_):
    return ("local_default", LOCAL_DEFAULT) if type_ == LOCAL else ("default", DEFAULT)


def _same_scores(got, wanted, what):
    sc, sk = got
    bad = np.nonzero((sc != wanted["score"]) | (sk != wanted["sink"]).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size}/{len(sc)} differ, first #{bad[0]}: gpu {sc[bad[0]]} {sk[bad[0]]} "
                           f"model {wanted['score'][bad[0]]} {wanted['sink'][bad[0]]}")


def _same_traceback(got, wanted, what):
    for f in ("score", "source", "sink"):
        bad = np.nonzero((got[f] != wanted[f]).reshape(len(got[f]), -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {f} of {bad.size} pairs differ, first #{bad[0]}: gpu {got[f][bad[0]]} model {wanted[f][bad[0]]}"
    bad = [k for k, (a, b) in enumerate(zip(got["ops"], wanted["ops"])) if not np.array_equal(a, b)]
    assert not bad, f"{what}: ops of {len(bad)} pairs differ, first #{bad[0]}"


def _all_three(engine, sc, type_, band, P, T, flat, wanted, what, max_p):
    """The packed scorer, the int32 scorer and the traceback against the model's traceback dict."""
    al, q = gotoh(type_, sc), nv_quals(sc, flat)
    assert G.nv_describe_banded_qual_plan(al, q, band, max_p).startswith("nvbio_banded16_qual_")
    _same_scores(engine.nv_banded_qual_score_host(al, q, band, P, T), wanted, f"{what} packed")
    try:
        _env("GASALX_NVB16", "0")
        assert G.nv_describe_banded_qual_plan(al, q, band, max_p).startswith("nvbio_banded_qual_")
        _same_scores(engine.nv_banded_qual_score_host(al, q, band, P, T), wanted, f"{what} int32")
    finally:
        _env("GASALX_NVB16", None)
    _same_traceback(engine.nv_banded_qual_traceback_host(al, q, band, P, T), wanted, f"{what} traceback")


def _mixed(n, seed):
    """n pairs whose lane partners differ in length, every seventh pattern past 1,000 symbols, with
    qualities; empty and one-symbol patterns and texts shorter than their patterns come from tie_pairs."""
    pats, texts = R.tie_pairs(seed, n=n, max_m=150, symbols=5)
    rng = np.random.default_rng(seed + 1)
    for k in range(0, n, 7):
        m = 1001 + int(rng.integers(0, 60))
        texts[k] = rng.integers(0, 4, m + int(rng.integers(0, 20))).astype(np.uint32)
        pats[k] = texts[k][:m].copy()
        sub = rng.random(m) < 0.08
        pats[k][sub] = rng.integers(0, 5, int(sub.sum()))
    quals = Q.attach_quals(seed, pats)
    return dict(pats=pats, texts=texts, quals=quals, flat=Q.flat_quals(quals), P=G.PackedSet.pack(pats, 4, True),
                T=G.PackedSet.pack(texts, 2, False), max_p=max(len(p) for p in pats))


_long = {}


def long_inputs():
    if not _long:
        _long.update(_mixed(140, 0x10A6))
    return _long


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("tname", list(TYPES))
def test_every_instance(engine, tname, band):
    # every BMAX instance at and inside its edges, the exact 7 / 15 / 31 traceback instances; then the same
    # with lane partners of very different lengths, patterns past 1,000 symbols inside the packed window
    type_ = TYPES[tname]
    d = inputs()
    name, sc = scheme_of(type_)
    _all_three(engine, sc, type_, band, d["P"], d["T"], d["flat"], want(name, type_, band), f"{tname} band {band}", 200)
    m = long_inputs()
    wanted = Q.traceback(MIXED, type_, band, m["pats"], m["quals"], m["texts"])
    _all_three(engine, MIXED, type_, band, m["P"], m["T"], m["flat"], wanted, f"long {tname} band {band}", m["max_p"])


@pytest.mark.parametrize("n", [1, 2, 3, 257])
def test_pair_counts(engine, n):
    # the odd half of a packed lane, and a last block that is not full (257: one thread of the second
    # block holds a pair; every other thread of it must still reach the barrier and store nothing)
    m = _mixed(n, 0x16 + n)
    for type_ in (GLOBAL, LOCAL, SEMI):
        wanted = Q.traceback(MIXED, type_, 15, m["pats"], m["quals"], m["texts"])
        _all_three(engine, MIXED, type_, 15, m["P"], m["T"], m["flat"], wanted, f"n {n} type {type_}", m["max_p"])


@pytest.mark.parametrize("tname", list(TYPES))
def test_constant_tables_equal_the_plain_entry_points(engine, tname):
    # constant tables: the outputs of gasalx_nv_banded_score_sinks_* and gasalx_nv_banded_traceback_* on the
    # same pairs, which are run too (and still equal the oracle: untouched)
    type_ = TYPES[tname]
    d = inputs()
    for (a, b, go, ge), levels in (((2, -1, -2, -1), 41), ((5, -4, -10, -1), 1)):
        al = G.NvAligner(G.NV_GOTOH, type_, a, b, go, ge)
        sc = Q.constant_scheme(a, b, go, ge, levels)
        q = nv_quals(sc, d["flat"])
        blind = G.NvAligner(G.NV_GOTOH, type_, 77, 78, go, ge)          # match / mismatch must not be read
        for band in (7, 12, 32):
            o = O.nv_banded_traceback(al, band, d["P"], d["T"])
            plain_sc = engine.nv_banded_score_sinks_host(al, band, d["P"], d["T"])
            plain_tb = engine.nv_banded_traceback_host(al, band, d["P"], d["T"])
            _same_scores(plain_sc, o, f"plain band {band}")
            _same_traceback(plain_tb, o, f"plain band {band}")
            got = engine.nv_banded_qual_score_host(blind, q, band, d["P"], d["T"])
            assert np.array_equal(got[0], plain_sc[0]) and np.array_equal(got[1], plain_sc[1]), band
            try:
                _env("GASALX_NVB16", "0")
                got = engine.nv_banded_qual_score_host(blind, q, band, d["P"], d["T"])
            finally:
                _env("GASALX_NVB16", None)
            assert np.array_equal(got[0], plain_sc[0]) and np.array_equal(got[1], plain_sc[1]), band
            _same_traceback(engine.nv_banded_qual_traceback_host(blind, q, band, d["P"], d["T"]), plain_tb, f"band {band}")


def _subset(n):
    d = inputs()
    pats, texts, quals = d["pats"][:n], d["texts"][:n], d["quals"][:n]
    return pats, texts, quals, G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, 2, False)


@pytest.mark.parametrize("levels", [1, 41, 256])
def test_levels_and_extreme_qualities(engine, levels):
    # a table whose last entry differs from the rest, so the clamp of a byte >= levels is visible;
    # qualities as generated, all 0 and all 255
    pats, texts, quals, P, T = _subset(300)
    mism = [-2] * (levels - 1) + [-7]
    sc = Q.Scheme([1] * levels, mism, -6, -2)
    for kind in ("own", 0, 255):
        qs = quals if kind == "own" else [np.full(len(p), kind, np.uint8) for p in pats]
        for type_ in (LOCAL, SEMI):
            wanted = Q.traceback(sc, type_, 15, pats, qs, texts)
            _all_three(engine, sc, type_, 15, P, T, Q.flat_quals(qs), wanted, f"levels {levels} quals {kind}", 200)
    if levels > 1:
        a = Q.best_sinks(sc, SEMI, 15, pats, [np.full(len(p), levels - 2, np.uint8) for p in pats], texts)[0]
        b = Q.best_sinks(sc, SEMI, 15, pats, [np.full(len(p), 255, np.uint8) for p in pats], texts)[0]
        assert (a != b).sum() >= 30                                     # the last entry is seen


@pytest.mark.parametrize("bits,big", [(2, True), (2, False), (4, True), (4, False), (8, True), (8, False)])
def test_text_encodings(engine, bits, big):
    pats, texts, quals, P, _ = _subset(300)
    T = G.PackedSet.pack(texts, bits, big)
    flat = Q.flat_quals(quals)
    for type_ in (GLOBAL, LOCAL, SEMI):
        _, sc = scheme_of(type_)
        al, q = gotoh(type_, sc), nv_quals(sc, flat)
        wanted = Q.traceback(sc, type_, 17, pats, quals, texts)
        _same_scores(engine.nv_banded_qual_score_host(al, q, 17, P, T), wanted, f"type {type_}")
        _same_traceback(engine.nv_banded_qual_traceback_host(al, q, 17, P, T), wanted, f"type {type_}")


@pytest.mark.parametrize("bits", [2, 8])
def test_shared_text(engine, bits):
    # one text for every pattern (offsets NULL); the longest pattern is longer than the text
    rng = np.random.default_rng(0x5A)
    text = np.tile(rng.permutation(4)[:3], 30).astype(np.uint32)
    pats = [text[st:st + m].copy() for m in (0, 1, 30, 60, 88, 89, 90) for st in (0, 1)] + [np.tile(text, 2)[:91]]
    for p in pats:
        p[rng.random(len(p)) < 0.1] = 3
    quals = Q.attach_quals(0x5A, pats)
    P = G.PackedSet.pack(pats, 4, True)
    T = G.PackedSet.pack([text], bits, False, shared=True)
    for type_ in (GLOBAL, LOCAL, SEMI):
        _, sc = scheme_of(type_)
        al, q = gotoh(type_, sc), nv_quals(sc, Q.flat_quals(quals))
        wanted = Q.traceback(sc, type_, 9, pats, quals, [text] * len(pats))
        _same_scores(engine.nv_banded_qual_score_host(al, q, 9, P, T), wanted, f"type {type_}")
        _same_traceback(engine.nv_banded_qual_traceback_host(al, q, 9, P, T), wanted, f"type {type_}")
        assert wanted["score"][-1] == Q.INT32_MIN


def test_pattern_offsets_off_the_quality_words():
    # the inputs' pattern offsets fall on every residue of 4: quality words are read unaligned to the patterns
    off = np.asarray(inputs()["P"].offsets[:-1], np.int64)
    assert all((off % 4 == r).sum() >= 50 for r in range(4))


def _device_sets(P, T, flat, lead):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")
    keep = [dev(P.words), dev(P.offsets), dev(T.words), dev(T.offsets)]
    # the quality bytes `lead` bytes into their allocation: the array itself need not be word-aligned
    dq = torch.from_numpy(np.concatenate([np.zeros(lead, np.uint8), flat, np.zeros(8, np.uint8)])).to("cuda:0")
    keep.append(dq)
    mk = lambda S, w, off: {"words": w.data_ptr(), "offsets": off.data_ptr(), "length": 0, "bits": S.bits,
                            "big_endian": S.big_endian}
    return keep, mk(P, keep[0], keep[1]), mk(T, keep[2], keep[3]), dq.data_ptr() + lead


@pytest.mark.parametrize("max_pattern_len,lead", [(0, 0), (256, 1), (256, 3)])
def test_device_entry_points_on_a_stream(engine, max_pattern_len, lead):
    # the bound read back (0) or given as an upper bound; each optional output alone leaves the other
    # buffer untouched; the quality array is a device pointer, at any byte alignment
    import torch
    d = inputs()
    P, T, n = d["P"], d["T"], N_PAIRS
    name, sc = scheme_of(LOCAL)
    al = gotoh(LOCAL, sc)
    wanted = want(name, LOCAL, 31)
    keep, pat, txt, qptr = _device_sets(P, T, d["flat"], lead)
    q = nv_quals(sc, None, quals_ptr=qptr)
    stream = torch.cuda.Stream()
    fresh = lambda m, dt=torch.int32: torch.full((m,), -77, dtype=dt, device="cuda:0")
    for want_sc, want_sk in ((True, True), (True, False), (False, True)):
        dsc, dsk = fresh(n), fresh(2 * n)
        torch.cuda.synchronize()
        engine.nv_banded_qual_score_device_ptrs(al, q, 31, n, pat, txt, dsc.data_ptr() if want_sc else 0,
                                                dsk.data_ptr() if want_sk else 0, max_pattern_len=max_pattern_len,
                                                stream=stream.cuda_stream)
        stream.synchronize()
        sc_, sk_ = dsc.cpu().numpy(), dsk.cpu().numpy().view(np.uint32).reshape(n, 2)
        assert np.array_equal(sc_, wanted["score"]) if want_sc else (sc_ == -77).all()
        assert np.array_equal(sk_, wanted["sink"]) if want_sk else (dsk.cpu().numpy() == -77).all()
    with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): null argument"):
        engine.nv_banded_qual_score_device_ptrs(al, q, 31, n, pat, txt, 0, 0)
    stride = 2 * max(max_pattern_len, 200) + 31                        # the rule holds for the bound that is given
    outs = dict(score=fresh(n), source=fresh(2 * n), sink=fresh(2 * n), ops=torch.zeros(n * stride, dtype=torch.uint8, device="cuda:0"), n_ops=fresh(n))
    torch.cuda.synchronize()
    engine.nv_banded_qual_traceback_device_ptrs(al, q, 31, n, pat, txt, {k: v.data_ptr() for k, v in outs.items()}, stride,
                                                max_pattern_len=max_pattern_len, stream=stream.cuda_stream)
    stream.synchronize()
    nops = outs["n_ops"].cpu().numpy().view(np.uint32)
    ops = outs["ops"].cpu().numpy()
    got = dict(score=outs["score"].cpu().numpy(), source=outs["source"].cpu().numpy().view(np.uint32).reshape(n, 2),
               sink=outs["sink"].cpu().numpy().view(np.uint32).reshape(n, 2),
               ops=[ops[k * stride:k * stride + int(nops[k])] for k in range(n)])
    _same_traceback(got, wanted, "device traceback")


def test_traceback_in_chunks(engine):
    d = inputs()
    name, sc = scheme_of(SEMI)
    al, q = gotoh(SEMI, sc), nv_quals(sc, d["flat"])
    per = G.nv_banded_traceback_workspace(200, 15, 1)
    try:
        _env("GASALX_NV_TB_BUDGET", str(per * (N_PAIRS // 3 + 1)))
        assert -(-N_PAIRS // (N_PAIRS // 3 + 1)) == 3
        got = engine.nv_banded_qual_traceback_host(al, q, 15, d["P"], d["T"])
    finally:
        _env("GASALX_NV_TB_BUDGET", None)
    _same_traceback(got, want(name, SEMI, 15), "three chunks")


def test_range_rules_come_last(engine):
    # step 7 of the checks: everything before it passes.  (max pattern + band + 3) * the largest magnitude
    # (here a table entry, 200) above 32736; then the ops_stride rule
    pats, texts, quals, P, T = _subset(300)
    flat = Q.flat_quals(quals)
    big = G.NvQuals(flat, [0, 200], [-1, -2])
    al = G.NvAligner(G.NV_GOTOH, SEMI, 0, 0, -8, -3)
    assert (200 + 15 + 3) * 200 > 32736
    with pytest.raises(RuntimeError, match=rf"\({ERANGE}\): banded traceback: scores would leave"):
        engine.nv_banded_qual_traceback_host(al, big, 15, P, T)
    with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): banded traceback: ops_stride"):
        engine.nv_banded_qual_traceback_host(al, nv_quals(DEFAULT, flat), 15, P, T, ops_stride=100)
    # the scorer has no range rule of its own: outside the packed window it runs in int32
    sc = Q.Scheme([0, 200], [-1, -2], -8, -3)
    _same_scores(engine.nv_banded_qual_score_host(al, big, 15, P, T), Q.traceback(sc, SEMI, 15, pats, quals, texts), "int32")


def test_client_tool_agrees_with_itself():
    # tools/nvbio_qual_test (client of include/nvbio_batched.h alone): nvBowtie's default scheme under the
    # banded scorer with sinks against the banded traceback, and every alignment replayed on the host
    prog = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "nvbio_qual_test")
    r = subprocess.run([prog, "2000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "2000 pairs" in r.stdout and " 0 differ" in r.stdout and " 0 replay to another score" in r.stdout
    assert len(r.stdout.splitlines()) == 1

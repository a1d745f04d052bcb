"""GPU parity of nvbio's banded Myers aligner (gasalx_nv_banded_myers_*, csrc/nvmyers.hpp) through
the flat C API: scores and BestSink positions bit-exact against the cited restatement of
banded_myers (tests/nvbio_myers_model.py, pinned by test_nvbio_myers_model.py).  Lengths sit where
the function changes course: pattern lengths around the band and the 32-bit register, text lengths
that skip the pair (pl - 1), give phase 2 one column (pl), and end it at s = -1 before and after
the text runs out (pl + band - 1, pl + band, pl + band + 5)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gasal_ffi as G
import nvbio_myers_model as R

pytestmark = pytest.mark.gpu

SEMI, GLOBAL, LOCAL = G.NV_SEMI_GLOBAL, G.NV_GLOBAL, G.NV_LOCAL
TYPES = {"semi": SEMI, "global": GLOBAL}
BANDS = (2, 7, 15, 31, 32)
ALPHABETS = (2, 4, 5)
EINVAL, EUNSUPPORTED = -1, -5


def _pattern_lens(band):
    return sorted({1, 2, band - 1, band, band + 1, 33, 100, 150} - {0})


def _text_lens(pl, band):
    return (pl - 1, pl, pl + 1, pl + band - 1, pl + band, pl + band + 5)


def _pair(rng, pl, tl, symbols):
    """A pattern of pl symbols related to a text of tl: cut from it a few columns in, with ~5%
    substitutions; `symbols`: the codes to draw from."""
    t = rng.choice(symbols, tl)
    if tl >= pl:
        st = int(rng.integers(0, min(tl - pl, 3) + 1))
        p = t[st:st + pl].copy()
    else:
        p = np.concatenate([t, rng.choice(symbols, pl - tl)])
    sub = rng.random(pl) < 0.05
    p[sub] = rng.choice(symbols, int(sub.sum()))
    return p.astype(np.uint32), t.astype(np.uint32)


def _length_grid(rng, band, symbols):
    pats, texts = [], []
    for pl in _pattern_lens(band):
        for tl in _text_lens(pl, band):
            p, t = _pair(rng, pl, tl, symbols)
            pats.append(p); texts.append(t)
    return pats, texts


def _compare(engine, type_, alphabet, band, P, T):
    rs, rk = R.batch(type_, alphabet, band, P, T)
    sc, sk = engine.nv_banded_myers_host(type_, alphabet, band, P, T)
    bad = np.nonzero((sc != rs) | (sk != rk).any(axis=1))[0]
    assert bad.size == 0, (f"{bad.size}/{len(sc)} differ, first #{bad[0]} (M={P.offsets[bad[0] + 1] - P.offsets[bad[0]]}): "
                           f"gpu={sc[bad[0]]} {sk[bad[0]]} model={rs[bad[0]]} {rk[bad[0]]}")
    return rs, rk


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("alphabet", ALPHABETS)
@pytest.mark.parametrize("tname", list(TYPES))
def test_length_grid(engine, tname, alphabet, band):
    # every pattern length against every text length; 2-bit strings for the 2- and 4-letter
    # alphabets, 4-bit big-endian patterns (nvbio's DNA_N reads) with N for the 5-letter one
    rng = np.random.default_rng(1000 * band + 10 * alphabet + TYPES[tname])
    symbols = np.arange(alphabet)
    pats, texts = _length_grid(rng, band, symbols)
    pbits = 4 if alphabet == 5 else 2
    P = G.PackedSet.pack(pats, pbits, True)
    T = G.PackedSet.pack(texts, 4 if alphabet == 5 else 2, False)
    rs, rk = _compare(engine, TYPES[tname], alphabet, band, P, T)
    # the grid holds the skipped pairs and, beside them, pairs that report
    skipped = np.array([len(t) < len(p) for p, t in zip(pats, texts)])
    assert skipped.any() and (rs[skipped] == R.INT32_MIN).all() and (rk[skipped] == R.NO_SINK).all()
    assert (rs[~skipped] > R.INT32_MIN).all()
    assert G.nv_describe_myers_plan(TYPES[tname], alphabet, band) == f"nvbio_myers_{tname}_a{alphabet}"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_pair_counts(engine, n):
    # one pair, a wave less one, a wave, a wave and one, more than one 256-thread block
    rng = np.random.default_rng(0xB0 + n)
    pats, texts = [], []
    for _ in range(n):
        pl = int(rng.integers(1, 151))
        p, t = _pair(rng, pl, pl + int(rng.integers(-1, 40)), np.arange(5))
        pats.append(p); texts.append(t)
    P, T = G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, 4, False)
    for type_ in (SEMI, GLOBAL):
        _compare(engine, type_, 5, 31, P, T)


def _tight(seqs, bits, big):
    """A set whose last string ends exactly at the end of the last word, with no word after it: the
    last string is lengthened to the word boundary with its own first symbol."""
    per = 32 // bits
    seqs = [np.asarray(s, np.uint32) for s in seqs]
    total = sum(len(s) for s in seqs)
    pad = (-total) % per
    seqs[-1] = np.concatenate([seqs[-1], np.full(pad, seqs[-1][0], np.uint32)])
    S = G.PackedSet.pack(seqs, bits, big)
    n_words = (total + pad) // per
    assert int(S.offsets[-1]) == n_words * per
    return seqs, G.PackedSet(S.words[:n_words].copy(), S.offsets, 0, bits, big)


LAYOUTS = [(pb, pe, tb, te) for pb, tb in ((2, 2), (4, 2), (2, 4), (4, 4), (8, 8), (8, 4), (4, 8))
           for pe, te in ((True, False), (False, True))] + [(2, True, 2, True), (8, False, 8, False)]


@pytest.mark.parametrize("pbits,pbig,tbits,tbig", LAYOUTS,
                         ids=[f"p{pb}{'be' if pe else 'le'}-t{tb}{'be' if te else 'le'}" for pb, pe, tb, te in LAYOUTS])
def test_string_layouts(engine, pbits, pbig, tbits, tbig):
    # 2-, 4- and 8-bit strings of both endiannesses; odd lengths, so pairs start at symbol offsets
    # that are not word-aligned; the sets end exactly at their last word.  Symbols use every bit of
    # the packing: under alphabet 5 that is N (4) and codes above 4 in patterns and texts, under
    # alphabets 4 and 2 codes with bits above the mask.
    rng = np.random.default_rng(0xC0 + pbits * 16 + tbits + (2 if pbig else 0) + (1 if tbig else 0))
    band = 15
    lens = [(1, 1), (3, 9), (5, 4), (7, 21), (14, 29), (15, 30), (16, 31), (33, 47), (37, 60), (100, 131), (9, 9)]
    psym, tsym = np.arange(min(1 << pbits, 12)), np.arange(min(1 << tbits, 12))
    pats, texts = [], []
    for pl, tl in lens:
        p, t = _pair(rng, pl, tl, np.arange(4))
        # sprinkle the packing's other codes over both strings
        hp, ht = rng.random(pl) < 0.15, rng.random(tl) < 0.15
        p[hp] = rng.choice(psym, int(hp.sum()))
        t[ht] = rng.choice(tsym, int(ht.sum()))
        pats.append(p); texts.append(t)
    pats, P = _tight(pats, pbits, pbig)
    texts, T = _tight(texts, tbits, tbig)
    assert any(int(o) % (32 // pbits) for o in P.offsets[1:-1]) and any(int(o) % (32 // tbits) for o in T.offsets[1:-1])
    if pbits > 2:
        assert max(int(p.max()) for p in pats) > 4 and any((p == 4).any() for p in pats)
    if tbits > 2:
        assert max(int(t.max()) for t in texts) > 4 and any((t == 4).any() for t in texts)
    for alphabet in ALPHABETS:
        for type_ in (SEMI, GLOBAL):
            _compare(engine, type_, alphabet, band, P, T)


def test_shared_text(engine):
    # one text for every pattern (offsets NULL), as the neighbouring entry points take it
    rng = np.random.default_rng(0xD1)
    text = rng.integers(0, 4, 70).astype(np.uint32)
    pats = [text[:m].copy() for m in (1, 30, 40, 69, 70)] + [rng.integers(0, 4, 71).astype(np.uint32)]
    P = G.PackedSet.pack(pats, 4, True)
    T = G.PackedSet.pack([text], 2, False, shared=True)
    for type_ in (SEMI, GLOBAL):
        rs, _ = _compare(engine, type_, 4, 31, P, T)
        assert rs[-1] == R.INT32_MIN


def test_scores_only_sinks_only(engine):
    rng = np.random.default_rng(0xD2)
    pats, texts = _length_grid(rng, 7, np.arange(5))
    P, T = G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, 4, True)
    sc, sk = engine.nv_banded_myers_host(SEMI, 5, 7, P, T)
    only_sc, none_sk = engine.nv_banded_myers_host(SEMI, 5, 7, P, T, sinks=False)
    none_sc, only_sk = engine.nv_banded_myers_host(SEMI, 5, 7, P, T, scores=False)
    assert none_sk is None and none_sc is None
    assert np.array_equal(only_sc, sc) and np.array_equal(only_sk, sk)
    rs, rk = R.batch(SEMI, 5, 7, P, T)
    assert np.array_equal(sc, rs) and np.array_equal(sk, rk)


def _device_sets(P, T):
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")
    keep = [dev(P.words), dev(P.offsets), dev(T.words), dev(T.offsets)]
    mk = lambda S, w, off: {"words": w.data_ptr(), "offsets": off.data_ptr(), "length": 0, "bits": S.bits,
                            "big_endian": S.big_endian}
    return keep, mk(P, keep[0], keep[1]), mk(T, keep[2], keep[3])


@pytest.mark.parametrize("tname", list(TYPES))
def test_device_entry_point_on_a_stream(engine, tname):
    import torch
    type_ = TYPES[tname]
    rng = np.random.default_rng(0xD3)
    pats, texts = _length_grid(rng, 31, np.arange(5))
    P, T = G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, 4, False)
    rs, rk = R.batch(type_, 5, 31, P, T)
    n = P.n
    keep, pat, txt = _device_sets(P, T)
    stream = torch.cuda.Stream()
    fresh = lambda m: torch.full((m,), -77, dtype=torch.int32, device="cuda:0")
    for want_sc, want_sk in ((True, True), (True, False), (False, True)):
        dsc, dsk = fresh(n), fresh(2 * n)
        torch.cuda.synchronize()
        engine.nv_banded_myers_device_ptrs(type_, 5, 31, n, pat, txt, dsc.data_ptr() if want_sc else 0,
                                           dsk.data_ptr() if want_sk else 0, max_pattern_len=150,
                                           stream=stream.cuda_stream)
        stream.synchronize()
        sc, sk = dsc.cpu().numpy(), dsk.cpu().numpy().view(np.uint32).reshape(n, 2)
        # the output asked for is the model's; the other is untouched
        assert np.array_equal(sc, rs) if want_sc else (sc == -77).all()
        assert np.array_equal(sk, rk) if want_sk else (dsk.cpu().numpy() == -77).all()


ERRORS = [("local", LOCAL, 5, 31, EUNSUPPORTED, "no LOCAL form"),
          ("alphabet_3", SEMI, 3, 31, EINVAL, "alphabet size must be 2, 4 or 5"),
          ("band_1", SEMI, 5, 1, EINVAL, "band length must be 2..32"),
          ("band_33", SEMI, 5, 33, EINVAL, "band length must be 2..32")]


def _raw_host(engine, type_, alphabet, band, P, T, sc, sk):
    return G.lib().gasalx_nv_banded_myers_host(engine._h, ctypes.c_int32(type_), ctypes.c_uint32(alphabet),
                                               ctypes.c_uint32(band), ctypes.c_uint32(P.n),
                                               ctypes.byref(P.cstruct()), ctypes.c_uint64(len(P.words)),
                                               ctypes.byref(T.cstruct()), ctypes.c_uint64(len(T.words)),
                                               G._p(sc), G._p(sk))


@pytest.mark.parametrize("name,type_,alphabet,band,code,text", ERRORS, ids=[e[0] for e in ERRORS])
def test_refusals(engine, name, type_, alphabet, band, code, text):
    import torch
    pats, texts = _length_grid(np.random.default_rng(0xD4), 7, np.arange(4))
    P, T = G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, 2, False)
    n = P.n
    # the host entry: the code, the text, and the caller's arrays as they were
    sc, sk = np.full(n, -77, np.int32), np.full(2 * n, 77, np.uint32)
    assert _raw_host(engine, type_, alphabet, band, P, T, sc, sk) == code
    assert text in G.lib().gasalx_last_error().decode()
    assert (sc == -77).all() and (sk == 77).all()
    # the device entry
    keep, pat, txt = _device_sets(P, T)
    dsc = torch.full((n,), -77, dtype=torch.int32, device="cuda:0")
    dsk = torch.full((2 * n,), -77, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=rf"\({code}\): .*{text}"):
        engine.nv_banded_myers_device_ptrs(type_, alphabet, band, n, pat, txt, dsc.data_ptr(), dsk.data_ptr())
    torch.cuda.synchronize()
    assert (dsc.cpu().numpy() == -77).all() and (dsk.cpu().numpy() == -77).all()
    with pytest.raises(RuntimeError, match=rf"\({code}\)"):
        G.nv_describe_myers_plan(type_, alphabet, band)


def test_both_outputs_null(engine):
    pats, texts = _length_grid(np.random.default_rng(0xD5), 7, np.arange(4))
    P, T = G.PackedSet.pack(pats, 4, True), G.PackedSet.pack(texts, 2, False)
    with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): null argument"):
        engine.nv_banded_myers_host(SEMI, 5, 7, P, T, scores=False, sinks=False)
    keep, pat, txt = _device_sets(P, T)
    with pytest.raises(RuntimeError, match=rf"\({EINVAL}\): null argument"):
        engine.nv_banded_myers_device_ptrs(SEMI, 5, 7, P.n, pat, txt, 0, 0)


def _client_data(n, seed):
    """The pairs tools/nvbio_myers_test.cpp generates: the same LCG, drawn in the same order."""
    state = seed

    def lcg():
        nonlocal state
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        return state >> 16

    reads, genomes = [], []
    for _ in range(n):
        length, start = 50 + lcg() % 101, lcg() % 16
        genome = [lcg() % 4 for _ in range(length + 31)]
        read = []
        for i in range(length):
            r = lcg() % 100
            if r == 0:
                continue
            read.append(lcg() % 5 if r < 5 else genome[start + i])
        reads.append(np.array(read, np.uint32)); genomes.append(np.array(genome, np.uint32))
    return reads, genomes


def test_header_client_makes_qmaps_call():
    # tools/nvbio_myers_test (client of include/nvbio_batched.h alone): batch_banded_alignment_score<31>
    # with make_edit_distance_aligner<SEMI_GLOBAL, MyersTag<5>>(), every score and sink against the model
    n, seed = 200, 0x51A9
    prog = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "nvbio_myers_test")
    r = subprocess.run([prog, str(n), str(seed)], capture_output=True, text=True, check=True)
    got = np.array([[int(v) for v in line.split()] for line in r.stdout.splitlines()], np.int64)
    assert got.shape == (n, 4) and np.array_equal(got[:, 0], np.arange(n))
    reads, genomes = _client_data(n, seed)
    rs, rk = R.batch(SEMI, 5, 31, G.PackedSet.pack(reads, 4, True), G.PackedSet.pack(genomes, 2, False))
    assert np.array_equal(got[:, 1], rs.astype(np.int64))
    assert np.array_equal(got[:, 2:], rk.astype(np.int64))
    assert (rs > -20).all() and (rs < 0).any()     # related pairs: small distances, not all exact

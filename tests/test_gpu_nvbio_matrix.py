"""GPU parity of the matrix-scored Gotoh path (gasalx_nv_matrix_score_*, nvmatrix.hpp) through the
C ABI: scores and BestSink positions bit for bit against tests/nvbio_matrix_model.py (pinned by
test_nvbio_matrix_model.py).  Pattern lengths sit at the lane-group edges of the planned kernel
(G lanes x R rows, read from the plan name), text lengths at the 8-column stripe edges.  Every
comparison runs the sink form and the score-only form."""
import re

import numpy as np
import pytest

import gasal_ffi as G
import nvbio_matrix_model as M
import nvbio_sink_model as R

pytestmark = pytest.mark.gpu

TYPES = list(R.TYPES)


def _shape(name):
    m = re.search(r"^nvbio_matrix_gotoh_(global|local|semi)(_shared)?_G(\d+)R(\d+)(_sink)?$", name)
    assert m, name
    return int(m.group(3)), int(m.group(4))


def _plan(al, n, mp, mt, per_pair=True):
    name = G.nv_describe_matrix_plan(al, n, mp, mt, per_pair_texts=per_pair, sinks=True)
    assert ("_shared" in name) == (not per_pair) and name.endswith("_sink"), name
    assert G.nv_describe_matrix_plan(al, n, mp, mt, per_pair_texts=per_pair) + "_sink" == name
    return _shape(name)


def _max_lens(pats, texts):
    return max(len(p) for p in pats), max(len(t) for t in texts)


def _compare(engine, al, mat, pats, texts, P, T):
    sc, sk = engine.nv_matrix_score_host(al, mat, P, T)
    rs, rk, n_max = M.batch(al, mat, mat.n, pats, texts)
    bad = np.nonzero((sc != rs) | (sk != rk).any(axis=1))[0]
    assert bad.size == 0, (f"{bad.size}/{len(sc)} differ, first #{bad[0]} (M={len(pats[bad[0]])}, "
                           f"N={len(texts[bad[0] % len(texts)])}): gpu={sc[bad[0]]} {sk[bad[0]]} "
                           f"model={rs[bad[0]]} {rk[bad[0]]} {al}")
    # the score-only kernel on the same inputs
    only, none = engine.nv_matrix_score_host(al, mat, P, T, sinks=False)
    assert none is None and np.array_equal(only, rs)
    return sc, sk, n_max


def _simple(type_):
    ref_al = R.aligner("gotoh", type_)
    return ref_al, M.gotoh(type_, ref_al.gap_open, ref_al.gap_ext), M.simple_table(4, ref_al.match, ref_al.mismatch)


def _against_existing_kernel(engine, type_, pats, texts, P, T, tie_share):
    ref_al, al, mat = _simple(type_)
    sc, sk, n_max = _compare(engine, al, mat, pats, texts, P, T)
    esc, esk = engine.nv_score_sinks_host(ref_al, P, T)
    assert np.array_equal(sc, esc) and np.array_equal(sk, esk)
    if tie_share and type_ != "global":
        assert M.tie_share(n_max) >= 0.5


@pytest.mark.parametrize("type_", TYPES)
def test_lane_group_and_stripe_edges(engine, type_):
    # the existing sink test's inputs (tie families included) under the match / mismatch table: the
    # model, and the existing kernel's outputs
    _, al, _ = _simple(type_)
    g, r = _plan(al, 4, 150, 340)
    pats, texts, P, T = R.packed("edge", M.edge_lens(g, r), M.EDGE_SEED)
    mp, mt = _max_lens(pats, texts)
    assert mp == g * r and _plan(al, 4, mp, mt) == (g, r)
    _against_existing_kernel(engine, type_, pats, texts, P, T, tie_share=True)


@pytest.mark.parametrize("type_", TYPES)
def test_one_past_the_shape(engine, type_):
    _, al, _ = _simple(type_)
    g, r = _plan(al, 4, 150, 340)
    g2, r2 = _plan(al, 4, g * r + 1, 340)
    assert g2 * r2 > g * r
    pats, texts, P, T = R.packed("edge", (g * r + 1, r2, r2 + 1), 0xE1, text_lens=(9, 16, 301))
    assert _plan(al, 4, *_max_lens(pats, texts)) == (g2, r2)
    _against_existing_kernel(engine, type_, pats, texts, P, T, tie_share=False)


@pytest.mark.parametrize("type_", TYPES)
def test_pattern_limit_1024(engine, type_):
    _, al, _ = _simple(type_)
    rng = np.random.default_rng(0xE2)
    t = rng.integers(0, 4, 130).astype(np.uint32)
    p = np.concatenate([t] * 8)[:1024].astype(np.uint32)
    pats = [p, np.array([2] * 1023, np.uint32), np.array([1, 3] * 8, np.uint32)]
    texts = [t, np.array([2] * 100, np.uint32), np.array([3, 1] * 20, np.uint32)]
    assert _plan(al, 4, 1024, 130) == (64, 16)
    _against_existing_kernel(engine, type_, pats, texts, G.PackedSet.pack(pats, 4, True),
                             G.PackedSet.pack(texts, 2, False), tie_share=False)


def _random_batch(n_sym, lens, seed, text_lens=R.TEXT_LENS, top=None):
    rng = np.random.default_rng(seed)
    top = top or n_sym
    pats, texts = [], []
    for m in lens:
        for k in text_lens:
            t = rng.integers(0, top, k).astype(np.uint32)
            if k > m and rng.random() < 0.5:               # a noisy copy of a text window: long alignments
                st = int(rng.integers(0, k - m + 1))
                p = t[st:st + m].copy()
                flip = rng.random(m) < 0.1
                p[flip] = rng.integers(0, top, int(flip.sum()))
            else:
                p = rng.integers(0, top, m).astype(np.uint32)
            pats.append(p.astype(np.uint32)); texts.append(t)
    return pats, texts


# (n, pattern bits, pattern big-endian, text bits, text big-endian)
TABLES = {"n24_8bit": (24, 8, False, 8, False), "n4_2bit_texts": (4, 4, True, 2, False),
          "n16_4bit": (16, 4, True, 4, True), "n32_8bit": (32, 8, False, 8, False)}


@pytest.mark.parametrize("case", list(TABLES))
@pytest.mark.parametrize("type_", TYPES)
def test_random_asymmetric_tables(engine, type_, case):
    n, pb, pbig, tb, tbig = TABLES[case]
    al = M.gotoh(type_, -5, -3)
    mat = M.random_table(n, 0xA5 + n)
    assert not np.array_equal(mat.scores, mat.scores.T)
    g, r = _plan(al, n, 150, 340)
    pats, texts = _random_batch(n, M.edge_lens(g, r), 0xB0 + n)
    assert _plan(al, n, *_max_lens(pats, texts)) == (g, r)
    _compare(engine, al, mat, pats, texts, G.PackedSet.pack(pats, pb, pbig), G.PackedSet.pack(texts, tb, tbig))


def test_all_positive_table_local(engine):
    # entries 1..9: every step along a diagonal gains, so a pad row or a pad column (symbol 0, a real
    # symbol) would outscore the real cells of a shorter pair in the same wave
    al = M.gotoh("local", -5, -3)
    rng = np.random.default_rng(0xC1)
    mat = G.NvMatrix(rng.integers(1, 10, (24, 24)).astype(np.int8))
    g, r = _plan(al, 24, 150, 340)
    assert 64 // g >= 2                                    # several pairs per wave
    pats = [rng.integers(0, 24, int(m)).astype(np.uint32) for m in rng.integers(1, g * r + 1, 45)]
    texts = [rng.integers(0, 24, int(k)).astype(np.uint32) for k in rng.integers(1, 201, 45)]
    pats[0], texts[0] = pats[0][:1], texts[0][:1]
    pats[1], texts[1] = rng.integers(0, 24, g * r).astype(np.uint32), rng.integers(0, 24, 200).astype(np.uint32)
    sc, sk, _ = _compare(engine, al, mat, pats, texts, G.PackedSet.pack(pats, 8, False), G.PackedSet.pack(texts, 8, False))
    for k in range(len(pats)):                             # the sink is a real cell
        assert 1 <= sk[k, 0] <= len(texts[k]) and 1 <= sk[k, 1] <= len(pats[k])
    for type_ in ("global", "semi"):                       # real cells never depend on pads there: a smaller batch
        _compare(engine, M.gotoh(type_, -5, -3), mat, pats[:16], texts[:16], G.PackedSet.pack(pats[:16], 8, False),
                 G.PackedSet.pack(texts[:16], 8, False))


@pytest.mark.parametrize("type_", TYPES)
def test_clamp(engine, type_):
    # n = 20 under strings that hold every byte value: symbols >= 20 read as 19
    al = M.gotoh(type_, -4, -2)
    mat = M.random_table(20, 0xD4)
    pats, texts = _random_batch(20, (1, 9, 20, 64), 0xD5, text_lens=(1, 9, 17, 120), top=256)
    assert max(int(p.max()) for p in pats) > 200 and max(int(t.max()) for t in texts) > 200
    P, T = G.PackedSet.pack(pats, 8, False), G.PackedSet.pack(texts, 8, False)
    sc, sk, _ = _compare(engine, al, mat, pats, texts, P, T)
    cp, ct = [np.minimum(p, 19) for p in pats], [np.minimum(t, 19) for t in texts]
    csc, csk = engine.nv_matrix_score_host(al, mat, G.PackedSet.pack(cp, 8, False), G.PackedSet.pack(ct, 8, False))
    assert np.array_equal(sc, csc) and np.array_equal(sk, csk)


@pytest.mark.parametrize("type_", TYPES)
def test_shared_text(engine, type_):
    _, al, _ = _simple(type_)
    g, r = _plan(al, 4, 150, 301, per_pair=False)
    lens = (1, 9, r, g * r)
    pats, texts, P, T = R.packed("shared", lens, 0xE3, n_text=301)
    assert _plan(al, 4, g * r, 301, per_pair=False) == (g, r)
    _against_existing_kernel(engine, type_, pats, texts, P, T, tie_share=False)
    mat = M.random_table(4, 0xE5)
    _compare(engine, M.gotoh(type_, -3, -1), mat, pats, texts, P, R.packed("shared", lens, 0xE3, 4, True, n_text=301)[3])


def test_degenerate_pairs_and_part_filled_block(engine):
    # M = 0 and N = 0 pairs among real ones, 37 pairs: the last block (32 pairs at G = 8) part-filled
    rng = np.random.default_rng(0xF0)
    mat = M.random_table(24, 0xF1)
    pats = [rng.integers(0, 24, int(m)).astype(np.uint32) for m in rng.integers(1, 40, 37)]
    texts = [rng.integers(0, 24, int(k)).astype(np.uint32) for k in rng.integers(1, 90, 37)]
    empty = np.zeros(0, np.uint32)
    pats[0] = empty; texts[0] = rng.integers(0, 24, 9).astype(np.uint32)
    texts[5] = empty
    pats[36] = empty; texts[36] = empty
    pats[35] = empty
    P, T = G.PackedSet.pack(pats, 8, False), G.PackedSet.pack(texts, 8, False)
    none = [R.INT32_MIN, R.NO_SINK, R.NO_SINK]
    for type_ in TYPES:
        al = M.gotoh(type_, -5, -3)
        g, _ = _plan(al, 24, *_max_lens(pats, texts))
        assert 37 % (4 * (64 // g)) != 0
        sc, sk, _ = _compare(engine, al, mat, pats, texts, P, T)
        got = [[int(sc[k]), int(sk[k, 0]), int(sk[k, 1])] for k in range(37)]
        assert got[5] == none and got[36] == none
        if type_ == "local":
            assert got[0] == none and got[35] == none
        else:
            assert got[0][1:] == [9, 0]
            assert got[0][0] == (0 if type_ == "semi" else -5 - 3 * 8)


def test_refusals_and_null_outputs(engine):
    al = M.gotoh("local", -5, -3)
    mat = M.random_table(24, 0xF2)
    pats, texts = _random_batch(24, (1, 9, 20), 0xF3, text_lens=(8, 33))
    P, T = G.PackedSet.pack(pats, 8, False), G.PackedSet.pack(texts, 8, False)
    sc, sk = engine.nv_matrix_score_host(al, mat, P, T)
    only_sc, none_sk = engine.nv_matrix_score_host(al, mat, P, T, sinks=False)
    none_sc, only_sk = engine.nv_matrix_score_host(al, mat, P, T, scores=False)
    assert none_sk is None and none_sc is None
    assert np.array_equal(only_sc, sc) and np.array_equal(only_sk, sk)
    with pytest.raises(RuntimeError, match=r"\(-1\).*null argument"):
        engine.nv_matrix_score_host(al, mat, P, T, scores=False, sinks=False)
    for aligner in (G.NV_SW, G.NV_ED):
        with pytest.raises(RuntimeError, match=r"\(-5\)"):           # GASALX_EUNSUPPORTED
            engine.nv_matrix_score_host(G.NvAligner(aligner, G.NV_LOCAL, 1, -1, -5, -3, -1, -1), mat, P, T)
    for n in (1, 33):
        with pytest.raises(RuntimeError, match=r"\(-1\).*2\.\.32"):  # GASALX_EINVAL
            engine.nv_matrix_score_host(al, G.NvMatrix(np.zeros((n, n), np.int8)), P, T)
    # match / mismatch are not read, by the kernel or by the range check (the largest |entry| stands
    # in their place there); the gap scores are
    other = G.NvAligner(G.NV_GOTOH, G.NV_LOCAL, 1 << 27, -(1 << 27), -5, -3)
    assert np.array_equal(engine.nv_matrix_score_host(other, mat, P, T)[0], sc)
    with pytest.raises(RuntimeError, match=r"\(-2\).*exact range"):   # GASALX_ERANGE
        engine.nv_matrix_score_host(G.NvAligner(G.NV_GOTOH, G.NV_LOCAL, 0, 0, -(1 << 27), -3), mat, P, T)


def test_device_entry_on_its_own_stream(engine):
    import torch
    al = M.gotoh("local", -5, -3)
    mat = M.random_table(24, 0xF4)
    pats, texts = _random_batch(24, (1, 9, 20, 130), 0xF5, text_lens=(8, 33, 200))
    P, T = G.PackedSet.pack(pats, 8, False), G.PackedSet.pack(texts, 8, False)
    n = P.n
    rs, rk, _ = M.batch(al, mat, 24, pats, texts)
    dev = torch.device("cuda", 0)
    u = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    keep = [u(P.words), u(P.offsets), u(T.words), u(T.offsets)]
    mk = lambda S, w, off: {"words": w.data_ptr(), "offsets": off.data_ptr(), "length": 0, "bits": S.bits,
                            "big_endian": S.big_endian}
    pat, txt = mk(P, keep[0], keep[1]), mk(T, keep[2], keep[3])
    stream = torch.cuda.Stream()
    for bounds in ((0, 0), _max_lens(pats, texts)):            # lengths read back, and given
        dsc = torch.full((n,), -77, dtype=torch.int32, device=dev)
        dsk = torch.full((2 * n,), -77, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        table = G.NvMatrix(mat.scores.copy())
        engine.nv_matrix_score_device_ptrs(al, table, n, pat, txt, dsc.data_ptr(), dsk.data_ptr(), *bounds,
                                           stream=stream.cuda_stream)
        table.scores[:] = 0                                    # read during the call: the caller's again on return
        stream.synchronize()
        assert np.array_equal(dsc.cpu().numpy(), rs)
        assert np.array_equal(dsk.cpu().numpy().view(np.uint32).reshape(n, 2), rk)
    # sinks only: the scores array stays untouched
    dsc = torch.full((n,), -77, dtype=torch.int32, device=dev)
    dsk = torch.full((2 * n,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    engine.nv_matrix_score_device_ptrs(al, mat, n, pat, txt, 0, dsk.data_ptr(), *_max_lens(pats, texts),
                                       stream=stream.cuda_stream)
    stream.synchronize()
    assert (dsc.cpu().numpy() == -77).all()
    assert np.array_equal(dsk.cpu().numpy().view(np.uint32).reshape(n, 2), rk)

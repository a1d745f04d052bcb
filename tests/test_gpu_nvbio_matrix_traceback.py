"""GPU parity of the matrix-scored Gotoh traceback (gasalx_nv_matrix_traceback_*, nvmatrix_trace.hpp)
through the C ABI: score, source, sink, n_ops and every push bit for bit against
tests/nvbio_matrix_traceback_model.py (pinned to the C oracle, to hand-worked cells and by replay in
test_nvbio_matrix_traceback_model.py).  Pattern lengths sit at the edges of the stripes of 8 pattern
columns, batches at the edges of the 256-thread blocks."""
import ctypes

import numpy as np
import pytest

import gasal_ffi as G
import nvbio_matrix_model as M
import nvbio_matrix_traceback_model as T
import nvbio_sink_model as R

pytestmark = pytest.mark.gpu

TYPES = list(T.TYPES)
BUDGET = "GASALX_NV_TB_BUDGET"


def _pack(pats, texts, pb=8, pbig=False, tb=8, tbig=False):
    return G.PackedSet.pack(pats, pb, pbig), G.PackedSet.pack(texts, tb, tbig)


def _compare(engine, family, packing=(8, False, 8, False), what=""):
    al, mat, n, pats, texts = family
    P, Tx = _pack(pats, texts, *packing)
    got = engine.nv_matrix_traceback_host(al, mat, P, Tx)
    want = T.batch(al, mat, n, pats, texts)
    T.same(got, want, what)
    return got, want


# ---- stripe and block edges ----
@pytest.mark.parametrize("type_", TYPES)
def test_stripe_and_block_edges(engine, type_):
    fam = T.family_edges(type_)
    pats, texts = fam[3], fam[4]
    assert sorted({len(p) for p in pats}) == [1, 7, 8, 9, 16, 17, 63, 64, 65]
    assert sorted({len(t) for t in texts}) == [1, 8, 9, 33, 120]
    assert len(pats) == 45 and not np.array_equal(fam[1].scores, fam[1].scores.T) and fam[2] == 24
    _compare(engine, fam, what=f"edges {type_}")


@pytest.mark.parametrize("type_", TYPES)
def test_full_and_part_filled_block(engine, type_):
    # 300 pairs: one full block of 256 threads and one of 44; the tie family (at least half of the pairs
    # walk through a tied cell: test_nvbio_matrix_traceback_model.py::test_tie_family_ties)
    fam = T.family_block(type_)
    assert len(fam[3]) == 300
    _, want = _compare(engine, fam, what=f"block {type_}")
    assert T.tie_share(want["ties"]) >= 0.5


# ---- against the existing kernel ----
@pytest.mark.parametrize("type_", TYPES)
def test_simple_table_is_the_existing_traceback(engine, type_):
    ref_al = R.aligner("gotoh", type_)
    al, mat = M.gotoh(type_, ref_al.gap_open, ref_al.gap_ext), M.simple_table(4, ref_al.match, ref_al.mismatch)
    for kind, kw in (("edge", {}), ("shared", {"n_text": T.SIMPLE_SHARED_TEXT})):
        pats, texts, P, Tx = R.packed(kind, T.SIMPLE_LENS, T.SIMPLE_SEED, **kw)
        assert P.bits == 4 and P.big_endian and Tx.bits == 2 and (Tx.offsets is None) == (kind == "shared")
        got = engine.nv_matrix_traceback_host(al, mat, P, Tx)
        T.same(got, engine.nv_traceback_host(ref_al, P, Tx), f"{kind} {type_}: the existing kernel")
        T.same(got, T.batch(al, mat, 4, pats, texts), f"{kind} {type_}: the model")


# ---- packings ----
@pytest.mark.parametrize("case", list(T.PACKINGS))
@pytest.mark.parametrize("type_", TYPES)
def test_packings(engine, type_, case):
    n, pb, pbig, tb, tbig = T.PACKINGS[case]
    fam = T.family_packing(type_, case)
    assert fam[2] == n and not np.array_equal(fam[1].scores, fam[1].scores.T)
    _compare(engine, fam, (pb, pbig, tb, tbig), f"{case} {type_}")


# ---- pads ----
def test_all_positive_table(engine):
    # entries 1..9: every step along a diagonal gains, so a pad column of the last stripe (symbol 0, a real
    # symbol) holds more than any real cell of its row; none may become a sink or be walked
    fam = T.family_positive("local")
    al, mat, n, pats, texts = fam
    assert mat.scores.min() >= 1 and len(pats) == 45
    assert all(len(p) % 8 != 0 for p in pats) and len({len(p) % 8 for p in pats}) == 7
    assert len({len(p) for p in pats[:45]}) > 8                 # mixed lengths in one wave
    got, _ = _compare(engine, fam, what="positive local")
    for k in range(len(pats)):
        assert 1 <= got["sink"][k][0] <= len(texts[k]) and 1 <= got["sink"][k][1] <= len(pats[k])
        assert got["source"][k][0] < got["sink"][k][0] and got["source"][k][1] < got["sink"][k][1]
        assert T.replay(al, mat, n, pats[k], texts[k], T.one(got, k)) == got["score"][k]
    for type_ in ("global", "semi"):
        fam = T.family_positive(type_)
        assert len(fam[3]) == 16
        got, _ = _compare(engine, fam, what=f"positive {type_}")
        for k in range(16):
            assert T.replay(fam[0], fam[1], fam[2], fam[3][k], fam[4][k], T.one(got, k)) == got["score"][k]


# ---- clamp ----
@pytest.mark.parametrize("type_", TYPES)
def test_clamp(engine, type_):
    fam = T.family_clamp(type_)
    al, mat, n, pats, texts = fam
    assert n == 20 and max(int(p.max()) for p in pats) > 200 and max(int(t.max()) for t in texts) > 200
    got, _ = _compare(engine, fam, what=f"clamp {type_}")
    cp, ct = [np.minimum(p, 19) for p in pats], [np.minimum(t, 19) for t in texts]
    T.same(got, engine.nv_matrix_traceback_host(al, mat, *_pack(cp, ct)), "pre-clamped strings")


# ---- degenerate pairs ----
def test_degenerate_pairs(engine):
    rng = np.random.default_rng(0xF0)
    mat = M.random_table(24, 0xF1)
    pats = [rng.integers(0, 24, int(m)).astype(np.uint32) for m in rng.integers(1, 40, 37)]
    texts = [rng.integers(0, 24, int(k)).astype(np.uint32) for k in rng.integers(1, 90, 37)]
    empty = np.zeros(0, np.uint32)
    pats[0] = empty
    texts[5] = empty
    pats[36] = empty; texts[36] = empty
    for type_ in TYPES:
        got, _ = _compare(engine, (M.gotoh(type_, -5, -3), mat, 24, pats, texts), what=f"degenerate {type_}")
        for k in (0, 5, 36):                                     # gasalx_nv_traceback_*'s sentinels
            assert got["score"][k] == T.INT32_MIN and len(got["ops"][k]) == 0
            assert (got["source"][k] == T.NO_CELL).all() and (got["sink"][k] == T.NO_CELL).all()
        assert (got["score"][[1, 2, 3, 4]] != T.INT32_MIN).all()


# ---- chunks ----
@pytest.mark.parametrize("type_", TYPES)
def test_chunks(engine, monkeypatch, type_):
    al, mat, n, pats, texts = T.family_chunks(type_)
    assert len(pats) == 61
    lp, lt = [len(p) for p in pats], [len(t) for t in texts]
    assert int(np.argmax(lp)) >= 56 and int(np.argmax(lt)) >= 56      # the maxima lie in the last chunk of 7
    P, Tx = _pack(pats, texts)
    per = G.nv_traceback_workspace(max(lp), max(lt), 1)
    monkeypatch.setenv(BUDGET, str(7 * per))
    chunked = engine.nv_matrix_traceback_host(al, mat, P, Tx)
    monkeypatch.delenv(BUDGET)
    T.same(chunked, engine.nv_matrix_traceback_host(al, mat, P, Tx), f"chunks of 7 against one chunk, {type_}")
    T.same(chunked, T.batch(al, mat, n, pats, texts), f"chunks of 7, {type_}")


# ---- score agreement ----
@pytest.mark.parametrize("type_", TYPES)
def test_score_is_the_matrix_scorers(engine, type_):
    # the sinks are not compared: the traceback reports in pattern-stripe order, the scorer in text-stripe
    # order, so they may pick different cells among ties
    for fam in (T.family_edges(type_), T.family_packing(type_, "n32_8bit")):
        al, mat, n, pats, texts = fam
        P, Tx = _pack(pats, texts)
        sc, _ = engine.nv_matrix_score_host(al, mat, P, Tx, sinks=False)
        assert np.array_equal(engine.nv_matrix_traceback_host(al, mat, P, Tx)["score"], sc)


# ---- the device entry point ----
GUARD = 64
FILL32, FILL8 = 0x5A5A5A5A, 0xA5


def test_device_entry_on_the_callers_stream(engine):
    import torch
    al, mat, n_sym, pats, texts = T.family_device("local")
    P, Tx = _pack(pats, texts)
    n = P.n
    want = T.batch(al, mat, n_sym, pats, texts)
    max_p, max_t = max(len(p) for p in pats), max(len(t) for t in texts)
    stride = max_p + max_t                                          # its minimum
    dev = torch.device("cuda", 0)
    u = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
    keep = [u(P.words), u(P.offsets), u(Tx.words), u(Tx.offsets)]
    mk = lambda S, w, off: {"words": w.data_ptr(), "offsets": off.data_ptr(), "length": 0, "bits": S.bits,
                            "big_endian": S.big_endian}
    pat, txt = mk(P, keep[0], keep[1]), mk(Tx, keep[2], keep[3])
    stream = torch.cuda.Stream()
    sizes = {"score": n, "source": 2 * n, "sink": 2 * n, "ops": n * stride, "n_ops": n}
    for bounds in ((0, 0), (max_p, max_t)):                          # lengths read back, and exact
        outs = {k: (torch.full((sz + 2 * GUARD,), FILL8, dtype=torch.uint8, device=dev) if k == "ops"
                    else torch.full((sz + 2 * GUARD,), FILL32, dtype=torch.int32, device=dev)) for k, sz in sizes.items()}
        ptrs = {k: v.data_ptr() + GUARD * v.element_size() for k, v in outs.items()}
        torch.cuda.synchronize()
        table = G.NvMatrix(mat.scores.copy())
        engine.nv_matrix_traceback_device_ptrs(al, table, n, pat, txt, ptrs, stride, *bounds, stream=stream.cuda_stream)
        table.scores[:] = 0                                         # read during the call: the caller's again on return
        stream.synchronize()
        host = {k: v.cpu().numpy() for k, v in outs.items()}
        for k, a in host.items():
            fill = FILL8 if k == "ops" else FILL32
            assert (a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all(), f"{k}: a guard element was written"
        body = {k: a[GUARD:-GUARD] for k, a in host.items()}
        nops = body["n_ops"].view(np.uint32)
        got = dict(score=body["score"], source=body["source"].view(np.uint32).reshape(n, 2),
                   sink=body["sink"].view(np.uint32).reshape(n, 2),
                   ops=[body["ops"][k * stride:k * stride + int(nops[k])] for k in range(n)])
        T.same(got, want, f"device entry, bounds {bounds}")


# ---- refusals ----
def test_refusals(engine):
    al = M.gotoh("local", -5, -3)
    mat = M.random_table(24, 0xF2)
    pats, texts = T.random_pairs(24, (1, 9, 20), (8, 33), 0xF3)
    P, Tx = _pack(pats, texts)
    want = T.batch(al, mat, 24, pats, texts)
    T.same(engine.nv_matrix_traceback_host(al, mat, P, Tx), want, "as it stands")
    for aligner in (G.NV_SW, G.NV_ED):
        with pytest.raises(RuntimeError, match=r"\(-5\).*only the Gotoh aligner takes a substitution matrix"):
            engine.nv_matrix_traceback_host(G.NvAligner(aligner, G.NV_LOCAL, 1, -1, -5, -3, -1, -1), mat, P, Tx)
    for n in (1, 33):
        with pytest.raises(RuntimeError, match=r"\(-1\).*matrix size must be 2\.\.32"):
            engine.nv_matrix_traceback_host(al, G.NvMatrix(np.zeros((n, n), np.int8)), P, Tx)
    with pytest.raises(RuntimeError, match=r"\(-1\).*ops_stride < max pattern \+ max text length"):
        engine.nv_matrix_traceback_host(al, mat, P, Tx, ops_stride=20 + 33 - 1)
    # a table entry of 127: (max_p + max_t + 2) * 127 > 32767 from 257 symbols on (259 * 127 = 32893)
    big = G.NvMatrix(mat.scores.copy())
    big.scores[3, 5] = 127
    long_p = [np.zeros(100, np.uint32)]
    with pytest.raises(RuntimeError, match=r"\(-2\).*int16 columns"):
        engine.nv_matrix_traceback_host(al, big, *_pack(long_p, [np.zeros(157, np.uint32)]))
    engine.nv_matrix_traceback_host(al, big, *_pack(long_p, [np.zeros(156, np.uint32)]))     # 258 * 127 = 32766: inside
    # match / mismatch are never read, by the kernel or by the range rule
    other = G.NvAligner(G.NV_GOTOH, G.NV_LOCAL, 1 << 20, -(1 << 20), -5, -3)
    T.same(engine.nv_matrix_traceback_host(other, mat, P, Tx), want, "match / mismatch ignored")
    # a bit width of 16, a NULL output and a NULL table, through the C ABI itself
    lib = G.lib()
    ca, cm = al.cstruct(), mat.cstruct()
    n = P.n
    stride = 53
    sc, src, snk = np.zeros(n, np.int32), np.zeros(2 * n, np.uint32), np.zeros(2 * n, np.uint32)
    ops, nops = np.zeros(n * stride, np.uint8), np.zeros(n, np.uint32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(cp, ct, cmat=cm, scores=ptr(sc)):
        return lib.gasalx_nv_matrix_traceback_host(engine._h, ctypes.byref(ca), ctypes.byref(cmat), ctypes.c_uint32(n),
                                                   ctypes.byref(cp), ctypes.c_uint64(len(P.words)), ctypes.byref(ct),
                                                   ctypes.c_uint64(len(Tx.words)), scores, ptr(src), ptr(snk), ptr(ops),
                                                   ctypes.c_uint32(stride), ptr(nops))

    err = lambda: lib.gasalx_last_error().decode()
    assert call(P.cstruct(), Tx.cstruct()) == 0
    wide = P.cstruct()
    wide.bits = 16
    assert call(wide, Tx.cstruct()) == -1 and "symbol bits must be 2, 4 or 8" in err()
    assert call(P.cstruct(), Tx.cstruct(), scores=None) == -1 and "null argument" in err()
    assert call(P.cstruct(), Tx.cstruct(), cmat=G.CNvMatrix(None, 24)) == -1 and "null argument" in err()

"""gasalx_semi_cigar_* on the GPU against tests/semi_cigar_model.py, bit for bit: score, ends, starts,
op counts and CIGAR bytes, over both kernel families (the packed WF16_SEMI_TB flags kernel and the
int32 kernel), every shape edge, the length-sorted launch, ops, packed input, the device form and
the argument checks.  tests/test_semi_cigar_model.py ties the model to independent.semi on the
same batches."""
import os

import numpy as np
import pytest
import torch

import gasal_ffi as G
import independent as I
import semi_cigar_model as M

pytestmark = pytest.mark.gpu

FIELDS = ("score", "q_end", "t_end", "q_start", "t_start", "n_ops")


def gbatch(b):
    return G.Batch(*(np.ascontiguousarray(a) for a in (b.q_data, b.q_offsets, b.q_lens, b.t_data, b.t_offsets, b.t_lens)))


def params(sc=M.DEFAULT, **kw):
    return G.make_params(algo=G.SEMI_GLOBAL, head=G.TARGET, tail=G.TARGET, match=sc["a"], mismatch=sc["b"],
                         gap_open=sc["o"], gap_extend=sc["e"], **kw)


def same(g, m, b, what, cigar=True):
    for f in FIELDS:
        bad = np.flatnonzero(np.asarray(g[f]).astype(np.int64) != np.asarray(m[f]).astype(np.int64))
        assert bad.size == 0, (what, f, bad[:5], np.asarray(g[f])[bad[:5]], np.asarray(m[f])[bad[:5]])
    if cigar:
        # a CIGAR longer than its slot runs into the next pair's (as the GLOBAL walk's does): which of the
        # two walks writes such a byte last is not defined, so bytes that two pairs' ops cover are left out
        cover = np.zeros(b.q_bytes + 1, np.int64)
        lo = b.q_offsets.astype(np.int64)
        hi = np.minimum(lo + np.asarray(m["n_ops"]).astype(np.int64), b.q_bytes)
        np.add.at(cover, lo, 1)
        np.add.at(cover, hi, -1)
        own = np.cumsum(cover)[:b.q_bytes] <= 1
        diff = np.flatnonzero((g["cigar"] != m["cigar"]) & own)
        assert diff.size == 0, (what, "cigar bytes", diff[:5])


def run_named(engine, name, what, plan=None, **kw):
    b, m = M.reference(name)
    sc = M.named_batches()[name][1]
    p = params(sc, **kw)
    if plan:
        got = G.describe_semi_cigar_plan(p, int(b.q_lens.max()), int(b.t_lens.max()))
        assert got.startswith(plan), (what, got)
    g = engine.semi_cigar_host(gbatch(b), p)
    same(g, m, b, what)
    return engine.packed_pairs()


SHAPES = [(ql, tl) for ql in M.SHAPE_QL for tl in sorted(set(M.shape_tl(ql)))]


@pytest.mark.parametrize("ql,tl", SHAPES)
def test_shape_edges_packed(engine, ql, tl):
    handled, total = run_named(engine, f"shape_{ql}x{tl}", "packed", plan="wavefront16_semi_tb_G")
    assert handled == total == 300


@pytest.mark.parametrize("name,n", [("single", 1), ("seventeen", 17)])
def test_small_batches(engine, name, n):
    handled, total = run_named(engine, name, name, plan="wavefront16_semi_tb_G8R20")
    assert handled == total == n


@pytest.mark.parametrize("name", ["related", "unrelated", "overhang", "repeats"])
def test_content(engine, name):
    handled, total = run_named(engine, name, name, plan="wavefront16_semi_tb_G")
    assert handled == total


@pytest.mark.parametrize("ql,tl", SHAPES)
def test_shape_edges_int32_family(engine, monkeypatch, ql, tl):
    monkeypatch.setenv("GASALX_PACKED16", "0")
    handled, total = run_named(engine, f"shape_{ql}x{tl}", "PACKED16=0", plan="wavefront_semi_tb_G")
    assert (handled, total) == (0, 0)          # no packed flags launch (the score launch is int32 too)


@pytest.mark.parametrize("ql,tl", [(ql, tl) for ql in M.M200_QL for tl in sorted(set(M.shape_tl(ql)))])
def test_scores_outside_the_packed_window(engine, ql, tl):
    # match 200, mismatch 56: the packed kernel's table bytes refuse them at any length; the int16 range the
    # semi-global kernels keep admits these scores for the short shapes only, the others are refused with a text
    run_named(engine, f"m200_{ql}x{tl}", "match 200", plan="wavefront_semi_tb_G")


def test_scores_outside_the_int16_range_are_refused(engine):
    b, _ = M.reference("shape_150x150")
    with pytest.raises(RuntimeError, match=r"\(-2\): semi_cigar: lengths x scores leave the int16 range"):
        engine.semi_cigar_host(gbatch(b), params(M.MATCH200))


def test_n_targets_decline_blocks_inside_a_packed_launch(engine):
    handled, total = run_named(engine, "n_targets", "N targets", plan="wavefront16_semi_tb_G8R20")
    assert total == 300 and 0 < handled < total
    # with N_PENALTY the packed kernel scores N itself
    b, _ = M.reference("n_targets")
    m = M.semi_cigar(b, npen=2, **M.DEFAULT)
    g = engine.semi_cigar_host(gbatch(b), params(n_penalty=2))
    same(g, m, b, "N_PENALTY")
    assert engine.packed_pairs() == (300, 300)


@pytest.mark.parametrize("gmin", [8, 16, 32, 64])
def test_gmin(engine, monkeypatch, gmin):
    monkeypatch.setenv("GASALX_GMIN", str(gmin))
    want = {8: "G8R20", 16: "G16R16", 32: "G32R20", 64: "G64R20"}[gmin]
    handled, total = run_named(engine, "related", f"GMIN={gmin}", plan="wavefront16_semi_tb_" + want)
    assert handled == total


def _pack_codes(data):
    c = (np.asarray(data, np.uint8) & 15).reshape(-1, 8).astype(np.uint32)
    w = np.zeros(len(c), np.uint32)
    for k in range(8):
        w |= c[:, k] << np.uint32(28 - 4 * k)
    return w.view(np.uint8)


def test_ops_and_packed_input(engine):
    ob, m = M.reference("ops")
    b = M.ops_batch()
    qo, to = M.ops_codes(b.n)
    g = engine.semi_cigar_host(gbatch(b), params(), q_ops=qo, t_ops=to)
    same(g, m, b, "ops")
    qd = np.concatenate([_pack_codes(b.q_data), np.zeros(b.q_bytes // 2, np.uint8)])
    td = np.concatenate([_pack_codes(b.t_data), np.zeros(b.t_bytes // 2, np.uint8)])
    pb = G.Batch(qd, b.q_offsets, b.q_lens, td, b.t_offsets, b.t_lens)
    g = engine.semi_cigar_host(pb, params(is_packed=1), q_ops=qo, t_ops=to)
    same(g, m, b, "is_packed ops")
    g = engine.semi_cigar_host(pb, params(is_packed=1))
    same(g, M.semi_cigar(b), b, "is_packed")


def test_length_sorted(engine):
    handled, total = run_named(engine, "sorted", "sorted", plan="wavefront16_semi_tb_G8R20")
    assert handled == total == 4200


def _dev(b, n_extra=0):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = dict(q_batch=t(b.q_data), q_offsets=t(b.q_offsets.view(np.int32)), q_lens=t(b.q_lens.view(np.int32)),
             t_batch=t(b.t_data), t_offsets=t(b.t_offsets.view(np.int32)), t_lens=t(b.t_lens.view(np.int32)))
    o = dict(aln_score=torch.full((b.n,), -7, dtype=torch.int32, device="cuda"),
             q_end=torch.full((b.n,), -7, dtype=torch.int32, device="cuda"),
             t_end=torch.full((b.n,), -7, dtype=torch.int32, device="cuda"),
             q_start=torch.full((b.n,), -7, dtype=torch.int32, device="cuda"),
             t_start=torch.full((b.n,), -7, dtype=torch.int32, device="cuda"),
             cigar=torch.zeros(b.q_bytes + n_extra, dtype=torch.uint8, device="cuda"),
             n_cigar_ops=torch.zeros(b.n, dtype=torch.int32, device="cuda"))
    return d, o


def _dev_result(o, b):
    torch.cuda.synchronize()
    return {"score": o["aln_score"].cpu().numpy(), "q_end": o["q_end"].cpu().numpy(), "t_end": o["t_end"].cpu().numpy(),
            "q_start": o["q_start"].cpu().numpy(), "t_start": o["t_start"].cpu().numpy(),
            "n_ops": o["n_cigar_ops"].cpu().numpy(), "cigar": o["cigar"].cpu().numpy()[:b.q_bytes]}


def test_device_form(engine):
    b, m = M.reference("related")
    st = torch.cuda.Stream()
    for mq, mt in ((150, 182), (0, 0)):
        d, o = _dev(b)
        torch.cuda.synchronize()
        ptrs = {k: v.data_ptr() for k, v in {**d, **o}.items()}
        engine.semi_cigar_device_ptrs(params(), ptrs, b.q_bytes, b.t_bytes, b.n, mq, mt, stream=st.cuda_stream)
        st.synchronize()
        same(_dev_result(o, b), m, b, f"device form, max lens {mq} x {mt}")
    # two calls back to back on one engine, the second larger: the workspace grows between them
    small, big = M.reference("seventeen"), M.reference("sorted")
    outs = []
    for bb, _ in (small, big):
        d, o = _dev(bb)
        torch.cuda.synchronize()
        ptrs = {k: v.data_ptr() for k, v in {**d, **o}.items()}
        engine.semi_cigar_device_ptrs(params(), ptrs, bb.q_bytes, bb.t_bytes, bb.n, int(bb.q_lens.max()),
                                      int(bb.t_lens.max()), stream=st.cuda_stream)
        outs.append((d, o))
    st.synchronize()
    same(_dev_result(outs[0][1], small[0]), small[1], small[0], "back to back, first")
    same(_dev_result(outs[1][1], big[0]), big[1], big[0], "back to back, second")


def test_cigar_capacity(engine):
    # about 2 * ql op bytes per pair in slots of pad8(ql): as in the GLOBAL walk, a longer CIGAR runs into
    # the next pair's slot, the counts report every op, and nothing is written past the buffer
    b, m = M.reference("overflow")
    assert (m["n_ops"] > (b.q_lens + 7) // 8 * 8).sum() > 20
    d, o = _dev(b, n_extra=256)
    o["cigar"][b.q_bytes:] = 0xA5
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in {**d, **o}.items()}
    engine.semi_cigar_device_ptrs(params(M.OVERFLOW), ptrs, b.q_bytes, b.t_bytes, b.n, 16, 32)
    torch.cuda.synchronize()
    g = _dev_result(o, b)
    same(g, m, b, "overflow", cigar=False)
    assert bool((o["cigar"][b.q_bytes:] == 0xA5).all()), "bytes past the CIGAR buffer were written"
    # pair 0's own slot holds the head of its ops (no earlier pair runs into it)
    slot = (int(b.q_lens[0]) + 7) // 8 * 8
    assert bytes(g["cigar"][:slot]) == m["ops"][0][:slot]
    # the last pair's ops stop at the end of the buffer
    off = int(b.q_offsets[-1])
    assert bytes(g["cigar"][off:]) == m["ops"][-1][:b.q_bytes - off]


def _raises(fn, code, text):
    with pytest.raises(RuntimeError) as ex:
        fn()
    assert f"({code}): {text}" in str(ex.value), str(ex.value)


def test_argument_checks_in_order(engine):
    b, _ = M.reference("seventeen")
    gb = gbatch(b)
    lib = G.lib()
    import ctypes

    def call(p, cr_kw=None, cigar=None):
        n = gb.n
        out = {k: np.full(n, 77, np.int32) for k in ("s", "qe", "te", "qs", "ts", "s2", "qe2", "te2")}
        cg = np.full(gb.q_bytes, 0x5A, np.uint8) if cigar is None else cigar
        nops = np.full(n, 77, np.uint32)
        use = dict(s=True, cigar=True, nops=True, s2=False)
        use.update(cr_kw or {})
        cb = G.CBatch(G._p(gb.q_data), G._p(gb.q_offsets), G._p(gb.q_lens), G._p(gb.t_data), G._p(gb.t_offsets),
                      G._p(gb.t_lens), gb.q_bytes, gb.t_bytes, n, None, None, None, 0, 0)
        cr = G.CResults(G._p(out["s"]) if use["s"] else None, G._p(out["qe"]), G._p(out["te"]), G._p(out["qs"]),
                        G._p(out["ts"]), G._p(out["s2"]) if use["s2"] else None, None, None,
                        G._p(cg) if use["cigar"] else None, G._p(nops) if use["nops"] else None)
        rc = lib.gasalx_semi_cigar_host(engine._h, ctypes.byref(p), ctypes.byref(cb), ctypes.byref(cr))
        untouched = all((v == 77).all() for v in out.values()) and (nops == 77).all() and \
            (cigar is not None or (cg == 0x5A).all())
        return rc, lib.gasalx_last_error().decode(), untouched

    names = {G.NONE: "NONE", G.QUERY: "QUERY", G.TARGET: "TARGET", G.BOTH: "BOTH"}
    for head in names:
        for tail in names:
            if (head, tail) == (G.TARGET, G.TARGET):
                continue
            rc, msg, untouched = call(G.make_params(algo=G.SEMI_GLOBAL, head=head, tail=tail))
            assert rc == -5 and msg == (f"semi_cigar: HEAD={names[head]} TAIL={names[tail]} is not supported "
                                        "(HEAD=TARGET TAIL=TARGET only)"), (head, tail, rc, msg)
            assert untouched, (head, tail)
    # the order: algo, second_best, head / tail, required outputs, second-best outputs, the overlay
    rc, msg, _ = call(G.make_params(algo=G.LOCAL, second_best=1, head=G.NONE))
    assert (rc, msg) == (-1, "semi_cigar: algo must be SEMI_GLOBAL")
    rc, msg, _ = call(G.make_params(algo=G.SEMI_GLOBAL, second_best=1, head=G.NONE))
    assert (rc, msg) == (-5, "semi_cigar: second_best is not supported")
    rc, msg, _ = call(G.make_params(algo=G.SEMI_GLOBAL, head=G.NONE), dict(s=False))
    assert rc == -5 and msg.startswith("semi_cigar: HEAD=NONE TAIL=TARGET")
    for miss in ("s", "cigar", "nops"):
        rc, msg, untouched = call(params(), {miss: False, "s2": True})
        assert (rc, msg) == (-1, "semi_cigar: aln_score, cigar and n_cigar_ops outputs are required") and untouched
    rc, msg, untouched = call(params(), dict(s2=True), cigar=gb.q_data)
    assert (rc, msg) == (-1, "semi_cigar: the second-best outputs must be NULL") and untouched
    keep = gb.q_data.copy()
    rc, msg, untouched = call(params(), cigar=gb.q_data)
    assert (rc, msg) == (-1, "semi_cigar: cigar overlaps q_batch (it must be a buffer of its own)")
    assert untouched and np.array_equal(keep, gb.q_data)
    # start_pos is ignored; lengths with no wavefront shape are refused with a text
    g = engine.semi_cigar_host(gb, params(start_pos=G.WITH_START))
    same(g, M.reference("seventeen")[1], b, "start_pos ignored")
    long_q = M.ModelBatch.from_pairs([b"A" * 1281], [b"A" * 100])
    _raises(lambda: engine.semi_cigar_host(gbatch(long_q), params()), -2,
            "semi_cigar: padded query of 1288 over the largest wavefront shape (1280 rows)")
    _raises(lambda: engine.semi_cigar_host(gb, params(dict(M.DEFAULT, e=-1))), -5,
            "semi_cigar: negative gap_open or gap_extend is not supported")


def test_align_host_semi_with_tb_still_mimics_the_reference(engine):
    # the reference-shaped call keeps the reference's behaviour: the "CIGAR" is the query batch and the
    # op counts are the query lengths (gasal_align.cu:280-283)
    b, m = M.reference("seventeen")
    gb = gbatch(b)
    g = engine.align_host(gb, G.make_params(algo=G.SEMI_GLOBAL, head=G.TARGET, tail=G.TARGET, start_pos=G.WITH_TB))
    assert np.array_equal(g["cigar"], gb.q_data)
    assert np.array_equal(g["n_ops"], gb.q_lens)
    for f in ("score", "q_end", "t_end"):
        assert np.array_equal(g[f], m[f]), f

"""gasalx_semi_cigar_head_* on the GPU against tests/semi_cigar_head_model.py, bit for bit, for each of the
four heads: score, ends, both starts, op counts and CIGAR bytes, over both kernel families (the packed
flags kernel and the int32 kernel), every shape edge, the length-sorted launch, ops, packed input, the
device form and the cigar capacity; HEAD = TARGET byte-equal to gasalx_semi_cigar_host.
tests/test_semi_cigar_head_model.py ties the model to independent.semi on the same batches."""
import json
import os

import numpy as np
import pytest
import torch

import gasal_ffi as G
import semi_cigar_head_model as H
import semi_cigar_model as M
from test_gpu_semi_cigar import _dev, _dev_result, _pack_codes, gbatch, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = pytest.mark.parametrize("head", H.HEADS, ids=[H.HEAD_NAME[h] for h in H.HEADS])
SUFFIX = {H.NONE: "_hn", H.QUERY: "_hq", H.TARGET: "_ht", H.BOTH: "_hb"}


def params(head, sc=M.DEFAULT, **kw):
    return G.make_params(algo=G.SEMI_GLOBAL, head=head, tail=G.TARGET, match=sc["a"], mismatch=sc["b"],
                         gap_open=sc["o"], gap_extend=sc["e"], **kw)


def run_named(engine, name, head, what, plan=None, **kw):
    b, m = H.reference(name, head)
    p = params(head, H.named_batches()[name][1], **kw)
    if plan:
        got = G.describe_semi_cigar_head_plan(p, int(b.q_lens.max()), int(b.t_lens.max()))
        assert got.startswith(plan) and got.endswith(SUFFIX[head]), (what, got)
    g = engine.semi_cigar_head_host(gbatch(b), p)
    same(g, m, b, (what, H.HEAD_NAME[head]))
    return engine.packed_pairs()


SHAPES = [(ql, tl) for ql in M.SHAPE_QL for tl in sorted(set(M.shape_tl(ql)))]


@HEADS
@pytest.mark.parametrize("ql,tl", SHAPES)
def test_shape_edges_packed(engine, ql, tl, head):
    handled, total = run_named(engine, f"shape_{ql}x{tl}", head, "packed", plan="wavefront16_semi_tb_G")
    assert handled == total == 300


@HEADS
@pytest.mark.parametrize("ql,tl", SHAPES)
def test_shape_edges_int32_family(engine, monkeypatch, ql, tl, head):
    monkeypatch.setenv("GASALX_PACKED16", "0")
    handled, total = run_named(engine, f"shape_{ql}x{tl}", head, "PACKED16=0", plan="wavefront_semi_tb_G")
    assert (handled, total) == (0, 0)


@HEADS
@pytest.mark.parametrize("name,n", [("single", 1), ("seventeen", 17)])
def test_small_batches(engine, name, n, head):
    handled, total = run_named(engine, name, head, name, plan="wavefront16_semi_tb_G8R20")
    assert handled == total == n


@HEADS
@pytest.mark.parametrize("name", ["related", "unrelated", "overhang", "repeats", "overhang_q"])
def test_content(engine, name, head):
    handled, total = run_named(engine, name, head, name, plan="wavefront16_semi_tb_G")
    assert handled == total


@HEADS
def test_n_targets_decline_blocks_inside_a_packed_launch(engine, head):
    handled, total = run_named(engine, "n_targets", head, "N targets", plan="wavefront16_semi_tb_G8R20")
    assert total == 300 and 0 < handled < total
    b = H.batch_of("n_targets")
    m = H.semi_cigar_head(b, head, npen=2, **M.DEFAULT)
    g = engine.semi_cigar_head_host(gbatch(b), params(head, n_penalty=2))
    same(g, m, b, "N_PENALTY")
    assert engine.packed_pairs() == (300, 300)


@HEADS
@pytest.mark.parametrize("ql,tl", [(ql, tl) for ql in M.M200_QL for tl in sorted(set(M.shape_tl(ql)))])
def test_scores_outside_the_packed_window(engine, ql, tl, head):
    run_named(engine, f"m200_{ql}x{tl}", head, "match 200", plan="wavefront_semi_tb_G")


@HEADS
def test_scores_outside_the_int16_range_are_refused(engine, head):
    b = H.batch_of("shape_150x150")
    with pytest.raises(RuntimeError, match=r"\(-2\): semi_cigar_head: lengths x scores leave the int16 range"):
        engine.semi_cigar_head_host(gbatch(b), params(head, M.MATCH200))


@HEADS
def test_length_sorted(engine, head):
    handled, total = run_named(engine, "sorted", head, "sorted", plan="wavefront16_semi_tb_G8R20")
    assert handled == total == 4200


@HEADS
def test_ops_and_packed_input(engine, head):
    _, m = H.reference("ops", head)
    b = M.ops_batch()
    qo, to = M.ops_codes(b.n)
    g = engine.semi_cigar_head_host(gbatch(b), params(head), q_ops=qo, t_ops=to)
    same(g, m, b, "ops")
    qd = np.concatenate([_pack_codes(b.q_data), np.zeros(b.q_bytes // 2, np.uint8)])
    td = np.concatenate([_pack_codes(b.t_data), np.zeros(b.t_bytes // 2, np.uint8)])
    pb = G.Batch(qd, b.q_offsets, b.q_lens, td, b.t_offsets, b.t_lens)
    g = engine.semi_cigar_head_host(pb, params(head, is_packed=1), q_ops=qo, t_ops=to)
    same(g, m, b, "is_packed ops")
    g = engine.semi_cigar_head_host(pb, params(head, is_packed=1))
    same(g, H.semi_cigar_head(b, head), b, "is_packed")


@HEADS
def test_device_form_leaves_bytes_past_the_ops(engine, head):
    # every pair's ops fit its own slot here, so each byte of the buffer is one pair's op or nobody's: the
    # device form writes the first and leaves the poison in the second
    name = "overhang_q" if head in (H.QUERY, H.BOTH) else "overhang"
    b, m = H.reference(name, head)
    slots = (b.q_lens.astype(np.int64) + 7) // 8 * 8
    assert (m["n_ops"] <= slots).all()
    want = np.full(b.q_bytes, 0xA5, np.uint8)
    for p in range(b.n):
        off = int(b.q_offsets[p])
        want[off:off + len(m["ops"][p])] = np.frombuffer(m["ops"][p], np.uint8)
    st = torch.cuda.Stream()
    for mq, mt in ((150, 182), (0, 0)):
        d, o = _dev(b)
        o["cigar"][:] = 0xA5
        torch.cuda.synchronize()
        ptrs = {k: v.data_ptr() for k, v in {**d, **o}.items()}
        engine.semi_cigar_head_device_ptrs(params(head), ptrs, b.q_bytes, b.t_bytes, b.n, mq, mt, stream=st.cuda_stream)
        st.synchronize()
        g = _dev_result(o, b)
        same(g, m, b, f"device form, max lens {mq} x {mt}", cigar=False)
        assert np.array_equal(g["cigar"], want), np.flatnonzero(g["cigar"] != want)[:5]


@HEADS
def test_cigar_capacity(engine, head):
    b, m = H.reference("overflow", head)
    assert (m["n_ops"] > (b.q_lens + 7) // 8 * 8).sum() > 20
    d, o = _dev(b, n_extra=256)
    o["cigar"][b.q_bytes:] = 0xA5
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in {**d, **o}.items()}
    engine.semi_cigar_head_device_ptrs(params(head, M.OVERFLOW), ptrs, b.q_bytes, b.t_bytes, b.n, 16, 32)
    torch.cuda.synchronize()
    g = _dev_result(o, b)
    same(g, m, b, "overflow", cigar=False)
    assert bool((o["cigar"][b.q_bytes:] == 0xA5).all()), "bytes past the CIGAR buffer were written"
    slot = (int(b.q_lens[0]) + 7) // 8 * 8
    assert bytes(g["cigar"][:slot]) == m["ops"][0][:slot]
    off = int(b.q_offsets[-1])
    assert bytes(g["cigar"][off:]) == m["ops"][-1][:b.q_bytes - off]


@pytest.mark.parametrize("name", ["related", "overhang", "n_targets", "sorted", "shape_9x41", "m200_8x40"])
def test_head_target_is_byte_equal_to_semi_cigar_host(engine, name):
    b = H.batch_of(name)
    sc = H.named_batches()[name][1]
    new = engine.semi_cigar_head_host(gbatch(b), params(H.TARGET, sc))
    old = engine.semi_cigar_host(gbatch(b), params(H.TARGET, sc))
    for f in ("score", "q_end", "t_end", "q_start", "t_start", "n_ops", "cigar"):
        assert np.array_equal(new[f], old[f]), (name, f)


@HEADS
def test_plan_names_against_the_golden_file(engine, monkeypatch, head):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "semi_cigar_head_plan_names.json")))["rows"]
    for env in ("default", "GASALX_PACKED16=0"):
        if env != "default":
            monkeypatch.setenv(*env.split("="))
        for ql in (8, 150, 152, 300):
            for tl in (ql, ql + 32):
                b = H.batch_of(f"shape_{ql}x{tl}")
                got = G.describe_semi_cigar_head_plan(params(head), int(b.q_lens.max()), int(b.t_lens.max()))
                assert got == gold[f"{env}|{SUFFIX[head][1:]}|1/4/6/1|{ql}x{tl}"], (env, ql, tl, got)
    # the call runs the family it names
    handled, total = run_named(engine, "shape_150x182", head, "PACKED16=0", plan="wavefront_semi_tb_G8R20")
    assert (handled, total) == (0, 0)


def test_required_outputs_and_refusals(engine):
    import ctypes
    b = H.batch_of("seventeen")
    gb = gbatch(b)
    lib = G.lib()
    n = gb.n
    out = {k: np.full(n, 77, np.int32) for k in ("s", "qe", "te", "qs", "ts")}
    cg = np.full(gb.q_bytes, 0x5A, np.uint8)
    nops = np.full(n, 77, np.uint32)
    cb = G.CBatch(G._p(gb.q_data), G._p(gb.q_offsets), G._p(gb.q_lens), G._p(gb.t_data), G._p(gb.t_offsets),
                  G._p(gb.t_lens), gb.q_bytes, gb.t_bytes, n, None, None, None, 0, 0)

    def call(p, **kw):
        use = dict(s=G._p(out["s"]), cigar=G._p(cg), nops=G._p(nops))
        use.update(kw)
        cr = G.CResults(use["s"], G._p(out["qe"]), G._p(out["te"]), G._p(out["qs"]), G._p(out["ts"]), None, None,
                        None, use["cigar"], use["nops"])
        rc = lib.gasalx_semi_cigar_head_host(engine._h, ctypes.byref(p), ctypes.byref(cb), ctypes.byref(cr))
        untouched = all((v == 77).all() for v in out.values()) and (nops == 77).all() and (cg == 0x5A).all()
        return rc, lib.gasalx_last_error().decode(), untouched

    for tail, tn in ((G.NONE, "NONE"), (G.QUERY, "QUERY"), (G.BOTH, "BOTH")):
        rc, msg, untouched = call(G.make_params(algo=G.SEMI_GLOBAL, head=G.QUERY, tail=tail))
        assert (rc, msg) == (-5, f"semi_cigar_head: HEAD=QUERY TAIL={tn} is not supported (TAIL=TARGET only)")
        assert untouched
    # the order: algo, second_best, tail, required outputs, the overlay
    rc, msg, _ = call(G.make_params(algo=G.LOCAL, second_best=1, tail=G.NONE))
    assert (rc, msg) == (-1, "semi_cigar_head: algo must be SEMI_GLOBAL")
    rc, msg, _ = call(G.make_params(algo=G.SEMI_GLOBAL, second_best=1, tail=G.NONE))
    assert (rc, msg) == (-5, "semi_cigar_head: second_best is not supported")
    for miss in ("s", "cigar", "nops"):
        rc, msg, untouched = call(params(H.NONE), **{miss: None})
        assert (rc, msg) == (-1, "semi_cigar_head: aln_score, cigar and n_cigar_ops outputs are required") and untouched
    rc, msg, untouched = call(params(H.BOTH), cigar=G._p(gb.q_data))
    assert (rc, msg) == (-1, "semi_cigar_head: cigar overlaps q_batch (it must be a buffer of its own)") and untouched
    rc, msg, _ = call(params(H.QUERY))
    assert rc == 0, msg
    m = H.reference("seventeen", H.QUERY)[1]
    assert np.array_equal(out["s"], m["score"]) and np.array_equal(out["qs"], m["q_start"])

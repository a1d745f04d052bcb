"""The plain LOCAL score kernel's prologue (wf16_body.inc, ALGO_ == WF_LOCAL): lengths and offsets
loaded for every lane of a clamped slot and selected afterwards, the query read as dwords from
the dword below the lane's first row, the target quads of a wave fetched up to six trips at a time.

SW local a1 b4 o6 e1, score / q_end / t_end bit-exact against the oracle.  The planner gives a
small batch more lanes per pair (make_plan: G64R3 below 4,096 pairs of 150 bp), so the small
tests force the flagship shape with GASALX_GMIN=8: wf16_kernel<0,8,19>, 64 pairs per block, R = 19
rows per lane, five query dwords and one more per pair, six fetch trips.  Batches of one block,
one block and a pair, and three blocks and a partial one; query lengths whose last dword is the
padded sequence's last or holds pad bytes, lanes starting at every byte offset of a dword
(19 lg & 3); short pairs beside long ones (the sorted order, A.perm) and equal lengths (the
caller's order); a declined block between two packed ones; device buffers of exactly the
batch's size; packed input, which keeps the byte loads.  The mixed launch (wf16_mix_kernel<0,8,19,
32,5>, both regions' prologues) runs at the smallest batch that has a second region.
"""
import numpy as np
import pytest

import gasal_ffi as G
import helpers
import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("score", "q_end", "t_end")
KW = dict(algo=G.LOCAL, match=1, mismatch=4, gap_open=6, gap_extend=1)
PPB = 64   # pairs per block at G8: 4 waves x 8 slots x 2 pairs


@pytest.fixture(scope="module", autouse=True)
def _build():
    O.build()


@pytest.fixture
def g8(monkeypatch):
    """The flagship shape whatever the batch size: with GASALX_GMIN set the planner's minimum G no
    longer depends on n, so describe_plan (which has no n) names the launch that runs."""
    monkeypatch.setenv("GASALX_GMIN", "8")


def related(rng, n, ql, tl):
    qs, ts = [], []
    for _ in range(n):
        q = helpers.random_seq(rng, ql)
        qs.append(q)
        ts.append((helpers.mutate(rng, q) + helpers.random_seq(rng, tl))[:tl])
    return qs, ts


def same(g, o, b, what=""):
    for f in FIELDS:
        bad = np.nonzero(g[f] != o[f])[0]
        assert bad.size == 0, (f"{what} {f}: {bad.size}/{b.n} differ; first #{bad[0]}: gpu={g[f][bad[0]]} "
                               f"oracle={o[f][bad[0]]} q={b.q_lens[bad[0]]} t={b.t_lens[bad[0]]}")


def device_align(engine, b, **kw):
    """One device-resident call over torch buffers of exactly the batch's bytes."""
    import torch
    dev = torch.device("cuda", 0)
    u = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else a).to(dev)
    d = {"q_batch": u(b.q_data), "t_batch": u(b.t_data), "q_offsets": u(b.q_offsets), "t_offsets": u(b.t_offsets),
         "q_lens": u(b.q_lens), "t_lens": u(b.t_lens)}
    assert d["q_batch"].numel() == b.q_bytes and d["t_batch"].numel() == b.t_bytes
    for f in ("aln_score", "q_end", "t_end"):
        d[f] = torch.full((b.n,), -7, dtype=torch.int32, device=dev)
    engine.align_device_ptrs(G.make_params(**dict(KW, **kw)), {k: v.data_ptr() for k, v in d.items()}, b.q_bytes,
                             b.t_bytes, b.n, int(b.q_lens.max()), int(b.t_lens.max()))
    torch.cuda.synchronize()
    return {"score": d["aln_score"].cpu().numpy(), "q_end": d["q_end"].cpu().numpy(),
            "t_end": d["t_end"].cpu().numpy()}


@pytest.mark.parametrize("n", [PPB, PPB + 1, 3 * PPB + 5])
def test_block_counts_and_partial_last_block(engine, g8, n):
    assert G.describe_plan(G.make_params(**KW), 150, 150) == "wavefront16_local_G8R19"
    qs, ts = related(np.random.default_rng(0x9E0 + n), n, 150, 150)
    b = G.Batch.from_pairs(qs, ts)
    o = O.align(b, O.make_params(**KW))
    engine.packed_pairs()                                    # forget earlier launches
    same(engine.align_host(b, G.make_params(**KW)), o, b, "host")
    handled, total = engine.packed_pairs()
    assert handled == total == n, (handled, total)
    same(device_align(engine, b), o, b, "exact-size device buffers")


@pytest.mark.parametrize("ql", [129, 133, 137, 141, 144, 145, 147, 149, 150, 151, 152])
def test_query_dwords_of_the_flagship_shape(engine, g8, ql):
    # G8R19: lane lg starts at row 19 lg, byte (19 lg) & 3 of its first dword (3, 2, 1, 0, 3, 2, 1
    # for lanes 1..7), and takes bytes from dwords k / 4 = 0..4 of its six.  Lane 7 (rows 133..151)
    # reads dwords 33..38 of the query while they lie inside its padded length: the guard cuts after
    # dword 33 (ql <= 136), 35 (<= 144) or 37 (<= 152, the padded sequence's last; none is read past
    # it).  The last pair's query ends the exactly sized device buffer.
    assert G.describe_plan(G.make_params(**KW), ql, 150) == "wavefront16_local_G8R19", ql
    qs, ts = related(np.random.default_rng(0x9E1 + ql), PPB + 6, ql, 150)
    b = G.Batch.from_pairs(qs, ts)
    o = O.align(b, O.make_params(**KW))
    same(engine.align_host(b, G.make_params(**KW)), o, b, "host")
    same(device_align(engine, b), o, b, "exact-size device buffers")


@pytest.mark.parametrize("ql,tl", [(1, 150), (7, 9), (19, 40), (20, 150), (58, 60), (77, 150), (96, 101), (128, 40)])
def test_query_dwords_of_the_shorter_g8_shapes(engine, g8, ql, tl):
    # R = 8, 12 and 16 (two to four query dwords and one more); short targets take fewer than six
    # fetch trips (40 bp: 2), long ones all of them
    assert G.describe_plan(G.make_params(**KW), ql, tl).startswith("wavefront16_local_G8R"), (ql, tl)
    qs, ts = related(np.random.default_rng(0x9E5 + 200 * ql + tl), PPB + 6, ql, tl)
    b = G.Batch.from_pairs(qs, ts)
    o = O.align(b, O.make_params(**KW))
    same(engine.align_host(b, G.make_params(**KW)), o, b, "host")
    same(device_align(engine, b), o, b, "exact-size device buffers")


def test_small_batch_shape_without_forcing(engine):
    # what the planner itself gives 70 pairs: more lanes per pair (G64R3 at 150 bp), one query dword
    # and one more, two fetch trips
    qs, ts = related(np.random.default_rng(0x9E6), 70, 150, 150)
    b = G.Batch.from_pairs(qs, ts)
    o = O.align(b, O.make_params(**KW))
    same(engine.align_host(b, G.make_params(**KW)), o, b, "host")
    same(device_align(engine, b), o, b, "exact-size device buffers")


def test_long_and_short_blocks_sorted_and_in_order(engine, g8):
    # blocks of 150 x 150, 24 x 40, 150 x 152 and 8 x 8 pairs, a full one on either side: uneven
    # lengths run sorted by target length (A.perm), and each kind alone runs in the caller's order
    rng = np.random.default_rng(0x9E2)
    qs, ts = [], []
    for ql, tl in ((150, 150), (24, 40), (150, 152), (8, 8), (150, 150)):
        q, t = related(rng, PPB, ql, tl)
        qs += q
        ts += t
    b = G.Batch.from_pairs(qs, ts)
    assert G.describe_plan(G.make_params(**KW), 150, 152) == "wavefront16_local_G8R19"
    o = O.align(b, O.make_params(**KW))
    same(engine.align_host(b, G.make_params(**KW)), o, b, "mixed")
    same(device_align(engine, b), o, b, "mixed, device")
    for k in range(5):
        s = b.slice(PPB * k, PPB * k + PPB)
        same(engine.align_host(s, G.make_params(**KW)), O.align(s, O.make_params(**KW)), s, f"block {k}")


def test_declined_block_in_the_middle(engine, g8):
    # an N at a real query position in the middle block: its flag is 0 and the int32 kernel takes
    # its 64 pairs; the blocks before and after stay on the packed kernel
    assert G.describe_plan(G.make_params(**KW), 150, 150) == "wavefront16_local_G8R19"
    qs, ts = related(np.random.default_rng(0x9E3), 3 * PPB, 150, 150)
    qs[PPB + 17] = qs[PPB + 17][:40] + b"N" + qs[PPB + 17][41:]
    b = G.Batch.from_pairs(qs, ts)
    o = O.align(b, O.make_params(**KW))
    engine.packed_pairs()
    g = device_align(engine, b)
    handled, total = engine.packed_pairs()
    assert total == 3 * PPB and handled == 2 * PPB, (handled, total)
    same(g, o, b, "declined middle block")


def test_packed_input_keeps_its_loads(engine, g8):
    # is_packed = 1 reads nibbles through load4_codes: same results as the byte input
    import ctypes
    qs, ts = related(np.random.default_rng(0x9E4), 3 * PPB + 5, 150, 150)
    b = G.Batch.from_pairs(qs, ts)
    o = O.align(b, O.make_params(**KW))
    pq, pt = np.zeros(b.q_bytes // 8, np.uint32), np.zeros(b.t_bytes // 8, np.uint32)
    O.lib().orc_pack(O._ptr(b.q_data), ctypes.c_uint32(b.q_bytes), O._ptr(pq))
    O.lib().orc_pack(O._ptr(b.t_data), ctypes.c_uint32(b.t_bytes), O._ptr(pt))
    # the packed words take half the bytes; lengths and offsets keep the unpacked units
    pad = lambda w, nbytes: np.concatenate([w.view(np.uint8), np.zeros(nbytes - 4 * len(w), np.uint8)])
    bp = G.Batch(pad(pq, b.q_bytes), b.q_offsets, b.q_lens, pad(pt, b.t_bytes), b.t_offsets, b.t_lens)
    same(engine.align_host(bp, G.make_params(is_packed=1, **KW)), o, b, "packed")


# ------------------------------------------------ the mixed launch's region boundary ----
TAIL_PPB = 16   # pairs per block of the second region's shape, G32R5: 4 waves x 2 slots x 2 pairs


def tail_p0():
    """The slot at which the planner's tail_shape (dispatch.hip) starts the second region of the
    smallest launch that has one: two whole rounds of long waves, a round being 3 waves per SIMD x 4
    SIMDs x the device's CUs, 16 pairs per wave.  The C API has no call that returns it, so the
    rule is restated here for the device the test runs on, and test_region_boundary_is_where_the_
    planner_puts_it pins it through the launch's block flags."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 2 * (3 * 4 * cus) * 16


@pytest.fixture(scope="module")
def boundary():
    """p0 + 40 pairs of 150 x 150 and their oracle results, computed once: the smallest batch with a
    second region is its first p0 + 1 pairs."""
    p0 = tail_p0()
    b = G.Batch.synth(2, p0 + 40, 0x9E7)
    return p0, b, O.align(b, O.make_params(**KW))


def cut(o, n):
    return {f: o[f][:n] for f in FIELDS}


def test_smallest_batch_with_a_second_region(engine, monkeypatch, boundary):
    # n = p0 + 1: the long region's last block is full and the second region holds one pair, in one
    # block whose other 15 slots are empty (the clamped slot min(idx, nn - 1) serves them all);
    # one pair fewer is one shape.  Both against the oracle and the one-shape launch.
    p0, b, o = boundary
    assert G.describe_plan(G.make_params(**KW), 150, 150) == "wavefront16_local_G8R19"
    for n in (p0 + 1, p0):
        s = b.slice(0, n)
        monkeypatch.setenv("GASALX_TAIL", "1")
        engine.packed_pairs()
        g = device_align(engine, s)
        handled, total = engine.packed_pairs()
        assert handled == total == n, (handled, total)
        same(g, cut(o, n), s, f"n = {n}")
        monkeypatch.setenv("GASALX_TAIL", "0")
        same(device_align(engine, s), cut(o, n), s, f"n = {n}, one shape")


def test_region_boundary_is_where_the_planner_puts_it(engine, monkeypatch, boundary):
    # n = p0 + 40: second-region blocks of 16, 16 and 8 pairs.  An IUPAC code in the pair before
    # the boundary declines the long region's last block (64 pairs), one in the pair after it the
    # second region's first (16): 80 pairs on the int32 kernel only if the second region starts
    # exactly at p0 (one shape would decline 64 + 40).
    p0, b, o = boundary
    q = b.q_data.copy()
    for i in (p0 - 1, p0):
        q[int(b.q_offsets[i]) + 3] = ord("R")
    bb = G.Batch(q, b.q_offsets, b.q_lens, b.t_data, b.t_offsets, b.t_lens)
    rows = np.array([p0 - 1, p0])
    ob = O.align(bb.slice(p0 - 1, p0 + 1), O.make_params(**KW))
    oo = {f: o[f].copy() for f in FIELDS}
    for f in FIELDS:
        oo[f][rows] = ob[f]
    monkeypatch.setenv("GASALX_TAIL", "1")
    engine.packed_pairs()
    g = device_align(engine, bb)
    handled, total = engine.packed_pairs()
    assert total == bb.n and handled == bb.n - PPB - TAIL_PPB, (handled, total)
    same(g, oo, bb, "declined blocks on both sides of the boundary")

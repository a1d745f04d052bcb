"""The plain LOCAL score kernels (wf16_body.inc, ALGO_ == WF_LOCAL) run their prologue at raised
wave priority and drop it before the sweep.  Priority changes no arithmetic; what it changes is
which wave of a block reaches the vote (__syncthreads_or), the `handled` store and the staged
tables first.  So the batches here are the smallest that vary who arrives first: one pair, a
partial wave whose last slot holds one valid pair, a second wave / a second block of one pair,
20,000 pairs of the flagship shape (many blocks per CU, prologues beside sweeps), 20,000 pairs of
8 x 8 (a sweep of a few steps: the kernel is nearly all prologue), blocks that the packed path
declines between blocks it takes, and a launch with the mixed-shape second region.

SW local a1 b4 o6 e1 through the C-ABI, score / q_end / t_end bit-exact against the oracle.
"""
import numpy as np
import pytest

import gasal_ffi as G
import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("score", "q_end", "t_end")
KW = dict(algo=G.LOCAL, match=1, mismatch=4, gap_open=6, gap_extend=1)
PPB = 64        # pairs per block at G8: 4 waves x 8 slots x 2 pairs
TAIL_PPB = 16   # at the second region's G32R5: 4 waves x 2 slots x 2 pairs
LETTERS = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module", autouse=True)
def _build():
    O.build()


@pytest.fixture
def g8(monkeypatch):
    """The flagship shape whatever the batch size (the planner gives a small batch more lanes per pair)."""
    monkeypatch.setenv("GASALX_GMIN", "8")


def related(rng, n, ql, tl):
    """n pairs: the target starts with the query's head, 8 % substituted, odd pairs shifted by a base."""
    q = LETTERS[rng.integers(0, 4, (n, ql))]
    t = LETTERS[rng.integers(0, 4, (n, tl))]
    m = min(ql, tl)
    t[:, :m] = q[:, :m]
    t[1::2, 1:m] = q[1::2, :m - 1]
    sub = rng.random((n, m)) < 0.08
    t[:, :m][sub] = LETTERS[rng.integers(0, 4, int(sub.sum()))]
    return [r.tobytes() for r in q], [r.tobytes() for r in t]


def same(g, o, b, what=""):
    for f in FIELDS:
        bad = np.nonzero(g[f] != o[f])[0]
        assert bad.size == 0, (f"{what} {f}: {bad.size}/{b.n} differ; first #{bad[0]}: gpu={g[f][bad[0]]} "
                               f"oracle={o[f][bad[0]]} q={b.q_lens[bad[0]]} t={b.t_lens[bad[0]]}")


def device_align(engine, b):
    """One device-resident call (one launch over the whole batch; the host path stages a large
    batch in chunks) over torch buffers of exactly the batch's bytes."""
    import torch
    dev = torch.device("cuda", 0)
    u = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else a).to(dev)
    d = {"q_batch": u(b.q_data), "t_batch": u(b.t_data), "q_offsets": u(b.q_offsets), "t_offsets": u(b.t_offsets),
         "q_lens": u(b.q_lens), "t_lens": u(b.t_lens)}
    for f in ("aln_score", "q_end", "t_end"):
        d[f] = torch.full((b.n,), -7, dtype=torch.int32, device=dev)
    engine.align_device_ptrs(G.make_params(**KW), {k: v.data_ptr() for k, v in d.items()}, b.q_bytes, b.t_bytes,
                             b.n, int(b.q_lens.max()), int(b.t_lens.max()))
    torch.cuda.synchronize()
    return {"score": d["aln_score"].cpu().numpy(), "q_end": d["q_end"].cpu().numpy(),
            "t_end": d["t_end"].cpu().numpy()}


def run(engine, b, o, what, declined=0, device=False):
    """One call, host-staged or device-resident: every pair as the oracle has it, and exactly
    `declined` pairs left to the int32 kernel."""
    engine.packed_pairs()                                    # forget earlier launches
    g = device_align(engine, b) if device else engine.align_host(b, G.make_params(**KW))
    handled, total = engine.packed_pairs()
    assert total == b.n and handled == b.n - declined, (what, handled, total)
    same(g, o, b, what)


def with_code(b, rows, code=b"R"):
    """The batch with an IUPAC code, which the packed path declines, at a real position of the
    queries of `rows`."""
    q = b.q_data.copy()
    for i in rows:
        q[int(b.q_offsets[i]) + min(3, int(b.q_lens[i]) - 1)] = code[0]
    return G.Batch(q, b.q_offsets, b.q_lens, b.t_data, b.t_offsets, b.t_lens)


@pytest.mark.parametrize("n", [1, 31, 65])
def test_fewest_pairs_flagship_shape(engine, g8, n):
    # G8R19, 16 pairs per wave: 1 = one slot's first half; 31 = a full wave and one whose last slot
    # holds a valid and an invalid pair; 65 = 4 x 16 + 1, a second block of one pair
    assert G.describe_plan(G.make_params(**KW), 150, 150) == "wavefront16_local_G8R19"
    qs, ts = related(np.random.default_rng(0xA10 + n), n, 150, 150)
    b = G.Batch.from_pairs(qs, ts)
    run(engine, b, O.align(b, O.make_params(**KW)), f"G8, n = {n}")


@pytest.mark.parametrize("n", [1, 31, 65])
def test_fewest_pairs_planner_shape(engine, n):
    # the shape the planner itself gives a small batch (more lanes per pair, 2 pairs per wave at
    # G64): 31 ends in a wave with one valid pair, 65 in a block of one pair, several waves and
    # blocks before them
    qs, ts = related(np.random.default_rng(0xA20 + n), n, 150, 150)
    b = G.Batch.from_pairs(qs, ts)
    run(engine, b, O.align(b, O.make_params(**KW)), f"n = {n}")


def test_config2_20000_pairs(engine):
    b = G.Batch.synth(2, 20000, 0xA30)
    ql, tl = G.synth_spec(2)
    assert (ql, tl) == (150, 150)
    assert G.describe_plan(G.make_params(**KW), ql, tl) == "wavefront16_local_G8R19"
    run(engine, b, O.align(b, O.make_params(**KW)), "config 2, 20,000 pairs")


def test_nearly_all_prologue_20000_pairs_of_8x8(engine):
    qs, ts = related(np.random.default_rng(0xA40), 20000, 8, 8)
    b = G.Batch.from_pairs(qs, ts)
    assert G.describe_plan(G.make_params(**KW), 8, 8).startswith("wavefront16_local_")
    run(engine, b, O.align(b, O.make_params(**KW)), "8 x 8, 20,000 pairs")


def test_declined_blocks_between_packed_ones(engine, g8):
    # 6 blocks of 64 and one of 5 pairs; one pair of blocks 0, 2, 3 and 6 carries the code (in
    # wave 0, in the last wave, in the middle, in the partial block): the int32 kernel takes
    # exactly those 64 + 64 + 64 + 5 pairs.  Then one pair in every block: all of them.
    assert G.describe_plan(G.make_params(**KW), 150, 150) == "wavefront16_local_G8R19"
    n = 6 * PPB + 5
    qs, ts = related(np.random.default_rng(0xA50), n, 150, 150)
    b = G.Batch.from_pairs(qs, ts)
    some = with_code(b, [0, 2 * PPB + 63, 3 * PPB + 30, 6 * PPB + 4])
    run(engine, some, O.align(some, O.make_params(**KW)), "blocks 0, 2, 3, 6 declined", declined=3 * PPB + 5)
    every = with_code(b, [k * PPB + (11 * k + 3) % 5 for k in range(7)])
    run(engine, every, O.align(every, O.make_params(**KW)), "every block declined", declined=n)


def tail_p0():
    """Where the planner's tail_shape (dispatch.hip) starts the second region of the smallest launch
    that has one: two whole rounds of long waves, a round being 3 waves per SIMD x 4 SIMDs x the
    device's CUs, 16 pairs per wave.  The block flags below pin it."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 2 * (3 * 4 * cus) * 16


def test_mixed_shape_tail_region(engine, monkeypatch):
    # 150 x 40 pairs keep the G8R19 plan (the query sets R) at a fraction of the oracle's work.
    # n = p0 + 40: wf16_mix_kernel<0,8,19,32,5>, second-region blocks of 16, 16 and 8 pairs.  With
    # a code in pair p0 the second region's first block alone is declined: 16 pairs, which shows
    # tail_b0 > 0 (one shape would decline the 40 of a G8 block).
    monkeypatch.setenv("GASALX_TAIL", "1")
    assert G.describe_plan(G.make_params(**KW), 150, 40) == "wavefront16_local_G8R19"
    p0 = tail_p0()
    qs, ts = related(np.random.default_rng(0xA60), p0 + 40, 150, 40)
    b = G.Batch.from_pairs(qs, ts)
    o = O.align(b, O.make_params(**KW))
    run(engine, b, o, "both regions", device=True)
    bb = with_code(b, [p0])
    ob = O.align(bb.slice(p0, p0 + 1), O.make_params(**KW))
    oo = {f: o[f].copy() for f in FIELDS}
    for f in FIELDS:
        oo[f][p0] = ob[f][0]
    run(engine, bb, oo, "second region's first block declined", declined=TAIL_PPB, device=True)

"""bench.py's process model, without a GPU: `--gpus N` outside torchrun starts N
ranks (torch.distributed.run on 127.0.0.1) that split one global batch into
cell-balanced contiguous shards; a mismatched --gpus under torchrun fails.
And what a plain run does: it times --steps steps, writes --dump-outputs, and
leaves the parity, CPU baseline and host-staged legs to --full."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=300, env=e)


def test_gpus_flag_spawns_ranks():
    r = _run(["--gpus", "2", "--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert sorted(x["rank"] for x in lines) == [0, 1]
    assert all(x["world"] == 2 and x["gather"] for x in lines)
    shards = sorted(tuple(x["shard"]) for x in lines)
    assert shards == [(0, 1_000_000), (1_000_000, 2_000_000)]      # weak: 1M pairs per GPU


def test_strong_workload_shards_one_global_batch():
    r = _run(["--gpus", "4", "--dry-run", "--workload", "semi"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    shards = sorted(tuple(x["shard"]) for x in lines)
    assert shards[0][0] == 0 and shards[-1][1] == 10_000_000 and len(shards) == 4
    assert all(b - a == 2_500_000 for a, b in shards)


def test_gpus_mismatch_under_torchrun_fails():
    r = _run(["--gpus", "8", "--dry-run"], env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    # outputs past the 64 MB budget: the same seeded sample of the pairs in every array and every run
    import numpy as np
    import bench
    n = 3_000_000                                   # 3 int32 fields as float64: 72 MB
    res = {"score": np.arange(n, dtype=np.int32) % 301, "q_end": np.arange(n, dtype=np.int32)[::-1] % 150,
           "t_end": np.arange(n, dtype=np.int32) % 149}
    shapes = bench.dump_outputs(str(tmp_path / "a"), res)
    bench.dump_outputs(str(tmp_path / "b"), res)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["q_end.npy", "sample_index.npy", "score.npy", "t_end.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 1000 * 1000
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and shapes["score"] == [len(idx)]
    assert len(idx) > n // 2                        # the budget is used, not a token sample
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b)
        if f != "sample_index.npy":
            assert np.array_equal(a, res[f[:-4]][idx.astype(np.int64)])


def test_dump_outputs_cigar_rows(tmp_path):
    # one row per pair: the first n_ops bytes of its pad8(ql) slot, zeros after them; a pair whose
    # CIGAR (or whose left neighbour's) overflows its slot is order-dependent and written as zeros
    import numpy as np
    import bench
    q_lens = np.array([5, 16, 8, 8, 3], np.uint32)
    q_offs = np.array([0, 8, 24, 32, 40], np.uint32)
    cigar = np.arange(1, 49, dtype=np.uint8)
    n_ops = np.array([3, 16, 9, 2, 0], np.uint32)   # pair 2 overflows its 8-byte slot into pair 3's
    res = {"score": np.array([1.5, 2, 3, 4, 5], np.float32), "n_ops": n_ops, "cigar": cigar}
    bench.dump_outputs(str(tmp_path), res, q_offsets=q_offs, q_lens=q_lens)
    rows = np.load(tmp_path / "cigar.npy")
    assert rows.dtype == np.float32 and rows.shape == (5, 16)
    want = np.zeros((5, 16), np.float32)
    want[0, :3] = cigar[0:3]
    want[1, :16] = cigar[8:24]
    assert np.array_equal(rows, want)
    assert np.load(tmp_path / "score.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "n_ops.npy"), n_ops.astype(np.float64))
    assert not os.path.exists(tmp_path / "sample_index.npy")


def test_plain_run_times_steps_and_dumps_cpu_workload(tmp_path):
    # the config-1 workload runs on the host: --steps sets the timed passes, the line carries
    # ms_per_step, --dump-outputs holds what the timed path computed, and the same arguments give
    # the same arrays again
    import numpy as np
    import gasal_ffi as G
    import oracle as O
    outs = []
    for d in ("a", "b"):
        r = _run(["--gpus", "1", "--workload", "cpu_plumbing", "--steps", "2", "--warmup", "1", "--dump-outputs",
                  str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1]))
    line = outs[0]
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "GCUPS" and line["higher_is_better"] is True and line["value"] > 0
    batch = G.Batch.synth(1, 1024, 0x5EED0001)
    ref = O.align(batch, O.make_params(algo=O.LOCAL), n_threads=1)
    for f in ("score", "q_end", "t_end"):
        a = np.load(tmp_path / "a" / f"{f}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, ref[f])
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{f}.npy"))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_timed_outputs(tmp_path):
    # a plain run: the timed steps and the result line, nothing that --full adds; the dumped
    # arrays are the last timed step's device outputs, bit-exact against the oracle
    import numpy as np
    import gasal_ffi as G
    import oracle as O
    n = 4099
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", str(n), "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["parity"] is None and "cpu_baseline" not in line and "end_to_end" not in line
    batch = G.Batch.synth(2, n, 0x5EED0002)
    ref = O.align(batch, O.make_params(algo=O.LOCAL))
    for f in ("score", "q_end", "t_end"):
        a = np.load(tmp_path / f"{f}.npy")
        assert a.dtype == np.float64 and a.shape == (n,) and np.array_equal(a, ref[f])

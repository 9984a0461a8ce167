"""CPU test of bench.py's N-rank launch: started with --gpus 2 (no WORLD_SIZE)
it re-launches itself under torch.distributed.run with two ranks, and the
line rank 0 prints reports n_gpus = 2 (dry run: the packed-block all-gather
over gloo, no GPU)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_dry_run_two_ranks_reports_two_gpus():
    out = _run("--gpus", "2", "--dry-run")
    assert out["n_gpus"] == 2 and out["config"]["dry_run"]


def test_full_is_off_by_default_and_dump_outputs_writes_float_arrays(tmp_path):
    import numpy as np

    import bench

    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", str(tmp_path / "o")])
    assert a.full is True and a.dump_outputs == str(tmp_path / "o")
    # ids arrive as the packed block's uint64 or as the merge's int64 tensors; counts as int32
    ids = np.array([[2**40 + 3, 5], [7, 2**33]], np.int64)
    dists = np.array([[0.5, 1.5], [0.25, 2.0]], np.float32)
    bench.dump_outputs(a.dump_outputs, ids, dists, np.array([2, 2], np.int32))
    got = {s: np.load(tmp_path / "o" / f"{s}.npy") for s in ("ids", "dists", "counts")}
    assert got["ids"].dtype == np.float64 and np.array_equal(got["ids"].astype(np.int64), ids)
    assert got["dists"].dtype == np.float32 and np.array_equal(got["dists"], dists)
    assert got["counts"].dtype == np.float64 and np.array_equal(got["counts"], [2.0, 2.0])


def test_world_size_must_match_gpus():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert p.returncode != 0 and "WORLD_SIZE" in p.stderr

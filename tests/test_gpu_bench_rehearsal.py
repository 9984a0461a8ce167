"""The multi-GPU bench code on a one-GPU box (the driver's SCALE runs exactly
this code at N = 2, 4, 8 on an 8-GPU node): bench.py --gpus 2 --share-gpu
re-launches itself as two ranks on cuda:0 that exchange their packed top-k
blocks over gloo, and --workload slab1b deals 8 slabs to the ranks.  Each run
checks its merged results against the oracle's top-k over every shard's rows
(bench.py merge_check) -- here at sizes the host oracle finishes in seconds."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args, timeout=240, full=True):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    # --full: the oracle checks of the merged results and the scale legs are not part of a plain run
    legs = ["--full", "--no-cpu-baseline", "--configs", ""] if full else []
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *legs, *args],
                       capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


@pytest.mark.parametrize("gpus", [2, 3])
def test_flat_share_gpu_exchange_and_merge(gpus):
    out = run_bench("--gpus", str(gpus), "--share-gpu", "--rows", "300000", "--steps", "3", "--warmup", "1",
                    "--s1b-rows", "4000000", "--pq-rows", "400000")
    assert out["n_gpus"] == gpus and out["value"] > 0
    assert out["merge_check"]["ok"] is True, out["merge_check"]
    # the strong-scaling legs the driver's SCALE line carries (configs[4] and configs[3]), at test sizes
    legs = out["configs"]
    if gpus == 3:
        assert "skipped" in legs["config5_1b_x_128"]
    else:
        assert legs["config5_1b_x_128"]["slabs_per_gpu"] == 8 // gpus
        assert legs["config5_1b_x_128"]["merge_check"]["ok"] is True, legs["config5_1b_x_128"]
    assert legs["config4_pq_sharded"]["merge_check"]["ok"] is True, legs["config4_pq_sharded"]
    assert legs["config4_pq_sharded"]["rows_per_gpu"] >= 400000 // gpus
    # the one-process multi-GPU leg needs N devices in one process: skipped on a shared GPU
    assert "skipped" in legs["multi_gpu_one_process"]


def test_plain_run_is_headline_only_and_dumps_outputs(tmp_path, orc):
    """Without --full the line carries the headline and nothing that needs a
    run of its own; --dump-outputs writes the last timed step's results, which
    equal the oracle's top-k for that step's queries."""
    import numpy as np

    n, d, k, B, steps, warmup = 300_000, 128, 10, 16, 3, 1
    out = run_bench("--gpus", "1", "--rows", str(n), "--steps", str(steps), "--warmup", str(warmup),
                    "--dump-outputs", str(tmp_path / "o"), full=False)
    assert out["full"] is False and out["steps"] == steps and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["roofline"]["launches"] == steps and out["roofline"]["achieved"] > 0
    for key in ("merge_check", "configs", "cpu_baseline"):
        assert out[key] is None, key
    assert out["roofline"]["achieved_no_reuse"] is None and out["roofline"]["ceiling_GBps"] is None
    ids, dists, counts = (np.load(tmp_path / "o" / f"{s}.npy") for s in ("ids", "dists", "counts"))
    assert ids.dtype == np.float64 and dists.dtype == np.float32 and counts.dtype == np.float64
    assert ids.shape == dists.shape == (B, k) and counts.shape == (B,) and np.all(counts == k)
    q0 = ((warmup + steps - 1) * B) % 64  # the last timed step's queries (bench.py run_flat1m)
    qs = np.random.default_rng(43).uniform(-1, 1, (64, d)).astype(np.float32)[q0:q0 + B]
    rows = orc.synth_rows(42, 0, n, d, 0)
    for qi in range(B):
        wi, wd = orc.lex_topk(orc.dist_all(orc.L2, qs[qi], rows), np.arange(n, dtype=np.uint64), k)
        assert np.array_equal(ids[qi].astype(np.uint64), wi)
        assert np.array_equal(dists[qi].view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("gpus", [1, 2])
def test_slab1b_deal_merge(gpus):
    args = ["--workload", "slab1b", "--rows", "4000000", "--steps", "2", "--warmup", "1", "--gpus", str(gpus)]
    if gpus > 1:
        args.append("--share-gpu")
    out = run_bench(*args)
    assert out["config"]["slabs"] == 8 and out["config"]["slabs_per_gpu"] == 8 // gpus
    assert out["merge_check"]["ok"] is True, out["merge_check"]

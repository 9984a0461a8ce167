#!/usr/bin/env python3
"""The multi-GPU BQ heap flow's overhead on ONE GPU (wvg_multi_search_bq_candidates).

    python tools/bench_multi_bq.py [--rows 8000000] [--dim 1536] [--slabs 8] [--R 200]
                                   [--calls 200] [--out profiles/r08/multi_bq]
    python tools/bench_multi_bq.py --falling     (the overflow probe of tests/test_gpu_multi_bq.py)

A synthetic BQ corpus is dealt to `slabs` slabs of device 0 (devices = [0] *
slabs: the peer-copy exchange) and, in the same run, loaded into one plain
corpus, the baseline (wvg_search_bq_candidates).  Reported per leg (single
queries, a 16-query batch): p50 / p99 ms per call, and for the multi legs the
rows replayed through the host heap per query with the cross-slab bound on and
off (tuning key 36, wvgx_multi_bq_counters: tools build only).  Eight slabs on
one GPU serialise their scans, so this isolates what the exchange, the extra
launches and the host replay cost; it says nothing about multi-GPU scaling.
Needs the tools build: make -C weaviate_amd/csrc tools.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("WVG_LIB", os.path.join(ROOT, "tools", "libwvgpu_tools.so"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()  # torch's HIP context first (as bench.py does before the library's)
from oracle import wv_oracle as orc  # noqa: E402
from weaviate_amd import _lib  # noqa: E402
from weaviate_amd._lib import KIND_BQ, METRIC_L2  # noqa: E402
from weaviate_amd.device import (Context, Corpus, Multi, MultiCorpus, multi_search_bq_candidates,  # noqa: E402
                                 search_bq_candidates)

lib = _lib.load()
lib.wvgx_set_tuning.restype = ctypes.c_int
lib.wvgx_set_tuning.argtypes = [ctypes.c_int, ctypes.c_int]
lib.wvgx_multi_bq_counters.restype = ctypes.c_int
lib.wvgx_multi_bq_counters.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]


def counters(reset=True):
    """[multi calls, queries, rows replayed, overflow reruns]"""
    out = (ctypes.c_uint64 * 4)()
    lib.wvgx_multi_bq_counters(out, 1 if reset else 0)
    return [int(x) for x in out]


def timed(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    t = np.empty(calls)
    for i in range(calls):
        t0 = time.perf_counter()
        fn()
        t[i] = time.perf_counter() - t0
    return {"p50_ms": round(float(np.percentile(t, 50)) * 1e3, 4), "p99_ms": round(float(np.percentile(t, 99)) * 1e3, 4),
            "mean_ms": round(float(t.mean()) * 1e3, 4), "calls": calls}


def same(a, b):
    return bool(np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and
                np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


def main_bench(a):
    n, d, R = a.rows, a.dim, a.R
    qs = orc.synth_rows(4242, 0, 64, d, 0)
    res = {"rows": n, "dim": d, "slabs": a.slabs, "R": R, "devices": [0] * a.slabs,
           "note": "all slabs on one GPU: scans serialise; overhead of exchange + host replay only"}
    with Context(0) as ctx, Multi([0] * a.slabs) as m:
        plain = Corpus(ctx, KIND_BQ, METRIC_L2, d, n)
        mc = MultiCorpus(m, KIND_BQ, METRIC_L2, d, n)
        try:
            plain.fill_synthetic(42, n, 0)
            mc.fill_synthetic(42, n, 0)
            res["results_equal_plain"] = same(multi_search_bq_candidates(mc, qs[:16], R),
                                              search_bq_candidates(plain, qs[:16], R))
            it = [0]

            def one(call, corpus, batch):
                def f():
                    i = it[0] = (it[0] + 1) % (64 - batch + 1)
                    call(corpus, qs[i:i + batch], R)
                return f

            for name, batch, calls in (("single", 1, a.calls), ("batch16", 16, max(20, a.calls // 4))):
                leg = {"plain": timed(one(search_bq_candidates, plain, batch), calls)}
                for bound in (1, 0):
                    lib.wvgx_set_tuning(36, bound)
                    counters()
                    t = timed(one(multi_search_bq_candidates, mc, batch), calls)
                    c = counters()
                    t["rows_replayed_per_query"] = round(c[2] / max(c[1], 1), 1)
                    t["overflow_reruns"] = c[3]
                    leg["multi_bound_on" if bound else "multi_bound_off"] = t
                lib.wvgx_set_tuning(36, 1)
                res[name] = leg
        finally:
            mc.destroy()
            plain.destroy()
    return res


def main_falling(a):
    """tests/test_gpu_multi_bq.py::test_falling_distances_across_two_slabs' input: do the per-wave
    buffers overflow (a rerun) at slabs of 200,000 rows, and how many rows reach the host heap?"""
    n, d = 400_000, 1536
    w = d // 64
    nb = (1536 - (np.arange(n) % 1500)).astype(np.int64)
    codes = np.zeros((n, w), np.uint64)
    for j in range(w):
        c = np.clip(nb - 64 * j, 0, 64)
        codes[:, j] = np.where(c >= 64, np.uint64(0xFFFFFFFFFFFFFFFF),
                               (np.left_shift(np.uint64(1), np.minimum(c, 63).astype(np.uint64)) - np.uint64(1)))
    q = np.ones((2, d), np.float32)
    res = {"input": "falling distances, 400,000 x 1536, devices [0, 0]", "runs": []}
    with Multi([0, 0]) as m:
        mc = MultiCorpus(m, KIND_BQ, METRIC_L2, d, n)
        try:
            for i in range(2):
                h, base, slab = mc.shard(i)
                ids = np.arange(base, min(n, base + slab), dtype=np.uint64)
                part = np.ascontiguousarray(codes[base:base + slab])
                _lib.check(lib.wvg_corpus_upsert_codes(h, _lib.u64ptr(ids), part.ctypes.data_as(ctypes.c_void_p),
                                                       len(ids)))
            for bound in (1, 0):
                lib.wvgx_set_tuning(36, bound)
                for R in (1, 4, 200, 600):
                    for nq in (2, 1):
                        counters()
                        multi_search_bq_candidates(mc, q[:nq], R)
                        c = counters()
                        res["runs"].append({"bound": bound, "R": R, "nq": nq, "rows_replayed_per_query": c[2] / nq,
                                            "overflow_reruns": c[3]})
            lib.wvgx_set_tuning(36, 1)
        finally:
            mc.destroy()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--slabs", type=int, default=8)
    ap.add_argument("--R", type=int, default=200)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--falling", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "multi_bq"))
    args = ap.parse_args()
    result = main_falling(args) if args.falling else main_bench(args)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "falling.json" if args.falling else "bench_multi_bq.json")
    with open(path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))

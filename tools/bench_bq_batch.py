#!/usr/bin/env python3
"""Batched BQ Hamming search: batch_screen = 5 (K5m, the int8 MFMA kernel) against the default context (the
parent route: co-scheduled K5, one XOR + popcount scan of the codes per query) on one box.

Every measurement is a fresh child process (this script with --child), and the two settings alternate shape
by shape, so clock and cache state drift hits both alike.  A child fills the corpus, runs two warm batches,
then at least --reps batches and at least --min-seconds of them, a synchronize each; it prints one JSON line
with the median and p10-p90 of the batch time, the plan, checksums of ids and distance bits (the two settings
must agree on them) and, for a K5m batch, the whole call's int8 rate -- nq x rows x padded bits x 2 operations
over the batch time, merge and query image included, so a lower bound of the scoring launch's -- against the
5 POP/s peak.  Device API, queries in HBM.  Tooling only (product library).

  tools/bench_bq_batch.py                      every shape of the issue (100M x 1536 needs ~20 GB of HBM)
  tools/bench_bq_batch.py --shapes 10000000x1536 --ks 200 --nqs 1024"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# rows x dim : k list : nq list
SHAPES = "100000000x1536:10,200:1024;10000000x1536:200:1024,64;1000000x768:200:1024;10000000x128:200:1024"
PEAK_INT8 = 5.0e15


def child(a):
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    torch.cuda.init()
    from weaviate_amd import _lib
    from weaviate_amd.device import Context, Corpus

    n, d = (int(x) for x in a.child.split("x"))
    nq, k = a.nq, a.k
    dev = torch.device("cuda:0")
    tq = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (nq, d)).astype(np.float32)).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with Context(0, batch_screen=a.batch_screen, mfma_min_queries=32) as ctx:
        lib = ctx.lib
        c = Corpus(ctx, _lib.KIND_BQ, _lib.METRIC_L2, d, n)
        c.fill_synthetic(42, n, 0)
        ctx.synchronize()
        wsb = lib.wvg_search_workspace_size(c.handle, nq, k)
        ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oc = torch.empty(nq, dtype=torch.int32, device=dev)
        each = []
        while len(each) < 2 + a.reps or sum(each[2:]) < a.min_seconds * 1e3:  # (the first two: warm, dropped)
            t0 = time.perf_counter()
            _lib.check(lib.wvg_search_device(c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                             oc.data_ptr(), ws.data_ptr(), wsb, st))
            torch.cuda.synchronize()
            each.append((time.perf_counter() - t0) * 1e3)
        each = each[2:]
        p10, med, p90 = (round(float(x), 3) for x in np.percentile(each, [10, 50, 90]))
        plan, rate = c.batch_plan(nq, k), {}
        if plan["matrix"]:
            ops = 2.0 * nq * ((n + 63) // 64 * 64) * ((d + 511) // 512 * 512)
            rate = {"call_int8_ops_per_s": round(ops / (med * 1e-3), 0),
                    "call_share_of_int8_peak": round(ops / (med * 1e-3) / PEAK_INT8, 4)}
        print(json.dumps(rate | {
            "config": f"{n} x {d} BQ, {nq} queries, k={k}, batch_screen={a.batch_screen}",
            "plan": plan, "workspace_bytes": int(wsb), "batch_ms_median": med,
            "batch_ms_p10_p90": [p10, p90], "qps": round(nq / med * 1e3, 1), "reps": len(each),
            "result_crc": int(np.bitwise_xor.reduce(oi.cpu().numpy().view(np.uint64).ravel()) & 0xFFFFFFFF),
            "dist_sum_bits": int(od.cpu().numpy().view(np.uint32).astype(np.uint64).sum())}), flush=True)
        c.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="rows x dim : k,k : nq,nq ; ...")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--min-seconds", type=float, default=0.5, help="least timed work per measurement")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the two settings per shape")
    ap.add_argument("--child", default="", help="(internal) one shape, one setting, in this process")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--batch-screen", type=int, default=5)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for spec in a.shapes.split(";"):
        shape, ks, nqs = spec.split(":")
        for k in ks.split(","):
            for nq in nqs.split(","):
                for _ in range(a.rounds):
                    for bs in (5, 2):  # a fresh process each: never a new program in one that holds the GPU
                        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--nq", nq,
                                        "--k", k, "--reps", str(a.reps), "--min-seconds", str(a.min_seconds),
                                        "--batch-screen", str(bs)], check=True)


if __name__ == "__main__":
    main()

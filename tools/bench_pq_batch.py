#!/usr/bin/env python3
"""Batched PQ ADC search: batch_screen = 6 (K8m, the bf16 MFMA screen over rows decoded in the kernel + the exact
LUT rescore) or batch_screen = 7 (K8m-S as well: codebooks beyond LDS, --batch-screen 7 --shapes SLICE_SHAPES)
against the default context (the parent route: one ADC scan per query, co-scheduled at m = 32) on one box.

Every measurement is a fresh child process (this script with --child), and the two settings alternate shape by
shape, so clock and cache state drift hits both alike.  A child sets a uniform codebook, fills the corpus with
uniform random codes, runs two warm batches, then at least --reps batches and at least
--min-seconds of them, a synchronize each; it prints one JSON line with the median and p10-p90 of the batch
time, the plan, checksums of ids and distance bits (the two settings must agree on them) and, for a K8m batch,
the whole call's bf16 rate -- 2 x nq x rows x dim operations over the batch time, norms pass, rescore and merge
included, so a lower bound of the screen launch's -- against the 2.5 PFLOP/s peak.  Flagged queries and rescored
rows are not counted: the kernels have no counter for them.  Device API, queries in HBM.  Tooling only.

  tools/bench_pq_batch.py                      every shape of the issue (100M x 128, m = 32 needs ~4 GB of HBM)
  tools/bench_pq_batch.py --batch-screen 7 --shapes slice      K8m-S's shapes (SLICE_SHAPES)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# rows x dim x m : k list : nq list
SHAPES = "100000000x128x32:10,200:1024,64;10000000x128x32:10:1024;1000000x128x32:10:1024;10000000x128x16:10:1024"
# K8m-S (--batch-screen 7): 10M x 768 m = 96, 10M x 1536 m = 192, 10M x 384 m = 96 (dsub 4), 1M x 768; where K8m
# lost: 64 queries, and k = 200, at 10M x 768
SLICE_SHAPES = ("10000000x768x96:10:1024;10000000x1536x192:10:1024;10000000x384x96:10:1024;1000000x768x96:10:1024;"
                "10000000x768x96:10:64;10000000x768x96:200:1024")
PEAK_BF16 = 2.5e15


def child(a):
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    torch.cuda.init()
    from weaviate_amd import _lib
    from weaviate_amd.device import Context, Corpus

    n, d, m = (int(x) for x in a.child.split("x"))
    nq, k = a.nq, a.k
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    tq = torch.from_numpy(rng.uniform(-1, 1, (nq, d)).astype(np.float32)).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with Context(0, batch_screen=a.batch_screen, mfma_min_queries=32) as ctx:
        lib = ctx.lib
        c = Corpus(ctx, _lib.KIND_PQ, _lib.METRIC_L2, d, n)
        c.set_codebook(rng.uniform(-1, 1, (m, 256, d // m)).astype(np.float32))
        for r0 in range(0, n, 1 << 22):  # uniform random codes (the synthetic fill has no PQ form)
            r1 = min(n, r0 + (1 << 22))
            c.upsert_codes(np.arange(r0, r1, dtype=np.uint64), rng.integers(0, 256, (r1 - r0, m), dtype=np.uint8))
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
            ops = 2.0 * nq * n * d
            rate = {"call_bf16_flop_per_s": round(ops / (med * 1e-3), 0),
                    "call_share_of_bf16_peak": round(ops / (med * 1e-3) / PEAK_BF16, 4)}
        print(json.dumps(rate | {
            "config": f"{n} x {d} PQ m={m} ks=256, {nq} queries, k={k}, batch_screen={a.batch_screen}",
            "plan": plan, "workspace_bytes": int(wsb), "batch_ms_median": med,
            "batch_ms_p10_p90": [p10, p90], "qps": round(nq / med * 1e3, 1), "reps": len(each),
            "result_crc": int(np.bitwise_xor.reduce(oi.cpu().numpy().view(np.uint64).ravel()) & 0xFFFFFFFF),
            "dist_sum_bits": int(od.cpu().numpy().view(np.uint32).astype(np.uint64).sum())}), flush=True)
        c.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="rows x dim x m : k,k : nq,nq ; ...")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--min-seconds", type=float, default=0.5, help="least timed work per measurement")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the two settings per shape")
    ap.add_argument("--child", default="", help="(internal) one shape, one setting, in this process")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batch-screen", type=int, default=6, help="6 (K8m) or 7 (K8m and K8m-S) against the default")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.shapes == "slice":
        a.shapes = SLICE_SHAPES
    for spec in a.shapes.split(";"):
        shape, ks, nqs = spec.split(":")
        for k in ks.split(","):
            for nq in nqs.split(","):
                for _ in range(a.rounds):
                    for bs in (a.batch_screen, 2):  # a fresh process each: never a new program in one that holds the GPU
                        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--nq", nq,
                                        "--k", k, "--reps", str(a.reps), "--min-seconds", str(a.min_seconds),
                                        "--batch-screen", str(bs)], check=True)


if __name__ == "__main__":
    main()

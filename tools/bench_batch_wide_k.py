#!/usr/bin/env python3
"""Batched k-NN at 16 < k <= 256: batch_screen = 4 (K3c-W, the wide bf16 screen) against batch_screen = 2
(the parent route: K3b for dot / cosine, the co-scheduled K1 / K1Q scans for l2-squared) on one box.

Every measurement is a fresh child process (this script with --child), and the two settings alternate
shape by shape, so clock and cache state drift hits both alike.  A child fills the corpus, runs two warm
batches (the first builds the shadow), then at least --reps batches and at least --min-seconds of them, a
synchronize each; it prints one JSON line with the median and p10-p90 of the batch time, the plan, checksums
of ids and distance bits (the two settings must agree on them) and, for a K3c-W batch, the flagged queries
and the rescored rows per query of the last batch, read from the workspace (wide_layout mirrors screen_ws
and screen_wide_ranges).  Device API, queries in HBM.  Tooling only (product library).

  tools/bench_batch_wide_k.py                      every shape of the issue (10M x 768 needs ~50 GB of HBM)
  tools/bench_batch_wide_k.py --shapes 1000000x128xl2 --ks 100 --nqs 1024"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = "10000000x768xcosine,10000000x768xl2,1000000x128xl2"


def wide_layout(n, nq, k, d, l2, num_cus):
    """(row ranges, pool keys, byte offset of the flagged-query count) of a K3c-W workspace, after the 256-byte
    status block: screen_wide_ranges (wvg_screen.hip) and screen_ws (wvg_search.hip).  Keep in step with both: after
    a change to the carve order this would read another word of the zero-filled workspace, most likely 0."""
    sys.path.insert(0, HERE)
    from screen_bench import screen_nrr

    P = 2 * max(k, 64) + 256
    nqb, nblk = (nq + 127) // 128, ((n + 63) // 64 + 3) // 4
    want, cap = screen_nrr(n, nq, num_cus), (256 << 20) // (nq * P * 8)
    if want > cap:
        want = max(8, cap // 8 * 8)
        step = math.lcm(8, num_cus // math.gcd(num_cus, nqb))
        if want >= step:
            want = want // step * step
    nrr = max(1, min(want, nblk))
    nq_pad, kbn = (nq + 127) // 128 * 128, (d + 31) // 32 if l2 else (d + 63) // 64 * 2
    off = 0
    for b in (nq * nrr * P * 8, nq * 4, nq_pad // 16 * kbn * 1024, nq_pad * 4, nq_pad * 4, nq_pad * 4, nq * 4):
        off = (off + b + 255) // 256 * 256
    return nrr, P, off


def child(a):
    sys.path.insert(0, os.path.dirname(HERE))
    import torch

    torch.cuda.init()
    from weaviate_amd import _lib
    from weaviate_amd.device import Context, Corpus

    n, d, metric = a.child.split("x")
    n, d, nq, k = int(n), int(d), a.nq, a.k
    metric_id = {"l2": _lib.METRIC_L2, "dot": _lib.METRIC_DOT, "cosine": _lib.METRIC_COSINE}[metric]
    dev = torch.device("cuda:0")
    tq = torch.from_numpy(np.random.default_rng(7).uniform(0, 1, (nq, d)).astype(np.float32)).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with Context(0, batch_screen=a.batch_screen) as ctx:
        lib = ctx.lib
        c = Corpus(ctx, _lib.KIND_F32, metric_id, d, n)
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
        plan, wide = c.batch_plan(nq, k), {}
        if plan["screen"] and k > 16:
            nrr, P, nf = wide_layout(n, nq, k, d, metric == "l2", torch.cuda.get_device_properties(dev).multi_processor_count)
            keys = ws[256:256 + nq * nrr * P * 8].cpu().numpy().view(np.uint64)
            wide = {"row_ranges": nrr, "pool_keys": P,
                    "flagged_queries": int(ws[256 + nf:256 + nf + 4].cpu().numpy().view(np.uint32)[0]),
                    "rescored_rows_per_query": round(int((keys != np.iinfo(np.uint64).max).sum()) / nq, 2)}
        print(json.dumps(wide | {
            "config": f"{n} x {d} {metric}, {nq} queries, k={k}, batch_screen={a.batch_screen}",
            "plan": plan, "workspace_bytes": int(wsb), "batch_ms_median": med,
            "batch_ms_p10_p90": [p10, p90], "qps": round(nq / med * 1e3, 1), "reps": len(each),
            "result_crc": int(np.bitwise_xor.reduce(oi.cpu().numpy().view(np.uint64).ravel()) & 0xFFFFFFFF),
            "dist_sum_bits": int(od.cpu().numpy().view(np.uint32).astype(np.uint64).sum())}), flush=True)
        c.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="rows x dim x metric, comma separated")
    ap.add_argument("--ks", default="17,100,256")
    ap.add_argument("--nqs", default="1024,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--min-seconds", type=float, default=0.5, help="least timed work per measurement")
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the two settings per shape")
    ap.add_argument("--child", default="", help="(internal) one shape, one setting, in this process")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--batch-screen", type=int, default=4)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for shape in a.shapes.split(","):
        for k in a.ks.split(","):
            for nq in a.nqs.split(","):
                for _ in range(a.rounds):
                    for bs in (4, 2):  # a fresh process each: never a new program in one that holds the GPU
                        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--nq", nq,
                                        "--k", k, "--reps", str(a.reps), "--min-seconds", str(a.min_seconds),
                                        "--batch-screen", str(bs)], check=True)


if __name__ == "__main__":
    main()

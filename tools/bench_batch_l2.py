#!/usr/bin/env python3
"""Batched 10-NN over an fp32 l2-squared corpus: one run of one shape.  Device
API (queries in HBM), batches back to back on one stream; HIP events bound to
the scoring launch(es) (wvg_profile_start / _stop).

  --metric l2   the route the library takes for the batch (K3c-L2 = the bf16
                screen + exact rescore where Corpus.batch_plan says so, else the
                co-scheduled K1 / K1Q scans); --batch-screen 0 forces the latter
  --metric dot  K3c's yardstick: a dot corpus of the same shape (use
                --batch-screen 1 at d = 128 / 1536, where bf16 picks K3c)

--root points at another checkout's tree (a build of the parent commit) so both
can be timed on one box, interleaved by the caller.  Prints one JSON line:
batch_ms, qps, scoring_kernel_ms, bf16_peak_frac (2 Q N d FLOP / kernel time
against 2.5 PFLOP/s dense bf16; screened routes only), flagged queries and
rescored rows per query of the last batch.  Tooling only (product library)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--metric", default="l2", choices=["l2", "dot"])
    ap.add_argument("--batch-screen", type=int, default=2)
    ap.add_argument("--root", default=os.path.dirname(HERE), help="tree whose weaviate_amd package to load")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch

    torch.cuda.init()
    from weaviate_amd._lib import LIB_PATH, KIND_F32, METRIC_DOT, METRIC_L2, check  # (before screen_bench, which
    from weaviate_amd.device import Context, Corpus                                # puts its own tree first)

    sys.path.insert(0, HERE)
    from screen_bench import screen_nflag_offset, screen_offsets

    metric = METRIC_L2 if a.metric == "l2" else METRIC_DOT
    dev = torch.device("cuda:0")
    n, d, nq, k = a.rows, a.dim, a.nq, a.k
    q = np.random.default_rng(7).uniform(0, 1, (nq, d)).astype(np.float32)  # uniform as the rows (distribution 0)
    tq = torch.from_numpy(q).to(dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with Context(0, batch_screen=a.batch_screen) as ctx:
        lib = ctx.lib
        c = Corpus(ctx, KIND_F32, metric, d, n)
        c.fill_synthetic(42, n, 0)
        ctx.synchronize()
        plan = c.batch_plan(nq, k) if hasattr(c, "batch_plan") else None
        screened = bool(plan["screen"]) if plan else metric == METRIC_DOT and a.batch_screen != 0 and nq >= 32
        wsb = lib.wvg_search_workspace_size(c.handle, nq, k)
        ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oc = torch.empty(nq, dtype=torch.int32, device=dev)

        def run():
            check(lib.wvg_search_device(c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                        ws.data_ptr(), wsb, st))

        t0 = time.time()
        run()  # a screened route builds the shadow here
        torch.cuda.synchronize()
        first_s = time.time() - t0
        run()
        torch.cuda.synchronize()
        check(lib.wvg_profile_start(ctx.handle))
        t0 = time.time()
        for _ in range(a.reps):
            run()
        torch.cuda.synchronize()
        wall = (time.time() - t0) / a.reps
        ms, nl = ctypes.c_double(), ctypes.c_uint64()
        check(lib.wvg_profile_stop(ctx.handle, ctypes.byref(ms), ctypes.byref(nl)))
        kern_ms = ms.value / max(1, a.reps)
        out = {"label": a.label, "config": f"{n} x {d} {a.metric}, {nq} queries, k={k}, batch_screen={a.batch_screen}",
               "plan": plan, "lib": os.path.relpath(LIB_PATH, os.path.dirname(HERE)), "batch_ms": round(wall * 1e3, 3), "qps": round(nq / wall, 1),
               "scoring_ms_per_batch": round(kern_ms, 3), "profiled_launches": int(nl.value),
               "first_call_s": round(first_s, 3),
               "result_crc": int(np.bitwise_xor.reduce(oi.cpu().numpy().view(np.uint64).ravel()) & 0xFFFFFFFF),
               "dist_sum_bits": int(od.cpu().numpy().view(np.uint32).astype(np.uint64).sum())}
        if screened:
            flop = 2.0 * nq * n * d
            out["bf16_peak_frac"] = round(flop / (kern_ms / 1e3) / 2.5e15, 3)
            out["flagged_queries"] = int(ws[256 + screen_nflag_offset(n, nq, k, d):][:4].cpu().numpy().view(np.uint32)[0])
            co, ncand, _ = screen_offsets(n, nq, k, d)
            cand = ws[256 + co:256 + co + nq * ncand * 8].cpu().numpy().view(np.uint64)
            out["rescored_rows_per_query"] = round(int((cand != np.iinfo(np.uint64).max).sum()) / nq, 2)
        print(json.dumps(out), flush=True)
        c.destroy()


if __name__ == "__main__":
    main()

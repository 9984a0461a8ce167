"""BQ search with exact rescore for a caller whose queries and results live in HBM, two ways on one GPU:

  new:  wvg_search_device_bq_rescore -- Hamming top-R and the fused rescore on the stream, one synchronize at the end;
  old:  what such a caller did before it: wvg_search_device_pipelined (R <= 256; wvg_search_device above) for the
        R candidates, synchronize, ids to the host, wvg_corpus_distance_by_ids_batch (host pointers, the rows stay on
        the GPU), the top-k by (distance, id) on the host, results back to the device.

The two are timed interleaved (old, new, old, new, ...) with a host clock around work that ends in a synchronize,
after warm-up calls of each; the results of the two routes are compared for equality first.  One JSON line per shape:
median, p10 and p90 of each route in microseconds, and new / old.

  python tools/bench_bq_rescore_device.py [--rows 10000000] [--reps 40] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1536, 200, 10, 16), (128, 200, 10, 16), (1536, 300, 10, 16)]  # (d, rescore_limit, k, nq)


def main():
    import torch

    from oracle import wv_oracle as orc
    from weaviate_amd import _lib
    from weaviate_amd._lib import KIND_BQ, KIND_F32, METRIC_L2
    from weaviate_amd.device import (Context, Corpus, search_device_bq_rescore,
                                     search_device_bq_rescore_workspace_size)

    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
    dev = torch.device("cuda:0")
    lines = []
    with Context(0) as ctx:
        lib = ctx.lib
        for d, rl, k, nq in SHAPES:
            R = max(rl, k)
            bq = Corpus(ctx, KIND_BQ, METRIC_L2, d, args.rows)
            f32 = Corpus(ctx, KIND_F32, METRIC_L2, d, args.rows)
            bq.fill_synthetic(42, args.rows, 0)
            f32.fill_synthetic(42, args.rows, 0)
            qs = orc.synth_rows(43, 0, nq, d, 0)
            tq = torch.from_numpy(qs).to(dev)
            s = torch.cuda.current_stream().cuda_stream
            ws = torch.zeros(search_device_bq_rescore_workspace_size(bq, f32, nq, k, rl), dtype=torch.uint8, device=dev)
            ci = torch.empty((nq, R), dtype=torch.int64, device=dev)
            cd = torch.empty((nq, R), dtype=torch.float32, device=dev)
            cc = torch.empty(nq, dtype=torch.int32, device=dev)
            out = [(torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev),
                    torch.empty(nq, dtype=torch.int32, device=dev)) for _ in range(2)]
            hi = torch.empty((nq, k), dtype=torch.int64).pin_memory()
            hd = torch.empty((nq, k), dtype=torch.float32).pin_memory()
            stage1 = lib.wvg_search_device_pipelined if R <= 256 else lib.wvg_search_device

            def new():
                oi, od, oc = out[0]
                search_device_bq_rescore(bq, f32, tq.data_ptr(), nq, k, rl, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                         ws.data_ptr(), ws.numel(), s)
                torch.cuda.synchronize()

            def old():
                oi, od, oc = out[1]
                _lib.check(stage1(bq.handle, tq.data_ptr(), nq, R, ci.data_ptr(), cd.data_ptr(), cc.data_ptr(),
                                  ws.data_ptr(), ws.numel(), s))
                ids = ci.cpu().numpy().view(np.uint64)  # synchronizes
                cnt = cc.cpu().numpy()
                res = f32.distance_by_ids_batch(qs, [ids[q][:cnt[q]] for q in range(nq)])
                hi.fill_(-1)
                hd.fill_(float("inf"))
                for q, (dist, ok) in enumerate(res):
                    i, x = orc.lex_topk(dist[ok], ids[q][:cnt[q]][ok], k)
                    hi[q, :len(i)] = torch.from_numpy(i.view(np.int64))
                    hd[q, :len(i)] = torch.from_numpy(x)
                oi.copy_(hi, non_blocking=True)
                od.copy_(hd, non_blocking=True)
                torch.cuda.synchronize()

            for _ in range(args.warmup):
                old()
                new()
            same = bool(torch.equal(out[0][0], out[1][0])) and bool(torch.equal(out[0][1].view(torch.int32),
                                                                                out[1][1].view(torch.int32)))
            t = {"old": [], "new": []}
            for _ in range(args.reps):
                for name, fn in (("old", old), ("new", new)):
                    t0 = time.perf_counter()
                    fn()
                    t[name].append((time.perf_counter() - t0) * 1e6)
            rec = {"rows": args.rows, "d": d, "rescore_limit": rl, "k": k, "nq": nq, "reps": args.reps, "results_equal": same}
            for name in ("old", "new"):
                a = np.array(t[name])
                rec[name + "_us"] = {"median": round(float(np.median(a)), 1), "p10": round(float(np.percentile(a, 10)), 1),
                                     "p90": round(float(np.percentile(a, 90)), 1)}
            rec["new_over_old"] = round(rec["new_us"]["median"] / rec["old_us"]["median"], 3)
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            bq.destroy()
            f32.destroy()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

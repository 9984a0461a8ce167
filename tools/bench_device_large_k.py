#!/usr/bin/env python3
"""wvg_search_device with k above 256 (the device select route, wvg_dselect.hip) against the only
route the same request had before it: the host call wvg_search with the same nq and k
(search_large_k: one query at a time, two stream syncs per query).

--configs kind:rows x dim:metric:k, comma separated; the default is 1M x 128 l2 at k = 1000 and
k = 10000, 1M x 768 cosine at k = 1000, a BQ corpus of 10M x 1536 at k = 1000 and, for context,
1M x 128 l2 at k = 256 (the fused top-k on both routes).  --batch queries (default 16) per call.
Per configuration, us per call of

  device   wvg_search_device: queries and results in HBM, the call plus one stream sync
  host     wvg_search: queries and results in host memory (it synchronizes by itself)

Both in one process, alternating run by run; `--runs` runs of `--calls` calls each, wall clock.
Every run, the median, the minimum and the maximum are reported.  Before timing, the device
results are compared with the host's bit for bit.  One JSON line per configuration on stdout,
appended to --out.  Corpora are synthetic (fill_synthetic).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEFAULT = ("f32:1000000x128:l2:1000,f32:1000000x128:l2:10000,f32:1000000x128:l2:256,f32:1000000x768:cosine:1000,"
           "bq:10000000x1536:l2:1000")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=DEFAULT)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)

    import torch

    torch.cuda.init()
    from weaviate_amd import _lib as lib_mod
    from weaviate_amd import device as dev_mod
    from oracle import wv_oracle as orc

    kinds = {"f32": lib_mod.KIND_F32, "bq": lib_mod.KIND_BQ}
    metrics = {"l2": lib_mod.METRIC_L2, "dot": lib_mod.METRIC_DOT, "cosine": lib_mod.METRIC_COSINE}
    dev = torch.device("cuda:0")
    nq = args.batch
    with dev_mod.Context(0) as ctx:
        lib = ctx.lib
        stream = torch.cuda.current_stream().cuda_stream
        corpus, shape = None, None
        for cfg in args.configs.split(","):
            kind, dims, metric, k = cfg.split(":")
            n, d = (int(v) for v in dims.split("x"))
            k = int(k)
            if shape != (kind, n, d, metric):  # consecutive configurations of one shape share the corpus
                if corpus is not None:
                    corpus.destroy()
                    torch.cuda.empty_cache()
                corpus = dev_mod.Corpus(ctx, kinds[kind], metrics[metric], d, n)
                corpus.fill_synthetic(42, n, 0)
                shape = (kind, n, d, metric)
            c = corpus
            qs = np.ascontiguousarray(orc.synth_rows(43, 0, nq, d, 0))
            dq = np.stack([orc.normalize(q) for q in qs]) if metric == "cosine" else qs
            tq = torch.from_numpy(np.ascontiguousarray(dq, dtype=np.float32)).to(dev)
            ws = torch.zeros(lib.wvg_search_workspace_size(c.handle, nq, k), dtype=torch.uint8, device=dev)
            oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
            od = torch.empty((nq, k), dtype=torch.float32, device=dev)
            oc = torch.empty(nq, dtype=torch.int32, device=dev)

            def device():
                lib_mod.check(lib.wvg_search_device(c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                                    oc.data_ptr(), ws.data_ptr(), ws.numel(), stream))
                torch.cuda.synchronize()

            def host():
                return c.search(qs, k)

            modes = [device, host]
            rec = {"label": args.label, "kind": kind, "rows": n, "dim": d, "metric": metric, "k": k,
                   "queries_per_call": nq, "calls_per_run": args.calls, "workspace_bytes": ws.numel(),
                   "us_per_call": {fn.__name__: [] for fn in modes}, "median_us": {}, "min_us": {}, "max_us": {}}
            device()
            hi, hd, hc = host()
            rec["device_equals_host"] = bool(np.array_equal(oi.cpu().numpy().view(np.uint64), hi) and
                                             np.array_equal(od.cpu().numpy().view(np.uint32), hd.view(np.uint32)) and
                                             np.array_equal(oc.cpu().numpy().astype(np.uint32), hc))
            for fn in modes:
                for _ in range(max(1, args.warmup)):
                    fn()
            for _ in range(args.runs):  # the legs alternate run by run
                for fn in modes:
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        fn()
                    rec["us_per_call"][fn.__name__].append(round((time.perf_counter() - t0) * 1e6 / args.calls, 1))
            for fn in modes:
                v = rec["us_per_call"][fn.__name__]
                rec["median_us"][fn.__name__] = float(np.median(v))
                rec["min_us"][fn.__name__] = float(np.min(v))
                rec["max_us"][fn.__name__] = float(np.max(v))
            rec["host_over_device"] = round(rec["median_us"]["host"] / rec["median_us"]["device"], 2)
            lib_mod.check(lib.wvg_search_device_check(ctx.handle, ws.data_ptr(), stream))
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del ws, tq, oi, od, oc
        if corpus is not None:
            corpus.destroy()


if __name__ == "__main__":
    main()

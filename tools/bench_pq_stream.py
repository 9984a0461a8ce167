#!/usr/bin/env python3
"""The device query stream of PQ corpora against the calls it replaces: random PQ codes
(--configs rows x m x k at dim 128 and ks = 256; default 100M x 32 at k = 10 and k = 100,
100M x 64, 10M x 32 and 1M x 32), --batch queries (default 16) per call.  Per configuration,
us per call of

  pipelined       wvg_search_device_pipelined, one call of 16 queries (the shared-row scan)
  pipelined_10pct the same through wvg_search_device_pipelined_filtered, every query with a
                  10 % allow list of its own
  device          wvg_search_device with the same 16 queries (K8e, co-scheduled, at m = 32)
  singles         16 calls of wvg_search_device with one query each

The codes are random bytes upserted in chunks (fill_synthetic does not take PQ corpora), the
codebook random centroids.  `--runs` runs of `--calls` calls each, timed with events on one
stream, the legs interleaved run by run; every run and the median are reported.  A library
without the PQ stream (the parent commit's) reports the last two only: `--lib PATH` picks the
library, which runs with its own tree's package if it lies in a built tree
(<tree>/weaviate_amd/libwvgpu.so) and with this tree's otherwise.

Before timing, the pipelined results are compared with wvg_search_device's for the same
queries, bit for bit.  One JSON line per configuration on stdout, appended to --out.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DIM, KS = 128, 256
CHUNK = 4_000_000  # rows per upsert_codes call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "weaviate_amd", "libwvgpu.so"))
    ap.add_argument("--configs", default="100000000x32x10,100000000x32x100,100000000x64x10,10000000x32x10,1000000x32x10")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-filtered", action="store_true", help="skip the 10 % allow-list leg (its lists take host time)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    lib_path = os.path.abspath(args.lib)
    tree = os.path.dirname(os.path.dirname(lib_path))
    root = tree if os.path.exists(os.path.join(tree, "weaviate_amd", "_lib.py")) else ROOT
    os.environ["WVG_LIB"] = lib_path
    sys.path.insert(0, root)

    import torch

    torch.cuda.init()
    from weaviate_amd import _lib as lib_mod
    from weaviate_amd import device as dev_mod
    from oracle import wv_oracle as orc

    dev = torch.device("cuda:0")
    nq = args.batch
    configs = [tuple(int(v) for v in c.split("x")) for c in args.configs.split(",")]
    with dev_mod.Context(0) as ctx:
        lib = ctx.lib
        stream = torch.cuda.current_stream().cuda_stream
        corpus, shape = None, None
        for n, m, k in configs:
            if shape != (n, m):  # consecutive configurations of one shape share the corpus
                if corpus is not None:
                    corpus.destroy()
                    torch.cuda.empty_cache()
                corpus = dev_mod.Corpus(ctx, lib_mod.KIND_PQ, lib_mod.METRIC_L2, DIM, n)
                corpus.set_codebook(orc.synth_rows(41, 0, m * KS, DIM // m, 0).reshape(m, KS, DIM // m))
                rng = np.random.default_rng(42)
                for lo in range(0, n, CHUNK):
                    rows = min(CHUNK, n - lo)
                    corpus.upsert_codes(np.arange(lo, lo + rows, dtype=np.uint64),
                                        rng.integers(0, KS, (rows, m), dtype=np.uint8))
                shape = (n, m)
            c = corpus
            tq = torch.from_numpy(np.ascontiguousarray(orc.synth_rows(43, 0, nq, DIM, 0))).to(dev)
            ws_bytes = max(lib.wvg_search_workspace_size(c.handle, j, k) for j in (1, nq))  # `singles` runs on it too
            ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
            oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
            od = torch.empty((nq, k), dtype=torch.float32, device=dev)
            oc = torch.empty(nq, dtype=torch.int32, device=dev)
            sp = lib_mod.StreamPlan()
            has_stream = lib.wvg_search_device_pipelined_plan(c.handle, nq, k, sp) == lib_mod.WVG_OK
            filtered = has_stream and not args.no_filtered
            stride = (n + 63) // 64
            allow = torch.from_numpy(_ten_percent_words(np.random.default_rng(7), nq, stride if filtered else 0)).to(dev)
            out = (oi.data_ptr(), od.data_ptr(), oc.data_ptr(), ws.data_ptr(), ws.numel(), stream)

            def device():
                lib_mod.check(lib.wvg_search_device(c.handle, tq.data_ptr(), nq, k, *out))

            def singles():
                for i in range(nq):
                    lib_mod.check(lib.wvg_search_device(c.handle, tq[i].data_ptr(), 1, k, oi[i].data_ptr(), od[i].data_ptr(),
                                                        oc[i:].data_ptr(), ws.data_ptr(), ws.numel(), stream))

            def pipelined():
                lib_mod.check(lib.wvg_search_device_pipelined(c.handle, tq.data_ptr(), nq, k, *out))

            def pipelined_10pct():
                lib_mod.check(lib.wvg_search_device_pipelined_filtered(c.handle, tq.data_ptr(), nq, k, allow.data_ptr(),
                                                                       stride, 0, *out))

            modes = [device, singles] + ([pipelined] if has_stream else []) + ([pipelined_10pct] if filtered else [])
            rec = {"lib": os.path.relpath(lib_path, ROOT), "label": args.label, "rows": n, "dim": DIM, "m": m, "ks": KS, "k": k,
                   "queries_per_call": nq, "calls_per_run": args.calls, "pq_stream": has_stream,
                   "us_per_call": {fn.__name__: [] for fn in modes}, "median_us": {}}
            if has_stream:
                rec["plan"] = c.search_device_plan(nq, k)
                device()
                torch.cuda.synchronize()
                want = (oi.cpu().numpy().copy(), od.cpu().numpy().view(np.uint32).copy(), oc.cpu().numpy().copy())
                oi.zero_(), od.zero_(), oc.zero_()
                pipelined()
                torch.cuda.synchronize()
                rec["pipelined_equals_device"] = bool(np.array_equal(oi.cpu().numpy(), want[0]) and
                                                      np.array_equal(od.cpu().numpy().view(np.uint32), want[1]) and
                                                      np.array_equal(oc.cpu().numpy(), want[2]))
            for fn in modes:
                for _ in range(max(1, args.warmup)):
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.runs):  # the legs interleaved run by run
                for fn in modes:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.calls):
                        fn()
                    e1.record()
                    e1.synchronize()
                    rec["us_per_call"][fn.__name__].append(round(e0.elapsed_time(e1) * 1e3 / args.calls, 1))
            for fn in modes:
                rec["median_us"][fn.__name__] = float(np.median(rec["us_per_call"][fn.__name__]))
            lib_mod.check(lib.wvg_search_device_check(ctx.handle, ws.data_ptr(), stream))
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del ws, tq, allow
        if corpus is not None:
            corpus.destroy()


def _ten_percent_words(rng, nq, stride):
    """[nq][stride] allow words (as int64), every bit set with probability 0.10, one query at a time."""
    out = np.empty((nq, stride), np.int64)
    for q in range(nq):
        out[q] = np.packbits(rng.random(stride * 64, dtype=np.float32) < 0.10, bitorder="little").view(np.int64)
    return out


if __name__ == "__main__":
    main()

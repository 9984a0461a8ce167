#!/usr/bin/env python3
"""wvg_search_device_pipelined across fp32 dimensions: 1M rows, L2, k = 10, 16
single-query searches per launch, d in --dims (default 256, 384, 512, 1024,
1536).  Reports us per launch: `--runs` runs of `--launches` launches each per
dimension, timed with events on one stream, and their median.

--lib PATH picks the library.  A library that lies in a built tree
(<tree>/weaviate_amd/libwvgpu.so, e.g. a checkout of the parent commit in a
directory of its own) runs with that tree's package, so that the binding
matches the library; any other path (tools/libwvgpu_tools.so) runs with this
tree's package.  --qshare N sets tuning key 34 before the first search (tools
library only; 3 = the runtime-dimension form at d = 128 and 768 too).

Before timing, query 0's result of the launch is compared with a
wvg_search_device call of that query alone.  One JSON line on stdout, appended
to --out when given.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "weaviate_amd", "libwvgpu.so"))
    ap.add_argument("--dims", default="256,384,512,1024,1536")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--qshare", type=int, default=None, help="tuning key 34 (tools library)")
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
    n, nq, k = args.rows, args.batch, args.k
    rec = {"lib": os.path.relpath(lib_path, ROOT), "label": args.label, "rows": n, "k": k, "queries_per_launch": nq,
           "launches_per_run": args.launches, "qshare": args.qshare, "us_per_launch": {}, "median_us": {},
           "query0_equals_single_search": {}, "plan": {}}
    with dev_mod.Context(0) as ctx:
        lib = ctx.lib
        if args.qshare is not None:
            lib.wvgx_set_tuning.restype = ctypes.c_int
            lib.wvgx_set_tuning.argtypes = [ctypes.c_int, ctypes.c_int]
            lib.wvgx_set_tuning(34, args.qshare)
        stream = torch.cuda.current_stream().cuda_stream
        for d in [int(x) for x in args.dims.split(",")]:
            c = dev_mod.Corpus(ctx, lib_mod.KIND_F32, lib_mod.METRIC_L2, d, n)
            c.fill_synthetic(42, n, 0)
            tq = torch.from_numpy(np.ascontiguousarray(orc.synth_rows(43, 0, nq, d, 0))).to(dev)
            ws = torch.zeros(lib.wvg_search_workspace_size(c.handle, nq, k), dtype=torch.uint8, device=dev)
            oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
            od = torch.empty((nq, k), dtype=torch.float32, device=dev)
            oc = torch.empty(nq, dtype=torch.int32, device=dev)

            def launch(fn=lib.wvg_search_device_pipelined, m=nq):
                lib_mod.check(fn(c.handle, tq.data_ptr(), m, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                 ws.data_ptr(), ws.numel(), stream))

            launch(lib.wvg_search_device, 1)
            torch.cuda.synchronize()
            one = (oi[0].cpu().numpy().copy(), od[0].cpu().numpy().view(np.uint32).copy())
            for _ in range(max(1, args.warmup)):
                launch()
            torch.cuda.synchronize()
            rec["query0_equals_single_search"][str(d)] = bool(
                np.array_equal(oi[0].cpu().numpy(), one[0]) and np.array_equal(od[0].cpu().numpy().view(np.uint32), one[1]))
            if hasattr(c, "search_device_plan"):
                rec["plan"][str(d)] = c.search_device_plan(nq, k)
            us = []
            for _ in range(args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    launch()
                e1.record()
                e1.synchronize()
                us.append(round(e0.elapsed_time(e1) * 1e3 / args.launches, 2))
            lib_mod.check(lib.wvg_search_device_check(ctx.handle, ws.data_ptr(), stream))
            rec["us_per_launch"][str(d)] = us
            rec["median_us"][str(d)] = float(np.median(us))
            c.destroy()
            del ws, tq
            torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

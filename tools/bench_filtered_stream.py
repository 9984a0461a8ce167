#!/usr/bin/env python3
"""Filtered shared-row query stream at the bench's shape: 1M x 128 L2, k = 10,
16 single-query searches per wvg_search_device_pipelined_filtered launch.

  launch leg: us per launch, `--runs` plain runs of `--launches` launches each,
    timed with events on one stream, the variants interleaved inside a run:
      none    wvg_search_device_pipelined (no filter)
      ones    all-ones lists
      p10     a random 10 % list per query
      p1      a random 1 % list per query
      ranges  16 disjoint contiguous ranges of 1/16 of the corpus (the tile skip)
    Before timing, every filtered variant's results are compared with host
    wvg_search calls carrying the same lists.
  host leg: the same 16 filtered queries the only way a build without the
    filtered entry point serves them: one wvg_search per query from 16 native
    caller threads (tools/libhostcalls.so), 10 % and 1 % lists.

--root DIR runs a leg against another built tree (its weaviate_amd package and
library), e.g. the parent commit for the host leg and the unfiltered launch.
One JSON line per leg on stdout, appended to --out when given.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def words_of(masks):
    """[nq][n] bool -> [nq][ceil(n / 64)] uint64, bit b of word w = row 64 w + b."""
    nq, n = masks.shape
    pad = np.zeros((nq, (n + 63) // 64 * 64), np.uint8)
    pad[:, :n] = masks
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint64)


def variants(n, nq, seed=47):
    rng = np.random.default_rng(seed)
    ranges = np.zeros((nq, n), bool)
    for q in range(nq):
        ranges[q, q * n // nq:(q + 1) * n // nq] = True
    return {"ones": np.ones((nq, n), bool), "p10": rng.random((nq, n)) < 0.10, "p1": rng.random((nq, n)) < 0.01,
            "ranges": ranges}


def launch_leg(args, lib_mod, dev_mod):
    import torch

    n, d, k, nq = args.rows, 128, 10, 16
    dev = torch.device("cuda:0")
    with dev_mod.Context(0) as ctx:
        lib = ctx.lib
        c = dev_mod.Corpus(ctx, lib_mod.KIND_F32, lib_mod.METRIC_L2, d, n)
        c.fill_synthetic(42, n, 0)
        sys.path.insert(0, args.root)
        from oracle import wv_oracle as orc

        qs = np.ascontiguousarray(orc.synth_rows(43, 0, nq, d, 0))
        tq = torch.from_numpy(qs).to(dev)
        ws = torch.zeros(lib.wvg_search_workspace_size(c.handle, nq, k), dtype=torch.uint8, device=dev)
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oc = torch.empty(nq, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        filtered = hasattr(lib, "wvg_search_device_pipelined_filtered") and not args.unfiltered_only
        var = variants(n, nq) if filtered else {}
        if args.only:
            var = {name: m for name, m in var.items() if name in args.only.split(",")}
        host_words = {name: words_of(m) for name, m in var.items()}
        dev_words = {name: torch.from_numpy(w.view(np.int64)).to(dev) for name, w in host_words.items()}
        stride = (n + 63) // 64

        def launch(name):
            if name == "none":
                rc = lib.wvg_search_device_pipelined(c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                                     oc.data_ptr(), ws.data_ptr(), ws.numel(), stream)
            else:
                rc = lib.wvg_search_device_pipelined_filtered(c.handle, tq.data_ptr(), nq, k, dev_words[name].data_ptr(),
                                                              stride, 0, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                                              ws.data_ptr(), ws.numel(), stream)
            lib_mod.check(rc)

        names = ["none"] + list(var)
        checked = {}
        for name in var:  # the filtered results against host wvg_search calls with the same lists
            launch(name)
            torch.cuda.synchronize()
            gi, gd = oi.cpu().numpy().view(np.uint64), od.cpu().numpy()
            ok = True
            for q in range(nq):
                hi, hd, _ = c.search(qs[[q]], k, allow=host_words[name][q])
                ok = ok and np.array_equal(gi[q], hi[0]) and np.array_equal(gd[q].view(np.uint32), hd[0].view(np.uint32))
            checked[name] = bool(ok)
        for name in names:
            for _ in range(args.warmup):
                launch(name)
        torch.cuda.synchronize()
        us = {name: [] for name in names}
        for _ in range(args.runs):
            for name in names:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    launch(name)
                e1.record()
                e1.synchronize()
                us[name].append(round(e0.elapsed_time(e1) * 1e3 / args.launches, 2))
        lib_mod.check(lib.wvg_search_device_check(ctx.handle, ws.data_ptr(), stream))
        c.destroy()
    return {"leg": "launch", "root": args.root, "rows": n, "dim": d, "k": k, "queries_per_launch": nq,
            "launches_per_run": args.launches, "us_per_launch": us,
            "median_us": {name: float(np.median(v)) for name, v in us.items()}, "equal_host_wvg_search": checked}


def host_leg(args, lib_mod, dev_mod):
    import ctypes

    n, d, k, nq, T = args.rows, 128, 10, 16, 16
    path = os.path.join(args.root, "tools", "libhostcalls.so")
    hc = ctypes.CDLL(path)
    hc.wvgb_call_loop.restype = ctypes.c_int
    hc.wvgb_call_loop.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32] * 3 + [
        ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
        ctypes.c_double, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    sys.path.insert(0, args.root)
    from oracle import wv_oracle as orc

    out = {"leg": "host", "root": args.root, "rows": n, "dim": d, "k": k, "callers": T, "qps": {}, "us_per_16_queries": {}}
    with dev_mod.Context(0) as ctx:
        lib = ctx.lib
        c = dev_mod.Corpus(ctx, lib_mod.KIND_F32, lib_mod.METRIC_L2, d, n)
        c.fill_synthetic(42, n, 0)
        qs = np.ascontiguousarray(orc.synth_rows(43, 0, nq, d, 0))
        var = variants(n, nq)
        fn = ctypes.cast(lib.wvg_search, ctypes.c_void_p).value
        for name in ("p10", "p1"):
            allows = [np.ascontiguousarray(w) for w in words_of(var[name])]
            arr = (ctypes.c_void_p * nq)(*[x.ctypes.data for x in allows])
            nwords = np.array([len(x) for x in allows], np.uint64)
            out["qps"][name], out["us_per_16_queries"][name] = [], []
            for _ in range(args.runs):
                cap = 400_000
                lat = np.zeros(T * cap, np.float64)
                cnt = np.zeros(T, np.uint64)
                el = ctypes.c_double()
                rc = hc.wvgb_call_loop(fn, c.handle, qs.ctypes.data, nq, d, k, None, 0, ctypes.cast(arr, ctypes.c_void_p),
                                       nwords.ctypes.data, nq, T, args.seconds, lat.ctypes.data, cap, cnt.ctypes.data,
                                       ctypes.byref(el))
                if rc != 0:
                    raise RuntimeError(f"native caller loop failed: {rc}")
                qps = float(cnt.sum()) / el.value
                out["qps"][name].append(round(qps, 1))
                out["us_per_16_queries"][name].append(round(16e6 / qps, 2))
        c.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["launch", "host"], default="launch")
    ap.add_argument("--root", default=os.path.dirname(HERE), help="built tree whose package and library run the leg")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0, help="host leg: wall time of a run")
    ap.add_argument("--unfiltered-only", action="store_true", help="launch leg: time only the launch with no filter")
    ap.add_argument("--only", default="", help="launch leg: comma list of the filtered variants to run (default: all)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.root = os.path.abspath(args.root)
    sys.path.insert(0, args.root)
    from weaviate_amd import _lib as lib_mod
    from weaviate_amd import device as dev_mod

    rec = launch_leg(args, lib_mod, dev_mod) if args.leg == "launch" else host_leg(args, lib_mod, dev_mod)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

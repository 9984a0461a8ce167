#!/usr/bin/env python3
"""What K8's global-LUT fallback costs: time per query of a lone ADC scan at
Weaviate's own segment counts, with the LUT in LDS (m = 128, 144) and in
global memory (m = 160, 256), ks = 256, top-10, on one MI355X in one run.

The shapes alternate inside every round, so box and clock drift hit them
alike; the scan time is the kernel's own (wvg_profile_start / _stop: events
bound to the scan dispatch), the wall time includes the LUT kernel, the merge
and the host call.  One JSON line per (round, shape), then one summary line
per shape with the medians.  Product library only.

Usage: python tools/pq_large_m_probe.py [--rows 1000000] [--rounds 5] [--calls 32] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(128, 6), (256, 6), (144, 2), (160, 2)]  # (m, ds)
KS, K = 256, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    torch.cuda.init()
    from weaviate_amd._lib import KIND_PQ, METRIC_L2
    from weaviate_amd.device import Context, Corpus

    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    n = args.rows
    rng = np.random.default_rng(7)
    with Context(0) as ctx:
        lib = ctx.lib
        corpora = []
        for m, ds in SHAPES:
            d = m * ds
            c = Corpus(ctx, KIND_PQ, METRIC_L2, d, n)
            c.set_codebook(rng.uniform(-1, 1, (m, KS, ds)).astype(np.float32))
            ids = np.arange(n, dtype=np.uint64)
            for lo in range(0, n, 250_000):
                hi = min(n, lo + 250_000)
                c.upsert_codes(ids[lo:hi], rng.integers(0, KS, (hi - lo, m), dtype=np.uint8))
            qs = rng.uniform(-1, 1, (args.calls, d)).astype(np.float32)
            for q in qs:  # warm-up: code objects, clocks
                c.search(q, K)
            corpora.append((m, ds, c, qs))
        res = {m: [] for m, _ in SHAPES}
        for rnd in range(args.rounds):
            for m, ds, c, qs in corpora:
                c.search(qs[0], K)
                lib.wvg_profile_start(ctx.handle)
                t0 = time.perf_counter()
                for q in qs:
                    c.search(q, K)
                wall = (time.perf_counter() - t0) / len(qs)
                ms, nl = ctypes.c_double(), ctypes.c_uint64()
                lib.wvg_profile_stop(ctx.handle, ctypes.byref(ms), ctypes.byref(nl))
                scan_us = ms.value * 1e3 / max(1, nl.value)
                res[m].append((scan_us, wall * 1e6))
                emit({"round": rnd, "m": m, "ks": KS, "rows": n, "lut_KiB": m * KS * 4 // 1024,
                      "lut": "LDS" if m * KS * 4 + 8192 <= 160 * 1024 else "global", "scan_us": round(scan_us, 2),
                      "call_us": round(wall * 1e6, 2), "scan_launches": nl.value})
        for m, ds in SHAPES:
            scan = np.array([x[0] for x in res[m]])
            call = np.array([x[1] for x in res[m]])
            emit({"summary": True, "m": m, "ks": KS, "rows": n, "k": K,
                  "lut": "LDS" if m * KS * 4 + 8192 <= 160 * 1024 else "global",
                  "scan_us_median": round(float(np.median(scan)), 2), "scan_us_min": round(float(scan.min()), 2),
                  "scan_us_max": round(float(scan.max()), 2), "call_us_median": round(float(np.median(call)), 2),
                  "code_GBps": round(n * m / (float(np.median(scan)) * 1e-6) / 1e9, 1)})
        for _, _, c, _ in corpora:
            c.destroy()
    if out:
        out.close()


if __name__ == "__main__":
    main()

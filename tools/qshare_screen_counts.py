#!/usr/bin/env python3
"""The admission counts of the screened shared-row scan (scan_f32_qshare_screen_kernel,
wvg_qshare.hip) on the bench's shape: runs wvg_search_device_pipelined on a
synthetic corpus with the tools build and reads its per-launch counters: the
(query, tile) pairs with at least one admitted row and all (query, tile) pairs
(wvgx_qshare_screen_counts), the admitted (query, row) pairs and the rounds of
the exact chain (wvgx_qshare_row_counts).  Tooling only.

    make -C weaviate_amd/csrc tools
    python tools/qshare_screen_counts.py [--rows 1000000] [--batch 16] [--k 10] [--sample 32]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("WVG_LIB", os.path.join(ROOT, "tools", "libwvgpu_tools.so"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--sample", type=int, default=-1, help="tuning key 37: tiles of the seed sample")
    ap.add_argument("--launches", type=int, default=8)
    a = ap.parse_args()

    import torch

    torch.cuda.init()
    from weaviate_amd._lib import KIND_F32, METRIC_L2, check
    from weaviate_amd.device import Context, Corpus

    dev = torch.device("cuda:0")
    ctx = Context(0)
    lib = ctx.lib
    lib.wvgx_set_tuning.restype = ctypes.c_int
    lib.wvgx_set_tuning.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.wvgx_qshare_screen_counts.restype = ctypes.c_int
    lib.wvgx_qshare_screen_counts.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    lib.wvgx_qshare_row_counts.restype = ctypes.c_int
    lib.wvgx_qshare_row_counts.argtypes = lib.wvgx_qshare_screen_counts.argtypes
    if a.sample >= 0:
        lib.wvgx_set_tuning(37, a.sample)
    n, d, B, k = a.rows, 128, a.batch, a.k
    c = Corpus(ctx, KIND_F32, METRIC_L2, d, (n + 63) // 64 * 64)
    c.fill_synthetic(42, n, 0)
    qs = torch.from_numpy(np.random.default_rng(43).uniform(-1, 1, (a.launches * B, d)).astype(np.float32)).to(dev)
    wsb = lib.wvg_search_workspace_size(c.handle, B, k)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    oi = torch.empty((B, k), dtype=torch.int64, device=dev)
    od = torch.empty((B, k), dtype=torch.float32, device=dev)
    oc = torch.empty(B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    folded = pairs = admitted = rounds = 0
    out2 = (ctypes.c_uint64 * 2)()
    for s in range(a.launches):
        check(lib.wvg_search_device_pipelined(c.handle, qs[s * B].data_ptr(), B, k, oi.data_ptr(), od.data_ptr(),
                                              oc.data_ptr(), ws.data_ptr(), wsb, st))
        check(lib.wvgx_qshare_screen_counts(c.handle, B, k, ws.data_ptr(), st, out2))
        folded += out2[0]
        pairs += out2[1]
        check(lib.wvgx_qshare_row_counts(c.handle, B, k, ws.data_ptr(), st, out2))
        admitted += out2[0]
        rounds += out2[1]
    check(lib.wvg_search_device_check(ctx.handle, ws.data_ptr(), st))
    print(json.dumps({"rows": n, "batch": B, "k": k, "sample_tiles": a.sample, "launches": a.launches,
                      "pairs_per_launch": pairs // max(1, a.launches), "folded_per_launch": folded // max(1, a.launches),
                      "fold_fraction": round(folded / max(1, pairs), 4),
                      "admitted_rows_per_launch": admitted // max(1, a.launches),
                      "rounds_per_launch": rounds // max(1, a.launches),
                      # per live tile, all passes together: `pairs` counts a tile once per query
                      "admitted_rows_per_tile": round(admitted * B / max(1, pairs), 3),
                      "rounds_per_tile": round(rounds * B / max(1, pairs), 3)}), flush=True)
    c.destroy()
    ctx.close()


if __name__ == "__main__":
    main()

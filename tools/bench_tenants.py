"""Multi-tenant search: many small corpora, every query to one tenant of its own
(adapters/repos/db/index.go:1516-1539).  Three ways to answer the same stream of
queries, each to a distinct random tenant, on one build and in one process:

  a  one thread issuing wvg_search calls one after another
  b  16 threads issuing wvg_search calls concurrently
  c  one wvg_search_group call per nq queries, nq in --nqs

With --compression bq every tenant is a BQ corpus and an F32 corpus and the legs
run flat.searchByVectorBQ (V/flat/index.go:347-389): a and b call
wvg_search_bq_rescore, c calls wvg_search_group_bq_rescore, with --rescore-limit
as the rescore window.  The line then also holds, for a few queries, the rows the
grouped filter keeps and the rows the heap inserts (recomputed on the host from
the tenant's codes with weaviate_amd.flat.group_bq_kept_rows).

Per leg: per-call microseconds (p50 / p99), queries per second and, for c, the
algorithmic time of a call (nq x rows x dim x 4 bytes at 8 TB/s).  --allow-frac
gives every query an allow list of that fraction of its tenant's ids.  The legs
are run --repeats times interleaved (a, b, c.., a, b, c..) and the medians over
the repeats are reported; every leg's last results are compared with leg a's.

The product library, no tuning keys.  Examples:
  python tools/bench_tenants.py                                  # 1024 x 10k x 128, L2, k = 10
  python tools/bench_tenants.py --allow-frac 0.1
  python tools/bench_tenants.py --tenants 64 --rows 100000 --dim 768 --metric cosine
  python tools/bench_tenants.py --compression bq --rescore-limit 200 --dim 1536
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(p / 100.0 * len(xs)))]


def kept_rows(codes, target, qs, allows, n, R, nqueries):
    """For the first queries of the stream: [rows the grouped filter keeps (256-row chunks), rows the
    heap of R inserts], from the tenant's codes read back from the device."""
    import heapq

    from weaviate_amd.flat import group_bq_kept_rows

    out = []
    for i in range(min(nqueries, len(qs))):
        rows, ok = codes[target[i]].get_batch(np.arange(n, dtype=np.uint64))
        bits = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :qs.shape[1]]
        ham = (bits != (qs[i] < 0)).sum(axis=1).astype(np.float32)  # sign bits: normalization keeps them
        live = ok.copy()
        if allows:
            live &= np.unpackbits(allows[i].view(np.uint8), bitorder="little")[:n].astype(bool)
        kept = int(group_bq_kept_rows(ham, live, R).sum())
        top, inserted = [], 0  # insertToHeap: below R rows, or strictly below the R-th smallest so far
        for x in ham[live]:
            if len(top) < R:
                heapq.heappush(top, -x)
                inserted += 1
            elif -top[0] > x:
                heapq.heapreplace(top, -x)
                inserted += 1
        out.append([kept, inserted])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tenants", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=10_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--metric", default="l2-squared")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--queries", type=int, default=1024, help="queries of the stream (a multiple of the largest nq)")
    ap.add_argument("--nqs", default="1,4,16,64,256")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--allow-frac", type=float, default=0.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--compression", default="none", choices=["none", "bq"])
    ap.add_argument("--rescore-limit", type=int, default=200, help="with --compression bq: the rescore window")
    ap.add_argument("--kept-queries", type=int, default=4, help="with --compression bq: queries whose kept rows are counted")
    ap.add_argument("--out", default=None, help="also write the result line to this file")
    a = ap.parse_args()
    import torch

    torch.cuda.init()
    from weaviate_amd._lib import KIND_BQ, KIND_F32, METRIC_BY_NAME, check, fptr, u32ptr, u64ptr
    from weaviate_amd.device import Context, Corpus, allow_bitmap

    metric = METRIC_BY_NAME[a.metric]
    nqs = [int(x) for x in a.nqs.split(",")]
    legs = a.legs.split(",")
    Q, k, d, n = a.queries, a.k, a.dim, a.rows
    assert all(Q % x == 0 for x in nqs), "--queries must be a multiple of every nq"
    ctx = Context(0)
    lib = ctx.lib
    bq, rl = a.compression == "bq", a.rescore_limit
    tenants, codes = [], []  # the F32 corpora; with --compression bq the BQ corpora of the same rows
    for t in range(a.tenants):
        c = Corpus(ctx, KIND_F32, metric, d, n)
        c.fill_synthetic(1000 + t, n, 0)
        tenants.append(c)
        if bq:
            b = Corpus(ctx, KIND_BQ, metric, d, n)
            b.fill_synthetic(1000 + t, n, 0)
            codes.append(b)
    ctx.synchronize()
    rng = np.random.default_rng(7)
    # every query to a tenant of its own while the tenants last
    target = np.concatenate([rng.permutation(a.tenants) for _ in range(-(-Q // a.tenants))])[:Q]
    qs = rng.uniform(-1, 1, (Q, d)).astype(np.float32)
    allows = None
    if a.allow_frac > 0:
        allows = [allow_bitmap(np.sort(rng.choice(n, max(1, int(n * a.allow_frac)), replace=False)), n) for _ in range(Q)]

    ids = np.empty((Q, k), np.uint64)
    dists = np.empty((Q, k), np.float32)
    counts = np.empty(Q, np.uint32)

    single = lib.wvg_search_bq_rescore if bq else lib.wvg_search
    group = lib.wvg_search_group_bq_rescore if bq else lib.wvg_search_group

    def single_args(i, oi, od, oc):
        aw = allows[i] if allows else None
        head = (codes[target[i]].handle, tenants[target[i]].handle, fptr(qs[i:i + 1]), 1, k, rl) if bq else \
               (tenants[target[i]].handle, fptr(qs[i:i + 1]), 1, k)
        return head + (u64ptr(aw) if aw is not None else None, len(aw) if aw is not None else 0,
                       u64ptr(oi[i:i + 1]), fptr(od[i:i + 1]), u32ptr(oc[i:i + 1]))

    def leg_a():
        args = [single_args(i, ids, dists, counts) for i in range(Q)]
        for i in range(min(Q, 64)):
            check(single(*args[i]))
        per = []
        t0 = time.perf_counter()
        for i in range(Q):
            t1 = time.perf_counter()
            check(single(*args[i]))
            per.append(time.perf_counter() - t1)
        wall = time.perf_counter() - t0
        return per, wall, (ids.copy(), dists.copy(), counts.copy())

    def leg_b():
        oi, od, oc = np.empty_like(ids), np.empty_like(dists), np.empty_like(counts)
        args = [single_args(i, oi, od, oc) for i in range(Q)]
        per = [0.0] * Q
        errs = []
        start = threading.Barrier(a.threads + 1)

        def work(w):
            try:
                for i in range(w, min(Q, 4 * a.threads), a.threads):
                    check(single(*args[i]))
                start.wait()
                for i in range(w, Q, a.threads):
                    t1 = time.perf_counter()
                    check(single(*args[i]))
                    per[i] = time.perf_counter() - t1
            except Exception as e:  # noqa: BLE001
                errs.append(e)
                start.abort()

        ths = [threading.Thread(target=work, args=(w,)) for w in range(a.threads)]
        for t in ths:
            t.start()
        start.wait()
        t0 = time.perf_counter()
        for t in ths:
            t.join()
        wall = time.perf_counter() - t0
        if errs:
            raise errs[0]
        return per, wall, (oi, od, oc)

    def leg_c(nq):
        oi, od, oc = np.empty_like(ids), np.empty_like(dists), np.empty_like(counts)
        calls = []
        for c0 in range(0, Q, nq):
            hs = (ctypes.c_void_p * nq)(*[tenants[target[i]].handle for i in range(c0, c0 + nq)])
            ap_, aw_ = None, None
            if allows:
                ap_ = (ctypes.c_void_p * nq)(*[allows[i].ctypes.data for i in range(c0, c0 + nq)])
                aw_ = np.array([len(allows[i]) for i in range(c0, c0 + nq)], np.uint64)
            head = (hs, fptr(qs[c0:c0 + nq]), nq, k)
            if bq:
                hb = (ctypes.c_void_p * nq)(*[codes[target[i]].handle for i in range(c0, c0 + nq)])
                head = (hb, hs, fptr(qs[c0:c0 + nq]), nq, k, rl)
            calls.append((head + (ap_, u64ptr(aw_) if aw_ is not None else None, u64ptr(oi[c0:c0 + nq]),
                                  fptr(od[c0:c0 + nq]), u32ptr(oc[c0:c0 + nq])), aw_))
        for cl in calls[:min(len(calls), 8)]:
            check(group(*cl[0]))
        per = []
        t0 = time.perf_counter()
        for cl in calls:
            t1 = time.perf_counter()
            check(group(*cl[0]))
            per.append(time.perf_counter() - t1)
        wall = time.perf_counter() - t0
        return per, wall, (oi, od, oc)

    runs = {}  # leg -> [(p50 us, p99 us, qps)]
    base = None
    checked = {}

    def record(name, per, wall, res):
        nonlocal base
        runs.setdefault(name, []).append((pct(per, 50) * 1e6, pct(per, 99) * 1e6, Q / wall))
        if name == "a":
            base = res
        elif base is not None:
            checked[name] = bool(np.array_equal(res[0], base[0]) and np.array_equal(res[2], base[2]) and
                                 np.array_equal(res[1].view(np.uint32), base[1].view(np.uint32)))

    for _ in range(a.repeats):
        if "a" in legs:
            record("a", *leg_a())
        if "b" in legs:
            record("b", *leg_b())
        if "c" in legs:
            for nq in nqs:
                record(f"c{nq}", *leg_c(nq))

    out = {"tenants": a.tenants, "rows": n, "dim": d, "metric": a.metric, "k": k, "queries": Q,
           "allow_frac": a.allow_frac, "threads": a.threads, "repeats": a.repeats, "legs": {}}
    if bq:
        out["compression"], out["rescore_limit"] = "bq", rl
        out["kept_rows"] = kept_rows(codes, target, qs, allows, n, max(rl, k), a.kept_queries)
    for name, rs in runs.items():
        e = {"call_us_p50": round(statistics.median(r[0] for r in rs), 2),
             "call_us_p99": round(statistics.median(r[1] for r in rs), 2),
             "qps": round(statistics.median(r[2] for r in rs), 1),
             "qps_runs": [round(r[2], 1) for r in rs]}
        if name.startswith("c"):
            nq = int(name[1:])
            e["nq"] = nq
            row_bytes = (d + 127) // 128 * 16 if bq else d * 4  # the scanned rows: codes in 16-byte chunks, or floats
            e["algorithmic_us_at_8TBs"] = round(nq * n * row_bytes / 8e12 * 1e6, 2)
        if name in checked:
            e["equals_leg_a"] = checked[name]
        out["legs"][name] = e
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for c in tenants + codes:
        c.destroy()
    ctx.close()
    if not all(checked.values()):
        raise SystemExit(f"results differ from leg a: {checked}")


if __name__ == "__main__":
    main()

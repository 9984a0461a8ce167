"""wvg_search_device with k above the fused register top-k (k > 256): the device select route
(weaviate_amd/csrc/wvg_dselect.hip) -- keys for groups of 4 queries, batched radix select,
exact-count compaction, sort, emit, all on the caller's stream.

The reference is Corpus.search(qs, k), the host path (search_large_k: S1-S4 of wvg_select.hip, one
query at a time), on the same corpus; tests/test_gpu_select.py pins that path to the oracle.  The
comparison is on ids, distance bits, counts and padding.  For cosine the device call takes the
normalized queries and the host call the raw ones (it normalizes them itself).

The corpora here stay below 8,000 rows: every CU-capped grid makes one trip and dsel_scan_kernel gives
each thread one range.  tests/test_gpu_select_wrap.py holds the large sizes (a wave's second and third
tile, the compaction's second trip, two and three ranges per scan thread)."""
import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import (KIND_BQ, KIND_F32, KIND_PQ, METRIC_COSINE, METRIC_DOT, METRIC_HAMMING, METRIC_L2,
                               METRIC_MANHATTAN, ORDER_AVX256, ORDER_AVX512)
from weaviate_amd.device import Corpus

pytestmark = pytest.mark.gpu

ORC_METRIC = {METRIC_L2: 0, METRIC_DOT: 1, METRIC_COSINE: 2}
NONE = np.uint64(2**64 - 1)
RANGE = 2048  # DSEL_RANGE: slots per compaction workgroup


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def dev_queries(orc, metric, qs):
    qs = np.ascontiguousarray(qs, dtype=np.float32)
    return np.stack([orc.normalize(q) for q in qs]) if metric == METRIC_COSINE else qs


def dev_search(c, dq, k, with_counts=True, ws=None, entry="wvg_search_device"):
    """One device call on the current stream: (ids [nq][k], dists, counts or None)."""
    import torch

    lib = c.lib
    dev = torch.device("cuda:0")
    dq = np.ascontiguousarray(dq, dtype=np.float32)
    nq = len(dq)
    if ws is None:
        ws = torch.zeros(lib.wvg_search_workspace_size(c.handle, nq, k), dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(dq).to(dev)
    oi = torch.full((nq, k), 7, dtype=torch.int64, device=dev)
    od = torch.full((nq, k), -7.0, dtype=torch.float32, device=dev)
    oc = torch.full((nq,), 77, dtype=torch.int32, device=dev)
    _lib.check(getattr(lib, entry)(c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                   oc.data_ptr() if with_counts else None, ws.data_ptr(), ws.numel(),
                                   torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return (oi.cpu().numpy().view(np.uint64), od.cpu().numpy(),
            oc.cpu().numpy().astype(np.uint32) if with_counts else None)


def same(got, want, what=""):
    gi, gd, gc = got
    hi, hd, hc = want
    assert np.array_equal(gc, hc), (what, gc, hc)
    assert np.array_equal(gi, hi), what
    assert np.array_equal(bits(gd), bits(hd)), what
    for qi, n in enumerate(hc):  # padding
        assert np.all(gi[qi, n:] == NONE) and np.all(np.isposinf(gd[qi, n:])), what


def same_as_host(c, orc, qs, k, what=""):
    """The device call against the host path; returns the host result."""
    want = c.search(qs, k)
    same(dev_search(c, dev_queries(orc, c.metric, qs), k), want, (what, k))
    return want


def kth_ties(all_d, k):
    """True where the k-th and (k+1)-th smallest of the distances are equal."""
    s = np.sort(all_d)
    return k < len(s) and s[k - 1] == s[k]


# ---- 1. F32 L2 / dot / cosine ----------------------------------------------------------------------
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT, METRIC_COSINE])
def test_f32_shared_rows(ctx, orc, metric):
    """n = 7005 (110 tiles, 4 compaction workgroups), d = 96, id_base 640, deletes, nq = 5: one full
    group of 4 and a remainder of 1; k up to and past the row count."""
    n, d, nq, base = 7005, 96, 5, 640
    rows = orc.synth_rows(2201, 0, n, d, 0)
    qs = orc.synth_rows(2202, 0, nq, d, 0)
    ids_all = np.arange(base, base + n, dtype=np.uint64)
    c = Corpus(ctx, KIND_F32, metric, d, n, id_base=base)
    try:
        c.upsert(ids_all, rows)
        c.delete(np.array([base + 7, base + 64, base + 4000], np.uint64))
        valid = np.ones(n, bool)
        valid[[7, 64, 4000]] = False
        srows = orc.normalize_rows(rows) if metric == METRIC_COSINE else rows
        dq = dev_queries(orc, metric, qs)
        all_d = [orc.dist_all(ORC_METRIC[metric], dq[qi], srows) for qi in range(nq)]
        for k in [257, 1000, 4096, n, n + 100]:
            hi, hd, hc = same_as_host(c, orc, qs, k, metric)
            for qi in range(nq):  # and the oracle directly
                wi, wd = orc.lex_topk(all_d[qi][valid], ids_all[valid], k)
                assert hc[qi] == len(wi) == min(k, n - 3)
                assert np.array_equal(hi[qi, :len(wi)], wi) and np.array_equal(bits(hd[qi, :len(wi)]), bits(wd))
    finally:
        c.destroy()


# ---- 2. row-length forms of the AVX2 order -----------------------------------------------------------
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT, METRIC_COSINE])
@pytest.mark.parametrize("d", [4, 8, 44, 136, 200])
def test_row_length_forms(ctx, orc, metric, d):
    """32-blocks, leftover 8-blocks and the 4-float scalar tail in every mix (8 = one 8-block; 44 = 32 +
    8 + 4; 136 = 4 x 32 + 8; 200 = 6 x 32 + 8); d = 4 takes the per-query keys."""
    n, nq, k = 1500, 3, 300
    rows = orc.synth_rows(2210 + d, 0, n, d, 0)
    qs = orc.synth_rows(2211 + d, 0, nq, d, 0)
    c = Corpus(ctx, KIND_F32, metric, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        same_as_host(c, orc, qs, k, (metric, d))
    finally:
        c.destroy()


# ---- 3. ties -------------------------------------------------------------------------------------------
def test_ties_f32(ctx, orc):
    """Integer rows floor(x / 64) (values 0..3, d = 8: a handful of distinct distances), every 7th row
    deleted, two of the four queries identical.  The compaction gives workgroup r the 2048 consecutive
    slots [2048 r, 2048 (r + 1)): n = 7000 is 110 tiles = 7040 slots = 4 workgroups, so the rows that tie
    at the threshold are ranked across workgroup boundaries."""
    n, d = 7000, 8
    assert ((n + 63) // 64 * 64 + RANGE - 1) // RANGE >= 3  # compaction workgroups
    rows = np.floor(orc.synth_rows(2221, 0, n, d, 1) / 64).astype(np.float32)
    qs = np.floor(orc.synth_rows(2222, 0, 4, d, 1) / 64).astype(np.float32)
    qs[2] = qs[0]
    ids_all = np.arange(n, dtype=np.uint64)
    c = Corpus(ctx, KIND_F32, METRIC_L2, d, n)
    try:
        c.upsert(ids_all, rows)
        c.delete(np.arange(0, n, 7, dtype=np.uint64))
        valid = np.ones(n, bool)
        valid[::7] = False
        tied = 0
        for k in [300, 2000, 5000]:
            tied += sum(kth_ties(orc.dist_all(0, q, rows)[valid], k) for q in qs)
            got = dev_search(c, qs, k)
            same(got, c.search(qs, k), k)
            assert np.array_equal(got[0][0], got[0][2]) and np.array_equal(bits(got[1][0]), bits(got[1][2]))
            assert got[2][0] == got[2][2] == k
        assert tied >= 1  # the tie rule was exercised
    finally:
        c.destroy()


# ---- 4. BQ ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 200])
def test_bq(ctx, orc, d):
    """Hamming distances 0..d: thousands of rows tie at the threshold."""
    n, nq = 5003, 9
    rows = orc.synth_rows(2231 + d, 0, n, d, 0)
    qs = orc.synth_rows(2232 + d, 0, nq, d, 0)
    c = Corpus(ctx, KIND_BQ, METRIC_L2, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        c.delete(np.array([7, 64, 4000], np.uint64))
        valid = np.ones(n, bool)
        valid[[7, 64, 4000]] = False
        codes = np.stack([orc.bq_encode(r) for r in rows])
        tied = 0
        for k in [300, 3000]:
            same_as_host(c, orc, qs, k, d)
            tied += sum(kth_ties(orc.bq_dist_all(orc.bq_encode(q), codes)[valid], k) for q in qs)
        assert tied >= 1
    finally:
        c.destroy()


# ---- 5. PQ ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,d,metric", [(16, 64, METRIC_DOT), (192, 192, METRIC_L2)])
def test_pq(ctx, orc, m, d, metric):
    """LUT in LDS (16 x 256 x 4 B = 16 KiB) and beyond it (192 x 256 x 4 B = 192 KiB > 160 KiB)."""
    n, nq, k, ks = 3000, 5, 500, 256
    centers = orc.synth_rows(2241 + m, 0, m * ks, d // m, 0).reshape(m, ks, d // m)
    rows = orc.synth_rows(2242 + m, 0, n, d, 0)
    qs = orc.synth_rows(2243 + m, 0, nq, d, 0)
    c = Corpus(ctx, KIND_PQ, metric, d, n)
    try:
        c.set_codebook(centers)
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        c.delete(np.array([7, 64], np.uint64))
        same_as_host(c, orc, qs, k, m)
    finally:
        c.destroy()


# ---- 6. per-query key routes ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [METRIC_MANHATTAN, METRIC_HAMMING])
def test_manhattan_hamming(ctx, orc, metric):
    n, d, nq, k = 2000, 16, 5, 300
    dist = 1 if metric == METRIC_HAMMING else 0
    rows = orc.synth_rows(2251, 0, n, d, dist)
    qs = orc.synth_rows(2252, 0, nq, d, dist)
    if metric == METRIC_HAMMING:  # few distinct values, so elements do coincide
        rows, qs = np.floor(rows / 64).astype(np.float32), np.floor(qs / 64).astype(np.float32)
    c = Corpus(ctx, KIND_F32, metric, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        c.delete(np.array([3, 1999], np.uint64))
        same_as_host(c, orc, qs, k, metric)
    finally:
        c.destroy()


@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT])
def test_avx512_order(ctx, orc, metric):
    n, d, nq, k = 2000, 256, 5, 300
    rows = orc.synth_rows(2261, 0, n, d, 0)
    qs = orc.synth_rows(2262, 0, nq, d, 0)
    c = Corpus(ctx, KIND_F32, metric, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        want256 = c.search(qs, k)
        ctx.set_distance_order(ORDER_AVX512)
        try:
            want = same_as_host(c, orc, qs, k, metric)
        finally:
            ctx.set_distance_order(ORDER_AVX256)
        assert not np.array_equal(bits(want[1]), bits(want256[1]))  # the order is not a no-op at d = 256
        same(dev_search(c, qs, k), want256, "back in the AVX2 order")
    finally:
        c.destroy()


# ---- 7. edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 100, 256, 257])
def test_small_corpora(ctx, orc, n):
    """k = 257 at n = 100 and n = 256 (exactly 4 tiles) covers every slot: no select.  n = 257 has 320
    slots, so the select runs and finds exactly k live rows."""
    d, k = 32, 257
    rows = orc.synth_rows(2271 + n, 0, n, d, 0)
    qs = orc.synth_rows(2272 + n, 0, 5, d, 0)
    c = Corpus(ctx, KIND_F32, METRIC_L2, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        want = same_as_host(c, orc, qs, k, n)
        assert np.all(want[2] == min(k, n))
        one = dev_search(c, qs[:1], k)  # nq = 1
        same(one, tuple(x[:1] for x in want), "nq = 1")
        gi, gd, gc = dev_search(c, qs, k, with_counts=False)  # d_counts = NULL
        assert gc is None and np.array_equal(gi, want[0]) and np.array_equal(bits(gd), bits(want[1]))
    finally:
        c.destroy()


def test_all_deleted_and_empty(ctx, orc):
    n, d, k, nq = 300, 32, 257, 3
    rows = orc.synth_rows(2281, 0, n, d, 0)
    qs = orc.synth_rows(2282, 0, nq, d, 0)
    c = Corpus(ctx, KIND_F32, METRIC_L2, d, n)
    e = Corpus(ctx, KIND_F32, METRIC_L2, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        c.delete(np.arange(n, dtype=np.uint64))
        for corpus in (c, e):
            gi, gd, gc = dev_search(corpus, qs, k)
            assert np.all(gc == 0) and np.all(gi == NONE) and np.all(np.isposinf(gd))
            same((gi, gd, gc), corpus.search(qs, k))
    finally:
        c.destroy()
        e.destroy()


# ---- 8. special values ---------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT])
def test_special_values(ctx, orc, metric):
    """Rows holding +inf, -inf and NaN elements in the 32-block, the 8-block and the scalar tail of
    d = 44: distances of +inf, -inf and NaN (NaN sorts last among the live rows)."""
    n, d, nq, k = 700, 44, 3, 400
    rng = np.random.default_rng(2291 + metric)
    rows = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    qs = rng.uniform(-1, 1, (nq, d)).astype(np.float32)
    for i, pos in enumerate((5, 35, 41)):
        rows[10 + i, pos] = np.inf
        rows[20 + i, pos] = -np.inf
        rows[30 + i, pos] = np.nan
        rows[300 + 64 * i, pos] = np.nan
    rows[40, 3], rows[40, 4] = np.inf, -np.inf
    c = Corpus(ctx, KIND_F32, metric, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        for kk in (k, n):
            want = same_as_host(c, orc, qs, kk, metric)
        assert np.isnan(want[1]).any() and np.isinf(want[1][:, :n]).any()
    finally:
        c.destroy()


# ---- 9. workspace and errors ---------------------------------------------------------------------------
def test_workspace_and_errors(ctx, orc):
    import torch

    lib = _lib.load()
    dev = torch.device("cuda:0")
    n, d, nq = 3000, 64, 5
    rows = orc.synth_rows(2301, 0, n, d, 0)
    qs = orc.synth_rows(2302, 0, nq, d, 0)
    c = Corpus(ctx, KIND_F32, METRIC_L2, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        size = lib.wvg_search_workspace_size(c.handle, nq, 1000)
        assert size == lib.wvg_search_workspace_size(c.handle, nq, 1000)
        assert size == lib.wvg_search_workspace_size(c.handle, 64, 1000)  # G key arrays, not nq (F32: no codes / LUTs)
        assert size >= 256 + 4 * 4 * 3008 + 2 * 4 * 1000 * 8
        tq = torch.from_numpy(qs).to(dev)
        oi = torch.full((nq, 1000), 7, dtype=torch.int64, device=dev)
        od = torch.full((nq, 1000), -7.0, dtype=torch.float32, device=dev)
        oc = torch.full((nq,), 77, dtype=torch.int32, device=dev)
        ws = torch.zeros(size, dtype=torch.uint8, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        with pytest.raises(_lib.WvgError, match="workspace too small") as ei:
            _lib.check(lib.wvg_search_device(c.handle, tq.data_ptr(), nq, 1000, oi.data_ptr(), od.data_ptr(),
                                             oc.data_ptr(), ws.data_ptr(), size - 1, s))
        assert ei.value.code == _lib.WVG_ERR_INVALID
        torch.cuda.synchronize()
        assert int((oi != 7).sum()) == 0 and int((od != -7.0).sum()) == 0 and int((oc != 77).sum()) == 0
        assert int(ws.sum()) == 0  # nothing was launched
        _lib.check(lib.wvg_search_device(c.handle, tq.data_ptr(), nq, 1000, oi.data_ptr(), od.data_ptr(),
                                         oc.data_ptr(), ws.data_ptr(), size, s))
        torch.cuda.synchronize()
        want1000 = c.search(qs, 1000)
        same((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)), want1000)
        # one workspace for calls of different k and entry points, in order on one stream
        big = max(lib.wvg_search_workspace_size(c.handle, nq, k) for k in (10, 1000))
        ws = torch.zeros(big, dtype=torch.uint8, device=dev)
        want10 = c.search(qs, 10)
        same(dev_search(c, qs, 10, ws=ws), want10, "k = 10")
        same(dev_search(c, qs, 1000, ws=ws), want1000, "k = 1000")
        same(dev_search(c, qs, 10, ws=ws, entry="wvg_search_device_pipelined"), want10, "pipelined")
        _lib.check(lib.wvg_search_device_check(ctx.handle, ws.data_ptr(), s))
        assert int(ws[:256].sum()) == 0  # the status block and the arrival counters stayed zero
        # the other entry points keep their cap
        with pytest.raises(_lib.WvgError, match="k above 256"):
            dev_search(c, qs, 300, ws=ws, entry="wvg_search_device_pipelined")
    finally:
        c.destroy()


# ---- 10. capture ---------------------------------------------------------------------------------------
def test_graph_capture(ctx, orc):
    import torch

    lib = _lib.load()
    dev = torch.device("cuda:0")
    n, d, nq, k = 5000, 64, 5, 1000
    rows = orc.synth_rows(2311, 0, n, d, 0)
    sets = [orc.synth_rows(2312 + i, 0, nq, d, 0) for i in range(3)]
    c = Corpus(ctx, KIND_F32, METRIC_DOT, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        ws = torch.zeros(lib.wvg_search_workspace_size(c.handle, nq, k), dtype=torch.uint8, device=dev)
        same(dev_search(c, sets[0], k, ws=ws), c.search(sets[0], k), "eager")
        tq = torch.from_numpy(sets[0]).to(dev)
        oi = torch.zeros((nq, k), dtype=torch.int64, device=dev)
        od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
        oc = torch.zeros(nq, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _lib.check(lib.wvg_search_device(c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                             oc.data_ptr(), ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert int(oi.abs().sum()) == 0 and int(oc.sum()) == 0  # captured, not run
        for qs in sets[1:]:
            tq.copy_(torch.from_numpy(qs))
            g.replay()
            torch.cuda.synchronize()
            same((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)),
                 c.search(qs, k), "replay")
    finally:
        c.destroy()

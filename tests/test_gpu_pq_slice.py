"""The slice form of the PQ query stream (scan_pq_qshare_slice_kernel, wvg_pq_qslice.hip) in a cache_reuse = 2
context.  The reference of every case is per query wvg_search(c, q_i, 1, k, allow_i) on the same corpus (K8,
pinned against the oracle by test_gpu_pq_k8_matrix.py): ids, distance bits, counts and padding equal."""
import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import METRIC_DOT, METRIC_L2
from weaviate_amd.device import Context

from test_gpu_bq_stream import _check_filtered, padded, plan, same
from test_gpu_parity import check_topk
from test_gpu_pq_k8_matrix import _all_d, _centers, _corpus, _near, _queries
from test_gpu_pq_stream import DEAD, N, Ref, _pipelined
from test_gpu_qshare_filter import filtered_search

pytestmark = pytest.mark.gpu

# (m, ks, ds): three full slices; a short last slice; 13 chunks, the last half filled; S = 64
SHAPES = [(96, 256, 4), (112, 256, 2), (200, 256, 2), (192, 128, 2)]
T = 8  # tiles per block at k <= 128 (4 above)
NQK = [(2, 10), (5, 100), (9, 200)]  # E = 1; a last pass of one query, E = 2; E = 4
# 16 T + 16 T / 2 + 3 tiles per row range at 256 ranges: a full and a short block beside waves with a tile more
N_BIG = 64 * (16 * T + 16 * T // 2 + 3) * 256 + 17


@pytest.fixture(scope="module")
def ref2(ctx, orc):
    """Ref (N rows, DEAD deleted, 11 queries) of a shape on a cache_reuse = 2 context, made once."""
    c2, made = Context(0, cache_reuse=2), {}
    yield lambda *key: made[key] if key in made else made.setdefault(key, Ref(c2, orc, *key))
    for r in made.values():
        r.c.destroy()
    c2.close()


def _check(c, qs, k, words=None, calls=None):
    """The calls' results (default: two unfiltered calls, both directions) against nq wvg_search calls; the last."""
    res = [c.search(qs[[i]], k, allow=None if words is None else words[i]) for i in range(len(qs))]
    want = tuple(np.concatenate([r[j] for r in res]) for j in range(3))
    padded(want)
    assert plan(c, len(qs), k) == (1, 4, -(-len(qs) // 4), 0, 0)
    for got in calls or _pipelined(c, qs, k):
        same(got, want)
    return got


@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT])
@pytest.mark.parametrize("m,ks,ds", SHAPES)
def test_matrix(ref2, orc, m, ks, ds, metric):
    r = ref2(m, ks, ds, metric)
    for nq, k in NQK:
        got = _check(r.c, r.pq[:nq], k)
    if m == 96:  # adc_all, the numpy restatement of the sum (k = 200)
        valid = np.ones(N, bool)
        valid[DEAD] = False
        for qi, d in enumerate(_all_d(orc, metric, r.raw[:nq], r.centers, r.codes)):
            check_topk(orc, got[0][qi], got[1][qi], got[2][qi], *_near(d, valid, 256), k)
        # 100 rows: fifteen waves have no tile and still meet every barrier
        c = _corpus(r.c.ctx, metric, r.centers, r.codes[:100], np.array([3], np.uint64))
        for nq, k in NQK:
            _check(c, r.pq[:nq], k)
        c.destroy()
    if m == 112 and metric == METRIC_L2:  # the stream tests' lists and window (id_base 640)
        for nq, k in ((9, 10), (5, 200)):
            _check_filtered(ref2(m, ks, ds, metric, 640), nq, k)


def test_blocks_and_filters(ref2, orc):
    """N_BIG rows at (96, 256), several row ranges, scattered deleted rows and three dead tiles in one
    block; then per-query lists: tiles 1000 .. 1039 (more than 2 T) allowed by no query of pass 0."""
    rng = np.random.default_rng(7702)
    dead = np.unique(np.concatenate([np.arange(64 * 2001, 64 * 2004), rng.choice(N_BIG, 3000, replace=False)]))
    c = _corpus(ref2(96, 256, 4, METRIC_L2).c.ctx, METRIC_L2, _centers(orc, 7701, 96, 256, 4),
                rng.integers(0, 256, (N_BIG, 96), dtype=np.uint8), dead.astype(np.uint64))
    try:
        qs = _queries(orc, 7703, 9, 384)
        for nq, k in NQK:
            _check(c, qs[:nq], k)
        rows = np.arange(N_BIG + -N_BIG % 64)
        hole = (rows >= 64 * 1000) & (rows < 64 * 1040)
        masks = [(rows >= 64 * 300) & ~hole,  # begins after the first row range
                 rows < 0,                    # all zeros
                 (rows % 7 == 0) & (rows >= 64 * 990) & (rows < 64 * 5000) & ~hole,
                 (rows >= 64 * 2000) & (rows < 64 * 2008),  # the block with the dead tiles
                 rows >= 0]                   # pass 1
        words = np.stack([np.packbits(mk, bitorder="little").view(np.uint64) for mk in masks])
        for k in (10, 200):
            got = _check(c, qs[:5], k, words, filtered_search(c, qs[:5], k, [words, words], 0, words.shape[1]))
            assert got[2][1] == 0 and got[2][0] == k
    finally:
        c.destroy()


def test_plan_and_workspace(ctx, ref2, orc):
    for m, ds, q in ((96, 4, 4), (64, 2, 2), (32, 4, 4)):
        cs = [_corpus(cx, METRIC_L2, _centers(orc, 7800 + m, m, 256, ds), np.zeros((5000, m), np.uint8),
                      np.zeros(0, np.uint64)) for cx in (ref2(96, 256, 4, METRIC_L2).c.ctx, ctx)]
        for k in (10, 100, 200):
            for nq in (2, 5, 9):
                assert plan(cs[0], nq, k) == (1, q, -(-nq // q), 0, 0)
                assert plan(cs[1], nq, k) == ((1, q, -(-nq // q), 0, 0) if m < 96 else (0, 1, nq, 0, 0))
                assert len({c.lib.wvg_search_workspace_size(c.handle, nq, k) for c in cs}) == 1
            assert plan(cs[0], 1, k) == (0, 1, 1, 0, 0)
        for c in cs:
            c.destroy()


def test_captured_call_replays(ref2):
    import torch

    r = ref2(96, 256, 4, METRIC_L2)
    lib, nq, k, dev = r.c.lib, 5, 10, torch.device("cuda:0")
    want = _pipelined(r.c, r.pq[:nq], k, reps=1)[0]
    ws = torch.zeros(lib.wvg_search_workspace_size(r.c.handle, nq, k), dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(np.ascontiguousarray(r.pq[:nq])).to(dev)
    oi, od, oc = (torch.zeros(sh, dtype=t, device=dev) for sh, t in
                  (((nq, k), torch.int64), ((nq, k), torch.float32), (nq, torch.int32)))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(lib.wvg_search_device_pipelined(r.c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                                   oc.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   torch.cuda.current_stream().cuda_stream))
    for _ in range(2):
        oi.zero_(), od.zero_(), oc.zero_()
        g.replay()
        same((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)), want)

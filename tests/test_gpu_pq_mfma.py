"""K8m (wvg_pq_mfma.hip: batched PQ ADC search on the bf16 matrix cores, a batch_screen = 6 context) returns the
ids, distance bits, counts and padding of the default route (one K8 scan per query); two queries per case also go
against the oracle's ADC distances (orc.pq_lut / orc.pq_adc, pinned to adc_all in test_gpu_pq_k8_matrix.py)."""
import ctypes

import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import KIND_BQ, KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_L2
from weaviate_amd.device import Context, Corpus, allow_bitmap

from test_gpu_parity import check_topk
from test_gpu_pq_k8_matrix import _centers, _corpus, _queries, _same, adc_all

pytestmark = pytest.mark.gpu

SHAPES = [(32, 256, 4), (16, 256, 8), (8, 256, 4), (24, 256, 4), (64, 64, 8)]  # (m, ks, dsub)
N = 3 * 2048 + 100  # three of the kernel's minimum row ranges and a ragged last tile
DEAD = np.array([0, 63, 64, 2047, 2048, 4100, N - 1], np.uint64)


@pytest.fixture(scope="module")
def pair_ctx(ctx):
    m, p = Context(0, batch_screen=6, mfma_min_queries=2), Context(0, mfma_min_queries=2)
    yield m, p
    m.close()
    p.close()


def plan_of(c, nq, k):
    bp = _lib.BatchPlan()
    _lib.check(c.lib.wvg_search_batch_plan(c.handle, nq, k, 0, ctypes.byref(bp)))
    return int(bp.matrix), int(bp.screen), int(bp.shadow_bytes_per_row), int(bp.reserved)


_CASES = {}


def case_of(orc, pair_ctx, name, m, ks, ds):
    """(centers, codes, queries, valid, allow words, K8m corpus, default corpus) of a case: built once, read only."""
    key = (name, m, ks, ds)
    if key in _CASES:
        return _CASES[key]
    n = {"few": 50, "ties": 3000}.get(name, N)
    cen = _centers(orc, 7100 + m + ks, m, ks, ds)
    codes = np.random.default_rng(7200 + m + ks + len(name)).integers(0, ks, (n, m), dtype=np.uint8)
    qs = _queries(orc, 7300 + m, 67, m * ds)
    if name == "ties":
        codes[700:2200] = codes[700]
        qs[::3] = cen[np.arange(m), codes[700]].reshape(-1)
    if name == "tighten":  # queries around one point, rows stored farthest first: every step tightens the bound
        qs = (qs[0] + np.float32(0.05) * qs).astype(np.float32)
        codes = codes[np.argsort(-adc_all(0, orc.pq_lut(0, qs[0], cen), codes), kind="stable")]
    if name == "nonfinite":
        cen = cen.copy()
        cen[1, 5, 0], cen[m - 1, 7, ds - 1] = np.nan, np.inf
        qs[3, 2], qs[5] = np.nan, np.float32(1e30)
    valid, al = np.ones(n, np.uint8), None
    dead = DEAD if n == N else np.array([1], np.uint64)
    valid[dead.astype(np.int64)] = 0
    if name == "allow":
        al = allow_bitmap(np.arange(1, n, 3, dtype=np.uint64), n)
        valid[0::3] = valid[2::3] = 0
    _CASES[key] = (cen, codes, qs, valid, al, *(_corpus(cx, METRIC_L2, cen, codes, dead) for cx in pair_ctx))
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _destroy_cases(pair_ctx):  # (after pair_ctx: the corpora go before their contexts)
    yield
    for v in _CASES.values():
        v[5].destroy()
        v[6].destroy()
    _CASES.clear()


def check(orc, case, nq, k, oracle=True):
    cen, codes, qs, valid, al, a, b = case
    qs = qs[[0, 66]] if nq == 2 else qs[:nq]
    pa = plan_of(a, nq, k)
    assert pa[:3] == (1, 1, 0) and pa[3] >= 1 and plan_of(b, nq, k) == (0, 0, 0, 0)
    got = a.search(qs, k, al)
    _same(got, b.search(qs, k, al))
    cnt = min(k, int(valid.sum()))
    assert np.all(got[2] == cnt)
    assert np.all(got[0][:, cnt:] == np.uint64(0xFFFFFFFFFFFFFFFF)) and np.all(np.isposinf(got[1][:, cnt:]))
    for qi in (0, nq - 1) if oracle else ():
        lut = orc.pq_lut(0, qs[qi], cen)
        all_d = adc_all(0, lut, codes)  # (orc.pq_adc row by row, vectorised; pinned on a few rows)
        assert all(all_d[r].tobytes() == orc.pq_adc(0, lut, codes[r]).tobytes() for r in (0, len(codes) - 1))
        check_topk(orc, got[0][qi], got[1][qi], got[2][qi], all_d, np.arange(len(codes), dtype=np.uint64), k, valid)


@pytest.mark.parametrize("k", [1, 10, 200, 256])
@pytest.mark.parametrize("nq", [2, 67])
@pytest.mark.parametrize("m,ks,ds", SHAPES)
def test_mfma_equals_default(pair_ctx, orc, m, ks, ds, nq, k):
    check(orc, case_of(orc, pair_ctx, "base", m, ks, ds), nq, k)


@pytest.mark.parametrize("k", [10, 256])
@pytest.mark.parametrize("name", ["allow", "few", "ties", "tighten"])
def test_mfma_extra_cases(pair_ctx, orc, name, k):
    case = case_of(orc, pair_ctx, name, 32, 256, 4)
    if name == "tighten":  # a range longer than two pools: a second compaction runs whatever the data
        ranges = plan_of(case[5], 67, k)[3]
        assert ranges >= 2 and (N // 256 // ranges) * 256 > 2 * (2 * max(k, 64) + 256)
    check(orc, case, 67, k)


def test_nonfinite(pair_ctx, orc):
    """A NaN and a +inf centroid, a query with a NaN, a query of 1e30: never a skip, the default route's results."""
    check(orc, case_of(orc, pair_ctx, "nonfinite", 32, 256, 4), 67, 10, oracle=False)


def test_plans(pair_ctx, orc):
    """Outside its rule a PQ batch keeps its route (and its results); F32 and BQ plans under 6 are 2's."""
    m6, dflt = pair_ctx
    base = case_of(orc, pair_ctx, "base", 32, 256, 4)
    assert plan_of(base[5], 67, 257)[0] == 0 and plan_of(base[5], 1, 10)[0] == 0
    lib = base[5].lib
    with Context(0, batch_screen=2, mfma_min_queries=2) as two:
        for i, (m, ks, ds) in enumerate([(16, 256, 2), (12, 256, 4), (64, 256, 8)]):  # dsub 2, dim % 32, 256 KiB
            cen = _centers(orc, 7400 + i, m, ks, ds)
            codes = np.random.default_rng(7500 + i).integers(0, ks, (300, m), dtype=np.uint8)
            qs = _queries(orc, 7600 + i, 5, m * ds)
            a, b = (_corpus(cx, METRIC_L2, cen, codes, np.array([3], np.uint64)) for cx in (m6, dflt))
            assert plan_of(a, 5, 10) == (0, 0, 0, 0)
            _same(a.search(qs, 10), b.search(qs, 10))
            a.destroy()
            b.destroy()
        cen, codes = base[0], base[1][:200]
        for cx, metric in ((m6, METRIC_DOT), (two, METRIC_L2)):  # a dot corpus; a batch_screen = 2 context
            c = _corpus(cx, metric, cen, codes, np.array([1], np.uint64))
            assert plan_of(c, 67, 10) == (0, 0, 0, 0)
            c.destroy()
        c2 = _corpus(two, METRIC_L2, base[0], base[1], DEAD)
        assert lib.wvg_search_workspace_size(base[5].handle, 67, 10) >= lib.wvg_search_workspace_size(c2.handle, 67, 10)
        c2.destroy()
        for kind, metric, fd in ((KIND_F32, METRIC_L2, 768), (KIND_F32, METRIC_COSINE, 96), (KIND_BQ, METRIC_L2, 130)):
            f6, f2 = (Corpus(cx, kind, metric, fd, 256) for cx in (m6, two))
            for f in (f6, f2):
                f.upsert(np.arange(200, dtype=np.uint64), orc.synth_rows(7700, 0, 200, fd, 0))
            assert all(plan_of(f6, 32, k) == plan_of(f2, 32, k) for k in (10, 100, 257))
            f6.destroy()
            f2.destroy()


def test_device_graph_first_call(pair_ctx, orc):
    """wvg_search_device takes K8m; captured as the very first call on a fresh workspace (the route has no shadow to
    warm) it replays three times to the same bits: every count, bound, flag and threshold is set inside the call."""
    import torch
    nq, k = 67, 256
    cen, codes, qs, valid, al, a, b = case_of(orc, pair_ctx, "tighten", 32, 256, 4)
    want = b.search(qs, k)
    assert plan_of(a, nq, k)[0] == 1
    lib, dev = a.lib, torch.device("cuda:0")
    ws = torch.full((lib.wvg_search_workspace_size(a.handle, nq, k),), 0xA5, dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(qs).to(dev)
    oi, od, oc = (torch.zeros(sh, dtype=t, device=dev)
                  for sh, t in (((nq, k), torch.int64), ((nq, k), torch.float32), (nq, torch.int32)))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(lib.wvg_search_device(a.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    for _ in range(3):
        for t in (oi, od, oc):
            t.zero_()
        ws.fill_(0xA5)  # whatever an earlier replay left behind
        g.replay()
        torch.cuda.synchronize()
        _same((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)), want)

"""K8m-S (wvg_pq_mfma.hip: the batched PQ ADC screen for codebooks beyond LDS, a batch_screen = 7 context) returns
the ids, distance bits, counts and padding of the default route; two queries per case also go against the oracle's
ADC distances (orc.pq_lut / orc.pq_adc, pinned to adc_all in test_gpu_pq_k8_matrix.py)."""
import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import KIND_BQ, KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_L2
from weaviate_amd.device import Context, Corpus, allow_bitmap

from test_gpu_parity import check_topk
from test_gpu_pq_k8_matrix import _centers, _corpus, _queries, _same, adc_all
from test_gpu_pq_mfma import plan_of

pytestmark = pytest.mark.gpu

# (m, ks, dsub): 6 chunks; half-chunk slices; 12 chunks; rotated rows; test_plans' shape; a half chunk; ks < 256
SHAPES = [(96, 256, 4), (96, 256, 8), (192, 256, 8), (32, 256, 8), (64, 256, 8), (72, 256, 8), (192, 64, 8)]
N = 3 * 2048 + 100  # three of the kernel's minimum row ranges (four 512-row blocks) and a ragged last block and tile
DEAD = np.array([0, 63, 64, 511, 512, 2047, 2048, 4095, 4096, 6143, 6144, N - 1], np.uint64)  # tile, block, range edges


@pytest.fixture(scope="module")
def pair_ctx(ctx):
    with Context(0, batch_screen=7, mfma_min_queries=2) as m, Context(0, mfma_min_queries=2) as p:
        yield m, p


_CASES = {}


def case_of(orc, pair_ctx, name, m, ks, ds):
    """(centers, codes, queries, valid, allow words, K8m-S corpus, default corpus) of a case: built once, read only."""
    if (key := (name, m, ks, ds)) in _CASES:
        return _CASES[key]
    n = {"few": 50, "ties": 3000}.get(name, N)
    cen = _centers(orc, 8100 + m + ks + ds, m, ks, ds)
    codes = np.random.default_rng(8200 + m + ks + len(name)).integers(0, ks, (n, m), dtype=np.uint8)
    qs = _queries(orc, 8300 + m, 67, m * ds)
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
    assert np.all(got[2] == cnt) and np.all(got[0][:, cnt:] == np.uint64(2**64 - 1)) and np.all(np.isposinf(got[1][:, cnt:]))
    for qi in (0, nq - 1) if oracle else ():
        lut = orc.pq_lut(0, qs[qi], cen)
        all_d = adc_all(0, lut, codes)  # (orc.pq_adc row by row, vectorised; pinned on two rows)
        assert all(all_d[r].tobytes() == orc.pq_adc(0, lut, codes[r]).tobytes() for r in (0, len(codes) - 1))
        check_topk(orc, got[0][qi], got[1][qi], got[2][qi], all_d, np.arange(len(codes), dtype=np.uint64), k, valid)


@pytest.mark.parametrize("k", [1, 10, 256])
@pytest.mark.parametrize("nq", [2, 67])
@pytest.mark.parametrize("m,ks,ds", SHAPES)
def test_slice_equals_default(pair_ctx, orc, m, ks, ds, nq, k):
    check(orc, case_of(orc, pair_ctx, "base", m, ks, ds), nq, k)


@pytest.mark.parametrize("k", [10, 256])
@pytest.mark.parametrize("name", ["allow", "few", "ties", "tighten"])
def test_slice_extra_cases(pair_ctx, orc, name, k):
    case = case_of(orc, pair_ctx, name, 96, 256, 8)
    if name == "tighten":  # a range longer than two pools: a second compaction runs whatever the data
        ranges = plan_of(case[5], 67, k)[3]
        assert ranges >= 2 and (N // 512 // ranges) * 512 > 2 * (2 * max(k, 64) + 256)
    check(orc, case, 67, k)


def test_nonfinite(pair_ctx, orc):
    # a NaN and a +inf centroid, a query with a NaN, a query of 1e30: never a skip, the default route's results
    check(orc, case_of(orc, pair_ctx, "nonfinite", 96, 256, 8), 67, 10, oracle=False)


def test_routing(pair_ctx, orc):
    """K8m's shapes stay K8m's under 7; a dot corpus keeps its route; the workspace only grows; F32 and BQ as 2."""
    m7, dflt = pair_ctx
    big, lib = case_of(orc, pair_ctx, "base", 96, 256, 8), m7.lib
    cen = _centers(orc, 8400, 32, 256, 4)
    codes = np.random.default_rng(8401).integers(0, 256, (N, 32), dtype=np.uint8)
    qs = _queries(orc, 8402, 67, 128)
    with Context(0, batch_screen=6, mfma_min_queries=2) as six, Context(0, batch_screen=2, mfma_min_queries=2) as two:
        a, b = (_corpus(cx, METRIC_L2, cen, codes, DEAD) for cx in (m7, six))
        assert plan_of(a, 67, 10) == plan_of(b, 67, 10) and plan_of(a, 67, 10)[0] == 1
        _same(a.search(qs, 10), b.search(qs, 10))
        a.destroy()
        b.destroy()
        c = _corpus(m7, METRIC_DOT, big[0], big[1][:200], np.array([1], np.uint64))
        assert plan_of(c, 67, 10) == (0, 0, 0, 0)
        c.destroy()
        for cx in (six, two):
            c = _corpus(cx, METRIC_L2, big[0], big[1], DEAD)
            assert lib.wvg_search_workspace_size(big[5].handle, 67, 10) >= lib.wvg_search_workspace_size(c.handle, 67, 10)
            c.destroy()
        for kind, metric, fd in ((KIND_F32, METRIC_L2, 768), (KIND_F32, METRIC_COSINE, 96), (KIND_BQ, METRIC_L2, 130)):
            f7, f2 = (Corpus(cx, kind, metric, fd, 256) for cx in (m7, two))
            for f in (f7, f2):
                f.upsert(np.arange(200, dtype=np.uint64), orc.synth_rows(8500, 0, 200, fd, 0))
            assert all(plan_of(f7, 32, k) == plan_of(f2, 32, k) for k in (10, 100, 257))
            f7.destroy()
            f2.destroy()


def test_device_graph_first_call(pair_ctx, orc):
    """Captured as the very first call on a fresh workspace, wvg_search_device replays three times to the same bits."""
    import torch
    nq, k = 67, 256
    cen, codes, qs, valid, al, a, b = case_of(orc, pair_ctx, "tighten", 96, 256, 8)
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

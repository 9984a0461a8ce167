"""K5m (wvg_bq_mfma.hip: batched BQ Hamming search on the int8 matrix cores, a batch_screen = 5 context)
returns the ids, distance bits, counts and padding of the default route (co-scheduled K5); two queries per
case also go against the oracle's exact integer Hamming distances."""
import ctypes

import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import KIND_BQ, KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_L2
from weaviate_amd.device import Context, Corpus, allow_bitmap

from test_gpu_bq_k5_matrix import DEAD, N, Q_NEG, make_queries, make_rows
from test_gpu_parity import check_topk, prep_query, stored_rows
from test_gpu_screen import _same

pytestmark = pytest.mark.gpu

DIMS = [(METRIC_L2, 64), (METRIC_L2, 130), (METRIC_COSINE, 130), (METRIC_L2, 768), (METRIC_L2, 1536),
        (METRIC_L2, 2048), (METRIC_L2, 2112)]
TIGHTEN_N = 3 * 2048 + 100  # three row ranges of at least 2048 rows each


@pytest.fixture(scope="module")
def pair_ctx(ctx):
    m, p = Context(0, batch_screen=5, mfma_min_queries=2), Context(0, mfma_min_queries=2)
    yield m, p
    m.close()
    p.close()


def plan_of(c, nq, k):
    """(matrix, K5m's planned row ranges) of a batch."""
    bp = _lib.BatchPlan()
    _lib.check(c.lib.wvg_search_batch_plan(c.handle, nq, k, 0, ctypes.byref(bp)))
    return int(bp.matrix), int(bp.reserved)


_CASES = {}


def case_of(orc, pair_ctx, name, metric, d):
    """(rows, queries, valid, allow words, K5m corpus, default corpus) of a case: built once, read only."""
    key = (name, metric, d)
    if key in _CASES:
        return _CASES[key]
    if name in ("base", "allow"):
        rows = make_rows(orc, d)
        qs = np.concatenate([make_queries(orc, d), orc.synth_rows(4100 + d, 0, 59, d, 0)])
    else:
        n = {"few": 50, "ties": 3000, "tighten": TIGHTEN_N}[name]
        rows, qs = orc.synth_rows(5000 + d, 0, n, d, 0), orc.synth_rows(5001 + d, 0, 67, d, 0)
    if name == "ties":
        rows[700:2200] = rows[700]
        qs[::3] = rows[700]
    if name == "tighten":  # queries around one point, rows stored farthest first: every step tightens the bound
        qs = (qs[0] + np.float32(0.05) * qs).astype(np.float32)
        far = orc.bq_dist_all(orc.bq_encode(qs[0]), orc.bq_encode_rows(rows))
        rows = rows[np.argsort(-far, kind="stable")]
    n = len(rows)
    valid, al = np.ones(n, np.uint8), None
    dead = np.array(DEAD if n == N else [], np.uint64)
    valid[dead.astype(np.int64)] = 0
    if name == "allow":
        al = allow_bitmap(np.arange(1, n, 3, dtype=np.uint64), n)
        valid[0::3] = valid[2::3] = 0
    corpora = []
    for cx in pair_ctx:
        c = Corpus(cx, KIND_BQ, metric, d, n)
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        if len(dead):
            c.delete(dead)
        corpora.append(c)
    _CASES[key] = (rows, qs, valid, al, *corpora)
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def _destroy_cases(pair_ctx):  # (after pair_ctx: the corpora go before their contexts)
    yield
    for v in _CASES.values():
        v[4].destroy()
        v[5].destroy()
    _CASES.clear()


def check(orc, case, metric, nq, k):
    rows, qs, valid, al, a, b = case
    qs = qs[[0, Q_NEG]] if nq == 2 else qs[:nq]
    assert plan_of(a, nq, k)[0] == 1 and plan_of(b, nq, k)[0] == 0
    got = a.search(qs, k, al)
    _same(got, b.search(qs, k, al))
    cnt = min(k, int(valid.sum()))
    assert np.all(got[2] == cnt)
    assert np.all(got[0][:, cnt:] == np.uint64(0xFFFFFFFFFFFFFFFF)) and np.all(np.isposinf(got[1][:, cnt:]))
    codes = orc.bq_encode_rows(stored_rows(orc, metric, rows))
    for qi in (0, nq - 1):
        all_d = orc.bq_dist_all(orc.bq_encode(prep_query(orc, metric, qs[qi])), codes)
        check_topk(orc, got[0][qi], got[1][qi], got[2][qi], all_d, np.arange(len(rows), dtype=np.uint64), k, valid)


@pytest.mark.parametrize("k", [1, 10, 200, 256])
@pytest.mark.parametrize("nq", [2, 67])
@pytest.mark.parametrize("metric,d", DIMS)
def test_mfma_equals_default(pair_ctx, orc, metric, d, nq, k):
    check(orc, case_of(orc, pair_ctx, "base", metric, d), metric, nq, k)


@pytest.mark.parametrize("k", [10, 200, 256])
@pytest.mark.parametrize("name", ["allow", "few", "ties", "tighten"])
@pytest.mark.parametrize("d", [130, 1536])
def test_mfma_extra_cases(pair_ctx, orc, d, name, k):
    case = case_of(orc, pair_ctx, name, METRIC_L2, d)
    if name == "tighten":  # a range longer than two pools: a second compaction runs whatever the data
        ranges = plan_of(case[4], 67, k)[1]
        assert ranges >= 2 and (TIGHTEN_N // 256 // ranges) * 256 > 2 * (2 * max(k, 64) + 256)
    check(orc, case, METRIC_L2, 67, k)


def test_plans(pair_ctx, orc):
    """Past 4096 bits, past k = 256 and outside a batch_screen = 5 context a BQ batch keeps K5; F32 plans are 2's."""
    m, p = pair_ctx
    d, n = 4160, 300
    rows, qs = orc.synth_rows(5100, 0, n, d, 0), orc.synth_rows(5101, 0, 5, d, 0)
    c = Corpus(m, KIND_BQ, METRIC_L2, d, n)
    with Context(0, batch_screen=2, mfma_min_queries=2) as two:
        try:
            c.upsert(np.arange(n, dtype=np.uint64), rows)
            assert plan_of(c, 5, 10) == (0, 0)
            ids, dists, counts = c.search(qs, 10)
            codes = orc.bq_encode_rows(rows)
            for qi in range(5):
                check_topk(orc, ids[qi], dists[qi], counts[qi], orc.bq_dist_all(orc.bq_encode(qs[qi]), codes),
                           np.arange(n, dtype=np.uint64), 10)
            base = case_of(orc, pair_ctx, "base", METRIC_L2, 130)
            assert plan_of(base[4], 67, 257)[0] == 0 and plan_of(base[4], 1, 10)[0] == 0
            c2 = Corpus(two, KIND_BQ, METRIC_L2, 130, 64)
            c2.upsert(np.arange(40, dtype=np.uint64), base[0][:40])
            assert plan_of(c2, 67, 10) == (0, 0)
            c2.destroy()
            for metric, fd in ((METRIC_L2, 768), (METRIC_DOT, 768), (METRIC_COSINE, 96)):
                f5, f2 = (Corpus(cx, KIND_F32, metric, fd, 256) for cx in (m, two))
                for f in (f5, f2):
                    f.upsert(np.arange(200, dtype=np.uint64), orc.synth_rows(5102, 0, 200, fd, 0))
                assert all(f5.batch_plan(32, k) == f2.batch_plan(32, k) for k in (10, 100, 257))
                f5.destroy()
                f2.destroy()
        finally:
            c.destroy()


def test_device_graph_replay(pair_ctx, orc):
    """wvg_search_device takes K5m; captured after one eager batch it replays three times to the same bits
    (image, counts, bounds and flags are all (re)initialised by kernels inside the capture)."""
    import torch
    d, nq, k = 130, 67, 256
    rows, qs, valid, al, a, b = case_of(orc, pair_ctx, "tighten", METRIC_L2, d)
    want = b.search(qs, k)
    lib, dev = a.lib, torch.device("cuda:0")
    ws = torch.zeros(lib.wvg_search_workspace_size(a.handle, nq, k), dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(qs).to(dev)
    oi, od, oc = (torch.zeros(sh, dtype=t, device=dev)
                  for sh, t in (((nq, k), torch.int64), ((nq, k), torch.float32), (nq, torch.int32)))

    def call():
        _lib.check(lib.wvg_search_device(a.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))

    call()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(4):  # the eager batch's result, then three replays
        torch.cuda.synchronize()
        _same((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)), want)
        for t in (oi, od, oc):
            t.zero_()
        ws.fill_(0xA5)  # whatever an earlier replay left behind
        g.replay()

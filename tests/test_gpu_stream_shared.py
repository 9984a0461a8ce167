"""The shared-row query stream (scan_f32_qshare_kernel, wvg_qshare.hip):
wvg_search_device_pipelined with two or more queries on an L2 / dot / cosine
corpus of d = 128 or 768 reads each row once per pass and scores every query of
the pass against it.  Its results must be those of nq independent searches:
equal to the oracle and, bit for bit, to nq separate wvg_search_device calls.

Matrix: d x metric x nq x k over the 4017-row corpus of test_gpu_k1_matrix
(deleted ids 0, 63, 64, 4016).  nq crosses the query-group and pass boundaries
of every form of the kernel (16 / 8 / 4 / 2 queries per pass), k the
E = 1 | 2 | 4 list sizes.  Every call runs twice back to back without a sync in
between, so the upward and the downward walk are both checked.  The single-query
reference of a (d, metric, k) is computed once and shared by the nq cases.
"""
import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_L2
from weaviate_amd.device import Context, Corpus

from test_gpu_k1_matrix import Case, device_search
from test_gpu_parity import bits, check_topk

DIMS = (128, 768)
METRICS = (METRIC_L2, METRIC_DOT, METRIC_COSINE)
NQS = (2, 3, 4, 5, 16, 17, 33)
KS = (1, 10, 64, 65, 129, 256)
NQ_MAX = max(NQS)

_cases = {}    # (metric, d) -> Case with NQ_MAX queries
_singles = {}  # (metric, d, k) -> [(ids, dists, count)] of NQ_MAX single-query wvg_search_device calls


@pytest.fixture(scope="module")
def cases(ctx, orc):
    def get(metric, d):
        if (metric, d) not in _cases:
            _cases[(metric, d)] = Case(ctx, orc, metric, d, nq=NQ_MAX)
        return _cases[(metric, d)]

    yield get
    for cs in _cases.values():
        cs.c.destroy()
    _cases.clear()
    _singles.clear()


def singles(cs, k):
    """Every query of the case alone through wvg_search_device (scan_f32_kernel +
    merge_keys_kernel), each checked against the oracle once."""
    key = (cs.metric, cs.d, k)
    if key not in _singles:
        out = []
        for qi in range(NQ_MAX):
            ids, dists, counts = device_search(cs.c.lib, cs.c, cs.c.lib.wvg_search_device, cs.pq[[qi]], k, reps=1)[0]
            check_topk(cs.orc, ids[0], dists[0], counts[0], cs.all_d[qi], cs.ids, k, cs.valid)
            out.append((ids[0].copy(), dists[0].copy(), counts[0]))
        _singles[key] = out
    return _singles[key]


def same_as_singles(res, ref, nq):
    ids, dists, counts = res
    for qi in range(nq):
        assert counts[qi] == ref[qi][2], qi
        assert np.array_equal(ids[qi], ref[qi][0]), qi
        assert np.array_equal(bits(dists[qi]), bits(ref[qi][1])), qi


@pytest.mark.gpu
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_shared_rows_matrix(cases, metric, d, nq):
    cs = cases(metric, d)
    lib = cs.c.lib
    qsel = list(range(nq))
    for k in KS:
        ref = singles(cs, k)
        for res in device_search(lib, cs.c, lib.wvg_search_device_pipelined, cs.pq[qsel], k, reps=2):
            cs.check(res, qsel, k, cs.valid)   # the oracle
            same_as_singles(res, ref, nq)      # nq separate searches, bit for bit


def _oracle_check(orc, c, rows, qs, k, metric=METRIC_L2, id0=0, reps=2, counts=True):
    """wvg_search_device_pipelined twice back to back against the oracle; the results of the last call."""
    import torch

    lib = c.lib
    dev = torch.device("cuda:0")
    nq, n = len(qs), len(rows)
    ws = torch.zeros(lib.wvg_search_workspace_size(c.handle, nq, k), dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(np.ascontiguousarray(qs, dtype=np.float32)).to(dev)
    outs = []
    for _ in range(reps):
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oc = torch.full((nq,), 12345, dtype=torch.int32, device=dev)
        _lib.check(lib.wvg_search_device_pipelined(c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                                   oc.data_ptr() if counts else 0, ws.data_ptr(), ws.numel(),
                                                   torch.cuda.current_stream().cuda_stream))
        outs.append((oi, od, oc))
    torch.cuda.synchronize()
    all_ids = np.arange(id0, id0 + n, dtype=np.uint64)
    want = min(k, n)
    all_d = [orc.dist_all(metric, q, rows) for q in qs]
    res = None
    for oi, od, oc in outs:
        res = (oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32))
        for qi in range(nq):
            cnt = res[2][qi] if counts else want
            if not counts:
                assert res[2][qi] == 12345  # untouched
            check_topk(orc, res[0][qi], res[1][qi], cnt, all_d[qi], all_ids, k)
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 70])
def test_shared_rows_tiny_corpus(ctx, orc, n):
    """One and two tiles: most waves own nothing and publish empty lists."""
    d = 128
    rows = orc.synth_rows(11, 0, n, d, 0)
    qs = orc.synth_rows(12, 0, 3, d, 0)
    c = Corpus(ctx, KIND_F32, METRIC_L2, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        for k in (1, 10, 100):
            _oracle_check(orc, c, rows, qs, k)
    finally:
        c.destroy()


@pytest.mark.gpu
def test_shared_rows_id_base_null_counts_and_repeated_query(ctx, orc):
    n, d, k = 1000, 128, 10
    base = 64_000_000
    rows = orc.synth_rows(21, 0, n, d, 0)
    qs = orc.synth_rows(22, 0, 4, d, 0)
    qs[2] = qs[0]  # the same query twice in one batch
    c = Corpus(ctx, KIND_F32, METRIC_L2, d, n, id_base=base)
    try:
        c.upsert(np.arange(base, base + n, dtype=np.uint64), rows)
        ids, dists, _ = _oracle_check(orc, c, rows, qs, k, id0=base)
        assert ids.min() >= base
        assert np.array_equal(ids[0], ids[2]) and np.array_equal(bits(dists[0]), bits(dists[2]))
        _oracle_check(orc, c, rows, qs, k, id0=base, counts=False)  # d_counts NULL
    finally:
        c.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 100])
def test_shared_rows_exact_ties(ctx, orc, k):
    """Integer-valued rows: a few distinct distances, hundreds of rows tied at the k-th.
    The result is the oracle's lexicographic top-k (smallest ids among the ties)."""
    n, d = 3000, 128
    rng = np.random.default_rng(5)
    rows = np.zeros((n, d), np.float32)
    rows[:, :2] = rng.integers(0, 2, size=(n, 2)).astype(np.float32)  # four distinct rows
    qs = np.zeros((3, d), np.float32)
    qs[1, 0] = 1.0
    qs[2, :2] = 0.5
    c = Corpus(ctx, KIND_F32, METRIC_L2, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        all_d = orc.dist_all(METRIC_L2, qs[0], rows)
        kth = np.sort(all_d)[k - 1]
        assert (all_d == kth).sum() > 200
        _oracle_check(orc, c, rows, qs, k)
    finally:
        c.destroy()


@pytest.mark.gpu
def test_shared_rows_whole_grid_and_streaming_context(ctx, orc):
    """200,000 x 128, 16 queries: every scan workgroup (two per CU) and every merger runs.
    A cache_reuse = 0 context (one full scan per query) returns the same results."""
    n, d, nq = 200_000, 128, 16
    rows = orc.synth_rows(42, 0, n, d, 0)
    qs = orc.synth_rows(43, 0, nq, d, 0)
    all_d = [orc.dist_all(METRIC_L2, q, rows) for q in qs]
    all_ids = np.arange(n, dtype=np.uint64)
    c = Corpus(ctx, KIND_F32, METRIC_L2, d, n)
    cx = Context(0, cache_reuse=0)
    c0 = Corpus(cx, KIND_F32, METRIC_L2, d, n)
    try:
        c.fill_synthetic(42, n, 0)
        c0.fill_synthetic(42, n, 0)
        for k in (10, 100):
            shared = device_search(c.lib, c, c.lib.wvg_search_device_pipelined, qs, k, reps=2)
            for ids, dists, counts in shared:
                for qi in range(nq):
                    check_topk(orc, ids[qi], dists[qi], counts[qi], all_d[qi], all_ids, k)
            for ids, dists, counts in device_search(c0.lib, c0, c0.lib.wvg_search_device_pipelined, qs, k, reps=2):
                assert np.array_equal(ids, shared[0][0])
                assert np.array_equal(bits(dists), bits(shared[0][1]))
                assert np.array_equal(counts, shared[0][2])
    finally:
        c.destroy()
        c0.destroy()
        cx.close()

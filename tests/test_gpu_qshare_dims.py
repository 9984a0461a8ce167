"""The shared-row query stream at every fp32 dimension (scan_f32_qshare_dyn_kernel
and scan_f32_qshare_dyn_filt_kernel, wvg_qshare.hip): wvg_search_device_pipelined
with two or more queries on an L2 / dot / cosine corpus of any d >= 8 reads each
row once per pass of 4 queries (2 for k > 128).  The runtime-dimension form walks
d >> 5 blocks of 32 floats, then the tail of the AVX2 order: up to three 8-float
blocks into accumulator row 0 and, for d % 8 == 4, four scalar updates into the
sum the reduction adds last.  Results must be those of nq independent searches:
equal to the oracle and, bit for bit, to nq separate wvg_search_device calls.

wvg_search_device_pipelined_plan tells what a call will do; the first test pins
it for the new and the old routes.
"""
import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import (KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_L2, METRIC_MANHATTAN, ORDER_AVX256,
                               ORDER_AVX512)
from weaviate_amd.device import Context, Corpus

from test_gpu_k1_matrix import Case, device_search
from test_gpu_parity import bits, check_topk

# nb = d >> 5 in {0, 1, 2, 3, 6, 8, 12, 48} (even, odd: the block loop's unroll remainder), 0..3 leftover
# 8-float blocks, with and without the 4-float scalar tail
DIMS = (8, 12, 32, 36, 44, 60, 64, 96, 100, 200, 256, 384, 1536)
METRICS = (METRIC_L2, METRIC_DOT, METRIC_COSINE)
NQS = (2, 4, 5, 17)          # a short pass, an exact pass, pass boundaries for 4 and 2 queries per pass
KS = (1, 10, 65, 129, 256)   # E = 1 | 2 | 4
NQ_MAX = max(NQS)

_cases = {}    # (metric, d) -> Case with NQ_MAX queries
_singles = {}  # (metric, d, k) -> [(ids, dists, count)] of NQ_MAX single-query wvg_search_device calls


def _small_corpus(cx, metric, d, n=100):
    c = Corpus(cx, KIND_F32, metric, d, n)
    c.upsert(np.arange(n, dtype=np.uint64), np.random.default_rng(d).uniform(-1, 1, (n, d)).astype(np.float32))
    return c


def _plan(c, nq, k):
    sp = _lib.StreamPlan()
    _lib.check(c.lib.wvg_search_device_pipelined_plan(c.handle, nq, k, sp))
    got = (sp.shared_rows, sp.queries_per_pass, sp.passes, sp.seeded, sp.screened)
    assert c.search_device_plan(nq, k) == dict(zip(("shared_rows", "queries_per_pass", "passes", "seeded", "screened"), got))
    return got


@pytest.mark.gpu
def test_plan(ctx):
    made = []

    def corpus(cx, metric, d):
        made.append(_small_corpus(cx, metric, d))
        return made[-1]

    cx0 = Context(0, cache_reuse=0)
    try:
        c384 = corpus(ctx, METRIC_L2, 384)
        assert _plan(c384, 17, 10) == (1, 4, 5, 0, 0)
        assert _plan(c384, 17, 128) == (1, 4, 5, 0, 0)
        assert _plan(c384, 17, 129) == (1, 2, 9, 0, 0)
        assert _plan(c384, 4, 10) == (1, 4, 1, 0, 0)
        assert _plan(corpus(ctx, METRIC_COSINE, 36), 5, 10) == (1, 4, 2, 0, 0)
        assert _plan(corpus(ctx, METRIC_DOT, 768), 17, 129) == (1, 2, 9, 0, 0)
        c128 = corpus(ctx, METRIC_L2, 128)   # today's values: 16 / 8 / 4, seeded, screened for L2 k <= 64
        assert _plan(c128, 17, 10) == (1, 16, 2, 1, 1)
        assert _plan(c128, 17, 64) == (1, 16, 2, 1, 1)
        assert _plan(c128, 17, 65) == (1, 8, 3, 1, 0)
        assert _plan(c128, 17, 129) == (1, 4, 5, 1, 0)
        assert _plan(corpus(ctx, METRIC_DOT, 128), 17, 10) == (1, 16, 2, 1, 0)
        # one scan per query
        assert _plan(c384, 1, 10) == (0, 1, 1, 0, 0)
        assert _plan(corpus(ctx, METRIC_MANHATTAN, 384), 17, 10) == (0, 1, 17, 0, 0)
        assert _plan(corpus(ctx, METRIC_L2, 4), 17, 10) == (0, 1, 17, 0, 0)
        assert _plan(corpus(cx0, METRIC_L2, 384), 17, 10) == (0, 1, 17, 0, 0)
        ctx.set_distance_order(ORDER_AVX512)
        try:
            assert _plan(c384, 17, 10) == (0, 1, 17, 0, 0)
        finally:
            ctx.set_distance_order(ORDER_AVX256)
        assert _plan(c384, 17, 10) == (1, 4, 5, 0, 0)
    finally:
        for c in made:
            c.destroy()
        cx0.close()


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
    """Every query of the case alone through wvg_search_device, each checked against the oracle once."""
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
def test_dimension_matrix(cases, metric, d, nq):
    cs = cases(metric, d)
    lib = cs.c.lib
    assert cs.c.search_device_plan(nq, 10)["shared_rows"] == 1
    qsel = list(range(nq))
    for k in KS:
        ref = singles(cs, k)
        for res in device_search(lib, cs.c, lib.wvg_search_device_pipelined, cs.pq[qsel], k, reps=2):
            cs.check(res, qsel, k, cs.valid)   # the oracle
            same_as_singles(res, ref, nq)      # nq separate searches, bit for bit


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT])
def test_special_values_in_the_tails(ctx, metric):
    """d = 44: one block (elements 0..31), one 8-float block (32..39), a scalar tail (40..43).  NaN, +-inf,
    -0.0 and a denormal in each of the three parts of some rows and of one query; an all-zero row and an
    all-zero query (dot: the sum of signed zeros).  Bit for bit the results of separate searches."""
    n, d, nq, k = 200, 44, 5, 10
    rng = np.random.default_rng(44 + metric)
    rows = rng.uniform(-1, 1, (n, d)).astype(np.float32)
    qs = rng.uniform(-1, 1, (nq, d)).astype(np.float32)
    block, eight, tail = 5, 35, 41
    den = np.float32(1e-40)
    assert den != 0 and den < np.finfo(np.float32).tiny
    for i, pos in enumerate((block, eight, tail)):
        rows[10 + i, pos] = np.nan
        rows[20 + i, pos] = np.inf
        rows[30 + i, pos] = -np.inf
        rows[40 + i, pos] = -0.0
        rows[50 + i, pos] = den
        rows[60 + i, pos] = -den
    rows[70, [block, eight, tail]] = np.inf      # all three parts at once
    rows[71, [block, tail]] = [np.inf, -np.inf]
    rows[72, [eight, tail]] = [-0.0, den]
    rows[80] = 0.0
    rows[81] = -0.0
    rows[199, 40:] = [np.nan, np.inf, -0.0, den]  # the ragged last tile
    qs[1, [block, eight, tail]] = [-0.0, den, np.inf]
    qs[2, tail + 1] = np.nan
    qs[3] = 0.0
    qs[4, [block, eight, tail]] = [den, -np.inf, -0.0]
    c = Corpus(ctx, KIND_F32, metric, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        lib = c.lib
        assert c.search_device_plan(nq, k)["shared_rows"] == 1
        ref = [device_search(lib, c, lib.wvg_search_device, qs[[qi]], k, reps=1)[0] for qi in range(nq)]
        for ids, dists, counts in device_search(lib, c, lib.wvg_search_device_pipelined, qs, k, reps=2):
            for qi in range(nq):
                assert counts[qi] == ref[qi][2][0], qi
                assert np.array_equal(ids[qi], ref[qi][0][0]), qi
                assert np.array_equal(bits(dists[qi]), bits(ref[qi][1][0])), qi
    finally:
        c.destroy()


@pytest.mark.gpu
def test_many_tiles_per_wave_and_streaming_context(ctx, orc):
    """150,000 x 36 (2,344 tiles: with two workgroups of four waves per CU some waves own two or more).  A
    cache_reuse = 0 context (one full scan per query) returns the same arrays."""
    n, d, nq = 150_000, 36, 16
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
        assert c.search_device_plan(nq, 10)["shared_rows"] == 1 and c0.search_device_plan(nq, 10)["shared_rows"] == 0
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


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 70])
def test_tiny_corpus(ctx, orc, n):
    """One and two tiles: most waves own nothing and publish empty lists."""
    from test_gpu_stream_shared import _oracle_check

    d = 36
    rows = orc.synth_rows(11, 0, n, d, 0)
    qs = orc.synth_rows(12, 0, 3, d, 0)
    c = Corpus(ctx, KIND_F32, METRIC_L2, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        for k in (1, 10, 100):
            _oracle_check(orc, c, rows, qs, k)
    finally:
        c.destroy()


# ---- allow lists (scan_f32_qshare_dyn_filt_kernel) -----------------------------------------------

_fcorps = {}


@pytest.fixture(scope="module")
def fcorps(ctx, orc):
    from test_gpu_qshare_filter import DEAD, FCorp, N, make_lists

    def get(metric, d):
        if (metric, d) not in _fcorps:
            rows = orc.synth_rows(3000 + 7 * d + metric, 0, N, d, 0)
            qs = orc.synth_rows(4000 + 7 * d + metric, 0, NQ_MAX, d, 0)
            for k in (10, 129):
                make_lists(k, 100 + k)  # the lists' preconditions, before the first GPU call
            _fcorps[(metric, d)] = FCorp(ctx, orc, metric, rows, qs, DEAD)
        return _fcorps[(metric, d)]

    yield get
    for cp in _fcorps.values():
        cp.destroy()
    _fcorps.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [2, 5, 17])
@pytest.mark.parametrize("d", [36, 384])
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT])
def test_filtered(fcorps, metric, d, nq):
    from test_gpu_qshare_filter import two_calls

    cp = fcorps(metric, d)
    for k in (10, 129):
        cp.check_filtered(nq, k, two_calls(nq, k))


@pytest.mark.gpu
@pytest.mark.parametrize("window", ["inner", "before", "empty"])
@pytest.mark.parametrize("shape", [(METRIC_L2, 36, 10), (METRIC_DOT, 384, 129)])
def test_filtered_windows(fcorps, shape, window):
    from test_gpu_qshare_filter import BASE, UINT64_MAX, filtered_search, two_calls

    metric, d, k = shape
    cp = fcorps(metric, d)
    for nq in (5, 17):
        cp.check_filtered(nq, k, two_calls(nq, k), window)
    if window == "empty":
        ids, dists, counts = filtered_search(cp.c, cp.pq[:17], k, [np.zeros((17, 0), np.uint64)], BASE, 0)[0]
        assert np.all(counts == 0) and np.all(ids == UINT64_MAX) and np.all(np.isposinf(dists))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(METRIC_L2, 36, 10), (METRIC_DOT, 384, 129)])
def test_null_allow_is_the_unfiltered_call(fcorps, shape):
    from test_gpu_qshare_filter import BASE, TILES, filtered_search

    metric, d, k = shape
    cp = fcorps(metric, d)
    lib = cp.c.lib
    for nq in (1, 17):
        want = device_search(lib, cp.c, lib.wvg_search_device_pipelined, cp.pq[:nq], k, reps=2)
        got = filtered_search(cp.c, cp.pq[:nq], k, [None, None], BASE, TILES)
        for (wi, wd, wc), (gi, gd, gc) in zip(want, got):
            assert np.array_equal(wi, gi) and np.array_equal(bits(wd), bits(gd)) and np.array_equal(wc, gc)


@pytest.mark.gpu
def test_captured_launch_replays(cases):
    """One capture of a d = 384, nq = 5 call into a graph: the replay writes what the eager call wrote."""
    import torch

    cs = cases(METRIC_L2, 384)
    lib = cs.c.lib
    nq, k = 5, 10
    dev = torch.device("cuda:0")
    eager = device_search(lib, cs.c, lib.wvg_search_device_pipelined, cs.pq[:nq], k, reps=1)[0]
    ws = torch.zeros(lib.wvg_search_workspace_size(cs.c.handle, nq, k), dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(np.ascontiguousarray(cs.pq[:nq], dtype=np.float32)).to(dev)
    oi = torch.zeros((nq, k), dtype=torch.int64, device=dev)
    od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    oc = torch.zeros(nq, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(lib.wvg_search_device_pipelined(cs.c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                                   oc.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert int(oi.abs().sum()) == 0 and int(oc.sum()) == 0  # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(oi.cpu().numpy().view(np.uint64), eager[0])
    assert np.array_equal(bits(od.cpu().numpy()), bits(eager[1]))
    assert np.array_equal(oc.cpu().numpy().astype(np.uint32), eager[2])
    _lib.check(lib.wvg_search_device_check(cs.c.ctx.handle, ws.data_ptr(), torch.cuda.current_stream().cuda_stream))

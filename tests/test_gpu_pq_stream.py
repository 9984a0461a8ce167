"""The device query stream of PQ corpora: wvg_search_device_pipelined and
wvg_search_device_pipelined_filtered on a WVG_KIND_PQ corpus.

Two or more queries in a context with cache_reuse on, over a codebook of which at least two
LUTs fit one workgroup's LDS, run scan_pq_qshare_kernel<E, ROT, Q, FILT, PLAIN>
(wvg_pq_qshare.hip): grid (row ranges, passes), pass p scores queries [p Q, min(nq, (p + 1) Q))
against every 64-row tile of its range, the tile loaded once and every (row, segment) looked up
once for the Q queries in an LDS image that keeps their LUT entries side by side; then
launch_merge_lists.  Q = 4 where four LUTs fit (m <= 32 at ks = 256; the rotated form at m = 32,
ks = 256), 2 up to m = 64; one query, cache_reuse = 0 or a larger codebook (m = 96) is
wvg_search_device's route (with allow lists: one K8 launch per query and one merge).
wvg_search_device_pipelined_plan tells which; Q is read from it.

Per query the sum is the reference's sequential fp32 sum in segment order from float32(0), then
Wrap (CH/product_quantization.go:85-104, 352-361), so the result must be bit for bit
wvg_search_device's for the same queries (itself checked against adc_all, the K8 matrix's
reference), and with allow lists bit for bit nq host calls wvg_search(c, q_i, 1, k, allow_i).
Codes are loaded as given (upsert_codes).
"""
import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import KIND_BQ, KIND_F32, KIND_PQ, METRIC_COSINE, METRIC_DOT, METRIC_L2
from weaviate_amd.device import Context, Corpus, allow_window

from test_gpu_bq_stream import F_BASE, F_STRIDE, _check_filtered, _filter_lists, padded, plan, same
from test_gpu_k1_matrix import device_search
from test_gpu_parity import check_topk
from test_gpu_pq_k8_matrix import N_PIPE, ORC, _all_d, _centers, _corpus, _near, _queries, adc_all
from test_gpu_qshare_filter import filtered_search

pytestmark = pytest.mark.gpu

UINT64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
N = 4000 + 17  # ragged against the 64-row tile (the filtered helpers of the BQ stream use the same N)
DEAD = [0, 63, 64, N - 1]
NQ_MAX = 11  # 2 Q + 3 at Q = 4
KS = [1, 10, 65, 129, 256]  # E = 1, 2, 4
#         m   ks   ds  Q
SHAPES = [(8, 256, 4, 4),     # generic form, m < 16: the s < m guard
          (16, 256, 2, 4),    # one full chunk
          (20, 256, 2, 4),    # a partial second chunk
          (32, 256, 4, 4),    # the rotated form
          (32, 255, 4, 4),    # rotated storage through the generic form
          (32, 16, 2, 4),
          (64, 256, 2, 2),    # two LUTs fill LDS
          (96, 256, 4, 1)]    # Weaviate's 384-d default: no shared scan
CASES = [(m, ks, ds, q, METRIC_L2) for m, ks, ds, q in SHAPES]
CASES += [(m, ks, ds, q, metric) for m, ks, ds, q in SHAPES if (m, ks) in ((32, 256), (64, 256))
          for metric in (METRIC_DOT, METRIC_COSINE)]


def q_of(c, k):
    return c.search_device_plan(2, k)["queries_per_pass"]


def _codes(m, ks, n=N):
    codes = np.random.default_rng(7000 + 1000 * m + ks).integers(0, ks, (n, m), dtype=np.uint8)
    if n >= 640:
        codes[576:640] = codes[576]  # a tile of identical rows (ties)
    return codes


class Ref:
    """One (m, ks, ds, metric): the corpus, NQ_MAX queries as the device routes take them (normalized for
    cosine) and adc_all's distances, made once and never modified; per k the batched wvg_search_device
    results, each query checked against adc_all."""

    def __init__(self, cx, orc, m, ks, ds, metric, id_base=0):
        self.orc, self.metric = orc, metric
        self.centers = _centers(orc, 7100 + m + ks, m, ks, ds)
        self.codes = _codes(m, ks)
        self.raw = _queries(orc, 7101 + m + ks, NQ_MAX, m * ds)
        self.pq = np.stack([orc.normalize(q) for q in self.raw]) if metric == METRIC_COSINE else self.raw
        self.valid = np.ones(N, bool)
        self.valid[DEAD] = False
        self.c = Corpus(cx, KIND_PQ, metric, m * ds, N, id_base=id_base)
        self.c.set_codebook(self.centers)
        self.c.upsert_codes(id_base + np.arange(N, dtype=np.uint64), self.codes)
        self.c.delete(id_base + np.array(DEAD, np.uint64))
        self._dev, self._host, self._near = {}, {}, None

    def device(self, k):
        if k not in self._dev:
            lib = self.c.lib
            res = device_search(lib, self.c, lib.wvg_search_device, self.pq, k, reps=1)[0]
            if self._near is None:
                self._near = [_near(d, self.valid, 256) for d in _all_d(self.orc, self.metric, self.raw, self.centers, self.codes)]
            for qi, (d, i) in enumerate(self._near):
                check_topk(self.orc, res[0][qi], res[1][qi], res[2][qi], d, i, k)
            padded(res)
            self._dev[k] = res
        return self._dev[k]

    def host(self, qi, k, mask):
        """wvg_search(c, q_i, 1, k, allow_i): the list as a bitmap over global docIDs (the BQ stream's FRef)."""
        from weaviate_amd.device import allow_bitmap

        key = (qi, k, mask.tobytes())
        if key not in self._host:
            words = allow_bitmap(F_BASE + np.flatnonzero(mask).astype(np.uint64), F_BASE + N)
            self._host[key] = self.c.search(self.raw[[qi]], k, allow=words)
        return self._host[key]


_refs = {}


@pytest.fixture(scope="module")
def refs(ctx, orc):
    def get(m, ks, ds, metric, id_base=0):
        key = (m, ks, ds, metric, id_base)
        if key not in _refs:
            _refs[key] = Ref(ctx, orc, m, ks, ds, metric, id_base)
        return _refs[key]

    yield get
    for r in _refs.values():
        r.c.destroy()
    _refs.clear()


def _pipelined(c, qs, k, reps=2):
    return device_search(c.lib, c, c.lib.wvg_search_device_pipelined, qs, k, reps=reps)


# ---- 1. the matrix ---------------------------------------------------------------------------------
@pytest.mark.parametrize("m,ks,ds,q,metric", CASES)
def test_matrix(refs, m, ks, ds, q, metric):
    r = refs(m, ks, ds, metric)
    for k in KS:
        want = r.device(k)  # adc_all's lexicographic top-k, through wvg_search_device
        assert q_of(r.c, k) == q
        for nq in sorted({2, max(q, 2), q + 1, 2 * q + 3}):
            if q >= 2:
                assert plan(r.c, nq, k) == (1, q, (nq + q - 1) // q, 0, 0)
            else:
                assert plan(r.c, nq, k) == (0, 1, nq, 0, 0)
            for got in _pipelined(r.c, r.pq[:nq], k):  # two calls in a row: both directions
                same(got, want, nq)


# ---- 2. special values -------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT])
@pytest.mark.parametrize("m,ds", [(32, 4), (16, 2)])
def test_special_values(ctx, orc, m, ds, metric):
    """LUT entries and sums that are +-inf, NaN or zero (a dot distance of -0.0): the shared scan's sums
    must be the single-query kernels' bit for bit, whatever lands in the other queries' lanes of an entry."""
    ks = 256
    centers = _centers(orc, 7200 + m, m, ks, ds).copy()
    centers[0, 5] = np.inf
    centers[1, 6] = -np.inf
    centers[2, 7, 0] = np.nan
    centers[3, 8] = 3e19        # squares and products overflow
    centers[4, 9] = -3e19
    centers[:, 11] = 0.0        # rows of code 11 everywhere: sum +0.0, a dot distance of -0.0
    centers[5, 12] = -0.0
    codes = _codes(m, ks).copy()
    codes[100:110] = 11
    codes[200:300, 0] = 5
    codes[300:400, 1] = 6
    codes[400:500, 2] = 7
    codes[500:600, 3] = 8
    codes[600:700, 4] = 9
    codes[650:750, 3] = 8       # +inf + -inf
    qs = _queries(orc, 7201 + m, NQ_MAX, m * ds).copy()
    qs[1, :ds] = 0.0
    qs[2] = 0.0                 # every LUT entry of this query is zero for dot
    qs[3, ds] = 3e19
    qs[3, :ds] = 1.0            # segment 0 against the +inf centroid: +inf for L2 and for dot
    d3 = adc_all(ORC[metric], orc.pq_lut(ORC[metric], qs[3], centers), codes)
    assert np.isnan(d3).any() and np.isinf(d3).any()  # the inputs do what they are there for
    c = _corpus(ctx, metric, centers, codes, np.array(DEAD, np.uint64))
    try:
        lib = c.lib
        for k in (10, 129):
            q = q_of(c, k)
            assert q == 4
            want = device_search(lib, c, lib.wvg_search_device, qs, k, reps=1)[0]
            if metric == METRIC_DOT:  # the all-zero query: rows of code 11 are at -0.0
                assert (want[1][2].view(np.uint32) == 0x80000000).any()
            for nq in (2, 2 * q + 3):
                for got in _pipelined(c, qs[:nq], k):
                    same(got, want, nq)
    finally:
        c.destroy()


# ---- 3. allow lists --------------------------------------------------------------------------------
@pytest.mark.parametrize("m,ks,ds,q", [(32, 256, 4, 4), (32, 255, 4, 4), (64, 256, 2, 2), (96, 256, 4, 1)])
def test_filtered(refs, m, ks, ds, q):
    r = refs(m, ks, ds, METRIC_L2, F_BASE)
    for k in (10, 65, 256):
        assert q_of(r.c, k) == q
        for nq in sorted({2, q + 1, 2 * q + 3}):
            _check_filtered(r, nq, k)
    _check_filtered(r, 1, 10)  # one query: K8 with its window


def test_filtered_edges(refs):
    r = refs(32, 256, 4, METRIC_L2, F_BASE)
    lib = r.c.lib
    k = 10
    nq = 2 * q_of(r.c, k) + 1
    # allow_stride = 0: every result empty
    ids, dists, counts = filtered_search(r.c, r.pq[:nq], k, [np.zeros((nq, 0), np.uint64)], 0, 0)[0]
    assert np.all(counts == 0) and np.all(ids == UINT64_MAX) and np.all(np.isposinf(dists))
    # d_allow = NULL: the unfiltered call
    for n in (1, nq):
        want = device_search(lib, r.c, lib.wvg_search_device_pipelined, r.pq[:n], k, reps=2)
        got = filtered_search(r.c, r.pq[:n], k, [None, None], 0, F_STRIDE)
        for w, g in zip(want, got):
            same(g, w)
    # a window that does not begin on a word: invalid, nothing launched
    rcs = []
    words = np.full((nq, F_STRIDE), UINT64_MAX, np.uint64)
    ids, dists, counts = filtered_search(r.c, r.pq[:nq], k, [words], 32, F_STRIDE, fn=rcs.append)[0]
    assert rcs == [_lib.WVG_ERR_INVALID]
    assert np.all(ids == np.uint64(7)) and np.all(dists == -7.0) and np.all(counts == 77)


# ---- 4. small and degenerate corpora ---------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 100])
def test_small_corpus(ctx, orc, n):
    """Most waves own no tile and leave empty lists; k above the live count."""
    m, ks, ds = 32, 256, 4
    centers = _centers(orc, 7300, m, ks, ds)
    codes = _codes(m, ks, n)
    c = _corpus(ctx, METRIC_L2, centers, codes, np.zeros(0, np.uint64))
    try:
        nq = 2 * q_of(c, 10) + 3
        qs = _queries(orc, 7301, nq, m * ds)
        near = [_near(d, np.ones(n, bool), 256) for d in _all_d(orc, METRIC_L2, qs, centers, codes)]
        for k in (1, 10, 200):
            assert plan(c, nq, k)[0] == 1
            for res in _pipelined(c, qs, k):
                padded(res)
                for qi in range(nq):
                    assert res[2][qi] == min(k, n)
                    check_topk(orc, res[0][qi], res[1][qi], res[2][qi], near[qi][0], near[qi][1], k)
    finally:
        c.destroy()


def test_degenerate_corpora(ctx, orc):
    m, ks, ds = 32, 256, 4
    nq, k = 11, 10
    centers = _centers(orc, 7310, m, ks, ds)
    qs = _queries(orc, 7311, nq, m * ds)
    for cap in (0, 640):  # empty corpus
        c = Corpus(ctx, KIND_PQ, METRIC_L2, m * ds, cap, id_base=64)
        try:
            c.set_codebook(centers)
            assert plan(c, nq, k) == (0, 1, 0, 0, 0)
            for ids, dists, counts in _pipelined(c, qs, k):
                assert np.all(counts == 0) and np.all(ids == UINT64_MAX) and np.all(np.isposinf(dists))
        finally:
            c.destroy()
    n = 200
    codes = np.tile(_codes(m, ks, 1), (n, 1))  # every row the same code
    dead = np.array([0, 2, 64], np.uint64)
    c = _corpus(ctx, METRIC_L2, centers, codes, dead)
    try:
        live = np.setdiff1d(np.arange(n, dtype=np.uint64), dead)
        for kk in (10, 129):  # ties resolved by id
            for ids, dists, counts in _pipelined(c, qs, kk):
                assert np.all(counts == kk)
                for qi in range(nq):
                    assert np.array_equal(ids[qi], live[:kk]) and len(set(dists[qi].view(np.uint32).tolist())) == 1
        for res in _pipelined(c, qs, 256):  # k above the live count
            ids, dists, counts = res
            assert np.all(counts == len(live))
            padded(res)
            for qi in range(nq):
                assert np.array_equal(ids[qi][:len(live)], live)
        c.delete(live)  # every row deleted
        for ids, dists, counts in _pipelined(c, qs, k):
            assert np.all(counts == 0) and np.all(ids == UINT64_MAX) and np.all(np.isposinf(dists))
    finally:
        c.destroy()


# ---- 5. many tiles per wave ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(ctx, orc):
    """N_PIPE rows at (32, 256) and (64, 256) with dead runs at the start, in the middle and at the end of a
    wave's range (the chain of live tiles of the rotated form has to step over them)."""
    rng = np.random.default_rng(7400)
    full = N_PIPE // 64
    deleted = np.unique(np.concatenate([np.arange(64 * 10, 64 * 40), np.arange(64 * 2000, 64 * 2300),
                                        np.arange(64 * (full - 3), 64 * full),
                                        rng.choice(N_PIPE, 3000, replace=False)])).astype(np.uint64)
    out = {}
    for m, ds in ((32, 4), (64, 2)):
        centers = _centers(orc, 7401 + m, m, 256, ds)
        codes = np.random.default_rng(7402 + m).integers(0, 256, (N_PIPE, m), dtype=np.uint8)
        codes[6400:6464] = codes[6400]
        out[m] = (_corpus(ctx, METRIC_L2, centers, codes, deleted), m * ds)
    yield out
    for c, _ in out.values():
        c.destroy()


@pytest.mark.parametrize("m", [32, 64])
def test_many_tiles_per_wave(big, orc, m):
    c, d = big[m]
    lib = c.lib
    nq = 2 * q_of(c, 10) + 1
    qs = _queries(orc, 7410 + m, nq, d)
    for k in (200, 10):
        assert plan(c, nq, k)[0] == 1
        want = device_search(lib, c, lib.wvg_search_device, qs, k, reps=1)[0]
        assert np.all(want[2] == k)
        for got in _pipelined(c, qs, k):
            same(got, want)


# ---- 6. one workspace, mixed calls, no sync between them ----------------------------------------------
def test_mixed_calls_on_one_workspace(ctx, orc, big, refs):
    import torch

    pqc, pd = big[32]
    lib = pqc.lib
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    nqp = 2 * q_of(pqc, 10) + 1
    fr = refs(32, 256, 4, METRIC_L2, F_BASE)
    f = Corpus(ctx, KIND_F32, METRIC_L2, 36, 3000)
    b = Corpus(ctx, KIND_BQ, METRIC_L2, 768, 3000)
    try:
        f.fill_synthetic(7, 3000, 0)
        b.fill_synthetic(8, 3000, 0)
        qp = _queries(orc, 7500, nqp, pd)
        qf = orc.synth_rows(7501, 0, 6, 36, 0)
        qb = orc.synth_rows(7502, 0, 9, 768, 0)
        lists = _filter_lists(nqp)
        words = allow_window([F_BASE + np.flatnonzero(m).astype(np.uint64) for m in lists], 0, F_STRIDE)
        # the references, each on a workspace of its own
        want = [device_search(lib, pqc, lib.wvg_search_device, qp, 200, reps=1)[0],
                device_search(lib, f, lib.wvg_search_device, qf, 10, reps=1)[0],
                filtered_search(fr.c, fr.pq[:nqp], 10, [words], 0, F_STRIDE)[0],
                device_search(lib, b, lib.wvg_search_device, qb, 10, reps=1)[0]]
        calls = [(pqc, qp, 200, None), (f, qf, 10, None), (fr.c, fr.pq[:nqp], 10, words), (b, qb, 10, None)]
        size = max(lib.wvg_search_workspace_size(c.handle, len(qs), k) for c, qs, k, _ in calls)
        ws = torch.zeros(size, dtype=torch.uint8, device=dev)
        outs, keep = [], []
        for c, qs, k, w in calls:
            nq = len(qs)
            tq = torch.from_numpy(np.ascontiguousarray(qs, dtype=np.float32)).to(dev)
            oi = torch.full((nq, k), 7, dtype=torch.int64, device=dev)
            od = torch.full((nq, k), -7.0, dtype=torch.float32, device=dev)
            oc = torch.full((nq,), 77, dtype=torch.int32, device=dev)
            keep.append(tq)
            if w is None:
                _lib.check(lib.wvg_search_device_pipelined(c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                                           oc.data_ptr(), ws.data_ptr(), ws.numel(), s))
            else:
                tw = torch.from_numpy(w.view(np.int64)).to(dev)
                keep.append(tw)
                c.search_device_pipelined(tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), ws.data_ptr(),
                                          ws.numel(), s, tw.data_ptr(), F_STRIDE, 0)
            outs.append((oi, od, oc))
        _lib.check(lib.wvg_search_device_check(ctx.handle, ws.data_ptr(), s))
        assert int(ws[:256].cpu().numpy().view(np.uint32).sum()) == 0  # the status block and its counters stay zero
        for (oi, od, oc), w in zip(outs, want):
            same((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)), w)
    finally:
        f.destroy()
        b.destroy()


# ---- 7. graph capture ------------------------------------------------------------------------------
def test_captured_calls_replay(refs):
    """One unfiltered and one filtered call captured on one stream; the queries and lists are overwritten in
    place before each replay, and the replays write what uncaptured calls with those inputs write."""
    import torch

    r = refs(32, 256, 4, METRIC_L2, F_BASE)
    lib = r.c.lib
    k = 10
    nq = 2 * q_of(r.c, k) + 1
    dev = torch.device("cuda:0")
    sets = []
    for sh in (0, 1, 2):  # the inputs at capture time, then those of the two replays
        qs = np.ascontiguousarray(np.roll(r.pq, -sh, axis=0)[:nq], dtype=np.float32)
        lists = _filter_lists(nq + sh)[sh:]
        words = allow_window([F_BASE + np.flatnonzero(m).astype(np.uint64) for m in lists], 0, F_STRIDE)
        sets.append((qs, words))
    eager = [(device_search(lib, r.c, lib.wvg_search_device_pipelined, qs, k, reps=1)[0],
              filtered_search(r.c, qs, k, [words], 0, F_STRIDE)[0]) for qs, words in sets[1:]]
    ws = torch.zeros(lib.wvg_search_workspace_size(r.c.handle, nq, k), dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(sets[0][0]).to(dev)
    tw = torch.from_numpy(sets[0][1].view(np.int64)).to(dev)
    out = [(torch.zeros((nq, k), dtype=torch.int64, device=dev), torch.zeros((nq, k), dtype=torch.float32, device=dev),
            torch.zeros(nq, dtype=torch.int32, device=dev)) for _ in range(2)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = torch.cuda.current_stream().cuda_stream
        (oi, od, oc), (fi, fd, fc) = out
        _lib.check(lib.wvg_search_device_pipelined(r.c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                                   oc.data_ptr(), ws.data_ptr(), ws.numel(), s))
        _lib.check(lib.wvg_search_device_pipelined_filtered(r.c.handle, tq.data_ptr(), nq, k, tw.data_ptr(), F_STRIDE, 0,
                                                            fi.data_ptr(), fd.data_ptr(), fc.data_ptr(), ws.data_ptr(),
                                                            ws.numel(), s))
    torch.cuda.synchronize()
    assert int(out[0][0].abs().sum()) == 0 and int(out[1][2].sum()) == 0  # captured, not run
    for (qs, words), (want_u, want_f) in zip(sets[1:], eager):
        tq.copy_(torch.from_numpy(qs))
        tw.copy_(torch.from_numpy(words.view(np.int64)))
        g.replay()
        torch.cuda.synchronize()
        for (ti, td, tc), want in zip(out, (want_u, want_f)):
            same((ti.cpu().numpy().view(np.uint64), td.cpu().numpy(), tc.cpu().numpy().astype(np.uint32)), want)
    _lib.check(lib.wvg_search_device_check(r.c.ctx.handle, ws.data_ptr(), torch.cuda.current_stream().cuda_stream))


# ---- 8. plan and errors ----------------------------------------------------------------------------
def test_plan_and_errors(ctx, orc, refs, big):
    import torch

    r = refs(32, 256, 4, METRIC_L2)
    r64 = refs(64, 256, 2, METRIC_L2)
    r96 = refs(96, 256, 4, METRIC_L2)
    lib = r.c.lib
    dev = torch.device("cuda:0")
    for rr, q in ((r, 4), (r64, 2)):
        for k in (10, 65, 129, 256):
            assert q_of(rr.c, k) == q
            for nq in (2, q, q + 1, 100):
                assert plan(rr.c, nq, k) == (1, q, -(-nq // q), 0, 0)
            assert plan(rr.c, 1, k) == (0, 1, 1, 0, 0)
    for k in (10, 256):
        for nq in (1, 2, 5, 100):
            assert plan(r96.c, nq, k) == (0, 1, nq, 0, 0)
    assert plan(r.c, 0, 10) == (0, 1, 0, 0, 0) and plan(r.c, 5, 0) == (0, 1, 0, 0, 0)
    # cache_reuse = 0: one full scan per query, the same arrays
    cx0 = Context(0, cache_reuse=0)
    c0 = Corpus(cx0, KIND_PQ, METRIC_L2, 128, N)
    bare = Corpus(ctx, KIND_PQ, METRIC_L2, 64, 640)  # no codebook
    try:
        c0.set_codebook(r.centers)
        c0.upsert_codes(np.arange(N, dtype=np.uint64), r.codes)
        c0.delete(np.array(DEAD, np.uint64))
        nq = NQ_MAX
        assert plan(c0, nq, 10) == (0, 1, nq, 0, 0) and plan(c0, 1, 10) == (0, 1, 1, 0, 0)
        for k in (10, 200):
            want = device_search(lib, r.c, lib.wvg_search_device, r.pq, k, reps=1)[0]
            for got in _pipelined(c0, r.pq[:nq], k):
                same(got, want, nq)
        # a workspace one byte short of the call's layout.  The size is the largest of the layouts; the largest
        # is the per-query launches' (a single query's K8 grid has at least as many row ranges as the shared
        # scan): a filtered call on the m = 96 corpus, and wvg_search_device's own for one query.  The shared
        # scan's layout is smaller, so the size also serves it (the large corpus, nq = 9, k = 200).
        s = torch.cuda.current_stream().cuda_stream
        for c, n, k, d, filt in ((r96.c, 5, 10, 384, True), (r.c, 1, 10, 128, False)):
            size = lib.wvg_search_workspace_size(c.handle, n, k)
            ws = torch.zeros(size, dtype=torch.uint8, device=dev)
            tq = torch.zeros((n, d), dtype=torch.float32, device=dev)
            tw = torch.full((n, 70), -1, dtype=torch.int64, device=dev)
            oi = torch.zeros((n, k), dtype=torch.int64, device=dev)
            od = torch.zeros((n, k), dtype=torch.float32, device=dev)
            oc = torch.zeros(n, dtype=torch.int32, device=dev)

            def call(nbytes):
                if filt:
                    return lib.wvg_search_device_pipelined_filtered(c.handle, tq.data_ptr(), n, k, tw.data_ptr(), 70, 0,
                                                                    oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                                                    ws.data_ptr(), nbytes, s)
                return lib.wvg_search_device_pipelined(c.handle, tq.data_ptr(), n, k, oi.data_ptr(), od.data_ptr(),
                                                       oc.data_ptr(), ws.data_ptr(), nbytes, s)

            assert call(size - 1) == _lib.WVG_ERR_INVALID
            assert call(size) == _lib.WVG_OK
            torch.cuda.synchronize()
        bigc, bd = big[32]
        assert plan(bigc, 9, 200)[0] == 1
        assert lib.wvg_search_workspace_size(bigc.handle, 9, 200) >= lib.wvg_search_workspace_size(bigc.handle, 1, 200)
        # k = 257 and a PQ corpus without a codebook are unsupported: the plan, the call, the filtered call
        sp = _lib.StreamPlan()
        assert lib.wvg_search_device_pipelined_plan(bare.handle, 5, 10, sp) == _lib.WVG_ERR_UNSUPPORTED
        assert lib.wvg_search_device_pipelined_plan(r.c.handle, 5, 257, sp) == _lib.WVG_ERR_UNSUPPORTED
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
        tq = torch.zeros((5, 128), dtype=torch.float32, device=dev)
        tw = torch.zeros((5, 4), dtype=torch.int64, device=dev)
        oi = torch.zeros((5, 257), dtype=torch.int64, device=dev)
        od = torch.zeros((5, 257), dtype=torch.float32, device=dev)
        oc = torch.zeros(5, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        for c, k in ((bare, 10), (r.c, 257)):
            rc = lib.wvg_search_device_pipelined(c.handle, tq.data_ptr(), 5, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), s)
            assert rc == _lib.WVG_ERR_UNSUPPORTED
            rc = lib.wvg_search_device_pipelined_filtered(c.handle, tq.data_ptr(), 5, k, tw.data_ptr(), 4, 0, oi.data_ptr(),
                                                          od.data_ptr(), oc.data_ptr(), ws.data_ptr(), ws.numel(), s)
            assert rc == _lib.WVG_ERR_UNSUPPORTED
        # wvg_search_device keeps its own answer for a corpus without a codebook
        rc = lib.wvg_search_device(bare.handle, tq.data_ptr(), 5, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                   ws.data_ptr(), ws.numel(), s)
        assert rc == _lib.WVG_ERR_INVALID
    finally:
        bare.destroy()
        c0.destroy()
        cx0.close()


def test_python_wrappers_take_pq(refs):
    """ShardedFlatIndex.search_device(pipelined=True) with and without allow words on a PQ corpus."""
    import torch

    from weaviate_amd.shard import ShardedFlatIndex

    r = refs(32, 256, 4, METRIC_L2, F_BASE)
    lib = r.c.lib
    k, nq = 10, 11
    dev = torch.device("cuda:0")
    lists = _filter_lists(nq)
    words = allow_window([F_BASE + np.flatnonzero(m).astype(np.uint64) for m in lists], 0, F_STRIDE)
    want_u = device_search(lib, r.c, lib.wvg_search_device_pipelined, r.pq[:nq], k, reps=1)[0]
    want_f = filtered_search(r.c, r.pq[:nq], k, [words], 0, F_STRIDE)[0]
    tq = torch.from_numpy(np.ascontiguousarray(r.pq[:nq])).to(dev)
    tw = torch.from_numpy(words.view(np.int64)).to(dev)
    idx = ShardedFlatIndex(r.c.ctx, r.c)
    for want, kw in ((want_u, {}), (want_f, {"allow": tw, "allow_first_id": 0})):
        ids, dists, counts = idx.search_device(tq, k, pipelined=True, **kw)
        torch.cuda.synchronize()
        same((ids.cpu().numpy().view(np.uint64), dists.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)), want)

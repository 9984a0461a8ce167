"""The device query stream of BQ corpora: wvg_search_device_pipelined and
wvg_search_device_pipelined_filtered on a WVG_KIND_BQ corpus.

Two or more queries in a context with cache_reuse on run scan_bq_qshare_kernel
<E, NCH, Q, FILT, PLAIN> (wvg_bq_qshare.hip): grid (row ranges, passes), pass p scores
queries [p Q, min(nq, (p + 1) Q)) against every 64-row tile of its range, the tile
loaded once; then launch_merge_lists.  One query, or cache_reuse = 0, is
wvg_search_device's route (with allow lists: one K5 launch per query and one merge).
wvg_search_device_pipelined_plan tells which; Q is read from it.

Per query the result must be the (Hamming distance, docID)-lexicographic top-k: the
oracle's over bq_dist_all, bit for bit wvg_search_device's for the same queries, and
with allow lists bit for bit nq host calls wvg_search(c, q_i, 1, k, allow_i).

The rows are the K5 matrix's (tests/test_gpu_bq_k5_matrix.py): N = 4017, ragged against
the tile, dead rows 0, 63, 64 and N - 1, the all-negative, all-positive, +-0 and
non-finite rows; the queries are its eight (all-negative, all-positive and non-finite
among them) and random ones up to 2 Q + 3.
"""
import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import KIND_BQ, KIND_F32, KIND_PQ, METRIC_COSINE, METRIC_L2
from weaviate_amd.device import Context, Corpus, allow_bitmap, allow_window

from test_gpu_bq_k5_matrix import DEAD, KS, N, Q_NEG, ROW_NEG, make_queries, make_rows
from test_gpu_k1_matrix import allow_ids, device_search
from test_gpu_parity import bits, check_topk, prep_query, stored_rows
from test_gpu_qshare_filter import filtered_search

pytestmark = pytest.mark.gpu

UINT64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
NQ_MAX = 35  # 2 Q + 3 for Q up to 16 (asserted where Q is read)
#        d      chunks kernel
CASES = [(METRIC_L2, 64),      # 1   NCH 1, one word: the upper half of the only chunk is padding
         (METRIC_L2, 130),     # 2   generic, odd word count
         (METRIC_COSINE, 130),
         (METRIC_L2, 300),     # 3   generic
         (METRIC_L2, 768),     # 6   NCH 6
         (METRIC_L2, 1440),    # 12  NCH 12, odd word count
         (METRIC_L2, 1536),    # 12  NCH 12
         (METRIC_COSINE, 1536),
         (METRIC_L2, 3072)]    # 24  generic, long loop


def plan(c, nq, k):
    sp = c.search_device_plan(nq, k)
    return (sp["shared_rows"], sp["queries_per_pass"], sp["passes"], sp["seeded"], sp["screened"])


def q_of(c, k):
    q = c.search_device_plan(2, k)["queries_per_pass"]
    assert 2 <= q and 2 * q + 3 <= NQ_MAX
    return q


def same(got, want, nq=None):
    """Two (ids, dists, counts): ids, distance bits, counts and padding equal (the first nq queries of `want`)."""
    gi, gd, gc = got
    wi, wd, wc = want
    nq = len(gi) if nq is None else nq
    assert len(gi) == nq
    assert np.array_equal(gc, wc[:nq])
    assert np.array_equal(gi, wi[:nq])
    assert np.array_equal(bits(gd), bits(wd[:nq]))


def padded(res):
    ids, dists, counts = res
    for i, cnt in enumerate(counts):
        assert np.all(ids[i][cnt:] == UINT64_MAX) and np.all(np.isposinf(dists[i][cnt:]))


class Ref:
    """One (metric, d): the corpus, NQ_MAX prepared queries and the oracle's distances, made once and
    never modified; per k the batched wvg_search_device results, each query checked against the oracle."""

    def __init__(self, cx, orc, metric, d):
        self.orc, self.metric, self.d = orc, metric, d
        rows = make_rows(orc, d)
        qs = np.concatenate([make_queries(orc, d), orc.synth_rows(5000 + 7 * d, 0, NQ_MAX - 8, d, 0)])
        self.codes = orc.bq_encode_rows(stored_rows(orc, metric, rows))
        self.pq = np.stack([prep_query(orc, metric, q) for q in qs])  # the device routes take these
        self.all_d = [orc.bq_dist_all(orc.bq_encode(q), self.codes) for q in self.pq]
        self.ids = np.arange(N, dtype=np.uint64)
        self.valid = np.ones(N, np.uint8)
        self.valid[DEAD] = 0
        self.c = Corpus(cx, KIND_BQ, metric, d, N)
        self.c.upsert(self.ids, rows)
        self.c.delete(np.array(DEAD, np.uint64))
        self._dev = {}

    def device(self, k):
        if k not in self._dev:
            lib = self.c.lib
            res = device_search(lib, self.c, lib.wvg_search_device, self.pq, k, reps=1)[0]
            for qi in range(NQ_MAX):
                check_topk(self.orc, res[0][qi], res[1][qi], res[2][qi], self.all_d[qi], self.ids, k, self.valid)
            assert res[0][Q_NEG][0] == ROW_NEG and bits(res[1][Q_NEG][0]) == 0  # distance 0, first
            padded(res)
            self._dev[k] = res
        return self._dev[k]


_refs = {}


@pytest.fixture(scope="module")
def refs(ctx, orc):
    def get(metric, d):
        if (metric, d) not in _refs:
            _refs[(metric, d)] = Ref(ctx, orc, metric, d)
        return _refs[(metric, d)]

    yield get
    for r in _refs.values():
        r.c.destroy()
    _refs.clear()


# ---- 1. the matrix ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nqi", [0, 1, 2, 3])  # nq = 2, Q, Q + 1, 2 Q + 3
@pytest.mark.parametrize("metric,d", CASES)
def test_matrix(refs, metric, d, nqi):
    r = refs(metric, d)
    lib = r.c.lib
    for k in KS:
        q = q_of(r.c, k)
        nq = (2, q, q + 1, 2 * q + 3)[nqi]
        assert plan(r.c, nq, k) == (1, q, (nq + q - 1) // q, 0, 0)
        want = r.device(k)  # the oracle's lexicographic top-k, through wvg_search_device
        for got in device_search(lib, r.c, lib.wvg_search_device_pipelined, r.pq[:nq], k, reps=2):  # both directions
            same(got, want, nq)


# ---- 2. allow lists --------------------------------------------------------------------------------
F_BASE = 640
F_TILES = (N + 63) // 64
F_STRIDE = F_BASE // 64 + F_TILES - 2  # the window begins at docID 0, before the corpus, and ends before its last two tiles


def _filter_lists(nq):
    """Row masks, list i % 5 for query i: all ones, the allow_ids pattern, all zeros, one id, only deleted rows."""
    pattern = np.zeros(N, bool)
    pattern[allow_ids(N).astype(np.int64)] = True
    one = np.zeros(N, bool)
    one[1234] = True
    dead = np.zeros(N, bool)
    dead[DEAD] = True
    kinds = [np.ones(N, bool), pattern, np.zeros(N, bool), one, dead]
    return [kinds[i % 5] for i in range(nq)]


class FRef:
    """One (metric, d) filtered corpus at id_base 640 with its host references."""

    def __init__(self, cx, orc, metric, d):
        self.metric, self.d = metric, d
        rows = make_rows(orc, d)
        self.raw = np.concatenate([make_queries(orc, d), orc.synth_rows(5000 + 7 * d, 0, NQ_MAX - 8, d, 0)])
        self.pq = np.stack([prep_query(orc, metric, q) for q in self.raw])
        self.c = Corpus(cx, KIND_BQ, metric, d, N, id_base=F_BASE)
        self.c.upsert(F_BASE + np.arange(N, dtype=np.uint64), rows)
        self.c.delete(F_BASE + np.array(DEAD, np.uint64))
        self._host = {}

    def host(self, qi, k, mask):
        """wvg_search(c, q_i, 1, k, allow_i): the list as a bitmap over global docIDs."""
        key = (qi, k, mask.tobytes())
        if key not in self._host:
            words = allow_bitmap(F_BASE + np.flatnonzero(mask).astype(np.uint64), F_BASE + N)
            self._host[key] = self.c.search(self.raw[[qi]], k, allow=words)
        return self._host[key]


_frefs = {}


@pytest.fixture(scope="module")
def frefs(ctx, orc):
    def get(metric, d):
        if (metric, d) not in _frefs:
            _frefs[(metric, d)] = FRef(ctx, orc, metric, d)
        return _frefs[(metric, d)]

    yield get
    for r in _frefs.values():
        r.c.destroy()
    _frefs.clear()


def _check_filtered(r, nq, k, shifts=(0, 2)):
    """Two filtered calls back to back (the second with the lists shifted) against nq host calls each."""
    inwin = np.arange(N) < (F_STRIDE - F_BASE // 64) * 64
    per_call = []
    for sh in shifts:
        lists = _filter_lists(nq + sh)[sh:]
        per_call.append(lists)
    refs_ = [[r.host(qi, k, lists[qi] & inwin) for qi in range(nq)] for lists in per_call]  # (these synchronize)
    words = [allow_window([F_BASE + np.flatnonzero(m).astype(np.uint64) for m in lists], 0, F_STRIDE) for lists in per_call]
    for w in words:
        w[:, :F_BASE // 64] = UINT64_MAX  # bits that name no row of the corpus must be ignored
    outs = filtered_search(r.c, r.pq[:nq], k, words, 0, F_STRIDE)
    for ci, (ids, dists, counts) in enumerate(outs):
        padded((ids, dists, counts))
        for qi in range(nq):
            ri, rd, rc = refs_[ci][qi]
            tag = (ci, qi, k)
            assert counts[qi] == rc[0], tag
            assert np.array_equal(ids[qi], ri[0]), tag
            assert np.array_equal(bits(dists[qi]), bits(rd[0])), tag
            eff = per_call[ci][qi] & inwin
            eff[DEAD] = False
            assert counts[qi] == min(k, int(eff.sum())), tag
            assert np.isin(ids[qi][:counts[qi]] - np.uint64(F_BASE), np.flatnonzero(eff)).all(), tag


@pytest.mark.parametrize("metric,d", [(METRIC_L2, 1536), (METRIC_COSINE, 130), (METRIC_L2, 768), (METRIC_L2, 64)])
def test_filtered(frefs, metric, d):
    r = frefs(metric, d)
    for k in (10, 65, 256):
        q = q_of(r.c, k)
        for nq in (2, q + 1, 2 * q + 3):
            _check_filtered(r, nq, k)
    _check_filtered(r, 1, 10)  # one query: K5 with its window


def test_filtered_edges(frefs):
    r = frefs(METRIC_L2, 1536)
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


# ---- 3. small and degenerate corpora ---------------------------------------------------------------
def _pipelined(c, qs, k, reps=2):
    return device_search(c.lib, c, c.lib.wvg_search_device_pipelined, qs, k, reps=reps)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100])
def test_small_corpus(ctx, orc, n):
    """Most waves own no tile and leave empty lists; k above the live count."""
    d = 1536
    rows = orc.synth_rows(11, 0, n, d, 0)
    codes = orc.bq_encode_rows(rows)
    c = Corpus(ctx, KIND_BQ, METRIC_L2, d, n)
    try:
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        nq = 2 * q_of(c, 10) + 3
        qs = orc.synth_rows(12, 0, nq, d, 0)
        all_d = [orc.bq_dist_all(orc.bq_encode(q), codes) for q in qs]
        ids_all = np.arange(n, dtype=np.uint64)
        for k in (1, 10, 200):
            assert plan(c, nq, k)[0] == 1
            for res in _pipelined(c, qs, k):
                padded(res)
                for qi in range(nq):
                    assert res[2][qi] == min(k, n)
                    check_topk(orc, res[0][qi], res[1][qi], res[2][qi], all_d[qi], ids_all, k)
    finally:
        c.destroy()


def test_degenerate_corpora(ctx, orc):
    d, nq, k = 768, 11, 10
    qs = orc.synth_rows(13, 0, nq, d, 0)
    for cap in (0, 640):  # empty corpus
        c = Corpus(ctx, KIND_BQ, METRIC_L2, d, cap, id_base=64)
        try:
            assert plan(c, nq, k) == (0, 1, 0, 0, 0)
            for ids, dists, counts in _pipelined(c, qs, k):
                assert np.all(counts == 0) and np.all(ids == UINT64_MAX) and np.all(np.isposinf(dists))
        finally:
            c.destroy()
    n = 200
    c = Corpus(ctx, KIND_BQ, METRIC_L2, d, n)
    try:
        # every row the same code: the k smallest live ids at one distance
        c.upsert(np.arange(n, dtype=np.uint64), np.tile(orc.synth_rows(14, 0, 1, d, 0), (n, 1)))
        c.delete(np.array([0, 2, 64], np.uint64))
        live = np.setdiff1d(np.arange(n, dtype=np.uint64), [0, 2, 64])
        for kk in (10, 129):
            for ids, dists, counts in _pipelined(c, qs, kk):
                assert np.all(counts == kk)
                for qi in range(nq):
                    assert np.array_equal(ids[qi], live[:kk]) and len(set(bits(dists[qi]).tolist())) == 1
        # k above the live count
        for res in _pipelined(c, qs, 256):
            ids, dists, counts = res
            assert np.all(counts == len(live))
            padded(res)
            for qi in range(nq):
                assert np.array_equal(ids[qi][:len(live)], live)
        # every row deleted
        c.delete(live)
        for ids, dists, counts in _pipelined(c, qs, k):
            assert np.all(counts == 0) and np.all(ids == UINT64_MAX) and np.all(np.isposinf(dists))
    finally:
        c.destroy()


# ---- 4. many tiles per wave ------------------------------------------------------------------------
BIG_N, BIG_D = 200_017, 1536


@pytest.fixture(scope="module")
def big(ctx):
    c = Corpus(ctx, KIND_BQ, METRIC_L2, BIG_D, BIG_N)
    c.fill_synthetic(42, BIG_N, 0)
    yield c
    c.destroy()


def test_many_tiles_per_wave(big, orc):
    """3,126 tiles: every wave of the two workgroups per CU walks two or more, prefetching the next."""
    lib = big.lib
    nq = 2 * q_of(big, 10) + 1
    qs = orc.synth_rows(43, 0, nq, BIG_D, 0)
    for k in (200, 10):
        assert plan(big, nq, k)[0] == 1
        want = device_search(lib, big, lib.wvg_search_device, qs, k, reps=1)[0]
        assert np.all(want[2] == k)
        for got in _pipelined(big, qs, k):
            same(got, want)


# ---- 5. one workspace, mixed calls, no sync between them ----------------------------------------------
def test_mixed_calls_on_one_workspace(ctx, orc, big, frefs):
    import torch

    lib = big.lib
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    q = q_of(big, 10)
    nqb = 2 * q + 1
    fr = frefs(METRIC_L2, 1536)
    fd, fn = 36, 3000
    f = Corpus(ctx, KIND_F32, METRIC_L2, fd, fn)
    try:
        f.fill_synthetic(7, fn, 0)
        qb = orc.synth_rows(44, 0, nqb, BIG_D, 0)
        qf = orc.synth_rows(45, 0, 6, fd, 0)
        lists = _filter_lists(nqb)
        words = allow_window([F_BASE + np.flatnonzero(m).astype(np.uint64) for m in lists], 0, F_STRIDE)
        # the references, each on a workspace of its own
        want = [device_search(lib, big, lib.wvg_search_device, qb[:5], 10, reps=1)[0],
                device_search(lib, f, lib.wvg_search_device, qf, 10, reps=1)[0],
                device_search(lib, big, lib.wvg_search_device, qb, 200, reps=1)[0],
                filtered_search(fr.c, fr.pq[:nqb], 10, [words], 0, F_STRIDE)[0]]
        calls = [(big, qb[:5], 10, None), (f, qf, 10, None), (big, qb, 200, None), (fr.c, fr.pq[:nqb], 10, words)]
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


# ---- 6. graph capture ------------------------------------------------------------------------------
def test_captured_calls_replay(frefs):
    """One unfiltered and one filtered call captured on one stream; the queries and lists are overwritten in
    place before each replay, and the replays write what uncaptured calls with those inputs write."""
    import torch

    r = frefs(METRIC_L2, 1536)
    lib = r.c.lib
    k = 10
    nq = 2 * q_of(r.c, k) + 1
    dev = torch.device("cuda:0")
    sets = []
    for sh in (0, 1, 3):  # the inputs at capture time, then those of the two replays
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


# ---- 7. plan and errors ----------------------------------------------------------------------------
def test_plan_and_errors(ctx, orc, refs, big):
    import torch

    r = refs(METRIC_L2, 1536)
    lib = r.c.lib
    dev = torch.device("cuda:0")
    for k in (10, 65, 129, 256):
        q = q_of(r.c, k)
        for nq in (2, q, q + 1, 2 * q + 3, 100):
            assert plan(r.c, nq, k) == (1, q, -(-nq // q), 0, 0)
        assert plan(r.c, 1, k) == (0, 1, 1, 0, 0)
    assert plan(r.c, 0, 10) == (0, 1, 0, 0, 0) and plan(r.c, 5, 0) == (0, 1, 0, 0, 0)
    # cache_reuse = 0: one full scan per query, the same arrays
    cx0 = Context(0, cache_reuse=0)
    c0 = Corpus(cx0, KIND_BQ, METRIC_L2, 1536, N)
    pq = Corpus(ctx, KIND_PQ, METRIC_L2, 64, 640)
    try:
        c0.upsert(r.ids, make_rows(orc, 1536))
        c0.delete(np.array(DEAD, np.uint64))
        nq = 2 * q_of(r.c, 10) + 3
        assert plan(c0, nq, 10) == (0, 1, nq, 0, 0) and plan(c0, 1, 10) == (0, 1, 1, 0, 0)
        for k in (10, 200):
            for got in _pipelined(c0, r.pq[:nq], k):
                same(got, r.device(k), nq)
        # a workspace one byte short of the call's layout: the shared-row layout on the large corpus (its lists
        # outnumber wvg_search_device's), wvg_search_device's for one query
        for c, n, k in ((big, 2 * q_of(big, 200) + 1, 200), (r.c, 1, 10)):
            size = lib.wvg_search_workspace_size(c.handle, n, k)
            ws = torch.zeros(size, dtype=torch.uint8, device=dev)
            tq = torch.zeros((n, 1536), dtype=torch.float32, device=dev)
            oi = torch.zeros((n, k), dtype=torch.int64, device=dev)
            od = torch.zeros((n, k), dtype=torch.float32, device=dev)
            oc = torch.zeros(n, dtype=torch.int32, device=dev)
            args = (oi.data_ptr(), od.data_ptr(), oc.data_ptr(), ws.data_ptr())
            s = torch.cuda.current_stream().cuda_stream
            assert lib.wvg_search_device_pipelined(c.handle, tq.data_ptr(), n, k, *args, size - 1, s) == _lib.WVG_ERR_INVALID
            assert lib.wvg_search_device_pipelined(c.handle, tq.data_ptr(), n, k, *args, size, s) == _lib.WVG_OK
            torch.cuda.synchronize()
        # PQ corpora and k = 257 stay unsupported
        sp = _lib.StreamPlan()
        assert lib.wvg_search_device_pipelined_plan(pq.handle, 5, 10, sp) == _lib.WVG_ERR_UNSUPPORTED
        assert lib.wvg_search_device_pipelined_plan(r.c.handle, 5, 257, sp) == _lib.WVG_ERR_UNSUPPORTED
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
        tq = torch.zeros((5, 1536), dtype=torch.float32, device=dev)
        oi = torch.zeros((5, 257), dtype=torch.int64, device=dev)
        od = torch.zeros((5, 257), dtype=torch.float32, device=dev)
        oc = torch.zeros(5, dtype=torch.int32, device=dev)
        for c, k in ((pq, 10), (r.c, 257)):
            rc = lib.wvg_search_device_pipelined(c.handle, tq.data_ptr(), 5, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
            assert rc == _lib.WVG_ERR_UNSUPPORTED
    finally:
        pq.destroy()
        c0.destroy()
        cx0.close()


def test_python_wrappers_take_bq(frefs):
    """ShardedFlatIndex.search_device(pipelined=True) with and without allow words on a BQ corpus."""
    import torch

    from weaviate_amd.shard import ShardedFlatIndex

    r = frefs(METRIC_L2, 1536)
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

"""The k > 256 routes past the sizes at which their CU-capped grids wrap.

Every route above the fused register top-k is a chain of kernels whose grids stop at a multiple of the
CU count C and loop over the rest; tests/test_gpu_select.py, test_gpu_device_large_k.py and
test_gpu_heap_replay.py stay below every one of those loops' second trip.  With tiles = 64 slots and
ranges = 2048 slots (DSEL_RANGE):

  keys kernels (ordkeys_f32 / bq / pq_kernel, dsel_keys_f32_kernel)   grid min(tiles / 4, 8 C) blocks of 4 waves,
      a wave takes tile gw, gw + NW, ...: a second tile from tiles > NW = 32 C
  key_compact_kernel, key_compact_chunks_kernel                       grid min(slots / 256, 8 C) blocks of 256
      slots per trip: a second trip from slots > 2048 C
  dsel_scan_kernel                                                    256 threads, per = ceil(ranges / 256) ranges
      each: per > 1 from ranges > 256

geometry(C) derives two corpus sizes from the device's C: N2 (second tile, second trip, per = 2, ragged
last tile) and N3 (a third tile for some waves, per = 3); its inequalities are asserted before any GPU
call, and for C = 256 by a test that needs no device.  Rows are 8 floats wide, so the corpora are some
20 to 40 MB.  Everything is compared bit for bit -- ids, distance bits, counts, padding -- with the oracle
and, for the device route, also with the host route."""
import numpy as np
import pytest

from test_gpu_device_large_k import bits, dev_queries, dev_search, kth_ties, same
from test_gpu_heap_replay import assert_pops
from test_gpu_select import check_lex
from weaviate_amd import _lib
from weaviate_amd._lib import KIND_BQ, KIND_F32, KIND_PQ, METRIC_COSINE, METRIC_DOT, METRIC_L2
from weaviate_amd.device import Corpus, allow_bitmap

gpu = pytest.mark.gpu  # per test: test_geometry_at_256_cus runs without a device

ORC_METRIC = {METRIC_L2: 0, METRIC_DOT: 1, METRIC_COSINE: 2}
NONE = np.uint64(2**64 - 1)
RANGE = 2048  # DSEL_RANGE
BASE_ID = 640
T0 = 5        # a dead tile that is some wave's first
KS = [257, 1000, 100_000]


def tiles(n):
    return (n + 63) // 64


def ranges(n):
    return (64 * tiles(n) + RANGE - 1) // RANGE


def geometry(C):
    """(N2, N3, NW) for a device of C CUs, with the trip counts they were chosen for asserted."""
    base = max(32 * C * 64, 8 * C * 256, 256 * RANGE)
    n2 = base * 7 // 6 + 37
    n3 = 2 * base + base // 8 + 37
    nw = 4 * min((tiles(n2) + 3) // 4, 8 * C)  # waves of the capped keys grids
    assert nw == 4 * min((tiles(n3) + 3) // 4, 8 * C) == 32 * C
    assert tiles(n2) > nw                      # keys: some waves take a second tile
    assert 64 * tiles(n2) > 8 * C * 256        # compaction: a second trip
    assert ranges(n2) > 256                    # dsel_scan_kernel: per = 2
    assert (ranges(n2) + 255) // 256 == 2
    assert tiles(n3) > 2 * nw                  # keys: some waves take a third tile
    assert ranges(n3) > 512                    # per = 3
    assert (ranges(n3) + 255) // 256 == 3
    assert n2 % 64 != 0 and n3 % 64 != 0       # ragged last tiles
    assert 7 + nw < tiles(n2) - 1 and T0 + nw < tiles(n2) - 1  # the planted tiles exist
    return n2, n3, nw


def test_geometry_at_256_cus():
    """The arithmetic at the MI355X's 256 CUs; needs no device."""
    n2, n3, nw = geometry(256)
    assert (n2, tiles(n2), ranges(n2)) == (611_706, 9_558, 299)
    assert (n3, tiles(n3), ranges(n3)) == (1_114_149, 17_409, 545)
    assert nw == 8192
    for C in (64, 104, 228, 304):  # the sizes scale with C
        geometry(C)


def cu_count():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count  # what wvg_open reads


def normalize_rows(orc, X):
    """orc.normalize of every row, vectorised: the squares summed in element order in float32, the root in
    double, one float32 division per element.  Checked against orc.normalize on sampled rows."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    norm = np.zeros(len(X), np.float32)
    for j in range(X.shape[1]):
        norm = norm + X[:, j] * X[:, j]
    root = np.sqrt(norm.astype(np.float64)).astype(np.float32)
    out = np.zeros_like(X)
    np.divide(X, root[:, None], out=out, where=(norm != 0)[:, None])
    for i in np.random.default_rng(3).choice(len(X), 512, replace=False):
        assert np.array_equal(bits(out[i]), bits(orc.normalize(X[i]))), i
    return out


def assert_padding(ids, dists, counts):
    for qi, n in enumerate(counts):
        assert np.all(ids[qi, n:] == NONE) and np.all(np.isposinf(dists[qi, n:])), qi


# ---- the F32 corpora at N2 ---------------------------------------------------------------------------
class F32Set:
    """Rows, deletes and plants at N2, one corpus per metric (made on first use), and per metric the
    oracle's lexicographic list of every query down to max(KS), from which each k takes its prefix."""

    def __init__(self, ctx, orc):
        self.ctx, self.orc = ctx, orc
        self.C = cu_count()
        self.n, _, self.nw = geometry(self.C)
        n, nw = self.n, self.nw
        self.t1 = 7 + nw  # a dead tile that is the second of the wave whose first is tile 7
        self.rows = orc.synth_rows(2401, 0, n, 8, 0)
        self.qs = orc.synth_rows(2402, 0, 10, 8, 0)
        self.valid = np.ones(n, bool)
        self.valid[0:10_000:7] = False
        self.valid[64 * T0:64 * T0 + 64] = False
        self.valid[64 * self.t1:64 * self.t1 + 64] = False
        # plants: tile T0 + NW is the second of the wave whose first tile is dead; tile 7 is the first of
        # the wave whose second tile is dead
        self.plants = [64 * (T0 + nw) + 9, 64 * 7 + 9]
        assert all(self.valid[p] for p in self.plants)
        self.rows[self.plants[0]] = self.qs[0]
        self.rows[self.plants[1]] = self.qs[1]
        self.ids_all = np.arange(BASE_ID, BASE_ID + n, dtype=np.uint64)
        self.corpora, self.lists, self.srows = {}, {}, {}

    def stored(self, metric):
        if metric != METRIC_COSINE:
            return self.rows
        if metric not in self.srows:
            self.srows[metric] = normalize_rows(self.orc, self.rows)
        return self.srows[metric]

    def corpus(self, metric):
        if metric not in self.corpora:
            c = Corpus(self.ctx, KIND_F32, metric, 8, self.n, id_base=BASE_ID)
            self.corpora[metric] = c
            c.upsert(self.ids_all, self.rows)
            c.delete(self.ids_all[~self.valid])
            assert c.info()[0] == int(self.valid.sum())
        return self.corpora[metric]

    def all_d(self, metric, qi):
        dq = dev_queries(self.orc, metric, self.qs[qi:qi + 1])[0]
        return self.orc.dist_all(ORC_METRIC[metric], dq, self.stored(metric))

    def oracle(self, metric):
        if metric not in self.lists:
            live_ids = self.ids_all[self.valid]
            self.lists[metric] = [self.orc.lex_topk(self.all_d(metric, qi)[self.valid], live_ids, max(KS))
                                  for qi in range(len(self.qs))]
        return self.lists[metric]

    def destroy(self):
        for c in self.corpora.values():
            c.destroy()


@pytest.fixture(scope="module")
def f32set(ctx, orc):
    s = F32Set(ctx, orc)
    try:
        yield s
    finally:
        s.destroy()


# ---- 1. host route against the oracle at N2 ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", KS)
def test_host_route_at_n2(f32set, orc, k):
    """wvg_search, k > 256 (search_large_k: ordkeys_f32_kernel, select, key_compact_kernel, sort) over 9558
    tiles at C = 256: waves with a second tile, one of them dead for a wave either way round, the
    compaction's second trip.  Plain, with an allow list of every third id, and with a window of 700 ids
    near the end (tile_begin != 0, slot0 above 2^19, fewer rows than k: padding)."""
    s = f32set
    n, c, qs = s.n, s.corpus(METRIC_L2), s.qs[:2]
    all_d = [s.all_d(METRIC_L2, qi) for qi in range(2)]
    third = np.arange(BASE_ID + 100, BASE_ID + n - 100, 3, dtype=np.uint64)
    w0 = n - 4000
    window = np.arange(BASE_ID + w0, BASE_ID + w0 + 700, dtype=np.uint64)
    assert w0 // 64 != 0 and w0 // 64 * 64 > 2**19 and s.valid[w0:w0 + 700].all()
    for what, allow in (("plain", None), ("third", third), ("window", window)):
        keep = s.valid if allow is None else s.valid & np.isin(s.ids_all, allow)
        ids, dists, counts = c.search(qs, k, None if allow is None else allow_bitmap(allow))
        for qi in range(2):
            check_lex(orc, ids[qi], dists[qi], counts[qi], all_d[qi][keep], s.ids_all[keep], k)
        assert np.all(counts == min(k, int(keep.sum()))), what
        assert_padding(ids, dists, counts)
    assert counts[0] == (257 if k == 257 else 700)  # the window pads for the two larger k


# ---- 2. trip plants ------------------------------------------------------------------------------------
@gpu
def test_trip_plants(f32set, orc):
    """Query 0 equals a row of tile T0 + NW, the second tile of the wave whose first tile T0 is dead
    (m == 0 -> continue in dsel_keys_f32_kernel): the wave must still deliver distance 0 there.  Query 1
    equals a row of tile 7, whose wave's second tile 7 + NW is dead: the wave must keep its first."""
    s = f32set
    c, qs = s.corpus(METRIC_L2), s.qs[:2]
    for got in (c.search(qs, 257), dev_search(c, qs, 257)):
        for qi in range(2):
            assert got[0][qi][0] == np.uint64(BASE_ID + s.plants[qi])
            assert bits(got[1][qi][:1])[0] == 0
            assert got[2][qi] == 257


# ---- 3. device route against host and oracle at N2 -----------------------------------------------------
@gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT, METRIC_COSINE])
def test_device_route_at_n2(f32set, orc, metric, k):
    """wvg_search_device, k > 256 (dsel_search) with nq = 10: groups of 4 + 4 + 2 -- a second full group's
    query offset and gq = 2 -- over 299 compaction ranges at C = 256 (dsel_scan_kernel: per = 2, its
    last threads past the end)."""
    s = f32set
    c, qs = s.corpus(metric), s.qs
    nq = len(qs)
    size = c.lib.wvg_search_workspace_size(c.handle, nq, k)
    assert size == c.lib.wvg_search_workspace_size(c.handle, 64, k)  # G key arrays, not nq
    want = c.search(qs, k)
    same(dev_search(c, dev_queries(orc, metric, qs), k), want, (metric, k))
    hi, hd, hc = want
    for qi, (wi, wd) in enumerate(s.oracle(metric)):
        assert hc[qi] == k
        assert np.array_equal(hi[qi], wi[:k]) and np.array_equal(bits(hd[qi]), bits(wd[:k])), qi


# ---- 4. ties across hundreds of ranges at N2 -----------------------------------------------------------
class TieSet:
    def __init__(self, ctx, orc):
        self.n, _, self.nw = geometry(cu_count())
        n = self.n
        self.rows = np.floor(orc.synth_rows(2421, 0, n, 8, 1) / 64).astype(np.float32)
        self.qs = np.floor(orc.synth_rows(2422, 0, 6, 8, 1) / 64).astype(np.float32)
        self.qs[5] = self.qs[0]  # identical queries in different groups of 4
        self.ids_all = np.arange(n, dtype=np.uint64)
        self.all_d = [orc.dist_all(0, q, self.rows) for q in self.qs]
        # the largest tie class of query 0, as [start, start + count) of the sorted distances
        vals, starts, cnts = np.unique(np.sort(self.all_d[0]), return_index=True, return_counts=True)
        j = int(np.argmax(cnts))
        assert j + 1 < len(vals)
        self.ks = {"mid": (int(starts[j] + cnts[j] // 2), vals[j]),        # half of the class is kept
                   "boundary": (int(starts[j + 1] + 1), vals[j + 1])}      # one row of the next class
        self.c = Corpus(ctx, KIND_F32, METRIC_L2, 8, n)
        self.c.upsert(self.ids_all, self.rows)


@pytest.fixture(scope="module")
def tieset(ctx, orc):
    s = TieSet(ctx, orc)
    try:
        yield s
    finally:
        s.c.destroy()


@gpu
@pytest.mark.parametrize("which", ["mid", "boundary"])
def test_ties_across_ranges(tieset, orc, which):
    """Integer rows floor(x / 64): a few dozen distinct distances over N2 rows.  k at the midpoint of query
    0's largest tie class, and one row into the class after it: the rows equal to the threshold spread
    over hundreds of compaction ranges and over first and second tiles, and the first krem of them in
    slot order are the result (the rank / scan / compact carry across ranges)."""
    s = tieset
    k, thr = s.ks[which]
    assert k > 256 and kth_ties(s.all_d[0], k) and np.sort(s.all_d[0])[k - 1] == thr
    cls = np.flatnonzero(s.all_d[0] == thr)
    assert len(np.unique(cls // RANGE)) >= 200
    assert (cls // 64 < s.nw).any() and (cls // 64 >= s.nw).any()
    host = s.c.search(s.qs, k)
    dev = dev_search(s.c, s.qs, k)
    same(dev, host, which)
    lists = [orc.lex_topk(d, s.ids_all, k) for d in s.all_d]
    for got in (host, dev):
        assert np.all(got[2] == k)
        for qi, (wi, wd) in enumerate(lists):
            assert np.array_equal(got[0][qi], wi) and np.array_equal(bits(got[1][qi]), bits(wd)), qi
        assert np.array_equal(got[0][0], got[0][5]) and np.array_equal(bits(got[1][0]), bits(got[1][5]))


# ---- 5. device route at N3 -----------------------------------------------------------------------------
@gpu
def test_device_route_at_n3(ctx, orc):
    """N3: 17409 tiles and 545 ranges at C = 256 -- a third tile for some waves (one of them dead), per = 3
    in dsel_scan_kernel, the slot count of the 1M-row benchmark shape."""
    _, n, nw = geometry(cu_count())
    nq = 5
    rows = orc.synth_rows(2431, 0, n, 8, 0)
    qs = orc.synth_rows(2432, 0, nq, 8, 0)
    ids_all = np.arange(n, dtype=np.uint64)
    valid = np.ones(n, bool)
    valid[[3, 64 * nw + 1, 128 * nw + 2, n - 1]] = False
    t3 = 2 * nw + 11  # the third tile of wave 11
    assert t3 < tiles(n) - 1
    valid[64 * t3:64 * t3 + 64] = False
    rows[64 * (2 * nw + 12) + 5] = qs[0]  # the nearest row of query 0 sits in a third tile
    c = Corpus(ctx, KIND_F32, METRIC_L2, 8, n)
    try:
        c.upsert(ids_all, rows)
        c.delete(ids_all[~valid])
        lists = [orc.lex_topk(orc.dist_all(0, q, rows)[valid], ids_all[valid], 100_000) for q in qs]
        for k in (1000, 100_000):
            hi, hd, hc = want = c.search(qs, k)
            same(dev_search(c, qs, k), want, k)
            for qi, (wi, wd) in enumerate(lists):
                assert hc[qi] == k
                assert np.array_equal(hi[qi], wi[:k]) and np.array_equal(bits(hd[qi]), bits(wd[:k])), qi
        assert hi[0][0] == 64 * (2 * nw + 12) + 5 and bits(hd[0][:1])[0] == 0
    finally:
        c.destroy()


# ---- 6. BQ at N2 ---------------------------------------------------------------------------------------
class BqSet:
    def __init__(self, ctx, orc):
        self.n, _, self.nw = geometry(cu_count())
        n, nw = self.n, self.nw
        rng = np.random.default_rng(2441)
        self.codes = rng.integers(0, 2**64, (n, 1), dtype=np.uint64)  # d = 64: one word per row
        self.qs = orc.synth_rows(2442, 0, 9, 64, 0)
        self.qcodes = [orc.bq_encode(q) for q in self.qs]
        self.ids_all = np.arange(n, dtype=np.uint64)
        self.valid = np.ones(n, np.uint8)
        self.valid[[7, 64, 4000, 64 * nw + 3, n - 1]] = 0
        self.valid[64 * (3 + nw):64 * (3 + nw) + 64] = 0  # a whole tile, the second of its wave
        self.c = Corpus(ctx, KIND_BQ, METRIC_L2, 64, n)
        self.c.upsert_codes(self.ids_all, self.codes)
        self.c.delete(self.ids_all[self.valid == 0])


@pytest.fixture(scope="module")
def bqset(ctx, orc):
    s = BqSet(ctx, orc)
    try:
        yield s
    finally:
        s.c.destroy()


@gpu
@pytest.mark.parametrize("k", [300, 50_000])
def test_bq_at_n2(bqset, orc, k):
    """ordkeys_bq_kernel's second tile on both routes, Hamming distances 0..64: tens of thousands of rows
    tie at the threshold.  nq = 9: groups of 4 + 4 + 1."""
    s = bqset
    live = s.valid != 0
    hi, hd, hc = want = s.c.search(s.qs, k)
    same(dev_search(s.c, s.qs, k), want, k)
    tied = 0
    for qi, qc in enumerate(s.qcodes):
        ham = orc.bq_dist_all(qc, s.codes)[live]
        tied += kth_ties(ham, k)
        wi, wd = orc.lex_topk(ham, s.ids_all[live], k)
        assert hc[qi] == k
        assert np.array_equal(hi[qi], wi) and np.array_equal(bits(hd[qi]), bits(wd)), qi
    assert tied >= 1


@gpu
@pytest.mark.parametrize("R", [257, 3000])
def test_bq_heap_replay_at_n2(bqset, orc, R):
    """The heap replay for windows above 256 (bq_select_kept): key_compact_chunks_kernel's second trip,
    and the counts and selects over prefixes of the keys (launch_key_count, launch_select_kth) up to
    lengths beyond the capped grids' first trip.  One query and two."""
    s = bqset
    assert_pops(orc, s.c, s.qs[:1], s.codes, s.qcodes[:1], R, s.valid)
    assert_pops(orc, s.c, s.qs[:2], s.codes, s.qcodes[:2], R, s.valid)


# ---- 7. PQ at N2 ---------------------------------------------------------------------------------------
@gpu
def test_pq_at_n2(ctx, orc):
    """ordkeys_pq_kernel's second tile on both routes: m = 8 segments of one float, 256 centroids each."""
    n, _, nw = geometry(cu_count())
    m, ks, nq, k = 8, 256, 5, 1000
    centers = orc.synth_rows(2451, 0, m * ks, 1, 0).reshape(m, ks, 1)
    codes = np.random.default_rng(2452).integers(0, ks, (n, m), dtype=np.uint8)
    qs = orc.synth_rows(2453, 0, nq, m, 0)
    ids_all = np.arange(n, dtype=np.uint64)
    valid = np.ones(n, bool)
    valid[[7, 64, 64 * nw + 3]] = False
    valid[64 * (3 + nw):64 * (3 + nw) + 64] = False
    c = Corpus(ctx, KIND_PQ, METRIC_L2, m, n)
    try:
        c.set_codebook(centers)
        c.upsert_codes(ids_all, codes)
        c.delete(ids_all[~valid])
        hi, hd, hc = want = c.search(qs, k)
        same(dev_search(c, qs, k), want)
        sample = np.random.default_rng(2454).choice(n, 512, replace=False)
        for qi in range(nq):
            lut = orc.pq_lut(0, qs[qi], centers)
            acc = np.zeros(n, np.float32)  # orc.pq_adc of every row: the segments in order, float32
            for seg in range(m):
                acc = acc + lut[seg, codes[:, seg]]
            for i in sample:
                assert bits(acc[i:i + 1])[0] == bits([orc.pq_adc(0, lut, codes[i])])[0], (qi, i)
            wi, wd = orc.lex_topk(acc[valid], ids_all[valid], k)
            assert hc[qi] == k
            assert np.array_equal(hi[qi], wi) and np.array_equal(bits(hd[qi]), bits(wd)), qi
    finally:
        c.destroy()


# ---- 8. range search at N2 -----------------------------------------------------------------------------
@gpu
def test_search_by_distance_at_n2(f32set, orc):
    """wvg_search_by_distance: key_compact_kernel with a threshold from the host on its second trip, and
    results beyond 100,000 rows, against the growing-limit loop over the oracle's list."""
    s = f32set
    c, q = s.corpus(METRIC_L2), s.qs[2]
    all_d = s.all_d(METRIC_L2, 2)[s.valid]
    li, ld = orc.lex_topk(all_d, s.ids_all[s.valid], len(all_d))  # the whole list once; a search is a prefix

    def search_fn(total):
        return li[:total], ld[:total]

    srt = ld  # ascending
    targets = [srt[50], srt[5000], srt[150_000], np.nextafter(srt[5000], np.float32(-np.inf))]
    longest = 0
    for t in targets:
        for max_limit in (-1, 11_100):
            ei, ed = orc.search_by_distance(search_fn, t, max_limit)
            gi, gd = c.search_by_distance(q, t, max_limit)
            assert len(gi) == len(ei), (t, max_limit, len(gi), len(ei))
            assert np.array_equal(gi, ei) and np.array_equal(bits(gd), bits(ed)), (t, max_limit)
            longest = max(longest, len(gi))
    assert longest > 100_000


# ---- 9. capture of the non-F32 forms -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["bq", "pq"])
def test_graph_capture_bq_pq(ctx, orc, kind):
    """test_graph_capture of test_gpu_device_large_k.py records the F32 form.  The BQ form also records a
    memset, a 2-D device copy and the encode of the queries, the PQ form the LUT kernel: one call of each
    captured, then replayed with two new query sets."""
    import torch

    lib = _lib.load()
    dev = torch.device("cuda:0")
    n, nq, k = 5000, 5, 1000
    if kind == "bq":
        d = 200
        c = Corpus(ctx, KIND_BQ, METRIC_L2, d, n)
    else:
        d, m, ks = 64, 16, 256
        c = Corpus(ctx, KIND_PQ, METRIC_DOT, d, n)
    try:
        if kind == "pq":
            c.set_codebook(orc.synth_rows(2461, 0, m * ks, d // m, 0).reshape(m, ks, d // m))
        c.upsert(np.arange(n, dtype=np.uint64), orc.synth_rows(2462, 0, n, d, 0))
        c.delete(np.array([7, 64, 4000], np.uint64))
        sets = [orc.synth_rows(2463 + i, 0, nq, d, 0) for i in range(3)]
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

"""wvg_search_group: nq single-query flat searches, query i against a corpus of
its own (the tenants of a multi-tenant class), in one scan launch and one merge
launch.  Its outputs must be those of nq separate wvg_search calls -- ids,
distance bits, counts and padding -- and, where the rows are on the host, the
lexicographic (distance, docID) top-k of the oracle.

The scan kernel is a template over <METRIC, D, E> like K1 (tests/
test_gpu_k1_matrix.py): METRIC 0 L2, 1 DOT (dot and cosine), 3 MANHATTAN,
4 HAMMING; D the fixed row lengths or 0 for the generic one; E = 1 for k <= 64,
2 for k <= 128, 4 above.  GROUP below is what test_equals_separate_calls runs;
tests/test_group_descriptors.py compares it with the kernels in the library.
"""
import ctypes
import threading

import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import (KIND_BQ, KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_HAMMING, METRIC_L2,
                               METRIC_MANHATTAN, ORDER_AVX256, ORDER_AVX512)
from weaviate_amd.device import Context, Corpus, allow_bitmap, search_group

GROUP = {"fixed_d": (128, 768, 1536), "generic_d": (3, 100), "ks": (1, 10, 64, 100, 256)}
METRICS = [METRIC_L2, METRIC_DOT, METRIC_COSINE, METRIC_MANHATTAN, METRIC_HAMMING]  # = the oracle's metric ids
DIMS = GROUP["fixed_d"] + GROUP["generic_d"]
METRIC_KERNEL = {METRIC_L2: 0, METRIC_DOT: 1, METRIC_COSINE: 1, METRIC_MANHATTAN: 3, METRIC_HAMMING: 4}


def list_registers(k):
    return 1 if k <= 64 else (2 if k <= 128 else 4)


def kernel_forms():
    """The (metric kernel, D, E) instantiations test_equals_separate_calls reaches."""
    return {(METRIC_KERNEL[m], d if d in GROUP["fixed_d"] else 0, list_registers(k))
            for m in METRICS for d in DIMS for k in GROUP["ks"]}


ROWS = [0, 1, 63, 64, 65, 257, 1000, 5000]  # around the 64-row tile; 5000 rows = 79 tiles = several work items
ID_BASES = [0, 64, 6400]
NQ = 24


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def synth(orc, metric, seed, n, d, dist=0):
    """Uniform [-1, 1) rows (dist 0) or integers 0..255 (dist 1: exact sums, many
    distance ties); hamming counts unequal elements, so integers 0..3 there."""
    if n == 0:
        return np.empty((0, d), np.float32)
    if metric == METRIC_HAMMING:
        return np.floor(orc.synth_rows(seed, 0, n, d, 1) / 64).astype(np.float32)
    return orc.synth_rows(seed, 0, n, d, dist)


class Tenant:
    """One corpus with its host rows, stored (normalized) rows and live mask."""

    def __init__(self, cx, orc, metric, d, rows, id_base, spare, seed, dist=0):
        self.orc, self.metric, self.id_base, self.n = orc, metric, id_base, rows
        self.c = Corpus(cx, KIND_F32, metric, d, max(rows + spare, 64), id_base)
        self.ids = np.arange(id_base, id_base + rows, dtype=np.uint64)
        self.rows = synth(orc, metric, seed, rows, d, dist)
        if rows:
            self.c.upsert(self.ids, self.rows)
        self.stored = orc.normalize_rows(self.rows) if metric == METRIC_COSINE and rows else self.rows
        self.live = np.ones(rows, bool)

    def delete(self, ids):
        ids = np.asarray(ids, np.uint64)
        self.c.delete(ids)
        self.live[(ids - np.uint64(self.id_base)).astype(np.int64)] = False

    def distances(self, q, dist_all=None):
        """The oracle's distance of q to every stored row."""
        pq = self.orc.normalize(q) if self.metric == METRIC_COSINE else np.asarray(q, np.float32)
        return (dist_all or self.orc.dist_all)(self.metric, pq, self.stored)

    def oracle(self, all_d, k, allowed=None):
        """(ids, dists) of the lexicographic top-k over the live (and allowed) rows."""
        sel = self.live if allowed is None else self.live & allowed
        return self.orc.lex_topk(all_d[sel], self.ids[sel], k)


def make_tenants(cx, orc, metric, d, seed, dist=0, rows=ROWS):
    return [Tenant(cx, orc, metric, d, n, ID_BASES[i % 3], 128 * (i % 2), seed + i, dist) for i, n in enumerate(rows)]


def destroy(tenants):
    for t in tenants:
        t.c.destroy()


def assert_equals_separate(tenants, which, qs, k, allows=None, res=None):
    """The grouped call == Corpus.search(q_i, k, allow_i) on tenants[which[i]], padding included."""
    ids, dists, counts = res if res is not None else search_group([tenants[t].c for t in which], qs, k, allows)
    assert ids.shape == (len(which), k) and dists.shape == (len(which), k) and counts.shape == (len(which),)
    for i, t in enumerate(which):
        a = None if allows is None else allows[i]
        wi, wd, wc = tenants[t].c.search(qs[i], k, a)
        assert counts[i] == wc[0], (i, t, counts[i], wc[0])
        assert np.array_equal(ids[i], wi[0]), (i, t)
        assert np.array_equal(bits(dists[i]), bits(wd[0])), (i, t)
    return ids, dists, counts


def oracle_distances(tenants, which, qs, dist_all=None):
    """Per query the oracle's distances to its tenant's rows (None for an empty tenant): computed
    once per case and shared by every k."""
    return [tenants[t].distances(qs[i], dist_all) if tenants[t].n else None for i, t in enumerate(which)]


def assert_equals_oracle(tenants, which, all_d, k, res, allowed=None):
    ids, dists, counts = res
    for i, t in enumerate(which):
        if all_d[i] is None:
            wi, wd = np.empty(0, np.uint64), np.empty(0, np.float32)
        else:
            wi, wd = tenants[t].oracle(all_d[i], k, None if allowed is None else allowed[i])
        n = len(wi)
        assert counts[i] == n, (i, t, counts[i], n)
        assert np.array_equal(ids[i, :n], wi), (i, t)
        assert np.array_equal(bits(dists[i, :n]), bits(wd)), (i, t)
        assert np.all(ids[i, n:] == np.uint64(0xFFFFFFFFFFFFFFFF)) and np.all(np.isposinf(dists[i, n:])), (i, t)


def shuffled_targets(seed, ntenants, nq=NQ):
    """Every tenant at least once, one of them (the largest) several times, in shuffled order."""
    rng = np.random.default_rng(seed)
    which = list(range(ntenants)) + [ntenants - 1] * 3
    which += list(rng.integers(0, ntenants, nq - len(which)))
    rng.shuffle(which)
    return [int(t) for t in which]


# ---- 1. equality with separate calls and with the oracle -----------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_equals_separate_calls(ctx, orc, metric, d):
    # integer-valued rows at d = 128 and 3: exact distance ties across rows, decided by docID
    dist = 1 if d in (128, 3) else 0
    tenants = make_tenants(ctx, orc, metric, d, 5000 + 11 * d + metric, dist)
    try:
        which = shuffled_targets(d + metric, len(tenants))
        qs = synth(orc, metric, 9000 + d + metric, NQ, d, dist)
        all_d = oracle_distances(tenants, which, qs)
        for k in GROUP["ks"]:  # k above the rows of the small tenants
            res = assert_equals_separate(tenants, which, qs, k)
            assert_equals_oracle(tenants, which, all_d, k, res)
    finally:
        destroy(tenants)


# ---- 2. per-query filters in one call ---------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("metric,d,k", [(METRIC_L2, 128, 10), (METRIC_COSINE, 100, 100)])
def test_per_query_filters(ctx, orc, metric, d, k):
    tenants = make_tenants(ctx, orc, metric, d, 700 + d, rows=[5000, 1000, 257, 0])
    try:
        rng = np.random.default_rng(d)
        which, allows, allowed = [], [], []

        def add(t, ids, n_bits=None, words=None):
            tn = tenants[t]
            which.append(t)
            if ids is None:
                allows.append(None)
                allowed.append(None)
                return
            ids = np.asarray(ids, np.uint64)
            allows.append(allow_bitmap(ids, n_bits) if words is None else words)
            m = np.zeros(tn.n, bool)
            loc = ids[(ids >= tn.id_base) & (ids < tn.id_base + tn.n)] - np.uint64(tn.id_base)
            m[loc.astype(np.int64)] = True
            allowed.append(m)

        for t, tn in enumerate(tenants):
            base, n = tn.id_base, tn.n
            add(t, None)                                                   # no filter
            add(t, [], words=np.empty(0, np.uint64))                       # non-NULL, 0 words: nothing
            if n == 0:
                add(t, [base + 3])                                         # a list over an empty tenant
                continue
            add(t, [base + n // 2])                                        # a single id
            add(t, np.arange(base + n // 3, base + n // 3 + min(n // 2, 700)))   # a contiguous range
            add(t, base + rng.choice(n, max(1, n // 10), replace=False))   # ~10 % random ids
            add(t, [base + 1, base + n // 4])                              # a bitmap shorter than the corpus
            add(t, [base + n + 200, base + n + 4000])                      # set bits only beyond the tenant's rows
            if base:
                add(t, [0, base - 1])                                      # ... and only before its docID range
        qs = synth(orc, metric, 31 + d, len(which), d)
        res = assert_equals_separate(tenants, which, qs, k, allows)
        assert_equals_oracle(tenants, which, oracle_distances(tenants, which, qs), k, res, allowed)
        assert res[2][1] == 0 and res[2][0] == min(k, tenants[0].n)  # the empty list empties its own query only
    finally:
        destroy(tenants)


# ---- 3. deletes ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_deletes_and_k_above_live_count(ctx, orc):
    d = 128
    tenants = make_tenants(ctx, orc, METRIC_L2, d, 1200, rows=[300, 1000, 65])
    try:
        for tn in tenants:
            b, n = tn.id_base, tn.n
            scattered = [b, b + 7, b + 63, b + n // 2]
            whole_tile = list(range(b + 64, b + 128)) if n >= 192 else []  # one whole 64-row tile
            tn.delete(sorted(set(scattered + whole_tile + [b + n - 1])))   # and the tenant's last row
        which = [0, 1, 2, 1, 0, 2]
        qs = synth(orc, METRIC_L2, 77, len(which), d)
        all_d = oracle_distances(tenants, which, qs)
        for k in (10, 256):  # 256 > the live rows of tenants 0 and 2
            res = assert_equals_separate(tenants, which, qs, k)
            assert_equals_oracle(tenants, which, all_d, k, res)
        assert res[2][0] == int(tenants[0].live.sum()) < 256
    finally:
        destroy(tenants)


# ---- 4. the AVX-512 order -------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("metric,d", [(METRIC_L2, 768), (METRIC_DOT, 300)])
def test_avx512_order(ctx, orc, metric, d):
    ctx.set_distance_order(ORDER_AVX512)
    try:
        tenants = make_tenants(ctx, orc, metric, d, 4100 + d, rows=[1000, 65, 257])
        try:
            which = [2, 0, 1, 0]
            qs = synth(orc, metric, 4200 + d, len(which), d)
            res = assert_equals_separate(tenants, which, qs, 10)
            assert_equals_oracle(tenants, which, oracle_distances(tenants, which, qs, orc.dist_all_512), 10, res)
        finally:
            destroy(tenants)
    finally:
        ctx.set_distance_order(ORDER_AVX256)


# ---- 5. many lists per query ------------------------------------------------------------
# The item rule (group_item_tiles, wvg_group.hip): a call's tile total is
# cut into items of at most T = max(8, ceil(total / (4 * CUs))) tiles (two items for each of the
# two workgroups resident per CU), and a query of n tiles gets ceil(n / T) lists.  The calls
# below total fewer than 5000 tiles, so the ceiling term stays at or below 8 on any chip of 157+
# CUs and T = 8: 40 000 rows = 625 tiles = 79 lists (> 64, one merge wave's first round),
# 300 000 rows = 4688 tiles = 586 lists (> 512, all eight merge waves' first round).
@pytest.mark.gpu
@pytest.mark.parametrize("big_rows,lists", [(40_000, 79), (300_000, 586)])
def test_multi_range_merge(ctx, orc, big_rows, lists):
    d, k = 128, 64
    assert -(-(-(-big_rows // 64)) // 8) == lists
    small = make_tenants(ctx, orc, METRIC_L2, d, 300, rows=[64, 300, 512])  # 1, 5 and 8 tiles: one list each
    big = Tenant(ctx, orc, METRIC_L2, d, 0, 6400, big_rows, 0)
    big.c.fill_synthetic(99, big_rows, 0)
    tenants = small + [big]
    try:
        which = [0, 3, 1, 2, 0, 0]  # the large tenant once: the call's tile total stays below 5000
        allows = [None, None, None, None, None, np.empty(0, np.uint64)]  # the last query gets no list
        qs = synth(orc, METRIC_L2, 555, len(which), d)
        ids, dists, counts = assert_equals_separate(tenants, which, qs, k, allows)
        assert counts.tolist() == [64, 64, 64, 64, 64, 0]
        assert len(set(ids[1].tolist())) == k and ids[1].min() >= 6400
    finally:
        destroy(tenants)


# ---- 6. validation ------------------------------------------------------------------------
@pytest.mark.gpu
def test_validation_leaves_outputs_untouched(ctx, orc):
    lib = ctx.lib
    d, k = 32, 4
    a = Corpus(ctx, KIND_F32, METRIC_L2, d, 64)
    b = Corpus(ctx, KIND_F32, METRIC_L2, d, 64)
    other_dim = Corpus(ctx, KIND_F32, METRIC_L2, d + 4, 64)
    other_metric = Corpus(ctx, KIND_F32, METRIC_DOT, d, 64)
    bq = Corpus(ctx, KIND_BQ, METRIC_L2, d, 64)
    ctx2 = Context(0)
    foreign = Corpus(ctx2, KIND_F32, METRIC_L2, d, 64)
    try:
        for c in (a, b):
            c.upsert(np.arange(8, dtype=np.uint64), synth(orc, METRIC_L2, 1, 8, d))
        qs = synth(orc, METRIC_L2, 2, 3, d)

        def call(corpora, kk=k, queries=qs):
            ids = np.full((3, max(kk, 1)), 0x1234, np.uint64)
            dists = np.full((3, max(kk, 1)), -7.0, np.float32)
            counts = np.full(3, 99, np.uint32)
            hs = (ctypes.c_void_p * 3)(*[c.handle if c is not None else None for c in corpora])
            rc = lib.wvg_search_group(hs, _lib.fptr(queries) if queries is not None else None, 3, kk, None, None,
                                      _lib.u64ptr(ids), _lib.fptr(dists), _lib.u32ptr(counts))
            msg = lib.wvg_last_error().decode()
            untouched = bool(np.all(ids == 0x1234) and np.all(dists == -7.0) and np.all(counts == 99))
            return rc, msg, untouched

        assert call([a, b, a])[0] == _lib.WVG_OK
        for corpora, kk, queries, code, word in [
                ([a, other_dim, b], k, qs, _lib.WVG_ERR_INVALID, "corpora[1]"),
                ([a, b, other_metric], k, qs, _lib.WVG_ERR_INVALID, "corpora[2]"),
                ([a, foreign, b], k, qs, _lib.WVG_ERR_INVALID, "corpora[1]"),
                ([a, None, b], k, qs, _lib.WVG_ERR_INVALID, "corpora[1]"),
                ([a, b, a], k, None, _lib.WVG_ERR_INVALID, "queries"),
                ([a, bq, b], k, qs, _lib.WVG_ERR_UNSUPPORTED, "corpora[1]"),
                ([a, b, a], 257, qs, _lib.WVG_ERR_UNSUPPORTED, "256")]:
            rc, msg, untouched = call(corpora, kk, queries)
            assert rc == code, (rc, msg)
            assert msg and word in msg, msg
            assert untouched, msg
        # nq = 0 is a no-op; k = 0 writes the counts only, as wvg_search does
        assert lib.wvg_search_group(None, None, 0, k, None, None, None, None, None) == _lib.WVG_OK
        ids, dists, counts = search_group([a, b], qs[:2], 0)
        assert counts.tolist() == [0, 0]
    finally:
        for c in (a, b, other_dim, other_metric, bq, foreign):
            c.destroy()
        ctx2.close()


# ---- 7. concurrency -------------------------------------------------------------------
@pytest.mark.gpu
def test_concurrent_groups_and_writers(ctx, orc):
    """Group calls over overlapping tenant sets in different orders while a writer upserts
    and deletes rows too far away to enter any top-k: every result is the static one, and
    nothing deadlocks (the shared locks are taken in one global order)."""
    d, k, calls = 32, 10, 50
    tenants = make_tenants(ctx, orc, METRIC_L2, d, 8800, rows=[500, 257, 1000, 300, 65, 700])
    try:
        orders = [[0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [2, 0, 5, 1, 0, 2], [3, 5, 1, 4, 2, 3]]
        qs = [synth(orc, METRIC_L2, 60 + i, len(o), d) for i, o in enumerate(orders)]
        want = [search_group([tenants[t].c for t in o], q, k) for o, q in zip(orders, qs)]
        for o, q, w in zip(orders, qs, want):
            assert_equals_oracle(tenants, o, oracle_distances(tenants, o, q), k, w)
        errors, stop = [], threading.Event()

        def reader(i):
            try:
                cs = [tenants[t].c for t in orders[i]]
                for _ in range(calls):
                    got = search_group(cs, qs[i], k)
                    for g, w in zip(got, want[i]):
                        if not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
                            raise AssertionError(f"reader {i}: a result changed")
            except Exception as e:  # noqa: BLE001 -- reported by the main thread
                errors.append(e)

        def writer():
            try:
                far = np.full((4, d), 1e6, np.float32)  # L2 distance ~1e13: never among the 10 nearest
                while not stop.is_set():
                    for t in (0, 2):
                        tn = tenants[t]
                        ids = np.arange(tn.id_base + tn.n, tn.id_base + tn.n + 4, dtype=np.uint64)  # in the spare capacity
                        tn.c.reserve(tn.n + 64)
                        tn.c.upsert(ids, far)
                        tn.c.delete(ids)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        readers = [threading.Thread(target=reader, args=(i,), daemon=True) for i in range(4)]
        w = threading.Thread(target=writer, daemon=True)
        w.start()
        for t in readers:
            t.start()
        for t in readers:
            t.join(timeout=120)
        stop.set()
        w.join(timeout=30)
        assert not any(t.is_alive() for t in readers) and not w.is_alive(), "timed out: a group call or the writer hangs"
        assert not errors, errors
    finally:
        destroy(tenants)


# ---- the Python wrappers ------------------------------------------------------------------
@pytest.mark.gpu
def test_flat_search_by_vector_group(ctx, orc):
    from weaviate_amd.flat import AllowList, FlatIndex, SearchByVectorGroup

    d, k = 64, 5
    idx = [FlatIndex(ctx, d, "l2-squared", capacity=256, id_base=b) for b in (0, 640)]
    try:
        for i, ix in enumerate(idx):
            ix.AddBatch(np.arange(ix.vectors.id_base, ix.vectors.id_base + 200), orc.synth_rows(40 + i, 0, 200, d, 0))
        qs = orc.synth_rows(50, 0, 3, d, 0)
        allows = [None, AllowList(641, 650, 700), AllowList()]
        got = SearchByVectorGroup([idx[0], idx[1], idx[0]], qs, k, allows)
        for (gi, gd), ix, q, a in zip(got, [idx[0], idx[1], idx[0]], qs, allows):
            wi, wd = ix.SearchByVector(q, k, a)
            assert np.array_equal(gi, wi) and np.array_equal(bits(gd), bits(wd))
        assert len(got[1][0]) == 3 and len(got[2][0]) == 0
    finally:
        for ix in idx:
            ix.vectors.destroy()

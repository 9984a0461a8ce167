"""wvg_search_group_bq_rescore / wvg_search_group_bq_candidates: nq
flat.searchByVectorBQ calls (V/flat/index.go:347-389), query i against tenant i
(a BQ corpus and an F32 corpus), in three launches.  The outputs must be those of
nq separate wvg_search_bq_rescore / wvg_search_bq_candidates calls -- ids in
order, distance bits, counts and padding -- and the oracle's restatement of the
reference heaps (oracle/wv_oracle.c), ties at the R-th Hamming distance, the pop
order and the k-heap fed in pop order included.
"""
import ctypes
import threading

import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import KIND_BQ, KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_L2, ORDER_AVX256, ORDER_AVX512
from weaviate_amd.device import (Context, Corpus, allow_bitmap, search_bq_candidates, search_bq_rescore,
                                 search_group_bq_candidates, search_group_bq_rescore)

pytestmark = pytest.mark.gpu

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
ROWS = [0, 1, 63, 64, 65, 257, 1000, 5000]  # around the 64-row tile and the 256-row chunk; 5000 rows = 79 tiles
ID_BASES = [0, 64, 6400]
NQ = 24


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


class Tenant:
    """One tenant: its BQ and F32 corpora, the stored (normalized) host rows, their codes, the live mask."""

    def __init__(self, cx, orc, metric, d, n, id_base, spare, seed, rows=None):
        self.orc, self.metric, self.id_base, self.n, self.d = orc, metric, id_base, n, d
        cap = max(n + spare, 64)
        self.f = Corpus(cx, KIND_F32, metric, d, cap, id_base)
        self.b = Corpus(cx, KIND_BQ, metric, d, cap, id_base)
        self.ids = np.arange(id_base, id_base + n, dtype=np.uint64)
        self.rows = orc.synth_rows(seed, 0, n, d, 0) if rows is None else np.asarray(rows, np.float32)
        if n:
            self.f.upsert(self.ids, self.rows)
            self.b.upsert(self.ids, self.rows)
        self.stored = orc.normalize_rows(self.rows) if metric == METRIC_COSINE and n else self.rows
        self.codes = orc.bq_encode_rows(self.stored) if n else np.zeros((0, (d + 63) // 64), np.uint64)
        self.live = np.ones(n, bool)

    def delete(self, ids):
        ids = np.asarray(ids, np.uint64)
        self.f.delete(ids)
        self.b.delete(ids)
        self.live[(ids - np.uint64(self.id_base)).astype(np.int64)] = False

    def prep(self, q):
        return self.orc.normalize(q) if self.metric == METRIC_COSINE else np.asarray(q, np.float32)

    def valid(self, allowed=None):
        return (self.live if allowed is None else self.live & allowed).astype(np.uint8)

    def oracle_pops(self, q, R, allowed=None):
        """(global ids, Hamming distances) the reference heap of R pops, in pop order."""
        if self.n == 0:
            return np.empty(0, np.uint64), np.empty(0, np.float32)
        pi, pd = self.orc.bq_heap_pops(self.codes, self.orc.bq_encode(self.prep(q)), R, self.valid(allowed))
        return pi + np.uint64(self.id_base), pd

    def oracle_search(self, q, k, rl, allowed=None):
        """flat.searchByVectorBQ restated by the oracle: (global ids, distances)."""
        if self.n == 0:
            return np.empty(0, np.uint64), np.empty(0, np.float32)
        ri, rd = self.orc.flat_search_bq(self.stored, self.prep(q), k, rl, self.metric, self.valid(allowed))
        return ri + np.uint64(self.id_base), rd

    def destroy(self):
        self.f.destroy()
        self.b.destroy()


def make_tenants(cx, orc, metric, d, seed, rows=ROWS):
    return [Tenant(cx, orc, metric, d, n, ID_BASES[i % 3], 128 * (i % 2), seed + i) for i, n in enumerate(rows)]


def destroy(tenants):
    for t in tenants:
        t.destroy()


def shuffled_targets(seed, ntenants, nq=NQ):
    """Every tenant at least once, the last (largest) several times, in shuffled order."""
    rng = np.random.default_rng(seed)
    which = list(range(ntenants)) + [ntenants - 1] * 3
    which += list(rng.integers(0, ntenants, nq - len(which)))
    rng.shuffle(which)
    return [int(t) for t in which]


def assert_padded(ids, dists, counts, width):
    assert ids.shape == dists.shape == (len(counts), width)
    for i, c in enumerate(counts):
        assert np.all(ids[i, c:] == NONE) and np.all(np.isposinf(dists[i, c:])), i


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("ids", "dists", "counts")):
        g = bits(g) if g.dtype == np.float32 else g
        w = bits(w) if w.dtype == np.float32 else w
        assert np.array_equal(g, w), (what, name)


def check_rescore(tenants, which, qs, k, rl, allows=None, allowed=None, oracle=True):
    """The grouped rescore call == one search_bq_rescore per query (padding included) == the oracle."""
    got = search_group_bq_rescore([tenants[t].b for t in which], [tenants[t].f for t in which], qs, k, rl, allows)
    assert_padded(*got, k)
    for i, t in enumerate(which):
        a = None if allows is None else allows[i]
        if a is not None and len(a) == 0:
            want = (np.full((1, k), NONE), np.full((1, k), np.inf, np.float32), np.zeros(1, np.uint32))
        else:
            want = search_bq_rescore(tenants[t].b, tenants[t].f, qs[i], k, rl, a)
        assert_same([x[i:i + 1] for x in got], want, ("separate", i, t))
        if oracle:
            oi, od = tenants[t].oracle_search(qs[i], k, rl, None if allowed is None else allowed[i])
            c = int(got[2][i])
            assert c == len(oi), (i, t, c, len(oi))
            assert np.array_equal(got[0][i, :c], oi) and np.array_equal(bits(got[1][i, :c]), bits(od)), (i, t)
    return got


def check_candidates(tenants, which, qs, R, allows=None, allowed=None, separate=True):
    """The grouped candidates call == one search_bq_candidates per query == orc.bq_heap_pops."""
    got = search_group_bq_candidates([tenants[t].b for t in which], qs, R, allows)
    assert_padded(*got, R)
    for i, t in enumerate(which):
        a = None if allows is None else allows[i]
        if separate and not (a is not None and len(a) == 0):
            assert_same([x[i:i + 1] for x in got], search_bq_candidates(tenants[t].b, qs[i], R, a), ("separate", i, t))
        pi, pd = tenants[t].oracle_pops(qs[i], R, None if allowed is None else allowed[i])
        c = int(got[2][i])
        assert c == len(pi), (i, t, c, len(pi))
        assert np.array_equal(got[0][i, :c], pi) and np.array_equal(bits(got[1][i, :c]), bits(pd)), (i, t)
    return got


# ---- 1. equality with separate calls and with the oracle -----------------------------
# NCH 1, generic (2 chunks), 6, 12; then odd word counts (3 / 11 / 23 words) under the generic, 6 and 12 kernels
@pytest.mark.parametrize("d", [64, 200, 768, 1536, 130, 700, 1440])
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT, METRIC_COSINE])
def test_equals_separate_calls_and_oracle(ctx, orc, metric, d):
    tenants = make_tenants(ctx, orc, metric, d, 7000 + 13 * d + metric)
    try:
        which = shuffled_targets(d + metric, len(tenants))
        qs = orc.synth_rows(9100 + d + metric, 0, NQ, d, 0)
        check_rescore(tenants, which, qs, 10, 200)
        check_candidates(tenants, which, qs, 200)
    finally:
        destroy(tenants)


# ---- 2. heavy ties ------------------------------------------------------------------------
def test_heavy_ties_any_window(ctx, orc):
    """d = 64: Hamming distances 0..64, so every R-th distance is shared by many rows; R from 1
    to beyond the row count (and beyond 256, the scan top-k's limit elsewhere)."""
    d = 64
    tenants = make_tenants(ctx, orc, METRIC_L2, d, 510, rows=[300, 3000, 20_000])
    try:
        which = [2, 0, 1, 2, 1, 0]
        qs = orc.synth_rows(511, 0, len(which), d, 0)
        for R in (1, 7, 64, 200, 256, 257, 700, 3000):
            check_candidates(tenants, which, qs, R, separate=R in (200, 700))
    finally:
        destroy(tenants)


# ---- 3. ties in both heaps ------------------------------------------------------------------
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT])
def test_integer_rows_ties_in_both_heaps(ctx, orc, metric):
    n, d, k = 8000, 32, 10
    rows = orc.synth_rows(601, 0, n, d, 1) - np.float32(128)
    rows[5000:5100] = rows[17]  # exact duplicates: equal Hamming and equal exact distances
    big = Tenant(ctx, orc, metric, d, n, 64, 0, 0, rows=rows)
    small = Tenant(ctx, orc, metric, d, 300, 0, 0, 0, rows=rows[4900:5200])
    tenants = [big, small]
    try:
        qs = np.concatenate([orc.synth_rows(602, 0, 3, d, 1) - np.float32(128), rows[17:18], rows[17:18]])
        which = [0, 1, 0, 0, 1]  # the last two: a query equal to the duplicated row
        for rl in (200, 600):
            check_rescore(tenants, which, qs, k, rl)
    finally:
        destroy(tenants)


# ---- 4. chunk edges ---------------------------------------------------------------------
def test_chunk_edges_and_k_above_live_count(ctx, orc):
    """The filter's chunks are 256 rows: live row counts around one and two chunks, and a tenant
    whose deletes leave fewer than R = 200 live rows ahead of its second and third chunk (their
    threshold is still +inf)."""
    d = 64
    tenants = [Tenant(ctx, orc, METRIC_L2, d, n + 20, ID_BASES[i % 3], 0, 4400 + i)
               for i, n in enumerate([255, 256, 257, 511, 513])]
    sparse = Tenant(ctx, orc, METRIC_L2, d, 1100, 64, 0, 4410)
    tenants.append(sparse)
    try:
        rng = np.random.default_rng(44)
        for tn in tenants[:5]:
            tn.delete(tn.id_base + np.sort(rng.choice(tn.n, 20, replace=False)))
        gone = np.sort(rng.choice(512, 512 - 150, replace=False))  # 150 live rows in the first two chunks
        sparse.delete(sparse.id_base + gone)
        assert [int(t.live.sum()) for t in tenants[:5]] == [255, 256, 257, 511, 513]
        assert sparse.live[:256].sum() < 200 and sparse.live[:512].sum() == 150
        which = [0, 1, 2, 3, 4, 5, 5, 2]
        qs = orc.synth_rows(4420, 0, len(which), d, 0)
        check_rescore(tenants, which, qs, 10, 200)
        check_candidates(tenants, which, qs, 200)
        got = check_rescore(tenants, which, qs, 300, 200)  # k (= R) above the live rows of tenants 0..2
        assert got[2][:3].tolist() == [255, 256, 257]
    finally:
        destroy(tenants)


# ---- 5. per-query filters in one call ---------------------------------------------------
@pytest.mark.parametrize("deletes", [False, True])
def test_per_query_filters(ctx, orc, deletes):
    d, k, R = 128, 10, 200
    tenants = make_tenants(ctx, orc, METRIC_COSINE, d, 5500, rows=[5000, 1000, 257])
    try:
        rng = np.random.default_rng(55)
        if deletes:
            for tn in tenants:
                tn.delete(tn.id_base + np.sort(rng.choice(tn.n, tn.n // 10, replace=False)))
        which, allows, allowed = [], [], []

        def add(t, ids, words=None):
            tn = tenants[t]
            which.append(t)
            if ids is None:
                allows.append(None)
                allowed.append(None)
                return
            ids = np.asarray(ids, np.uint64)
            allows.append(allow_bitmap(ids) if words is None else words)
            m = np.zeros(tn.n, bool)
            loc = ids[(ids >= tn.id_base) & (ids < tn.id_base + tn.n)] - np.uint64(tn.id_base)
            m[loc.astype(np.int64)] = True
            allowed.append(m)

        for t, tn in enumerate(tenants):
            base, n = tn.id_base, tn.n
            add(t, base + rng.choice(n, max(1, n // 10), replace=False))   # a 10 % list
            add(t, [base + n // 2])                                        # a single id
            add(t, np.arange(base + n // 3, base + n // 3 + min(n // 2, 300)))  # a narrow window
            add(t, [], words=np.empty(0, np.uint64))                       # non-NULL, 0 words: nothing
            add(t, None)                                                   # no filter
            add(t, [base + n + 200, base + n + 4000])                      # no id of this tenant
        qs = orc.synth_rows(5600, 0, len(which), d, 0)
        got = check_rescore(tenants, which, qs, k, R, allows, allowed)
        check_candidates(tenants, which, qs, R, allows, allowed)
        assert got[2][3] == 0 and got[2][5] == 0 and got[2][4] == k  # the empty lists empty their own query only
    finally:
        destroy(tenants)


# ---- 6. many work items per tenant ------------------------------------------------------
def test_many_items_per_tenant(ctx, orc):
    """40 000 rows = 625 tiles = 79 work items at 8 tiles per item (the item rule of
    wvg_group.hip; the call's tile total stays far below 4 x CUs x 8) and 157 filter chunks."""
    d = 128
    small = make_tenants(ctx, orc, METRIC_L2, d, 6600, rows=[64, 300, 512])
    big = Tenant(ctx, orc, METRIC_L2, d, 40_000, 6400, 0, 6610)
    tenants = small + [big]
    try:
        which = [0, 3, 1, 2, 3, 0]
        qs = orc.synth_rows(6620, 0, len(which), d, 0)
        for rl in (200, 600):
            check_rescore(tenants, which, qs, 10, rl)
            check_candidates(tenants, which, qs, rl, separate=False)
    finally:
        destroy(tenants)


def test_records_beyond_the_head(ctx, orc):
    """Distances falling with the docID (128 - 128 i / n set bits against an all-zero query
    code): nearly every row beats the R-th distance of the rows before its chunk, so the filter
    keeps far more than the head of records copied back with the totals (1600 at R = 200) and
    the rest of that query's records comes in a second round -- beside a query that needs none."""
    from weaviate_amd.flat import group_bq_kept_rows

    n, d, R = 6000, 128, 200
    nb = 128 - (np.arange(n) * 128) // n
    codes = np.zeros((n, 2), np.uint64)
    for j in range(2):
        c = np.clip(nb - 64 * j, 0, 64)
        codes[:, j] = np.where(c >= 64, NONE, np.left_shift(np.uint64(1), np.minimum(c, 63).astype(np.uint64)) - np.uint64(1))
    falling = Corpus(ctx, KIND_BQ, METRIC_L2, d, n, 64)
    plain = Tenant(ctx, orc, METRIC_L2, d, 1000, 0, 0, 6900)
    try:
        falling.upsert_codes(np.arange(64, 64 + n, dtype=np.uint64), codes)
        assert group_bq_kept_rows(nb.astype(np.float32), None, R).sum() > 2 * 1600
        qs = np.ones((3, d), np.float32)  # code 0: distance = set bits
        qs[1] = orc.synth_rows(6901, 0, 1, d, 0)[0]
        ids, dists, counts = search_group_bq_candidates([falling, plain.b, falling], qs, R)
        assert_padded(ids, dists, counts, R)
        pi, pd = orc.bq_heap_pops(codes, np.zeros(2, np.uint64), R)
        for i in (0, 2):
            assert counts[i] == len(pi) == R
            assert np.array_equal(ids[i], pi + np.uint64(64)) and np.array_equal(bits(dists[i]), bits(pd))
        wi, wd = plain.oracle_pops(qs[1], R)
        assert np.array_equal(ids[1], wi) and np.array_equal(bits(dists[1]), bits(wd))
        assert_same([x[:1] for x in (ids, dists, counts)], search_bq_candidates(falling, qs[0], R), "separate")
    finally:
        falling.destroy()
        plain.destroy()


# ---- 7. the AVX-512 order -------------------------------------------------------------
def test_avx512_order(ctx, orc):
    metric, d, k, R = METRIC_L2, 768, 10, 200
    ctx.set_distance_order(ORDER_AVX512)
    try:
        tenants = make_tenants(ctx, orc, metric, d, 7700, rows=[1000, 65, 257])
        try:
            which = [2, 0, 1, 0]
            qs = orc.synth_rows(7710, 0, len(which), d, 0)
            got = check_rescore(tenants, which, qs, k, R, oracle=False)
            for i, t in enumerate(which):
                tn = tenants[t]
                pi, _ = tn.oracle_pops(qs[i], R)
                loc = (pi - np.uint64(tn.id_base)).astype(np.int64)
                d512 = orc.dist_all_512(metric, tn.prep(qs[i]), tn.stored[loc])
                wi, wd = orc.heap_topk(d512, pi, k)  # the k-heap fed in pop order
                c = int(got[2][i])
                assert c == len(wi)
                assert np.array_equal(got[0][i, :c], wi) and np.array_equal(bits(got[1][i, :c]), bits(wd)), i
        finally:
            destroy(tenants)
    finally:
        ctx.set_distance_order(ORDER_AVX256)


# ---- 8. validation ------------------------------------------------------------------------
def test_validation_leaves_outputs_untouched(ctx, orc):
    lib = ctx.lib
    d, k = 32, 4

    def pair(cx, metric=METRIC_L2, dim=d, base=0):
        return Corpus(cx, KIND_BQ, metric, dim, 64, base), Corpus(cx, KIND_F32, metric, dim, 64, base)

    a = pair(ctx)
    b = pair(ctx)
    other_dim = pair(ctx, dim=d + 4)
    other_metric = pair(ctx, metric=METRIC_DOT)
    other_base = pair(ctx, base=64)
    wide = pair(ctx, dim=8256)  # above the filter's LDS histogram
    ctx2 = Context(0)
    foreign = pair(ctx2)
    ctx0 = Context(0, heap_replay=0)
    lexi = pair(ctx0)
    everything = (a, b, other_dim, other_metric, other_base, wide, foreign, lexi)
    try:
        for p in (a, b):
            rows = orc.synth_rows(1, 0, 8, d, 0)
            for c in p:
                c.upsert(np.arange(8, dtype=np.uint64), rows)
        qs = orc.synth_rows(2, 0, 3, d, 0)
        wide_qs = orc.synth_rows(3, 0, 3, 8256, 0)

        def call(bqs, f32s, kk=k, queries=qs, cand=False, allow_no_words=False):
            w = max(kk, 1)
            ids = np.full((3, w), 0x1234, np.uint64)
            dists = np.full((3, w), -7.0, np.float32)
            counts = np.full(3, 99, np.uint32)
            hb = (ctypes.c_void_p * 3)(*[c.handle if c is not None else None for c in bqs]) if bqs else None
            hf = (ctypes.c_void_p * 3)(*[c.handle if c is not None else None for c in f32s]) if f32s else None
            qp = _lib.fptr(queries) if queries is not None else None
            ap = None
            if allow_no_words:
                word = np.ones(1, np.uint64)
                ap = (ctypes.c_void_p * 3)(None, word.ctypes.data, None)
            if cand:
                rc = lib.wvg_search_group_bq_candidates(hb, qp, 3, kk, ap, None, _lib.u64ptr(ids), _lib.fptr(dists),
                                                        _lib.u32ptr(counts))
            else:
                rc = lib.wvg_search_group_bq_rescore(hb, hf, qp, 3, kk, 2 * kk, ap, None, _lib.u64ptr(ids),
                                                     _lib.fptr(dists), _lib.u32ptr(counts))
            msg = lib.wvg_last_error().decode()
            untouched = bool(np.all(ids == 0x1234) and np.all(dists == -7.0) and np.all(counts == 99))
            return rc, msg, untouched

        B, F = 0, 1
        ok = [a, b, a]
        assert call([p[B] for p in ok], [p[F] for p in ok])[0] == _lib.WVG_OK
        assert call([p[B] for p in ok], None, cand=True)[0] == _lib.WVG_OK
        INV, UNS = _lib.WVG_ERR_INVALID, _lib.WVG_ERR_UNSUPPORTED
        cases = [
            # (bq list, f32 list, kwargs, code, word in the message)
            ([a[B], a[F], b[B]], [a[F], b[F], b[F]], {}, INV, "bq[1]"),              # an F32 corpus as bq[1]
            ([a[B], b[B], a[B]], [a[F], b[F], b[B]], {}, INV, "f32[2]"),             # a BQ corpus as f32[2]
            ([a[B], other_dim[B], b[B]], [a[F], other_dim[F], b[F]], {}, INV, "bq[1]"),
            ([a[B], b[B], a[B]], [a[F], other_dim[F], a[F]], {}, INV, "f32[1]"),
            ([a[B], b[B], other_metric[B]], [a[F], b[F], other_metric[F]], {}, INV, "bq[2]"),
            ([a[B], b[B], a[B]], [a[F], b[F], other_metric[F]], {}, INV, "f32[2]"),
            ([a[B], foreign[B], b[B]], [a[F], foreign[F], b[F]], {}, INV, "bq[1]"),
            ([a[B], b[B], a[B]], [a[F], foreign[F], a[F]], {}, INV, "f32[1]"),
            ([a[B], b[B], a[B]], [a[F], other_base[F], a[F]], {}, INV, "f32[1]"),    # id_base of bq[1] and f32[1]
            ([a[B], None, b[B]], [a[F], b[F], b[F]], {}, INV, "bq[1]"),
            ([a[B], b[B], a[B]], [a[F], b[F], None], {}, INV, "f32[2]"),
            ([a[B], b[B], a[B]], [a[F], b[F], a[F]], {"queries": None}, INV, "queries"),
            ([a[B], b[B], a[B]], None, {}, INV, "f32"),
            ([a[B], b[B], a[B]], [a[F], b[F], a[F]], {"allow_no_words": True}, INV, "allow_bits[1]"),
            ([lexi[B]] * 3, [lexi[F]] * 3, {}, UNS, "heap_replay"),
            ([wide[B]] * 3, [wide[F]] * 3, {"queries": wide_qs}, UNS, "8192"),
            # the candidates form
            ([a[B], a[F], b[B]], None, {"cand": True}, INV, "bq[1]"),
            ([a[B], other_dim[B], b[B]], None, {"cand": True}, INV, "bq[1]"),
            ([a[B], b[B], foreign[B]], None, {"cand": True}, INV, "bq[2]"),
            ([a[B], b[B], a[B]], None, {"cand": True, "queries": None}, INV, "queries"),
            ([lexi[B]] * 3, None, {"cand": True}, UNS, "heap_replay"),
            ([wide[B]] * 3, None, {"cand": True, "queries": wide_qs}, UNS, "8192"),
        ]
        for bqs, f32s, kw, code, word in cases:
            rc, msg, untouched = call(bqs, f32s, **kw)
            assert rc == code, (rc, msg, word)
            assert msg and word in msg, (msg, word)
            assert untouched, msg
        # nq = 0 is a no-op; k = 0 (R = 0 for the candidates) writes the counts only
        assert lib.wvg_search_group_bq_rescore(None, None, None, 0, k, 8, None, None, None, None, None) == _lib.WVG_OK
        assert lib.wvg_search_group_bq_candidates(None, None, 0, 8, None, None, None, None, None) == _lib.WVG_OK
        assert search_group_bq_rescore([a[B], b[B]], [a[F], b[F]], qs[:2], 0, 0)[2].tolist() == [0, 0]
        assert search_group_bq_candidates([a[B], b[B]], qs[:2], 0)[2].tolist() == [0, 0]
        # k without a 256 cap (the k-heap runs on the host): 8 rows, k = 300
        ids, dists, counts = search_group_bq_rescore([a[B], b[B]], [a[F], b[F]], qs[:2], 300, 0)
        assert counts.tolist() == [8, 8] and np.all(ids[:, 8:] == NONE)
    finally:
        for p in everything:
            for c in p:
                c.destroy()
        ctx2.close()
        ctx0.close()


# ---- 9. the call's cost does not depend on nq -----------------------------------------
def test_one_scan_launch_per_call(ctx, orc):
    d = 64
    tenants = make_tenants(ctx, orc, METRIC_L2, d, 9900, rows=[300, 1000, 65])
    try:
        lib = ctx.lib
        for nq in (1, 24):
            which = [i % 3 for i in range(nq)]
            qs = orc.synth_rows(9910, 0, nq, d, 0)
            bqs, f32s = [tenants[t].b for t in which], [tenants[t].f for t in which]
            for run in (lambda: search_group_bq_rescore(bqs, f32s, qs, 10, 200),
                        lambda: search_group_bq_candidates(bqs, qs, 200)):
                _lib.check(lib.wvg_profile_start(ctx.handle))
                run()
                run()
                ms, nl = ctypes.c_double(), ctypes.c_uint64()
                _lib.check(lib.wvg_profile_stop(ctx.handle, ctypes.byref(ms), ctypes.byref(nl)))
                assert nl.value == 2, (nq, nl.value)  # one scan launch per call
                assert ms.value > 0
    finally:
        destroy(tenants)


# ---- 10. concurrency ------------------------------------------------------------------
def test_concurrent_groups_and_writers(ctx, orc):
    """Group calls over overlapping tenant sets in different orders while a writer upserts rows
    into both corpora of two tenants and deletes them again.  The written rows are the negated
    query direction scaled up: the largest Hamming distance and exact distance there is, so a
    state with them holds the same candidates and the same top-k as the state without; every
    result is the static one, and nothing deadlocks (one global lock order over BQ and F32)."""
    d, k, R, calls = 64, 10, 50, 40
    tenants = make_tenants(ctx, orc, METRIC_L2, d, 8800, rows=[500, 257, 1000, 300, 65, 700])
    try:
        for tn in tenants:  # room for the writer's rows without a reallocation changing the race
            tn.f.reserve(tn.n + 64)
            tn.b.reserve(tn.n + 64)
        orders = [[0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [2, 0, 5, 1, 0, 2], [3, 5, 1, 4, 2, 3]]
        q0 = np.abs(orc.synth_rows(60, 0, 1, d, 0)[0]) + np.float32(0.5)  # every query: all components positive
        qs = [np.abs(orc.synth_rows(61 + i, 0, len(o), d, 0)) + np.float32(0.5) for i, o in enumerate(orders)]
        far = np.tile(-1e3 * q0, (4, 1)).astype(np.float32)  # code all ones vs the queries' all zeros: Hamming d
        want = [search_group_bq_rescore([tenants[t].b for t in o], [tenants[t].f for t in o], q, k, R)
                for o, q in zip(orders, qs)]
        for o, q, w in zip(orders, qs, want):
            for i, t in enumerate(o):
                oi, od = tenants[t].oracle_search(q[i], k, R)
                assert np.array_equal(w[0][i, :len(oi)], oi) and np.array_equal(bits(w[1][i, :len(oi)]), bits(od))
        errors, stop = [], threading.Event()

        def reader(i):
            try:
                bqs, f32s = [tenants[t].b for t in orders[i]], [tenants[t].f for t in orders[i]]
                for _ in range(calls):
                    got = search_group_bq_rescore(bqs, f32s, qs[i], k, R)
                    for g, w in zip(got, want[i]):
                        if not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
                            raise AssertionError(f"reader {i}: a result changed")
            except Exception as e:  # noqa: BLE001 -- reported by the main thread
                errors.append(e)

        def writer():
            try:
                while not stop.is_set():
                    for t in (0, 2):
                        tn = tenants[t]
                        ids = np.arange(tn.id_base + tn.n, tn.id_base + tn.n + 4, dtype=np.uint64)  # the spare rows
                        tn.b.upsert(ids, far)
                        tn.f.upsert(ids, far)
                        tn.f.delete(ids)
                        tn.b.delete(ids)
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


# ---- 11. the Python wrappers ------------------------------------------------------------
def test_flat_search_by_vector_group_bq(ctx, orc):
    from weaviate_amd.flat import AllowList, FlatIndex, SearchByVectorGroup

    d, k = 64, 5
    idx = [FlatIndex(ctx, d, "l2-squared", compression="bq", rescore_limit=40, capacity=256, id_base=b)
           for b in (0, 640)]
    plain = FlatIndex(ctx, d, "l2-squared", capacity=64)
    try:
        for i, ix in enumerate(idx):
            ix.AddBatch(np.arange(ix.vectors.id_base, ix.vectors.id_base + 200), orc.synth_rows(40 + i, 0, 200, d, 0))
        qs = orc.synth_rows(50, 0, 3, d, 0)
        allows = [None, AllowList(641, 650, 700), AllowList()]
        got = SearchByVectorGroup([idx[0], idx[1], idx[0]], qs, k, allows)
        for (gi, gd), ix, q, a in zip(got, [idx[0], idx[1], idx[0]], qs, allows):
            wi, wd = ix.SearchByVector(q, k, a)
            assert np.array_equal(gi, wi) and np.array_equal(bits(gd), bits(wd))
        assert len(got[0][0]) == k and len(got[1][0]) == 3 and len(got[2][0]) == 0
        with pytest.raises(ValueError):  # mixed lists still raise
            SearchByVectorGroup([idx[0], plain], qs[:2], k)
    finally:
        for ix in idx + [plain]:
            ix.vectors.destroy()
            if ix.bq is not None:
                ix.bq.destroy()

"""K8, the ADC scan for any (m, ks), at the segment counts Weaviate itself
picks (calculateOptimalSegments: 128-d -> 64, 384-d -> 96, 512 / 768-d -> 128,
1024 / 1536-d -> 256, all with ks = 256) and at every size where the kernel
takes another path, bit for bit against the oracle's LookUp
(CH/product_quantization.go:85-104, PQDistancer.Distance :352-361).

Paths: the fixed-M forms scan_pq_kernel<E, 8|16|64, 256> with their two-tile
prefetch pipeline (many tiles per wave, dead runs at the start, in the middle
and at the end of a wave's range, E = 1 / 2 / 4); the generic <E, 0, 0> form
(m < 16, partial chunks, the rotated m = 32 storage with ks < 256, m >= 96);
and its global-LUT form, taken where the m x ks fp32 LUT does not fit in LDS
beside the workgroup top-k buffer (8 / 16 / 32 KiB for k <= 64 / 128 / 256:
at ks = 256 the LDS form ends at m = 152 / 144 / 128).  ordkeys_pq_kernel
(k > 256, search_by_distance) has the same two forms.

Codes are loaded as given (upsert_codes), so a wrong scan cannot hide behind a
wrong encode; the encoder is pinned separately at ds = 2 and ds = 6.

The reference distance of every row is `adc_all` (one np.float32 add per
segment, in segment order, then Wrap), pinned here to orc.pq_adc.  check_topk
gets the live, allowed rows whose distance is <= the K-th smallest of them
(K >= every k asked): a set that holds the whole lexicographic top-k and every
row tied at its boundary, so both of check_topk's comparisons are what they
would be over all rows, without sorting 300k rows per call.
"""
import functools

import numpy as np
import pytest

from weaviate_amd._lib import (KIND_PQ, METRIC_COSINE, METRIC_DOT, METRIC_HAMMING, METRIC_L2, METRIC_MANHATTAN)
from weaviate_amd.device import Corpus, allow_bitmap

from test_gpu_parity import ORC_METRIC, bits, check_topk

pytestmark = pytest.mark.gpu

ORC = dict(ORC_METRIC)
ORC.update({METRIC_MANHATTAN: 3, METRIC_HAMMING: 4})


def adc_all(metric, lut, codes):
    """Sequential fp32 sum over segments for every row (vectorised over rows; the
    per-row order is the reference's) + Wrap (dot: -x, cosine: 1 - x)."""
    s = np.zeros(len(codes), np.float32)
    for i in range(lut.shape[0]):
        s = (s + lut[i, codes[:, i]]).astype(np.float32)
    if metric == 1:
        return (-s).astype(np.float32)
    if metric == 2:
        return (np.float32(1.0) - s).astype(np.float32)
    return s


def _centers(orc, seed, m, ks, ds, metric=METRIC_L2):
    if metric == METRIC_HAMMING:  # repeated integer values: equal elements are what hamming counts
        return np.floor(orc.synth_rows(seed, 0, m * ks, ds, 1) / 64).astype(np.float32).reshape(m, ks, ds)
    return orc.synth_rows(seed, 0, m * ks, ds, 0).reshape(m, ks, ds)


def _queries(orc, seed, nq, d, metric=METRIC_L2):
    if metric == METRIC_HAMMING:
        return np.floor(orc.synth_rows(seed, 0, nq, d, 1) / 64).astype(np.float32)
    return orc.synth_rows(seed, 0, nq, d, 0)


def _lut(orc, metric, q, centers):
    """The LUT the host API builds: cosine queries are normalized first."""
    return orc.pq_lut(ORC[metric], orc.normalize(q) if metric == METRIC_COSINE else q, centers)


def _all_d(orc, metric, qs, centers, codes):
    return [adc_all(ORC[metric], _lut(orc, metric, q, centers), codes) for q in qs]


def _near(all_d, mask, kmax):
    """(dists, ids) of the rows of `mask` no farther than the kmax-th nearest of them."""
    idx = np.flatnonzero(mask)
    d = all_d[idx]
    if len(d) > kmax:
        keep = d <= np.partition(d, kmax - 1)[kmax - 1]
        idx, d = idx[keep], d[keep]
    return d, idx.astype(np.uint64)


def _check(orc, res, refs, k):
    ids, dists, counts = res
    assert len(counts) == len(refs)
    for qi, (d, i) in enumerate(refs):
        check_topk(orc, ids[qi], dists[qi], counts[qi], d, i, k)


def _same(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


def _corpus(ctx, metric, centers, codes, deleted):
    m, _, ds = centers.shape
    n = len(codes)
    c = Corpus(ctx, KIND_PQ, metric, m * ds, n)
    c.set_codebook(centers)
    c.upsert_codes(np.arange(n, dtype=np.uint64), codes)
    c.delete(deleted)
    return c


@functools.lru_cache(maxsize=None)
def _third(n):
    """An allow list of every third id: (bitmap, row mask)."""
    am = np.zeros(n, bool)
    am[::3] = True
    return allow_bitmap(np.arange(0, n, 3, dtype=np.uint64), n), am


@functools.lru_cache(maxsize=None)
def _every(n):
    return allow_bitmap(np.arange(n, dtype=np.uint64))


# ---------------------------------------------------------------------------
# the reference itself
@pytest.mark.parametrize("metric,m,ks,ds", [(METRIC_L2, 64, 256, 2), (METRIC_DOT, 96, 256, 4),
                                            (METRIC_COSINE, 256, 256, 6), (METRIC_MANHATTAN, 64, 256, 2),
                                            (METRIC_HAMMING, 64, 256, 2), (METRIC_L2, 32, 255, 4)])
def test_adc_all_is_the_oracle_rowwise(orc, metric, m, ks, ds):
    rng = np.random.default_rng(1000 + m + ks)
    codes = rng.integers(0, ks, (200, m), dtype=np.uint8)
    centers = _centers(orc, 1001, m, ks, ds, metric)
    q = _queries(orc, 1002, 1, m * ds, metric)[0]
    lut = _lut(orc, metric, q, centers)
    want = np.array([orc.pq_adc(ORC[metric], lut, cd) for cd in codes], np.float32)
    assert np.array_equal(bits(adc_all(ORC[metric], lut, codes)), bits(want))


# ---------------------------------------------------------------------------
# the fixed-M prefetch pipeline
N_PIPE = 300_037  # 4688 full tiles and a 5-row tail: ~4.6 tiles per wave for a 4-query batch, 1-2 for one query
_pipe_codes = {}


@pytest.fixture(scope="module")
def pipe_dead():
    """Dead runs at the start, in the middle and at the end of waves' ranges."""
    rng = np.random.default_rng(1100)
    full = N_PIPE // 64
    deleted = np.concatenate([np.arange(64 * 10, 64 * 40), np.arange(64 * 2000, 64 * 2300),
                              np.arange(64 * (full - 3), 64 * full), rng.choice(N_PIPE, 3000, replace=False)])
    deleted = np.unique(deleted).astype(np.uint64)
    valid = np.ones(N_PIPE, bool)
    valid[deleted.astype(np.int64)] = False
    return deleted, valid


def _pipe(m):
    if m not in _pipe_codes:
        codes = np.random.default_rng(1101 + m).integers(0, 256, (N_PIPE, m), dtype=np.uint8)
        codes[6400:6464] = codes[6400]  # a tile of identical rows (ties)
        _pipe_codes[m] = codes
    return _pipe_codes[m]


@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT, METRIC_COSINE])
@pytest.mark.parametrize("m,ds", [(8, 4), (16, 2), (64, 2)])
def test_fixed_m_pipeline(ctx, orc, pipe_dead, m, ds, metric):
    deleted, valid = pipe_dead
    codes = _pipe(m)
    centers = _centers(orc, 1110 + m, m, 256, ds)
    qs = _queries(orc, 1111 + m, 4, m * ds)
    third, am = _third(N_PIPE)
    every = _every(N_PIPE)
    all_d = _all_d(orc, metric, qs, centers, codes)
    ref = [_near(d, valid, 256) for d in all_d]
    ref3 = [_near(d, valid & am, 256) for d in all_d]
    c = _corpus(ctx, metric, centers, codes, deleted)
    try:
        for k in (10, 100, 256):  # E = 1, 2, 4
            batch = c.search(qs, k)
            singles = [c.search(qs[i], k) for i in range(len(qs))]
            single = tuple(np.concatenate([x[j] for x in singles]) for j in range(3))
            _check(orc, batch, ref, k)
            _check(orc, single, ref, k)
            _same(batch, single)
            _check(orc, c.search(qs, k, allow=third), ref3, k)
            _check(orc, c.search(qs, k, allow=every), ref, k)
    finally:
        c.destroy()


def test_fixed_m_pipeline_all_inf(ctx, orc, pipe_dead):
    """Segment 0 of the LUT is +inf for every centroid: every row ties at inf
    and the ids come back in docID order."""
    deleted, valid = pipe_dead
    m, ds = 64, 2
    codes = _pipe(m)
    centers = _centers(orc, 1110 + m, m, 256, ds)
    qs = _queries(orc, 1120, 4, m * ds).copy()
    qs[:, :2] = 3e19  # (3e19 - c)^2 overflows
    assert np.all(np.isposinf(orc.pq_lut(0, qs[0], centers)[0]))
    all_d = _all_d(orc, METRIC_L2, qs, centers, codes)
    ref = [_near(d, valid, 256) for d in all_d]
    live = np.flatnonzero(valid).astype(np.uint64)
    c = _corpus(ctx, METRIC_L2, centers, codes, deleted)
    try:
        for k in (10, 100, 256):
            batch = c.search(qs, k)
            single = c.search(qs[1], k)
            _check(orc, batch, ref, k)
            _check(orc, single, ref[1:2], k)
            for res in (batch, single):
                assert np.all(res[2] == k) and np.all(res[0] == live[:k]) and np.all(np.isposinf(res[1]))
    finally:
        c.destroy()


# ---------------------------------------------------------------------------
# the generic form and the LDS boundary
N_GEN = 20_037
SHAPES = [(4, 256, 2),     # m < 16: the s < m guard
          (24, 256, 4),    # a partial second chunk
          (32, 64, 4),     # rotated storage through <E, 0, 0>
          (32, 255, 4),
          (64, 16, 2),     # ks != 256 at a fixed-M count
          (96, 256, 4),    # Weaviate's 384-d default
          (128, 256, 6),   # 768-d default: 128 KiB LUT, exactly full at E = 4
          (144, 256, 2),   # LDS at k = 10 and 100, global at k = 200
          (152, 256, 2),   # LDS only at k <= 64
          (160, 256, 2),   # never in LDS
          (256, 256, 4),   # 1024-d default
          (256, 256, 6)]   # 1536-d default
_gen_codes = {}


@pytest.fixture(scope="module")
def gen_dead():
    rng = np.random.default_rng(1200)
    deleted = np.unique(np.concatenate([np.arange(64 * 3, 64 * 7), rng.choice(N_GEN, 300, replace=False)]))
    valid = np.ones(N_GEN, bool)
    valid[deleted] = False
    return deleted.astype(np.uint64), valid


def _gen(m, ks):
    if (m, ks) not in _gen_codes:
        codes = np.random.default_rng(1201 + 1000 * m + ks).integers(0, ks, (N_GEN, m), dtype=np.uint8)
        codes[576:640] = codes[576]  # a tile of identical rows (ties)
        _gen_codes[(m, ks)] = codes
    return _gen_codes[(m, ks)]


def _cases():
    out = [(m, ks, ds, metric) for (m, ks, ds) in SHAPES for metric in (METRIC_L2, METRIC_DOT)]
    out += [(m, ks, ds, METRIC_COSINE) for (m, ks, ds) in SHAPES if m in (128, 256)]
    out += [(64, 256, 2, METRIC_MANHATTAN), (64, 256, 2, METRIC_HAMMING)]
    return out


@pytest.mark.parametrize("m,ks,ds,metric", _cases())
def test_any_m_ks(ctx, orc, gen_dead, m, ks, ds, metric):
    deleted, valid = gen_dead
    codes = _gen(m, ks)
    centers = _centers(orc, 1210 + m + ks, m, ks, ds, metric)
    qs = _queries(orc, 1211 + m + ks, 4, m * ds, metric).copy()
    if metric == METRIC_HAMMING:
        qs[0, 5] = np.nan  # Step counts a NaN (Go's !=)
    third, am = _third(N_GEN)
    all_d = _all_d(orc, metric, qs, centers, codes)
    ref = [_near(d, valid, 200) for d in all_d]
    ref3 = [_near(d, valid & am, 200) for d in all_d]
    c = _corpus(ctx, metric, centers, codes, deleted)
    try:
        for k in (10, 100, 200):
            _check(orc, c.search(qs, k), ref, k)
            _check(orc, c.search(qs, k, allow=third), ref3, k)
    finally:
        c.destroy()


@pytest.mark.parametrize("m,ks,ds", [(24, 256, 4), (144, 256, 2), (256, 256, 6)])
def test_unbounded_selection_both_sides_of_the_lds_limit(ctx, orc, gen_dead, m, ks, ds):
    """ordkeys_pq_kernel: k > 256 and search_by_distance, LUT in LDS (m = 24,
    144) and in global memory (m = 256)."""
    deleted, valid = gen_dead
    codes = _gen(m, ks)
    centers = _centers(orc, 1210 + m + ks, m, ks, ds)
    qs = _queries(orc, 1220 + m, 2, m * ds)
    live = np.flatnonzero(valid).astype(np.uint64)
    for metric in (METRIC_L2, METRIC_DOT):
        all_d = _all_d(orc, metric, qs, centers, codes)
        c = _corpus(ctx, metric, centers, codes, deleted)
        try:
            _check(orc, c.search(qs, 300), [_near(d, valid, 300) for d in all_d], 300)
            for qi in range(len(qs)):
                ld = all_d[qi][valid]
                target = np.sort(ld)[49]
                gi, gd = c.search_by_distance(qs[qi], target, -1)
                ei, ed = orc.search_by_distance(lambda total: orc.lex_topk(ld, live, total), target, -1)
                assert len(ei) >= 50
                assert np.array_equal(gi, ei) and np.array_equal(bits(gd), bits(ed))
        finally:
            c.destroy()


def test_distance_by_ids_at_256_segments(ctx, orc, gen_dead):
    deleted, valid = gen_dead
    m, ks, ds = 256, 256, 6
    codes = _gen(m, ks)
    centers = _centers(orc, 1210 + m + ks, m, ks, ds)
    q = _queries(orc, 1230, 1, m * ds)[0]
    rng = np.random.default_rng(1231)
    ids = np.concatenate([rng.choice(N_GEN, 440, replace=False), deleted[:40].astype(np.int64),
                          np.arange(N_GEN, N_GEN + 20)]).astype(np.uint64)
    rng.shuffle(ids)
    want_ok = (ids < N_GEN) & valid[np.minimum(ids, N_GEN - 1).astype(np.int64)]
    for metric in (METRIC_L2, METRIC_COSINE):
        all_d = _all_d(orc, metric, [q], centers, codes)[0]
        c = _corpus(ctx, metric, centers, codes, deleted)
        try:
            dists, ok = c.distance_by_ids(q, ids)
            assert np.array_equal(ok, want_ok) and 0 < want_ok.sum() < len(ids)
            assert np.array_equal(bits(dists[ok]), bits(all_d[ids[ok].astype(np.int64)]))
            assert np.all(dists[~ok] == 0)
        finally:
            c.destroy()


# ---------------------------------------------------------------------------
# the encoder at ds = 2 and ds = 6, and a search over what it stored
@pytest.mark.parametrize("m,ks,ds", [(64, 256, 2), (128, 256, 6), (256, 256, 6)])
def test_encode_then_search(ctx, orc, m, ks, ds):
    n, d = 1000, m * ds
    centers = _centers(orc, 1300 + m, m, ks, ds)
    rows = orc.synth_rows(1301 + m, 0, n, d, 0)
    rows[:3] = centers[np.arange(m), 7].reshape(d)  # exact hits
    qs = _queries(orc, 1302 + m, 2, d)
    c = Corpus(ctx, KIND_PQ, METRIC_L2, d, n)
    try:
        c.set_codebook(centers)
        c.upsert(np.arange(n, dtype=np.uint64), rows)
        got, ok = c.get_batch(np.arange(n, dtype=np.uint64), pq_m=m)
        assert ok.all()
        assert np.array_equal(got, orc.pq_encode(rows, centers))
        all_d = _all_d(orc, METRIC_L2, qs, centers, got)
        _check(orc, c.search(qs, 10), [_near(dd, np.ones(n, bool), 10) for dd in all_d], 10)
    finally:
        c.destroy()

"""wvg_search_group over PQ tenants (wvg_group_pq.hip): query i against tenant i's
codes with tenant i's OWN codebook, equal -- ids, distance bits, counts, padding --
to Corpus.search per tenant and to the oracle's lexicographic top-k of adc_all.

scan_pq_group_kernel<E, NC, GL>: E = 1 / 2 / 4 for k <= 64 / 128 / 256; NC = m / 16
for m in {16, 32, 64, 96, 128}, else 0 (generic); GL = the generic form reading the
LUT in global memory where it does not fit in 160 KiB beside the 16-wave combine
buffer (at ks = 256 the LDS form ends at m = 152 / 128 for E = 1 / 4).
tests/test_group_pq_descriptors.py compares kernel_forms() with the library.
Items are at most 32 tiles here (group_pq_item_tiles): 9000 rows are five or more.
"""
import ctypes

import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import (KIND_BQ, KIND_F32, KIND_PQ, METRIC_COSINE, METRIC_DOT, METRIC_L2, METRIC_MANHATTAN)
from weaviate_amd.device import Corpus, allow_bitmap, search_group

from test_gpu_group import ID_BASES, NQ, assert_equals_oracle, assert_equals_separate, destroy, oracle_distances
from test_gpu_group import Tenant as F32Tenant, shuffled_targets
from test_gpu_pq_k8_matrix import ORC, _centers, _lut, _queries, adc_all

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 63, 64, 65, 257, 1000, 5000, 9000]
KS = (1, 10, 100, 256)
SHAPES = [(8, 256, 4),     # a partial chunk: generic
          (16, 16, 2),     # small ks
          (32, 256, 4),    # rotated storage
          (32, 255, 4),
          (64, 256, 2),    # NC = 4
          (96, 256, 2),    # NC = 6
          (128, 256, 2),   # NC = 8: a 128 KiB LUT, the last LDS form at E = 4
          (129, 256, 2),   # generic: LDS at E = 1, 2, global at E = 4
          (152, 256, 2),   # the last LDS form at E = 1
          (153, 256, 2),   # global at every E
          (160, 256, 2)]
MORE_METRICS = [(32, 256, 4), (64, 256, 2)]


def kernel_forms():
    """The (E, NC, GL) instantiations test_equals_separate_calls reaches."""
    out = set()
    for (m, ks, _), e in ((s, 1 if k <= 64 else (2 if k <= 128 else 4)) for s in SHAPES for k in KS):
        nc = m // 16 if m % 16 == 0 and m // 16 in (1, 2, 4, 6, 8) else 0
        out.add((e, nc, m * ks * 4 + (8 if 1 <= nc <= 4 else 16) * 64 * e * 8 > 160 * 1024))
    return out


class Tenant(F32Tenant):
    """A PQ corpus with a codebook of its own, its host codes and live mask (delete / oracle: the F32 tenant's)."""

    def __init__(self, cx, orc, metric, m, ks, ds, rows, id_base, spare, seed):
        self.orc, self.metric, self.id_base, self.n = orc, metric, id_base, rows
        self.centers = _centers(orc, seed, m, ks, ds, metric)
        self.codes = np.random.default_rng(seed).integers(0, ks, (rows, m), dtype=np.uint8)
        self.c = Corpus(cx, KIND_PQ, metric, m * ds, max(rows + spare, 64), id_base)
        self.c.set_codebook(self.centers)
        self.ids = np.arange(id_base, id_base + rows, dtype=np.uint64)
        if rows:
            self.c.upsert_codes(self.ids, self.codes)
        self.live = np.ones(rows, bool)

    def distances(self, q, _=None):
        return adc_all(ORC[self.metric], _lut(self.orc, self.metric, q, self.centers), self.codes)


def make_tenants(cx, orc, metric, m, ks, ds, seed, rows=ROWS):
    ts = [Tenant(cx, orc, metric, m, ks, ds, n, ID_BASES[i % 3], 128 * (i % 2), seed + i) for i, n in enumerate(rows)]
    for tn in ts:  # scattered deletes, the last row and, from 192 rows on, one whole tile
        b, n = tn.id_base, tn.n
        if n >= 65:
            tn.delete(sorted({b, b + 7, b + 63, b + n // 2, b + n - 1} | (set(range(b + 64, b + 128)) if n >= 192 else set())))
    return ts


CASES = [(*s, METRIC_L2) for s in SHAPES] + [(*s, mt) for s in MORE_METRICS
                                             for mt in (METRIC_DOT, METRIC_COSINE, METRIC_MANHATTAN)]


@pytest.mark.parametrize("m,ks,ds,metric", CASES)
def test_equals_separate_calls(ctx, orc, m, ks, ds, metric):
    tenants = make_tenants(ctx, orc, metric, m, ks, ds, 7000 + 13 * m + ks + metric)
    try:
        which = shuffled_targets(m + ks + metric, len(tenants))
        qs = _queries(orc, 9100 + m + metric, NQ, m * ds, metric)
        all_d = oracle_distances(tenants, which, qs)
        for k in KS:  # k above the rows of the small tenants
            res = assert_equals_separate(tenants, which, qs, k)
            assert_equals_oracle(tenants, which, all_d, k, res)
    finally:
        destroy(tenants)


@pytest.mark.parametrize("m,ks,ds", MORE_METRICS)
def test_per_query_filters(ctx, orc, m, ks, ds):
    tenants = make_tenants(ctx, orc, METRIC_L2, m, ks, ds, 7700 + m, rows=[9000, 1000, 257, 0])
    try:
        which, allows, allowed = [], [], []
        for t, tn in enumerate(tenants):
            b, n = tn.id_base, tn.n
            outside = [b + n + 200, b + n + 4000] + ([0, b - 1] if b else [])  # beyond / before the docID window
            for ids in (None, np.arange(b, b + n, 3), np.arange(b, b + n), [], outside):
                which.append(t)
                if ids is None:
                    allows.append(None)
                    allowed.append(None)
                    continue
                ids = np.asarray(ids, np.uint64)
                allows.append(allow_bitmap(ids) if len(ids) else np.empty(0, np.uint64))
                mask = np.zeros(n, bool)
                mask[(ids[(ids >= b) & (ids < b + n)] - np.uint64(b)).astype(np.int64)] = True
                allowed.append(mask)
        qs = _queries(orc, 7800 + m, len(which), m * ds)
        for k in (10, 256):
            res = assert_equals_separate(tenants, which, qs, k, allows)
            assert_equals_oracle(tenants, which, oracle_distances(tenants, which, qs), k, res, allowed)
        assert res[2][3] == 0 and res[2][4] == 0 and res[2][2] == 256
    finally:
        destroy(tenants)


def test_ties_come_back_in_docid_order(ctx, orc):
    m, ks, ds = 64, 256, 2
    tenants = make_tenants(ctx, orc, METRIC_L2, m, ks, ds, 8100, rows=[9000, 300])
    try:
        big = tenants[0]
        big.codes[6400:6464] = big.codes[6400]  # a tile of identical codes
        big.c.upsert_codes(big.ids[6400:6464], big.codes[6400:6464])
        which = [0, 1, 0]
        qs = _queries(orc, 8200, len(which), m * ds).copy()
        qs[2, :ds] = 3e19  # (3e19 - c)^2 overflows: LUT segment 0 is +inf, every row ties at +inf
        assert np.all(np.isposinf(_lut(orc, METRIC_L2, qs[2], big.centers)[0]))
        all_d = oracle_distances(tenants, which, qs)
        for k in (10, 100, 256):
            res = assert_equals_separate(tenants, which, qs, k)
            assert_equals_oracle(tenants, which, all_d, k, res)
            assert np.array_equal(res[0][2], big.ids[big.live][:k]) and np.all(np.isposinf(res[1][2]))
    finally:
        destroy(tenants)


def test_validation_leaves_outputs_untouched(ctx, orc):
    lib, k, (m, ks, ds) = ctx.lib, 4, (16, 16, 2)
    d = m * ds

    def pq(mm, kk, book=True):
        c = Corpus(ctx, KIND_PQ, METRIC_L2, d, 64)
        if book:
            c.set_codebook(_centers(orc, 1, mm, kk, d // mm))
        return c

    a, b, bare, other_ks, other_m = pq(m, ks), pq(m, ks), pq(m, ks, False), pq(m, 8), pq(8, ks)
    f32, bq = Corpus(ctx, KIND_F32, METRIC_L2, d, 64), Corpus(ctx, KIND_BQ, METRIC_L2, d, 64)
    try:
        qs = _queries(orc, 2, 3, d)

        def call(corpora, kk=k):
            ids = np.full((3, kk), 0x1234, np.uint64)
            dists = np.full((3, kk), -7.0, np.float32)
            counts = np.full(3, 99, np.uint32)
            hs = (ctypes.c_void_p * 3)(*[c.handle for c in corpora])
            rc = lib.wvg_search_group(hs, _lib.fptr(qs), 3, kk, None, None, _lib.u64ptr(ids), _lib.fptr(dists),
                                      _lib.u32ptr(counts))
            untouched = bool(np.all(ids == 0x1234) and np.all(dists == -7.0) and np.all(counts == 99))
            return rc, lib.wvg_last_error().decode(), untouched

        rc, msg, untouched = call([a, b, a])
        assert rc == _lib.WVG_OK and not untouched, msg
        for corpora, kk, code, word in [([a, bq, b], k, _lib.WVG_ERR_UNSUPPORTED, "corpora[1]"),
                                        ([a, b, f32], k, _lib.WVG_ERR_INVALID, "corpora[2]"),
                                        ([f32, a, f32], k, _lib.WVG_ERR_INVALID, "corpora[1]"),
                                        ([a, bare, b], k, _lib.WVG_ERR_INVALID, "PQ corpus has no codebook"),
                                        ([a, other_ks, b], k, _lib.WVG_ERR_INVALID, "corpora[1]"),
                                        ([a, b, other_m], k, _lib.WVG_ERR_INVALID, "corpora[2]"),
                                        ([a, b, a], 257, _lib.WVG_ERR_UNSUPPORTED, "256")]:
            rc, msg, untouched = call(corpora, kk)
            assert rc == code and word in msg and untouched, (rc, msg, untouched)
    finally:
        for c in (a, b, bare, other_ks, other_m, f32, bq):
            c.destroy()

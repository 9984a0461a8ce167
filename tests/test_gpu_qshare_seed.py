"""The seeded shared-row query stream (qshare_seed_kernel + scan_f32_qshare_kernel,
wvg_qshare.hip): before the scan a prologue launch scores the first S tiles of
the range for every query and leaves the sample's k-th key; every wave's list
then starts from that bound instead of empty.  The results must not change:
wvg_search_device_pipelined is compared with nq separate wvg_search_device
calls bit for bit (ids, distance bits, counts) and with the oracle.  Every call
runs twice back to back without a sync in between, so both walk directions run.

The corpora are a little larger than the sample (S + 3 tiles and a ragged last
one), so rows on both sides of it compete for the result.  S and the
tiles-per-wave limit of seeding are the Tuning defaults of wvg_internal.hpp.
The host seeds d = 128 only (qshare_seed_tiles): at d = 768 the same calls run
the prologue without a sample and the scan with open bounds.
"""
import os
import re

import numpy as np
import pytest

from weaviate_amd._lib import KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_L2
from weaviate_amd.device import Corpus

from test_gpu_k1_matrix import device_search
from test_gpu_parity import bits, check_topk, prep_query, stored_rows


def _tuning_default(name):
    hdr = os.path.join(os.path.dirname(__file__), "..", "weaviate_amd", "csrc", "wvg_internal.hpp")
    m = re.search(r"\bint %s = (\d+);" % name, open(hdr).read())
    assert m, name
    return int(m.group(1))


S = _tuning_default("qshare_seed")          # tiles of the sample
TPW = _tuning_default("qshare_seed_tpw")    # seeding stops above this many tiles per wave
N = (S + 3) * 64 + 17
BASE = 64 * 100_000                          # id_base (a multiple of 64)
DIMS = (128, 768)
METRICS = (METRIC_L2, METRIC_DOT, METRIC_COSINE)
NQS = (2, 16, 17, 33)
KS = (1, 10, 64, 65, 128, 129, 256)
NQ_MAX = max(NQS)
DEAD = [0, 63, 64, 1000, S * 64 - 1, S * 64, N - 1]  # inside the sample, at its edge, outside
UINT64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


class Corp:
    """A corpus at id_base BASE with its oracle distances; singles(k) = every query alone
    through wvg_search_device (computed once per k)."""

    def __init__(self, cx, orc, metric, rows, qs, dead=()):
        self.orc, self.metric = orc, metric
        n, d = rows.shape
        self.n = n
        self.c = Corpus(cx, KIND_F32, metric, d, n, id_base=BASE)
        self.ids = np.arange(BASE, BASE + n, dtype=np.uint64)
        self.c.upsert(self.ids, rows)
        self.valid = np.ones(n, np.uint8)
        if len(dead):
            dead = np.asarray(dead, np.int64)
            self.c.delete(self.ids[dead])
            self.valid[dead] = 0
        srows = stored_rows(orc, metric, rows)
        self.pq = np.stack([prep_query(orc, metric, q) for q in qs])
        self.all_d = [orc.dist_all(metric, q, srows) for q in self.pq]
        self._singles = {}

    def singles(self, k):
        if k not in self._singles:
            lib = self.c.lib
            self._singles[k] = [device_search(lib, self.c, lib.wvg_search_device, self.pq[[qi]], k, reps=1)[0]
                                for qi in range(len(self.pq))]
        return self._singles[k]

    def lex(self, qi, k):
        sel = self.valid.astype(bool)
        return self.orc.lex_topk(self.all_d[qi][sel], self.ids[sel], k)

    def check(self, nq, k, heap=True):
        """The first nq queries in one pipelined call, twice: the singles bit for bit, the oracle."""
        lib = self.c.lib
        ref = self.singles(k)
        for ids, dists, counts in device_search(lib, self.c, lib.wvg_search_device_pipelined, self.pq[:nq], k, reps=2):
            for qi in range(nq):
                ri, rd, rc = ref[qi]
                cnt = int(counts[qi])
                assert cnt == rc[0], (qi, k)
                assert np.array_equal(ids[qi], ri[0]), (qi, k)
                assert np.array_equal(bits(dists[qi]), bits(rd[0])), (qi, k)
                if heap:
                    check_topk(self.orc, ids[qi], dists[qi], cnt, self.all_d[qi], self.ids, k, self.valid)
                else:  # rows with NaN distances: the lexicographic order only
                    li, ld = self.lex(qi, k)
                    assert cnt == len(li) and np.array_equal(ids[qi][:cnt], li), (qi, k)
                    assert np.array_equal(bits(dists[qi][:cnt]), bits(ld)), (qi, k)
                assert np.all(ids[qi][cnt:] == UINT64_MAX) and np.all(np.isposinf(dists[qi][cnt:])), (qi, k)

    def destroy(self):
        self.c.destroy()


_corps = {}


@pytest.fixture(scope="module")
def corps(ctx, orc):
    def get(metric, d):
        if (metric, d) not in _corps:
            rows = orc.synth_rows(3000 + 7 * d + metric, 0, N, d, 0)
            qs = orc.synth_rows(4000 + 7 * d + metric, 0, NQ_MAX, d, 0)
            _corps[(metric, d)] = Corp(ctx, orc, metric, rows, qs, DEAD)
        return _corps[(metric, d)]

    yield get
    for cp in _corps.values():
        cp.destroy()
    _corps.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_seeded_corpus_larger_than_sample(corps, metric, d, nq):
    cp = corps(metric, d)
    for k in KS:
        cp.check(nq, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 100])
def test_seeded_ties_at_the_bound(ctx, orc, k):
    """Eight distinct vectors repeated through the corpus: every distance occurs ~N / 8 times,
    inside and outside the sample, so rows tied with the seed key lie on both sides of it.
    The smaller ids win, as in the single searches."""
    d = 128
    base = np.floor(orc.synth_rows(61, 0, 8, d, 0) * 4).astype(np.float32)
    rows = base[np.arange(N) % 8]
    qs = np.concatenate([base[:2], np.floor(orc.synth_rows(62, 0, 3, d, 0) * 4).astype(np.float32)])
    cp = Corp(ctx, orc, METRIC_L2, rows, qs, DEAD)
    try:
        assert (cp.all_d[0] == np.sort(cp.all_d[0])[k - 1]).sum() > 100
        cp.check(len(qs), k)
    finally:
        cp.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sample_deleted", "k_minus_1_in_sample", "k_above_live_rows"])
def test_seeded_fewer_than_k_live_rows_in_sample(ctx, orc, case):
    d, k = 128, 10
    rows = orc.synth_rows(71, 0, N, d, 0)
    qs = orc.synth_rows(72, 0, 5, d, 0)
    if case == "sample_deleted":          # the first S tiles hold nothing: open bound
        dead = np.arange(S * 64)
    elif case == "k_minus_1_in_sample":   # k - 1 live rows in the sample: still open
        dead = np.setdiff1d(np.arange(S * 64), np.linspace(5, S * 64 - 1, k - 1).astype(np.int64))
    else:                                  # 7 live rows in all, 4 of them in the sample
        dead = np.setdiff1d(np.arange(N), [5, 700, S * 32, S * 64 - 1, S * 64, N - 20, N - 1])
    cp = Corp(ctx, orc, METRIC_L2, rows, qs, dead)
    try:
        for kk in (k, 100):
            cp.check(len(qs), kk)
        if case == "k_above_live_rows":
            ids, dists, counts = device_search(cp.c.lib, cp.c, cp.c.lib.wvg_search_device_pipelined, cp.pq, k, reps=1)[0]
            assert np.all(counts == 7)
    finally:
        cp.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["bound_is_special", "all_live"])
def test_seeded_special_values(ctx, orc, where):
    """Rows giving NaN, +inf, -inf and -0.0 distances (DOT: dist = -dot) inside the sample and
    outside it.  bound_is_special: the sample keeps 8 rows below +inf, then three +inf and three NaN rows, so
    its 10-th key is an inf key and its 13-th a NaN key, and that key is the bound of every wave."""
    d = 128
    rows = np.floor(orc.synth_rows(81, 0, N, d, 0) * 2).astype(np.float32)
    qs = np.floor(orc.synth_rows(82, 0, 5, d, 0) * 2).astype(np.float32)
    qs[:, :16] = 1.0  # the columns the special rows use: the sign of an inf product is known
    out = S * 64  # first row outside the sample
    nan_rows, pinf_rows, ninf_rows = [100, 101, out - 48, out + 5], [200, 201, out - 30, out + 70], [300, out + 130]
    zero_rows = [400, 401, out + 200]
    rows[nan_rows, 5] = np.nan
    rows[pinf_rows, 7] = -np.inf     # dot -inf -> dist +inf
    rows[ninf_rows, 9] = np.inf      # dist -inf
    rows[zero_rows] = 0.0            # dot +0 -> dist -0
    rows[402] = -0.0
    special = nan_rows + pinf_rows + ninf_rows + zero_rows + [402]
    finite_kept = [10, out // 2, out - 100, out - 2]
    if where == "bound_is_special":
        keep = set(finite_kept + [r for r in special if r < out])
        dead = [i for i in range(out) if i not in keep]
    else:
        dead = [64, out + 1]
    cp = Corp(ctx, orc, METRIC_DOT, rows, qs, dead)
    try:
        for k in (1, 10, 13, 64, 100):
            cp.check(len(qs), k, heap=False)
    finally:
        cp.destroy()


@pytest.mark.gpu
def test_unseeded_above_tiles_per_wave_limit(ctx):
    """A corpus just past the tiles-per-wave limit: the host passes S = 0, the prologue only
    zeroes the hand-off words and the lists start open.  Two queries against the two single searches."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = 2 * cus * 4                    # qshare_groups x SCAN_WAVES
    n = (TPW + 1) * waves * 64 + 64        # ntiles / waves = TPW + 1
    d, k = 128, 10
    if n * d * 4 > 8 * 2**30:
        pytest.skip(f"{n} x {d} fp32 rows ({n * d * 4 / 2**30:.1f} GiB) for {TPW} tiles per wave on {cus} CUs: above 8 GiB")
    c = Corpus(ctx, KIND_F32, METRIC_L2, d, n)
    try:
        c.fill_synthetic(91, n, 0)
        qs = np.random.default_rng(92).uniform(-1, 1, (2, d)).astype(np.float32)
        lib = c.lib
        ref = [device_search(lib, c, lib.wvg_search_device, qs[[qi]], k, reps=1)[0] for qi in range(2)]
        for ids, dists, counts in device_search(lib, c, lib.wvg_search_device_pipelined, qs, k, reps=2):
            for qi in range(2):
                assert counts[qi] == ref[qi][2][0] == k
                assert np.array_equal(ids[qi], ref[qi][0][0])
                assert np.array_equal(bits(dists[qi]), bits(ref[qi][1][0]))
    finally:
        c.destroy()

"""The bound of K8m (wvg_pq_mfma.hip, the comment block above PqmArgs) and its per-query constants
(pqm_qconst_kernel), restated in numpy as the kernels compute them.  It is K3c-L2's bound (test_screen_l2_bound.py,
whose bf16 / fma / norm / sigma restatements are imported) with alpha = (2 (m + dsub) + 20) 2^-24 for K8's chain:
rows are decoded from the codebook, their bf16 image is the element-wise bf16 of the centroids, the MFMA dot in
float64 is moved against the side under test by its fp32 accumulation term.  r = the oracle's pq_adc of pq_lut
(adc_all, pinned to it row by row in test_gpu_pq_k8_matrix.py).  For every (query, row):
    (a) lower <= r,   (b) r <= lower + 2 E_tot,   (c) E_tot <= Emax_q,
and a non-finite or overflowing centroid, row norm or query never ends in "skip"."""
import numpy as np
import pytest

from test_gpu_pq_k8_matrix import adc_all
from test_screen_l2_bound import F32, bf16, fma32, norm_upper, skipped

SHAPES = [(32, 4), (16, 8), (192, 8)]  # (m, dsub)
KS = 16


def alpha_of(m, ds):
    return (2.0 * (m + ds) + 20.0) * 2.0**-24


def bound(q, cen, codes, side):
    """(u, lower, E_tot, Cq, Emax_q) of every row as K8m computes them (side: see test_screen_l2_bound.bound)."""
    m, _, ds = cen.shape
    d, al = m * ds, alpha_of(m, ds)
    with np.errstate(all="ignore"):
        sq = np.sum(cen.astype(np.float64) ** 2, axis=2)  # pqm_prep_kernel's table
        nx = norm_upper(np.sum(sq[np.arange(m), codes], axis=1))  # pqm_norms_kernel
        ss = np.sum(q.astype(np.float64) ** 2)  # pqm_qconst_kernel = screen_l2_query_consts at alpha
        nq = norm_upper(ss)
        c = F32(F32(2.0**-7) + F32(2.0**-15)) + F32(d) * F32(2.0**-21)
        k1, k2 = F32(c * nq) + F32(2.0**-120), F32(F32(2.0**-120) * nq) + F32(2.0**-110)
        cq = F32(ss * (1.0 - 2.0**-19 - al) - 2.0**-100)
        if not nq <= F32(2.0**56):
            k1, cq = F32(np.inf), F32(-np.inf)
        beta = al + 2.0**-18
        emax = F32((2.0 * float(fma32(nx.max(), k1, k2)) + beta * (float(nq) ** 2 + float(nx.max()) ** 2) + 2.0**-99)
                   * (1.0 + 2.0**-20))
        xb = bf16(cen)[np.arange(m), codes].reshape(len(codes), d).astype(np.float64)  # the image, gathered
        qb = bf16(q).astype(np.float64)
        s = xb @ qb + side * 3 * d * 2.0**-24 * (np.abs(xb) @ np.abs(qb))
        s = np.nextafter(s.astype(np.float32), F32(side * np.inf))
        hg = F32((1.0 - (al + 2.0**-18)) * 0.5 * (1.0 - 2.0**-23))
        h = np.where(nx <= F32(2.0**60), (nx * nx) * hg, F32(np.nan)).astype(np.float32)
        e1 = fma32(nx, k1, k2)
        u = (s - h).astype(np.float32) + e1
        lower = cq - F32(2.0) * u
        lower = np.where(np.isnan(lower), F32(-np.inf), np.maximum(lower, F32(0.0)))  # sc_lower_l2
        etot = 2.0 * e1.astype(np.float64) + beta * (float(nq) ** 2 + nx.astype(np.float64) ** 2) + 2.0**-99
    return u, lower, etot, cq, emax


def check(orc, qs, cen, codes):
    for q in qs:
        r = adc_all(0, orc.pq_lut(0, q, cen), codes).astype(np.float64)
        u, lo, _, cq, _ = bound(q, cen, codes, -1)
        assert np.all(lo <= r), (np.flatnonzero(~(lo <= r))[:5], lo[~(lo <= r)][:5], r[~(lo <= r)][:5])
        _, hi, etot, _, emax = bound(q, cen, codes, +1)
        ok = r <= hi.astype(np.float64) + 2.0 * etot
        assert np.all(ok), (np.flatnonzero(~ok)[:5], hi[~ok][:5], etot[~ok][:5], r[~ok][:5])
        assert np.all(etot <= float(emax)), (etot.max(), emax)
        for i in range(0, len(codes), 7):  # with tau = the row's own exact distance the row is not skipped
            assert not skipped(u[i], lo[i], F32(r[i]), cq)


def book(orc, seed, m, ds, n=512):
    cen = orc.synth_rows(seed, 0, m * KS, ds, 0).reshape(m, KS, ds)
    return cen, np.random.default_rng(seed).integers(0, KS, (n, m), dtype=np.uint8), orc.synth_rows(seed + 1, 0, 4, m * ds, 0)


@pytest.mark.parametrize("m,ds", SHAPES)
def test_uniform_unit_integer_and_scaled_codebooks(orc, m, ds):
    cen, codes, qs = book(orc, 8100 + m, m, ds)
    check(orc, qs, cen, codes)
    check(orc, (qs / np.linalg.norm(qs, axis=1, keepdims=True)).astype(np.float32), (cen / np.sqrt(m * ds)).astype(np.float32), codes)
    check(orc, np.floor(qs * 3).astype(np.float32), np.floor(cen * 3).astype(np.float32), codes)
    for scale in (1e-20, 1e15):
        check(orc, (qs * F32(scale)).astype(np.float32), (cen * F32(scale)).astype(np.float32), codes)
        check(orc, qs[:2], (cen * F32(scale)).astype(np.float32), codes)
    # and the bound is useful: on uniform codebooks its slack 2 E_tot is a small part of the distances
    r = adc_all(0, orc.pq_lut(0, qs[0], cen), codes)
    assert np.max(2 * bound(qs[0], cen, codes, -1)[2]) < 0.1 * np.median(r)


@pytest.mark.parametrize("m,ds", SHAPES)
def test_rows_that_decode_to_the_query_and_mixed_magnitudes(orc, m, ds):
    cen, codes, _ = book(orc, 8200 + m, m, ds, 64)
    for row in codes[:4]:
        q = cen[np.arange(m), row].reshape(-1)
        assert adc_all(0, orc.pq_lut(0, q, cen), row[None])[0] == 0
        check(orc, [q], cen, codes)
        assert bound(q, cen, row[None], -1)[1][0] == 0
    rng = np.random.default_rng(8300 + m)
    mixed = (rng.choice([-1.0, 1.0], cen.shape) * 2.0 ** rng.uniform(-60, 25, cen.shape)).astype(np.float32)
    qm = (rng.choice([-1.0, 1.0], (2, m * ds)) * 2.0 ** rng.uniform(-60, 25, (2, m * ds))).astype(np.float32)
    check(orc, qm, mixed, codes)
    check(orc, np.zeros((1, m * ds), np.float32), mixed, codes)
    check(orc, qm, np.zeros_like(cen), codes)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e30])
def test_non_finite_and_huge_inputs_never_skip(orc, bad):
    m, ds = 32, 4
    cen, codes, qs = book(orc, 8400, m, ds, 256)
    cen_bad = cen.copy()
    cen_bad[np.arange(m), np.arange(m) % KS, np.arange(m) % ds] = bad
    qs_bad = qs.copy()
    qs_bad[0, 1], qs_bad[3] = bad, bad
    taus = [F32(t) for t in (0.0, 1.0, 85.0, 1e30, 3.4e38, np.inf)]
    for q, cb in [(qs[0], cen_bad), (qs_bad[0], cen), (qs_bad[0], cen_bad), (qs_bad[3], cen_bad), (qs_bad[3], cen)]:
        r = adc_all(0, orc.pq_lut(0, q, cb), codes)
        for side in (-1, +1):
            u, lower, _, cq, emax = bound(q, cb, codes, side)
            for tau in taus:
                sk = np.array([skipped(u[i], lower[i], tau, cq) for i in range(len(codes))])
                with np.errstate(invalid="ignore"):
                    assert not (sk & ~(r > tau)).any(), (bad, tau)  # a skipped row's exact distance lies above tau
                assert not (sk & np.isnan(r)).any()
            assert not skipped(u, lower, F32(np.inf), cq).any()  # an open tau admits every row
            if not np.isfinite(bad):
                assert not np.isfinite(emax)  # every bound such a codebook or query gives is open

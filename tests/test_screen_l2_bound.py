"""The bound of the batched l2-squared screen (wvg_screen.hip, "K3c-L2") and its
per-query constants (screen_qconst_l2_kernel), restated in numpy as the kernels
compute them: bf16 round-to-nearest-even operands, the MFMA dot in float64 moved
against the side under test by its fp32 accumulation term (3 d 2^-24 sum |q^ x^|),
the row side and the combine in float32, the query side in float64.  For every
(query, row), r = the oracle's AVX2-order L2 chain (orc.dist_all):
    lower <= r,   r <= lower + 2 E_tot,   E_tot <= Emax_q,
and a non-finite or overflowing row or query, or an open tau, never ends in "skip".
"""
import numpy as np
import pytest

F32 = np.float32
DIMS = [32, 96, 128, 768, 1536]


def bf16(x):
    """float32 -> bf16 (round to nearest even), returned as float32."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), np.float32(np.nan), r)


def fma32(a, b, c):
    """float32 fma (products of float32 are exact in float64)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def norm_upper(ss):
    """norm_upper: sqrt of the fp64 square sum, rounded up past the float cast; +inf for a non-finite sum."""
    ss = np.asarray(ss, np.float64)
    with np.errstate(all="ignore"):
        return np.where(ss < 1e300, np.sqrt(ss) * (1.0 + 1e-6), np.inf).astype(np.float32)


def alpha_of(d):
    return (d / 16.0 + 32.0) * 2.0**-24


def hg_of(d):
    """launch_screen's hg = (1 - g) / 2 rounded down, g = alpha + 2^-18."""
    return F32((1.0 - (alpha_of(d) + 2.0**-18)) * 0.5 * (1.0 - 2.0**-23))


def query_side(q, nmax):
    """screen_qconst_l2_kernel: K1, K2, Cq, Emax_q (float32) of one query; nmax = the corpus maximum norm bound."""
    d = len(q)
    with np.errstate(all="ignore"):
        ss = np.sum(q.astype(np.float64) ** 2)
        nq = norm_upper(ss)
        c = F32(F32(2.0**-7) + F32(2.0**-15)) + F32(d) * F32(2.0**-21)
        k1 = F32(c * nq) + F32(2.0**-120)
        k2 = F32(F32(2.0**-120) * nq) + F32(2.0**-110)
        cq = F32(ss * (1.0 - 2.0**-19 - alpha_of(d)) - 2.0**-100)
        if not nq <= F32(2.0**56):
            k1, cq = F32(np.inf), F32(-np.inf)
        e1 = float(fma32(nmax, k1, k2))
        beta = alpha_of(d) + 2.0**-18
        emax = F32((2.0 * e1 + beta * (float(nq) ** 2 + float(nmax) ** 2) + 2.0**-99) * (1.0 + 2.0**-20))
    return k1, k2, cq, emax, nq


def row_norms(rows):
    return norm_upper(np.sum(rows.astype(np.float64) ** 2, axis=1))


def bound(q, rows, side):
    """(u, lower, E_tot) of every row as K3c-L2 computes them; side = -1: the MFMA dot at the low end of its
    accumulation error (the worst case of lower <= r), +1: at the high end (of r <= lower + 2 E_tot)."""
    d = len(q)
    with np.errstate(all="ignore"):
        nx = row_norms(rows)
        k1, k2, cq, emax, nq = query_side(q, nx.max())
        qb, xb = bf16(q).astype(np.float64), bf16(rows).astype(np.float64)
        s = xb @ qb + side * 3 * d * 2.0**-24 * (np.abs(xb) @ np.abs(qb))
        s = np.nextafter(s.astype(np.float32), F32(side * np.inf))
        h = np.where(nx <= F32(2.0**60), (nx * nx) * hg_of(d), F32(np.nan)).astype(np.float32)
        e1 = fma32(nx, k1, k2)
        u = (s - h).astype(np.float32) + e1
        lower = cq - F32(2.0) * u
        lower = np.where(np.isnan(lower), F32(-np.inf), np.maximum(lower, F32(0.0)))  # sc_lower_l2
        beta = alpha_of(d) + 2.0**-18
        etot = 2.0 * e1.astype(np.float64) + beta * (float(nq) ** 2 + nx.astype(np.float64) ** 2) + 2.0**-99
    return u, lower, etot, cq, emax


def sigma(tau, cq):
    """sc_sigma_l2."""
    with np.errstate(all="ignore"):
        if not tau < np.inf:
            return F32(-np.inf)
        dd = F32(cq - F32(tau))
        s = fma32(F32(-2.0**-22), np.abs(dd), F32(0.5) * dd) - F32(2.0**-120)
        return s if s == s else F32(-np.inf)


def skipped(u, lower, tau, cq):
    """The kernel's decision: the u-space compare of the epilogue, then sc_insert's distance-space one."""
    with np.errstate(invalid="ignore"):
        return (u < sigma(tau, cq)) | ~(lower <= tau)


def check(orc, qs, rows):
    for q in qs:
        r = orc.dist_all(orc.L2, q, rows).astype(np.float64)
        u, lo, _, cq, _ = bound(q, rows, -1)
        assert np.all(lo <= r), (np.flatnonzero(~(lo <= r))[:5], lo[~(lo <= r)][:5], r[~(lo <= r)][:5])
        _, hi, etot, _, emax = bound(q, rows, +1)
        ok = r <= hi.astype(np.float64) + 2.0 * etot
        assert np.all(ok), (np.flatnonzero(~ok)[:5], hi[~ok][:5], etot[~ok][:5], r[~ok][:5])
        assert np.all(etot <= float(emax)), (etot.max(), emax)
        # with tau = the row's own exact distance the row is not skipped (the fast check is a superset test)
        for i in range(0, len(rows), 7):
            assert not skipped(u[i], lo[i], F32(r[i]), cq)


@pytest.mark.parametrize("d", DIMS)
def test_uniform_unit_and_integer_rows(orc, d):
    rows = orc.synth_rows(11 + d, 0, 1024, d, 0)
    qs = orc.synth_rows(12 + d, 0, 4, d, 0)
    check(orc, qs, rows)
    unit = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
    check(orc, (qs / np.linalg.norm(qs, axis=1, keepdims=True)).astype(np.float32), unit)
    check(orc, np.floor(qs * 3).astype(np.float32), np.floor(rows * 3).astype(np.float32))
    # and the bound is useful: on uniform rows its slack 2 E_tot is a small part of the distances
    r = orc.dist_all(orc.L2, qs[0], rows)
    _, lo, etot, _, _ = bound(qs[0], rows, -1)
    assert np.median(r - lo) < 0.1 * np.median(r) and np.max(2 * etot) < 0.1 * np.median(r)


@pytest.mark.parametrize("d", DIMS)
def test_rows_equal_to_the_query(orc, d):
    qs = orc.synth_rows(21 + d, 0, 4, d, 0)
    for q in qs:
        rows = np.repeat(q[None], 64, 0)
        rows[32:] = np.nextafter(rows[32:], F32(np.inf))  # and one ulp away in every element
        assert np.all(orc.dist_all(orc.L2, q, rows[:32]) == 0)
        check(orc, [q], rows)
        assert np.all(bound(q, rows, -1)[1][:32] == 0)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("scale", [1e-20, 1e15])
def test_scaled_rows(orc, d, scale):
    rows = (orc.synth_rows(31 + d, 0, 512, d, 0) * F32(scale)).astype(np.float32)
    qs = (orc.synth_rows(32 + d, 0, 4, d, 0) * F32(scale)).astype(np.float32)
    check(orc, qs, rows)
    check(orc, orc.synth_rows(33 + d, 0, 2, d, 0), rows)


@pytest.mark.parametrize("d", DIMS)
def test_mixed_magnitude_rows(orc, d):
    rng = np.random.default_rng(6 + d)
    n = 512
    sign = rng.choice([-1.0, 1.0], (n + 4, d))
    mixed = (sign * 2.0 ** rng.uniform(-60, 25, (n + 4, d))).astype(np.float32)
    check(orc, mixed[:4], mixed[4:])
    check(orc, orc.synth_rows(41 + d, 0, 2, d, 0), mixed[4:])
    zeros = np.zeros((2, d), np.float32)
    check(orc, zeros, mixed[4:68])
    check(orc, mixed[:2], zeros)


@pytest.mark.parametrize("d", [128, 768])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e30])
def test_non_finite_and_huge_inputs_never_skip(orc, d, bad):
    rows = orc.synth_rows(51, 0, 256, d, 0)
    qs = orc.synth_rows(52, 0, 4, d, 0)
    rows_bad = rows.copy()
    rows_bad[np.arange(256), np.arange(256) % d] = bad
    rows_bad[7] = bad  # a whole row
    qs_bad = qs.copy()
    qs_bad[np.arange(3), [0, 1, d - 1]] = bad
    qs_bad[3] = bad
    taus = [F32(t) for t in (0.0, 1.0, 85.0, 1e30, 3.4e38, np.inf)]
    for q, rr in [(qs[0], rows_bad), (qs_bad[0], rows), (qs_bad[1], rows_bad), (qs_bad[3], rows_bad),
                  (qs_bad[3], rows)]:
        r = orc.dist_all(orc.L2, q, rr)
        for side in (-1, +1):
            u, lower, _, cq, emax = bound(q, rr, side)
            for tau in taus + [None]:
                t = np.where(np.isnan(r), F32(np.inf), r) if tau is None else tau  # (a threshold is never NaN)
                sk = np.array([skipped(u[i], lower[i], t[i] if tau is None else t, cq) for i in range(len(rr))])
                with np.errstate(invalid="ignore"):
                    # a skipped row's exact distance lies above tau; a NaN distance never skips
                    assert not (sk & ~(r > t)).any(), (bad, tau)
                assert not (sk & np.isnan(r)).any()
            assert not skipped(u, lower, F32(np.inf), cq).any()  # an open tau admits every row
            if not np.isfinite(bad):
                # every bound such a corpus or query gives is open: Emax_q is not finite, tau stays +inf
                assert not np.isfinite(emax)

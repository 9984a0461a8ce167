"""The bound of K3i-L2 (wvg_screen.hip, "K3i-L2") restated in numpy as the kernels compute it: int8 codes at
the corpus scale S (from the rows of the first build) and the query's Sq, the exact int32 dot, float32 for
every fp32 step of the combine, float64 where shadow_i8_norm_kernel / screen_qconst_l2_i8_kernel use it.  For
every (query, row), r = the oracle's l2_256 chain: lower <= r <= lower + 2 E_tot, E_tot <= Emax_q, the row is
not skipped at tau = r, and a non-finite or huge row or query never ends in "skip"."""
import numpy as np
import pytest

from test_screen_l2_bound import F32, alpha_of, fma32, hg_of, norm_upper, skipped

DIMS = [512, 768, 1024]


def codes(x, inv):
    """si_code: nearest at 1 / inv, clamped to +-127, NaN -> 0."""
    with np.errstate(all="ignore"):
        r = np.rint((x * F32(inv)).astype(np.float32))
        return np.where(r >= 127, 127, np.where(r <= -127, -127, np.where(r == r, r, 0))).astype(np.float64)


def bound(q, rows, nbuilt):
    """(u, lower, E_tot, Cq, Emax_q); the corpus scale comes from rows[:nbuilt], later rows clamp."""
    d = len(q)
    with np.errstate(all="ignore"):
        fin = np.abs(rows[:nbuilt])
        S = F32(F32(fin[fin <= F32(3.4028235e38)].max()) / F32(127))
        x8 = codes(rows, F32(1) / S)
        x64 = rows.astype(np.float64)
        nx = norm_upper(np.sum(x64 * x64, axis=1))
        ex = norm_upper(np.sum((x64 - float(S) * x8) ** 2, axis=1))
        aq = np.abs(q)
        bad = not np.all(aq <= F32(3.4028235e38))
        amax = F32(aq[aq <= F32(3.4028235e38)].max()) if np.any(aq <= F32(3.4028235e38)) else F32(0)
        sq = F32(amax / F32(127)) if amax > 0 else F32(1)
        q8 = codes(q, F32(1) / sq)
        q64, qt = q.astype(np.float64), float(sq) * q8
        sn = np.sum(q64 * q64)
        nqt, eq, nqu = (float(norm_upper(v)) for v in (np.sum(qt * qt), np.sum((q64 - qt) ** 2), sn))
        A = F32(nqt * (1 + 2.0**-19) + 2.0**-120)
        B = F32(eq * (1 + 2.0**-19) + 4.0 * d * 2.0**-24 * nqu + 2.0**-19 * nqt + 2.0**-120)
        K2 = F32(2.0**-120 * nqu + 2.0**-110)
        cq = F32(sn * (1 - 2.0**-19 - alpha_of(d)) - 2.0**-100)
        cs = F32(S * sq)
        if bad or not (F32(2.0**-100) <= cs <= F32(2.0**100)) or not A < np.inf or not nqu <= 2.0**56:
            A, cq = F32(np.inf), F32(-np.inf)
        beta = alpha_of(d) + 2.0**-18
        e1m = float(fma32(ex.max(), A, fma32(nx.max(), B, K2)))
        emax = F32((2 * e1m + beta * (nqu**2 + float(nx.max()) ** 2) + 2.0**-99) * (1 + 2.0**-20))
        s = ((x8 @ q8).astype(np.float32) * cs).astype(np.float32)  # exact int32 sum, scaled once
        h = np.where(nx <= F32(2.0**60), ((nx * nx).astype(np.float32) * hg_of(d)).astype(np.float32), F32(np.nan))
        e1 = fma32(ex, A, fma32(nx, B, K2))
        u = ((s - h).astype(np.float32) + e1).astype(np.float32)
        lower = (cq - F32(2) * u).astype(np.float32)
        lower = np.where(np.isnan(lower), F32(-np.inf), np.maximum(lower, F32(0)))
        etot = 2.0 * e1.astype(np.float64) + beta * (nqu**2 + nx.astype(np.float64) ** 2) + 2.0**-99
    return u, lower, etot, cq, emax


def families(orc, d):
    """name -> (queries, rows, rows of the first build): the inputs at which this bound can go wrong."""
    rows = orc.synth_rows(61 + d, 0, 600, d, 0)
    qs = orc.synth_rows(62 + d, 0, 4, d, 0)
    big = rows.copy()
    big[:8] *= F32(8)
    clamp = rows.copy()
    clamp[500:] *= F32(50)  # upserted after the first build: codes clamp, Ex ~ |x|
    zero = rows.copy()
    zero[3] = 0
    return {"random": (qs, rows, 600),
            "copies": (np.stack([big[0], np.nextafter(big[1], F32(np.inf)), rows[9]]), big, 600),
            "clamped": (np.stack([qs[0], clamp[500], np.nextafter(clamp[501], F32(0))]), clamp, 500),
            "zeros": (np.stack([np.zeros(d, np.float32), qs[1]]), zero, 600),
            "ties": (rows[7][None], np.repeat(rows[7][None], 40, 0), 40)}


@pytest.mark.parametrize("name", ["random", "copies", "clamped", "zeros", "ties"])
@pytest.mark.parametrize("d", DIMS)
def test_two_sided_bound(orc, d, name):
    qs, rows, nbuilt = families(orc, d)[name]
    assert len(qs) and len(rows)
    for q in qs:
        r = orc.dist_all(orc.L2, q, rows).astype(np.float64)
        u, lo, etot, cq, emax = bound(q, rows, nbuilt)
        assert np.all(lo <= r), (lo[~(lo <= r)][:5], r[~(lo <= r)][:5])
        ok = r <= lo.astype(np.float64) + 2.0 * etot
        assert np.all(ok), (lo[~ok][:5], etot[~ok][:5], r[~ok][:5])
        assert np.all(etot <= float(emax)), (etot.max(), emax)
        assert not any(skipped(u[i], lo[i], F32(r[i]), cq) for i in range(0, len(rows), 7))


@pytest.mark.parametrize("bad", [np.nan, np.inf, 2.0**58])
@pytest.mark.parametrize("d", DIMS)
def test_non_finite_and_huge_never_skip(orc, d, bad):
    rows = orc.synth_rows(71 + d, 0, 128, d, 0)
    q = orc.synth_rows(72 + d, 0, 1, d, 0)[0]
    rows_bad, q_bad = rows.copy(), (q * F32(bad)).astype(np.float32)
    rows_bad[5, 3], rows_bad[6] = bad, rows_bad[6] * F32(bad)
    for qq, rr in [(q, rows_bad), (q_bad, rows), (q_bad, rows_bad)]:
        r = orc.dist_all(orc.L2, qq, rr)
        u, lower, _, cq, _ = bound(qq, rr, 128)
        for tau in [F32(t) for t in (0.0, 85.0, 1e30, np.inf)]:
            sk = np.array([skipped(u[i], lower[i], tau, cq) for i in range(len(rr))])
            with np.errstate(invalid="ignore"):
                assert not (sk & ~(r > tau)).any(), (bad, tau)  # a skipped row lies above tau; NaN never skips

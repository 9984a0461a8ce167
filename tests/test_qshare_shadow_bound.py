"""The bound of the shadow-fed shared-row scan (qshare_shadow_body, wvg_qshare.hip) at d = 128.  It is
K3c-L2's, on K3c-L2's operands -- the shadow's bf16 fragments and norm bounds, hg, and the per-query
K1 / K2 / Cq of screen_l2_query_consts -- so the numpy restatement is test_screen_l2_bound.py's, imported;
what is restated here is only what the shared-row scan does differently: the prologue's fp64 square sum
runs in its own order (a lane's four squares, then the butterfly over the lanes), and the decision is
"skip only if lower > tau_dist and lower < +inf" with tau_dist NaN for an open tau.  For every (query,
row), r = the oracle's AVX2-order L2 chain:
    lower <= r   (so a skipped pair has r > tau_dist: no key below tau),
and a non-finite input never produces a finite lower above a finite r, and never a skip of a row whose
exact distance is NaN or at or below tau.
"""
import numpy as np
import pytest

from test_screen_l2_bound import F32, alpha_of, bf16, bound, fma32, hg_of, norm_upper, query_side, row_norms

D = 128


def prologue_ss(q):
    """screen_query_side's square sum: lane c < 32 sums its chunk's four squares, then off = 32 .. 1 butterflies."""
    x = q.astype(np.float64).reshape(32, 4)
    lanes = np.zeros(64)
    with np.errstate(all="ignore"):
        lanes[:32] = ((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]) + x[:, 3] * x[:, 3]
        for off in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[np.arange(64) ^ off]
    return lanes[0]


def prologue_consts(q):
    """screen_l2_query_consts of the prologue's sum: K1, K2, Cq (float32)."""
    with np.errstate(all="ignore"):
        ss = prologue_ss(q)
        nq = norm_upper(ss)
        c = F32(F32(2.0**-7) + F32(2.0**-15)) + F32(D) * F32(2.0**-21)
        k1 = F32(c * nq) + F32(2.0**-120)
        k2 = F32(F32(2.0**-120) * nq) + F32(2.0**-110)
        cq = F32(ss * (1.0 - 2.0**-19 - alpha_of(D)) - 2.0**-100)
        if not nq <= F32(2.0**56):
            k1, cq = F32(np.inf), F32(-np.inf)
    return k1, k2, cq


def lower_of(q, rows, side=-1):
    """The kernel's lower bound of every row: the MFMA dot at the low end of its accumulation error."""
    with np.errstate(all="ignore"):
        k1, k2, cq = prologue_consts(q)
        nx = row_norms(rows)
        qb, xb = bf16(q).astype(np.float64), bf16(rows).astype(np.float64)
        s = xb @ qb + side * 3 * D * 2.0**-24 * (np.abs(xb) @ np.abs(qb))
        s = np.nextafter(s.astype(np.float32), F32(side * np.inf))
        h = np.where(nx <= F32(2.0**60), (nx * nx) * hg_of(D), F32(np.nan)).astype(np.float32)
        u = (s - h).astype(np.float32) + fma32(nx, k1, k2)
        lower = cq - F32(2.0) * u
        return np.where(np.isnan(lower), F32(-np.inf), np.maximum(lower, F32(0.0)))


def skipped(lower, tau_dist):
    with np.errstate(invalid="ignore"):
        return (lower > tau_dist) & (lower < np.inf)


def check(orc, qs, rows):
    for q in qs:
        r = orc.dist_all(orc.L2, q, rows)
        lo = lower_of(q, rows)
        bad = ~(lo.astype(np.float64) <= r.astype(np.float64))
        assert not bad.any(), (np.flatnonzero(bad)[:5], lo[bad][:5], r[bad][:5])
        # with tau at the row's own distance the row is admitted; an open tau (NaN) admits everything
        assert not skipped(lo, r).any()
        assert not skipped(lo, F32(np.nan)).any()


def test_constants_are_k3c_l2s(orc):
    """The same formulas on the prologue's sum: equal to query_side's wherever the two fp64 sums round alike,
    and never further than one float32 ulp of Cq apart."""
    for q in orc.synth_rows(7001, 0, 64, D, 0):
        k1, k2, cq = prologue_consts(q)
        w1, w2, wq, _, _ = query_side(q, F32(1.0))
        assert k1 == w1 and k2 == w2
        assert abs(float(cq) - float(wq)) <= float(np.spacing(wq))
    assert np.all(bound(orc.synth_rows(7002, 0, 1, D, 0)[0], orc.synth_rows(7003, 0, 8, D, 0), -1)[1] >= 0)


def test_random_and_near_duplicate_pairs(orc):
    rows = orc.synth_rows(7011, 0, 2048, D, 0)
    qs = orc.synth_rows(7012, 0, 8, D, 0)
    check(orc, qs, rows)
    rng = np.random.default_rng(7013)
    for q in qs[:4]:
        near = np.repeat(q[None], 256, 0)
        near[64:128] = np.nextafter(near[64:128], F32(np.inf))
        near[128:] += rng.uniform(-9e-4, 9e-4, (128, D)).astype(np.float32)
        assert np.all(orc.dist_all(orc.L2, q, near[:64]) == 0)
        check(orc, [q], near)
        assert np.all(lower_of(q, near)[:64] == 0)


@pytest.mark.parametrize("e", [-60, -30, -1, 20, 40, 55])
def test_norms_from_tiny_to_huge(orc, e):
    scale = F32(2.0**e / np.sqrt(D / 3.0))  # uniform(-1, 1) rows have norm ~sqrt(d / 3)
    rows = (orc.synth_rows(7021, 0, 512, D, 0) * scale).astype(np.float32)
    qs = (orc.synth_rows(7022, 0, 4, D, 0) * scale).astype(np.float32)
    check(orc, qs, rows)
    check(orc, orc.synth_rows(7023, 0, 2, D, 0), rows)  # and unit-scale queries against them
    check(orc, qs, orc.synth_rows(7024, 0, 256, D, 0))


def test_worst_case_bf16_rounding(orc):
    """Every element a hair from a bf16 rounding midpoint: the largest error the operands can carry, all with
    one sign (down) or the other (up), rows and queries alike and opposed."""
    def push(x, low):
        u = np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
        return (u | np.uint32(0x7FFF if low else 0x8001)).view(np.float32)

    rows = orc.synth_rows(7031, 0, 512, D, 0)
    qs = orc.synth_rows(7032, 0, 4, D, 0)
    for rl in (True, False):
        for ql in (True, False):
            check(orc, push(qs, ql), push(rows, rl))
    q = push(qs[:1], True)[0]
    check(orc, [q], np.repeat(push(q[None], False), 8, 0))  # a near duplicate rounded the other way


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 1e30, 3e38])
def test_non_finite_inputs_never_skip_wrongly(orc, bad):
    rows = orc.synth_rows(7041, 0, 256, D, 0)
    qs = orc.synth_rows(7042, 0, 4, D, 0)
    rows_bad = rows.copy()
    rows_bad[np.arange(256), np.arange(256) % D] = bad
    rows_bad[7] = bad
    qs_bad = qs.copy()
    qs_bad[np.arange(3), [0, 1, D - 1]] = bad
    qs_bad[3] = bad
    taus = [F32(t) for t in (0.0, 1.0, 85.0, 1e30, 3.4e38, np.inf, np.nan)]
    for q, rr in [(qs[0], rows_bad), (qs_bad[0], rows), (qs_bad[1], rows_bad), (qs_bad[3], rows_bad), (qs_bad[3], rows)]:
        r = orc.dist_all(orc.L2, q, rr)
        for side in (-1, +1):
            lo = lower_of(q, rr, side)
            with np.errstate(invalid="ignore"):
                fin = np.isfinite(lo) & np.isfinite(r)
                assert not (fin & (lo > r)).any(), bad  # no finite lower above a finite r
                for tau in taus:
                    sk = skipped(lo, tau)
                    assert not (sk & ~(r > tau)).any(), (bad, tau)  # a skipped row's distance lies above tau
                    assert not (sk & np.isnan(r)).any(), (bad, tau)

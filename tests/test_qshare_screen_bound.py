"""The lower bound of the screened shared-row scan (wvg_qshare.hip, "The bound"),
restated in numpy as the kernel computes it: bf16 round-to-nearest-even operands,
the MFMA dot in float64 moved against the bound by its fp32 accumulation term
(3 d 2^-24 sum |q^ x^|), the row norm and the combine in float32, the query side
in float64.  lower <= r must hold for every (query, row), r = the oracle's
AVX2-order L2 chain (orc.dist_all); non-finite inputs must never end in "skip".
"""
import numpy as np
import pytest

D = 128
C = 2.0**-7 + 2.0**-15 + D * 2.0**-21
G = np.float32(2.0**-15)
F32 = np.float32


def bf16(x):
    """float32 -> bf16 (round to nearest even), returned as float32."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), np.float32(np.nan), r)


def fma32(a, b, c):
    """float32 fma (products of float32 are exact in float64)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def query_side(q):
    ss = np.sum(q.astype(np.float64) ** 2)
    nq = np.sqrt(ss) * (1.0 + 1e-6)
    k1 = (2.0 * C * nq + 2.0**-60) * (1.0 + 2.0**-20)
    k2 = float(G) * ss + 2.0**-60 * nq + 2.0**-100
    return F32(k1), F32(ss - k2)


def lower_bound(q, rows):
    """The kernel's lower bound of |q - row|^2 for every row, with the worst MFMA accumulation."""
    with np.errstate(all="ignore"):
        k1, cq = query_side(q)
        n2a = np.zeros((len(rows), 2), np.float32)
        n2b = np.zeros((len(rows), 2), np.float32)
        for c in range(D // 4):
            lo, hi = rows[:, 4 * c:4 * c + 2], rows[:, 4 * c + 2:4 * c + 4]
            n2a, n2b = fma32(lo, lo, n2a), fma32(hi, hi, n2b)
        n2 = n2a + n2b
        nx2 = n2[:, 0] + n2[:, 1]
        nx = np.sqrt(nx2) * F32(1.0 + 2.0**-16)
        bx = nx2 * (F32(1.0) - G)
        qb, xb = bf16(q).astype(np.float64), bf16(rows).astype(np.float64)
        m = xb @ qb - 3 * D * 2.0**-24 * (np.abs(xb) @ np.abs(qb))  # the accumulation error, against the bound
        m = np.nextafter(m.astype(np.float32), F32(-np.inf))
        t = fma32(np.full_like(m, -2.0), m, bx + cq)
        return fma32(np.full_like(nx, -k1), nx, t)


def skipped(lower, tau):
    """The kernel's decision: a row is ruled out only by a finite lower bound above tau."""
    with np.errstate(invalid="ignore"):
        return (lower > tau) & (lower < np.inf)


def check(orc, qs, rows):
    for q in qs:
        r = orc.dist_all(orc.L2, q, rows)
        lower = lower_bound(q, rows)
        bad = skipped(lower, r)  # with tau = the row's own exact distance the row must not be skipped
        assert not bad.any(), (np.flatnonzero(bad)[:5], lower[bad][:5], r[bad][:5])


def test_uniform_and_unit_norm_rows(orc):
    rows = orc.synth_rows(11, 0, 4096, D, 0)
    qs = orc.synth_rows(12, 0, 8, D, 0)
    check(orc, qs, rows)
    unit = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
    check(orc, (qs / np.linalg.norm(qs, axis=1, keepdims=True)).astype(np.float32), unit)
    # and the bound is useful: its slack is below 1 where the distances are ~85 (2 c |q| |x| ~ 0.7)
    lower = lower_bound(qs[0], rows)
    r = orc.dist_all(orc.L2, qs[0], rows)
    assert np.all(r - lower < 1.0) and np.median(r) > 50


def test_rows_at_and_next_to_the_query(orc):
    """Cancellation: rows equal to the query and within 1-3 ulps of it per element."""
    rng = np.random.default_rng(5)
    qs = orc.synth_rows(21, 0, 4, D, 0)
    for q in qs:
        rows = np.repeat(q[None], 512, 0)
        for i in range(1, 512):
            steps = rng.integers(-3, 4, D)
            steps[rng.random(D) < (i % 8) / 8.0] = 0
            v = rows[i]
            for s in (1, 2, 3):
                up, dn = steps >= s, steps <= -s
                v = np.where(up, np.nextafter(v, F32(np.inf)), np.where(dn, np.nextafter(v, F32(-np.inf)), v))
            rows[i] = v
        check(orc, [q], rows)


def test_mixed_magnitudes_denormals_and_zeros(orc):
    rng = np.random.default_rng(6)
    n = 2048
    sign = rng.choice([-1.0, 1.0], (n + 8, D))
    mixed = (sign * 2.0 ** rng.uniform(-120, 60, (n + 8, D))).astype(np.float32)
    check(orc, mixed[:8], mixed[8:])
    check(orc, orc.synth_rows(31, 0, 4, D, 0), mixed[8:])
    den = (sign * rng.integers(0, 1 << 23, (n + 8, D)) * 2.0**-149).astype(np.float32)  # denormals and zeros
    assert np.all(np.abs(den) < 2.0**-126)
    small = (sign * 2.0 ** rng.uniform(-80, -55, (n + 8, D))).astype(np.float32)  # squares underflow
    for rows in (den, small, np.where(rng.random((n + 8, D)) < 0.5, den, mixed)):
        check(orc, rows[:8], rows[8:])
        check(orc, orc.synth_rows(32, 0, 2, D, 0), rows[8:])
        check(orc, mixed[:4], rows[8:])
    zeros = np.zeros((4, D), np.float32)
    zeros[1] = -0.0
    for other in (mixed[:64], den[:64], orc.synth_rows(33, 0, 64, D, 0), zeros):
        check(orc, zeros[:2], other)
        check(orc, other[:4], zeros)


def test_integer_rows(orc):
    rows = orc.synth_rows(41, 0, 4096, D, 1)  # integers 0..255: large norms
    check(orc, orc.synth_rows(42, 0, 8, D, 1), rows)
    check(orc, orc.synth_rows(43, 0, 4, D, 0), rows)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 3e38, -3e38])
def test_non_finite_and_overflowing_inputs_never_skip(orc, bad):
    rows = orc.synth_rows(51, 0, 256, D, 0)
    qs = orc.synth_rows(52, 0, 4, D, 0)
    rows_bad = rows.copy()
    rows_bad[np.arange(256), np.arange(256) % D] = bad
    qs_bad = qs.copy()
    qs_bad[np.arange(4), [0, 1, 63, 127]] = bad
    taus = np.array([0.0, 1.0, 85.0, 1e30, 3.4e38, np.inf], np.float32)
    for q, rr in [(qs[0], rows_bad), (qs_bad[0], rows), (qs_bad[1], rows_bad), (qs_bad[3], rows_bad)]:
        lower = lower_bound(q, rr)
        r = orc.dist_all(orc.L2, q, rr)
        for tau in list(taus) + [None]:
            sk = skipped(lower, r if tau is None else tau)
            # a skipped row's exact distance lies above tau (r = inf for an overflowing chain); NaN rows never skip
            assert not (sk & ~(r > (r if tau is None else tau))).any(), (bad, tau)
            assert not (sk & np.isnan(r)).any()
    if not np.isfinite(bad):
        for q, rr in [(qs[0], rows_bad), (qs_bad[0], rows)]:
            assert not np.isfinite(lower_bound(q, rr)).any()

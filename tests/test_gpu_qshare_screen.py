"""The screened shared-row scan (scan_f32_qshare_screen_kernel, wvg_qshare.hip):
seeded L2 launches at d = 128 with k <= 64 score every tile with a bf16 MFMA
lower bound first and run the exact chain only for the (query, tile) pairs the
bound cannot rule out.  The results must not change: as in
test_gpu_qshare_seed.py, wvg_search_device_pipelined is compared with nq
separate wvg_search_device calls bit for bit (ids, distance bits, counts) and
with the oracle, every call twice back to back so both walk directions run.
k = 65 takes the unscreened form and must agree as well.
"""
import os

import numpy as np
import pytest

from weaviate_amd._lib import METRIC_L2

from test_gpu_k1_matrix import device_search
from test_gpu_qshare_seed import BASE, DEAD, NQS, Corp, N, S

D = 128
KS = (1, 10, 64, 65)
NQ_MAX = max(NQS)
OUT = S * 64  # first row outside the sample


def _uniform(orc):
    return orc.synth_rows(5001, 0, N, D, 0), orc.synth_rows(5002, 0, NQ_MAX, D, 0), DEAD + list(range(5 * 64, 6 * 64))


def _near_ties(orc):
    """200 copies of one row with single elements moved by 1-4 ulps, queries 1e-3 away from it."""
    rng = np.random.default_rng(7)
    rows = orc.synth_rows(5011, 0, N, D, 0)
    base = rows[17].copy()
    where = rng.choice(N, 200, replace=False)
    for r in where:
        v = base.copy()
        e = rng.integers(D)
        for _ in range(rng.integers(1, 5)):
            v[e] = np.nextafter(v[e], np.float32(np.inf if r & 1 else -np.inf))
        rows[r] = v
    qs = (base[None] + rng.uniform(-1e-3, 1e-3, (NQ_MAX, D))).astype(np.float32)
    return rows, qs, DEAD


def _duplicates(orc):
    base = np.floor(orc.synth_rows(5021, 0, 8, D, 0) * 4).astype(np.float32)
    qs = np.concatenate([base[:3], np.floor(orc.synth_rows(5022, 0, NQ_MAX - 3, D, 0) * 4).astype(np.float32)])
    return base[np.arange(N) % 8], qs, DEAD


def _special_rows(orc):
    rows = orc.synth_rows(5031, 0, N, D, 0)
    vals = [np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-40, -1e-42]
    for i, v in enumerate(vals):
        for r in (70 + 9 * i, OUT - 40 + i, OUT + 30 + 11 * i, N - 9 + i):  # inside the sample and outside it
            rows[r, (13 * i + r) % D] = v
    rows[OUT + 3] = 1e-41
    rows[99] = 0.0
    return rows, orc.synth_rows(5032, 0, NQ_MAX, D, 0), DEAD


def _special_queries(orc):
    qs = orc.synth_rows(5042, 0, NQ_MAX, D, 0)
    qs[1, 77] = np.inf
    qs[2] = 0.0
    qs[5, 3] = -3e38
    qs[16, 100] = -np.inf
    return orc.synth_rows(5041, 0, N, D, 0), qs, DEAD


def _open_seeds(orc):
    """Five live rows in the sample: open seeds for k = 10 and up (everything folds), a seed for k = 1."""
    dead = np.setdiff1d(np.arange(OUT), [5, 700, S * 32, OUT - 65, OUT - 1])
    return orc.synth_rows(5051, 0, N, D, 0), orc.synth_rows(5052, 0, NQ_MAX, D, 0), list(dead) + [OUT, N - 1]


def _integers(orc):
    return orc.synth_rows(5061, 0, N, D, 1), orc.synth_rows(5062, 0, NQ_MAX, D, 1), DEAD


def _nine_tiles(orc):
    """Nine tiles for three workgroups of four waves: some waves get no tile at all."""
    return orc.synth_rows(5071, 0, 9 * 64, D, 0), orc.synth_rows(5072, 0, NQ_MAX, D, 0), [0, 63, 64, 575]


CORPORA = {
    "uniform_deletes_dead_tile": (_uniform, True),
    "near_ties": (_near_ties, True),
    "duplicates": (_duplicates, True),
    "special_rows": (_special_rows, False),      # NaN distances: the lexicographic check only
    "special_queries": (_special_queries, False),
    "open_seeds": (_open_seeds, True),
    "integers": (_integers, True),
    "nine_tiles": (_nine_tiles, True),
}
_corps = {}


@pytest.fixture(scope="module")
def corps(ctx, orc):
    def get(name):
        if name not in _corps:
            rows, qs, dead = CORPORA[name][0](orc)
            _corps[name] = Corp(ctx, orc, METRIC_L2, rows, qs, dead)
        return _corps[name]

    yield get
    for cp in _corps.values():
        cp.destroy()
    _corps.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("name", list(CORPORA))
def test_screened_equals_single_searches(corps, name, nq):
    cp = corps(name)
    for k in KS:
        cp.check(nq, k, heap=CORPORA[name][1])


@pytest.mark.gpu
def test_near_ties_lie_within_the_slack(corps):
    """The cloud does what it is for: hundreds of exact distances within the bf16 slack (~0.7) of the k-th."""
    cp = corps("near_ties")
    d = np.sort(cp.all_d[0][cp.valid.astype(bool)])
    assert (d < d[9] + 0.5).sum() > 150


@pytest.mark.gpu
def test_screen_switched_off_returns_the_same_bytes(corps, orc):
    """A context opened with WVG_QSHARE_SCREEN=0 folds every (query, tile) pair: the same bytes."""
    from weaviate_amd.device import Context

    os.environ["WVG_QSHARE_SCREEN"] = "0"
    try:
        cx = Context(0)
    finally:
        del os.environ["WVG_QSHARE_SCREEN"]
    try:
        for name in ("uniform_deletes_dead_tile", "near_ties", "special_rows"):
            on = corps(name)
            rows, qs, dead = CORPORA[name][0](orc)
            off = Corp(cx, orc, METRIC_L2, rows, qs, dead)
            try:
                for k in (1, 10, 64):
                    a = device_search(on.c.lib, on.c, on.c.lib.wvg_search_device_pipelined, on.pq, k, reps=2)
                    b = device_search(off.c.lib, off.c, off.c.lib.wvg_search_device_pipelined, off.pq, k, reps=2)
                    for (ia, da, ca), (ib, db, cb) in zip(a, b):
                        assert ia.tobytes() == ib.tobytes() and da.tobytes() == db.tobytes() and ca.tobytes() == cb.tobytes()
            finally:
                off.destroy()
    finally:
        cx.close()

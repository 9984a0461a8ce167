"""Row-level admission in the screened shared-row scan (scan_f32_qshare_screen_kernel,
wvg_qshare.hip): the screen leaves every lane a mask of the queries whose lower
bound on the lane's row does not exceed tau, and rounds of the exact chain run
while any lane has a bit -- each lane scores its own row against one of its own
admitted queries per round.  The results must not change: as in
test_gpu_qshare_seed.py, wvg_search_device_pipelined is compared with nq
separate wvg_search_device calls bit for bit (ids, distance bits, counts) and
with the oracle, every call twice back to back so both walk directions run.

split_rounds: one tile outside the sample holds rows built from the queries, so
that a query is offered in more than one round of the tile (the lane of
(q0 + q1) / 2 takes q0 first and q1 in the second round, the lane of q1 + noise
takes q1 in the first), some lanes carry every query of each of the three
passes (the mean of the queries, the zero row, the NaN row), a deleted exact
match shares the tile, and passes 2 and 3 at nq = 17 and 33 hold one query.
crowded_lane: one lane position of every tile outside the sample holds the same
row, close to all queries: that lane runs 16 rounds per tile while the others
run next to none, and the lists fill with ties broken by id.

The preconditions are checked on oracle distances on the CPU before any GPU
call: every planted (query, row) pair lies below the query's 10th distance over
the live sample rows (so the pair is admitted whatever the bf16 slack), and
q1 + noise lies above query 0's by more than 2 (the bf16 slack of the bound is
about 0.7 at these norms), so that lane does not take q0.
"""
import numpy as np
import pytest

from weaviate_amd._lib import METRIC_L2

from test_gpu_k1_matrix import device_search
from test_gpu_parity import bits
from test_gpu_qshare_seed import DEAD, NQS, Corp, N, S

D = 128
KS = (1, 10, 64)
NQ_MAX = max(NQS)
OUT = S * 64        # first row outside the sample
T = OUT + 64        # first row of the planted tile (the second tile outside the sample)
LANE = 5            # crowded_lane: the lane position (the ragged last tile has it too)

# split_rounds: lane of the planted tile -> what lies there
L_MID01, L_Q1, L_MID1617, L_Q17, L_Q32, L_MEAN, L_ZERO, L_NAN, L_COPY1 = 3, 10, 20, 21, 30, 40, 41, 50, 60


def _sample_tenth(orc, rows, qs, dead):
    """Every query's 10th smallest oracle distance over the live rows of the sample."""
    live = np.setdiff1d(np.arange(OUT), np.asarray(dead, np.int64))
    return np.array([np.sort(orc.dist_all(METRIC_L2, q, rows[live]))[9] for q in qs])


def _dist(orc, q, row):
    return float(orc.dist_all(METRIC_L2, q, row[None])[0])


def _split_rounds(orc):
    rows = orc.synth_rows(6001, 0, N, D, 0)
    qs = orc.synth_rows(6002, 0, NQ_MAX, D, 0)
    noise = np.random.default_rng(6003).uniform(-9e-4, 9e-4, (3, D)).astype(np.float32)
    rows[T + L_MID01] = (qs[0] + qs[1]) / 2
    rows[T + L_Q1] = qs[1] + noise[0]
    rows[T + L_MID1617] = (qs[16] + qs[17]) / 2
    rows[T + L_Q17] = qs[17] + noise[1]
    rows[T + L_Q32] = qs[32] + noise[2]
    rows[T + L_MEAN] = qs.mean(axis=0, dtype=np.float64).astype(np.float32)
    rows[T + L_ZERO] = 0.0
    rows[T + L_NAN, 77] = np.nan
    rows[T + L_COPY1] = qs[1]
    dead = DEAD + [T + L_COPY1]
    # the preconditions, on oracle distances (CPU)
    tenth = _sample_tenth(orc, rows, qs, dead)
    planted = [(0, L_MID01), (1, L_MID01), (1, L_Q1), (16, L_MID1617), (17, L_MID1617), (17, L_Q17), (32, L_Q32), (1, L_COPY1)]
    planted += [(j, L_MEAN) for j in range(NQ_MAX)] + [(j, L_ZERO) for j in range(NQ_MAX)]
    for j, lane in planted:
        assert _dist(orc, qs[j], rows[T + lane]) < tenth[j], (j, lane, tenth[j])
    assert _dist(orc, qs[0], rows[T + L_Q1]) > tenth[0] + 2.0, tenth[0]
    return rows, qs, dead


def _crowded_lane(orc):
    rows = orc.synth_rows(6011, 0, N, D, 0)
    qs = orc.synth_rows(6012, 0, NQ_MAX, D, 0)
    crowd = np.arange(OUT + LANE, N, 64)
    assert len(crowd) == 4 and crowd[-1] >= OUT + 3 * 64  # the ragged tile's too
    rows[crowd] = qs.mean(axis=0, dtype=np.float64).astype(np.float32)
    tenth = _sample_tenth(orc, rows, qs, DEAD)
    for j in range(NQ_MAX):
        assert _dist(orc, qs[j], rows[crowd[0]]) < tenth[j], (j, tenth[j])
    return rows, qs, DEAD


CORPORA = {
    "split_rounds": (_split_rounds, False),   # a NaN distance: the lexicographic check only
    "crowded_lane": (_crowded_lane, True),
}
_corps = {}


@pytest.fixture(scope="module")
def corps(ctx, orc):
    def get(name):
        if name not in _corps:
            rows, qs, dead = CORPORA[name][0](orc)  # asserts its preconditions before the first GPU call
            _corps[name] = Corp(ctx, orc, METRIC_L2, rows, qs, dead)
        return _corps[name]

    yield get
    for cp in _corps.values():
        cp.destroy()
    _corps.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("name", list(CORPORA))
def test_row_rounds_equal_single_searches(corps, name, nq):
    cp = corps(name)
    for k in KS:
        cp.check(nq, k, heap=CORPORA[name][1])


@pytest.mark.gpu
def test_crowded_lane_ties_broken_by_id(corps):
    """The four copies of the crowded row tie for every query: they come out in id order."""
    cp = corps("crowded_lane")
    crowd = [int(i) for i in cp.ids[np.arange(OUT + LANE, N, 64)]]
    lib = cp.c.lib
    ids, dists, counts = device_search(lib, cp.c, lib.wvg_search_device_pipelined, cp.pq, 10, reps=1)[0]
    for qi in range(NQ_MAX):
        got = [int(i) for i in ids[qi] if int(i) in crowd]
        assert got == crowd, (qi, got)
        assert len(set(bits(dists[qi][[list(ids[qi]).index(i) for i in crowd]]).tolist())) == 1, qi

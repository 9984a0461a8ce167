"""The tile-parallel prologue of the shared-row query stream (qshare_seed_kernel,
qshare_seed_filt_kernel; wvg_qshare.hip): one wave scores one (sample tile,
query) pair, publishes the tile's sorted keys and its workgroup arrives at one of
PRO_COUNTERS counters in the workspace's status block (query block b at counter
b mod PRO_COUNTERS); the workgroup that arrives last at a counter merges its
queries' lists into seeds[q] and resets the counter.  A wrong seed shows in the
results: a seed that is too small loses rows, a counter that is off leaves stale
or missing seeds.

wvg_search_device_pipelined / _filtered are compared with one wvg_search_device
(or host wvg_search) call per query: ids, distance bits, counts, padding.  Every
call runs twice back to back without a sync in between.

The sample of a range of n tiles is min(S, max(FLOOR, n / SHARE), n) tiles
(qshare_seed_tiles): S and SHARE are the Tuning defaults of wvg_internal.hpp,
FLOOR and the workgroup's query block QB are read from wvg_qshare.hip.  The
corpora sit on both sides of FLOOR and of S, and one is long enough (SHARE x S
tiles and a ragged one) for the sample to reach S.
"""
import os
import re

import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import METRIC_DOT, METRIC_L2

from test_gpu_k1_matrix import device_search
from test_gpu_parity import bits
from test_gpu_qshare_filter import TILES, WINDOWS, FCorp, window_words
from test_gpu_qshare_seed import BASE, DEAD, Corp, N, S, _tuning_default

UINT64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def _source_const(name):
    src = os.path.join(os.path.dirname(__file__), "..", "weaviate_amd", "csrc", "wvg_qshare.hip")
    m = re.search(r"\b%s = (\d+);" % name, open(src).read())
    assert m, name
    return int(m.group(1))


def _header_const(name):
    hdr = os.path.join(os.path.dirname(__file__), "..", "weaviate_amd", "csrc", "wvg_internal.hpp")
    m = re.search(r"\b%s = (\d+);" % name, open(hdr).read())
    assert m, name
    return int(m.group(1))


SHARE = _tuning_default("qshare_seed_share")
FLOOR = _source_const("QSHARE_SEED_FLOOR")
QB = _source_const("PRO_WAVES")          # queries of one workgroup of the prologue
NQ_MAX = 33


def sample_tiles(ntiles):
    return min(S, max(FLOOR, ntiles // SHARE), ntiles)


def rows_of(tiles, ragged=0):
    """Rows of a corpus of `tiles` tiles; ragged: the last tile holds only that many rows."""
    return (tiles - 1) * 64 + (ragged or 64)


# name -> rows: 1 tile; around FLOOR and around S (the sample is the whole range, then stops growing);
# a ragged last tile of 17 rows; a range long enough for a sample of S tiles
RANGES = {
    "1_tile": rows_of(1),
    "floor-1": rows_of(FLOOR - 1),
    "floor": rows_of(FLOOR),
    "floor+3_ragged": rows_of(FLOOR + 4, 17),
    "S-1": rows_of(S - 1),
    "S": rows_of(S),
    "S+3_ragged": rows_of(S + 4, 17),
    "share_x_S+3_ragged": rows_of(SHARE * S + 4, 17),
}


def test_ranges_cover_the_sample_sizes():
    assert sample_tiles(1) == 1 and sample_tiles(FLOOR - 1) == FLOOR - 1 and sample_tiles(FLOOR + 4) == FLOOR
    assert sample_tiles(SHARE * S + 4) == S
    assert N == rows_of(S + 4, 17)


_made = {}


@pytest.fixture(scope="module")
def make(ctx, orc):
    """make(name, n, d, metric, dead, tweak): a corpus with NQ_MAX queries, built once per name."""

    def get(name, n, d=128, metric=METRIC_L2, dead=(), tweak=None):
        if name not in _made:
            rows = orc.synth_rows(7000 + len(_made), 0, n, d, 0)
            qs = orc.synth_rows(7500 + len(_made), 0, NQ_MAX, d, 0)
            if tweak:
                tweak(rows, qs)
            _made[name] = Corp(ctx, orc, metric, rows, qs, dead)
        return _made[name]

    yield get
    for cp in _made.values():
        cp.destroy()
    _made.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RANGES))
def test_range_against_sample(make, name):
    n = RANGES[name]
    cp = make("range_" + name, n)
    for k in (10, 65):
        cp.check(QB + 1, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1_tile", "floor+3_ragged", "S+3_ragged"])
def test_range_with_17_live_rows(make, name):
    """17 live rows in all: three in the first tile, the rest spread to the last row."""
    n = RANGES[name]
    live = np.unique(np.concatenate([[0, 5, min(63, n - 2)], np.linspace(0, n - 1, 14).astype(np.int64)]))
    extra = [r for r in range(n) if r not in set(live.tolist())]
    live = np.concatenate([live, extra[:17 - len(live)]])
    assert len(live) == 17
    cp = make("live17_" + name, n, dead=np.setdiff1d(np.arange(n), live))
    for k in (1, 10, 17, 18, 65):
        cp.check(QB + 1, k)
    ids, dists, counts = device_search(cp.c.lib, cp.c, cp.c.lib.wvg_search_device_pipelined, cp.pq[:3], 64, reps=1)[0]
    assert np.all(counts == 17)


@pytest.mark.gpu
@pytest.mark.parametrize("nq", sorted({2, QB - 1, QB, QB + 1, 33}))
def test_query_counts_against_the_query_block(make, nq):
    cp = make("range_S+3_ragged", N)
    for k in (10, 129):
        cp.check(nq, k)


@pytest.mark.gpu
def test_more_query_blocks_than_counters(ctx, orc):
    """COUNTERS x QB + 3 queries: two query blocks arrive at one counter, whose last arriver merges both."""
    nq = _header_const("PRO_COUNTERS") * QB + 3
    cp = Corp(ctx, orc, METRIC_L2, orc.synth_rows(7950, 0, N, 128, 0), orc.synth_rows(7951, 0, nq, 128, 0), DEAD)
    try:
        for k in (10, 65):
            cp.check(nq, k)
            cp.check(nq - 4, k)
    finally:
        cp.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 10, 64, 65, 128, 256])
def test_k(make, k):
    """E = 1, 2, 4 and lists of up to 64 keys per tile; a sample with 40 live rows (k above it: open
    seeds, the results come from the rest) and a corpus with 100 live rows (k above it)."""
    cp = make("range_S+3_ragged", N)
    cp.check(QB + 1, k)
    st = sample_tiles(TILES) * 64
    few = np.linspace(1, st - 2, 40).astype(np.int64)
    cp = make("sample_40_live", N, dead=np.setdiff1d(np.arange(st), few))
    cp.check(QB + 1, k)
    live = np.concatenate([few, np.linspace(st, N - 1, 60).astype(np.int64)])
    cp = make("corpus_100_live", N, dead=np.setdiff1d(np.arange(N), live))
    cp.check(QB + 1, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one_tile", "first_and_last", "whole_sample"])
def test_empty_pairs_still_arrive(make, case):
    """Deleted sample tiles: their waves publish empty lists and arrive like any other."""
    st = sample_tiles(TILES)
    if case == "one_tile":
        dead = np.arange(5 * 64, 6 * 64)
    elif case == "first_and_last":
        dead = np.concatenate([np.arange(64), np.arange((st - 1) * 64, st * 64)])
    else:
        dead = np.arange(st * 64)
    cp = make("dead_" + case, N, dead=dead)
    for nq in (2, QB + 1):
        for k in (10, 65):
            cp.check(nq, k)


_fcorp = []


@pytest.fixture(scope="module")
def fcorp(ctx, orc):
    if not _fcorp:
        _fcorp.append(FCorp(ctx, orc, METRIC_L2, orc.synth_rows(7900, 0, N, 128, 0), orc.synth_rows(7901, 0, NQ_MAX, 128, 0), DEAD))
    yield _fcorp[0]
    _fcorp.pop().destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 65])
def test_filtered_empty_pairs(fcorp, k):
    """Query 0's list names no sample row (every one of its pairs is empty) beside all-ones lists;
    then all-ones lists for everyone; then a window that begins after the sample."""
    st = sample_tiles(TILES)
    ones = np.ones(N, bool)
    none_in_sample = ones.copy()
    none_in_sample[:st * 64] = False
    for nq in (QB - 1, QB + 1):
        calls = [[none_in_sample if i == 0 else ones for i in range(nq)], [ones] * nq]
        fcorp.check_filtered(nq, k, calls)
        fcorp.check_filtered(nq, k, calls, (BASE + 64 * st, TILES - st))
    assert WINDOWS["cover"] == (BASE, TILES)


@pytest.mark.gpu
def test_special_values(make):
    """A NaN row and a +inf row inside the sample, a NaN query beside finite ones: the lexicographic
    order only."""

    def tweak(rows, qs):
        rows[70, 3] = np.nan
        rows[200, 9] = np.inf
        rows[N - 5, 1] = np.nan
        qs[1, 0] = np.nan

    cp = make("special", N, tweak=tweak)
    for nq in (3, QB + 1):
        for k in (1, 10, 65):
            cp.check(nq, k, heap=False)


def _equal(got, ref, tag):
    ids, dists, counts = got
    for qi, (ri, rd, rc) in enumerate(ref):
        cnt = int(counts[qi])
        assert cnt == int(rc[0]), (tag, qi)
        assert np.array_equal(ids[qi], ri[0]), (tag, qi)
        assert np.array_equal(bits(dists[qi]), bits(rd[0])), (tag, qi)
        assert np.all(ids[qi][cnt:] == UINT64_MAX) and np.all(np.isposinf(dists[qi][cnt:])), (tag, qi)


@pytest.mark.gpu
@pytest.mark.parametrize("junk", [False, True])
def test_one_workspace_mixed_calls(fcorp, junk):
    """Calls of different (nq, k) and entry points in order on one workspace, zero-filled once, no sync
    between them: the counters keep their place whatever the layout, and every call leaves them at zero.
    junk: between the calls everything behind the 256-byte status block is filled with 0x01 bytes, the
    "whatever an earlier call left there" of the contract made certain: a call may rely on nothing in its
    layout that it has not written itself.  A counter that lay there would start from 0x01010101 and never
    complete, and a seed that no merge has written would read as a tiny positive distance and empty the
    results; so would the seeds of a call whose counters the call before had not put back."""
    import torch

    cp, lib = fcorp, fcorp.c.lib
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    ones = np.ones(N, bool)
    tenth = np.random.default_rng(5).random(N) < 0.10
    masks = [tenth if i % 2 else ones for i in range(16)]
    words = torch.from_numpy(window_words(masks, BASE, TILES).view(np.int64)).to(dev)
    # (kind, nq, k)
    calls = [("pipe", 16, 10), ("device", 33, 100), ("pipe", 16, 10), ("pipe", 1, 10), ("pipe", 2, 256), ("filt", 16, 10),
             ("pipe", 16, 10)]
    refs = []
    for kind, nq, k in calls:  # the references first: they synchronize
        if kind == "filt":
            refs.append([cp.host(qi, k, masks[qi]) for qi in range(nq)])
        else:
            refs.append(cp.singles(k)[:nq])
    wsb = max(lib.wvg_search_workspace_size(cp.c.handle, nq, k) for _, nq, k in calls)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(np.ascontiguousarray(cp.pq, dtype=np.float32)).to(dev)
    outs = []
    for kind, nq, k in calls:
        oi = torch.full((nq, k), 7, dtype=torch.int64, device=dev)
        od = torch.full((nq, k), -7.0, dtype=torch.float32, device=dev)
        oc = torch.full((nq,), 77, dtype=torch.int32, device=dev)
        args = (oi.data_ptr(), od.data_ptr(), oc.data_ptr(), ws.data_ptr(), ws.numel(), st)
        if junk and outs:
            ws[256:].fill_(1)  # on the calls' stream
        if kind == "pipe":
            _lib.check(lib.wvg_search_device_pipelined(cp.c.handle, tq.data_ptr(), nq, k, *args))
        elif kind == "device":
            _lib.check(lib.wvg_search_device(cp.c.handle, tq.data_ptr(), nq, k, *args))
        else:
            _lib.check(lib.wvg_search_device_pipelined_filtered(cp.c.handle, tq.data_ptr(), nq, k, words.data_ptr(), TILES,
                                                                BASE, *args))
        outs.append((oi, od, oc))
    torch.cuda.synchronize()
    _lib.check(lib.wvg_search_device_check(cp.c.ctx.handle, ws.data_ptr(), st))
    for ci, ((kind, nq, k), (oi, od, oc)) in enumerate(zip(calls, outs)):
        got = (oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32))
        _equal(got, refs[ci], (ci, kind, nq, k))


@pytest.mark.gpu
def test_graph_capture_and_three_replays(fcorp):
    import torch

    cp, lib = fcorp, fcorp.c.lib
    dev = torch.device("cuda:0")
    nq, k = 16, 10
    ref = cp.singles(k)[:nq]
    ws = torch.zeros(lib.wvg_search_workspace_size(cp.c.handle, nq, k), dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(np.ascontiguousarray(cp.pq[:nq], dtype=np.float32)).to(dev)
    oi = torch.zeros((nq, k), dtype=torch.int64, device=dev)
    od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    oc = torch.zeros(nq, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(lib.wvg_search_device_pipelined(cp.c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                                   oc.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert int(oc.sum()) == 0  # captured, not run
    for rep in range(3):
        oi.fill_(7)
        od.fill_(-7.0)
        oc.fill_(77)
        g.replay()
        torch.cuda.synchronize()
        _equal((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)), ref, rep)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(METRIC_DOT, 768), (METRIC_DOT, 128)])
def test_768_and_dot(make, shape):
    """d = 768: the prologue without a sample (every seed opened by the new grid); dot at d = 128: a
    seeded launch the screen does not take."""
    metric, d = shape
    cp = make("dims_%d_%d" % shape, N, d=d, metric=metric, dead=DEAD)
    plan = cp.c.search_device_plan(QB + 1, 10)
    assert plan["shared_rows"] == 1 and plan["seeded"] == int(d == 128) and plan["screened"] == 0, plan
    for nq in (2, QB + 1):
        for k in (10, 65):
            cp.check(nq, k)

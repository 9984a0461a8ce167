"""The shadow-fed screened shared-row scan (scan_f32_qshare_shadow_kernel and its filtered twin,
wvg_qshare.hip): a screened wvg_search_device_pipelined call in a context with batch_screen != 0
screens every tile from the corpus's bf16 shadow (fragments + norm bounds, the one l2-squared batches
use) and gathers the fp32 values of admitted (query, row) pairs only.  Results must not change: the
calls are compared bit for bit (ids, distance bits, counts) with nq separate wvg_search_device calls,
with the oracle, and with the same corpus in a batch_screen = 0 context, which keeps the fp32-screened
kernel (the fallback) covered.  Every call runs twice back to back, so both walk directions run.

Shapes are those of test_gpu_qshare_seed.py: N = (S + 3) * 64 + 17 rows, d = 128, nq in (2, 16, 17, 33),
k in (1, 10, 64).  The split_rounds and crowded_lane corpora come from test_gpu_qshare_rows.py (the NaN
row, the zero row, the mean row admitted for every query of every pass, a deleted exact match, ties
broken by id, the ragged last tile).  operand_map plants what the new MFMA operand map can get wrong: a
lane of the shadow-fed kernel holds four queries 4 g .. 4 g + 3 x four rows i, i + 16, i + 32, i + 48 (the
other operand choice would hold one query x rows 16 rg + 4 g .. + 3), so in one tile outside the sample
two rows 16 apart and two rows 4 apart are close to one query (one lane then holds two admitted pairs
under either choice), one row is close to queries q, q + 4, q + 8, q + 12 and one to q .. q + 3.  The
preconditions are checked on oracle distances on the CPU before any GPU call: every planted pair lies
below the query's 10th distance over the live sample, the negatives further than 2.0 above it.
"""
import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import KIND_F32, METRIC_DOT, METRIC_L2
from weaviate_amd.device import Context, Corpus

from test_gpu_k1_matrix import device_search
from test_gpu_parity import bits
from test_gpu_qshare_filter import FCorp, filtered_search, window_words
from test_gpu_qshare_rows import CORPORA, OUT, T, _dist, _sample_tenth
from test_gpu_qshare_seed import BASE, DEAD, NQS, Corp, N

D = 128
KS = (1, 10, 64)
NQ_MAX = max(NQS)
TILES = (N + 63) // 64
# operand_map: lanes of the planted tile
L_A0, L_A16, L_B0, L_B4, L_STRIDE4, L_RUN4 = 2, 18, 33, 37, 44, 51
QA, QS4, QR4 = 0, 2, 20  # the query of the four near rows; q of (q, q + 4, q + 8, q + 12); q of (q .. q + 3)


def _operand_map(orc):
    rows = orc.synth_rows(6101, 0, N, D, 0)
    qs = orc.synth_rows(6102, 0, NQ_MAX, D, 0)
    noise = np.random.default_rng(6103).uniform(-9e-4, 9e-4, (4, D)).astype(np.float32)
    for i, lane in enumerate((L_A0, L_A16, L_B0, L_B4)):
        rows[T + lane] = qs[QA] + noise[i]
    rows[T + L_STRIDE4] = qs[[QS4, QS4 + 4, QS4 + 8, QS4 + 12]].mean(axis=0, dtype=np.float64).astype(np.float32)
    rows[T + L_RUN4] = qs[QR4:QR4 + 4].mean(axis=0, dtype=np.float64).astype(np.float32)
    tenth = _sample_tenth(orc, rows, qs, DEAD)
    planted = [(QA, lane) for lane in (L_A0, L_A16, L_B0, L_B4)]
    planted += [(QS4 + 4 * i, L_STRIDE4) for i in range(4)] + [(QR4 + i, L_RUN4) for i in range(4)]
    for j, lane in planted:
        assert _dist(orc, qs[j], rows[T + lane]) < tenth[j], (j, lane, tenth[j])
    for lane in (L_A0, L_A16, L_B0, L_B4):  # the negatives: not query 1's rows
        assert _dist(orc, qs[1], rows[T + lane]) > tenth[1] + 2.0, (lane, tenth[1])
    return rows, qs, DEAD


BUILDERS = {**{name: b for name, (b, _) in CORPORA.items()}, "operand_map": _operand_map}
HEAP = {**{name: h for name, (_, h) in CORPORA.items()}, "operand_map": True}


@pytest.fixture(scope="module")
def exact_ctx():
    c = Context(0, batch_screen=0)  # the stream stays off the shadow: the fp32-screened kernel
    yield c
    c.close()


_pairs = {}


@pytest.fixture(scope="module")
def pairs(ctx, exact_ctx, orc):
    """name -> (the corpus in the default context, the same rows in the batch_screen = 0 context)."""
    def get(name):
        if name not in _pairs:
            rows, qs, dead = BUILDERS[name](orc)  # asserts its preconditions before the first GPU call
            _pairs[name] = (Corp(ctx, orc, METRIC_L2, rows, qs, dead), Corp(exact_ctx, orc, METRIC_L2, rows, qs, dead))
            _pairs[name][0].rows = rows
        return _pairs[name]

    yield get
    for a, b in _pairs.values():
        a.destroy()
        b.destroy()
    _pairs.clear()


def _same(got, want, tag=None):
    assert np.array_equal(got[2], want[2]), tag
    assert np.array_equal(got[0], want[0]), tag
    assert np.array_equal(bits(got[1]), bits(want[1])), tag


def _stream(c, pq, k, reps=2):
    return device_search(c.lib, c, c.lib.wvg_search_device_pipelined, pq, k, reps=reps)


@pytest.mark.gpu
def test_route(ctx, exact_ctx, orc):
    rows = orc.synth_rows(6201, 0, N, D, 0)
    ids = np.arange(N, dtype=np.uint64)
    made = []

    def corpus(cx, metric, d, r):
        c = Corpus(cx, KIND_F32, metric, d, N)
        c.upsert(ids, r)
        made.append(c)
        return c

    own = Context(0, cache_reuse=0)
    try:
        c = corpus(ctx, METRIC_L2, D, rows)
        for nq in NQS:
            for k in KS:
                assert c.search_device_plan(nq, k)["screened"] == 1
                assert c.search_device_shadow(nq, k) == {"reads_shadow": 1, "shadow_bytes_per_row": 2 * D + 4}, (nq, k)
        no = {"reads_shadow": 0, "shadow_bytes_per_row": 0}
        assert c.search_device_shadow(16, 65) == no
        assert c.search_device_shadow(1, 10) == no
        assert c.search_device_shadow(0, 10) == no
        assert corpus(ctx, METRIC_L2, 768, orc.synth_rows(6202, 0, N, 768, 0)).search_device_shadow(16, 10) == no
        assert corpus(ctx, METRIC_DOT, D, rows).search_device_shadow(16, 10) == no
        assert corpus(exact_ctx, METRIC_L2, D, rows).search_device_shadow(16, 10) == no
        assert corpus(own, METRIC_L2, D, rows).search_device_shadow(16, 10) == no
        # the workspace does not depend on the shadow's state, and the unscreened shapes allocate none: only
        # the first corpus's screened search changes what a batch plan reports as existing
        before = c.lib.wvg_search_workspace_size(c.handle, 16, 10)
        _stream(c, rows[:16], 10, reps=1)
        assert c.lib.wvg_search_workspace_size(c.handle, 16, 10) == before
    finally:
        for c in made:
            c.destroy()
        own.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("name", list(BUILDERS))
def test_same_bits_as_singles_oracle_and_fallback(pairs, name, nq):
    a, b = pairs(name)
    assert a.c.search_device_shadow(nq, 10)["reads_shadow"] == 1 and b.c.search_device_shadow(nq, 10)["reads_shadow"] == 0
    for k in KS:
        a.check(nq, k, heap=HEAP[name])  # twice back to back: the singles bit for bit, the oracle
        for got, want in zip(_stream(a.c, a.pq[:nq], k), _stream(b.c, b.pq[:nq], k)):
            _same(got, want, (name, nq, k))


@pytest.mark.gpu
def test_operand_map_plants_come_back(pairs):
    a, _ = pairs("operand_map")
    ids, dists, counts = _stream(a.c, a.pq, 10, reps=1)[0]
    for lane in (L_A0, L_A16, L_B0, L_B4):
        assert BASE + T + lane in ids[QA], lane
    for i in range(4):
        assert BASE + T + L_STRIDE4 in ids[QS4 + 4 * i], i
        assert BASE + T + L_RUN4 in ids[QR4 + i], i


@pytest.mark.gpu
def test_shadow_follows_writes(ctx, exact_ctx, orc):
    """Upserts, deletes and growth between searches: a stale shadow fails the first step (the planted row
    would be screened with its old values and skipped)."""
    rows = orc.synth_rows(6301, 0, N, D, 0)
    qs = orc.synth_rows(6302, 0, 16, D, 0)
    a, b = Corpus(ctx, KIND_F32, METRIC_L2, D, N), Corpus(exact_ctx, KIND_F32, METRIC_L2, D, N)
    k = 10
    try:
        for x in (a, b):
            x.upsert(np.arange(N, dtype=np.uint64), rows)
        first = _stream(a, qs, k)
        for got, want in zip(first, _stream(b, qs, k)):
            _same(got, want, "first")
        near = int(first[0][0][3][0])          # query 3's nearest row so far
        plant = OUT + 64 + 7                   # a tile outside the sample
        gone = int(first[0][0][5][0])          # query 5's nearest row: deleted
        assert len({near, plant, gone}) == 3
        far = np.full(D, 10.0, np.float32)
        for x in (a, b):
            x.upsert(np.array([plant, near], np.uint64), np.stack([qs[3], far]))
            x.delete(np.array([gone], np.uint64))
        second = _stream(a, qs, k)
        for got, want in zip(second, _stream(b, qs, k)):
            _same(got, want, "after writes")
        for ids, dists, _ in second:
            assert ids[3][0] == plant and bits(dists[3][:1])[0] == 0
            assert near not in ids[3] and gone not in ids[5]
        for x in (a, b):
            x.reserve(N + 5000)                # realloc: the shadow is dropped and built again
            x.upsert(np.array([N + 4000], np.uint64), qs[6][None])
        third = _stream(a, qs, k)
        for got, want in zip(third, _stream(b, qs, k)):
            _same(got, want, "after growth")
        for ids, dists, _ in third:
            assert ids[6][0] == N + 4000 and bits(dists[6][:1])[0] == 0
            assert ids[3][0] == plant
    finally:
        a.destroy()
        b.destroy()


@pytest.fixture(scope="module")
def fcorp(ctx, orc):
    rows, qs, dead = _operand_map(orc)
    cp = FCorp(ctx, orc, METRIC_L2, rows, qs, dead)
    yield cp
    cp.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("nq", NQS)
def test_filtered(fcorp, nq):
    """Per-query allow lists: all-ones, 10 %, and a list of zero for the planted tile, against the host
    wvg_search with the same lists and the oracle (FCorp.check_filtered)."""
    rng = np.random.default_rng(6400 + nq)
    ones = np.ones(N, bool)
    hole = ones.copy()
    hole[T:T + 64] = False
    lists = [ones, rng.random(N) < 0.10, hole]
    calls = [[lists[(i + s) % 3] for i in range(nq)] for s in (0, 1)]
    assert fcorp.c.search_device_shadow(nq, 10)["reads_shadow"] == 1
    for k in KS:
        fcorp.check_filtered(nq, k, calls)
    if nq == NQ_MAX:  # a query whose list has a zero word for the planted tile does not get its rows
        got = filtered_search(fcorp.c, fcorp.pq[:1], 10, [window_words([hole], BASE, TILES)], BASE, TILES)[0]
        assert not np.isin(got[0][0], BASE + T + np.arange(64, dtype=np.uint64)).any()


def _captured(c, pq, k, warm):
    """One call captured in a torch.cuda.graph (after `warm` eager calls) and replayed twice."""
    import torch

    lib = c.lib
    dev = torch.device("cuda:0")
    nq = len(pq)
    ws = torch.zeros(lib.wvg_search_workspace_size(c.handle, nq, k), dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(np.ascontiguousarray(pq, dtype=np.float32)).to(dev)
    oi = torch.zeros((nq, k), dtype=torch.int64, device=dev)
    od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    oc = torch.zeros(nq, dtype=torch.int32, device=dev)

    def call():
        _lib.check(lib.wvg_search_device_pipelined(c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                                   oc.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   torch.cuda.current_stream().cuda_stream))

    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    for t in (oi, od, oc):
        t.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    torch.cuda.synchronize()
    assert int(oc.sum()) == 0  # captured, not run
    outs = []
    for _ in range(2):
        oi.fill_(7)
        od.fill_(-7.0)
        oc.fill_(77)
        g.replay()
        torch.cuda.synchronize()
        outs.append((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("warm", [1, 0])
def test_capture(ctx, pairs, orc, warm):
    """warm = 1: the shadow is there and clean, the capture records the shadow-fed kernel.  warm = 0: a fresh
    corpus without a shadow, nothing is allocated under capture and the fallback kernel is recorded."""
    a, b = pairs("operand_map")
    nq, k = 17, 10
    want = _stream(b.c, b.pq[:nq], k, reps=1)[0]
    if warm:
        c = a.c
    else:
        rows, _, dead = _operand_map(orc)
        c = Corpus(ctx, KIND_F32, METRIC_L2, D, N, id_base=BASE)
        c.upsert(a.ids, rows)
        c.delete(a.ids[np.asarray(dead, np.int64)])
    try:
        for got in _captured(c, a.pq[:nq], k, warm):
            _same(got, want, warm)
    finally:
        if not warm:
            c.destroy()


@pytest.mark.gpu
def test_special_queries_on_a_shared_workspace(pairs):
    """A NaN query and a query of norm 2^57 admit everything (Cq = NaN / -inf: no pair is skipped) and are
    still exact; the two routes alternate on ONE workspace, so nothing the other left is picked up."""
    import torch

    a, b = pairs("operand_map")
    lib = a.c.lib
    dev = torch.device("cuda:0")
    nq, k = 17, 10
    qs = a.pq[:nq].copy()
    qs[4, 9] = np.nan
    qs[11] = 0.0
    qs[11, 3] = 2.0 ** 57
    ws = torch.zeros(max(lib.wvg_search_workspace_size(x.c.handle, nq, k) for x in (a, b)), dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(qs).to(dev)
    outs = []
    for x in (a, b, a, b):
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oc = torch.empty(nq, dtype=torch.int32, device=dev)
        _lib.check(lib.wvg_search_device_pipelined(x.c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                                   oc.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   torch.cuda.current_stream().cuda_stream))
        outs.append((oi, od, oc))
    torch.cuda.synchronize()
    outs = [(oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)) for oi, od, oc in outs]
    singles = [device_search(lib, a.c, lib.wvg_search_device, qs[[qi]], k, reps=1)[0] for qi in range(nq)]
    for got in outs:
        _same(got, outs[1], "routes")
        for qi in range(nq):
            _same(tuple(x[qi] for x in got), tuple(x[0] for x in singles[qi]), qi)
    live = a.valid.astype(bool)  # and the oracle's lexicographic top-k of the huge query (distances near 2^114)
    li, ld = a.orc.lex_topk(a.orc.dist_all(METRIC_L2, qs[11], a.rows)[live], a.ids[live], k)
    assert np.array_equal(outs[0][0][11], li) and np.array_equal(bits(outs[0][1][11]), bits(ld))

"""Per-query allow lists in the shared-row query stream
(wvg_search_device_pipelined_filtered; scan_f32_qshare_filt_kernel,
scan_f32_qshare_screen_filt_kernel and qshare_seed_filt_kernel, wvg_qshare.hip).

One launch answers nq queries, each with an allow list of its own: a window of
the docID space on the device, [nq][stride] words whose bit b of word w is docID
first_id + 64 w + b.  The outputs must be exactly what nq host calls
wvg_search(c, q_i, 1, k, allow_i) write -- ids, distance bits, counts, padding --
and the oracle's lexicographic top-k over valid & allowed.  Every call runs
twice back to back on one workspace without a sync in between, so both walk
directions run, and the second call carries different lists, so a seed or a
hand-off word left by the first would show.

The corpora are those of test_gpu_qshare_seed.py: N = (S + 3) * 64 + 17 rows at
id_base 6,400,000, deleted rows inside, at the edge of and outside the
prologue's sample of S tiles.  Query i of a call takes list (i + shift) mod 10 of
LISTS, so one pass of the scan mixes all of them.  The lists' properties (e.g.
"exactly k - 1 allowed live rows in the sample") are asserted on the CPU before
the first GPU call.
"""
import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import METRIC_COSINE, METRIC_DOT, METRIC_L2, METRIC_MANHATTAN
from weaviate_amd.device import Context

from test_gpu_parity import bits
from test_gpu_qshare_seed import BASE, DEAD, NQS, Corp, N, S
from test_gpu_qshare_rows import L_COPY1, L_MEAN, L_MID01, L_Q1, T, _split_rounds

UINT64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
NQ_MAX = max(NQS)
OUT = S * 64                      # first row outside the sample
TILES = (N + 63) // 64
RAGGED = (TILES - 1) * 64         # first row of the ragged last tile
NLISTS = 10
LIVE = np.ones(N, bool)
LIVE[DEAD] = False


def make_lists(k, seed):
    """The ten lists of the issue as boolean masks over the N rows (index = list number - 1)."""
    rng = np.random.default_rng(seed)
    z = lambda: np.zeros(N, bool)
    lists = [np.ones(N, bool), rng.random(N) < 0.10, rng.random(N) < 0.01]
    m = z(); m[OUT + 100] = True; lists.append(m)            # 4: a single live id outside the sample
    m = z(); m[1000] = True; lists.append(m)                  # 5: a single deleted id
    lists.append(z())                                         # 6: all zeros
    m = z(); m[200:600] = True; lists.append(m)               # 7: a range wholly inside the sample
    m = z(); m[OUT + 70:OUT + 180] = True; lists.append(m)    # 8: a range wholly outside the sample
    m = z()                                                   # 9: k - 1 allowed live rows in the sample, more outside
    inside = np.flatnonzero(LIVE[:OUT])
    m[inside[np.linspace(3, len(inside) - 1, k - 1).astype(np.int64)]] = True
    m[OUT + 10:OUT + 10 + 2 * k + 8] = True
    lists.append(m)
    m = z(); m[RAGGED:] = True; lists.append(m)               # 10: only the ragged last tile
    # the preconditions (CPU)
    assert LIVE[OUT + 100] and not LIVE[1000]
    assert 0 < (lists[2] & LIVE).sum() < 64, "list 3: fewer than 64 allowed live rows, so k = 64 returns fewer than k"
    assert (lists[1] & LIVE).sum() > 64
    assert lists[6][OUT:].sum() == 0 and (lists[6] & LIVE)[:OUT].sum() >= 256
    assert lists[7][:OUT].sum() == 0 and (lists[7] & LIVE).sum() >= 100
    assert (lists[8] & LIVE)[:OUT].sum() == k - 1, "list 9: exactly k - 1 allowed live rows in the sample"
    assert (lists[8] & LIVE)[OUT:].sum() >= min(k + 1, 150), "list 9: and more outside it"
    assert lists[9][:RAGGED].sum() == 0 and (lists[9] & LIVE).sum() == N - RAGGED - 1  # (row N - 1 is deleted)
    return lists


def window_words(masks, first_id, stride, junk=True):
    """[nq][stride] uint64 words of the window beginning at docID first_id: the rows' bits, and with
    junk every bit that names no row of the corpus set (such bits must be ignored)."""
    nbits = 64 * stride
    doc = first_id + np.arange(nbits, dtype=np.int64)
    row = doc - BASE
    inside = (row >= 0) & (row < N)
    out = np.zeros((len(masks), max(stride, 1)), np.uint64)
    for q, m in enumerate(masks):
        b = np.zeros(nbits, np.uint8)
        b[inside] = m[row[inside]]
        if junk:
            b[~inside] = 1
        if stride:
            out[q, :stride] = np.packbits(b, bitorder="little").view(np.uint64)
    return out[:, :stride] if stride else out[:, :0]


def in_window(first_id, stride):
    """Mask over the rows of the docIDs inside [first_id, first_id + 64 stride)."""
    doc = BASE + np.arange(N, dtype=np.int64)
    return (doc >= first_id) & (doc < first_id + 64 * stride)


# name -> (first docID, words): covering the corpus; beginning 5 tiles in and ending 3 tiles before the
# corpus does; beginning 7 tiles before the corpus (and ending one word after it); empty
WINDOWS = {
    "cover": (BASE, TILES),
    "inner": (BASE + 64 * 5, TILES - 5 - 3),
    "before": (BASE - 64 * 7, TILES + 7 + 1),
    "empty": (BASE, 0),
}


def filtered_search(c, pq, k, calls, first_id, stride, fn=None):
    """`len(calls)` filtered calls back to back on one workspace, no sync between them; calls[i] = the
    [nq][stride] words of call i, or None for d_allow = NULL.  [(ids, dists, counts)] per call."""
    import torch

    lib = c.lib
    dev = torch.device("cuda:0")
    nq = len(pq)
    ws = torch.zeros(lib.wvg_search_workspace_size(c.handle, nq, k), dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(np.ascontiguousarray(pq, dtype=np.float32)).to(dev)
    # (an empty window still gets a valid pointer: NULL means "no filter")
    tws = [None if w is None else torch.from_numpy(np.ascontiguousarray(w).view(np.int64)).to(dev)
           for w in calls]
    pad = torch.zeros(8, dtype=torch.int64, device=dev)
    outs = []
    for tw in tws:
        oi = torch.full((nq, k), 7, dtype=torch.int64, device=dev)
        od = torch.full((nq, k), -7.0, dtype=torch.float32, device=dev)
        oc = torch.full((nq,), 77, dtype=torch.int32, device=dev)
        ap = 0 if tw is None else (tw.data_ptr() if tw.numel() else pad.data_ptr())
        rc = lib.wvg_search_device_pipelined_filtered(c.handle, tq.data_ptr(), nq, k, ap, stride, first_id, oi.data_ptr(),
                                                      od.data_ptr(), oc.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      torch.cuda.current_stream().cuda_stream)
        if fn is not None:
            fn(rc)
        else:
            _lib.check(rc)
        outs.append((oi, od, oc))
    torch.cuda.synchronize()
    return [(oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32))
            for oi, od, oc in outs]


class FCorp(Corp):
    """Corp with the raw queries (the host API prepares them itself) and the two references of a
    filtered query: the host wvg_search with the list as a global docID bitmap, and the oracle."""

    def __init__(self, cx, orc, metric, rows, qs, dead=()):
        super().__init__(cx, orc, metric, rows, qs, dead)
        self.raw = np.asarray(qs, np.float32)
        self._host = {}

    def host(self, qi, k, mask):
        key = (qi, k, mask.tobytes())
        if key not in self._host:
            words = np.zeros((BASE + self.n + 63) // 64, np.uint64)  # bitmap over global docIDs
            sub = np.zeros(((self.n + 63) // 64) * 64, np.uint8)
            sub[:self.n] = mask
            words[BASE // 64:] = np.packbits(sub, bitorder="little").view(np.uint64)
            self._host[key] = self.c.search(self.raw[[qi]], k, allow=words)
        return self._host[key]

    def check_filtered(self, nq, k, masks_per_call, window="cover"):
        first_id, stride = WINDOWS[window] if isinstance(window, str) else window
        inwin = in_window(first_id, stride)
        calls = [window_words(masks, first_id, stride) for masks in masks_per_call]
        # both references first (the host calls synchronize), then the back-to-back device calls
        refs = [[self.host(qi, k, masks[qi] & inwin) for qi in range(nq)] for masks in masks_per_call]
        outs = filtered_search(self.c, self.pq[:nq], k, calls, first_id, stride)
        for ci, (ids, dists, counts) in enumerate(outs):
            for qi in range(nq):
                eff = masks_per_call[ci][qi] & inwin
                ri, rd, rc = refs[ci][qi]
                cnt = int(counts[qi])
                tag = (ci, qi, k, window)
                assert cnt == int(rc[0]), tag
                assert np.array_equal(ids[qi], ri[0]), tag
                assert np.array_equal(bits(dists[qi]), bits(rd[0])), tag
                sel = self.valid.astype(bool) & eff
                li, ld = self.orc.lex_topk(self.all_d[qi][sel], self.ids[sel], k)
                assert cnt == len(li) and np.array_equal(ids[qi][:cnt], li), tag
                assert np.array_equal(bits(dists[qi][:cnt]), bits(ld)), tag
                assert np.all(ids[qi][cnt:] == UINT64_MAX) and np.all(np.isposinf(dists[qi][cnt:])), tag
                assert not np.isin(ids[qi][:cnt], self.ids[~eff]).any(), tag  # nothing outside the list or the window


def two_calls(nq, k):
    """Query i takes list (i + shift) mod 10; the second call shifts by 3 and draws other random lists."""
    a, b = make_lists(k, 100 + k), make_lists(k, 200 + k)
    return [[a[i % NLISTS] for i in range(nq)], [b[(i + 3) % NLISTS] for i in range(nq)]]


_corps = {}


@pytest.fixture(scope="module")
def corps(ctx, orc):
    def get(metric, d):
        if (metric, d) not in _corps:
            rows = orc.synth_rows(3000 + 7 * d + metric, 0, N, d, 0)
            qs = orc.synth_rows(4000 + 7 * d + metric, 0, NQ_MAX, d, 0)
            for k in (1, 10, 64, 65, 129, 256):
                make_lists(k, 100 + k)  # the lists' preconditions, before the first GPU call
            _corps[(metric, d)] = FCorp(ctx, orc, metric, rows, qs, DEAD)
        return _corps[(metric, d)]

    yield get
    for cp in _corps.values():
        cp.destroy()
    _corps.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("nq", NQS)
def test_l2_128_screened_and_whole_row_routes(corps, nq):
    """k <= 64: the screened filtered kernel; k = 65 and 256: the whole-row form at E = 2 and E = 4."""
    cp = corps(METRIC_L2, 128)
    for k in (1, 10, 64, 65, 256):
        cp.check_filtered(nq, k, two_calls(nq, k))


@pytest.mark.gpu
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("metric", [METRIC_DOT, METRIC_COSINE])
def test_dot_and_cosine_128(corps, metric, nq):
    cp = corps(metric, 128)
    for k in (10, 65):
        cp.check_filtered(nq, k, two_calls(nq, k))


@pytest.mark.gpu
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT])
def test_block_form_768(corps, metric, nq):
    cp = corps(metric, 768)
    for k in (10, 129):
        cp.check_filtered(nq, k, two_calls(nq, k))


@pytest.mark.gpu
@pytest.mark.parametrize("window", ["inner", "before", "empty"])
@pytest.mark.parametrize("shape", [(METRIC_L2, 128, 10), (METRIC_L2, 128, 65), (METRIC_DOT, 768, 10)])
def test_windows(corps, shape, window):
    """A window inside the corpus (rows outside it must not appear), one that begins before the
    corpus, and the empty one (every result empty)."""
    metric, d, k = shape
    cp = corps(metric, d)
    for nq in (2, 17):
        cp.check_filtered(nq, k, two_calls(nq, k), window)
    if window == "empty":
        ids, dists, counts = filtered_search(cp.c, cp.pq[:17], k, [np.zeros((17, 0), np.uint64)], BASE, 0)[0]
        assert np.all(counts == 0) and np.all(ids == UINT64_MAX) and np.all(np.isposinf(dists))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(METRIC_L2, 128, 10), (METRIC_L2, 128, 65), (METRIC_DOT, 768, 10)])
def test_null_allow_is_the_unfiltered_call(corps, shape):
    from test_gpu_k1_matrix import device_search

    metric, d, k = shape
    cp = corps(metric, d)
    lib = cp.c.lib
    for nq in (1, 17):
        want = device_search(lib, cp.c, lib.wvg_search_device_pipelined, cp.pq[:nq], k, reps=2)
        got = filtered_search(cp.c, cp.pq[:nq], k, [None, None], BASE, TILES)
        for (wi, wd, wc), (gi, gd, gc) in zip(want, got):
            assert np.array_equal(wi, gi) and np.array_equal(bits(wd), bits(gd)) and np.array_equal(wc, gc)


@pytest.mark.gpu
def test_unaligned_first_id_is_invalid_and_launches_nothing(corps):
    cp = corps(METRIC_L2, 128)
    k, nq = 10, 16
    masks = two_calls(nq, k)[0]
    rcs = []
    ids, dists, counts = filtered_search(cp.c, cp.pq[:nq], k, [window_words(masks, BASE, TILES)], BASE + 32, TILES,
                                         fn=rcs.append)[0]
    assert rcs == [_lib.WVG_ERR_INVALID]
    assert np.all(ids == np.uint64(7)) and np.all(dists == -7.0) and np.all(counts == 77)  # the outputs as they were


FALLBACK_LISTS = (1, 5, 7)  # lists 2, 6 and 8


def _fallback_calls(nq, k):
    a, b = make_lists(k, 300 + k), make_lists(k, 400 + k)
    return [[a[FALLBACK_LISTS[i % 3]] for i in range(nq)], [b[FALLBACK_LISTS[(i + 1) % 3]] for i in range(nq)]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nq1", "manhattan", "d96", "cache_reuse0"])
def test_fallback_routes(ctx, orc, corps, case):
    """Calls the shared-row kernel does not take: one query (the query-stream kernel's window),
    and K1 with per-query windows + the merge for a manhattan corpus, d = 96 and cache_reuse = 0."""
    k = 10
    if case == "nq1":
        cp = corps(METRIC_L2, 128)
        a, b = make_lists(k, 300 + k), make_lists(k, 400 + k)
        for shift in range(3):
            calls = [[a[FALLBACK_LISTS[shift]]], [b[FALLBACK_LISTS[(shift + 1) % 3]]]]
            cp.check_filtered(1, k, calls)
            cp.check_filtered(1, k, calls, "inner")
        return
    own_ctx = Context(0, cache_reuse=0) if case == "cache_reuse0" else None
    metric = METRIC_MANHATTAN if case == "manhattan" else METRIC_L2
    d = 96 if case == "d96" else 128
    rows = orc.synth_rows(5000 + d + metric, 0, N, d, 0)
    qs = orc.synth_rows(5100 + d + metric, 0, 5, d, 0)
    cp = FCorp(own_ctx or ctx, orc, metric, rows, qs, DEAD)
    try:
        for nq in (2, 5):
            cp.check_filtered(nq, k, _fallback_calls(nq, k))
        cp.check_filtered(5, k, _fallback_calls(5, k), "inner")
        cp.check_filtered(5, k, _fallback_calls(5, k), "before")
    finally:
        cp.destroy()
        if own_ctx:
            own_ctx.close()


@pytest.mark.gpu
def test_planted_tile_forbidden_rows_are_not_scored(ctx, orc):
    """The split_rounds corpus of test_gpu_qshare_rows.py: the rows at lanes L_Q1 (q1 + noise) and
    L_COPY1 (a deleted copy of q1) of the planted tile are forbidden for query 1 and allowed for query 0.
    The screen would admit L_Q1 for query 1 (it lies below query 1's sample bound): it must not come back
    for query 1, and the other queries -- those sharing a lane with a forbidden pair included -- get what
    they get alone.  The second call also forbids query 1 the lanes every query is admitted on."""
    rows, qs, dead = _split_rounds(orc)  # asserts the planted pairs' preconditions on the CPU
    allow_all = np.ones(N, bool)
    m1 = allow_all.copy()
    m1[[T + L_Q1, T + L_COPY1]] = False
    m2 = m1.copy()
    m2[[T + L_MEAN, T + L_MID01]] = False
    # precondition (oracle): alone and unfiltered, query 1 returns the row at L_Q1
    live = np.ones(N, bool)
    live[dead] = False
    d1 = orc.dist_all(METRIC_L2, qs[1], rows)
    top = orc.lex_topk(d1[live], (BASE + np.arange(N, dtype=np.uint64))[live], 10)[0]
    assert BASE + T + L_Q1 in top and BASE + T + L_MEAN in top
    cp = FCorp(ctx, orc, METRIC_L2, rows, qs, dead)
    try:
        for nq in (2, 17, 33):
            for k in (1, 10, 64):
                calls = [[m1 if i == 1 else allow_all for i in range(nq)], [m2 if i == 1 else allow_all for i in range(nq)]]
                cp.check_filtered(nq, k, calls)
        calls = [[m1 if i == 1 else allow_all for i in range(17)]]
        ids, _, _ = filtered_search(cp.c, cp.pq[:17], 10, [window_words(calls[0], BASE, TILES)], BASE, TILES)[0]
        assert BASE + T + L_Q1 not in ids[1] and BASE + T + L_COPY1 not in ids[1]
        assert BASE + T + L_MEAN in ids[1] and BASE + T + L_MEAN in ids[0]
    finally:
        cp.destroy()


@pytest.mark.gpu
def test_python_wrappers_pass_the_window_through(corps):
    """device.allow_window + Corpus.search_device_pipelined and ShardedFlatIndex.search_device(allow=...)
    give what the entry point gives with the same lists."""
    import torch

    from weaviate_amd.device import allow_window
    from weaviate_amd.shard import ShardedFlatIndex

    cp = corps(METRIC_L2, 128)
    nq, k = 17, 10
    masks = two_calls(nq, k)[0]
    first_id, stride = WINDOWS["inner"]
    want_i, want_d, want_c = filtered_search(cp.c, cp.pq[:nq], k, [window_words(masks, first_id, stride, junk=False)],
                                             first_id, stride)[0]
    words = allow_window([cp.ids[m] for m in masks], first_id, stride)
    assert np.array_equal(words, window_words(masks, first_id, stride, junk=False))
    dev = torch.device("cuda:0")
    tq = torch.from_numpy(np.ascontiguousarray(cp.pq[:nq])).to(dev)
    tw = torch.from_numpy(words.view(np.int64)).to(dev)
    ids, dists, counts = ShardedFlatIndex(cp.c.ctx, cp.c).search_device(tq, k, pipelined=True, allow=tw,
                                                                        allow_first_id=first_id)
    torch.cuda.synchronize()
    assert np.array_equal(ids.cpu().numpy().view(np.uint64), want_i)
    assert np.array_equal(bits(dists.cpu().numpy()), bits(want_d))
    assert np.array_equal(counts.cpu().numpy().astype(np.uint32), want_c)
    ws = torch.zeros(cp.c.lib.wvg_search_workspace_size(cp.c.handle, nq, k), dtype=torch.uint8, device=dev)
    oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
    od = torch.empty((nq, k), dtype=torch.float32, device=dev)
    oc = torch.empty(nq, dtype=torch.int32, device=dev)
    cp.c.search_device_pipelined(tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), ws.data_ptr(),
                                 ws.numel(), torch.cuda.current_stream().cuda_stream, tw.data_ptr(), stride, first_id)
    torch.cuda.synchronize()
    assert np.array_equal(oi.cpu().numpy().view(np.uint64), want_i) and np.array_equal(bits(od.cpu().numpy()), bits(want_d))
    with pytest.raises(ValueError):
        ShardedFlatIndex(cp.c.ctx, cp.c).search_device(tq, k, pipelined=False, allow=tw, allow_first_id=first_id)

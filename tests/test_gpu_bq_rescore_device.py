"""wvg_search_device_bq_rescore (bq_rescore_kernel, wvg_bq_rescore.hip) against numpy and the oracle, compared for
equality.  Reference per query: Hamming distances = popcounts of the XOR of the oracle's sign codes; candidates = the
top-R (R = max(rescore_limit, k)) by (distance, id) over the rows live in `bq` and allowed; exact distances = the
oracle's per-pair function in the context's order; result = the top-k by (distance bits, id) over the candidates live in
`f32`.  Every pair sits at id_base 640; ids deleted from f32 only: id % 7 == 3, bq only: id % 11 == 5, both: id % 13 == 0."""
import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import KIND_BQ, KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_L2, ORDER_AVX256, ORDER_AVX512
from weaviate_amd.device import (Context, Corpus, allow_window, search_bq_rescore, search_device_bq_rescore,
                                 search_device_bq_rescore_workspace_size)

from test_gpu_parity import bits, prep_query, stored_rows

pytestmark = pytest.mark.gpu
BASE = 640
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


class Pair:
    """A BQ and an F32 corpus over the same rows, with the oracle's view of them."""

    def __init__(self, cx, orc, metric, d, n, dup=False, f32_only=True):
        self.orc, self.metric, self.d, self.n = orc, metric, d, n
        rows = orc.synth_rows(100 + d, 0, n, d, 0)
        if dup:  # 16 distinct integer-valued rows: Hamming and exact distances tie heavily, the id decides
            rows = (orc.synth_rows(7, 0, 16, d, 1) - 128.0)[np.arange(n) % 16]
        self.ids = BASE + np.arange(n, dtype=np.uint64)
        self.rows = stored_rows(orc, metric, rows)
        self.codes = orc.bq_encode_rows(self.rows)
        i = np.arange(n)
        self.live_f = ~(((i % 7 == 3) & f32_only) | (i % 13 == 0))
        self.live_b = ~((i % 11 == 5) | (i % 13 == 0))
        self.bq = Corpus(cx, KIND_BQ, metric, d, n, id_base=BASE)
        self.f32 = Corpus(cx, KIND_F32, metric, d, n, id_base=BASE)
        for c, live in ((self.bq, self.live_b), (self.f32, self.live_f)):
            c.upsert(self.ids, rows)
            c.delete(self.ids[~live])

    def queries(self, nq, seed=0, dup=False):
        qs = self.orc.synth_rows(900 + seed, 0, nq, self.d, 1 if dup else 0) - (128.0 if dup else 0.0)
        return np.stack([prep_query(self.orc, self.metric, q) for q in qs]).astype(np.float32)

    def reference(self, qs, k, rescore_limit, masks=None, o512=False):
        R = max(rescore_limit, k)
        oi = np.full((len(qs), k), NONE, np.uint64)
        od = np.full((len(qs), k), np.inf, np.float32)
        oc = np.zeros(len(qs), np.uint32)
        for qi, q in enumerate(qs):
            x = self.codes ^ self.orc.bq_encode(q)[None, :]
            ham = np.unpackbits(np.ascontiguousarray(x).view(np.uint8), axis=1).sum(axis=1)
            ok = np.flatnonzero(self.live_b if masks is None else self.live_b & masks[qi])
            cand = ok[np.lexsort((ok, ham[ok]))[:R]]
            cand = cand[self.live_f[cand]]
            dist = (self.orc.dist_all_512 if o512 else self.orc.dist_all)(self.metric, q, self.rows[cand])
            ri, rd = self.orc.lex_topk(dist, self.ids[cand], k)
            oi[qi, :len(ri)], od[qi, :len(ri)], oc[qi] = ri, rd, len(ri)
        return oi, od, oc

    def destroy(self):
        self.bq.destroy()
        self.f32.destroy()


def run(bq, f32, qs, k, rescore_limit, words=None, first_id=0, ws_short=0, expect=_lib.WVG_OK, replays=()):
    """One call on sentinel-filled outputs and a zeroed workspace (an error must leave all of them as they were); with
    `replays` the call is captured instead and replayed once per query set written into the same buffer."""
    import torch
    dev, nq = torch.device("cuda:0"), len(qs)
    size = search_device_bq_rescore_workspace_size(bq, f32, nq, k, rescore_limit)
    ws = torch.zeros(max(size, 256) - ws_short, dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(np.ascontiguousarray(qs, dtype=np.float32)).to(dev)
    tw = torch.from_numpy(words.view(np.int64)).to(dev) if words is not None else None
    oi = torch.full((nq, k), 7, dtype=torch.int64, device=dev)
    od = torch.full((nq, k), -7.0, dtype=torch.float32, device=dev)
    oc = torch.full((nq,), 77, dtype=torch.int32, device=dev)
    untouched = lambda: bool((oi == 7).all()) and bool((od == -7.0).all()) and bool((oc == 77).all())
    result = lambda: (oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32))

    def call():
        try:
            search_device_bq_rescore(bq, f32, tq.data_ptr(), nq, k, rescore_limit, oi.data_ptr(), od.data_ptr(),
                                     oc.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream,
                                     tw.data_ptr() if tw is not None else 0, words.shape[1] if tw is not None else 0, first_id)
        except _lib.WvgError as e:
            return e.code
        return _lib.WVG_OK

    if replays:
        g, outs = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(g):
            assert call() == _lib.WVG_OK
        torch.cuda.synchronize()
        assert untouched()  # captured, not run
        for q in replays:
            tq.copy_(torch.from_numpy(q))
            g.replay()
            torch.cuda.synchronize()
            outs.append(result())
        return outs
    rc = call()
    torch.cuda.synchronize()
    assert rc == expect
    assert int(ws[:256].sum()) == 0  # the status block is never touched
    assert rc == _lib.WVG_OK or (int(ws.sum()) == 0 and untouched())
    return result()


def same(got, want):
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))  # padding included: ids UINT64_MAX, dists +inf


@pytest.fixture(scope="module")
def pairs(ctx, orc):
    made = {}
    yield lambda *key: made.get(key) or made.setdefault(key, Pair(ctx, orc, *key))
    for p in made.values():
        p.destroy()


# d: 8 = one leftover 8-block, 36 = a 32-block and the scalar tail, 128 / 1536 = whole blocks; nq: 1 / 5 / 9 = the single-
# query route, one and two passes of the 8-query scan; (10, 300): the select route; (10, 8): R < k; n = 209: R above the live rows
@pytest.mark.parametrize("metric,d,n,nq,k,rl,dup", [
    (METRIC_L2, 8, 209, 1, 1, 1, False),
    (METRIC_L2, 36, 209, 5, 10, 200, False),
    (METRIC_L2, 36, 209, 5, 10, 200, True),
    (METRIC_DOT, 128, 5003, 9, 10, 200, False),
    (METRIC_COSINE, 1536, 209, 5, 256, 256, False),
    (METRIC_L2, 1536, 5003, 9, 10, 300, False),
    (METRIC_COSINE, 36, 5003, 1, 10, 8, False),
    (METRIC_DOT, 8, 209, 5, 10, 300, False),
    (METRIC_L2, 128, 5003, 9, 256, 256, False),
    (METRIC_DOT, 1536, 5003, 1, 100, 200, False),
])
def test_matches_reference(pairs, metric, d, n, nq, k, rl, dup):
    p = pairs(metric, d, n, dup)
    qs = p.queries(nq, dup=dup)
    want = p.reference(qs, k, rl)
    same(run(p.bq, p.f32, qs, k, rl), want)


def test_allow_windows(pairs):
    """Per-query windows that begin at docID 0, before id_base: 10 % lists, an all-zero row, the whole corpus."""
    p = pairs(METRIC_L2, 128, 5003)
    nq, stride = 9, (BASE + 4800) // 64  # the window ends before the last rows
    rng = np.random.default_rng(5)
    masks = [rng.random(p.n) < 0.1 for _ in range(nq)]
    masks[2] = np.zeros(p.n, bool)
    masks[4] = np.ones(p.n, bool)
    words = allow_window([p.ids[m] for m in masks], 0, stride)
    words[:, :BASE // 64] = NONE  # bits that name no row are ignored
    inwin = p.ids < np.uint64(64 * stride)
    qs = p.queries(nq, 1)
    for nqq, k, rl in ((nq, 10, 200), (1, 256, 256)):
        got = run(p.bq, p.f32, qs[:nqq], k, rl, words[:nqq], 0)
        same(got, p.reference(qs[:nqq], k, rl, [m & inwin for m in masks]))
    run(p.bq, p.f32, qs, 10, 300, words, 0, expect=_lib.WVG_ERR_UNSUPPORTED)  # the select route has no filter
    run(p.bq, p.f32, qs, 10, 200, words, 32, expect=_lib.WVG_ERR_INVALID)


def test_host_call_and_avx512_order(orc):
    """A heap_replay = 0 context: wvg_search_bq_rescore returns the same bits; then the AVX-512 order (d = 300: two
    128-blocks, a 32-block, an 8-block, a tail of 4).  No row is deleted from f32 alone: that host route scores its stale data."""
    cx = Context(0, heap_replay=0)
    p = Pair(cx, orc, METRIC_L2, 300, 1009, f32_only=False)
    try:
        qs = p.queries(5, 2)
        for order in (ORDER_AVX256, ORDER_AVX512):
            cx.set_distance_order(order)
            for k, rl in ((10, 200), (10, 300)):
                got = run(p.bq, p.f32, qs, k, rl)
                same(got, p.reference(qs, k, rl, o512=order == ORDER_AVX512))
                same(got, search_bq_rescore(p.bq, p.f32, qs, k, rl))
    finally:
        p.destroy()
        cx.close()


def test_captured_call_replays(pairs):
    p = pairs(METRIC_DOT, 128, 5003)
    sets = [p.queries(9, s) for s in (3, 4, 5)]  # at capture time, then the two replays
    for qs, got in zip(sets[1:], run(p.bq, p.f32, sets[0], 10, 200, replays=sets[1:])):
        same(got, p.reference(qs, 10, 200))


def test_errors_launch_nothing(pairs):
    p = pairs(METRIC_L2, 128, 5003)
    qs = p.queries(5)
    run(p.bq, pairs(METRIC_L2, 36, 209).f32, qs, 10, 200, expect=_lib.WVG_ERR_INVALID)  # dim differs
    run(p.bq, pairs(METRIC_DOT, 128, 5003).f32, qs, 10, 200, expect=_lib.WVG_ERR_INVALID)  # metric differs
    run(p.f32, p.bq, qs, 10, 200, expect=_lib.WVG_ERR_INVALID)  # kinds swapped
    run(p.bq, p.f32, qs, 257, 300, expect=_lib.WVG_ERR_UNSUPPORTED)
    for rl in (200, 300):
        run(p.bq, p.f32, qs, 10, rl, ws_short=1, expect=_lib.WVG_ERR_INVALID)

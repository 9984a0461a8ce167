"""K3c-L2 -- the bf16 MFMA screen of batched l2-squared searches with a per-row
error bound + the exact fp32 rescore of every row the bound cannot rule out
(weaviate_amd/csrc/wvg_screen.hip, screen_l2_kernel) -- returns exactly what the
exact path returns: the same ids, the same distance bits, the same counts
(Q flat.searchByVector calls, V/flat/index.go:319; SingleDist = l2_256,
D/l2.go, D/c/l2_avx256_amd64.c).  The exact path here is a context with
wvg_options.batch_screen = 0 -- for l2-squared the co-scheduled K1 / K1Q scans,
pinned to the oracle in test_gpu_parity; two queries per case also go against
the oracle directly (not the NaN / inf case: the oracle's heap is not defined on
NaN distances; tests/test_gpu_k1_special_values.py pins that order for K1).  Corpus.batch_plan shows which route a batch takes."""
import numpy as np
import pytest

from weaviate_amd._lib import KIND_F32, METRIC_COSINE, METRIC_L2
from weaviate_amd.device import Context, Corpus, Multi, MultiCorpus, allow_bitmap

from test_gpu_parity import ORC_METRIC, bits, check_topk
from test_gpu_screen import _pair, _same, bf16_ctx, exact_ctx  # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu

DIMS = [32, 96, 128, 768, 1536]


def _l2_pair(ctx, exact_ctx, d, rows, ids=None):
    a, b = _pair(ctx, exact_ctx, METRIC_L2, d, rows, ids)
    assert a.batch_plan(32, 10)["screen"] == 1 and b.batch_plan(32, 10)["screen"] == 0
    return a, b


def _oracle(orc, got, qs, rows, k, qis, valid=None, ids=None):
    """Queries qis of a search result against the oracle's lexicographic top-k over rows."""
    ids = np.arange(len(rows), dtype=np.uint64) if ids is None else ids
    valid = np.ones(len(rows), np.uint8) if valid is None else valid
    for qi in qis:
        all_d = orc.dist_all(ORC_METRIC[METRIC_L2], qs[qi], rows)
        check_topk(orc, got[0][qi], got[1][qi], got[2][qi], all_d, ids, k, valid)


def test_route(ctx, bf16_ctx, exact_ctx, orc):
    """The plan query: K3c-L2 exactly where K3c would take a dot batch of the same shape."""
    made = []

    def corpus(cx, metric, d):
        c = Corpus(cx, KIND_F32, metric, d, 256)
        c.upsert(np.arange(200, dtype=np.uint64), orc.synth_rows(2000 + d, 0, 200, d, 0))
        made.append(c)
        return c

    try:
        for cx in (ctx, bf16_ctx):
            for d in DIMS:
                c = corpus(cx, METRIC_L2, d)
                want = {"matrix": 1, "screen": 1, "shadow_bytes_per_row": 2 * d + 4}
                assert c.batch_plan(32, 10) == want, d
                assert c.batch_plan(32, 10, allow=True) == want
                assert c.batch_plan(1024, 16) == want
                for nq, k in [(31, 10), (32, 17)]:
                    assert c.batch_plan(nq, k)["screen"] == 0, (d, nq, k)
                    assert c.batch_plan(nq, k) == {"matrix": 0, "screen": 0, "shadow_bytes_per_row": 0}
            assert corpus(cx, METRIC_L2, 100).batch_plan(32, 10)["screen"] == 0
        assert corpus(exact_ctx, METRIC_L2, 128).batch_plan(32, 10)["screen"] == 0
        with Context(0, mfma_min_queries=0) as c0:
            c = Corpus(c0, KIND_F32, METRIC_L2, 128, 256)
            c.upsert(np.arange(200, dtype=np.uint64), orc.synth_rows(2128, 0, 200, 128, 0))
            assert c.batch_plan(32, 10)["screen"] == 0
            c.destroy()
        c = corpus(ctx, METRIC_L2, 768)
        ctx.set_distance_order(1)  # the AVX-512 order
        try:
            assert c.batch_plan(32, 10)["screen"] == 0
        finally:
            ctx.set_distance_order(0)
        assert c.batch_plan(32, 10)["screen"] == 1
        # dot / cosine keep their routes: int8 at d = 768 on the default context, bf16 on batch_screen = 1
        assert corpus(ctx, METRIC_COSINE, 768).batch_plan(32, 10) == {
            "matrix": 1, "screen": 2, "shadow_bytes_per_row": 768 + 8}
        assert corpus(bf16_ctx, METRIC_COSINE, 768).batch_plan(32, 10) == {
            "matrix": 1, "screen": 1, "shadow_bytes_per_row": 2 * 768 + 4}
        assert corpus(exact_ctx, METRIC_COSINE, 768).batch_plan(32, 10) == {
            "matrix": 1, "screen": 0, "shadow_bytes_per_row": 0}
    finally:
        for c in made:
            c.destroy()


@pytest.mark.parametrize("d", [128, 256, 96, 768, 1536, 32])
def test_screen_equals_exact(ctx, exact_ctx, orc, d):
    n = 30_000 + 77
    rows = orc.synth_rows(1000 + d, 0, n, d, 0)
    qs = orc.synth_rows(1001 + d, 0, 300, d, 0)
    a, b = _l2_pair(ctx, exact_ctx, d, rows)
    dead = np.array([0, 5, 64, 255, 256, 20_000, n - 1], np.uint64)
    a.delete(dead)
    b.delete(dead)
    try:
        for nq, k in [(32, 10), (300, 10), (40, 1), (129, 16), (64, 7)]:
            _same(a.search(qs[:nq], k), b.search(qs[:nq], k))
        ids, dists, counts = a.search(qs[:32], 10)
        valid = np.ones(n, np.uint8)
        valid[dead.astype(np.int64)] = 0
        for qi in (0, 31):
            all_d = orc.dist_all(ORC_METRIC[METRIC_L2], qs[qi], rows)
            check_topk(orc, ids[qi], dists[qi], counts[qi], all_d, np.arange(n, dtype=np.uint64), 10, valid)
    finally:
        a.destroy()
        b.destroy()


def test_ties_overflow_rescan(ctx, exact_ctx, orc):
    """3000 copies of one row and queries equal to it: every copy is at distance 0, the range
    lists fill below tau, the queries are flagged and rescanned exactly -- still the
    lexicographic (distance, docID) top-k."""
    n, d = 20_000, 256
    rows = orc.synth_rows(1100, 0, n, d, 0)
    rows[1000:4000] = rows[1000]
    qs = orc.synth_rows(1101, 0, 40, d, 0)
    qs[::3] = rows[1000]
    a, b = _l2_pair(ctx, exact_ctx, d, rows)
    try:
        for k in (1, 10, 16):
            got = a.search(qs, k)
            _same(got, b.search(qs, k))
            assert np.all(got[1][::3] == 0) and np.array_equal(got[0][0], np.arange(1000, 1000 + k))
        all_d = orc.dist_all(ORC_METRIC[METRIC_L2], qs[0], rows)
        ids, dists, counts = a.search(qs, 10)
        check_topk(orc, ids[0], dists[0], counts[0], all_d, np.arange(n, dtype=np.uint64), 10, np.ones(n, np.uint8))
    finally:
        a.destroy()
        b.destroy()


def test_integer_grid(ctx, exact_ctx, orc):
    """floor(3 x) rows and queries: heavy exact ties at non-zero distances."""
    n, d = 20_000, 128
    rows = np.floor(orc.synth_rows(1150, 0, n, d, 0) * 3).astype(np.float32)
    qs = np.floor(orc.synth_rows(1151, 0, 64, d, 0) * 3).astype(np.float32)
    a, b = _l2_pair(ctx, exact_ctx, d, rows)
    try:
        for k in (1, 10, 16):
            _same(a.search(qs, k), b.search(qs, k))
        ids, dists, counts = a.search(qs, 10)
        for qi in (0, 63):
            all_d = orc.dist_all(ORC_METRIC[METRIC_L2], qs[qi], rows)
            check_topk(orc, ids[qi], dists[qi], counts[qi], all_d, np.arange(n, dtype=np.uint64), 10,
                       np.ones(n, np.uint8))
    finally:
        a.destroy()
        b.destroy()


@pytest.mark.parametrize("d", [128, 768])
def test_nonfinite_and_zero(ctx, exact_ctx, orc, d):
    """Rows and queries with inf / NaN / zero / 1e30 / 1e-30 components: their bound is open
    (always rescored) or their distance exact; NaN sorts last."""
    n = 8000
    rows = np.floor(orc.synth_rows(1200, 0, n, d, 0) * 3).astype(np.float32)
    rows[10, 3] = np.nan
    rows[11, 4] = np.inf
    rows[12, 5] = -np.inf
    rows[[13, 14]] = 0.0
    rows[15] = 1e30
    qs = np.floor(orc.synth_rows(1201, 0, 48, d, 0) * 3).astype(np.float32)
    qs[1] = 0.0
    qs[2, 7] = np.inf
    qs[3] = 1e-30
    a, b = _l2_pair(ctx, exact_ctx, d, rows)
    try:
        for k in (1, 10):
            _same(a.search(qs, k), b.search(qs, k))
    finally:
        a.destroy()
        b.destroy()


@pytest.mark.parametrize("scale", [1e15, 1e-20])
def test_scaled_magnitudes(ctx, exact_ctx, orc, scale):
    """Rows and queries scaled to 1e15 (squares near 1e33) and 1e-20 (squares below the normal
    range), and the large finite magnitudes on both sides of the fast check's limits."""
    n, d = 6000, 768
    rows = orc.synth_rows(1250, 0, n, d, 0)
    qs = orc.synth_rows(1251, 0, 40, d, 0)
    sc = (rows * np.float32(scale)).astype(np.float32), (qs * np.float32(scale)).astype(np.float32)
    mixed_rows, mixed_qs = rows.copy(), qs.copy()
    mixed_rows[100:110] *= np.float32(1e10)     # norm ~1e11: fast-eligible
    mixed_rows[200:210] *= np.float32(1e19)     # norm ~1e20 > 2^60: forced exact
    mixed_rows[300] = np.float32(3e38)          # bf16 rounds it to inf
    mixed_qs[1] *= np.float32(1e10)
    mixed_qs[2] *= np.float32(1e17)             # norm > 2^56: no fast rejection
    mixed_qs[3] *= np.float32(1e25)
    for rr, qq in (sc, (mixed_rows, mixed_qs)):
        a, b = _l2_pair(ctx, exact_ctx, d, rr)
        try:
            for k in (1, 10, 16):
                got = a.search(qq, k)
                _same(got, b.search(qq, k))
            _oracle(orc, got, qq, rr, 16, (0, 39))
        finally:
            a.destroy()
            b.destroy()


@pytest.mark.parametrize("d", [128, 768])
def test_shared_allow_list(ctx, exact_ctx, orc, d):
    n = 9000 + 5
    rows = orc.synth_rows(1300 + d, 0, n, d, 0)
    qs = orc.synth_rows(1301 + d, 0, 64, d, 0)
    a, b = _l2_pair(ctx, exact_ctx, d, rows)
    try:
        for allowed in (np.arange(1, n, 3, dtype=np.uint64), np.array([7, 4000, 8999], np.uint64)):
            al = allow_bitmap(allowed)
            got = a.search(qs, 10, al)
            _same(got, b.search(qs, 10, al))
            valid = np.zeros(n, np.uint8)
            valid[allowed.astype(np.int64)] = 1
            _oracle(orc, got, qs, rows, 10, (0, 63), valid)
        assert np.all(got[2] == 3) and np.array_equal(np.sort(got[0][0][:3]), [7, 4000, 8999])
    finally:
        a.destroy()
        b.destroy()


def test_shadow_follows_writes(ctx, exact_ctx, orc):
    """The shadow is rebuilt over the tiles written since the last screened search and dropped on growth."""
    n, d = 12_000, 256
    rows = orc.synth_rows(1400, 0, n, d, 0)
    qs = orc.synth_rows(1401, 0, 40, d, 0)
    a = Corpus(ctx, KIND_F32, METRIC_L2, d, n + 100)
    b = Corpus(exact_ctx, KIND_F32, METRIC_L2, d, n + 100)
    try:
        for x in (a, b):
            x.upsert(np.arange(n, dtype=np.uint64), rows)
        assert a.batch_plan(40, 10)["screen"] == 1
        _same(a.search(qs, 10), b.search(qs, 10))  # builds the shadow
        # overwrite live rows and add new ones past the last: the queries themselves, distance 0
        ids = np.array([7, 4000, 11_999, n + 3, n + 99], np.uint64)
        dead = np.array([7, 100, n + 99], np.uint64)
        for x in (a, b):
            x.upsert(ids, qs[:5])
            x.delete(dead)
        got = a.search(qs, 10)
        _same(got, b.search(qs, 10))
        assert got[0][1][0] == 4000 and got[0][2][0] == 11_999 and got[0][3][0] == n + 3
        assert np.all(got[1][1:4, 0] == 0) and got[0][0][0] != 7 and got[0][4][0] != n + 99
        more = orc.synth_rows(1402, 0, 5000, d, 0)
        more[:3] = qs[5:8]
        mids = np.arange(15_000, 20_000, dtype=np.uint64)
        for x in (a, b):
            x.reserve(20_000)  # realloc: the shadow is rebuilt from scratch
            x.upsert(mids, more)
        got = a.search(qs, 10)
        _same(got, b.search(qs, 10))
        assert got[0][5][0] == 15_000 and got[0][7][0] == 15_002
        stored = np.zeros((20_000, d), np.float32)
        stored[:n] = rows
        stored[ids.astype(np.int64)] = qs[:5]
        stored[mids.astype(np.int64)] = more
        valid = np.zeros(20_000, np.uint8)
        valid[:n] = 1
        valid[ids.astype(np.int64)] = 1
        valid[mids.astype(np.int64)] = 1
        valid[dead.astype(np.int64)] = 0
        _oracle(orc, got, qs, stored, 10, (0, 39), valid)
    finally:
        a.destroy()
        b.destroy()


def test_device_path_and_graph_replay(ctx, exact_ctx, orc):
    """wvg_search_device takes K3c-L2 for a batch of 64 and returns the host call's results;
    captured in a graph after one warm batch (the shadow exists), it replays to the same bits."""
    import torch

    from weaviate_amd import _lib

    n, d, nq, k = 25_000, 128, 64, 10
    rows = orc.synth_rows(1500, 0, n, d, 0)
    qs = orc.synth_rows(1501, 0, nq, d, 0)
    a, b = _l2_pair(ctx, exact_ctx, d, rows)
    try:
        want = b.search(qs, k)
        _same(a.search(qs, k), want)
        _oracle(orc, want, qs, rows, k, (0, 63))
        lib = ctx.lib
        dev = torch.device("cuda:0")
        ws = torch.zeros(lib.wvg_search_workspace_size(a.handle, nq, k), dtype=torch.uint8, device=dev)
        tq = torch.from_numpy(qs).to(dev)
        oi = torch.zeros((nq, k), dtype=torch.int64, device=dev)
        od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
        oc = torch.zeros(nq, dtype=torch.int32, device=dev)

        def call():
            _lib.check(lib.wvg_search_device(a.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                             oc.data_ptr(), ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream().cuda_stream))

        def result():
            torch.cuda.synchronize()
            return oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)

        call()  # the warm batch
        _same(result(), want)
        for t in (oi, od, oc):
            t.zero_()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        torch.cuda.synchronize()
        assert int(oi.abs().sum()) == 0 and int(oc.sum()) == 0  # captured, not run
        g.replay()
        _same(result(), want)
        g.replay()
        _same(result(), want)
    finally:
        a.destroy()
        b.destroy()


def test_slabs(ctx, exact_ctx, orc):
    """One Multi([0, 0]) search of 64 l2-squared queries equals the single corpus."""
    n, d, k = 40_000, 128, 10
    rows = orc.synth_rows(1600, 0, n, d, 0)
    qs = orc.synth_rows(1601, 0, 64, d, 0)
    ids = np.arange(n, dtype=np.uint64)
    ref = Corpus(exact_ctx, KIND_F32, METRIC_L2, d, n)
    ref.upsert(ids, rows)
    try:
        with Multi([0, 0]) as m:
            mc = MultiCorpus(m, KIND_F32, METRIC_L2, d, n)
            try:
                mc.upsert(ids, rows)
                got = mc.search(qs, k)
                _same(got, ref.search(qs, k))
                _oracle(orc, got, qs, rows, k, (0, 63))
            finally:
                mc.destroy()
    finally:
        ref.destroy()

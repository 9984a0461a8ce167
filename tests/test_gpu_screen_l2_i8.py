"""K3i-L2 -- the int8 MFMA screen of batched l2-squared searches in a batch_screen = 3 context
(wvg_screen.hip: screen_i8_l2_kernel at d = 512 / 768, screen_ar_l2_kernel at d = 1024) + the exact
rescore -- returns the oracle's l2_256 top-k (ids, counts, padding, distance bits) and exactly what a
batch_screen = 0 context returns.  Rows not a multiple of 64, one 256-row block per row range."""
import numpy as np
import pytest

from weaviate_amd._lib import KIND_F32, METRIC_L2
from weaviate_amd.device import Context, Corpus, allow_bitmap

from test_gpu_screen import _same, exact_ctx  # noqa: F401  (module-scoped fixture)
from test_gpu_screen_l2 import _oracle

pytestmark = pytest.mark.gpu

N, DIMS, KS, NQS = 5037, [512, 768, 1024], [1, 10, 16], [2, 33, 129]
PLAN = lambda d: {"matrix": 1, "screen": 2, "shadow_bytes_per_row": d + 8}  # noqa: E731
BF16 = lambda d: {"matrix": 1, "screen": 1, "shadow_bytes_per_row": 2 * d + 4}  # noqa: E731


@pytest.fixture(scope="module")
def i8_ctx(ctx):
    c = Context(0, batch_screen=3, mfma_min_queries=2)
    yield c
    c.close()


def _corpus(cx, d, rows, cap=None):
    c = Corpus(cx, KIND_F32, METRIC_L2, d, cap or len(rows))
    c.upsert(np.arange(len(rows), dtype=np.uint64), rows)
    return c


@pytest.fixture(scope="module")
def cases(i8_ctx, exact_ctx, orc):
    """Per d: (screened corpus, exact corpus, rows, valid, queries) for the ordinary rows [0] and the
    adversarial ones [1]; built once, the shadow of [1] from the rows before the late upserts."""
    out, made = {}, []
    for d in DIMS:
        rows = orc.synth_rows(3000 + d, 0, N, d, 0)
        qs = orc.synth_rows(3001 + d, 0, 129, d, 0)
        dead = np.array([0, 64, 255, 256, N - 1], np.uint64)
        valid = np.ones(N, np.uint8)
        valid[dead.astype(np.int64)] = 0
        pair = [_corpus(i8_ctx, d, rows), _corpus(exact_ctx, d, rows)]
        for c in pair:
            c.delete(dead)
        adv, aq = rows.copy(), qs.copy()
        adv[2000:2010] *= np.float32(8.0)           # large norms: their copies cancel to 0 / a few ulps
        adv[1030:1070] = adv[1030]                  # 40 identical rows inside one row range: its list overflows
        adv[3000], adv[3001, 5], adv[3002, 7] = 0.0, np.nan, np.inf
        late = (adv[4000:4008] * np.float32(50.0)).astype(np.float32)  # above the corpus scale: codes clamp
        aq[0], aq[1] = adv[1030], late[0]
        aq[2], aq[3] = adv[2000], np.nextafter(adv[2001], np.float32(np.inf))
        aq[4], aq[5] = 0.0, aq[5] * np.float32(2.0**58)  # (norm above 2^56, distances still finite)
        apair = [_corpus(i8_ctx, d, adv), _corpus(exact_ctx, d, adv)]
        assert apair[0].batch_plan(33, 10) == PLAN(d)
        apair[0].search(aq[:33], 10)                # the first build: the scale comes from the rows so far
        adv[4000:4008] = late
        for c in apair:
            c.upsert(np.arange(4000, 4008, dtype=np.uint64), late)
        avalid = np.ones(N, np.uint8)
        avalid[[3001, 3002]] = 0                    # NaN / inf distances sort last: never in a top-16
        out[d] = ((*pair, rows, valid, qs), (*apair, adv, avalid, aq))
        made += pair + apair
    yield out
    for c in made:
        c.destroy()


def test_route_and_plan(ctx, i8_ctx, orc):
    for d in DIMS:
        rows = orc.synth_rows(3100 + d, 0, 200, d, 0)
        a, b = _corpus(i8_ctx, d, rows), _corpus(ctx, d, rows)
        try:
            assert a.batch_plan(2, 10) == a.batch_plan(1024, 16) == PLAN(d)
            assert b.batch_plan(32, 10) == b.batch_plan(1024, 16) == BF16(d)
            assert a.batch_plan(33, 17)["screen"] == 0
            i8_ctx.set_distance_order(1)  # the AVX-512 order
            try:
                assert a.batch_plan(33, 10)["screen"] == 0
            finally:
                i8_ctx.set_distance_order(0)
        finally:
            a.destroy()
            b.destroy()


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("family", [0, 1])
def test_parity(cases, orc, family, d, k, nq):
    a, b, rows, valid, qs = cases[d][family]
    assert a.batch_plan(nq, k) == PLAN(d)
    got = a.search(qs[:nq], k)
    _same(got, b.search(qs[:nq], k))
    _oracle(orc, got, qs, rows, k, range(min(nq, 6)), valid)
    al = allow_bitmap(np.arange(1, N, 3, dtype=np.uint64))
    got = a.search(qs[:nq], k, al)
    _same(got, b.search(qs[:nq], k, al))
    av = valid.copy()
    av[np.arange(N) % 3 != 1] = 0
    _oracle(orc, got, qs, rows, k, range(min(nq, 2)), av)


def test_shadow_life_cycle(i8_ctx, exact_ctx, orc):
    d, n = 768, 3000
    rows = orc.synth_rows(3200, 0, n, d, 0)
    qs = orc.synth_rows(3201, 0, 33, d, 0)
    a, b = _corpus(i8_ctx, d, rows, 4000), _corpus(exact_ctx, d, rows, 4000)
    z, zb = _corpus(i8_ctx, d, np.zeros((300, d), np.float32)), _corpus(exact_ctx, d, np.zeros((300, d), np.float32))
    try:
        _same(a.search(qs, 10), b.search(qs, 10))
        for c in (a, b):
            c.upsert(np.array([7, n + 5], np.uint64), qs[:2])  # the dirty rebuild finds them
        got = a.search(qs, 10)
        _same(got, b.search(qs, 10))
        assert got[0][0][0] == 7 and got[0][1][0] == n + 5 and np.all(got[1][:2, 0] == 0)
        for c in (a, b):
            c.reserve(9000)  # drops the shadow
            c.upsert(np.array([8500], np.uint64), qs[2:3])
        got = a.search(qs, 10)
        _same(got, b.search(qs, 10))
        assert got[0][2][0] == 8500 and a.batch_plan(33, 10) == PLAN(d)
        assert z.batch_plan(33, 10) == PLAN(d)  # an all-zero corpus: the first build falls back to bf16
        _same(z.search(qs, 10), zb.search(qs, 10))
        assert z.batch_plan(33, 10) == BF16(d)
    finally:
        for c in (a, b, z, zb):
            c.destroy()


def test_graph_replay(cases, i8_ctx):
    import torch

    from weaviate_amd import _lib

    a, b, _, _, qs = cases[768][0]
    nq, k, lib, dev = 33, 10, i8_ctx.lib, torch.device("cuda:0")
    want = b.search(qs[:nq], k)
    ws = torch.zeros(lib.wvg_search_workspace_size(a.handle, nq, k), dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(qs[:nq].copy()).to(dev)
    oi = torch.zeros((nq, k), dtype=torch.int64, device=dev)
    od = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    oc = torch.zeros(nq, dtype=torch.int32, device=dev)

    def call():
        _lib.check(lib.wvg_search_device(a.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                         ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))

    def result():
        torch.cuda.synchronize()
        return oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)

    call()  # the warm batch
    _same(result(), want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(2):
        oi.zero_()
        g.replay()
        _same(result(), want)

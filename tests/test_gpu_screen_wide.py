"""K3c-W (wvg_screen.hip: the bf16 screen at 16 < k <= 256 in a batch_screen = 4 context, survivor pools in
HBM) returns the ids, distance bits and counts of the exact path (a batch_screen = 0 context); two queries
per case also go against the oracle's exact top-k (not the NaN / inf case: its heap is undefined on NaN)."""
import functools

import numpy as np
import pytest

from weaviate_amd._lib import KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_L2
from weaviate_amd.device import Context, Corpus, allow_bitmap

from test_gpu_parity import ORC_METRIC, check_topk, prep_query, stored_rows
from test_gpu_screen import _pair, _same, exact_ctx  # noqa: F401  (module-scoped fixture)

pytestmark = pytest.mark.gpu

CASES = {"ragged": 2037, "masked": 2037, "nonfinite": 2037, "compaction": 256 * 4 * 256 + 37, "ties": 3000, "few": 50}


@pytest.fixture(scope="module")
def wide_ctx(ctx):
    c = Context(0, batch_screen=4, mfma_min_queries=2)
    yield c
    c.close()


@functools.lru_cache(maxsize=2)
def _case(orc, case, metric, d):
    """(rows, queries) of a case, shared by its k (read only).  compaction: a query block gets a row range per
    CU, so 256 ranges of four row blocks make a pool pass P - 256 inside a range (k = 256: P keys after three)."""
    rows = orc.synth_rows(7000 + d, 0, CASES[case], d, 0)
    qs = orc.synth_rows(7001 + d, 0, 33, d, 0)
    if case == "compaction":
        # queries around one point, rows stored farthest first: every row block tightens the bound
        qs = (qs[0] + np.float32(0.05) * qs).astype(np.float32)
        far = orc.dist_all(ORC_METRIC[metric], prep_query(orc, metric, qs.mean(0)), stored_rows(orc, metric, rows))
        rows = rows[np.argsort(-far, kind="stable")]
    if case == "ties":
        rows[700:2200] = rows[700]
        qs[::3] = rows[700]
    if case == "nonfinite":
        rows[10, 3] = np.nan
        rows[300, 4] = np.inf
    return rows, qs


@pytest.mark.parametrize("k", [17, 100, 256])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("d", [32, 96])
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT, METRIC_COSINE])
def test_wide_equals_exact(wide_ctx, exact_ctx, orc, metric, d, k, case):
    rows, qs = _case(orc, case, metric, d)
    n = len(rows)
    a, b = _pair(wide_ctx, exact_ctx, metric, d, rows)
    try:
        assert a.batch_plan(len(qs), k)["screen"] == 1 and b.batch_plan(len(qs), k)["screen"] == 0
        valid, al = np.ones(n, np.uint8), None
        if case == "masked":
            dead = np.array([0, 5, 64, 255, 256, 1999, n - 1], np.uint64)
            a.delete(dead)
            b.delete(dead)
            al = allow_bitmap(np.arange(1, n, 3, dtype=np.uint64))
            valid[:] = 0
            valid[1::3] = 1
            valid[dead.astype(np.int64)] = 0
        got = a.search(qs, k, al)
        _same(got, b.search(qs, k, al))
        assert np.all(got[2] == min(k, int(valid.sum())))
        if case != "nonfinite":
            srows = stored_rows(orc, metric, rows)
            for qi in (0, len(qs) - 1):
                all_d = orc.dist_all(ORC_METRIC[metric], prep_query(orc, metric, qs[qi]), srows)
                check_topk(orc, got[0][qi], got[1][qi], got[2][qi], all_d, np.arange(n, dtype=np.uint64), k, valid)
    finally:
        a.destroy()
        b.destroy()


@pytest.mark.parametrize("metric,d", [(METRIC_L2, 128), (METRIC_L2, 96), (METRIC_DOT, 768), (METRIC_COSINE, 32)])
def test_plans(wide_ctx, orc, metric, d):
    """Wide batches screen on the bf16 shadow; k <= 16 is batch_screen = 2's plan; k > 256 stays off the screen."""
    with Context(0, batch_screen=2, mfma_min_queries=2) as two:
        c, c2 = (Corpus(cx, KIND_F32, metric, d, 256) for cx in (wide_ctx, two))
        try:
            for x in (c, c2):
                x.upsert(np.arange(200, dtype=np.uint64), orc.synth_rows(7100 + d, 0, 200, d, 0))
            bf16 = 64 * ((d + 31) // 32 if metric == METRIC_L2 else (d + 63) // 64 * 2) + 4
            want = {"matrix": 1, "screen": 1, "shadow_bytes_per_row": bf16}
            assert c.batch_plan(32, 17) == want and c.batch_plan(1024, 256) == want
            assert c.batch_plan(32, 257)["screen"] == 0 and c2.batch_plan(32, 17)["screen"] == 0
            assert c.batch_plan(32, 16) == want  # bf16 at every k: the int8 screens are off under 4
            assert metric != METRIC_L2 or c.batch_plan(32, 16) == c2.batch_plan(32, 16)
        finally:
            c.destroy()
            c2.destroy()


def test_device_graph_replay(wide_ctx, exact_ctx, orc):
    """wvg_search_device takes K3c-W; captured after one warm batch it replays three times to the same bits
    (the counts, flags and bounds are reset by kernels inside the capture)."""
    import torch
    from weaviate_amd import _lib
    d, nq, k = 96, 33, 100
    rows, qs = _case(orc, "compaction", METRIC_L2, d)
    a, b = _pair(wide_ctx, exact_ctx, METRIC_L2, d, rows)
    try:
        want = b.search(qs, k)
        lib, dev = wide_ctx.lib, torch.device("cuda:0")
        ws = torch.zeros(lib.wvg_search_workspace_size(a.handle, nq, k), dtype=torch.uint8, device=dev)
        tq = torch.from_numpy(qs).to(dev)
        oi, od, oc = (torch.zeros(sh, dtype=t, device=dev)
                      for sh, t in (((nq, k), torch.int64), ((nq, k), torch.float32), (nq, torch.int32)))

        def call():
            _lib.check(lib.wvg_search_device(a.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(),
                                             oc.data_ptr(), ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream().cuda_stream))

        call()  # the warm batch builds the shadow
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        for _ in range(4):  # the warm batch's result, then three replays
            torch.cuda.synchronize()
            _same((oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)), want)
            for t in (oi, od, oc):
                t.zero_()
            ws.fill_(0xA5)  # whatever an earlier replay left behind
            g.replay()
    finally:
        a.destroy()
        b.destroy()

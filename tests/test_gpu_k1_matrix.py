"""K1 (fp32 flat scan) specialization matrix: every reachable instantiation of
the four kernel families against the oracle, bit-exact.

The kernels are templates over <METRIC, D, E, ...>:
  METRIC  0 L2, 1 DOT (cosine runs the DOT kernel with the 1 - x wrap:
          with_metric, wvg_internal.hpp:211-219), 3 MANHATTAN, 4 HAMMING
  D       128 / 768 / 1536 fixed-length kernels, 0 the generic-length one
          (the `switch (a.dim)` of launch_f32_e / launch_stream_e,
          wvg_scan.hip:841-868)
  E       64-key registers per wave list: 1 for k <= 64, 2 for k <= 128, 4
          above (launch_f32_m / launch_stream_m, wvg_scan.hip:872-891)

Routes of one (metric, d) case and the instantiation each is meant to reach
(D = d for d in K1["fixed_d"], else 0; M = the metric's kernel; E from k):

  route  call                                   d          metric        kernel
  R1     c.search(q, k), one query              any        any           scan_f32_stream_kernel<M, D, E>
         (wvg_search -> search_coalesced -> search_batch; inlaunch_single,
         wvg_search.hip:342-345, 391-431; the query rides in
         the kernel arguments up to STREAM_QIN_FLOATS = 256 floats and is
         staged above, wvg_search.hip:908-922)
  R2     c.search(qs, k), nq = 5                128, 768   L2/DOT/COS    scan_f32_mq_kernel<M, D, E, 4, false>
         (plan_search sets mq = k1_mq = 4, wvg_search.hip:257-270;             two workgroup query groups: 4 + 1
         launch_f32_e, wvg_scan.hip:819-837)
  R2     the same call                          128, 768   MANH/HAMM     scan_f32_kernel<M, D, E, true>  (COS)
  R2     the same call                          other d    any           scan_f32_kernel<M, D or 0, E, true>
         (launch_f32_e, wvg_scan.hip:839-848)
  R3     c.search(qs, k, allow), nq = 5         any        any           scan_f32_kernel<M, D, E, true> with the
         (K1Q needs !allow, wvg_search.hip:264)                               shared allow window (tile_mask)
  R4     c.search(q, k, allow), one query       any        any           scan_f32_stream_kernel<M, D, E>, allow
         (wvg_search.hip:924-930: the window read from pinned host memory)    window
  R5     wvg_search_device, nq = 1              d % 4 == 0 any           scan_f32_kernel<M, D, E, false> +
         (run_search without a slot -> launch_scan_f32 -> launch_fixed,       merge_keys_kernel<E>
         wvg_scan.hip:849-856; launch_merge_lists, wvg_search.hip:442)
  R6     wvg_search_device_pipelined, nq = 3    d % 4 == 0 any           scan_f32_stream_kernel<M, D, E> over 3
         (wvg_search.hip:1334-1374)                                           queries, per-list ready hand-offs

Every call runs twice back to back: consecutive scans of a corpus alternate
direction (next_direction, wvg_search.hip:141), so the upward and the downward
walk must each equal the oracle.

Row loads: at these sizes plain_loads (wvg_search.hip:158-164) gives the
default-policy loads (row_dot_or_l2_fixed<M, D, 64, false>); the second test
opens a cache_reuse = 0 context, where R1 and R6 run the non-temporal form
row_dot_or_l2_fixed<M, D, 64> at d = 768 / 1536 (R2's co-scheduled launch keeps
default-policy loads by design, wvg_search.hip:376-379).

Not reached from here: scan_f32_mq_kernel<.., Q = 2, ..> (the product's k1_mq
is 4), the FILT = true form (coalesced filtered callers,
tests/test_gpu_coalesce.py) and scan_f32_qlist_kernel (the bf16 screen's exact
rescan, tests/test_gpu_screen.py).  profiles/r07/k1_matrix/ holds the kernel
names one traced run of this module launched.

tests/test_capi.py checks K1 below against the kernel names in the library, so
a new fixed length fails there until it has a row here.
"""
import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import (KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_HAMMING, METRIC_L2, METRIC_MANHATTAN)
from weaviate_amd.device import Corpus, allow_bitmap

from test_gpu_parity import bits, check_topk, prep_query, stored_rows

# The specializations the library is expected to hold (tests/test_capi.py compares
# them with the kernel names): fixed row lengths of the scan / stream / COS kernels,
# the lengths K1Q is built for, and the register-list sizes.
K1 = {"fixed_d": (128, 768, 1536), "mq_d": (128, 768), "e": (1, 2, 4)}
GENERIC_D = (200, 300, 37)  # a multiple of 4; above the 256-float inline query; a scalar tail (host routes only)
DIMS = K1["fixed_d"] + GENERIC_D
METRICS = [METRIC_L2, METRIC_DOT, METRIC_COSINE, METRIC_MANHATTAN, METRIC_HAMMING]  # = the oracle's metric ids
KS = [1, 64, 65, 128, 129, 256]  # both sides of the E = 1 | 2 | 4 boundaries and the largest fused k

N = 4000 + 17  # ragged against the 64-row tile
DEAD = [0, 63, 64, 4016]


def synth(orc, metric, seed, n, d):
    """Uniform [-1, 1) rows; hamming counts equal elements, so integers 0..3 there."""
    if metric == METRIC_HAMMING:
        return np.floor(orc.synth_rows(seed, 0, n, d, 1) / 64).astype(np.float32)
    return orc.synth_rows(seed, 0, n, d, 0)


def allow_ids(n):
    """~300 ids over the whole range with a five-tile hole (tiles 20..24), so
    tiles are skipped (mask 0) and partially allowed; some deleted ids too."""
    a = np.arange(5, n, 13)
    a = a[(a < 1280) | (a >= 1600)]
    return np.union1d(a, [63, 64, n - 1]).astype(np.uint64)


def device_search(lib, c, fn, qs, k, reps=2):
    """wvg_search_device / wvg_search_device_pipelined: `reps` calls back to back on
    one workspace, no sync between them; [(ids, dists, counts)] per call."""
    import torch

    dev = torch.device("cuda:0")
    nq = len(qs)
    ws = torch.zeros(lib.wvg_search_workspace_size(c.handle, nq, k), dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(np.ascontiguousarray(qs, dtype=np.float32)).to(dev)
    outs = []
    for _ in range(reps):
        oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
        od = torch.empty((nq, k), dtype=torch.float32, device=dev)
        oc = torch.empty(nq, dtype=torch.int32, device=dev)
        _lib.check(fn(c.handle, tq.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), ws.data_ptr(),
                      ws.numel(), torch.cuda.current_stream().cuda_stream))
        outs.append((oi, od, oc))
    torch.cuda.synchronize()
    return [(oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32))
            for oi, od, oc in outs]


class Case:
    """One corpus, its queries and the oracle's distances (computed once)."""

    def __init__(self, cx, orc, metric, d, nq=5):
        self.orc, self.metric, self.d = orc, metric, d
        rows = synth(orc, metric, 1000 + 7 * d + metric, N, d)
        self.qs = synth(orc, metric, 2000 + 7 * d + metric, nq, d)
        self.c = Corpus(cx, KIND_F32, metric, d, N)
        self.c.upsert(np.arange(N, dtype=np.uint64), rows)
        self.c.delete(np.array(DEAD, np.uint64))
        self.valid = np.ones(N, np.uint8)
        self.valid[DEAD] = 0
        self.allowed = allow_ids(N)
        self.allow_valid = np.zeros(N, np.uint8)
        self.allow_valid[self.allowed.astype(np.int64)] = 1
        self.allow_valid &= self.valid
        self.allow_words = allow_bitmap(self.allowed, N)
        srows = stored_rows(orc, metric, rows)
        self.pq = np.stack([prep_query(orc, metric, q) for q in self.qs])  # cosine: normalized (device routes take these)
        self.all_d = [orc.dist_all(metric, q, srows) for q in self.pq]
        self.ids = np.arange(N, dtype=np.uint64)

    def check(self, res, qsel, k, valid):
        ids, dists, counts = res
        assert len(ids) == len(qsel)
        for j, qi in enumerate(qsel):
            check_topk(self.orc, ids[j], dists[j], counts[j], self.all_d[qi], self.ids, k, valid)

    def host(self, qsel, k, allow=False):
        """c.search twice back to back (R1 - R4)."""
        q = self.qs[qsel[0]] if len(qsel) == 1 else self.qs[qsel]
        for _ in range(2):
            res = self.c.search(q, k, self.allow_words if allow else None)
            self.check(res, qsel, k, self.allow_valid if allow else self.valid)

    def device(self, fn, qsel, k):
        """R5 / R6: two calls back to back, each against the oracle."""
        for res in device_search(self.c.lib, self.c, fn, self.pq[qsel], k):
            self.check(res, qsel, k, self.valid)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_k1_matrix(ctx, orc, metric, d):
    cs = Case(ctx, orc, metric, d)
    lib = cs.c.lib
    try:
        for k in KS:
            cs.host([0], k)                        # R1
            cs.host([0, 1, 2, 3, 4], k)            # R2
            cs.host([0, 1, 2, 3, 4], k, True)      # R3
            cs.host([1], k, True)                  # R4
            if d % 4 == 0:
                cs.device(lib.wvg_search_device, [2], k)                  # R5
                cs.device(lib.wvg_search_device_pipelined, [4, 0, 3], k)  # R6
    finally:
        cs.c.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [768, 1536])
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT])
def test_k1_matrix_nontemporal_loads(ctx, orc, metric, d):
    """A streaming context (cache_reuse = 0): the fixed-length kernels' non-temporal row loads."""
    from weaviate_amd.device import Context

    cx = Context(0, cache_reuse=0)
    try:
        cs = Case(cx, orc, metric, d)
        try:
            for k in [10, 129]:
                cs.host([0], k)                                                     # R1
                cs.host([0, 1, 2, 3, 4], k)                                         # R2
                cs.device(cs.c.lib.wvg_search_device_pipelined, [4, 0, 3], k)       # R6
        finally:
            cs.c.destroy()
    finally:
        cx.close()

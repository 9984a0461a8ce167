"""K5 (BQ Hamming scan) specialization matrix: every reachable instantiation of
scan_bq_kernel, and the other readers of the tiled code layout, against the
oracle's CPU popcount -- bit-exact (Hamming distances are integers < 2^24).

scan_bq_kernel<E, NCH, COS, EMIT> (wvg_bq.hip:45-145):
  E     64-key registers per wave list: 1 for k <= 64, 2 for k <= 128, 4 above
        (launch_bq_k, wvg_bq.hip:168-174)
  NCH   16-byte chunks per row: 1 / 6 / 12 fixed (the next live tile's chunks are
        prefetched), 0 the generic loop (launch_bq_ec, wvg_bq.hip:147-159)
  COS   the co-scheduled 1D grid of an unfiltered batch (launch_bq_e,
        wvg_bq.hip:161-166; plan_search, wvg_search.hip:251-254)
  EMIT  0 plain; 1 the heap replay's per-wave record in LDS; 2 the record in HBM
        (launch_scan_bq_emit, wvg_bq.hip:181-186)

A row of words = ceil(d / 64) code words is stored as ceil(words / 2) chunks of
two words; with an odd word count the upper half of the last chunk is padding,
zero in the tiles (bq_store_kernel, wvg_bq.hip:216-229) and in the query
(prepare_queries_host, wvg_search.hip:100-117; on the device route a memset plus
a 2-D copy whose pitches differ only then, wvg_search.hip:1621-1628).  DIMS gives
every fixed NCH an even and an odd word count and the generic loop short, odd
and long rows.

Routes of one d (NCH = chunks if chunks in K5["nch"] else 0; E from k or R):

  route  call                                        kernel
  B1     c.search(q, k), one query                   scan_bq_kernel<E, NCH, false, 0>
         (wvg_search -> search_coalesced, wvg_search.hip:856-862; 3 workgroups
         per CU, wvg_search.hip:235-236)
  B2     c.search(qs, k), nq = 5                     scan_bq_kernel<E, NCH, true, 0>
         (search_batch, wvg_search.hip:869; cosched = nq > 1 && !allow)
  B3     c.search(qs, k, allow), nq = 5 and nq = 1   scan_bq_kernel<E, NCH, false, 0> with the
         (a filtered batch is not co-scheduled; a filtered  allow window: next_live of the fixed-NCH
         BQ query skips the coalescer, wvg_search.hip:856)  prefetch walks over skipped tiles
  B4     wvg_search_device, nq = 1 and nq = 3        bq_encode_kernel, the pitched copy, then
         (wvg_search.hip:1621-1629; normalized queries)     scan_bq_kernel<E, NCH, nq > 1, 0>
  B5     search_bq_candidates(b, qs, R), nq = 1 / 8  scan_bq_kernel<E, NCH, false | true, 1>
         (wvg_search.hip:1240-1265 -> bq_rescore_replay, wvg_replay.hip:759 ->
         replay_scan, :651; emit_plan_for, :480-497, plans these sizes into LDS);
         search_bq_rescore adds the exact rescore of the popped ids
  B6     c.search(q, 300), candidates at R = 300     ordkeys_bq_kernel (wvg_select.hip:68-91) via
         (wvg_search.hip:882-883; wvg_replay.hip:771,793)   search_large_k / bq_heap_candidates_select
  B7     upsert_codes, get / get_batch,              bq_store_kernel, the tile reads of
         distance_by_ids                             wvg_corpus.hip:492-515 and dist_by_ids_kernel
                                                     (wvg_select.hip:415)
  rerun  search_bq_candidates, a batch of 160        first pass scan_bq_kernel<E, NCH, true, 1 | 2>,
         (test_bq_rerun_reached below)               then rerun_full (wvg_replay.hip:574-623):
                                                     scan_bq_kernel<E, NCH, false, 2> with emit_seed

Every call runs twice back to back (consecutive scans of a corpus alternate
direction, next_direction, wvg_search.hip:141).

Not reached from here: scan_bq_kernel<1, NCH, true, 2> -- a co-scheduled first
pass recorded into HBM needs a batch that emit_plan_for plans out of LDS, which
at R <= 64 happens only above ~4400 rows per wave (est + 6 sqrt(est) + 64 > the
smallest LDS record, 512 keys): a batch of >= 129 queries over more than 140k
rows, left out to keep the corpora small (the rerun test's R = 128 / 256 reach
the E = 2 / 4 forms) -- and scan_bq_group_kernel
(tests/test_gpu_group_bq.py).  profiles/r15/bq_k5_matrix/ holds the kernel
names one traced run of this module launched: 68 of the 72 instantiations.

tests/test_capi.py checks K5 and DIMS below against the kernel names in the
library, so a new `case N:` of launch_bq_ec fails there until it has rows here.
"""
import numpy as np
import pytest

from weaviate_amd._lib import KIND_BQ, KIND_F32, METRIC_COSINE, METRIC_L2
from weaviate_amd.device import Corpus, allow_bitmap, search_bq_candidates, search_bq_rescore

from test_gpu_k1_matrix import allow_ids, device_search
from test_gpu_parity import bits, check_topk, prep_query, stored_rows

pytestmark = pytest.mark.gpu

# The specializations the library is expected to hold (tests/test_capi.py compares
# them with the kernel names): fixed chunk counts, register-list sizes, record modes.
K5 = {"nch": (1, 6, 12), "e": (1, 2, 4), "emit": (0, 1, 2)}
#        d: words chunks kernel
DIMS = (64,    # 1   1   NCH 1, odd: the upper half of the only chunk is padding
        100,   # 2   1   NCH 1, 36 used bits in the last word
        128,   # 2   1   NCH 1
        130,   # 3   2   generic, odd, 2 used bits in the last word
        300,   # 5   3   generic, odd (a real model size)
        1024,  # 16  8   generic
        3072,  # 48  24  generic, long loop
        700,   # 11  6   NCH 6, odd
        768,   # 12  6   NCH 6
        1440,  # 23  12  NCH 12, odd
        1536)  # 24  12  NCH 12
ODD_DIMS = (130, 700, 1440)  # B6 / B7: odd word counts under the generic, NCH 6 and NCH 12 kernels
KS = [1, 64, 65, 128, 129, 256]  # both sides of the E = 1 | 2 | 4 boundaries and the largest fused list
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)

N = 4000 + 17  # ragged against the 64-row tile
DEAD = [0, 63, 64, N - 1]
ROW_POS, ROW_NZERO, ROW_ZERO, ROW_NONFINITE, ROW_NEG = 100, 101, 102, 103, N - 2  # ROW_NEG: in the ragged last tile
NQ = 8
Q_NEG, Q_POS, Q_NONFINITE = 5, 6, 7  # queries 0..4 are random


def words_of(d):
    return (d + 63) // 64


def nch_of(d):
    """The NCH template argument launch_bq_ec picks for dimension d (0: the generic loop)."""
    chunks = (words_of(d) + 1) // 2
    return chunks if chunks in K5["nch"] else 0


def make_rows(orc, d):
    rows = orc.synth_rows(3000 + 7 * d, 0, N, d, 0)  # uniform [-1, 1)
    j = np.arange(d)
    rows[ROW_NEG] = np.float32(-0.5)   # every used bit set
    rows[ROW_POS] = np.float32(0.75)   # code 0
    rows[ROW_NZERO] = np.float32(-0.0)  # -0.0 < 0 is false: code 0
    rows[ROW_ZERO] = np.float32(0.0)
    rows[ROW_NONFINITE, j % 3 == 0] = np.nan  # NaN < 0 is false
    rows[ROW_NONFINITE, j % 3 == 1] = -np.inf
    rows[ROW_NONFINITE, j % 7 == 2] = np.inf
    return rows


def make_queries(orc, d):
    qs = orc.synth_rows(4000 + 7 * d, 0, NQ, d, 0)
    j = np.arange(d)
    qs[Q_NEG] = np.float32(-0.25)
    qs[Q_POS] = np.float32(0.25)
    qs[Q_NONFINITE, j % 5 == 0] = np.nan
    qs[Q_NONFINITE, j % 5 == 1] = np.float32(-0.0)
    qs[Q_NONFINITE, j % 7 == 3] = -np.inf
    return qs


class Ref:
    """Rows, queries and the oracle's codes and Hamming distances of one (metric, d):
    computed once, shared by the tests of that case and never modified."""

    def __init__(self, orc, metric, d):
        self.orc, self.metric, self.d = orc, metric, d
        self.rows = make_rows(orc, d)
        self.qs = make_queries(orc, d)
        self.srows = stored_rows(orc, metric, self.rows)  # cosine: normalized before the sign; zero stays zero
        self.codes = orc.bq_encode_rows(self.srows)
        self.pq = np.stack([prep_query(orc, metric, q) for q in self.qs])  # the device route takes these
        self.qcodes = [orc.bq_encode(q) for q in self.pq]
        self.all_d = [orc.bq_dist_all(qc, self.codes) for qc in self.qcodes]
        self.ids = np.arange(N, dtype=np.uint64)
        self.valid = np.ones(N, np.uint8)
        self.valid[DEAD] = 0
        self.allowed = allow_ids(N)  # a five-tile hole, partially allowed tiles, some deleted ids
        self.allow_valid = np.zeros(N, np.uint8)
        self.allow_valid[self.allowed.astype(np.int64)] = 1
        self.allow_valid &= self.valid
        self.allow_words = allow_bitmap(self.allowed, N)
        for a in (self.rows, self.qs, self.srows, self.codes, self.pq, self.valid, self.allow_valid, self.allow_words,
                  *self.qcodes, *self.all_d):
            a.setflags(write=False)
        # the fixture is what it claims: every used bit of the all-negative row and query is set, no padding bit is
        pop = lambda c: sum(bin(int(w)).count("1") for w in c)  # noqa: E731
        assert pop(self.codes[ROW_NEG]) == d and pop(self.qcodes[Q_NEG]) == d
        assert not self.codes[[ROW_POS, ROW_NZERO, ROW_ZERO]].any() and not self.qcodes[Q_POS].any()
        assert self.all_d[Q_NEG][ROW_NEG] == 0 and self.all_d[Q_POS][ROW_NEG] == d


_REFS = {}


def ref_of(orc, metric, d):
    if (metric, d) not in _REFS:
        _REFS[(metric, d)] = Ref(orc, metric, d)
    return _REFS[(metric, d)]


def bq_corpus(cx, r):
    c = Corpus(cx, KIND_BQ, r.metric, r.d, N)
    c.upsert(r.ids, r.rows)
    c.delete(np.array(DEAD, np.uint64))
    return c


def check_search(r, res, qsel, k, valid):
    ids, dists, counts = res
    assert len(ids) == len(qsel)
    for j, qi in enumerate(qsel):
        check_topk(r.orc, ids[j], dists[j], counts[j], r.all_d[qi], r.ids, k, valid)
        if qi == Q_NEG and valid[ROW_NEG]:  # the all-negative query finds the all-negative row at distance 0, first
            assert ids[j][0] == ROW_NEG and bits(dists[j][0]) == 0


def host(r, c, qsel, k, allow=False):
    """c.search twice back to back (B1 - B3, B6)."""
    q = r.qs[qsel[0]] if len(qsel) == 1 else r.qs[qsel]
    for _ in range(2):
        res = c.search(q, k, r.allow_words if allow else None)
        check_search(r, res, qsel, k, r.allow_valid if allow else r.valid)


def check_pops(r, c, qsel, R, reps=2):
    """search_bq_candidates == the reference heap's pop order (ids, distance bits, counts, KEY_NONE tail)."""
    q = r.qs[qsel[0]] if len(qsel) == 1 else r.qs[qsel]
    for _ in range(reps):
        ci, cd, cc = search_bq_candidates(c, q, R)
        assert len(ci) == len(qsel)
        for j, qi in enumerate(qsel):
            pi, pd = r.orc.heap_pops(r.all_d[qi], R, r.valid)
            assert cc[j] == len(pi), (qi, cc[j], len(pi))
            assert np.array_equal(ci[j][:cc[j]], pi), qi
            assert np.array_equal(bits(cd[j][:cc[j]]), bits(pd)), qi
            assert np.all(ci[j][cc[j]:] == KEY_NONE)


# ---- B1 - B3: the host routes --------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_COSINE])
def test_bq_k5_host_routes(ctx, orc, metric, d):
    r = ref_of(orc, metric, d)
    c = bq_corpus(ctx, r)
    try:
        for k in KS:
            host(r, c, [0], k)                                   # B1
            host(r, c, [Q_NEG], k)                               # B1, zero distance / padding
            host(r, c, [0, Q_NEG, Q_POS, Q_NONFINITE, 1], k)     # B2
            host(r, c, [2, Q_NEG, Q_NONFINITE, 3, 4], k, True)   # B3, nq = 5
            host(r, c, [1], k, True)                             # B3, nq = 1
    finally:
        c.destroy()


# ---- B4: the device route ----------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_COSINE])
def test_bq_k5_device_route(ctx, orc, metric, d):
    r = ref_of(orc, metric, d)
    c = bq_corpus(ctx, r)
    try:
        for k in KS:
            for qsel in ([Q_NEG], [4, Q_NEG, Q_NONFINITE]):  # nq = 3: the second and third query's pitch
                for res in device_search(c.lib, c, c.lib.wvg_search_device, r.pq[qsel], k):
                    check_search(r, res, qsel, k, r.valid)
    finally:
        c.destroy()


# ---- B5: the heap replay's recording scan ------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
def test_bq_k5_heap_replay(ctx, orc, d):
    r = ref_of(orc, METRIC_L2, d)
    c = bq_corpus(ctx, r)
    # the exact side of the rescore: the same sign codes, the non-finite row made finite (NaN distances carry
    # sign / payload bits that are not this module's subject; tests/test_gpu_k1_special_values.py pins those)
    frows = r.rows.copy()
    frows[ROW_NONFINITE] = np.where(r.rows[ROW_NONFINITE] < 0, np.float32(-2), np.float32(2))
    assert np.array_equal(orc.bq_encode(frows[ROW_NONFINITE]), r.codes[ROW_NONFINITE])
    f = Corpus(ctx, KIND_F32, METRIC_L2, d, N)
    try:
        f.upsert(r.ids, frows)
        f.delete(np.array(DEAD, np.uint64))
        for R in KS:
            check_pops(r, c, [Q_NEG], R)          # <E, NCH, false, 1>
            check_pops(r, c, list(range(NQ)), R)  # <E, NCH, true, 1>
        finite = [q for q in range(NQ) if q != Q_NONFINITE]
        for R in (64, 128, 256):  # one per E
            want = [orc.flat_search_bq(frows, r.qs[qi], 10, R, 0, r.valid) for qi in finite]
            for _ in range(2):
                gi, gd, gc = search_bq_rescore(c, f, r.qs[finite], 10, R)
                for j, qi in enumerate(finite):
                    ri, rd = want[j]
                    assert gc[j] == len(ri), (R, qi)
                    assert np.array_equal(gi[j][:gc[j]], ri), (R, qi, gi[j], ri)
                    assert np.array_equal(bits(gd[j][:gc[j]]), bits(rd)), (R, qi)
    finally:
        f.destroy()
        c.destroy()


# ---- B6: beyond the fused list -----------------------------------------------------------------
@pytest.mark.parametrize("d", ODD_DIMS)
def test_bq_k5_beyond_fused_list(ctx, orc, d):
    r = ref_of(orc, METRIC_L2, d)
    c = bq_corpus(ctx, r)
    try:
        host(r, c, [Q_NEG], 300)
        host(r, c, [0, Q_NEG, Q_POS, Q_NONFINITE, 1], 300)
        host(r, c, [1], 300, True)
        check_pops(r, c, [Q_NEG], 300)
        check_pops(r, c, list(range(NQ)), 300)
    finally:
        c.destroy()


# ---- B7: the other readers of the layout -------------------------------------------------------
@pytest.mark.parametrize("d", ODD_DIMS)
def test_bq_k5_layout_readers(ctx, orc, d):
    r = ref_of(orc, METRIC_L2, d)
    c = Corpus(ctx, KIND_BQ, METRIC_L2, d, N)
    try:
        c.upsert_codes(r.ids, r.codes)
        c.delete(np.array(DEAD, np.uint64))
        live = np.array([1, 62, 65, ROW_POS, ROW_NONFINITE, 2047, 2048, ROW_NEG], np.uint64)
        for i in live:
            assert np.array_equal(c.get(int(i)), r.codes[int(i)]), i
        some = np.concatenate([live, np.array(DEAD, np.uint64), np.arange(3, N, 41, dtype=np.uint64)])
        got, ok = c.get_batch(some)
        want_ok = r.valid[some.astype(np.int64)].astype(bool)
        assert np.array_equal(ok, want_ok)
        assert np.array_equal(got[ok], r.codes[some[ok].astype(np.int64)])
        assert not got[~ok].any()
        for qi in (0, Q_NEG, Q_NONFINITE):
            dd, ok = c.distance_by_ids(r.qs[qi], some)
            assert np.array_equal(ok, want_ok), qi
            assert np.array_equal(bits(dd[ok]), bits(r.all_d[qi][some[ok].astype(np.int64)])), qi
        # the rows as uploaded codes search like the encoded float rows
        for k in (1, 65, 256, 300):
            host(r, c, [Q_NEG], k)
            host(r, c, [0, Q_NEG, Q_POS, Q_NONFINITE, 1], k)
    finally:
        c.destroy()


# ---- the rerun -------------------------------------------------------------------------------------
RERUN_N, RERUN_NQ, RERUN_ZERO_Q = 65536, 160, (0, 77, 159)


def staircase_codes(d, n, seed):
    """Row i has nb = 64 - (i mod 2048) // 32 set bits: 64 down to 1, 32 rows per level, a new
    staircase every 2048 rows.  The bits fill a window of the d used bits that starts at a random
    bit and wraps, so only code 0 sees the staircase (distance = nb); a random code sees no trend."""
    w = words_of(d)
    rng = np.random.default_rng(seed)
    nb = (64 - (np.arange(n) % 2048) // 32).astype(np.int32)
    start = rng.integers(0, d, n).astype(np.int32)
    j = np.arange(d, dtype=np.int32)
    codes = np.zeros((n, w), np.uint64)
    for a in range(0, n, 8192):
        b = min(n, a + 8192)
        on = ((j[None, :] - start[a:b, None]) % d) < nb[a:b, None]
        packed = np.packbits(on, axis=1, bitorder="little")
        buf = np.zeros((b - a, w * 8), np.uint8)
        buf[:, :packed.shape[1]] = packed
        codes[a:b] = buf.view("<u8")
    return codes, nb


@pytest.mark.parametrize("d", [64, 130, 700, 1440])  # NCH 1, generic, 6, 12; every one an odd word count
def test_bq_rerun_reached(ctx, orc, d):
    """Three queries of a batch of 160 overflow every wave's record buffer, so replay_collect
    (wvg_replay.hip:713-722) reruns them with rerun_full: scan_bq_kernel<E, NCH, false, 2> seeded
    with the first pass's thresholds (emit_seed) -- and the result is still the heap's.

    The arithmetic, at 256 CUs (plan_search, wvg_search.hip:251-254; emit_plan_for,
    wvg_replay.hip:480-497):
      groups   pq_cosched_groups(160, 256 * bq_cos_gpc = 512) = 8 * max(1, 512 / 160 / 8) = 8: 32 waves
      ranges   ntiles = 65536 / 64 = 1024, so wave w scans tiles [32 w, 32 w + 32): 2048 rows, exactly
               one staircase of staircase_codes
      rows     (1024 / 32 + 2) * 64 = 2176
      LDS      wg_per_cu = ceil(8 * 160 / 256) = 5; lds_wg = max(16 KiB, 160 KiB / 5 - 16 KiB) = 16 KiB;
               lcap = 16 KiB / (4 waves * 8 B) = 512 keys
      R = 64   est = 64 (1 + ln(2176 / 64)) = 290; 512 >= 290 + 6 sqrt(290) + 64 = 456: LDS, cap 512
      R = 128  est = 491; 512 < 491 + 133 + 64: HBM, cap = align_up(2 * 491 + 256, 64) = 1280
      R = 256  est = 804; HBM, cap = align_up(2 * 804 + 256, 64) = 1920
    A wave records the rows strictly below its running R-th distance (offer_dist_emit,
    wvg_topk.hpp:254-273).  Against code 0 every 64-row tile of a wave holds two levels below all
    earlier ones, so all 2048 rows are recorded: above each cap.  The R = 128 / 256 first passes are
    the co-scheduled HBM form <E, NCH, true, 2>.  The other 157 queries are random sign vectors,
    the input the plan's estimate is made for: the batch mixes rerun and plain queries (at d = 64
    a few of the random ones overflow the 512-key record too and are rerun as well).

    No counter is exposed: profiles/r15/bq_k5_matrix/ lists the <E, NCH, false, 2> kernels one
    traced run of this test launched."""
    n, nq, w = RERUN_N, RERUN_NQ, words_of(d)
    codes, nb = staircase_codes(d, n, 900 + d)
    rng = np.random.default_rng(901 + d)
    qs = rng.choice(np.array([-1, 1], np.float32), size=(nq, d))
    qs[list(RERUN_ZERO_Q)] = np.float32(1)  # code 0
    qcodes = [orc.bq_encode(q) for q in qs]
    all_d = [orc.bq_dist_all(qc, codes) for qc in qcodes]
    assert not qcodes[0].any() and np.array_equal(all_d[0], nb.astype(np.float32))
    b = Corpus(ctx, KIND_BQ, METRIC_L2, d, n)
    try:
        b.upsert_codes(np.arange(n, dtype=np.uint64), codes)
        for R in (64, 128, 256):  # one per E
            ci, cd, cc = search_bq_candidates(b, qs, R)
            for qi in range(nq):
                pi, pd = orc.heap_pops(all_d[qi], R)
                assert cc[qi] == len(pi) == R, (R, qi, cc[qi])
                assert np.array_equal(ci[qi], pi), (R, qi)
                assert np.array_equal(bits(cd[qi]), bits(pd)), (R, qi)
    finally:
        b.destroy()

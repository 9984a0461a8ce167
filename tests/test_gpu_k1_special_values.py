"""NaN, +-inf and +-0 distances, and lists that cannot fill with finite
distances, through the K1 scan and everything that consumes its keys.

Order contract (wvg_common.hpp:19-22, oracle.ord_key): ascending by
(ord(dist), id) with NaN after +inf and -0 before +0.  Ids are compared
exactly; distance bits after mapping every NaN on both sides to 0x7FC00000
(the device canonicalises NaN, x86 gives 0xFFC00000 for inf - inf).  Only the
lexicographic oracle is used: the reference heap's comparisons are no total
order on NaN and on -0 / +0.

Corpus: 4017 integer-valued rows (floor(2x): exact ties are common) stored
with upsert_codes, so cosine rows stay as given and the oracle sees what is
stored.  Planted, each kind in the first tile and in a later one: a NaN
component, a +inf and a -inf component, rows of 3e38 (the L2 / manhattan sums
overflow to +inf), all-zero and all -0.0 rows, rows whose every product with
query 0 of scenario 1 underflows to -0, and three identical rows.  The
underflow rows are the only way to a +0 dot distance (dot = -0): the
reference's accumulators and its scalar-tail sum start at +0 and
(+0) + (-0) = +0, so zero rows and zero queries always give dot = +0, distance
-0; and without a scalar tail (d = 128) dot_256 ends in (+0) + t, so there the
oracle cannot produce a +0 dot distance at all.

Scenarios of test_k1_special_values (five queries each; every non-vacuity
assert is on the oracle's own numbers, before any GPU result is looked at):
  1  finite queries: the special rows rank at their documented places.  In
     this corpus the zeros of the dot distances rank around 650 - 750 of 4015:
     no returned list holds them, only search_by_distance(+inf) passes them.
  2  one +inf component: every distance is +inf, -inf or NaN.  L2 / manhattan:
     lists of +inf ties by id.  Dot: about 1000 -inf ties fill every returned
     list, the +inf and NaN rows rank behind them.  Cosine: the host routes
     normalize the query, which makes it NaN (the scenario equals 3 there);
     the device routes take the inf query as given: -inf ties as for dot.
  3  one NaN component: every distance is NaN, the result is the k smallest ids
  4  (dot only) all-zero queries: every finite row's distance is -0
Hamming distances are finite counts: its scenarios are a finite and a
NaN-holding query over rows with NaN components (as test_hamming_nan_rows).

The -0 / +0 order inside returned lists is test_k1_signed_zero_order's: a
corpus of its own whose twelve nearest rows are six -0 and six +0 distances,
at d = 37 and d = 44.

Paths, at d = 128 (fixed-length kernels) and d = 37 (generic, scalar tail; host
routes only): routes R1, R2, R5, R6 of tests/test_gpu_k1_matrix.py at k = 10 and
129, each route's two calls back to back, k = 300 (the radix select,
wvg_select.hip), both range searches with a finite and a +inf target, and
wvg_topk_merge_packed over the R6 results of the corpus split into two halves
(merge_pairs_kernel).
"""
import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import (KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_HAMMING, METRIC_L2, METRIC_MANHATTAN)
from weaviate_amd.device import Corpus

from test_gpu_k1_matrix import device_search

N = 4000 + 17
HALF = 2048  # the second half-corpus's id_base (a multiple of 64)
DEAD = [64, 3000]
NQ = 5
C_ROW, C_Q = 9, 20  # columns of the rows' and of the queries' planted inf / NaN component
TINY = np.float32(1.4e-45)  # the smallest subnormal: 0.375 * TINY rounds to zero, keeping the sign

# planted rows: (first tile, a later tile)
R_NAN, R_PINF, R_NINF, R_BIG, R_ZERO, R_NZERO, R_UFLOW = (5, 2005), (7, 2007), (9, 2009), (11, 2011), (13, 2013), \
    (15, 2015), (17, 2017)
R_SAME = (19, 21, 2019)


def canon(d):
    """Distance bits with every NaN mapped to 0x7FC00000."""
    u = np.asarray(d, dtype=np.float32).view(np.uint32).copy()
    u[((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)] = 0x7FC00000
    return u


def finite_queries(orc, d):
    """Multiples of 1/8 with no zero element: +-0.125, +-0.375 (sums stay exact)."""
    return (np.floor(orc.synth_rows(4100 + d, 0, NQ, d, 0) * 2) * np.float32(0.25) + np.float32(0.125)).astype(np.float32)


def make_rows(orc, metric, d):
    rows = np.floor(orc.synth_rows(4000 + d, 0, N, d, 0) * 2).astype(np.float32)
    if metric == METRIC_HAMMING:  # NaN components in the SIMD blocks and (d = 37) the scalar tail
        rng = np.random.default_rng(3)
        for r in range(0, N, 3):
            rows[r, rng.integers(0, d)] = np.nan
        rows[R_ZERO, :] = 0.0
        rows[R_NZERO, :] = -0.0
        rows[R_PINF, C_ROW] = np.inf
    else:
        rows[R_NAN, C_ROW] = np.nan
        rows[R_NAN[1], d - 1] = np.nan
        rows[R_PINF, C_ROW] = np.inf
        rows[R_NINF, C_ROW] = -np.inf
        rows[R_BIG, :] = np.float32(3e38)
        rows[R_ZERO, :] = 0.0
        rows[R_NZERO, :] = -0.0
        q0 = finite_queries(orc, d)[0]
        rows[R_UFLOW, :] = np.where(q0 > 0, -TINY, TINY)  # every product with query 0 is a negative underflow
    rows[R_SAME, :] = rows[23]
    return rows


def scenarios(orc, metric, d):
    """[(name, queries [NQ][d])]"""
    fin = finite_queries(orc, d)
    if metric == METRIC_HAMMING:
        fin = np.floor(fin * 4).astype(np.float32)  # integers, as the rows
        qn = fin.copy()
        qn[:, 1] = np.nan
        qn[:, d - 2] = np.nan
        return [("finite", fin), ("nan", qn)]
    qi = fin.copy()
    qi[:, C_Q] = np.inf
    qn = fin.copy()
    qn[np.arange(NQ), [C_Q, 0, d - 1, 3, d // 2]] = np.nan  # blocks and (d = 37) the tail
    out = [("finite", fin), ("inf", qi), ("nan", qn)]
    if metric == METRIC_DOT:
        out.append(("zero", np.zeros((NQ, d), np.float32)))
    return out


def oracle_dists(orc, metric, rows, qs):
    """Per query: the oracle's distances to the stored rows (cosine: the query normalized)."""
    return [orc.dist_all(metric, orc.normalize(q) if metric == METRIC_COSINE else q, rows) for q in qs]


def assert_not_vacuous(metric, d, name, all_d, valid, k=129):
    for qi, dd in enumerate(all_d):
        live = dd[valid.astype(bool)]
        u = live.view(np.uint32)
        if metric == METRIC_HAMMING:
            assert np.isfinite(live).all() and len(set(live.tolist())) > 5
        elif name == "finite":
            assert np.isnan(live).any() and (live == np.inf).any(), (metric, qi)
            if metric == METRIC_DOT:
                assert (live == -np.inf).any() and (u == 0x80000000).any(), qi
                # the underflow rows are made for query 0; without a scalar tail dot_256 ends in (+0) + t: never -0
                assert qi != 0 or d % 8 == 0 or (u == 0).any()
            assert np.isfinite(live).sum() > 300
        elif name == "inf":
            assert np.isfinite(live).sum() < 10 < k
            if metric == METRIC_DOT:
                assert (live == -np.inf).sum() > 300 and (live == np.inf).sum() > 300 and np.isnan(live).sum() > 300
        elif name == "nan":
            assert np.isnan(live).all()
        elif name == "zero":
            zero = live == 0
            assert (zero | np.isnan(live)).all() and zero.sum() > 300 and np.isnan(live).any()


def check_lex(orc, res, all_d, qsel, k, valid, where):
    ids, dists, counts = res
    sel = valid.astype(bool)
    all_ids = np.arange(N, dtype=np.uint64)
    for j, qi in enumerate(qsel):
        li, ld = orc.lex_topk(all_d[qi][sel], all_ids[sel], k)
        cnt = int(counts[j])
        assert cnt == len(li) == min(k, int(sel.sum())), (where, qi, k)
        assert np.array_equal(ids[j][:cnt], li), (where, qi, k)
        assert np.array_equal(canon(dists[j][:cnt]), canon(ld)), (where, qi, k)


def prepared(orc, metric, qs):
    return np.stack([orc.normalize(q) if metric == METRIC_COSINE else q for q in qs])


def build(cx, metric, d, rows, lo, hi, id_base=0):
    c = Corpus(cx, KIND_F32, metric, d, hi - id_base, id_base=id_base)
    c.upsert_codes(np.arange(lo, hi, dtype=np.uint64), rows[lo:hi])
    c.delete(np.array([i for i in DEAD if lo <= i < hi], np.uint64))
    return c


def merge_halves(ctx, lib, halves, pq, k):
    """R6 on each half straight into its packed block, then wvg_topk_merge_packed."""
    import torch

    dev = torch.device("cuda:0")
    nq = len(pq)
    blk = lib.wvg_topk_packed_bytes(nq, k)
    packed = torch.zeros(len(halves) * blk, dtype=torch.uint8, device=dev)
    tq = torch.from_numpy(np.ascontiguousarray(pq)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    keep = []
    for g, c in enumerate(halves):
        ws = torch.zeros(lib.wvg_search_workspace_size(c.handle, nq, k), dtype=torch.uint8, device=dev)
        keep.append(ws)
        base = packed.data_ptr() + g * blk
        _lib.check(lib.wvg_search_device_pipelined(c.handle, tq.data_ptr(), nq, k, base, base + nq * k * 8, None,
                                                   ws.data_ptr(), ws.numel(), stream))
    oi = torch.empty((nq, k), dtype=torch.int64, device=dev)
    od = torch.empty((nq, k), dtype=torch.float32, device=dev)
    oc = torch.empty(nq, dtype=torch.int32, device=dev)
    _lib.check(lib.wvg_topk_merge_packed(ctx.handle, packed.data_ptr(), nq, len(halves), k, k, oi.data_ptr(),
                                         od.data_ptr(), oc.data_ptr(), stream))
    torch.cuda.synchronize()
    return oi.cpu().numpy().view(np.uint64), od.cpu().numpy(), oc.cpu().numpy().astype(np.uint32)


def check_ranges(orc, c, q, dd, valid, where, finite_target=None):
    """SearchByVectorDistance in both callers' semantics, targets: a finite value
    (default: the 150th finite distance) and +inf."""
    sel = valid.astype(bool)
    live_d, live_ids = dd[sel], np.arange(N, dtype=np.uint64)[sel]
    fin = np.sort(live_d[np.isfinite(live_d)])
    if finite_target is None:
        finite_target = float(fin[min(150, len(fin) - 1)]) if len(fin) else 1.0

    def search_fn(total):
        return orc.lex_topk(live_d, live_ids, total)

    for target in (finite_target, float("inf")):
        wi, wd = orc.search_by_distance(search_fn, target, -1)
        gi, gd = c.search_by_distance(q, target, -1)
        assert np.array_equal(gi, wi) and np.array_equal(canon(gd), canon(wd)), (where, "by_distance", target)
        fi, fd, _ = orc.search_by_distance_flat(search_fn, target, -1, max_iterations=3)
        gi, gd = c.search_by_distance_window(q, target)
        assert np.array_equal(gi, fi) and np.array_equal(canon(gd), canon(fd)), (where, "window", target)


def test_comparison_rejects_wrong_special_value_results(orc):
    """check_lex on the oracle's own result passes, and fails for a -0 returned as
    +0, two tied ids swapped, a NaN row ranked before +inf and a short count."""
    metric, d, k = METRIC_DOT, 37, 129
    rows = make_rows(orc, metric, d)
    valid = np.ones(N, np.uint8)
    valid[DEAD] = 0
    all_d = oracle_dists(orc, metric, rows, scenarios(orc, metric, d)[3][1])  # zero queries: -0 distances
    sel = valid.astype(bool)

    def result(dd, kk=k):
        ids, dists = orc.lex_topk(dd[sel], np.arange(N, dtype=np.uint64)[sel], kk)
        return ids.copy(), dists.copy()

    def rejected(ids, dists, count, dd=all_d):
        with pytest.raises(AssertionError):
            check_lex(orc, (ids[None], dists[None], [count]), dd, [0], k, valid, "self-check")

    ids, dists = result(all_d[0])
    check_lex(orc, (ids[None], dists[None], [k]), all_d, [0], k, valid, "self-check")
    neg = np.flatnonzero(dists.view(np.uint32) == 0x80000000)
    assert len(neg) >= 2
    flipped = dists.copy()
    flipped[neg[0]] = 0.0
    rejected(ids, flipped, k)
    swapped = ids.copy()
    swapped[neg[:2]] = ids[neg[:2]][::-1]
    rejected(swapped, dists, k)
    rejected(ids, dists, k - 1)
    # all +inf / NaN (the manhattan "inf" scenario): a NaN row among the +inf ties is noticed
    qi = scenarios(orc, METRIC_MANHATTAN, d)[1][1]
    inf_d = oracle_dists(orc, METRIC_MANHATTAN, make_rows(orc, METRIC_MANHATTAN, d), qi)
    ids, dists = result(inf_d[0])
    assert ids[5] == 6 and (dists == np.inf).all()  # row 5 holds a NaN: it ranks after every +inf row
    wrong_i, wrong_d = ids.copy(), dists.copy()
    wrong_i[5:] = np.concatenate([[5], ids[5:-1]])
    wrong_d[5] = np.nan
    rejected(wrong_i, wrong_d, k, inf_d)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [128, 37])
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT, METRIC_COSINE, METRIC_MANHATTAN, METRIC_HAMMING])
def test_k1_special_values(ctx, orc, metric, d):
    rows = make_rows(orc, metric, d)
    valid = np.ones(N, np.uint8)
    valid[DEAD] = 0
    cases = []
    for name, qs in scenarios(orc, metric, d):
        all_d = oracle_dists(orc, metric, rows, qs)
        assert_not_vacuous(metric, d, name, all_d, valid)
        dev_q, dev_d = prepared(orc, metric, qs), all_d  # the device routes take cosine queries normalized
        if metric == METRIC_COSINE and name == "inf":
            # normalizing a query with an inf component gives NaN, so on the host routes this scenario is
            # all-NaN like the next one; the device routes take the query as given: 1 - dot is +-inf or NaN
            dev_q, dev_d = qs, [orc.dist_all(metric, q, rows) for q in qs]
            assert_not_vacuous(METRIC_DOT, d, name, dev_d, valid)
        cases.append((name, qs, all_d, dev_q, dev_d))
    c = build(ctx, metric, d, rows, 0, N)
    halves = [build(ctx, metric, d, rows, 0, HALF), build(ctx, metric, d, rows, HALF, N, HALF)] if d % 4 == 0 else []
    try:
        for name, qs, all_d, dev_q, dev_d in cases:
            run_paths(ctx, orc, c, halves, d, name, qs, all_d, dev_q, dev_d, valid)
    finally:
        for x in [c] + halves:
            x.destroy()


def run_paths(ctx, orc, c, halves, d, name, qs, all_d, dev_q, dev_d, valid, ks=(10, 129), finite_target=None):
    """Every path of the module for one scenario.  Each route's two calls are
    consecutive, so they scan in opposite directions (every search of a corpus
    flips it, next_direction)."""
    lib = _lib.load()
    for k in ks:
        for rep in range(2):
            check_lex(orc, c.search(qs[0], k), all_d, [0], k, valid, (name, "R1", rep))
        for rep in range(2):
            check_lex(orc, c.search(qs, k), all_d, range(NQ), k, valid, (name, "R2", rep))
        if d % 4 == 0:
            for rep, res in enumerate(device_search(lib, c, lib.wvg_search_device, dev_q[1:2], k)):
                check_lex(orc, res, dev_d, [1], k, valid, (name, "R5", rep))
            for rep, res in enumerate(device_search(lib, c, lib.wvg_search_device_pipelined, dev_q[2:5], k)):
                check_lex(orc, res, dev_d, [2, 3, 4], k, valid, (name, "R6", rep))
            check_lex(orc, merge_halves(ctx, lib, halves, dev_q[:3], k), dev_d, [0, 1, 2], k, valid,
                      (name, "merge_packed"))
    check_lex(orc, c.search(qs[:2], 300), all_d, [0, 1], 300, valid, (name, "select"))
    check_ranges(orc, c, qs[0], all_d[0], valid, name, finite_target)


# -0 / +0 at the head of the list --------------------------------------------------------------
Z_NEG = (13, 40, 70, 2013, 2050, 4000)  # dot = +0: distance -0
Z_POS = (5, 17, 66, 2005, 2017, 3990)   # dot = -0: distance +0 (smaller ids than their -0 neighbours)


def signed_zero_rows(orc, d):
    """Non-positive integer rows, so every dot with a positive query is <= 0 and
    every distance >= -0; the twelve planted rows are the head of every list."""
    rows = -np.abs(np.floor(orc.synth_rows(4200 + d, 0, N, d, 0) * 2)).astype(np.float32)
    rows[Z_NEG[0]] = 0.0
    rows[Z_NEG[1]] = -0.0
    rows[Z_NEG[2]] = TINY   # positive underflows: dot = +0
    rows[Z_NEG[3]] = 0.0
    rows[Z_NEG[4]] = TINY
    rows[Z_NEG[5]] = -0.0
    rows[Z_POS, :] = -TINY  # every product a negative underflow: dot = -0 (needs the scalar tail)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("d", [37, 44])
def test_k1_signed_zero_order(ctx, orc, d):
    """ord(-0) < ord(+0) inside the returned lists.  Dot distances, positive
    queries (0.125 / 0.375) over non-positive rows: six rows give -0 (zero, -0.0
    and positive-subnormal rows: dot = +0), six give +0 (negative-subnormal
    rows: every product underflows to -0 and, with a scalar tail, so does the
    sum), every other row a positive distance.  The +0 rows have the smaller
    ids, so an order by id alone among the zeros is wrong at every k: k = 10
    holds all six -0 rows and four +0 rows.  d = 37 and d = 44 both have a scalar
    tail (the only lengths at which dot_256 can return -0); 44 is a multiple of
    4, so the device routes and wvg_topk_merge_packed see the pair too.  The
    finite range target is 0: -0 and +0 rows are within it, nothing else."""
    rows = signed_zero_rows(orc, d)
    qs = np.abs(finite_queries(orc, d))
    valid = np.ones(N, np.uint8)
    valid[DEAD] = 0
    all_d = oracle_dists(orc, METRIC_DOT, rows, qs)
    ids = np.arange(N, dtype=np.uint64)[valid.astype(bool)]
    for dd in all_d:  # non-vacuity on the oracle's own top-k
        li, ld = orc.lex_topk(dd[valid.astype(bool)], ids, 16)
        u = ld.view(np.uint32)
        assert li[:6].tolist() == list(Z_NEG) and (u[:6] == 0x80000000).all()
        assert li[6:12].tolist() == list(Z_POS) and (u[6:12] == 0).all()
        assert (ld[12:] > 0).all()
    c = build(ctx, METRIC_DOT, d, rows, 0, N)
    halves = [build(ctx, METRIC_DOT, d, rows, 0, HALF), build(ctx, METRIC_DOT, d, rows, HALF, N, HALF)] \
        if d % 4 == 0 else []
    try:
        run_paths(ctx, orc, c, halves, d, "signed zero", qs, all_d, qs, all_d, valid, ks=(1, 10, 129), finite_target=0.0)
    finally:
        for x in [c] + halves:
            x.destroy()

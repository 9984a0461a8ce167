"""flat.searchByVectorBQ over a BQ class dealt over GPU slabs
(wvg_multi_search_bq_rescore / _candidates, wvg_multi.hip).

Every slab runs the recording Hamming scan, the slabs exchange distance
histograms so that slab s also drops what the R-th smallest distance of slabs
0..s-1 excludes (the cross-slab bound X_s), and the kept rows of all slabs go
through ONE host heap; the popped ids are rescored on the slab that owns them.
Everything here is asserted against the oracle's restatement of the heaps
(oracle/wv_oracle.c) with ids and distance BITS equal -- no tolerance -- and,
for the rescore, against wvg_search_bq_rescore on one plain corpus holding the
same rows.  The box has one GPU: devices = [0] runs the one-rank RCCL
all-gather of the histograms, [0, 0, 0] the peer-copy exchange over three
slabs.
"""
import ctypes
import threading

import numpy as np
import pytest

from weaviate_amd import _lib
from weaviate_amd._lib import (KIND_BQ, KIND_F32, METRIC_COSINE, METRIC_DOT, METRIC_L2, WVG_ERR_INVALID,
                               WVG_ERR_UNSUPPORTED, WvgError)
from weaviate_amd.device import (Corpus, Multi, MultiCorpus, allow_bitmap, multi_search_bq_candidates,
                                 multi_search_bq_rescore, search_bq_rescore)

pytestmark = pytest.mark.gpu

ORC_METRIC = {METRIC_L2: 0, METRIC_DOT: 1, METRIC_COSINE: 2}
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
DEVICES = [[0], [0, 0, 0]]


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def stored(orc, metric, rows):
    return orc.normalize_rows(rows) if metric == METRIC_COSINE else np.asarray(rows, np.float32)


def prep(orc, metric, q):
    return orc.normalize(q) if metric == METRIC_COSINE else np.asarray(q, np.float32)


def assert_pops(got, want, nq):
    """got = (ids, dists, counts) of a candidates call; want[q] = the oracle's (ids, dists) in pop order."""
    ci, cd, cc = got
    for qi in range(nq):
        pi, pd = want[qi]
        assert cc[qi] == len(pi), (qi, cc[qi], len(pi))
        assert np.array_equal(ci[qi][:cc[qi]], pi), qi
        assert np.array_equal(bits(cd[qi][:cc[qi]]), bits(pd)), qi
        assert np.all(ci[qi][cc[qi]:] == NONE)
        assert np.all(np.isposinf(cd[qi][cc[qi]:]))


# ---- the heavy-tie corpus shared by the candidates and the bound tests --------------

TIE_N, TIE_D = 50_037, 64


@pytest.fixture(scope="module")
def tie(orc):
    """d = 64: Hamming 0..64 over 50,037 rows, so hundreds of rows tie at every
    R-th distance; 8 queries; the oracle's pops per (R, mask) computed once."""
    rows = orc.synth_rows(501, 0, TIE_N, TIE_D, 0)
    qs = orc.synth_rows(502, 0, 8, TIE_D, 0)
    codes = orc.bq_encode_rows(rows)
    qcodes = [orc.bq_encode(q) for q in qs]
    cache = {}

    def pops(R, nq, valid=None, tag="all"):
        out = []
        for qi in range(nq):
            key = (R, qi, tag)
            if key not in cache:
                cache[key] = orc.bq_heap_pops(codes, qcodes[qi], R, valid)
            out.append(cache[key])
        return out

    return {"rows": rows, "qs": qs, "pops": pops}


def load_reversed(mc, n, rows):
    ids = np.arange(n, dtype=np.uint64)
    mc.upsert(ids[::-1], rows[::-1])  # any order: routed to the owning slab


@pytest.mark.parametrize("devices", DEVICES)
def test_candidates_equal_the_heap(tie, devices):
    """One heap over all slabs: counts, ids, distance bits and padding of the
    oracle's pops; R up to 256 the bounded filter, 257 and 700 the select-based
    superset per slab.  Three devices: slabs of 16,704 rows."""
    qs = tie["qs"]
    with Multi(devices) as m:
        mc = MultiCorpus(m, KIND_BQ, METRIC_L2, TIE_D, TIE_N)
        try:
            if len(devices) == 3:
                assert mc.shard(1)[2] == 16_704
            load_reversed(mc, TIE_N, tie["rows"])
            for R in (1, 7, 200, 256, 257, 700):
                assert_pops(multi_search_bq_candidates(mc, qs, R), tie["pops"](R, 8), 8)
                assert_pops(multi_search_bq_candidates(mc, qs[0], R), tie["pops"](R, 1), 1)
        finally:
            mc.destroy()


@pytest.mark.parametrize("devices", DEVICES)
def test_where_the_bound_can_go_wrong(tie, devices):
    """Allow windows that leave earlier slabs empty (every X is +inf) or only
    slab 0 populated, a 30 % allow list over 5 % deletes, slab 0 cut down to 50
    live rows at R = 200 (X_1 must stay +inf until 200 rows precede), and fewer
    than R live allowed rows in total (count < R)."""
    n, qs, R = TIE_N, tie["qs"], 200
    rng = np.random.default_rng(7)
    with Multi(devices) as m:
        mc = MultiCorpus(m, KIND_BQ, METRIC_L2, TIE_D, n)
        try:
            load_reversed(mc, n, tie["rows"])

            def check(nq, valid, tag, allow=None, RR=R):
                assert_pops(multi_search_bq_candidates(mc, qs[:nq], RR, allow), tie["pops"](RR, nq, valid, tag), nq)

            # a window inside the last slab only, and one inside slab 0 only
            for tag, lo, hi in (("last", n - 3000, n - 100), ("first", 1000, 9000)):
                av = np.zeros(n, np.uint8)
                av[lo:hi] = 1
                check(3, av, tag, allow_bitmap(range(lo, hi), n))
            # fewer than R live allowed rows in total
            few = np.sort(rng.choice(n, 120, replace=False))
            av = np.zeros(n, np.uint8)
            av[few] = 1
            check(2, av, "few", allow_bitmap(few, n))
            # 5 % deletes, then a 30 % allow list over them
            gone = rng.choice(n, n // 20, replace=False).astype(np.uint64)
            mc.delete(gone)
            valid = np.ones(n, np.uint8)
            valid[gone.astype(np.int64)] = 0
            check(8, valid, "del")
            check(2, valid, "del", RR=500)
            allowed = np.sort(rng.choice(n, int(n * 0.3), replace=False))
            av = np.zeros(n, np.uint8)
            av[allowed] = 1
            check(3, av & valid, "del+allow", allow_bitmap(allowed, n))
            # slab 0 (of three) down to 50 live rows
            slab0 = 16_704
            live0 = np.flatnonzero(valid[:slab0])
            drop = np.setdiff1d(live0, rng.choice(live0, 50, replace=False)).astype(np.uint64)
            mc.delete(drop)
            valid[drop.astype(np.int64)] = 0
            assert int(valid[:slab0].sum()) == 50
            check(8, valid, "slab0=50")
            check(1, valid, "slab0=50", RR=7)
        finally:
            mc.destroy()


def test_empty_slabs(orc):
    """A multi corpus created for 100,000 rows over four slabs of 25,024 holding
    20,000 rows: slab 0 is partly filled, slabs 1, 2 and 3 hold nothing."""
    n, d = 20_000, 64
    rows = orc.synth_rows(511, 0, n, d, 0)
    qs = orc.synth_rows(512, 0, 3, d, 0)
    codes = orc.bq_encode_rows(rows)
    with Multi([0, 0, 0, 0]) as m:
        mc = MultiCorpus(m, KIND_BQ, METRIC_L2, d, 100_000)
        try:
            assert mc.shard(1)[2] == 25_024
            load_reversed(mc, n, rows)
            for R in (200, 300):
                want = [orc.bq_heap_pops(codes, orc.bq_encode(q), R) for q in qs]
                assert_pops(multi_search_bq_candidates(mc, qs, R), want, 3)
        finally:
            mc.destroy()


# ---- the rescore ------------------------------------------------------------------


def rescore_case(ctx, orc, devices, metric, d, n, rows, qs, k, windows):
    """multi rescore == oracle == one plain corpus, per query and as a batch, for every R of `windows`."""
    ids = np.arange(n, dtype=np.uint64)
    f = Corpus(ctx, KIND_F32, metric, d, n)
    b = Corpus(ctx, KIND_BQ, metric, d, n)
    try:
        f.upsert(ids, rows)
        b.upsert(ids, rows)
        srows = stored(orc, metric, rows)
        with Multi(devices) as m:
            mb = MultiCorpus(m, KIND_BQ, metric, d, n)
            mf = MultiCorpus(m, KIND_F32, metric, d, n)
            try:
                load_reversed(mb, n, rows)
                load_reversed(mf, n, rows)
                for R in windows:
                    ref = [orc.flat_search_bq(srows, prep(orc, metric, q), k, R, ORC_METRIC[metric]) for q in qs]
                    pi, pd, pc = search_bq_rescore(b, f, qs, k, R)
                    for batch in (False, True):
                        got = [multi_search_bq_rescore(mb, mf, q, k, R) for q in ([qs] if batch else list(qs))]
                        gi = np.concatenate([g[0] for g in got])
                        gd = np.concatenate([g[1] for g in got])
                        gc = np.concatenate([g[2] for g in got])
                        assert np.array_equal(gc, pc)
                        assert np.array_equal(gi, pi) and np.array_equal(bits(gd), bits(pd)), (R, batch)
                        for qi in range(len(qs)):
                            ri, rd = ref[qi]
                            assert gc[qi] == len(ri)
                            assert np.array_equal(gi[qi][:gc[qi]], ri), (R, batch, qi, gi[qi], ri)
                            assert np.array_equal(bits(gd[qi][:gc[qi]]), bits(rd)), (R, batch, qi)
            finally:
                mb.destroy()
                mf.destroy()
    finally:
        f.destroy()
        b.destroy()


@pytest.mark.parametrize("devices", DEVICES)
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT, METRIC_COSINE])
@pytest.mark.parametrize("d,n", [(256, 6000), (64, 20000)])
def test_rescore_equals_reference(ctx, orc, devices, metric, d, n):
    rows = orc.synth_rows(55 + d, 0, n, d, 0)
    qs = orc.synth_rows(56 + d, 0, 3, d, 0)
    rescore_case(ctx, orc, devices, metric, d, n, rows, qs, 10, (200,))


@pytest.mark.parametrize("devices", DEVICES)
@pytest.mark.parametrize("metric", [METRIC_L2, METRIC_DOT])
def test_rescore_integer_rows_ties_in_both_heaps(ctx, orc, devices, metric):
    """Integer rows at d = 32 with rows 5000:5100 duplicated: the R-heap and the
    k-heap both tie at their boundary; R = 600 is the select-based superset."""
    n, d = 30_000, 32
    rows = orc.synth_rows(601, 0, n, d, 1) - np.float32(128)
    qs = orc.synth_rows(602, 0, 4, d, 1) - np.float32(128)
    rows[5000:5100] = rows[17]
    qs[3] = rows[17]  # its 100 copies tie at distance 0 / -|x|^2
    rescore_case(ctx, orc, devices, metric, d, n, rows, qs, 10, (200, 600))


# ---- falling distances across slabs -------------------------------------------------


def test_falling_distances_across_two_slabs(orc):
    """Distances falling with the docID (1536 - id mod 1500 set bits against an
    all-zero query code) over two slabs of 200,000 rows: every row beats its
    wave's running R-th, and in slab 1 the cross-slab bound X_1 cuts nearly all
    of them.  Codes go in through the shard handles.

    Measured once with the tools build (tools/bench_multi_bq.py --falling,
    profiles/r08/multi_bq/falling.json): at slabs of 200,000 rows the per-wave
    buffers do NOT overflow -- 0 reruns for every R, one query or two -- so this
    test does not reach the rerun; it pins the bounded filter on an adversarial
    order.  Rows replayed per query with / without the bound: R = 1: 1,500 /
    2,500; R = 4: 1,505 / 2,510; R = 200: 2,652 / 4,538; R = 600 (the select
    path, no bound): 11,243 either way.
    """
    n, d = 400_000, 1536
    w = d // 64
    nb = (1536 - (np.arange(n) % 1500)).astype(np.int64)
    codes = np.zeros((n, w), np.uint64)
    for j in range(w):
        c = np.clip(nb - 64 * j, 0, 64)
        codes[:, j] = np.where(c >= 64, NONE,
                               (np.left_shift(np.uint64(1), np.minimum(c, 63).astype(np.uint64)) - np.uint64(1)))
    lib = _lib.load()
    q = np.ones((2, d), np.float32)  # code 0: distance = set bits
    ham = nb.astype(np.float32)
    with Multi([0, 0]) as m:
        mc = MultiCorpus(m, KIND_BQ, METRIC_L2, d, n)
        try:
            for i in range(2):
                h, base, slab = mc.shard(i)
                ids = np.arange(base, min(n, base + slab), dtype=np.uint64)
                part = np.ascontiguousarray(codes[base:base + slab])
                _lib.check(lib.wvg_corpus_upsert_codes(h, _lib.u64ptr(ids), part.ctypes.data_as(ctypes.c_void_p),
                                                       len(ids)))
            for R in (1, 4, 200, 600):
                want = orc.heap_pops(ham, R)
                assert_pops(multi_search_bq_candidates(mc, q, R), [want, want], 2)
                assert_pops(multi_search_bq_candidates(mc, q[:1], R), [want], 1)
        finally:
            mc.destroy()


# ---- concurrency and errors ---------------------------------------------------------


def test_four_threads_equal_serial_calls(orc):
    n, d, k, R = 20_000, 64, 10, 200
    rows = orc.synth_rows(701, 0, n, d, 0)
    qs = orc.synth_rows(702, 0, 4, d, 0)
    with Multi([0, 0, 0]) as m:
        mb = MultiCorpus(m, KIND_BQ, METRIC_L2, d, n)
        mf = MultiCorpus(m, KIND_F32, METRIC_L2, d, n)
        try:
            load_reversed(mb, n, rows)
            load_reversed(mf, n, rows)
            serial = [multi_search_bq_rescore(mb, mf, qs[i], k, R) for i in range(4)]
            out, errs = [None] * 4, []
            gate = threading.Barrier(4)

            def run(i):
                try:
                    gate.wait()
                    out[i] = multi_search_bq_rescore(mb, mf, qs[i], k, R)
                except Exception as e:  # noqa: BLE001 (reported below)
                    errs.append(e)

            th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            assert not errs, errs
            for i in range(4):
                assert np.array_equal(out[i][2], serial[i][2])
                assert np.array_equal(out[i][0], serial[i][0])
                assert np.array_equal(bits(out[i][1]), bits(serial[i][1]))
            ri, rd = orc.flat_search_bq(rows, qs[0], k, R, 0)
            assert np.array_equal(serial[0][0][0], ri) and np.array_equal(bits(serial[0][1][0]), bits(rd))
        finally:
            mb.destroy()
            mf.destroy()


def test_errors(orc):
    n, d = 4096, 64
    q = orc.synth_rows(801, 0, 1, d, 0)
    with Multi([0, 0]) as m, Multi([0, 0]) as m2:
        mb = MultiCorpus(m, KIND_BQ, METRIC_L2, d, n)
        made = [mb]
        try:
            def other(mm, kind, metric, dd, nn):
                made.append(MultiCorpus(mm, kind, metric, dd, nn))
                return made[-1]

            bad = [(mb, other(m, KIND_F32, METRIC_L2, d, 2 * n)),      # another slab
                   (mb, other(m, KIND_F32, METRIC_L2, 2 * d, n)),      # another dim
                   (mb, other(m, KIND_F32, METRIC_DOT, d, n)),         # another metric
                   (mb, other(m, KIND_BQ, METRIC_L2, d, n)),           # not an F32 corpus
                   (other(m, KIND_F32, METRIC_L2, d, n), made[-1]),    # not a BQ corpus
                   (mb, other(m2, KIND_F32, METRIC_L2, d, n))]         # another multi handle
            for b, f in bad:
                with pytest.raises(WvgError) as e:
                    multi_search_bq_rescore(b, f, q, 10, 200)
                assert e.value.code == WVG_ERR_INVALID
            with pytest.raises(WvgError) as e:
                multi_search_bq_candidates(made[5], q, 200)
            assert e.value.code == WVG_ERR_INVALID
            # an empty corpus, an empty allow list, k = 0: empty results, as the single-device calls
            good = made[5]
            ids, dists, counts = multi_search_bq_rescore(mb, good, q, 10, 200)
            assert counts[0] == 0 and np.all(ids == NONE)
            ids, dists, counts = multi_search_bq_candidates(mb, q, 200, np.zeros(n // 64, np.uint64))
            assert counts[0] == 0 and np.all(ids == NONE) and np.all(np.isposinf(dists))
            assert multi_search_bq_rescore(mb, good, q, 0, 200)[2][0] == 0
        finally:
            for c in made:
                c.destroy()
    with Multi([0, 0], heap_replay=0) as m0:
        mb = MultiCorpus(m0, KIND_BQ, METRIC_L2, d, n)
        mf = MultiCorpus(m0, KIND_F32, METRIC_L2, d, n)
        try:
            for call in (lambda: multi_search_bq_candidates(mb, q, 200),
                         lambda: multi_search_bq_rescore(mb, mf, q, 10, 200)):
                with pytest.raises(WvgError) as e:
                    call()
                assert e.value.code == WVG_ERR_UNSUPPORTED
                assert "heap_replay" in str(e.value)
        finally:
            mb.destroy()
            mf.destroy()

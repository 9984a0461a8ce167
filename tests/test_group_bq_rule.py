"""CPU check of the grouped BQ flow's filter rule (bq_group_filter_kernel,
wvg_group_bq.hip; DESIGN.md section 5 "Grouped BQ search over tenants").

The heap of R inserts row i iff fewer than R live rows precede it or d_i < T_i
(T_i = the R-th smallest distance of the earlier live rows).  The filter walks a
query's rows in chunks of 256 and keeps the live rows with d_i < T, T taken at
the chunk's start: an upper bound of every T_i of the chunk.
weaviate_amd.flat.group_bq_kept_rows restates that in numpy; the oracle's heap
replayed over its rows only must pop what it pops over all rows, every row the
heap inserts must be kept, and with chunks of one row the kept rows are exactly
the inserted ones.
"""
import numpy as np
import pytest

from weaviate_amd.flat import group_bq_kept_rows


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def inserted_rows(d, valid, R):
    """Which rows flat.insertToHeap (V/flat/index.go:497-506) inserts, from its definition:
    fewer than R live rows before it, or a distance strictly below the R-th smallest of them."""
    import heapq

    ins = np.zeros(len(d), bool)
    top = []  # max-heap of the R smallest so far (negated)
    for i in range(len(d)):
        if not valid[i]:
            continue
        if len(top) < R:
            heapq.heappush(top, -float(d[i]))
            ins[i] = True
        elif -top[0] > d[i]:
            heapq.heapreplace(top, -float(d[i]))
            ins[i] = True
    return ins


def _case(rng, kind, n):
    if kind == "ties":  # a handful of distinct values: hundreds of rows tie at every R-th distance
        d = rng.integers(20, 28, n)
    elif kind == "binomial":  # Hamming distances of random codes at d = 64
        d = rng.binomial(64, 0.5, n)
    elif kind == "falling":  # every row beats the running R-th: everything is inserted
        d = 1000 - (np.arange(n) * 1000) // n
    else:  # "sawtooth": falling inside windows that straddle the chunk borders
        d = 300 - np.arange(n) % 257
    return d.astype(np.float32)


@pytest.mark.parametrize("kind", ["ties", "binomial", "falling", "sawtooth"])
def test_kept_rows_reproduce_the_heap(orc, kind):
    rng = np.random.default_rng({"ties": 21, "binomial": 22, "falling": 23, "sawtooth": 24}[kind])
    ncases = 0
    for R in (1, 7, 64, 200, 300, 3000):  # 3000: above every row count below
        n = int(rng.integers(700, 2600))
        d = _case(rng, kind, n)
        for mask in ("all", "sparse", "first_chunks_nearly_empty"):
            v = np.ones(n, np.uint8)
            if mask == "sparse":
                v = (rng.random(n) < 0.15).astype(np.uint8)
            elif mask == "first_chunks_nearly_empty":  # fewer than R live rows ahead of the later chunks
                v[:600] = 0
                v[rng.choice(600, min(R // 4 + 1, 50), replace=False)] = 1
            fi, fd = orc.heap_pops(d, R, v)
            ins = inserted_rows(d, v, R)
            for chunk in (256, 64, 1):
                keep = group_bq_kept_rows(d, v, R, chunk)
                assert not np.any(keep & (v == 0))
                assert not np.any(ins & ~keep), (kind, R, mask, chunk)  # a superset of the inserted rows
                if chunk == 1:
                    assert np.array_equal(keep, ins), (kind, R, mask)
                ki, kd = orc.heap_pops(d, R, keep.astype(np.uint8))
                assert np.array_equal(fi, ki), (kind, R, mask, chunk)
                assert np.array_equal(bits(fd), bits(kd))
                ncases += 1
    assert ncases == 54


def test_rule_is_strict_and_inf_below_r_rows():
    d = np.array([5, 5, 5, 5, 4, 5, 3, 5], np.float32)
    # chunks of 4 rows, R = 4: T of chunk 1 = 5, so it keeps only d < 5
    assert group_bq_kept_rows(d, None, 4, 4).tolist() == [True] * 4 + [True, False, True, False]
    # one row of chunk 0 deleted: 3 < R rows precede chunk 1, T = +inf, every live row is kept
    v = np.array([1, 0, 1, 1, 1, 1, 1, 1], np.uint8)
    assert group_bq_kept_rows(d, v, 4, 4).tolist() == [True, False, True, True] + [True] * 4
    # chunks of 2: three live rows precede the third chunk (T = +inf); five precede the fourth, T = 5
    assert group_bq_kept_rows(d, v, 4, 2).tolist() == [True, False, True, True, True, True, True, False]
    # the default chunk is the kernel's 256 rows
    assert group_bq_kept_rows(np.zeros(300, np.float32), None, 1).tolist() == [True] * 256 + [False] * 44

"""CPU checks of the multi-GPU BQ flow (wvg_multi_search_bq_*, wvg_multi.hip).

Rule R: the heap of R inserts row i iff fewer than R live allowed rows precede
it or d_i < T_i (T_i = the R-th smallest distance of the earlier live allowed
rows); slab s keeps the rows with d_i < min(thr[g], X_s), both upper bounds of
T_i.  weaviate_amd.flat.multi_bq_kept_rows restates that in numpy; replaying
only its rows through the oracle's heap must give the full corpus's pops, ids
and distance bits, on inputs built to tie.  Then what can be read without a
GPU: the new kernels use no scratch, and the Go methods guard the query slice
before the first cgo call.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from weaviate_amd.flat import multi_bq_kept_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _case(rng, kind, n, nslabs):
    """(distances, valid) of one tied input; distances are small integers like Hamming's."""
    if kind == "ties":  # a handful of distinct values: hundreds of rows tie at every R-th distance
        d = rng.integers(20, 28, n)
    elif kind == "binomial":
        d = rng.binomial(64, 0.5, n)
    elif kind == "falling":  # every row beats the running R-th: the filters keep (nearly) everything
        d = 1000 - (np.arange(n) * 1000) // n
    else:  # "sawtooth": falling inside windows that straddle the slab borders
        d = 300 - np.arange(n) % 257
    valid = np.ones(n, np.uint8)
    return d.astype(np.float32), valid


@pytest.mark.parametrize("kind", ["ties", "binomial", "falling", "sawtooth"])
def test_rule_r_kept_rows_reproduce_the_heap(orc, kind):
    rng = np.random.default_rng({"ties": 11, "binomial": 12, "falling": 13, "sawtooth": 14}[kind])
    ncases = 0
    for nslabs in (1, 2, 3, 4):
        for R in (1, 7, 64, 200):
            n = int(rng.integers(900, 2600))
            slab = ((n + nslabs - 1) // nslabs + 63) // 64 * 64
            d, valid = _case(rng, kind, n, nslabs)
            for mask in ("all", "sparse", "slab0_nearly_empty"):
                v = valid.copy()
                if mask == "sparse":
                    v = (rng.random(n) < 0.15).astype(np.uint8)
                elif mask == "slab0_nearly_empty":
                    v[:slab] = 0
                    v[rng.choice(min(slab, n), min(R // 4 + 1, 50), replace=False)] = 1
                for range_rows in (64, 320):
                    keep = multi_bq_kept_rows(d, v, R, slab, range_rows)
                    assert not np.any(keep & (v == 0))
                    fi, fd = orc.heap_pops(d, R, v)
                    ki, kd = orc.heap_pops(d, R, keep.astype(np.uint8))
                    assert np.array_equal(fi, ki), (kind, nslabs, R, mask, range_rows)
                    assert np.array_equal(bits(fd), bits(kd))
                    ncases += 1
    assert ncases == 96


def test_rule_r_strict_less_and_inf_below_r_rows():
    """X_s is +inf while fewer than R live rows precede the slab; the test is strict."""
    d = np.array([5, 5, 5, 5, 4, 5, 3, 5], np.float32)
    # slab = 4 rows, R = 4: X_1 = 5, so slab 1 keeps only d < 5
    assert multi_bq_kept_rows(d, None, 4, 4, 4).tolist() == [True] * 4 + [True, False, True, False]
    # one row of slab 0 deleted: 3 < R rows precede slab 1, X_1 = +inf, everything of range 0 is kept
    v = np.array([1, 0, 1, 1, 1, 1, 1, 1], np.uint8)
    assert multi_bq_kept_rows(d, v, 4, 4, 4).tolist() == [True, False, True, True] + [True] * 4
    # ranges of 2 rows: thr of slab 1's second range is +inf too (2 < R rows of the slab precede it)
    assert multi_bq_kept_rows(d, v, 4, 4, 2).tolist() == [True, False, True, True] + [True] * 4


def _gfx950_code_objects(path):
    import struct

    data = open(path, "rb").read()
    out, i = [], data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    while i >= 0:
        n = struct.unpack_from("<Q", data, i + 24)[0]
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + tl]
            p += tl
            if b"gfx950" in triple and size:
                out.append(data[i + off:i + off + size])
        i = data.find(b"__CLANG_OFFLOAD_BUNDLE__", i + 24)
    return out


def test_cross_slab_kernels_use_no_scratch(tmp_path):
    """slab_hist_kernel, slab_bound_kernel and the filter with its bound argument:
    private_segment_fixed_size = 0 in the gfx950 code objects of libwvgpu.so."""
    from weaviate_amd import _lib

    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not available")
    want = ("slab_hist_kernel", "slab_bound_kernel", "emit_filter_kernel")
    seen, bad = set(), []
    for j, co in enumerate(_gfx950_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"co{j}.o"
        f.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(f)], capture_output=True, text=True).stdout
        name = None
        for ln in notes.splitlines():
            ln = ln.strip()
            if ln.startswith(".name:"):
                name = ln.split(":", 1)[1].strip()
            elif ln.startswith(".private_segment_fixed_size:") and name:
                for w in want:
                    if w in name:
                        seen.add(w)
                        if int(ln.split(":", 1)[1]) != 0:
                            bad.append(name)
    assert seen == set(want), seen
    assert not bad, bad


def test_go_multi_methods_guard_the_query_slice():
    """MultiCorpus.SearchBatch, SearchBQRescore and SearchBQCandidates check
    len(qs) == nq * dims before the first C. call (a short slice is an
    out-of-bounds host read in the library)."""
    src = open(os.path.join(ROOT, "go", "gpu", "wvgpu.go")).read()
    src = re.sub(r"//[^\n]*", "", src)
    calls = {"SearchBatch": "wvg_multi_search", "SearchBQRescore": "wvg_multi_search_bq_rescore",
             "SearchBQCandidates": "wvg_multi_search_bq_candidates"}
    for fn, sym in calls.items():
        m = re.search(r"func \(x \*MultiCorpus\) %s\(([^)]*)\)[^{]*\{" % fn, src)
        assert m, fn
        assert "helpers.AllowList" in m.group(1)
        body = src[m.end():src.index("\n}\n", m.end())]
        guard = re.search(r"if len\(qs\) != nq\*x\.dims \{\s*return nil, ", body)
        first = body.find("C.")
        assert guard and 0 <= guard.start() < first, fn
        assert body[first:].startswith("C.%s(" % sym), fn

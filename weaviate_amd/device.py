"""Device context and device-resident corpora (handles of the C ABI).

One :class:`Context` per GPU.  Several GPUs serve one index either from one
process (:class:`Multi` / :class:`MultiCorpus`: wvg_multi_*, RCCL inside the
library) or with one process per GPU (weaviate_amd/shard.py, RCCL through
torch.distributed).
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_int, c_uint32, c_uint64, c_void_p

import numpy as np

from . import _lib
from ._lib import BatchPlan, StreamPlan, check, fptr, u32ptr, u64ptr


def device_count() -> int:
    lib = _lib.load()
    n = c_int(0)
    check(lib.wvg_device_count(byref(n)))
    return n.value


class Context:
    """wvg_open_ex / wvg_close.  Keyword options set the fields of
    wvg_options (mfma_min_queries, cache_reuse, merge_wait_us, batch_screen);
    the others keep wvg_options_default's values."""

    def __init__(self, device: int = 0, **options):
        self.lib = _lib.load()
        opts = _lib.Options()
        self.lib.wvg_options_default(byref(opts))
        for name, value in options.items():
            if name == "size" or name not in dict(_lib.Options._fields_):
                raise TypeError(f"unknown context option {name!r}")
            setattr(opts, name, int(value))
        h = c_void_p()
        check(self.lib.wvg_open_ex(device, byref(opts), byref(h)))
        self.handle = h
        self.device = device
        self.options = {name: getattr(opts, name) for name, _ in _lib.Options._fields_ if name != "size"}

    def close(self) -> None:
        if self.handle:
            self.lib.wvg_close(self.handle)
            self.handle = c_void_p()

    def synchronize(self) -> None:
        check(self.lib.wvg_synchronize(self.handle))

    def host_array(self, shape, dtype=np.float32):
        """wvg_host_alloc: a numpy array over page-locked host memory, which the
        entry points copy from / to without a staging copy; freed with
        free_host_array (the array must not be used afterwards)."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        p = c_void_p()
        check(self.lib.wvg_host_alloc(self.handle, max(n, 1), byref(p)))
        buf = (ctypes.c_uint8 * max(n, 1)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.uint8, count=n).view(dt).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def free_host_array(self, arr) -> None:
        p = self._pinned.pop(arr.ctypes.data)
        check(self.lib.wvg_host_free(self.handle, p))

    def set_distance_order(self, order: int) -> None:
        """wvg_set_distance_order: _lib.ORDER_AVX256 (default) or ORDER_AVX512
        (the kernels Weaviate dispatches on AMX + AVX-512 hosts)."""
        check(self.lib.wvg_set_distance_order(self.handle, order))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def allow_bitmap(ids, n_bits: int | None = None) -> np.ndarray:
    """helpers.AllowList -> bitmap over global docIDs (bit i of word i/64)."""
    ids = np.asarray(list(ids), dtype=np.uint64)
    top = int(ids.max()) + 1 if ids.size else 0
    n_bits = max(n_bits or 0, top)
    words = np.zeros((n_bits + 63) // 64, dtype=np.uint64)
    if ids.size:
        np.bitwise_or.at(words, (ids >> np.uint64(6)).astype(np.int64),
                         np.left_shift(np.uint64(1), ids & np.uint64(63)))
    return words


def allow_window(id_lists, first_id: int, stride: int) -> np.ndarray:
    """Per-query allow lists -> the [nq][stride] window wvg_search_device_pipelined_filtered reads: bit b of
    word w of row q = docID first_id + 64 w + b (first_id a multiple of 64); ids outside the window are dropped."""
    if first_id % 64:
        raise ValueError("first_id must be a multiple of 64")
    out = np.zeros((len(id_lists), stride), dtype=np.uint64)
    for q, ids in enumerate(id_lists):
        ids = np.asarray(list(ids), dtype=np.uint64)
        ids = ids[(ids >= np.uint64(first_id)) & (ids < np.uint64(first_id + 64 * stride))] - np.uint64(first_id)
        np.bitwise_or.at(out[q], (ids >> np.uint64(6)).astype(np.int64), np.left_shift(np.uint64(1), ids & np.uint64(63)))
    return out


class Corpus:
    """A device-resident corpus (wvg_corpus_*): F32 rows, BQ codes or PQ codes."""

    def __init__(self, ctx: Context, kind: int, metric: int, dim: int, capacity: int, id_base: int = 0):
        self.ctx = ctx
        self.lib = ctx.lib
        self.kind, self.metric, self.dim, self.id_base = kind, metric, dim, id_base
        h = c_void_p()
        check(self.lib.wvg_corpus_create(ctx.handle, kind, metric, dim, id_base, capacity, byref(h)))
        self.handle = h

    def destroy(self) -> None:
        if self.handle:
            self.lib.wvg_corpus_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def info(self):
        cnt, hw, cap = c_uint64(), c_uint64(), c_uint64()
        check(self.lib.wvg_corpus_info(self.handle, byref(cnt), byref(hw), byref(cap)))
        return cnt.value, hw.value, cap.value

    def reserve(self, capacity: int) -> None:
        check(self.lib.wvg_corpus_reserve(self.handle, capacity))

    def upsert(self, ids, vectors) -> None:
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        vectors = np.ascontiguousarray(vectors, dtype=np.float32)
        if vectors.ndim == 1:
            vectors = vectors[None, :]
        check(self.lib.wvg_corpus_upsert(self.handle, u64ptr(ids), fptr(vectors), len(ids),
                                         vectors.shape[1] if vectors.size else self.dim))

    def upsert_codes(self, ids, codes) -> None:
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        codes = np.ascontiguousarray(codes)
        check(self.lib.wvg_corpus_upsert_codes(self.handle, u64ptr(ids), codes.ctypes.data_as(c_void_p), len(ids)))

    def load_kv(self, keys, values) -> None:
        """wvg_corpus_load_kv: an LSM cursor's (8-byte big-endian key, LE row) pairs."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 8)
        values = np.ascontiguousarray(values, dtype=np.uint8).reshape(len(keys), -1)
        check(self.lib.wvg_corpus_load_kv(self.handle, keys.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                          values.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(keys),
                                          values.shape[1]))

    def distance_by_ids(self, query, ids):
        """wvg_corpus_distance_by_ids: (dists, ok) of the query to the rows with these docIDs."""
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1)
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        out = np.empty(len(ids), dtype=np.float32)
        ok = np.empty(len(ids), dtype=np.uint8)
        check(self.lib.wvg_corpus_distance_by_ids(self.handle, fptr(q), u64ptr(ids), len(ids), fptr(out),
                                                  ok.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out, ok.astype(bool)

    def distance_by_ids_batch(self, queries, id_lists):
        """wvg_corpus_distance_by_ids_batch: one launch for many queries' id lists;
        returns [(dists, ok)] per query."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(len(id_lists), -1)
        lists = [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1) for x in id_lists]
        offsets = np.zeros(len(lists) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(x) for x in lists])
        ids = np.concatenate(lists) if lists else np.empty(0, np.uint64)
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        out = np.empty(len(ids), dtype=np.float32)
        ok = np.empty(len(ids), dtype=np.uint8)
        check(self.lib.wvg_corpus_distance_by_ids_batch(self.handle, fptr(q), len(lists), u64ptr(offsets), u64ptr(ids),
                                                        fptr(out), ok.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        res = []
        for i in range(len(lists)):
            a, b = int(offsets[i]), int(offsets[i + 1])
            res.append((out[a:b], ok[a:b].astype(bool)))
        return res

    def delete(self, ids) -> None:
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        check(self.lib.wvg_corpus_delete(self.handle, u64ptr(ids), len(ids)))

    def get(self, id_: int, pq_m: int = 0) -> np.ndarray:
        if self.kind == _lib.KIND_F32:
            out = np.empty(self.dim, dtype=np.float32)
        elif self.kind == _lib.KIND_BQ:
            out = np.empty((self.dim + 63) // 64, dtype=np.uint64)
        else:
            out = np.empty(pq_m, dtype=np.uint8)
        check(self.lib.wvg_corpus_get(self.handle, id_, out.ctypes.data_as(c_void_p)))
        return out

    def get_batch(self, ids, pq_m: int = 0):
        """wvg_corpus_get_batch: (rows [n][...], ok [n]) for many docIDs in one call."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        n = len(ids)
        if self.kind == _lib.KIND_F32:
            out = np.empty((n, self.dim), dtype=np.float32)
        elif self.kind == _lib.KIND_BQ:
            out = np.empty((n, (self.dim + 63) // 64), dtype=np.uint64)
        else:
            out = np.empty((n, pq_m), dtype=np.uint8)
        ok = np.empty(n, dtype=np.uint8)
        check(self.lib.wvg_corpus_get_batch(self.handle, u64ptr(ids), n, out.ctypes.data_as(c_void_p),
                                            ok.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out, ok.astype(bool)

    def fill_synthetic(self, seed: int, n: int, distribution: int = 0) -> None:
        check(self.lib.wvg_corpus_fill_synthetic(self.handle, seed, n, distribution))

    def set_codebook(self, centers) -> None:
        centers = np.ascontiguousarray(centers, dtype=np.float32)
        m, ks, _ = centers.shape
        check(self.lib.wvg_pq_set_codebook(self.handle, fptr(centers), m, ks))

    def search(self, queries, k: int, allow=None):
        """wvg_search: returns (ids [nq][k], dists [nq][k], counts [nq])."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        ids = np.empty((nq, k), dtype=np.uint64)
        dists = np.empty((nq, k), dtype=np.float32)
        counts = np.empty(nq, dtype=np.uint32)
        aw, an = (None, 0) if allow is None else (np.ascontiguousarray(allow, dtype=np.uint64), len(allow))
        check(self.lib.wvg_search(self.handle, fptr(q), nq, k, u64ptr(aw) if aw is not None else None, an,
                                  u64ptr(ids), fptr(dists), u32ptr(counts)))
        return ids, dists, counts

    def search_device_pipelined(self, d_queries: int, nq: int, k: int, d_ids: int, d_dists: int, d_counts: int,
                                d_workspace: int, workspace_bytes: int, stream: int = 0, d_allow: int = 0,
                                allow_stride: int = 0, allow_first_id: int = 0) -> None:
        """wvg_search_device_pipelined on device pointers, asynchronous on `stream`; with d_allow (device
        words [nq][allow_stride], see allow_window) wvg_search_device_pipelined_filtered.  F32, BQ and PQ
        corpora (d_queries: the float rows; a PQ corpus needs its codebook)."""
        if not d_allow:
            check(self.lib.wvg_search_device_pipelined(self.handle, d_queries, nq, k, d_ids, d_dists, d_counts,
                                                       d_workspace, workspace_bytes, stream))
        else:
            check(self.lib.wvg_search_device_pipelined_filtered(self.handle, d_queries, nq, k, d_allow, allow_stride,
                                                                allow_first_id, d_ids, d_dists, d_counts, d_workspace,
                                                                workspace_bytes, stream))

    def search_device_plan(self, nq: int, k: int) -> dict:
        """wvg_search_device_pipelined_plan: what search_device_pipelined(nq, k) will do on this corpus --
        {shared_rows, queries_per_pass, passes, seeded, screened} (struct wvg_stream_plan).  Host only."""
        sp = StreamPlan()
        check(self.lib.wvg_search_device_pipelined_plan(self.handle, nq, k, byref(sp)))
        return {name: int(getattr(sp, name)) for name, _ in StreamPlan._fields_}

    def search_device_shadow(self, nq: int, k: int) -> dict:
        """wvg_search_device_pipelined_shadow: {reads_shadow, shadow_bytes_per_row} -- whether the next
        search_device_pipelined(nq, k) outside a stream capture reads the corpus's bf16 shadow, and what the
        first such call allocates per row of capacity (it also builds the shadow: one pass over the rows).
        Host only."""
        rs, bpr = c_uint32(), c_uint32()
        check(self.lib.wvg_search_device_pipelined_shadow(self.handle, nq, k, byref(rs), byref(bpr)))
        return {"reads_shadow": int(rs.value), "shadow_bytes_per_row": int(bpr.value)}

    def batch_plan(self, nq: int, k: int, allow: bool = False) -> dict:
        """wvg_search_batch_plan: the route a batch of nq queries takes on this corpus -- {matrix, screen,
        shadow_bytes_per_row} (struct wvg_batch_plan; allow: the batch shares one allow list).  Host only."""
        bp = BatchPlan()
        check(self.lib.wvg_search_batch_plan(self.handle, nq, k, 1 if allow else 0, byref(bp)))
        return {name: int(getattr(bp, name)) for name, _ in BatchPlan._fields_ if name != "reserved"}

    def search_by_distance(self, query, target: float, max_limit: int = -1, allow=None, capacity: int | None = None):
        """wvg_search_by_distance: (ids, dists) of every row within `target`
        (flat.SearchByVectorDistance, V/flat/index.go:531-591)."""
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1)
        aw, an = (None, 0) if allow is None else (np.ascontiguousarray(allow, dtype=np.uint64), len(allow))
        cnt = c_uint64()
        cap = capacity if capacity is not None else max(1, self.info()[1])
        while True:
            ids = np.empty(cap, dtype=np.uint64)
            dists = np.empty(cap, dtype=np.float32)
            check(self.lib.wvg_search_by_distance(self.handle, fptr(q), float(target), int(max_limit),
                                                  u64ptr(aw) if aw is not None else None, an, u64ptr(ids),
                                                  fptr(dists), cap, byref(cnt)))
            if cnt.value <= cap:
                return ids[:cnt.value], dists[:cnt.value]
            cap = cnt.value

    def search_by_distance_window(self, query, target: float, window: int = 100, allow=None):
        """wvg_search_by_distance_window: the flat index's own range-search
        result (its first window, V/flat/index.go:531-591 as written)."""
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1)
        aw, an = (None, 0) if allow is None else (np.ascontiguousarray(allow, dtype=np.uint64), len(allow))
        cnt = c_uint64()
        ids = np.empty(max(1, window), dtype=np.uint64)
        dists = np.empty(max(1, window), dtype=np.float32)
        check(self.lib.wvg_search_by_distance_window(self.handle, fptr(q), float(target), int(window),
                                                     u64ptr(aw) if aw is not None else None, an, u64ptr(ids),
                                                     fptr(dists), len(ids), byref(cnt)))
        return ids[:cnt.value], dists[:cnt.value]


def _group_allows(allows, nq):
    """The per-query allow tables of the grouped calls: (pointer table, word counts,
    the arrays to keep alive), or (None, None, []) for allows = None.  An empty array
    is a non-NULL pointer with 0 words: nothing allowed for that query."""
    if allows is None:
        return None, None, []
    ap = (c_void_p * max(nq, 1))()
    aw = np.zeros(max(nq, 1), dtype=np.uint64)
    keep = []
    for i, a in enumerate(allows):
        if a is None:
            continue
        words = np.ascontiguousarray(a, dtype=np.uint64)
        if words.size == 0:  # non-NULL with 0 words: nothing allowed
            words = np.zeros(1, dtype=np.uint64)
            aw[i] = 0
        else:
            aw[i] = words.size
        keep.append(words)
        ap[i] = words.ctypes.data
    return ap, aw, keep


def search_group(corpora, queries, k: int, allows=None):
    """wvg_search_group: query i against corpora[i] (the tenants of one class: F32,
    one context, one metric, one dim), all in one scan launch and one merge launch.
    allows: None, or one entry per query -- None (no filter) or a bitmap over that
    corpus's global docIDs (allow_bitmap; an empty array allows nothing).  Returns
    (ids [nq][k], dists [nq][k], counts [nq]), as nq Corpus.search calls would."""
    corpora = list(corpora)
    nq = len(corpora)
    q = np.ascontiguousarray(queries, dtype=np.float32)
    if q.ndim == 1:
        q = q[None, :]
    if q.shape[0] != nq:
        raise ValueError(f"{q.shape[0]} queries for {nq} corpora")
    if allows is not None and len(allows) != nq:
        raise ValueError(f"{len(allows)} allow lists for {nq} corpora")
    lib = _lib.load()
    handles = (c_void_p * max(nq, 1))(*[c.handle if c is not None else None for c in corpora])
    ids = np.empty((nq, k), dtype=np.uint64)
    dists = np.empty((nq, k), dtype=np.float32)
    counts = np.empty(nq, dtype=np.uint32)
    ap, aw, keep = _group_allows(allows, nq)  # keep: the bitmaps, alive through the call
    check(lib.wvg_search_group(handles, fptr(q), nq, k, ap, u64ptr(aw) if aw is not None else None,
                               u64ptr(ids), fptr(dists), u32ptr(counts)))
    return ids, dists, counts


def _group_bq_args(bqs, queries, allows):
    bqs = list(bqs)
    nq = len(bqs)
    q = np.ascontiguousarray(queries, dtype=np.float32)
    if q.ndim == 1:
        q = q[None, :]
    if q.shape[0] != nq:
        raise ValueError(f"{q.shape[0]} queries for {nq} corpora")
    if allows is not None and len(allows) != nq:
        raise ValueError(f"{len(allows)} allow lists for {nq} corpora")
    handles = (c_void_p * max(nq, 1))(*[c.handle if c is not None else None for c in bqs])
    return nq, q, handles, _group_allows(allows, nq)


def search_group_bq_rescore(bqs, f32s, queries, k: int, rescore_limit: int, allows=None):
    """wvg_search_group_bq_rescore: flat.searchByVectorBQ of query i against tenant
    (bqs[i], f32s[i]) -- BQ and F32 corpora of one context, metric and dim -- all in
    three launches.  allows as search_group.  Returns (ids [nq][k], dists [nq][k],
    counts [nq]), as nq search_bq_rescore calls would."""
    f32s = list(f32s)
    nq, q, hb, (ap, aw, keep) = _group_bq_args(bqs, queries, allows)
    if len(f32s) != nq:
        raise ValueError(f"{len(f32s)} F32 corpora for {nq} BQ corpora")
    hf = (c_void_p * max(nq, 1))(*[c.handle if c is not None else None for c in f32s])
    ids = np.empty((nq, k), dtype=np.uint64)
    dists = np.empty((nq, k), dtype=np.float32)
    counts = np.empty(nq, dtype=np.uint32)
    check(_lib.load().wvg_search_group_bq_rescore(hb, hf, fptr(q), nq, k, rescore_limit, ap,
                                                  u64ptr(aw) if aw is not None else None,
                                                  u64ptr(ids), fptr(dists), u32ptr(counts)))
    return ids, dists, counts


def search_group_bq_candidates(bqs, queries, rescore_limit: int, allows=None):
    """wvg_search_group_bq_candidates: per query the heap's candidates in pop order,
    as nq search_bq_candidates calls: (ids [nq][R], dists [nq][R], counts [nq])."""
    nq, q, hb, (ap, aw, keep) = _group_bq_args(bqs, queries, allows)
    R = rescore_limit
    ids = np.empty((nq, R), dtype=np.uint64)
    dists = np.empty((nq, R), dtype=np.float32)
    counts = np.empty(nq, dtype=np.uint32)
    check(_lib.load().wvg_search_group_bq_candidates(hb, fptr(q), nq, R, ap, u64ptr(aw) if aw is not None else None,
                                                     u64ptr(ids), fptr(dists), u32ptr(counts)))
    return ids, dists, counts


def search_bq_candidates(bq: Corpus, queries, rescore_limit: int, allow=None):
    """wvg_search_bq_candidates: findTopVectorsCached's heap of rescore_limit and
    its pop order (V/flat/index.go:355-374): (ids [nq][R], dists [nq][R], counts)."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    if q.ndim == 1:
        q = q[None, :]
    nq, R = q.shape[0], rescore_limit
    ids = np.empty((nq, R), dtype=np.uint64)
    dists = np.empty((nq, R), dtype=np.float32)
    counts = np.empty(nq, dtype=np.uint32)
    aw, an = (None, 0) if allow is None else (np.ascontiguousarray(allow, dtype=np.uint64), len(allow))
    check(bq.lib.wvg_search_bq_candidates(bq.handle, fptr(q), nq, R, u64ptr(aw) if aw is not None else None, an,
                                          u64ptr(ids), fptr(dists), u32ptr(counts)))
    return ids, dists, counts


def search_bq_rescore(bq: Corpus, f32: Corpus, queries, k: int, rescore_limit: int, allow=None):
    q = np.ascontiguousarray(queries, dtype=np.float32)
    if q.ndim == 1:
        q = q[None, :]
    nq = q.shape[0]
    ids = np.empty((nq, k), dtype=np.uint64)
    dists = np.empty((nq, k), dtype=np.float32)
    counts = np.empty(nq, dtype=np.uint32)
    aw, an = (None, 0) if allow is None else (np.ascontiguousarray(allow, dtype=np.uint64), len(allow))
    check(bq.lib.wvg_search_bq_rescore(bq.handle, f32.handle, fptr(q), nq, k, rescore_limit,
                                       u64ptr(aw) if aw is not None else None, an,
                                       u64ptr(ids), fptr(dists), u32ptr(counts)))
    return ids, dists, counts


class Multi:
    """wvg_multi_open / wvg_multi_close: one context per device in this process
    and, for distinct devices, an RCCL communicator per device."""

    def __init__(self, devices, **options):
        self.lib = _lib.load()
        opts = _lib.Options()
        self.lib.wvg_options_default(byref(opts))
        for name, value in options.items():
            if name == "size" or name not in dict(_lib.Options._fields_):
                raise TypeError(f"unknown context option {name!r}")
            setattr(opts, name, int(value))
        devs = (c_int * len(devices))(*devices)
        h = c_void_p()
        check(self.lib.wvg_multi_open(devs, len(devices), byref(opts), byref(h)))
        self.handle = h
        nd, rc = c_int(), c_int()
        check(self.lib.wvg_multi_info(h, byref(nd), byref(rc)))
        self.ndev, self.uses_rccl = nd.value, bool(rc.value)

    def close(self) -> None:
        if self.handle:
            check(self.lib.wvg_multi_close(self.handle))
            self.handle = c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class MultiCorpus:
    """wvg_multi_corpus_*: docIDs dealt to the devices in contiguous slabs;
    search = every slab's scan on its device, one RCCL all-gather, the merge.
    The exact BQ flow over a BQ (+ F32) multi corpus: multi_search_bq_rescore /
    multi_search_bq_candidates below."""

    def __init__(self, multi: Multi, kind: int, metric: int, dim: int, rows: int):
        self.multi, self.lib = multi, multi.lib
        self.kind, self.metric, self.dim = kind, metric, dim
        h = c_void_p()
        check(self.lib.wvg_multi_corpus_create(multi.handle, kind, metric, dim, rows, byref(h)))
        self.handle = h

    def destroy(self) -> None:
        if self.handle:
            check(self.lib.wvg_multi_corpus_destroy(self.handle))
            self.handle = c_void_p()

    def shard(self, i: int):
        """(wvg_corpus handle, id_base, slab rows) of shard i."""
        h, base, slab = c_void_p(), c_uint64(), c_uint64()
        check(self.lib.wvg_multi_corpus_shard(self.handle, i, byref(h), byref(base), byref(slab)))
        return h, base.value, slab.value

    def upsert(self, ids, vectors) -> None:
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        vectors = np.ascontiguousarray(vectors, dtype=np.float32).reshape(len(ids), -1)
        check(self.lib.wvg_multi_corpus_upsert(self.handle, u64ptr(ids), fptr(vectors), len(ids),
                                               vectors.shape[1] if vectors.size else self.dim))

    def delete(self, ids) -> None:
        ids = np.ascontiguousarray(ids, dtype=np.uint64)
        check(self.lib.wvg_multi_corpus_delete(self.handle, u64ptr(ids), len(ids)))

    def fill_synthetic(self, seed: int, n: int, distribution: int = 0) -> None:
        check(self.lib.wvg_multi_corpus_fill_synthetic(self.handle, seed, n, distribution))

    def set_codebook(self, centers) -> None:
        centers = np.ascontiguousarray(centers, dtype=np.float32)
        m, ks, _ = centers.shape
        check(self.lib.wvg_multi_corpus_set_codebook(self.handle, fptr(centers), m, ks))

    def search(self, queries, k: int, allow=None):
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq = q.shape[0]
        ids = np.empty((nq, k), dtype=np.uint64)
        dists = np.empty((nq, k), dtype=np.float32)
        counts = np.empty(nq, dtype=np.uint32)
        aw, an = (None, 0) if allow is None else (np.ascontiguousarray(allow, dtype=np.uint64), len(allow))
        check(self.lib.wvg_multi_search(self.handle, fptr(q), nq, k, u64ptr(aw) if aw is not None else None, an,
                                        u64ptr(ids), fptr(dists), u32ptr(counts)))
        return ids, dists, counts


def multi_search_bq_candidates(bq: MultiCorpus, queries, rescore_limit: int, allow=None):
    """wvg_multi_search_bq_candidates: search_bq_candidates over a BQ multi corpus
    (one heap of rescore_limit over all slabs; ids are global docIDs)."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    if q.ndim == 1:
        q = q[None, :]
    nq, R = q.shape[0], rescore_limit
    ids = np.empty((nq, R), dtype=np.uint64)
    dists = np.empty((nq, R), dtype=np.float32)
    counts = np.empty(nq, dtype=np.uint32)
    aw, an = (None, 0) if allow is None else (np.ascontiguousarray(allow, dtype=np.uint64), len(allow))
    check(bq.lib.wvg_multi_search_bq_candidates(bq.handle, fptr(q), nq, R, u64ptr(aw) if aw is not None else None,
                                                an, u64ptr(ids), fptr(dists), u32ptr(counts)))
    return ids, dists, counts


def multi_search_bq_rescore(bq: MultiCorpus, f32: MultiCorpus, queries, k: int, rescore_limit: int, allow=None):
    """wvg_multi_search_bq_rescore: search_bq_rescore over a BQ and an F32 multi
    corpus of the same Multi (flat.searchByVectorBQ, V/flat/index.go:347-389)."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    if q.ndim == 1:
        q = q[None, :]
    nq = q.shape[0]
    ids = np.empty((nq, k), dtype=np.uint64)
    dists = np.empty((nq, k), dtype=np.float32)
    counts = np.empty(nq, dtype=np.uint32)
    aw, an = (None, 0) if allow is None else (np.ascontiguousarray(allow, dtype=np.uint64), len(allow))
    check(bq.lib.wvg_multi_search_bq_rescore(bq.handle, f32.handle, fptr(q), nq, k, rescore_limit,
                                             u64ptr(aw) if aw is not None else None, an,
                                             u64ptr(ids), fptr(dists), u32ptr(counts)))
    return ids, dists, counts

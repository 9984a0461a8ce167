/*
 * wvgpu.h -- C ABI of the MI355X (gfx950) vector-scoring backend for
 * Weaviate's flat / BQ / PQ hot path.  Go binds it through cgo (see
 * INTEGRATION.md); the test and bench harness binds it through ctypes.
 *
 * Citations are relative to the reference tree (antas-marcin/weaviate):
 *   D/  = adapters/repos/db/vector/hnsw/distancer/
 *   CH/ = adapters/repos/db/vector/compressionhelpers/
 *   V/  = adapters/repos/db/vector/
 *
 * Conventions:
 *  - every function returns WVG_OK (0) or a negative WVG_ERR_*; the message is
 *    available from wvg_last_error() on the calling thread.  Nothing aborts.
 *  - host buffers are borrowed for the duration of the call only and never
 *    retained (cgo pointer rules); device memory belongs to the handles.
 *  - distances are float32, smaller is closer; results are ascending by
 *    (distance, id); ids are uint64 docIDs.
 *  - handles are safe for concurrent searches; upsert/delete/reserve take an
 *    exclusive lock on the corpus.
 */
#ifndef WVGPU_H
#define WVGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: wvg_options gained `coalesce` (round 4) and the device-memory / stream
 * entry points were added (wvg_device_alloc ... wvg_memcpy_d2h).
 * 3: wvg_options gained `heap_replay`; wvg_search_bq_candidates; the
 * multi-GPU handle (wvg_multi_*).  Added since without a version change
 * (purely additive): wvg_multi_search_bq_rescore / _bq_candidates. */
#define WVG_ABI_VERSION 3

#define WVG_OK 0
#define WVG_ERR_INVALID -1       /* bad argument (null, k < 0 analogue, bad kind) */
#define WVG_ERR_DIM_MISMATCH -2  /* "vector lengths don't match" (D/l2.go:47-50) */
#define WVG_ERR_NOMEM -3
#define WVG_ERR_DEVICE -4        /* HIP runtime error */
#define WVG_ERR_NOT_FOUND -5     /* id not present (deleted / never added) */
#define WVG_ERR_UNSUPPORTED -6
#define WVG_ERR_CAPACITY -7      /* id outside [id_base, id_base + capacity) */

/* corpus kinds */
#define WVG_KIND_F32 0 /* float32 rows (flat "vectors" bucket, V/flat/index.go:259-260) */
#define WVG_KIND_BQ 1  /* sign-bit codes (CH/binary_quantization.go:32) */
#define WVG_KIND_PQ 2  /* PQ byte codes (CH/product_quantization.go:420) */

/* metrics: entities/vectorindex/common/config.go:22-31 */
#define WVG_METRIC_L2 0     /* "l2-squared" D/l2.go */
#define WVG_METRIC_DOT 1    /* "dot"        D/dot_product.go */
#define WVG_METRIC_COSINE 2 /* "cosine-dot" D/cosine_dist.go (rows/queries normalized) */
#define WVG_METRIC_MANHATTAN 3 /* "manhattan" D/manhattan.go (pure Go on every host) */
#define WVG_METRIC_HAMMING 4   /* "hamming"   D/hamming.go -> hamming_256 / hamming_512
                                  (D/hamming_amd64.go:18-24); selected by name in
                                  adapters/repos/db/shard.go:406-421 like the others */

typedef struct wvg_ctx wvg_ctx;
typedef struct wvg_corpus wvg_corpus;

/* ---- library / device ---------------------------------------------------- */
int wvg_abi_version(void);
const char *wvg_last_error(void);
int wvg_device_count(int *out);
/* One context per GPU (one process per GPU in the multi-GPU deployment).
 * Environment, read when a context opens: WVG_QSHARE_SCREEN=0 switches off the
 * bf16 screen of wvg_search_device_pipelined's shared-row scan for that context
 * (results are identical either way; the screen only saves time). */
int wvg_open(int device, wvg_ctx **out);
/* Context options, fixed for the life of the context (wvg_open uses the
 * defaults).  Fill with wvg_options_default, change fields, then open.     */
typedef struct wvg_options {
    uint32_t size;             /* sizeof(wvg_options) (ABI guard; set by wvg_options_default) */
    uint32_t mfma_min_queries; /* dot / cosine / l2-squared batches of at least this many queries are scored
                                  on the matrix cores (bf16 / int8 screen + exact fp32 rescore, or -- dot /
                                  cosine only -- exact fp32 MFMA); smaller ones run one HBM-bound scan per
                                  query.  0 = never.  Default 32. */
    int32_t cache_reuse;       /* 1 (default): consecutive scans of a corpus alternate direction and read
                                  the last ~320 MB of each pass with the default cache policy, so the next
                                  scan starts on rows still in the 256 MiB Infinity Cache; the queries of a
                                  wvg_search_device_pipelined call share each row read.  0: streaming --
                                  one direction, non-temporal loads, no reuse between scans: one full scan
                                  per query (e.g. next to other memory-heavy work, or to measure the
                                  DRAM-bound rate). */
    uint32_t merge_wait_us;    /* bound on the in-launch merge's wait for one query's scan workgroups
                                  (wvg_search_device_pipelined); 0 = the default, 4 s.  On expiry the
                                  query gets empty results and wvg_search_device_check fails. */
    int32_t batch_screen;      /* 2 (default): batched dot / cosine searches screen every row with int8
                                  MFMA (d = 512 / 768 / 1024; other d: bf16) and a per-row error bound,
                                  then rescore the candidates exactly in fp32 (results identical to the
                                  exact path); 1: the bf16 screen for every d; 0: exact fp32 MFMA only.
                                  l2-squared batches (d % 32 == 0, k <= 16): 1 and 2 both mean the bf16
                                  screen (shadow: 2 * dim + 4 bytes per row, at the first screened
                                  batch); 0: the co-scheduled per-query scans, as batches of fewer than
                                  mfma_min_queries.
                                  The first screened search of a corpus allocates its shadow: int8 = dim
                                  + 8 bytes per row of capacity (7.7 GB at 10M x 768; its first build
                                  also takes one pass over the rows for the corpus scale and one host
                                  wait), bf16 = 2 * dim + 4 bytes per row (15.4 GB), kept until the
                                  corpus is destroyed or grows. */
    int32_t coalesce;          /* 1 (default): concurrent single-query wvg_search calls on one corpus
                                  join one batched launch -- while a batch runs, the calls that arrive
                                  queue up and the next batch takes them all (filtered calls, each with its
                                  own allow list, in batches of their own; any mix of k, run at the
                                  largest); right after a batch of 4 or more the next one waits a short window
                                  (at most a quarter of that batch's run time) for the callers just answered; each
                                  caller gets exactly its own results (identical to a call of its own); a
                                  lone call does not wait.  0: every call launches on its own. */
    int32_t heap_replay;       /* 1 (default): wvg_search_bq_rescore / wvg_search_bq_candidates return
                                  exactly what Weaviate's heaps return (V/flat/index.go:347-389,
                                  497-520): which rows of a tie at the R-th Hamming distance become
                                  candidates, their pop order, and the k-heap's choice and order among
                                  equal exact distances.  The scan also records the rows the heap could
                                  insert and the host replays the heap over them (~R ln(rows) per query).
                                  0: candidates = the (distance, docID)-lexicographic top-R, results
                                  ascending by (distance, docID) -- identical except at such ties. */
} wvg_options;
void wvg_options_default(wvg_options *opts);
int wvg_open_ex(int device, const wvg_options *opts, wvg_ctx **out);
int wvg_close(wvg_ctx *ctx);
int wvg_synchronize(wvg_ctx *ctx);
/* Page-locked host memory for a caller's reusable staging buffers (e.g. the
 * R rows flat.searchByVectorBQ gathers for its rescore, V/flat/index.go:375-385):
 * every entry point copies from / to such a buffer directly, without its own
 * staging copy.  Any other host pointer keeps working (copied through the
 * call's staging).  Free with wvg_host_free on the same context. */
int wvg_host_alloc(wvg_ctx *ctx, uint64_t bytes, void **out);
int wvg_host_free(wvg_ctx *ctx, void *p);
/* Device memory and streams of the context's GPU for the device-pointer
 * entry points below (wvg_search_device*, wvg_topk_merge_*), so a caller
 * without a HIP binding of its own (the Go backend) can hold queries,
 * results and workspaces in HBM: wvg_device_alloc returns `bytes` of HBM,
 * zero-filled when `zero` != 0 (a search workspace must be); free it with
 * wvg_device_free after the work using it has finished (wvg_stream_synchronize).
 * wvg_stream_create makes a non-blocking stream (a hipStream_t) for `stream`
 * arguments.  wvg_memcpy_h2d / _d2h copy on `stream` and return when the copy
 * is complete (so `src` / `dst` host memory may be a Go slice); `stream` NULL
 * = the default stream.  Replaces the cgo-side HIP plumbing a serving loop
 * would need (adapters/repos/db/vector_index.go:24-45 callers hold no HIP). */
int wvg_device_alloc(wvg_ctx *ctx, uint64_t bytes, int zero, void **out);
int wvg_device_free(wvg_ctx *ctx, void *p);
int wvg_stream_create(wvg_ctx *ctx, void **out);
int wvg_stream_destroy(wvg_ctx *ctx, void *stream);
int wvg_stream_synchronize(wvg_ctx *ctx, void *stream);
int wvg_memcpy_h2d(wvg_ctx *ctx, void *d_dst, const void *src, uint64_t bytes, void *stream);
int wvg_memcpy_d2h(wvg_ctx *ctx, void *dst, const void *d_src, uint64_t bytes, void *stream);
/* The reduction order of the fp32 distances (l2 / dot / cosine), i.e. which
 * of the reference's SIMD kernels the results must match bit for bit: its
 * init() picks l2_512 / dot_512 on hosts with AMX-BF16 and AVX-512, else
 * l2_256 / dot_256 (D/l2_amd64.go:19-25, D/dot_product_amd64.go:19-25).
 * Default WVG_ORDER_AVX256 (AMD EPYC hosts, which have no AMX).  Applies to
 * every fp32 distance of the context (scans, rescoring, DistanceToNode,
 * wvg_distance_batch); batched dot/cosine then scans with K1 instead of the
 * MFMA kernel, whose slices are the AVX2 order's chains.                  */
#define WVG_ORDER_AVX256 0
#define WVG_ORDER_AVX512 1
int wvg_set_distance_order(wvg_ctx *ctx, int order);

/* ---- corpus: the device-resident copy of a flat index's rows --------------
 * Replaces the LSM cursor scan of V/flat/index.go:411-452 and the BQ cache of
 * V/cache/sharded_lock_cache.go:29-60 (docID-indexed).  Slot = id - id_base.
 * id_base must be a multiple of 64; capacity is rounded up to 64 rows.      */
int wvg_corpus_create(wvg_ctx *ctx, int kind, int metric, uint32_t dim, uint64_t id_base,
                      uint64_t capacity, wvg_corpus **out);
int wvg_corpus_destroy(wvg_corpus *c);
/* cache.Grow analogue (V/cache/sharded_lock_cache.go:251): keeps contents. */
int wvg_corpus_reserve(wvg_corpus *c, uint64_t capacity);
int wvg_corpus_info(wvg_corpus *c, uint64_t *count, uint64_t *high_water, uint64_t *capacity);
/* flat.Add / AddBatch (V/flat/index.go:247-274): validates the dimension
 * ("insert called with a vector of the wrong size"), normalizes for cosine,
 * and for kind BQ encodes on device (index.go:262-270), for PQ encodes with
 * the codebook (CH/product_quantization.go:420).  vectors: [n][dim] float32. */
int wvg_corpus_upsert(wvg_corpus *c, const uint64_t *ids, const float *vectors, uint64_t n,
                      uint32_t dim);
/* Load already-stored rows (restart from the "vectors" / "vectors_compressed"
 * buckets, V/flat/index.go:640-681): F32 = [n][dim] float32 (already
 * normalized at Add for cosine), BQ = [n][ceil(dim/64)] uint64 LE words,
 * PQ = [n][m] bytes.  Stored as given (no normalization / encoding). */
int wvg_corpus_upsert_codes(wvg_corpus *c, const uint64_t *ids, const void *codes, uint64_t n);
/* Restart / PostStartup bulk load from an LSM cursor (V/flat/index.go:640-681):
 * keys [n][8] big-endian docIDs, values [n][value_bytes] little-endian rows as
 * the "vectors" (F32: dim float32) or "vectors_compressed" (BQ: uint64 words)
 * bucket stores them, or PQ codes (m bytes).  Stored as given; the capacity
 * grows to the largest id (bqCache.Grow(maxID)).                           */
int wvg_corpus_load_kv(wvg_corpus *c, const uint8_t *keys, const uint8_t *values, uint64_t n,
                       uint64_t value_bytes);
/* Batched Distance / CompressorDistancer.DistanceToNode(id) (CH/compression.go:306-325,
 * the HNSW rescore loop V/hnsw/search.go:564-581): the query's distance to
 * the rows with docIDs ids[n] (F32: SingleDist, BQ: Hamming, PQ: ADC);
 * out_ok[i] = 0 (and out_dists[i] = 0) where the id is not live, like the
 * reference's ok=false for deleted nodes.                                  */
int wvg_corpus_distance_by_ids(wvg_corpus *c, const float *query, const uint64_t *ids, uint64_t n,
                               float *out_dists, uint8_t *out_ok);
/* The same for many queries in ONE launch (batched HNSW rescore: every
 * query's ef candidates, V/hnsw/search.go:564-581, for concurrent queries):
 * queries [nq][dim]; query q's ids are ids[offsets[q] .. offsets[q+1]),
 * offsets[nq+1] non-decreasing from 0; outputs parallel to ids.            */
int wvg_corpus_distance_by_ids_batch(wvg_corpus *c, const float *queries, uint32_t nq, const uint64_t *offsets,
                                     const uint64_t *ids, float *out_dists, uint8_t *out_ok);
/* flat.Delete (V/flat/index.go:276-295): clears the validity bit. */
int wvg_corpus_delete(wvg_corpus *c, const uint64_t *ids, uint64_t n);
/* flat.vectorById (V/flat/index.go:401-407): copies the stored row
 * (F32: dim floats, BQ: words u64, PQ: m bytes); WVG_ERR_NOT_FOUND if absent. */
int wvg_corpus_get(wvg_corpus *c, uint64_t id, void *out);
/* vectorById for many ids in one call (the rescore loop's row fetches,
 * V/flat/index.go:375-385): out [n][row bytes as wvg_corpus_get];
 * out_ok[i] = 0 (row zero-filled) where ids[i] is not live.               */
int wvg_corpus_get_batch(wvg_corpus *c, const uint64_t *ids, uint64_t n, void *out, uint8_t *out_ok);
/* Bench / test helper: fills slots [0, n) with synthetic rows generated in
 * place from a counter-based RNG keyed by (seed, id_base + slot, column);
 * distribution 0 = uniform [-1,1), 1 = integers 0..255.  F32 and BQ only.  */
int wvg_corpus_fill_synthetic(wvg_corpus *c, uint64_t seed, uint64_t n, int distribution);
/* PQ codebook: centers [m][ks][dim/m] float32 (KMeans centers, CH/kmeans.go:85-93).
 * Validation as NewProductQuantizer (CH/product_quantization.go:187-197).
 * Every accepted shape (m a divisor of dim, ks <= 256) is searchable: the
 * scan keeps the query's m x ks fp32 lookup table in LDS while it fits beside
 * its top-k buffer (at ks = 256: m <= 152 for k <= 64, m <= 144 for k <= 128,
 * m <= 128 for k <= 256, and any m that fits 160 KiB above k = 256) and reads
 * it in global memory above that -- the same distances, bit for bit.      */
int wvg_pq_set_codebook(wvg_corpus *c, const float *centers, uint32_t m, uint32_t ks);

/* ---- search ---------------------------------------------------------------
 * flat.SearchByVector (V/flat/index.go:307-334) for F32 corpora; for BQ the
 * Hamming top-k of findTopVectorsCached (index.go:456-495); for PQ the ADC
 * top-k (PQDistancer.Distance, CH/product_quantization.go:352-361).
 * queries: [nq][dim] float32 (normalized internally for cosine, index.go:323).
 * allow_bits: optional bitmap over global docIDs (helpers.AllowList), bit i of
 * word i/64; an empty allow list yields empty results (index.go:425-427).
 * Outputs: [nq][k] ids/dists, counts[nq] = min(k, live allowed rows).
 * Any k: up to 256 the fused register top-k of the scan; above, a radix
 * select + sort over per-row distance keys in HBM (the same distances).
 * PQ: any (m, ks) of wvg_pq_set_codebook, wherever the lookup table lives.  */
int wvg_search(wvg_corpus *c, const float *queries, uint32_t nq, uint32_t k,
               const uint64_t *allow_bits, uint64_t allow_words, uint64_t *out_ids,
               float *out_dists, uint32_t *out_counts);
/* nq flat.SearchByVector calls (V/flat/index.go:307-334), query i against
 * corpora[i] -- the shards of a multi-tenant class, one tenant per query
 * (adapters/repos/db/index.go:1516-1539, 1554-1565) -- in ONE scan launch and
 * one merge launch.  All corpora: kind F32, one context, one metric, one dim
 * (a class's tenants share its vector index config); a corpus may appear any
 * number of times.  queries [nq][dim].  allow_bits: NULL (no query filtered)
 * or nq pointers, entry i NULL or a bitmap over corpora[i]'s global docIDs of
 * allow_words[i] words (non-NULL with 0 words, or no allowed id in the
 * corpus: empty result for that query, as wvg_search).  k <= 256.
 * Outputs [nq][k] / counts[nq] exactly as nq wvg_search(corpora[i], q_i, 1, k,
 * allow_i) calls would write them: ids, distance bits, counts, padding.     */
int wvg_search_group(wvg_corpus *const *corpora, const float *queries, uint32_t nq, uint32_t k,
                     const uint64_t *const *allow_bits, const uint64_t *allow_words,
                     uint64_t *out_ids, float *out_dists, uint32_t *out_counts);
/* flat.searchByVectorBQ (V/flat/index.go:347-389): Hamming top-R over `bq`,
 * R = max(rescore_limit, k) (index.go:297-305), exact rescore of the R
 * candidates against the device-resident float rows of `f32`, top-k.      */
int wvg_search_bq_rescore(wvg_corpus *bq, wvg_corpus *f32, const float *queries, uint32_t nq,
                          uint32_t k, uint32_t rescore_limit, const uint64_t *allow_bits,
                          uint64_t allow_words, uint64_t *out_ids, float *out_dists,
                          uint32_t *out_counts);
/* The first half of searchByVectorBQ for callers whose float rows are not on
 * the GPU (the LSM "vectors" bucket, V/flat/index.go:375-380): the candidates
 * findTopVectorsCached leaves in its heap of R = rescore_limit (index.go:
 * 355-357, 456-495) in the order heap.Pop() returns them (:369-374), i.e.
 * descending Hamming distance with the heap's own order among ties.  Outputs
 * [nq][R] ids / Hamming distances, counts[nq]; feed them in this order to
 * wvg_rescore (which inserts in input order, as :375-385 does).  With
 * heap_replay = 0: the lexicographic top-R, descending.  Any R.           */
int wvg_search_bq_candidates(wvg_corpus *bq, const float *queries, uint32_t nq, uint32_t rescore_limit,
                             const uint64_t *allow_bits, uint64_t allow_words, uint64_t *out_ids,
                             float *out_dists, uint32_t *out_counts);
/* nq flat.searchByVectorBQ calls (V/flat/index.go:347-389), query i against
 * tenant i = (bq[i], f32[i]) -- the shards of a multi-tenant BQ class, one
 * tenant per query (adapters/repos/db/index.go:1516-1539, 1554-1565) -- in
 * three launches whatever nq is: a Hamming scan, the filter that finds the rows
 * findTopVectorsCached's heap can insert (index.go:456-506), the exact rescore
 * (:375-385).  R = max(rescore_limit, k) (:297-305); any R and any k.  Every
 * bq[i] is a BQ and every f32[i] an F32 corpus of one context, metric and dim,
 * bq[i] and f32[i] with one id_base; a tenant may appear any number of times.
 * allow_bits / allow_words as wvg_search_group (per query, over tenant i's
 * global docIDs).  Outputs [nq][k] / counts[nq] exactly as nq
 * wvg_search_bq_rescore(bq[i], f32[i], q_i, 1, k, rescore_limit, allow_i)
 * calls would write them -- the reference heaps' result, ties included.
 * heap_replay = 0, or dim above 8192: WVG_ERR_UNSUPPORTED.                 */
int wvg_search_group_bq_rescore(wvg_corpus *const *bq, wvg_corpus *const *f32, const float *queries,
                                uint32_t nq, uint32_t k, uint32_t rescore_limit,
                                const uint64_t *const *allow_bits, const uint64_t *allow_words,
                                uint64_t *out_ids, float *out_dists, uint32_t *out_counts);
/* The first half only, for callers whose float rows are not on the GPU
 * (V/flat/index.go:355-374): per query what wvg_search_bq_candidates(bq[i],
 * q_i, 1, rescore_limit, allow_i) writes -- [nq][rescore_limit] ids / Hamming
 * distances in the heap's pop order, counts[nq].                           */
int wvg_search_group_bq_candidates(wvg_corpus *const *bq, const float *queries, uint32_t nq,
                                   uint32_t rescore_limit, const uint64_t *const *allow_bits,
                                   const uint64_t *allow_words, uint64_t *out_ids, float *out_dists,
                                   uint32_t *out_counts);

/* flat.SearchByVectorDistance (V/flat/index.go:531-591): every row with
 * dist <= target_distance or |dist - target| <= 1e-6 (floatcomp.InDelta,
 * usecases/floatcomp/delta.go:16-19), ascending, as far as the growing-limit
 * loop reaches (limits 100, 1100, 11100, ...; V/common/search_by_dist_params.go:
 * 14-83): it stops at the first window whose last row is above the target,
 * and before a limit above max_limit (max_limit < 0: unlimited).  One pass
 * over the corpus regardless of how many windows the loop takes.
 * *out_count = number of results; min(count, out_capacity) are written. */
int wvg_search_by_distance(wvg_corpus *c, const float *query, float target_distance, int64_t max_limit,
                           const uint64_t *allow_bits, uint64_t allow_words, uint64_t *out_ids,
                           float *out_dists, uint64_t out_capacity, uint64_t *out_count);
/* The flat index's own SearchByVectorDistance result (V/flat/index.go:
 * 531-591 as written): its loop calls recursiveSearch once -- the post
 * statement of the `for` is empty, so later iterations only grow the limit
 * until max_limit stops them (and never stop when max_limit < 0) -- so the
 * result is the first window: among the `window` (100:
 * V/common/search_by_dist_params.go:17) nearest rows, those with dist <=
 * target or within 1e-6 of it, up to the first row beyond.  HNSW callers use
 * wvg_search_by_distance (V/hnsw/search.go:85-151 re-searches).            */
int wvg_search_by_distance_window(wvg_corpus *c, const float *query, float target_distance, uint32_t window,
                                  const uint64_t *allow_bits, uint64_t allow_words, uint64_t *out_ids,
                                  float *out_dists, uint64_t out_capacity, uint64_t *out_count);

/* Device-pointer variants: inputs/outputs in HBM, asynchronous on `stream`
 * (a hipStream_t, NULL = default stream); no host synchronization, no
 * allocation (caller supplies a workspace of wvg_search_workspace_size bytes,
 * zero-filled once before its first use), so a call can be captured in a
 * hipGraph.  Exception: the first screened batch of a corpus (batch_screen;
 * dot / cosine / l2-squared) allocates and builds its shadow on `stream`;
 * under capture that never happens -- a corpus without a current shadow takes
 * the exact path, one with a shadow waits for it before the capture (run one
 * uncaptured batch first to warm it).  d_counts may be NULL.  One workspace
 * serves any number of calls issued in order on one stream.  Its first 256
 * bytes are a status block that is the same for every entry point, (nq, k)
 * and corpus: the sticky status word wvg_search_device_check reads, and the
 * arrival counter of wvg_search_device_pipelined's prologue, which is zero
 * between calls -- the one zero fill is what starts it.  An empty corpus
 * (e.g. a rank whose slab holds no rows) yields empty results: ids
 * UINT64_MAX, dists +inf, counts 0 (as wvg_search).  wvg_search_device
 * takes F32, BQ and PQ corpora (d_queries: float [nq][dim]; BQ codes and PQ
 * LUTs are built on the device -- size the workspace after the PQ codebook
 * is set); wvg_search_device_pipelined takes the same three kinds.  For a BQ
 * corpus, and for a PQ corpus with a codebook, the size is the largest of
 * wvg_search_device's layout and the pipelined ones (status block, partial
 * lists [nq][row ranges][k], the queries' codes or LUTs); it never got
 * smaller than it was.
 * Any k: up to 256 wvg_search_device uses the fused register top-k; above,
 * the select route on the device (F32 with dim % 4 == 0, every metric and both
 * distance orders; BQ; PQ with any (m, ks)), with the same guarantees:
 * asynchronous on `stream`, nothing read from or written to host memory, no
 * synchronization, no allocation, capturable, the status block untouched, and
 * on any error nothing launched.  The queries run in groups of G = 4 on the
 * stream, one group after another through one block of keys: the ordered
 * 32-bit distance key of every slot for each query of the group (L2 / dot /
 * cosine rows of d >= 8 in the AVX2 order: one pass over the rows for the
 * whole group, each 64-row tile loaded once; everywhere else one pass per
 * query), a radix select of the k-th key per query, a compaction that keeps
 * the keys below it and, in slot order, as many of the rows equal to it as
 * the result holds -- exactly min(k, live rows) entries however many rows
 * tie -- a sort, and the emit; no workgroup waits for another.  Per query the
 * outputs are wvg_search's for that query alone, bit for bit: ids ascending
 * by (distance, docID), counts = min(k, live rows), padding ids UINT64_MAX
 * and dists +inf.  k at or above the corpus's slot count skips the select; a
 * corpus of more than 2^32 slots answers WVG_ERR_UNSUPPORTED for k > 256 (the
 * keys hold the slot in 32 bits, as the host path's).  For k > 256
 * wvg_search_workspace_size returns this route's bytes, which depend on the
 * corpus geometry, nq and k alone and grow with G x slots, not nq x slots:
 *   256 (status block) + G x slots x 4 (keys) + G x 16 (select states)
 *   + G x 4096 x 4 (histograms) + G x ceil(slots / 2048) x 8 (range counts)
 *   + G x 8 (totals) + 2 x G x k x 8 (compacted and sorted entries)
 *   + the sort's temporary storage for k entries
 *   + the queries' codes or LUTs for all nq queries, as for k <= 256,
 * every piece rounded up to 256 bytes, slots = 64 x the corpus's tiles.  The
 * pipelined, grouped and multi-GPU entry points keep k <= 256.             */
size_t wvg_search_workspace_size(wvg_corpus *c, uint32_t nq, uint32_t k);
int wvg_search_device(wvg_corpus *c, const float *d_queries, uint32_t nq, uint32_t k,
                      uint64_t *d_ids, float *d_dists, uint32_t *d_counts, void *d_workspace,
                      size_t workspace_bytes, void *stream);
/* nq single-query searches (flat.SearchByVector per query, as concurrent
 * Weaviate queries issue them) in ONE launch.  The results are those of nq
 * independent searches, bit for bit.  Where the shared-row kernel applies
 * -- nq >= 2, an L2 / dot / cosine corpus of any d >= 8 (a multiple of 4, as
 * device search requires) in the AVX2 distance order, cache_reuse on -- the
 * rows are read once per pass of up to 16 queries at d = 128 (k <= 64; 8 for
 * k <= 128, 4 above) and of 4 queries at every other d (2 for k > 128), and
 * every query of the pass is scored against each row while it is in
 * registers; one merge workgroup per query merges its partial lists in the
 * same launch.  A short prologue launch on the same stream prepares that
 * scan's part of the workspace (its hand-off words and, where every wave
 * scans only a few tiles, per query the k-th distance of a sample of the
 * first rows, which bounds the scan's lists from the start; the results do
 * not depend on it).  In the prologue one wave scores one (sample tile,
 * query) pair anywhere on the chip and the workgroup that finishes last
 * combines them; no workgroup waits for another.  Everywhere else (one query, other metrics, d = 4, the
 * AVX-512 order, cache_reuse = 0) every query is one full scan of the corpus:
 * the scan workgroups walk the queries back to back and one extra workgroup
 * merges each query's lists while the scan moves on.  Same workspace size
 * rule; outputs as wvg_search_device.
 * BQ corpora (d_queries: float [nq][dim] of any dim, as wvg_search_device
 * takes them -- normalized by the caller for cosine; the sign codes are made
 * on the device): with nq >= 2 and cache_reuse on, two launches on `stream`,
 * a scan whose waves load every 64-row tile of codes once per pass of 8
 * queries and score it against each of them (XOR + popcount, the query words
 * wave-uniform), then the merge of the partial lists; no workgroup waits for
 * another and the status block is not touched.  One query, or cache_reuse =
 * 0, is wvg_search_device's route for that nq.  Per query the result is
 * wvg_search_device's for that query alone: the (Hamming distance, docID)-
 * lexicographic top-k, ascending.  The order the reference's heap keeps
 * inside ties is what wvg_search_bq_candidates returns, and that needs the
 * host; the rescore of the candidates stays with wvg_rescore or the caller.
 * PQ corpora (d_queries: float [nq][dim], as wvg_search_device takes them;
 * the LUTs are made on the device): with nq >= 2, cache_reuse on and a
 * codebook of which at least two LUTs (m x ks x 4 bytes each) fit one
 * workgroup's LDS, three launches on `stream`: the LUTs, a scan whose waves
 * load every 64-row tile of codes once per pass of Q queries -- Q = 4 where
 * four LUTs fit (m <= 32 at ks = 256), else 2 (m <= 64) -- and look each
 * (row, segment) up once for all of them in an LDS image that keeps the Q
 * queries' entries side by side, then the merge of the partial lists; no
 * workgroup waits for another and the status block is not touched.  Every
 * query's sum runs in segment order from 0, so per query the result is
 * wvg_search_device's for that query alone, bit for bit.  One query,
 * cache_reuse = 0 or a larger codebook (m >= 96 at ks = 256) is
 * wvg_search_device's route for that nq.  A PQ corpus whose codebook has not
 * been set has no (m, ks) and hence no route: WVG_ERR_UNSUPPORTED from this
 * call, the filtered one and the plan, checked before anything else about
 * the corpus (wvg_search_device answers WVG_ERR_INVALID, as before).
 * wvg_search_device_pipelined_plan tells which route a call takes.          */
int wvg_search_device_pipelined(wvg_corpus *c, const float *d_queries, uint32_t nq, uint32_t k,
                                uint64_t *d_ids, float *d_dists, uint32_t *d_counts,
                                void *d_workspace, size_t workspace_bytes, void *stream);
/* wvg_search_device_pipelined with one allow list per query (Weaviate attaches
 * an AllowList to every query that has a `where` filter; the flat index then
 * scans only the allowed docIDs, V/flat/index.go:423-449).  The lists are a
 * window of the docID space, resident on the device: d_allow holds
 * [nq][allow_stride] 64-bit words and bit b of word w of query q's row stands
 * for docID allow_first_id + 64 w + b.  allow_first_id must be a multiple of
 * 64 (WVG_ERR_INVALID otherwise, nothing launched).  Every docID outside
 * [allow_first_id, allow_first_id + 64 allow_stride) is not allowed; the
 * window may begin before the corpus's id_base or end after its rows, and bits
 * that name no row are ignored.  The caller fixes the window because the host
 * never reads the bitmap (that would need a synchronization); the kernels read
 * it in place, no copy of it is made in the workspace.
 * The outputs are exactly what nq calls wvg_search(c, q_i, 1, k, allow_i, ...)
 * write: ids, distance bits, counts and padding.  allow_stride == 0 or a row
 * of zeros gives that query an empty result (ids UINT64_MAX, dists +inf,
 * count 0), as an empty allow list does in wvg_search.  d_allow == NULL is
 * wvg_search_device_pipelined exactly.  Where the shared-row kernel applies
 * (see above) the filtered queries share each row read like unfiltered ones:
 * a query scores only the rows its list allows, and a 64-row tile that no
 * query of the pass allows is skipped before it is read.  Everywhere else
 * (one query, other metrics, d = 4, cache_reuse = 0) every query is one scan
 * with its own window, followed by a merge launch for nq >= 2.  BQ corpora:
 * the shared-row BQ scan masks each query's rows with its own words and does
 * not load a tile no query of the pass allows; with one query or cache_reuse
 * = 0, one Hamming scan launch per query, each with its window, and one
 * merge.  PQ corpora: the shared-row PQ scan does the same with its Q
 * queries per pass; where it does not apply (one query, cache_reuse = 0, a
 * codebook beyond it), one ADC scan launch per query, each with its window,
 * and one merge.  Otherwise as wvg_search_device_pipelined: F32, BQ and PQ
 * corpora (a PQ corpus without a codebook: WVG_ERR_UNSUPPORTED),
 * asynchronous on `stream`, no allocation, no host synchronization,
 * capturable; the same workspace rule.                                      */
int wvg_search_device_pipelined_filtered(wvg_corpus *c, const float *d_queries, uint32_t nq, uint32_t k,
                                         const uint64_t *d_allow, uint64_t allow_stride,
                                         uint64_t allow_first_id, uint64_t *d_ids, float *d_dists,
                                         uint32_t *d_counts, void *d_workspace, size_t workspace_bytes,
                                         void *stream);
/* What wvg_search_device_pipelined(c, ..., nq, k, ...) will do, for a caller
 * that sizes its batches to fill whole passes.  Host only: no device call,
 * nothing launched; computed by the functions the search itself routes with.
 * With an allow list the same call shares rows under the same conditions.
 * nq == 0, k == 0 or an empty corpus: passes = 0.  A BQ corpus: {1, Q,
 * ceil(nq / Q), 0, 0} with the scan's Q (8) for nq >= 2 and cache_reuse on,
 * {0, 1, nq, 0, 0} otherwise.  A PQ corpus: {1, Q, ceil(nq / Q), 0, 0} with
 * the scan's Q (4 or 2 by how many of its LUTs fit LDS for this k) for nq
 * >= 2 and cache_reuse on, {0, 1, nq, 0, 0} otherwise, a codebook beyond
 * the shared scan (m >= 96 at ks = 256) included.  Errors as the search's
 * (a PQ corpus without a codebook, k > 256, an F32 corpus with dim % 4 !=
 * 0).                                                                       */
typedef struct wvg_stream_plan {
    uint32_t shared_rows;      /* 1: the shared-row kernel; 0: one scan per query */
    uint32_t queries_per_pass; /* queries that share one read of the rows (1 if !shared_rows) */
    uint32_t passes;           /* reads of the corpus the call makes */
    uint32_t seeded;           /* the prologue samples rows */
    uint32_t screened;         /* the bf16 screen runs */
} wvg_stream_plan;
int wvg_search_device_pipelined_plan(wvg_corpus *c, uint32_t nq, uint32_t k, wvg_stream_plan *out);
/* Whether the next wvg_search_device_pipelined(c, ..., nq, k, ...) call outside a
 * stream capture reads the corpus's bf16 shadow, and what that costs in memory.
 * A screened call (wvg_stream_plan.screened: l2-squared, d = 128, k <= 64, a
 * seeded range) in a context with batch_screen != 0 screens every 64-row tile
 * from the shadow that l2-squared batches use (2 * dim + 4 bytes per row) and
 * reads fp32 values only for the rows the screen admits; results are the same
 * bits either way.  *reads_shadow = 1 then, and *shadow_bytes_per_row = what
 * the first such call allocates per row of capacity (0 with *reads_shadow = 0).
 * Two facts for the caller: the FIRST such call of a corpus allocates the
 * shadow and builds it with one pass over the rows on the call's stream (a
 * benchmark pays that in its warm-up), and rows written since are rebuilt at
 * the next call, as for batches; the shadow is dropped when the corpus grows.
 * batch_screen = 0 keeps the stream off the shadow as it keeps batches off it.
 * Under stream capture nothing is allocated or built: a captured call records
 * the shadow-fed kernel if the shadow exists and is current, and the
 * fp32-screened kernel otherwise, as it does after a failed allocation.
 * Unscreened calls (other metrics or dims, k > 64, one query, cache_reuse = 0,
 * long unseeded ranges) never allocate a shadow.  The workspace size does not
 * depend on any of this.  Host only; either pointer may be NULL.             */
int wvg_search_device_pipelined_shadow(wvg_corpus *c, uint32_t nq, uint32_t k, uint32_t *reads_shadow,
                                       uint32_t *shadow_bytes_per_row);
/* The route a batch of nq queries with this k takes on corpus c (wvg_search,
 * wvg_search_device, wvg_multi_search), for a caller that sizes its batches
 * or wants to see the route: results are identical on every route by design.
 * Host only: nothing launched; computed by the functions the search itself
 * routes with.  Answers for every kind and metric: F32 dot / cosine /
 * l2-squared batches of at least mfma_min_queries report matrix = 1 and their
 * screen (l2-squared: the bf16 screen, 1, where it applies -- d % 32 == 0,
 * k <= 16, the AVX2 order, batch_screen != 0 -- and no matrix path at all
 * elsewhere); BQ / PQ corpora, other metrics, smaller batches, k > 256, an
 * empty corpus, nq == 0 or k == 0: all zero.  shared_allow_list != 0: the
 * batch carries one allow list for all its queries; the route is the same.
 * Per-query allow windows never take the matrix path.                      */
typedef struct wvg_batch_plan {
    uint32_t matrix;   /* 1: scored on the matrix cores */
    uint32_t screen;   /* 0 none (exact only), 1 bf16 screen + exact rescore, 2 int8 screen + exact rescore */
    uint32_t shadow_bytes_per_row; /* what the first such search allocates per row of capacity; 0 if none */
    uint32_t reserved;
} wvg_batch_plan;
int wvg_search_batch_plan(wvg_corpus *c, uint32_t nq, uint32_t k, int shared_allow_list, wvg_batch_plan *out);
/* Synchronizes `stream` and reads (and clears) the workspace's sticky status
 * word: WVG_ERR_DEVICE if any device search on this workspace since the last
 * check could not complete -- the query-stream merge workgroup of
 * wvg_search_device_pipelined gave up waiting for the scan (bounded at 4 s);
 * the queries it could not merge were given empty results, never stale ones. */
int wvg_search_device_check(wvg_ctx *ctx, void *d_workspace, void *stream);
/* Multi-shard merge (Index.objectVectorSearch, adapters/repos/db/index.go:1644-1648):
 * [nlists][nq][k_in] (dist, id) lists (the layout an all-gather of per-GPU
 * [nq][k_in] results produces) -> [nq][k] ascending, ties by id; missing
 * entries carry id UINT64_MAX.                                            */
int wvg_topk_merge_device(wvg_ctx *ctx, const float *d_dists, const uint64_t *d_ids, uint32_t nq,
                          uint32_t nlists, uint32_t k_in, uint32_t k, uint64_t *d_out_ids,
                          float *d_out_dists, uint32_t *d_out_counts, void *stream);
/* The same merge over packed blocks, so one all-gather moves both halves of
 * every rank's result: a block holds ids [nq][k] uint64 at byte 0 and dists
 * [nq][k] float32 at byte nq*k*8, and is wvg_topk_packed_bytes(nq, k) bytes
 * (a multiple of 16); d_packed holds nlists consecutive blocks.  Write a
 * block directly with wvg_search_device*(..., d_ids = block,
 * d_dists = block + nq*k*8, ...).                                          */
size_t wvg_topk_packed_bytes(uint32_t nq, uint32_t k);
int wvg_topk_merge_packed(wvg_ctx *ctx, const void *d_packed, uint32_t nq, uint32_t nlists, uint32_t k_in,
                          uint32_t k, uint64_t *d_out_ids, float *d_out_dists, uint32_t *d_out_counts,
                          void *stream);

/* ---- several GPUs in one process ------------------------------------------
 * Index.objectVectorSearch (adapters/repos/db/index.go:1567-1648) fans a
 * search out over the shards of one process and merges their results by
 * distance.  A multi handle holds one context per device (opts as
 * wvg_open_ex) and, when the devices are distinct and RCCL loads, one
 * communicator per device (ncclCommInitAll).  A multi corpus deals docIDs to
 * the devices in contiguous slabs: shard i holds [i * slab, (i + 1) * slab),
 * slab = rows / ndev rounded up to 64.  wvg_multi_search runs every shard's
 * scan on its own device stream into a packed block, ONE grouped RCCL
 * all-gather of the blocks over xGMI (peer copies to device 0 when devices
 * repeat, e.g. a one-GPU rehearsal {0, 0}), the merge on device 0, and returns
 * [nq][k] ascending by (distance, docID) -- identical to one corpus holding
 * every row.  Per-shard operations (PQ codebooks, other search kinds) take
 * the shard's own handle from wvg_multi_corpus_shard.                      */
typedef struct wvg_multi wvg_multi;
typedef struct wvg_multi_corpus wvg_multi_corpus;
int wvg_multi_open(const int *devices, int ndev, const wvg_options *opts, wvg_multi **out);
int wvg_multi_close(wvg_multi *m);  /* after every multi corpus is destroyed */
int wvg_multi_info(wvg_multi *m, int *ndev, int *uses_rccl);
int wvg_multi_ctx(wvg_multi *m, int i, wvg_ctx **out);
int wvg_multi_corpus_create(wvg_multi *m, int kind, int metric, uint32_t dim, uint64_t rows,
                            wvg_multi_corpus **out);
int wvg_multi_corpus_destroy(wvg_multi_corpus *mc);
int wvg_multi_corpus_shard(wvg_multi_corpus *mc, int i, wvg_corpus **out, uint64_t *id_base, uint64_t *slab_rows);
/* flat.Add / Delete routed to the shard owning each docID (WVG_ERR_CAPACITY
 * for an id beyond the last slab). */
int wvg_multi_corpus_upsert(wvg_multi_corpus *mc, const uint64_t *ids, const float *vectors, uint64_t n,
                            uint32_t dim);
int wvg_multi_corpus_delete(wvg_multi_corpus *mc, const uint64_t *ids, uint64_t n);
/* As wvg_corpus_fill_synthetic over docIDs [0, n) of the whole corpus. */
int wvg_multi_corpus_fill_synthetic(wvg_multi_corpus *mc, uint64_t seed, uint64_t n, int distribution);
int wvg_multi_corpus_set_codebook(wvg_multi_corpus *mc, const float *centers, uint32_t m, uint32_t ks);
/* wvg_search over all shards (any kind; k <= 256; allow_bits over global docIDs). */
int wvg_multi_search(wvg_multi_corpus *mc, const float *queries, uint32_t nq, uint32_t k,
                     const uint64_t *allow_bits, uint64_t allow_words, uint64_t *out_ids, float *out_dists,
                     uint32_t *out_counts);
/* flat.searchByVectorBQ (V/flat/index.go:347-389, 456-506) over a BQ class
 * dealt over the devices: `bq` and `f32` are a BQ and an F32 multi corpus of
 * the same multi handle with the same dim, metric and slab.  Every slab runs
 * the recording Hamming scan on its device; the slabs' distance histograms
 * are exchanged (one grouped all-gather, or peer copies) so that slab s also
 * drops what the R-th smallest distance of slabs 0..s-1 already excludes; the
 * kept rows of all slabs, in docID order, go through ONE heap of R =
 * max(rescore_limit, k) on the host, the popped ids are rescored exactly on
 * the slab that owns them and inserted into the heap of k in pop order.
 * Outputs as wvg_search_bq_rescore, and equal to it on one corpus holding
 * every row.  Contexts opened with heap_replay = 0: WVG_ERR_UNSUPPORTED.    */
int wvg_multi_search_bq_rescore(wvg_multi_corpus *bq, wvg_multi_corpus *f32, const float *queries,
                                uint32_t nq, uint32_t k, uint32_t rescore_limit, const uint64_t *allow_bits,
                                uint64_t allow_words, uint64_t *out_ids, float *out_dists,
                                uint32_t *out_counts);
/* Its first half (V/flat/index.go:347-389, 456-506; see
 * wvg_search_bq_candidates): the heap's R = rescore_limit candidates over all
 * slabs in the order heap.Pop() returns them, ids as global docIDs.  Outputs
 * as wvg_search_bq_candidates.  heap_replay = 0: WVG_ERR_UNSUPPORTED.       */
int wvg_multi_search_bq_candidates(wvg_multi_corpus *bq, const float *queries, uint32_t nq,
                                   uint32_t rescore_limit, const uint64_t *allow_bits, uint64_t allow_words,
                                   uint64_t *out_ids, float *out_dists, uint32_t *out_counts);

/* The rescore loop of flat.searchByVectorBQ (V/flat/index.go:375-385) when
 * the candidate rows come from the host (LSM point gets): exact SingleDist of
 * q against rows [n][dim] (q used as given: normalize it first for cosine,
 * as index.go:352 does), each inserted into a heap of k in input order
 * (insertToHeap, :384) and extracted (extractHeap, :508-520), so ties among
 * equal distances resolve exactly as the reference's heap resolves them
 * (heap_replay = 0: ascending by (dist, input position)).  out_count = min(k, n). */
int wvg_rescore(wvg_ctx *ctx, int metric, const float *q, const float *rows, const uint64_t *ids,
                uint64_t n, uint32_t dim, uint32_t k, uint64_t *out_ids, float *out_dists,
                uint32_t *out_count);
/* Bulk PQ compression of a resident float corpus (hnsw.compress ->
 * compressor.Preload per vector, V/hnsw/compress.go:98-104): every live row
 * of `f32` is encoded with `pq`'s codebook into the same slot of `pq`.  Both
 * corpora must share dim and id_base. */
int wvg_pq_encode_corpus(wvg_corpus *pq, wvg_corpus *f32);
/* Bench / test helper: the synthetic generator of wvg_corpus_fill_synthetic
 * for arbitrary row ids: out [n][dim] (normalized if `normalize`). */
int wvg_synthetic_rows(wvg_ctx *ctx, uint64_t seed, const uint64_t *ids, uint64_t n, uint32_t dim,
                       int distribution, int normalize, float *out);

/* Profiling: while enabled, every scan-kernel launch of this context is
 * bracketed by a pair of HIP events on its stream; stop() synchronizes and
 * returns the summed scan-kernel time and the launch count (feeds the
 * vector_index_durations_ms metric, usecases/monitoring/prometheus.go:292). */
int wvg_profile_start(wvg_ctx *ctx);
int wvg_profile_stop(wvg_ctx *ctx, double *scan_ms_total, uint64_t *scan_launches);
/* Measurement helper: the HBM streaming-read rate of this GPU, in GB/s -- the
 * best of 16-byte non-temporal reads of a `bytes` buffer (its own
 * allocation, freed again) in two shapes -- grid-stride over 1024..8192
 * workgroups, and the scans' contiguous chunk per workgroup (8 KiB per wave
 * per step) over 256..2048 workgroups -- `reps` passes each.  The ceiling
 * the HBM-bound scans are compared with (roofline).                       */
int wvg_measure_hbm_read(wvg_ctx *ctx, uint64_t bytes, uint32_t reps, double *out_gbps);

/* ---- bulk primitives (distancer.BatchProvider / compressionhelpers bulk) --- */
/* Provider.SingleDist of q against n rows X [n][dim] (D/provider.go:14-20). */
int wvg_distance_batch(wvg_ctx *ctx, int metric, const float *q, const float *X, uint64_t n,
                       uint32_t dim, float *out);
/* distancer.Normalize of n rows (D/normalize.go:16-32). */
int wvg_normalize_batch(wvg_ctx *ctx, const float *X, uint64_t n, uint32_t dim, float *out);
/* BinaryQuantizer.Encode of n rows -> [n][ceil(dim/64)] words (CH/binary_quantization.go:32-45). */
int wvg_bq_encode(wvg_ctx *ctx, const float *X, uint64_t n, uint32_t dim, uint64_t *out_words);
/* BinaryQuantizer.DistanceBetweenCompressedVectors of q against n codes (:47-56). */
int wvg_bq_distance_batch(wvg_ctx *ctx, const uint64_t *q, const uint64_t *codes, uint64_t n,
                          uint32_t words, float *out);
/* ProductQuantizer.Encode of n rows (CH/product_quantization.go:420-426,
 * CH/kmeans.go:103-135; ties to the highest centroid index). */
int wvg_pq_encode(wvg_ctx *ctx, const float *centers, uint32_t m, uint32_t ks, const float *X,
                  uint64_t n, uint32_t dim, uint8_t *out_codes);
/* DistanceLookUpTable for one query (CH/product_quantization.go:62-104): [m][ks]. */
int wvg_pq_lut(wvg_ctx *ctx, int metric, const float *centers, uint32_t m, uint32_t ks,
               uint32_t dim, const float *q, float *out_lut);
/* PQDistancer.Distance of n codes against a LUT (CH/product_quantization.go:352-361). */
int wvg_pq_adc_batch(wvg_ctx *ctx, int metric, const float *lut, uint32_t m, uint32_t ks,
                     const uint8_t *codes, uint64_t n, float *out);

/* ProductQuantizer.Fit with the k-means encoder (CH/product_quantization.go:372-418):
 * the first training_limit rows (0 = all) of X [n][dim]; per segment
 * KMeans.Fit (CH/kmeans.go:220-250): ks initial centers drawn (with
 * replacement) from the rows, Lloyd iterations -- nNearest assignment (ties to
 * the highest index), empty clusters reseeded from a random row of a cluster
 * with more than one member, centers = sequential fp32 sums / size -- until
 * fewer than int(float32(n) * 0.01) rows change or after 11 passes.  The
 * random draws come from a counter RNG keyed by (seed, segment) instead of
 * Go's unseeded global math/rand.  out_centers: [m][ks][dim/m];
 * out_iterations (nullable): [m] Lloyd passes per segment.  "not enough data
 * to fit kmeans" if fewer than ks rows.                                    */
int wvg_pq_fit(wvg_ctx *ctx, const float *X, uint64_t n, uint32_t dim, uint32_t m, uint32_t ks,
               uint64_t training_limit, uint64_t seed, float *out_centers, uint32_t *out_iterations);
/* buildGlobalDistances (CH/product_quantization.go:236-251): [m][ks][ks]
 * table of Step(C_s[i], C_s[j]) (the symmetric-distance table of HNSW's
 * node-to-node PQ distances). */
int wvg_pq_global_distances(wvg_ctx *ctx, int metric, const float *centers, uint32_t m, uint32_t ks, uint32_t dim,
                            float *out_table);
/* DistanceBetweenCompressedVectors (CH/product_quantization.go:297-311) of
 * code x against n codes [n][m], from the table above. */
int wvg_pq_sdc_batch(wvg_ctx *ctx, int metric, const float *table, uint32_t m, uint32_t ks, const uint8_t *x,
                     const uint8_t *codes, uint64_t n, float *out);

#ifdef __cplusplus
}
#endif

#endif /* WVGPU_H */

// wvg_bq_rescore.hip -- the second half of flat.searchByVectorBQ (V/flat/index.go:375-385) for
// callers whose queries and results stay in HBM: wvg_search_device_bq_rescore.
//
// Stage 1 is the device BQ search that exists (the pipelined route up to R = 256, the select route
// above), writing its [nq][R] docIDs and counts into the workspace.  Stage 2 is the one kernel of
// this file, bq_rescore_kernel: per query, R scattered fp32 rows scored exactly and reduced to the
// final [k] in one launch -- no per-candidate distances in memory, no merge launch, no host.
//
// Work shape: a row of the tiled corpus is dim / 4 16-byte chunks 1 KiB apart,
// so a candidate is dim / 4 independent 16-byte reads and the kernel is bound by how many of them
// are in flight, not by arithmetic.  Mapping:
//   - one workgroup of 8 waves per query; the query lies in LDS (up to 32 KiB, zero-padded);
//   - a wave scores 8 candidates at a time: lane = 8 * row + c, and lane c of a row owns chunk
//     position c of every 32-element block (chunks c, c + 8, c + 16, ...).  That is rowdist's
//     32-position mapping four positions per lane: the lane's float4 accumulator IS the four AVX2
//     chains acc[c >> 1][4 (c & 1) ..], every chain runs in block order as the reference's, and
//     up to 16 of the lane's loads (all independent) are issued before the first is used:
//     8 waves x 64 lanes x 16 loads x 16 B = 128 KiB in flight per query (the lane then has 256
//     registers, which the 16 loads, the AVX-512 order's accumulators and a 256-entry list need);
//   - the 32 chains meet in three lane exchanges (xor 2, xor 4, xor 1 inside the 8 lanes, DPP), in
//     the reference's tree; the AVX-512 order keeps four accumulators per lane over the 128-blocks
//     (chains a5[(c >> 2) + 2 i][4 (c & 3) ..]) and folds them into lanes 0 / 1 first;
//   - the row's lane 0 offers (Wrap(distance), slot) to the wave's register top-k, and the 8
//     lists meet in the workgroup's tree merge, whose wave 0 writes ids, distances, count, padding.
// Nothing is indexed by a run-time value in registers: no private segment.
#include "wvg_host.hpp"
#include "wvg_internal.hpp"
#include "wvg_rowdist.hpp"
#include "wvg_stream.hpp"
#include "wvg_topk.hpp"

namespace wvg {

constexpr int BQR_WAVES = 8;           // waves per query workgroup
constexpr uint32_t BQR_MAX_DIM = 8192; // the query's LDS image: 32 KiB
constexpr int BQR_INFLIGHT = 16;       // 16-byte loads a lane issues before it uses the first

struct BqRescoreArgs {
    const float4 *rows;          // F32 corpus, tiled
    const uint64_t *valid;       // its validity bitmap, one word per tile
    const float *queries;        // [nq][dim]
    const uint64_t *cand;        // [nq][R] docIDs of stage 1 (padding UINT64_MAX)
    const uint32_t *cand_counts; // [nq]
    uint64_t *ids;               // [nq][k]
    float *dists;                // [nq][k]
    uint32_t *counts;            // [nq] or NULL
    uint64_t id_base, capacity;
    uint32_t dim, nchunks, R, k;
    int metric;
};

__device__ __forceinline__ float4 xor_lane_f4(float4 v, int m)
{
    auto x = [&](float f) {
        const uint32_t u = __float_as_uint(f);
        return __uint_as_float(m == 1 ? xor_lane32<1>(u) : m == 2 ? xor_lane32<2>(u) : xor_lane32<4>(u));
    };
    return make_float4(x(v.x), x(v.y), x(v.z), x(v.w));
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

template <int METRIC>
__device__ __forceinline__ void upd4(float4 &acc, float4 q, float4 x)
{
    acc_update<METRIC>(acc.x, q.x, x.x);
    acc_update<METRIC>(acc.y, q.y, x.y);
    acc_update<METRIC>(acc.z, q.z, x.z);
    acc_update<METRIC>(acc.w, q.w, x.w);
}

// U block-rows from row r on: the lane's chunk of block-row r + i is 8 (r + i) + c.  All U loads
// are issued first.  Rows at or past nr load row nr - 1 again (a valid address) and are dropped.
// NACC = 4: the AVX-512 128-blocks, accumulator (r + i) & 3 (r is a multiple of 4 there).
template <int METRIC, int U, int NACC>
__device__ __forceinline__ void block_rows(const float4 *__restrict__ rp, const float4 *sq4, int r, int nr, int c,
                                           float4 (&acc)[NACC])
{
    float4 x[U];
    int ch[U];
#pragma unroll
    for (int i = 0; i < U; i++) {
        const int ri = r + i < nr ? r + i : nr - 1;
        ch[i] = ri * 8 + c;
        x[i] = rp[(size_t)ch[i] * 64];
    }
#pragma unroll
    for (int i = 0; i < U; i++) {
        float4 a = acc[i & (NACC - 1)];
        upd4<METRIC>(a, sq4[ch[i]], x[i]);
        if (r + i < nr) acc[i & (NACC - 1)] = a;
    }
}

template <int METRIC, int NACC>
__device__ __forceinline__ void block_range(const float4 *__restrict__ rp, const float4 *sq4, int r, int nr, int c,
                                            float4 (&acc)[NACC])
{
    for (; r + BQR_INFLIGHT <= nr; r += BQR_INFLIGHT) block_rows<METRIC, BQR_INFLIGHT, NACC>(rp, sq4, r, nr, c, acc);
    for (; r < nr; r += 4) block_rows<METRIC, 4, NACC>(rp, sq4, r, nr, c, acc);
}

// Provider.SingleDist(query, row) by the row's 8 lanes (c = lane & 7), in the order of
// row_dot_or_l2_generic (O512: row_dist_512); the result is valid in the row's lane c = 0.
// rp: chunk 0 of the row; sq: the query in LDS, zero-padded to whole chunks; n >= 1.
template <int METRIC, bool O512>
__device__ __forceinline__ float row_dist_8lanes(const float4 *__restrict__ rp, const float *sq, int n, int c)
{
    const float4 *sq4 = reinterpret_cast<const float4 *>(sq);
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 acc[1] = {zero};
    int r0 = 0;
    if (O512 && n >= 128) {
        // 128-blocks: chunk 8 i + c of a block is chain row j = (c >> 2) + 2 i, lanes l = 4 (c & 3) ..
        float4 a5[4] = {zero, zero, zero, zero};
        r0 = (n >> 7) * 4;
        block_range<METRIC, 4>(rp, sq4, 0, r0, c, a5);
        // ((a1+a0) + (a3+a2)) + ((a5+a4) + (a7+a6)): lane c ^ 4 holds the other parity of j
        float4 p[4];
#pragma unroll
        for (int i = 0; i < 4; i++) p[i] = add4(xor_lane_f4(a5[i], 4), a5[i]);
        const float4 r = add4(add4(p[3], p[2]), add4(p[1], p[0]));
        // acc[0][l] = r[l] + acc[0][l], then r[8 + l] + acc[0][l]: lanes 0 / 1 take lanes 2 / 3
        const float4 lo = add4(r, zero);
        const float4 hi = add4(xor_lane_f4(r, 2), lo);
        acc[0] = c < 2 ? hi : zero;
    }
    const int nb = n >> 5;
    block_range<METRIC, 1>(rp, sq4, r0, nb, c, acc);
    // leftover 8-blocks (at most 3): chunks 2 t, 2 t + 1 continue chains acc[0][0..7] = lanes 0 / 1
    const int pos = nb * 32, n8 = (n - pos) >> 3;
    if (n8 > 0) {
        float4 x[3];
        int ch[3];
#pragma unroll
        for (int t = 0; t < 3; t++) {
            ch[t] = (t < n8 && c < 2) ? (pos >> 2) + 2 * t + c : 0;
            x[t] = rp[(size_t)ch[t] * 64];
        }
#pragma unroll
        for (int t = 0; t < 3; t++) {
            float4 a = acc[0];
            upd4<METRIC>(a, sq4[ch[t]], x[t]);
            if (t < n8 && c < 2) acc[0] = a;
        }
    }
    // scalar tail (< 8 elements) into `sum`, in element order; every lane of the row computes it
    float sum = 0.0f;
    const int e0 = pos + 8 * n8, rem = n - e0;
    if (rem > 0) {
        const int c0 = e0 >> 2, c1 = rem > 4 ? c0 + 1 : c0;
        const float4 x0 = rp[(size_t)c0 * 64], x1 = rp[(size_t)c1 * 64];
        const float xs[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
        for (int i = 0; i < 7; i++) {
            float s2 = sum;
            scalar_update<METRIC>(s2, sq[i < rem ? e0 + i : e0], xs[i]);
            if (i < rem) sum = s2;
        }
    }
    if (n < 8) return sum;
    // s_l = (acc3 + acc2) + (acc1 + acc0); ((s0+s1) + (s2+s3)) + ((s4+s5) + (s6+s7)); sum + .
    const float4 pair = add4(xor_lane_f4(acc[0], 2), acc[0]);  // j < 2: acc1 + acc0; else acc3 + acc2
    const float4 s = add4(xor_lane_f4(pair, 4), pair);
    const float h = (s.x + s.y) + (s.z + s.w);                 // c even: s0..s3; odd: s4..s7
    const float other = __uint_as_float(xor_lane32<1>(__float_as_uint(h)));
    return sum + (h + other);
}

template <int METRIC, int E, bool O512>
__global__ __launch_bounds__(BQR_WAVES * 64) void bq_rescore_kernel(BqRescoreArgs a)
{
    __shared__ __attribute__((aligned(16))) float sq[BQR_MAX_DIM];
    const uint32_t qi = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int c = lane & 7;
    for (uint32_t i = threadIdx.x; i < a.nchunks * 4; i += BQR_WAVES * 64)
        sq[i] = i < a.dim ? a.queries[(size_t)qi * a.dim + i] : 0.0f;
    __syncthreads();
    WaveTopK<E> tk;
    tk.init((int)a.k);
    const uint32_t cnt = a.cand_counts[qi];
    const uint32_t n = cnt < a.R ? cnt : a.R;
    for (uint32_t j0 = (uint32_t)wave * 8; j0 < n; j0 += BQR_WAVES * 8) {
        const uint32_t j = j0 + ((uint32_t)lane >> 3);
        const uint64_t id = j < n ? a.cand[(size_t)qi * a.R + j] : WVG_KEY_NONE;
        // docID -> slot; a candidate that is not a live row of the F32 corpus is skipped
        const uint64_t slot = id - a.id_base;
        bool live = id != WVG_KEY_NONE && id >= a.id_base && slot < a.capacity;
        if (live) live = (a.valid[slot >> 6] >> (slot & 63)) & 1ull;
        const uint64_t rs = live ? slot : 0;  // dead lanes read row 0 and offer nothing
        const float4 *rp = a.rows + ((size_t)(rs >> 6) * a.nchunks) * 64 + (rs & 63);
        const float d = wrap_metric(a.metric, row_dist_8lanes<METRIC, O512>(rp, sq, (int)a.dim, c));
        tk.offer(live && c == 0 ? wvg_make_key(d, (uint32_t)slot) : WVG_KEY_NONE);
    }
    merge_finish<E, BQR_WAVES>(tk, a.k, a.id_base, a.ids + (size_t)qi * a.k, a.dists + (size_t)qi * a.k,
                               a.counts ? a.counts + qi : nullptr, nullptr, 0, false);
}

template <int METRIC, int E>
static void launch_bq_rescore_o(const BqRescoreArgs &a, uint32_t nq, int o512, hipStream_t s)
{
    if (o512)
        hipLaunchKernelGGL((bq_rescore_kernel<METRIC, E, true>), dim3(nq), dim3(BQR_WAVES * 64), 0, s, a);
    else
        hipLaunchKernelGGL((bq_rescore_kernel<METRIC, E, false>), dim3(nq), dim3(BQR_WAVES * 64), 0, s, a);
}

template <int METRIC>
static void launch_bq_rescore_e(const BqRescoreArgs &a, uint32_t nq, int o512, hipStream_t s)
{
    if (a.k <= 64)
        launch_bq_rescore_o<METRIC, 1>(a, nq, o512, s);
    else if (a.k <= 128)
        launch_bq_rescore_o<METRIC, 2>(a, nq, o512, s);
    else
        launch_bq_rescore_o<METRIC, 4>(a, nq, o512, s);
}

static hipError_t launch_bq_rescore(const BqRescoreArgs &a, uint32_t nq, int o512, hipStream_t s)
{
    if (a.metric == WVG_M_L2)
        launch_bq_rescore_e<WVG_M_L2>(a, nq, o512, s);
    else  // dot and cosine: the raw dot product, Wrap at run time
        launch_bq_rescore_e<WVG_M_DOT>(a, nq, o512, s);
    return hipGetLastError();
}

// Workspace: stage 1's own workspace first (it begins with the status block, which stays where
// every entry point expects it), then the candidates it leaves for stage 2.
struct BqRescoreLayout {
    size_t stage1 = 0, cand = 0, cand_dists = 0, cand_counts = 0, total = 0;
};

static BqRescoreLayout bq_rescore_layout(wvg_corpus *bq, uint32_t nq, uint32_t R)
{
    auto up = [](size_t v) { return align_up(v, 256); };
    BqRescoreLayout l;
    l.stage1 = wvg_search_workspace_size(bq, nq, R);
    l.cand = up(l.stage1);
    l.cand_dists = l.cand + up((size_t)nq * R * 8);
    l.cand_counts = l.cand_dists + up((size_t)nq * R * 4);
    l.total = l.cand_counts + up((size_t)nq * 4);
    return l;
}

static int bq_rescore_check(wvg_corpus *bq, wvg_corpus *f32, uint32_t k)
{
    if (!bq || !f32 || !bq->ctx || bq->kind != WVG_KIND_BQ || f32->kind != WVG_KIND_F32)
        return fail(WVG_ERR_INVALID, "need a BQ corpus and an F32 corpus");
    if (bq->ctx != f32->ctx || bq->dim != f32->dim || bq->id_base != f32->id_base || bq->metric != f32->metric)
        return fail(WVG_ERR_INVALID, "BQ and F32 corpora disagree on context/dim/id_base/metric");
    if (bq->metric != WVG_METRIC_L2 && bq->metric != WVG_METRIC_DOT && bq->metric != WVG_METRIC_COSINE)
        return fail(WVG_ERR_UNSUPPORTED, "device BQ rescore: l2-squared, dot and cosine only");
    if (k > MAX_K) return fail(WVG_ERR_UNSUPPORTED, "device BQ rescore: k <= 256");
    if (bq->dim > BQR_MAX_DIM) return fail(WVG_ERR_UNSUPPORTED, "device BQ rescore: dim <= 8192");
    if (f32->capacity > (1ull << 32)) return fail(WVG_ERR_UNSUPPORTED, "device BQ rescore: more than 2^32 slots");
    return WVG_OK;
}

}  // namespace wvg

using namespace wvg;

extern "C" {

size_t wvg_search_device_bq_rescore_workspace_size(wvg_corpus *bq, wvg_corpus *f32, uint32_t nq, uint32_t k,
                                                   uint32_t rescore_limit)
{
    if (!bq || !f32) return 0;
    return bq_rescore_layout(bq, nq, std::max(rescore_limit, k)).total;
}

int wvg_search_device_bq_rescore(wvg_corpus *bq, wvg_corpus *f32, const float *d_queries, uint32_t nq, uint32_t k,
                                 uint32_t rescore_limit, const uint64_t *d_allow, uint64_t allow_stride,
                                 uint64_t allow_first_id, uint64_t *d_ids, float *d_dists, uint32_t *d_counts,
                                 void *d_workspace, size_t workspace_bytes, void *stream)
{
    // every check comes before the first launch: on an error nothing has run
    int rc = bq_rescore_check(bq, f32, k);
    if (rc) return rc;
    const uint32_t R = std::max(rescore_limit, k);  // searchTimeRescore (V/flat/index.go:297-305)
    if (d_allow && R > MAX_K)
        return fail(WVG_ERR_UNSUPPORTED, "device BQ rescore: allow lists need max(rescore_limit, k) <= 256");
    if (d_allow && allow_first_id % 64 != 0) return fail(WVG_ERR_INVALID, "allow_first_id must be a multiple of 64");
    if (nq == 0 || k == 0) return WVG_OK;
    if (!d_queries || !d_ids || !d_dists) return fail(WVG_ERR_INVALID, "null queries / outputs");
    hipStream_t s = (hipStream_t)stream;
    bool no_rows;
    {
        std::shared_lock<std::shared_mutex> lk(f32->rw);
        no_rows = f32->capacity == 0 || f32->count == 0 || !f32->d_data;
    }
    if (no_rows) {  // no float row to rescore against: every candidate is skipped
        WVG_HIP(launch_fill_empty(d_ids, d_dists, d_counts, nq, k, s));
        return WVG_OK;
    }
    const BqRescoreLayout l = bq_rescore_layout(bq, nq, R);
    if (!d_workspace || workspace_bytes < l.total) return fail(WVG_ERR_INVALID, "workspace too small");
    char *w = (char *)d_workspace;
    uint64_t *cand = (uint64_t *)(w + l.cand);
    float *cand_dists = (float *)(w + l.cand_dists);
    uint32_t *cand_counts = (uint32_t *)(w + l.cand_counts);
    // stage 1: the (Hamming distance, docID)-lexicographic top-R per query (an empty BQ corpus: none)
    if (R <= MAX_K)
        rc = wvg_search_device_pipelined_filtered(bq, d_queries, nq, R, d_allow, allow_stride, allow_first_id, cand,
                                                  cand_dists, cand_counts, d_workspace, l.stage1, stream);
    else
        rc = wvg_search_device(bq, d_queries, nq, R, cand, cand_dists, cand_counts, d_workspace, l.stage1, stream);
    if (rc) return rc;
    // stage 2: exact distances of the candidates that are live float rows, top-k
    std::shared_lock<std::shared_mutex> lk(f32->rw);
    BqRescoreArgs a{};
    a.rows = (const float4 *)f32->d_data;
    a.valid = f32->d_valid;
    a.queries = d_queries;
    a.cand = cand;
    a.cand_counts = cand_counts;
    a.ids = d_ids;
    a.dists = d_dists;
    a.counts = d_counts;
    a.id_base = f32->id_base;
    a.capacity = f32->capacity;
    a.dim = f32->dim;
    a.nchunks = f32->nchunks;
    a.R = R;
    a.k = k;
    a.metric = f32->metric;
    WVG_HIP(launch_bq_rescore(a, nq, f32->ctx->order512, s));
    return WVG_OK;
}

}  // extern "C"

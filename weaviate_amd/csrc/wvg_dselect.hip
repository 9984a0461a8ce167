// wvg_dselect.hip -- wvg_search_device for k above the fused register top-k
// (k > 256): the unbounded selection of wvg_select.hip as a chain of launches
// on the caller's stream, batched over groups of DSEL_G queries.  Nothing is
// read from or written to host memory, nothing synchronizes or allocates, the
// sizes of every launch are known on the host, and no workgroup waits for
// another, so a call can be captured in a graph.
//
// Per group of G queries (one group after another through one key block):
//   D1 keys    : the ordered u32 distance key of every slot for each query of
//                the group (0xFFFFFFFF = dead).  L2 / dot / cosine rows in the
//                AVX2 order with d >= 8: dsel_keys_f32_kernel, a wave loads
//                each 64-row tile once (lane = row) and feeds the G queries'
//                accumulator sets while a chunk is in registers.  Everywhere
//                else: one launch_ordkeys per query (wvg_select.hip S1).
//   D2 select  : the k-th smallest key per query, 12 + 12 + 8 bit digits, the
//                query a grid dimension, one pick workgroup per query; the
//                state is set up by dsel_init_kernel.  Afterwards the state
//                holds thr (the k-th key) and krem (how many of the rows with
//                key == thr belong to the result).
//   D3 compact : every live key below thr and the first krem slots, in slot
//                order, among the keys equal to thr: exactly min(k, live)
//                entries however many rows tie.  Workgroup r owns the DSEL_RANGE
//                consecutive slots [r DSEL_RANGE, (r + 1) DSEL_RANGE): dsel_rank_kernel counts
//                (below, equal) per range, dsel_scan_kernel turns the counts into
//                offsets (one workgroup per query), dsel_compact_kernel writes
//                (key << 32 | slot) at the offsets and pads up to k with all-ones.
//   D4 sort    : rocPRIM merge sort of the k entries of each query (block sort +
//                merge-path passes: no look-back between workgroups), temporary
//                storage from the workspace.
//   D5 emit    : ids (id_base + slot), dists, padding, counts.
//
// The results are wvg_search's for each query alone, bit for bit: the keys are
// the same per-lane distance code, and (key, slot) ascending with the tie rule
// above is the first k of the host path's "sort everything <= thr".
#include <rocprim/device/device_merge_sort.hpp>

#include "wvg_host.hpp"
#include "wvg_rowdist.hpp"

namespace wvg {

constexpr uint32_t DSEL_DEAD = 0xFFFFFFFFu;  // ORD_NONE of wvg_select.hip
constexpr uint32_t DSEL_RANGE = 2048;        // slots per compaction workgroup
constexpr int DSEL_BINS = 4096;

struct DselState {
    uint32_t prefix, mask;      // keys with (key & mask) == prefix are the candidates; at the end prefix = thr
    unsigned long long krem;    // rank of the wanted key among them; at the end the equal rows to take
};

// ---- D1: shared-row keys ---------------------------------------------------------
struct DselKeysArgs {
    const float4 *data;
    const uint64_t *valid;
    const float *queries;  // the group's first query
    uint32_t qpitch;       // floats between queries (a multiple of 4)
    uint32_t gq;           // queries present in this group (<= G)
    uint64_t tile_begin, tile_end;
    uint32_t dim, nchunks;
    int metric;
    uint32_t *keys;        // [G][key_stride]
    uint64_t key_stride;
};

// row_dot_or_l2_generic<METRIC, 64> for gq queries at once: per query the 4 x 8
// accumulators over the 32-blocks, the leftover 8-blocks into acc[0], the scalar
// tail (dim % 4 == 0: whole chunks, element by element), avx256_reduce.
template <int METRIC, int G>
__global__ __launch_bounds__(256) void dsel_keys_f32_kernel(DselKeysArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint64_t ntiles = a.tile_end - a.tile_begin;
    const uint64_t gw = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t gq = a.gq;
    const int n = (int)a.dim;
    const int nb = n >> 5;
    for (uint64_t i = gw; i < ntiles; i += nw) {
        const uint64_t t = a.tile_begin + i;
        const uint64_t m = a.valid[t];
        if (m == 0ull) {  // no live row: nothing to read
#pragma unroll
            for (int g = 0; g < G; g++)
                if ((uint32_t)g < gq) a.keys[(size_t)g * a.key_stride + i * 64 + lane] = DSEL_DEAD;
            continue;
        }
        const float4 *p = a.data + (size_t)t * a.nchunks * 64 + lane;
        float acc[G][4][8];
        float sum[G];
#pragma unroll
        for (int g = 0; g < G; g++) {
            sum[g] = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int l = 0; l < 8; l++) acc[g][j][l] = 0.0f;
        }
        // the next 32-block's chunks are loaded before this one's arithmetic: at two waves per SIMD
        // a wave has to cover its own load latency
        float4 xs[8];
        if (nb > 0) {
#pragma unroll
            for (int cc = 0; cc < 8; cc++) xs[cc] = p[(size_t)cc * 64];
        }
        for (int b = 0; b < nb; b++) {
            float4 xn[8];
            if (b + 1 < nb) {
#pragma unroll
                for (int cc = 0; cc < 8; cc++) xn[cc] = p[(size_t)((b + 1) * 8 + cc) * 64];
            } else {
#pragma unroll
                for (int cc = 0; cc < 8; cc++) xn[cc] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
#pragma unroll
            for (int g = 0; g < G; g++) {
                if ((uint32_t)g < gq) {
                    const float4 *q4 = reinterpret_cast<const float4 *>(a.queries + (size_t)g * a.qpitch);
#pragma unroll
                    for (int cc = 0; cc < 8; cc++) chunk_update<METRIC>(acc[g], cc, q4[b * 8 + cc], xs[cc]);
                }
            }
#pragma unroll
            for (int cc = 0; cc < 8; cc++) xs[cc] = xn[cc];
        }
        int pos = nb * 32, rem = n - pos;
        while (rem >= 8) {
            const int c = pos >> 2;
            const float4 x0 = p[(size_t)c * 64], x1 = p[(size_t)(c + 1) * 64];
#pragma unroll
            for (int g = 0; g < G; g++) {
                if ((uint32_t)g < gq) {
                    const float4 *q4 = reinterpret_cast<const float4 *>(a.queries + (size_t)g * a.qpitch);
                    chunk_update<METRIC>(acc[g], 0, q4[c], x0);
                    chunk_update<METRIC>(acc[g], 1, q4[c + 1], x1);
                }
            }
            pos += 8;
            rem -= 8;
        }
        if (rem) {  // 4 elements: one chunk, in element order
            const int c = pos >> 2;
            const float4 x = p[(size_t)c * 64];
#pragma unroll
            for (int g = 0; g < G; g++) {
                if ((uint32_t)g < gq) {
                    const float4 q = reinterpret_cast<const float4 *>(a.queries + (size_t)g * a.qpitch)[c];
                    scalar_update<METRIC>(sum[g], q.x, x.x);
                    scalar_update<METRIC>(sum[g], q.y, x.y);
                    scalar_update<METRIC>(sum[g], q.z, x.z);
                    scalar_update<METRIC>(sum[g], q.w, x.w);
                }
            }
        }
        const bool live = (m >> lane) & 1ull;
#pragma unroll
        for (int g = 0; g < G; g++) {
            if ((uint32_t)g < gq) {
                const float r = avx256_reduce(acc[g], sum[g]);
                a.keys[(size_t)g * a.key_stride + i * 64 + lane] =
                    live ? wvg_ord_f32(wrap_metric(a.metric, r)) : DSEL_DEAD;
            }
        }
    }
}

// ---- D2: batched radix select ------------------------------------------------------
// One workgroup per query: the select state and a clear histogram.  take_all:
// k covers every slot, so there is no select: thr = DSEL_DEAD keeps every live key.
__global__ __launch_bounds__(256) void dsel_init_kernel(DselState *st, uint32_t *hist, unsigned long long k, int take_all)
{
    const uint32_t g = blockIdx.x;
    if (threadIdx.x == 0) {
        DselState s;
        s.prefix = take_all ? DSEL_DEAD : 0u;
        s.mask = take_all ? 0xFFFFFFFFu : 0u;
        s.krem = take_all ? 0ull : k;
        st[g] = s;
    }
    for (int i = threadIdx.x; i < DSEL_BINS; i += blockDim.x) hist[(size_t)g * DSEL_BINS + i] = 0u;
}

// grid (blocks, gq): key_hist_kernel with the query as blockIdx.y.
__global__ __launch_bounds__(256) void dsel_hist_kernel(const uint32_t *keys, uint64_t n, uint64_t key_stride,
                                                        const DselState *st, int shift, int bits, uint32_t *hist)
{
    __shared__ uint32_t h[DSEL_BINS];
    const uint32_t g = blockIdx.y;
    keys += (size_t)g * key_stride;
    hist += (size_t)g * DSEL_BINS;
    for (int i = threadIdx.x; i < DSEL_BINS; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const uint32_t prefix = st[g].prefix, mask = st[g].mask;
    const uint32_t dmask = (1u << bits) - 1u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t k = keys[i];
        if ((k & mask) == prefix) atomicAdd(&h[(k >> shift) & dmask], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < DSEL_BINS; i += blockDim.x)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// grid (gq): key_pick_kernel's choice per query -- the digit whose cumulative count reaches krem --
// with the 256 partial sums scanned by the workgroup; clears the query's histogram for the next pass.
__global__ __launch_bounds__(256) void dsel_pick_kernel(DselState *st, uint32_t *hist, int shift, int bits)
{
    __shared__ unsigned long long part[256];
    const uint32_t g = blockIdx.x;
    st += g;
    hist += (size_t)g * DSEL_BINS;
    const int tid = threadIdx.x;
    const int nb = 1 << bits, per = nb / 256;
    unsigned long long loc = 0;
    for (int j = 0; j < per; j++) loc += hist[tid * per + j];
    part[tid] = loc;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {  // inclusive scan
        const unsigned long long v = tid >= off ? part[tid - off] : 0ull;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    const unsigned long long krem = st->krem, incl = part[tid], excl = incl - loc;
    // the first group of bins whose inclusive count reaches krem (krem >= 1), else the last one
    if ((excl < krem && incl >= krem) || (tid == 255 && incl < krem)) {
        unsigned long long cum = excl;
        int d = tid * per;
        for (;; d++) {
            const unsigned long long c = hist[d];
            if (cum + c >= krem || d == tid * per + per - 1) break;
            cum += c;
        }
        st->krem = krem - cum;
        st->prefix |= (uint32_t)d << shift;
        st->mask |= (uint32_t)(nb - 1) << shift;
    }
    __syncthreads();
    for (int i = tid; i < DSEL_BINS; i += 256) hist[i] = 0;
}

// ---- D3: exact-count compaction ------------------------------------------------------
// Per (range, query): rc[2 r] = live keys below thr, rc[2 r + 1] = live keys equal to thr.
__global__ __launch_bounds__(256) void dsel_rank_kernel(const uint32_t *keys, uint64_t n, uint64_t key_stride,
                                                        const DselState *st, uint32_t nranges, uint32_t *rc)
{
    __shared__ uint32_t wsum[2][4];
    const uint32_t g = blockIdx.y, r = blockIdx.x;
    keys += (size_t)g * key_stride;
    const uint32_t thr = st[g].prefix;
    const uint64_t lo = (uint64_t)r * DSEL_RANGE;
    uint32_t below = 0, equal = 0;
    for (uint32_t j = threadIdx.x; j < DSEL_RANGE; j += 256) {
        const uint64_t i = lo + j;
        const uint32_t k = i < n ? keys[i] : DSEL_DEAD;
        below += k < thr;
        equal += k == thr && k != DSEL_DEAD;
    }
    for (int off = 32; off > 0; off >>= 1) {
        below += __shfl_down(below, off);
        equal += __shfl_down(equal, off);
    }
    if ((threadIdx.x & 63) == 0) {
        wsum[0][threadIdx.x >> 6] = below;
        wsum[1][threadIdx.x >> 6] = equal;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t *o = rc + ((size_t)g * nranges + r) * 2;
        o[0] = wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
        o[1] = wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
    }
}

// grid (gq): the range counts become exclusive offsets in place; tot[2 g] = keys below
// thr, tot[2 g + 1] = result entries = below + min(krem, equal) = min(k, live).
__global__ __launch_bounds__(256) void dsel_scan_kernel(const DselState *st, uint32_t nranges, uint32_t *rc,
                                                        uint32_t *tot)
{
    __shared__ uint32_t sb[256], se[256];
    const uint32_t g = blockIdx.x;
    rc += (size_t)g * nranges * 2;
    const int tid = threadIdx.x;
    const uint32_t per = (nranges + 255) / 256;
    const uint32_t r0 = min((uint32_t)tid * per, nranges), r1 = min(r0 + per, nranges);
    uint32_t b = 0, e = 0;
    for (uint32_t r = r0; r < r1; r++) {
        b += rc[2 * r];
        e += rc[2 * r + 1];
    }
    sb[tid] = b;
    se[tid] = e;
    __syncthreads();
    if (tid == 0) {
        uint32_t cb = 0, ce = 0;
        for (int i = 0; i < 256; i++) {
            const uint32_t vb = sb[i], ve = se[i];
            sb[i] = cb;
            se[i] = ce;
            cb += vb;
            ce += ve;
        }
        const unsigned long long krem = st[g].krem;
        tot[2 * g] = cb;
        tot[2 * g + 1] = cb + (uint32_t)(krem < ce ? krem : ce);
    }
    __syncthreads();
    b = sb[tid];
    e = se[tid];
    for (uint32_t r = r0; r < r1; r++) {
        const uint32_t vb = rc[2 * r], ve = rc[2 * r + 1];
        rc[2 * r] = b;
        rc[2 * r + 1] = e;
        b += vb;
        e += ve;
    }
}

// grid (nranges, gq): out[g][.] = (key << 32 | slot) of the range's kept rows at the
// scanned offsets -- the keys below thr first, then the first krem equal ones in slot
// order -- and the workgroups together pad [count, k) with all-ones entries.
__global__ __launch_bounds__(256) void dsel_compact_kernel(const uint32_t *keys, uint64_t n, uint64_t key_stride,
                                                           const DselState *st, uint32_t nranges, const uint32_t *rc,
                                                           const uint32_t *tot, uint32_t slot0, uint64_t k,
                                                           uint64_t *out)
{
    __shared__ uint32_t wcnt[2][4];
    const uint32_t g = blockIdx.y, r = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    keys += (size_t)g * key_stride;
    out += (size_t)g * k;
    const uint32_t thr = st[g].prefix;
    const unsigned long long krem = st[g].krem;
    const uint32_t nbelow = tot[2 * g], count = tot[2 * g + 1];
    uint32_t bbase = rc[((size_t)g * nranges + r) * 2], ebase = rc[((size_t)g * nranges + r) * 2 + 1];
    const uint64_t lo = (uint64_t)r * DSEL_RANGE;
    for (uint32_t j0 = 0; j0 < DSEL_RANGE; j0 += 256) {  // 256 consecutive slots per step, in slot order
        const uint64_t i = lo + j0 + threadIdx.x;
        const uint32_t key = i < n ? keys[i] : DSEL_DEAD;
        const bool isb = key < thr, ise = key == thr && key != DSEL_DEAD;
        const uint64_t mb = __ballot(isb), me = __ballot(ise);
        if (lane == 0) {
            wcnt[0][w] = (uint32_t)__popcll(mb);
            wcnt[1][w] = (uint32_t)__popcll(me);
        }
        __syncthreads();
        uint32_t pb = 0, pe = 0, tb = 0, te = 0;
#pragma unroll
        for (int x = 0; x < 4; x++) {
            pb += x < w ? wcnt[0][x] : 0u;
            pe += x < w ? wcnt[1][x] : 0u;
            tb += wcnt[0][x];
            te += wcnt[1][x];
        }
        const uint64_t lower = (1ull << lane) - 1ull;
        const uint64_t entry = ((uint64_t)key << 32) | (uint32_t)(slot0 + (uint32_t)i);
        if (isb) out[bbase + pb + (uint32_t)__popcll(mb & lower)] = entry;
        if (ise) {
            const unsigned long long e = (unsigned long long)ebase + pe + (uint32_t)__popcll(me & lower);
            if (e < krem) out[nbelow + e] = entry;
        }
        bbase += tb;
        ebase += te;
        __syncthreads();
    }
    for (uint64_t i = (uint64_t)count + (uint64_t)r * 256 + threadIdx.x; i < k; i += (uint64_t)nranges * 256)
        out[i] = WVG_KEY_NONE;
}

// ---- D5: emit ---------------------------------------------------------------------------
// grid (blocks, gq): sorted [gq][k] -> the group's rows of ids / dists / counts.
__global__ __launch_bounds__(256) void dsel_emit_kernel(const uint64_t *sorted, uint64_t k, const uint32_t *tot,
                                                        uint64_t id_base, uint64_t *ids, float *dists,
                                                        uint32_t *counts)
{
    const uint32_t g = blockIdx.y;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && counts) counts[g] = tot[2 * g + 1];
    if (i >= k) return;
    const uint64_t e = sorted[(size_t)g * k + i];
    const bool live = e != WVG_KEY_NONE;
    if (ids) ids[(size_t)g * k + i] = live ? id_base + (uint32_t)e : WVG_KEY_NONE;
    if (dists) dists[(size_t)g * k + i] = live ? wvg_unord_f32((uint32_t)(e >> 32)) : __builtin_inff();
}

// ---- host -------------------------------------------------------------------------------
static size_t dsel_sort_temp_bytes(uint64_t k)
{
    size_t bytes = 0;
    (void)rocprim::merge_sort(nullptr, bytes, (const unsigned long long *)nullptr, (unsigned long long *)nullptr,
                              (size_t)k, rocprim::less<unsigned long long>(), (hipStream_t)0);
    return bytes;
}

// The workspace behind the status block.
struct DselLayout {
    size_t keys = 0, st = 0, hist = 0, rc = 0, tot = 0, cmp = 0, sorted = 0, temp = 0, queries = 0, total = 0;
    size_t temp_bytes = 0;
    uint32_t nranges = 0;
};
static DselLayout dsel_layout(const wvg_corpus *c, uint64_t nslots, uint32_t nq, uint32_t k)
{
    DselLayout l;
    Carver cv;
    l.nranges = (uint32_t)((nslots + DSEL_RANGE - 1) / DSEL_RANGE);
    l.temp_bytes = dsel_sort_temp_bytes(k);
    l.keys = cv.take((size_t)DSEL_G * nslots * 4);
    l.st = cv.take((size_t)DSEL_G * sizeof(DselState));
    l.hist = cv.take((size_t)DSEL_G * DSEL_BINS * 4);
    l.rc = cv.take((size_t)DSEL_G * l.nranges * 8);
    l.tot = cv.take((size_t)DSEL_G * 8);
    l.cmp = cv.take((size_t)DSEL_G * k * 8);
    l.sorted = cv.take((size_t)DSEL_G * k * 8);
    l.temp = cv.take(l.temp_bytes);
    l.queries = cv.take(device_query_bytes(c, nq));
    l.total = cv.off;
    return l;
}

size_t dsel_workspace_bytes(const wvg_corpus *c, uint64_t nslots, uint32_t nq, uint32_t k)
{
    return dsel_layout(c, nslots, nq, k).total;
}

static bool dsel_shares_rows(const wvg_corpus *c)
{
    return c->kind == WVG_KIND_F32 && !c->ctx->order512 && c->dim >= 8 && c->dim % 4 == 0 &&
           (c->metric == WVG_METRIC_L2 || c->metric == WVG_METRIC_DOT || c->metric == WVG_METRIC_COSINE);
}

static hipError_t launch_dsel_keys(const DselKeysArgs &a, int num_cus, hipStream_t s)
{
    const uint64_t ntiles = a.tile_end - a.tile_begin;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((ntiles + 3) / 4, (uint64_t)num_cus * 8));
    with_metric(a.metric, [&](auto M) {
        constexpr int MT = decltype(M)::value;
        if constexpr (MT == WVG_M_L2 || MT == WVG_M_DOT)
            hipLaunchKernelGGL((dsel_keys_f32_kernel<MT, DSEL_G>), dim3(grid), dim3(256), 0, s, a);
    });
    return hipGetLastError();
}

// wvg_search_device for k > MAX_K.  ws: the workspace behind its status block, ws_bytes of it.
// Checks first, then launches: on any error nothing has been launched.
int dsel_search(wvg_corpus *c, const float *d_queries, uint32_t nq, uint32_t k, const SearchPlan &p, uint64_t *d_ids,
                float *d_dists, uint32_t *d_counts, char *ws, size_t ws_bytes, hipStream_t s)
{
    const uint64_t ntiles = p.te - p.tb, nslots = ntiles * 64;
    if (p.te * 64 > (1ull << 32))
        return fail(WVG_ERR_UNSUPPORTED, "device search with k above 256 holds the slot in 32 bits");
    const DselLayout l = dsel_layout(c, nslots, nq, k);
    if (!ws || ws_bytes < l.total) return fail(WVG_ERR_INVALID, "workspace too small");
    const int cus = c->ctx->num_cus;
    uint32_t *keys = (uint32_t *)(ws + l.keys), *hist = (uint32_t *)(ws + l.hist);
    uint32_t *rc = (uint32_t *)(ws + l.rc), *tot = (uint32_t *)(ws + l.tot);
    DselState *st = (DselState *)(ws + l.st);
    uint64_t *cmp = (uint64_t *)(ws + l.cmp), *sorted = (uint64_t *)(ws + l.sorted);
    char *qbuf = ws + l.queries;
    const bool shared = dsel_shares_rows(c);
    const bool take_all = (uint64_t)k >= nslots;

    // the queries as the key kernels take them: F32 rows as given, PQ LUTs, BQ codes at the scan's pitch
    const char *dq = (const char *)d_queries;
    uint32_t qpitch = c->dim;
    size_t qbytes = (size_t)c->dim * 4;
    if (c->kind == WVG_KIND_PQ) {  // (CH/product_quantization.go:329-337)
        WVG_HIP(launch_pq_lut(c->metric, d_queries, nq, c->dim, c->d_centers, c->pq_m, c->pq_ks, c->pq_ds,
                              (float *)qbuf, s));
        dq = qbuf;
        qpitch = c->pq_m * c->pq_ks;
        qbytes = (size_t)qpitch * 4;
    } else if (c->kind == WVG_KIND_BQ) {  // sign bits (CH/binary_quantization.go:32-45)
        const uint32_t words = bq_words(c->dim);
        qpitch = bq_chunks(c->dim) * 2;
        uint64_t *codes = (uint64_t *)(qbuf + align_up((size_t)nq * qpitch * 8, 256));
        WVG_HIP(launch_bq_encode_rows(d_queries, nq, c->dim, 0, codes, s));
        WVG_HIP(hipMemsetAsync(qbuf, 0, (size_t)nq * qpitch * 8, s));
        WVG_HIP(hipMemcpy2DAsync(qbuf, (size_t)qpitch * 8, codes, (size_t)words * 8, (size_t)words * 8, nq,
                                 hipMemcpyDeviceToDevice, s));
        dq = qbuf;
        qbytes = (size_t)qpitch * 8;
    }

    const unsigned hgrid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nslots + 1023) / 1024, (uint64_t)cus * 4));
    const unsigned egrid = (unsigned)(((uint64_t)k + 255) / 256);
    for (uint32_t q0 = 0; q0 < nq; q0 += DSEL_G) {
        const uint32_t gq = std::min<uint32_t>(DSEL_G, nq - q0);
        // D1
        if (shared) {
            DselKeysArgs a{};
            a.data = (const float4 *)c->d_data;
            a.valid = c->d_valid;
            a.queries = (const float *)(dq + (size_t)q0 * qbytes);
            a.qpitch = qpitch;
            a.gq = gq;
            a.tile_begin = p.tb;
            a.tile_end = p.te;
            a.dim = c->dim;
            a.nchunks = c->nchunks;
            a.metric = c->metric;
            a.keys = keys;
            a.key_stride = nslots;
            WVG_HIP(launch_dsel_keys(a, cus, s));
        } else {
            for (uint32_t g = 0; g < gq; g++) {
                const ScanArgs a1 = scan_args_for(c, dq + (size_t)(q0 + g) * qbytes, qpitch, 1, k, nullptr, p.tb, p.te);
                WVG_HIP(launch_ordkeys(a1, c->kind, cus, keys + (size_t)g * nslots, s));
            }
        }
        // D2
        hipLaunchKernelGGL(dsel_init_kernel, dim3(gq), dim3(256), 0, s, st, hist, (unsigned long long)k,
                           take_all ? 1 : 0);
        if (!take_all) {
            const int shifts[3] = {20, 8, 0}, bits[3] = {12, 12, 8};
            for (int ps = 0; ps < 3; ps++) {
                hipLaunchKernelGGL(dsel_hist_kernel, dim3(hgrid, gq), dim3(256), 0, s, (const uint32_t *)keys, nslots,
                                   nslots, (const DselState *)st, shifts[ps], bits[ps], hist);
                hipLaunchKernelGGL(dsel_pick_kernel, dim3(gq), dim3(256), 0, s, st, hist, shifts[ps], bits[ps]);
            }
        }
        // D3
        hipLaunchKernelGGL(dsel_rank_kernel, dim3(l.nranges, gq), dim3(256), 0, s, (const uint32_t *)keys, nslots,
                           nslots, (const DselState *)st, l.nranges, rc);
        hipLaunchKernelGGL(dsel_scan_kernel, dim3(gq), dim3(256), 0, s, (const DselState *)st, l.nranges, rc, tot);
        hipLaunchKernelGGL(dsel_compact_kernel, dim3(l.nranges, gq), dim3(256), 0, s, (const uint32_t *)keys, nslots,
                           nslots, (const DselState *)st, l.nranges, (const uint32_t *)rc, (const uint32_t *)tot,
                           (uint32_t)(p.tb * 64), (uint64_t)k, cmp);
        WVG_HIP(hipGetLastError());
        // D4
        for (uint32_t g = 0; g < gq; g++) {
            size_t tb = l.temp_bytes;
            WVG_HIP(rocprim::merge_sort(ws + l.temp, tb, (const unsigned long long *)(cmp + (size_t)g * k),
                                        (unsigned long long *)(sorted + (size_t)g * k), (size_t)k,
                                        rocprim::less<unsigned long long>(), s));
        }
        // D5
        hipLaunchKernelGGL(dsel_emit_kernel, dim3(egrid, gq), dim3(256), 0, s, (const uint64_t *)sorted, (uint64_t)k,
                           (const uint32_t *)tot, c->id_base, d_ids ? d_ids + (size_t)q0 * k : nullptr,
                           d_dists ? d_dists + (size_t)q0 * k : nullptr, d_counts ? d_counts + q0 : nullptr);
        WVG_HIP(hipGetLastError());
    }
    return WVG_OK;
}

}  // namespace wvg

// wvg_bq_qshare.hip -- the shared-row query stream of BQ corpora
// (wvg_search_device_pipelined[_filtered] on a WVG_KIND_BQ corpus, nq >= 2).
//
// K5 (wvg_bq.hip) gives every (query, row range) a workgroup of its own, so a
// batch of nq queries reads the codes nq times.  Here a wave loads a 64-row tile
// once and scores it against every query of its pass: the grid is (row ranges,
// passes), pass p serves queries [p Q, min(nq, (p + 1) Q)), each with a
// WaveTopK of its own in registers.  The tile's chunks are vector registers,
// the queries' words wave-uniform scalar loads, a distance XOR + popcount: an
// integer, so the results are those of nq separate K5 scans bit for bit.  Two
// plain launches, this scan and launch_merge_lists; no workgroup waits for
// another.  Tiled layout as K5: [tile][chunk][lane][2 x u64], lane = row.
#include "wvg_internal.hpp"
#include "wvg_topk.hpp"

namespace wvg {

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// Queries per pass.  All per-query state (the lists, their thresholds) is indexed by
// compile-time indices only, so it stays in registers; at 8 the largest form (E = 4,
// NCH = 12) holds 8 lists x 8 + two tiles x 48 VGPRs and still runs two waves per SIMD.
// One value for every (chunk count, k) until a measured table replaces it.
constexpr int BQ_QSHARE_Q = 8;

uint32_t bq_qshare_queries_per_pass(uint32_t nchunks, uint32_t k)
{
    (void)nchunks;
    (void)k;
    return (uint32_t)BQ_QSHARE_Q;
}

// Row ranges of a shared-row BQ scan of ntiles tiles: every wave of the 4-wave
// workgroups gets at least two tiles where the corpus has them (the fixed-NCH forms
// prefetch the next tile), and at most two workgroups per CU -- what the largest form's
// registers let a CU hold at once, so a pass is one round of workgroups (K5's own cap
// is three of its smaller workgroups per CU, plan_search; with three here a 16-query launch over
// 100M x 1536 took 14.03 instead of 12.43 ms at k = 200 and 7.08 instead of 7.23 ms at k = 10,
// profiles/r19/bq_stream/ranges_per_cu_ab.jsonl).
uint32_t bq_qshare_groups(uint64_t ntiles, int num_cus)
{
    const uint64_t cap = 2ull * (uint64_t)std::max(num_cus, 1);
    return (uint32_t)std::min<uint64_t>(cap, std::max<uint64_t>(1, ntiles / (2 * BQ_SCAN_WAVES)));
}

// Query j's allow word of tile t (BQShareArgs: word t - allow_t0, zero outside the window).
__device__ __forceinline__ uint64_t bq_qshare_allow(const BQShareArgs &a, uint32_t q, uint64_t t)
{
    const uint64_t w = t - a.allow_t0;
    return w < a.allow_stride ? a.allow[(size_t)q * a.allow_stride + w] : 0ull;
}

// Code loads: the default cache policy (PLAIN) or non-temporal.  A template argument, not a run-time
// branch: the compiler merges the two arms of such a branch into one load and drops the hint.
template <bool PLAIN>
__device__ __forceinline__ u64x2 ld_codes(const u64x2 *p)
{
    if constexpr (PLAIN)
        return *p;
    else
        return __builtin_nontemporal_load(p);
}

template <int NCH, bool PLAIN>
__device__ __forceinline__ void load_tile(u64x2 (&dst)[NCH], const u64x2 *data, uint64_t t, int lane)
{
    const u64x2 *rp = data + (size_t)t * NCH * 64 + lane;
#pragma unroll
    for (int c = 0; c < NCH; c++) dst[c] = ld_codes<PLAIN>(rp + (size_t)c * 64);
}

// E: 64-key registers per list (k <= 64 E).  NCH: 1 / 6 / 12 fixed, the next live tile's
// chunks loaded while this one is scored; 0 = the generic loop over a.nchunks, every chunk
// loaded once and scored against the pass's queries.  FILT: per-query allow words.  PLAIN: ld_codes.
// No global store inside the scan loop (WaveTopK::offer_dist_emit explains what one costs).
template <int E, int NCH, int Q, bool FILT, bool PLAIN>
__global__ __launch_bounds__(BQ_SCAN_WAVES * 64) void scan_bq_qshare_kernel(BQShareArgs a)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t rng = blockIdx.x, G = gridDim.x, q0 = blockIdx.y * Q;
    const uint32_t nqp = min((uint32_t)Q, a.nq - q0);  // queries of this pass (>= 1: gridDim.y = ceil(nq / Q))
    const bool rev = ((a.reverse + blockIdx.y) & 1u) != 0u;  // one direction per pass
    const uint64_t *qb = a.queries + (size_t)q0 * a.qpitch;
    const u64x2 *data = reinterpret_cast<const u64x2 *>(a.data);
    const uint64_t ntiles = a.tile_end - a.tile_begin;
    const uint64_t total = (uint64_t)G * BQ_SCAN_WAVES;
    const uint64_t gw = (uint64_t)rng * BQ_SCAN_WAVES + wave;
    const uint64_t t0 = a.tile_begin + ntiles * gw / total, t1 = a.tile_begin + ntiles * (gw + 1) / total;
    const uint64_t n = t1 - t0;  // the wave walks i = 0 .. n - 1, tile t0 + i upwards or t1 - 1 - i downwards
    WaveTopK<E> tk[Q];
#pragma unroll
    for (int j = 0; j < Q; j++) {
        tk[j].init((int)a.k);
        tk[j].init_fast();
    }
    auto tile_of = [&](uint64_t i) { return rev ? t1 - 1 - i : t0 + i; };
    // live rows of tile t some query of the pass may take (wave-uniform)
    auto live_word = [&](uint64_t t) {
        uint64_t v = a.valid[t];
        if constexpr (FILT) {
            uint64_t u = 0ull;
#pragma unroll
            for (int j = 0; j < Q; j++)
                if ((uint32_t)j < nqp) u |= bq_qshare_allow(a, q0 + j, t);
            v &= u;
        }
        return v;
    };
    // first i' >= i whose tile has such a row (n if none), its word in m
    auto next_live = [&](uint64_t i, uint64_t &m) {
        for (; i < n; ++i) {
            m = live_word(tile_of(i));
            if (m) break;
        }
        return i;
    };
    if constexpr (NCH > 0) {
        // The tile being scored lives in `cur`, a copy of the registers the loads fill: the copy at the top
        // of an iteration is the one place that waits for loads (issued a whole tile's scoring earlier),
        // and nothing scored below depends on a load in flight.
        u64x2 cur[NCH], nxt[NCH];
        uint64_t m_nxt = 0;
        uint64_t i = next_live(0, m_nxt);
        if (i < n) load_tile<NCH, PLAIN>(nxt, data, tile_of(i), lane);
        while (i < n) {
#pragma unroll
            for (int c = 0; c < NCH; c++) cur[c] = nxt[c];
            const uint64_t t = tile_of(i), m_cur = m_nxt;
            i = next_live(i + 1, m_nxt);
            if (i < n) load_tile<NCH, PLAIN>(nxt, data, tile_of(i), lane);
#pragma unroll
            for (int j = 0; j < Q; j++) {
                if ((uint32_t)j < nqp) {
                    uint64_t m = m_cur;
                    if constexpr (FILT) m &= bq_qshare_allow(a, q0 + j, t);
                    if (m) {
                        const uint64_t *q = qb + (size_t)j * a.qpitch;
                        uint32_t tot = 0;
#pragma unroll
                        for (int c = 0; c < NCH; c++)
                            tot += (uint32_t)__popcll(cur[c].x ^ q[2 * c]) + (uint32_t)__popcll(cur[c].y ^ q[2 * c + 1]);
                        // exact: an integer < 2^24
                        tk[j].offer_dist_fast((float)tot, (uint32_t)(t * 64 + lane), m);
                    }
                }
            }
        }
    } else {
        const uint32_t nch = a.nchunks;
        uint64_t m_all = 0;
        for (uint64_t i = next_live(0, m_all); i < n; i = next_live(i + 1, m_all)) {
            const uint64_t t = tile_of(i);
            uint64_t mq[Q];
            uint32_t tot[Q];
#pragma unroll
            for (int j = 0; j < Q; j++) {
                mq[j] = (uint32_t)j < nqp ? m_all : 0ull;
                if constexpr (FILT) {
                    if ((uint32_t)j < nqp) mq[j] &= bq_qshare_allow(a, q0 + j, t);
                }
                tot[j] = 0;
            }
            const u64x2 *rp = data + (size_t)t * nch * 64 + lane;
            for (uint32_t c = 0; c < nch; c++) {
                const u64x2 x = ld_codes<PLAIN>(rp + (size_t)c * 64);
#pragma unroll
                for (int j = 0; j < Q; j++) {
                    if (mq[j]) {
                        const uint64_t *q = qb + (size_t)j * a.qpitch;
                        tot[j] += (uint32_t)__popcll(x.x ^ q[2 * c]) + (uint32_t)__popcll(x.y ^ q[2 * c + 1]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < Q; j++)
                if (mq[j]) tk[j].offer_dist_fast((float)tot[j], (uint32_t)(t * 64 + lane), mq[j]);
        }
    }
    // one list per (query, range); group_combine_store reuses one LDS buffer, hence the barrier
    // between queries (the q < nq test is the same for the whole workgroup)
#pragma unroll
    for (int j = 0; j < Q; j++) {
        if ((uint32_t)j < nqp) {
            if (j > 0) __syncthreads();
            group_combine_store<E, BQ_SCAN_WAVES>(tk[j], a.partials + ((size_t)(q0 + j) * G + rng) * a.k);
        }
    }
}

template <int E, int NCH>
static void launch_bq_qshare_f(const BQShareArgs &a, dim3 grid, hipStream_t s)
{
    const dim3 block(BQ_SCAN_WAVES * 64);
    if (a.allow) {
        if (a.plain)
            launch_timed((scan_bq_qshare_kernel<E, NCH, BQ_QSHARE_Q, true, true>), grid, block, 0, s, a);
        else
            launch_timed((scan_bq_qshare_kernel<E, NCH, BQ_QSHARE_Q, true, false>), grid, block, 0, s, a);
    } else {
        if (a.plain)
            launch_timed((scan_bq_qshare_kernel<E, NCH, BQ_QSHARE_Q, false, true>), grid, block, 0, s, a);
        else
            launch_timed((scan_bq_qshare_kernel<E, NCH, BQ_QSHARE_Q, false, false>), grid, block, 0, s, a);
    }
}

template <int E>
static void launch_bq_qshare_n(const BQShareArgs &a, dim3 grid, hipStream_t s)
{
    switch (a.nchunks) {
    case 1: launch_bq_qshare_f<E, 1>(a, grid, s); break;    // d <= 128
    case 6: launch_bq_qshare_f<E, 6>(a, grid, s); break;    // d = 768
    case 12: launch_bq_qshare_f<E, 12>(a, grid, s); break;  // d = 1536
    default: launch_bq_qshare_f<E, 0>(a, grid, s); break;
    }
}

hipError_t launch_scan_bq_qshare(const BQShareArgs &a, uint32_t groups, hipStream_t s)
{
    const uint32_t qpp = bq_qshare_queries_per_pass(a.nchunks, a.k);
    const uint32_t passes = (a.nq + qpp - 1) / qpp;
    if (a.k == 0 || a.k > 256 || a.nq == 0 || groups == 0 || passes > 65535u || qpp != (uint32_t)BQ_QSHARE_Q)
        return hipErrorInvalidValue;
    const dim3 grid(groups, passes);
    if (a.k <= 64)
        launch_bq_qshare_n<1>(a, grid, s);
    else if (a.k <= 128)
        launch_bq_qshare_n<2>(a, grid, s);
    else
        launch_bq_qshare_n<4>(a, grid, s);
    return hipGetLastError();
}

}  // namespace wvg

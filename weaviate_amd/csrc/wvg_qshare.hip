// wvg_qshare.hip -- the shared-row query stream of wvg_search_device_pipelined
// (QShareArgs, wvg_internal.hpp): the queries of a pass are scored against each
// 64-row tile while the tile is in registers, so a pass reads every row once
// whatever its number of queries.
//
// Each query's distance is the chain of a scan of its own (chunk_update in chunk
// order, avx256_reduce) and its keys go to a WaveTopK of its own, so the lists
// -- and the merged results -- are those of scan_f32_stream_kernel bit for bit.
//  WHOLE (d = 128): the lane's whole row is loaded (D / 4 float4) and the QP
//    queries are folded one after another, 32 accumulators live at a time.
//  blocks (d = 768, and d = 128 in the tools build for A/B): K1Q's body -- a
//    32-float block of the row is loaded and folded into the QP queries' chains
//    (QP x 32 accumulators live through the row).
// The query words and tile masks are wave-uniform and read through the constant
// address space: the publishes of the previous pass would otherwise make them
// "maybe clobbered" vector loads (wvg_topk.hpp, offer_dist_emit).  Nothing
// writes the queries or the validity words while the kernel runs.
// Workgroups 0..groups-1 scan and never wait; workgroups groups.. merge, merger
// m the queries m, m + mergers, ...: the waiting workgroups have the highest
// ids, so every workgroup they wait for is dispatched before them.
// Roofline: one HBM read of the rows per pass against nq x rows x d (sub, fma)
// pairs on the VALU.
#include <algorithm>

#include "wvg_internal.hpp"
#include "wvg_rowdist.hpp"
#include "wvg_stream.hpp"
#include "wvg_topk.hpp"

namespace wvg {

typedef __attribute__((address_space(4))) const f4v cf4;
typedef __attribute__((address_space(4))) const uint64_t cu64;

// chunk_update on pairs: acc[r][p] holds chains l = 2p, 2p + 1 of row r of the
// AVX2 accumulators, so a chunk is two packed subtractions and two packed fmas
// (v_pk_add_f32 / v_pk_fma_f32: per element the operations of acc_update) whose
// query operands are aligned scalar pairs as the scalar loads deliver them.
typedef float f2v __attribute__((ext_vector_type(2)));

template <int METRIC>
__device__ __forceinline__ void chunk_update2(f2v (&acc)[4][4], int cc, f4v q, float4 x)
{
    const int r = cc >> 1, p = (cc & 1) * 2;
    const f2v qlo = {q.x, q.y}, qhi = {q.z, q.w}, xlo = {x.x, x.y}, xhi = {x.z, x.w};
    if constexpr (METRIC == WVG_M_L2) {
        const f2v dl = qlo - xlo, dh = qhi - xhi;
        acc[r][p] = __builtin_elementwise_fma(dl, dl, acc[r][p]);
        acc[r][p + 1] = __builtin_elementwise_fma(dh, dh, acc[r][p + 1]);
    } else {
        acc[r][p] = __builtin_elementwise_fma(qlo, xlo, acc[r][p]);
        acc[r][p + 1] = __builtin_elementwise_fma(qhi, xhi, acc[r][p + 1]);
    }
}

__device__ __forceinline__ float avx256_reduce2(const f2v (&acc2)[4][4])
{
    float acc[4][8];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int p = 0; p < 4; p++) {
            acc[r][2 * p] = acc2[r][p].x;
            acc[r][2 * p + 1] = acc2[r][p].y;
        }
    return avx256_reduce(acc, 0.0f);
}

// Four chunks (16 floats, one scalar load) of a query.
__device__ __forceinline__ void ld_granule(f4v (&q)[4], cf4 *p)
{
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = p[i];
}

// Queries per pass: what fits beside the row registers without scratch
// (WHOLE: 128 row + 32 accumulator registers + 2 E per query).
constexpr int qshare_qp(int d, int e, bool whole)
{
    return whole ? (e == 1 ? 16 : (e == 2 ? 8 : 4)) : (d > 128 && e == 4 ? 2 : 4);
}

// (two waves per SIMD -- at most 256 registers -- so one wave's tile loads run under the other's folds)
template <int METRIC, int D, int E, bool WHOLE>
__global__ __launch_bounds__(SCAN_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_f32_qshare_kernel(
    QShareArgs a)
{
    static_assert(D % 32 == 0 && D > 0 && !is_abs_or_neq<METRIC>, "shared rows: fixed D, the AVX2 chains");
    constexpr int QP = qshare_qp(D, E, WHOLE);
    constexpr int NC = D / 4;
    const uint32_t G = a.groups;
    if (blockIdx.x >= G) {
        const uint32_t nm = gridDim.x - G;
        for (uint32_t q = blockIdx.x - G; q < a.nq; q += nm) {
            const bool got = merge_lists_ready<E, SCAN_WAVES>(
                a.partials + (size_t)q * G * a.k, a.ready + (size_t)q * G, 1u, G, a.k, a.wait_limit, a.id_base,
                a.ids ? a.ids + (size_t)q * a.k : nullptr, a.dists ? a.dists + (size_t)q * a.k : nullptr,
                a.counts ? a.counts + q : nullptr, nullptr, 0u);
            if (!got) {  // gave up: this query gets empty results (never stale ones), the status word tells
                if (threadIdx.x == 0) atomicOr(a.status, WVG_STATUS_MERGE_TIMEOUT);
                fill_empty_body(a.ids, a.dists, a.counts, q, q + 1, a.k);
            }
            __syncthreads();  // merge LDS reused by the next query
        }
        return;
    }
    const int lane = threadIdx.x & 63;
    const uint64_t ntiles = a.tile_end - a.tile_begin, total = (uint64_t)G * SCAN_WAVES;
    const uint64_t gw = (uint64_t)blockIdx.x * SCAN_WAVES + wave_id();
    const uint64_t t0 = a.tile_begin + ntiles * gw / total, t1 = a.tile_begin + ntiles * (gw + 1) / total;
    const uint64_t n = t1 - t0;
    // tiles i >= split load with the default policy (cache_tail256: only the tail of the pass)
    const uint64_t split = a.cache_tail256 ? n - ((n * a.cache_tail256) >> 8) : (a.plain ? 0 : n);
    const float4 *data = reinterpret_cast<const float4 *>(a.data);
    cu64 *valid = (cu64 *)a.valid;
    const uint32_t qstride = a.qpitch / 4;
    for (uint32_t q0 = 0, pass = 0; q0 < a.nq; q0 += QP, pass++) {
        const uint32_t nqp = a.nq - q0 < (uint32_t)QP ? a.nq - q0 : (uint32_t)QP;  // queries of this pass
        const bool rev = ((a.reverse + pass) & 1u) != 0;  // serpentine over the passes
        WaveTopK<E> tk[QP];
#pragma unroll
        for (int j = 0; j < QP; j++) tk[j].init((int)a.k);
        cf4 *qb = (cf4 *)a.queries + (size_t)q0 * qstride;
        uint64_t m_next = n ? valid[rev ? t1 - 1 : t0] : 0ull;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t t = rev ? t1 - 1 - i : t0 + i;
            const uint64_t m = m_next;
            if (i + 1 < n) m_next = valid[rev ? t - 1 : t + 1];  // scalar prefetch of the next mask
            if (m == 0ull) continue;  // wave-uniform: nothing live in this tile
            const float4 *rp = data + (size_t)t * NC * 64 + lane;
            if constexpr (WHOLE) {
                float4 xs[NC];
                if (i >= split) {
#pragma unroll
                    for (int c = 0; c < NC; c++) xs[c] = ld_stream<false>(rp + (size_t)c * 64);
                } else {
#pragma unroll
                    for (int c = 0; c < NC; c++) xs[c] = ld_stream<true>(rp + (size_t)c * 64);
                }
                // The query words come 16 floats (a granule = one scalar load) at a time, the next
                // granule -- at a query's end the next query's first -- requested before this one is
                // folded.  (The scheduler still gathers a query's loads at its start and parks some
                // of the words in vector lanes: about one v_readlane per four packed operations.)
                constexpr int NG = NC / 4;
                f4v qc[4], qn[4];
                ld_granule(qc, qb);
#pragma unroll
                for (int j = 0; j < QP; j++) {
                    if ((uint32_t)j < nqp) {  // wave-uniform
                        cf4 *qj = qb + (size_t)j * qstride;
                        cf4 *qnext = qb + (size_t)((uint32_t)j + 1 < nqp ? j + 1 : j) * qstride;
                        f2v acc[4][4];
#pragma unroll
                        for (int r = 0; r < 4; r++)
#pragma unroll
                            for (int p = 0; p < 4; p++) acc[r][p] = f2v{0.0f, 0.0f};
#pragma unroll
                        for (int g = 0; g < NG; g++) {
                            ld_granule(qn, g + 1 < NG ? qj + (g + 1) * 4 : qnext);
#pragma unroll
                            for (int c = 0; c < 4; c++) chunk_update2<METRIC>(acc, (g * 4 + c) & 7, qc[c], xs[g * 4 + c]);
#pragma unroll
                            for (int c = 0; c < 4; c++) qc[c] = qn[c];
                        }
                        tk[j].offer(lane_key(m, wrap_metric(a.metric, avx256_reduce2(acc)), t, lane));
                    }
                }
            } else {
                cf4 *qj[QP];
#pragma unroll
                for (int j = 0; j < QP; j++)  // (a short last pass repeats its last query and publishes nothing for it)
                    qj[j] = qb + (size_t)((uint32_t)j < nqp ? (uint32_t)j : nqp - 1) * qstride;
                f2v acc[QP][4][4];
#pragma unroll
                for (int j = 0; j < QP; j++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
#pragma unroll
                        for (int p = 0; p < 4; p++) acc[j][r][p] = f2v{0.0f, 0.0f};
                const bool dflt = i >= split;
#pragma unroll 2
                for (int b = 0; b < D / 32; b++) {
                    float4 xs[8];
                    if (dflt) {
#pragma unroll
                        for (int cc = 0; cc < 8; cc++) xs[cc] = ld_stream<false>(rp + (size_t)(b * 8 + cc) * 64);
                    } else {
#pragma unroll
                        for (int cc = 0; cc < 8; cc++) xs[cc] = ld_stream<true>(rp + (size_t)(b * 8 + cc) * 64);
                    }
#pragma unroll
                    for (int j = 0; j < QP; j++)
#pragma unroll
                        for (int cc = 0; cc < 8; cc++)
                            chunk_update2<METRIC>(acc[j], cc, qj[j][b * 8 + cc], xs[cc]);
                }
#pragma unroll
                for (int j = 0; j < QP; j++)
                    if ((uint32_t)j < nqp)
                        tk[j].offer(lane_key(m, wrap_metric(a.metric, avx256_reduce2(acc[j])), t, lane));
            }
        }
#pragma unroll
        for (int j = 0; j < QP; j++) {
            if ((uint32_t)j < nqp) {  // workgroup-uniform
                const size_t li = (size_t)(q0 + j) * G + blockIdx.x;
                group_combine_publish<E, SCAN_WAVES>(tk[j], a.partials + li * a.k, nullptr, a.ready + li, 1u);
            }
        }
    }
}

// Which corpora the kernel covers, its queries per pass and its grid.
bool qshare_supported(int metric, uint32_t dim, int order512)
{
    return (metric == WVG_M_L2 || metric == WVG_M_DOT || metric == WVG_M_COSINE) && (dim == 128 || dim == 768) &&
           !order512;
}

static bool qshare_whole(uint32_t dim)
{
#ifdef WVG_TOOLS
    if (tuning().qshare == 2) return false;  // A/B: the block shape at d = 128 too
#endif
    return dim == 128;
}

uint32_t qshare_queries_per_pass(uint32_t dim, uint32_t k)
{
    const int e = k <= 64 ? 1 : (k <= 128 ? 2 : 4);
    return (uint32_t)qshare_qp((int)dim, e, qshare_whole(dim));
}

// Two 4-wave workgroups per CU (the kernels stay within 256 registers), every wave at least one tile.
uint32_t qshare_groups(uint64_t ntiles, int num_cus)
{
    const uint64_t g = std::min<uint64_t>((uint64_t)num_cus * 2, (ntiles + SCAN_WAVES - 1) / SCAN_WAVES);
    return (uint32_t)std::max<uint64_t>(g, 1);
}

template <int METRIC, int E>
static hipError_t launch_qshare_e(const QShareArgs &a, uint32_t mergers, hipStream_t s)
{
    dim3 grid(a.groups + mergers), block(SCAN_WAVES * 64);
    if (a.dim == 128) {
#ifdef WVG_TOOLS
        if (!qshare_whole(a.dim)) {
            launch_timed((scan_f32_qshare_kernel<METRIC, 128, E, false>), grid, block, 0, s, a);
            return hipGetLastError();
        }
#endif
        launch_timed((scan_f32_qshare_kernel<METRIC, 128, E, true>), grid, block, 0, s, a);
    } else if (a.dim == 768) {
        launch_timed((scan_f32_qshare_kernel<METRIC, 768, E, false>), grid, block, 0, s, a);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_scan_f32_qshare(const QShareArgs &a, uint32_t mergers, hipStream_t s)
{
    if (!qshare_supported(a.metric, a.dim, 0) || mergers == 0) return hipErrorInvalidValue;
    auto go = [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        if (a.k <= 64) return launch_qshare_e<MM, 1>(a, mergers, s);
        if (a.k <= 128) return launch_qshare_e<MM, 2>(a, mergers, s);
        return launch_qshare_e<MM, 4>(a, mergers, s);
    };
    return a.metric == WVG_M_L2 ? go(MetricTag<WVG_M_L2>{}) : go(MetricTag<WVG_M_DOT>{});
}

}  // namespace wvg

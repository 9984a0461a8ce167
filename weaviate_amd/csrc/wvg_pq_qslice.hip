// wvg_pq_qslice.hip -- the shared-row query stream of PQ corpora whose LUTs do not fit LDS two at a
// time (at ks = 256: m >= 96, the segment counts Weaviate picks for 384-d and larger vectors), in a
// context with cache_reuse = 2.
//
// scan_pq_qshare_kernel (wvg_pq_qshare.hip) keeps the whole image of a pass's Q LUTs in LDS.  Here the
// image holds one SLICE of S consecutive segments of the pass's 4 LUTs -- entry (s, c) of the slice is
// the four queries' lut[s0 + s][c] side by side, 16 bytes at float ((s ks + c) 4), the generic form's
// entry -- and the workgroup walks the slices in segment order, refilling the image from the LUTs in
// the workspace.  A wave cannot finish a row inside one slice, so it works on a BLOCK of T live tiles
// and carries their T x 4 partial sums in registers from slice to slice: per slice it loads only
// that slice's chunks of its T tiles (S / 16 contiguous 1 KiB chunks per tile) and adds
// lut_j[s][code] to sum (tile, j) for s ascending.  After the last slice the T x 4 sums are offered
// to the queries' lists and the wave takes its next T tiles, starting again from slice 0.  A pass of
// 4 queries therefore reads every code once and the LUTs once per block (from L2: a block of 16 x T
// tiles reads m T KiB of codes and 16 m ks bytes of LUTs).
//
// Query j's sum of a row receives lut_j[s][code_s] for s = 0 .. m - 1 in that order from +0.0f with
// plain fp32 adds (the file builds with -ffp-contract=off and without packed fp32 operations), then
// Wrap: the reference's sequential sum (CH/product_quantization.go:85-104, 352-361) whichever slice a
// term comes from, so the results are those of 4 separate K8 scans bit for bit.  The other three
// floats of an entry never meet query j's sum.
//
// Barriers: the image is the workgroup's, so every refill stands between two workgroup barriers (all
// lookups of the previous slice done; all entries of this one written).  Every wave meets every
// barrier: the number of blocks is the workgroup's largest, found once at the start (each wave counts
// the tiles of its range in which some query of the pass has a live allowed row, the counts meet in
// the not yet filled image), and a wave that has run out of tiles -- or never had one -- walks the
// remaining slices with an empty block.  No workgroup waits for another; the status block is not
// touched.  Grid, row ranges, lists and merge are the whole-image scan's.
#include "wvg_internal.hpp"
#include "wvg_rowdist.hpp"
#include "wvg_topk.hpp"

namespace wvg {

typedef float f32x4s __attribute__((ext_vector_type(4)));

// Tiles per block.  The workgroup is 1024 threads on one CU: 128 VGPRs a lane, of which the four lists
// take 8 E and the sums 4 T.  T = 8 at E = 4 spills (13 to 43 VGPRs to the private segment).
template <int E>
constexpr int PQ_SLICE_T = E == 4 ? 4 : 8;

// E: 64-key registers per list (k <= 64 E).  Q = 4.  FILT: per-query allow words.  PLAIN: ld_pq_codes.
// S: segments per slice, a multiple of 16; the launch's dynamic LDS is 16 min(S, 16 nchunks) ks bytes.
// Queries of the last pass that do not exist (j >= nqp) have +0.0 image entries and are never offered.
template <int E, int Q, bool FILT, bool PLAIN>
__global__ __launch_bounds__(PQ_QSHARE_WAVES * 64) void scan_pq_qshare_slice_kernel(PQShareArgs a, uint32_t S)
{
    static_assert(Q == 4, "16-byte image entries");
    constexpr int T = PQ_SLICE_T<E>;
    extern __shared__ __attribute__((aligned(16))) float img[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t rng = blockIdx.x, G = gridDim.x, q0 = blockIdx.y * Q;
    const uint32_t nqp = min((uint32_t)Q, a.nq - q0);  // queries of this pass (>= 1: gridDim.y = ceil(nq / Q))
    const bool rev = ((a.reverse + blockIdx.y) & 1u) != 0u;  // one direction per pass
    const uint32_t m = a.m, ks = a.ks, nch = a.nchunks, SC = S / 16;
    const float *gl = a.luts + (size_t)q0 * a.lpitch;
    const uint4 *data = reinterpret_cast<const uint4 *>(a.data);
    const uint64_t ntiles = a.tile_end - a.tile_begin;
    const uint64_t total = (uint64_t)G * PQ_QSHARE_WAVES;
    const uint64_t gw = (uint64_t)rng * PQ_QSHARE_WAVES + wave;
    const uint64_t t0 = a.tile_begin + ntiles * gw / total, t1 = a.tile_begin + ntiles * (gw + 1) / total;
    const uint64_t n = t1 - t0;  // the wave walks i = 0 .. n - 1, tile t0 + i upwards or t1 - 1 - i downwards
    WaveTopK<E> tk[Q];
#pragma unroll
    for (int j = 0; j < Q; j++) {
        tk[j].init((int)a.k);
        tk[j].init_fast();
    }
    auto tile_of = [&](uint64_t i) { return rev ? t1 - 1 - i : t0 + i; };
    // live rows of tile t some query of the pass may take
    auto live_word = [&](uint64_t t) {
        uint64_t v = a.valid[t];
        if constexpr (FILT) {
            uint64_t u = 0ull;
#pragma unroll
            for (int j = 0; j < Q; j++)
                if ((uint32_t)j < nqp) u |= pq_qshare_allow(a, q0 + j, t);
            v &= u;
        }
        return v;
    };
    // The workgroup's block count: the wave's chain of tiles with such a row, 64 tiles of the range at
    // a time (a tile per lane), in blocks of T; the largest of the 16 waves.  The words meet in the image,
    // which the first refill overwrites only after its leading barrier.
    uint32_t chain = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += 64) {
        const uint64_t i = i0 + (uint64_t)lane;
        const uint64_t w = i < n ? live_word(tile_of(i)) : 0ull;
        chain += (uint32_t)__popcll(__ballot(w != 0ull));
    }
    uint32_t *blocks_of = reinterpret_cast<uint32_t *>(img);
    if (lane == 0) blocks_of[wave] = (chain + T - 1) / T;
    __syncthreads();
    uint32_t nblk = 0;
#pragma unroll
    for (int w = 0; w < PQ_QSHARE_WAVES; w++) nblk = max(nblk, blocks_of[w]);
    nblk = __builtin_amdgcn_readfirstlane(nblk);

    // one chunk of one tile: 16 (row, segment) lookups of the slice that begins at chunk c0, the four
    // queries' terms from one read; the corpus's last chunk may be partly filled
    auto add_chunk = [&](float (&sum)[Q], const uint4 &xw, uint32_t c, uint32_t c0) {
        const uint32_t ws[4] = {xw.x, xw.y, xw.z, xw.w};
        const float *base = img + (size_t)(c - c0) * 16u * ks * Q;
        if (c * 16u + 16u <= m) {
#pragma unroll
            for (int b = 0; b < 16; b++) {
                const uint32_t code = (ws[b >> 2] >> (8 * (b & 3))) & 0xFFu;
                const f32x4s v = *reinterpret_cast<const f32x4s *>(base + ((size_t)b * ks + code) * Q);
                sum[0] = sum[0] + v.x;
                sum[1] = sum[1] + v.y;
                sum[2] = sum[2] + v.z;
                sum[3] = sum[3] + v.w;
            }
        } else {
#pragma unroll
            for (int b = 0; b < 16; b++) {
                if (c * 16u + (uint32_t)b < m) {
                    const uint32_t code = (ws[b >> 2] >> (8 * (b & 3))) & 0xFFu;
                    const f32x4s v = *reinterpret_cast<const f32x4s *>(base + ((size_t)b * ks + code) * Q);
                    sum[0] = sum[0] + v.x;
                    sum[1] = sum[1] + v.y;
                    sum[2] = sum[2] + v.z;
                    sum[3] = sum[3] + v.w;
                }
            }
        }
    };

    uint64_t i = 0;  // the wave's place in its range
    for (uint32_t blk = 0; blk < nblk; blk++) {
        // the block: the next up to T tiles of the chain, tile and live word of block tile b in lane b
        uint64_t tv = 0ull, mv = 0ull;
        uint32_t nb = 0;
        while (nb < (uint32_t)T && i < n) {
            const uint64_t t = tile_of(i), w = live_word(t);
            if (w) {
                if ((uint32_t)lane == nb) {
                    tv = t;
                    mv = w;
                }
                nb++;
            }
            i++;
        }
        float acc[T][Q];
#pragma unroll
        for (int ti = 0; ti < T; ti++)
#pragma unroll
            for (int j = 0; j < Q; j++) acc[ti][j] = 0.0f;
        // Code loads run two chunks ahead of the lookups, in the order the lookups take them: slice by
        // slice, tile by tile, chunk by chunk; the cursor crosses into the next slice, so its first
        // chunks arrive during the refill.  (pt, pc): block tile and chunk of the next load, [pb, pe) the
        // chunks of its slice; pt = nb: the block's last chunk has been asked for.
        uint32_t pt = 0, pb = 0, pe = min(SC, nch), pc = 0;
        auto fetch = [&]() {
            uint4 x = make_uint4(0u, 0u, 0u, 0u);
            if (pt < nb) {
                x = ld_pq_codes<PLAIN>(data + ((size_t)readlane64(tv, (int)pt) * nch + pc) * 64 + lane);
                if (++pc == pe) {
                    pc = pb;
                    if (++pt == nb && pe < nch) {
                        pt = 0;
                        pb = pe;
                        pe = min(pe + SC, nch);
                        pc = pb;
                    }
                }
            }
            return x;
        };
        uint4 x0 = fetch(), x1 = fetch();
        for (uint32_t s0 = 0, c0 = 0; s0 < m; s0 += S, c0 += SC) {
            const uint32_t ne = min(S, m - s0) * ks, c1 = min(c0 + SC, nch);
            const float *gs = gl + (size_t)s0 * ks;
            __syncthreads();  // the lookups of the previous slice (or block) are done
            // thread e reads the four queries' entry e of the slice (coalesced per query) and writes it once
#pragma unroll 2
            for (uint32_t e = threadIdx.x; e < ne; e += PQ_QSHARE_WAVES * 64) {
                float v[Q];
#pragma unroll
                for (int j = 0; j < Q; j++) v[j] = (uint32_t)j < nqp ? gs[(size_t)j * a.lpitch + e] : 0.0f;
                *reinterpret_cast<f32x4s *>(img + (size_t)e * Q) = f32x4s{v[0], v[1], v[2], v[3]};
            }
            __syncthreads();
#pragma unroll
            for (int ti = 0; ti < T; ti++) {
                if ((uint32_t)ti < nb) {
                    for (uint32_t c = c0; c < c1; c++) {
                        const uint4 x = x0;
                        x0 = x1;
                        x1 = fetch();
                        add_chunk(acc[ti], x, c, c0);
                    }
                }
            }
        }
        // the block's sums to the lists of the queries that take a row of the tile
#pragma unroll
        for (int ti = 0; ti < T; ti++) {
            if ((uint32_t)ti < nb) {
                const uint64_t t = readlane64(tv, ti), live = readlane64(mv, ti);
#pragma unroll
                for (int j = 0; j < Q; j++) {
                    if ((uint32_t)j < nqp) {
                        uint64_t mq = live;
                        if constexpr (FILT) mq &= pq_qshare_allow(a, q0 + j, t);
                        if (mq) tk[j].offer_dist_fast(wrap_metric(a.metric, acc[ti][j]), (uint32_t)(t * 64 + lane), mq);
                    }
                }
            }
        }
    }
    // one list per (query, range); group_combine_store reuses one LDS buffer, hence the barrier
    // between queries (the j < nqp test is the same for the whole workgroup)
#pragma unroll
    for (int j = 0; j < Q; j++) {
        if ((uint32_t)j < nqp) {
            if (j > 0) __syncthreads();
            group_combine_store<E, PQ_QSHARE_WAVES>(tk[j], a.partials + ((size_t)(q0 + j) * G + rng) * a.k);
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------
// Segments per slice: the largest multiple of 16 whose image (4 S ks 4 bytes) fits one workgroup's LDS
// beside the kernel's own static LDS (group_combine_store's buffer, 8 KiB x E), as the code object
// states it; 0 = not even one chunk's segments fit.  At ks = 256: 32 (128 KiB) for every E.
template <int E>
static uint32_t pq_qslice_segments_e(uint32_t ks)
{
    for (uint32_t S = (uint32_t)(WVG_LDS_BYTES / (16u * ks)) / 16u * 16u; S >= 16u; S -= 16u)
        if (fits_lds<&scan_pq_qshare_slice_kernel<E, 4, false, false>>((size_t)16 * S * ks)) return S;
    return 0;
}

// (m = 32 rows are stored rotated; their image always fits whole, so the slice form does not read them)
uint32_t pq_qslice_queries_per_pass(uint32_t m, uint32_t ks, uint32_t k)
{
    if (m == 0 || ks == 0 || ks > 256 || k == 0 || k > 256 || pq_rotated(m)) return 1;
    const uint32_t S = k <= 64 ? pq_qslice_segments_e<1>(ks) : k <= 128 ? pq_qslice_segments_e<2>(ks) : pq_qslice_segments_e<4>(ks);
    return S >= 16u ? 4 : 1;
}

template <int E>
static hipError_t launch_pq_qslice_e(const PQShareArgs &a, uint32_t groups, hipStream_t s)
{
    const uint32_t S = pq_qslice_segments_e<E>(a.ks);
    if (S < 16u) return hipErrorInvalidValue;
    const uint32_t passes = (a.nq + 3) / 4;
    if (passes > 65535u) return hipErrorInvalidValue;
    const dim3 grid(groups, passes), block(PQ_QSHARE_WAVES * 64);
    const uint32_t lds = 16u * std::min(S, a.nchunks * 16u) * a.ks;
    if (a.allow) {
        if (a.plain)
            launch_timed((scan_pq_qshare_slice_kernel<E, 4, true, true>), grid, block, lds, s, a, S);
        else
            launch_timed((scan_pq_qshare_slice_kernel<E, 4, true, false>), grid, block, lds, s, a, S);
    } else {
        if (a.plain)
            launch_timed((scan_pq_qshare_slice_kernel<E, 4, false, true>), grid, block, lds, s, a, S);
        else
            launch_timed((scan_pq_qshare_slice_kernel<E, 4, false, false>), grid, block, lds, s, a, S);
    }
    return hipGetLastError();
}

hipError_t launch_scan_pq_qslice(const PQShareArgs &a, uint32_t groups, hipStream_t s)
{
    if (a.k == 0 || a.k > 256 || a.nq == 0 || groups == 0 || a.m == 0 || a.ks == 0 || a.ks > 256 ||
        a.nchunks != pq_chunks(a.m) || pq_rotated(a.m))
        return hipErrorInvalidValue;
    if (a.k <= 64) return launch_pq_qslice_e<1>(a, groups, s);
    if (a.k <= 128) return launch_pq_qslice_e<2>(a, groups, s);
    return launch_pq_qslice_e<4>(a, groups, s);
}

}  // namespace wvg

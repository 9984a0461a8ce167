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
//  runtime dimension (scan_f32_qshare_dyn_kernel: every other d >= 8, d % 4 == 0):
//    the block shape with a.dim >> 5 blocks, then the tail of the AVX2 order as
//    row_dot_or_l2_generic (wvg_rowdist.hpp) walks it -- the leftover 8-float
//    blocks into accumulator row 0, four last elements through scalar_update
//    into the sum avx256_reduce adds last.  Unseeded and unscreened.
// The query words and tile masks are wave-uniform and read through the constant
// address space: the publishes of the previous pass would otherwise make them
// "maybe clobbered" vector loads (wvg_topk.hpp, offer_dist_emit).  Nothing
// writes the queries or the validity words while the kernel runs.
// Workgroups 0..groups-1 scan and never wait; workgroups groups.. merge, merger
// m the queries m, m + mergers, ...: the waiting workgroups have the highest
// ids, so every workgroup they wait for is dispatched before them.
// Roofline: one HBM read of the rows per pass against nq x rows x d (sub, fma)
// pairs on the VALU.
// A wave of the 1M-row scan owns only ~8 tiles, so a list that starts empty
// never reaches the steady state where a batch is rejected by one compare: per
// query it pays a 64-key sort + merge on its first tile and a couple of dozen
// single inserts after it, and nearly all of those keys are dropped by the
// mergers.  qshare_seed_kernel (launched before the scan, in place of the
// memset of the ready words) scores a sample of the first tiles and leaves the
// sample's k-th key per query; the lists start from that bound (QShareArgs).
//
// The screen (scan_f32_qshare_screen_kernel: L2, d = 128, k <= 64, seeded
// launches).  With the seed bound nearly every exact distance is computed only
// to be rejected by one compare.  So per tile a bf16 MFMA dot of every row with
// every query of the pass gives a rigorous lower bound of the exact distance,
// and the exact chain runs only for the (query, row) pairs whose lower bound
// does not exceed the query's tau: the screen leaves every lane a mask of its
// row's admitted queries.  A pair that is not admitted holds no key below tau --
// offer_bounded would have dropped it at its first ballot -- so every list is
// the unscreened one after every tile, and only the exact chain produces keys.
//
// The rounds.  While any lane of the tile has a bit set, each lane takes its
// lowest admitted query jl, clears the bit and runs the unchanged chain on its
// own row (chunk_update2 in chunk order, avx256_reduce2, wrap_metric, lane_key:
// the same lane-wise instructions on the same operands, hence the same bits),
// the query chunks read from an fp32 LDS image of the pass's queries at its own
// jl (QS_FROW pads a query to 528 B so that lanes reading different queries at
// one chunk do not meet in one bank).  Then, for every query j that some lane
// took (an unrolled loop with a wave-uniform test: tk[] is never indexed
// dynamically), the lanes with jl = j offer their keys to tk[j] and the others
// offer KEY_NONE.  A query may so be offered in more than one round of a tile,
// and in an order that differs from lane to lane.  That changes no list: a list
// is the set of the k smallest unique keys below its bound among the keys
// offered so far, whatever the batches they came in (offer_bounded inserts or
// merges exactly the keys below tau, and tau only falls), and a pair admitted
// under an earlier, larger tau of the same tile is merely offered and dropped.
// So after each tile every list equals the one the tile-level fold left.  A NaN
// or infinite lower bound or an open tau sets the bit: a lane holding a NaN row
// runs up to 16 rounds, and a pass with open seeds runs 16 full rounds per tile,
// the unscreened cost.  On the bench's shape (1M x 128 uniform rows, k = 10, 16
// queries) 0.6 % of the pairs are admitted -- about 6 of a tile's 1,024 -- and a
// tile needs about 1.5 rounds, where the tile-level fold ran about 5.4 chains of
// 64 rows per tile (33.6 % of the (query, tile) pairs) at about 260 VALU
// instructions each; the screen's own epilogue is about 13 per query.
//
// The bound.  u = 2^-24, d = 128, q and x the fp32 vectors, D = |q - x|^2 =
// |q|^2 + |x|^2 - 2 q.x in real numbers, r = the exact chain's fp32 result.
//  (a) r >= D (1 - (d + 4) u) - 2^-109: every term of r is non-negative and
//      passes at most 2 (the subtraction, squared) + d / 8 (its chain's fmas)
//      + 5 (avx256_reduce) roundings; underflowing fmas lose at most d 2^-126.
//      D <= 2 (|q|^2 + |x|^2), so the loss is at most 2 (d + 4) u (|q|^2 + |x|^2).
//  (b) m = the MFMA dot of bf16(q), bf16(x) (round to nearest, |v - bf16(v)| <=
//      2^-8 |v|, products exact in fp32, fp32 accumulation): K3c's bound
//      (wvg_screen.hip) |q.x - m| <= c |q| |x| + (denormal terms), c = 2^-7 +
//      2^-15 + d 2^-21, by Cauchy-Schwarz.
//  (c) Nq2 = |q|^2 and Nq >= |q| come from a double sum in the prologue.  Nx2 is
//      the lane's fp32 sum of x_i^2 in any order: |x|^2 >= Nx2 (1 - d u), and
//      |x|^2 <= Nx2 (1 + d u) + d 2^-126 (squares below 2^-126 may vanish), so
//      with Nx = sqrt(Nx2) (1 + 2^-16) (v_sqrt_f32 is within 1 ulp and may flush
//      a denormal Nx2): |x| <= Nx + eta, eta = 2^-59.
//  (d) the combine runs in fp32: Bx = Nx2 (1 - g), t = Bx + Cq, t = fma(-2, m, t),
//      lower = fma(-K1q, Nx, t); each rounding is at most u times a value below
//      2.2 (Nq2 + Nx2).
// (a), (c) and (d) together cost less than 400 u (Nq2 + Nx2); g = 2^-15 = 512 u
// pays for them.  (b) with (c) costs 2 c (Nq Nx + eta (Nq + Nx) + eta^2) plus
// 2^-119 (Nq + Nx) + 2^-109 for bf16 operands and products that flush.  Hence
//   lower = (Nq2 + Nx2 - 2 m) - (K1q Nx + K2q + g Nx2) <= r,
//   K1q = (2 c Nq + 2^-60) (1 + 2^-20),  K2q = g Nq2 + 2^-60 Nq + 2^-100,
// the form lower = (Nq2 + Nx2 - 2m) - (K1q Nx + K2q (1 + Nx2)) with the second
// term's Nq2 kept apart from Nx2 (g (Nq2 + Nx2) instead of g max(1, Nq2) (1 +
// Nx2): the same bound for small norms, a useful one for large norms).  The
// prologue stores Cq = Nq2 - K2q.  Special values: a NaN or an infinity in q, x,
// the norms, m (bf16 or fp32 overflow included) makes lower NaN or infinite, and
// the pair is skipped only if lower > tau_dist AND lower < +inf: anything
// else is admitted.  tau_dist is the float under tau's high word (NaN for an open
// tau: admitted); lower > tau_dist gives ord(r) > ord(tau_dist), so no key below tau.
// The operands: v_mfma_f32_4x4x4_16b_bf16 is 16 independent 4x4x4 blocks, block
// = lane / 4.  B = 4 k-values of the lane's own row; A = the same 4 k-values of
// query 4 g + (lane & 3) from the LDS image; result register i of the lane = its
// row's dot with query 4 g + i.
//
// Allow lists (wvg_search_device_pipelined_filtered; QShareFilt, wvg_internal.hpp).  The filtered
// kernels -- scan_f32_qshare_filt_kernel, scan_f32_qshare_screen_filt_kernel, qshare_seed_filt_kernel --
// are the bodies below with FILT = true and the window as a second kernel argument; the unfiltered
// kernels instantiate FILT = false and keep their names, arguments and code.  Per tile and query j of the
// pass mq[j] = valid & allow_j: the allow words are wave-uniform scalar loads behind one window compare,
// prefetched a tile ahead; query j's keys come from the lanes of mq[j] only (unscreened: lane_key(mq[j]);
// screened: bit j of the admission mask is cleared elsewhere), and a tile no query of the pass allows is
// skipped before its rows are loaded.  A row a query does not allow never reaches that query's list, so
// each list is the one a filtered scan of its own keeps.
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

__device__ __forceinline__ float avx256_reduce2(const f2v (&acc2)[4][4], float sum = 0.0f)  // sum: the scalar tail's
{
    float acc[4][8];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int p = 0; p < 4; p++) {
            acc[r][2 * p] = acc2[r][p].x;
            acc[r][2 * p + 1] = acc2[r][p].y;
        }
    return avx256_reduce(acc, sum);
}

// Four chunks (16 floats, one scalar load) of a query.
__device__ __forceinline__ void ld_granule(f4v (&q)[4], cf4 *p)
{
#pragma unroll
    for (int i = 0; i < 4; i++) q[i] = p[i];
}

// Queries per pass: what fits beside the row registers without scratch
// (WHOLE: 128 row + 32 accumulator registers + 2 E per query).  d = 0: the
// runtime-dimension block form, the shape of d = 768.
constexpr int qshare_qp(int d, int e, bool whole)
{
    return whole ? (e == 1 ? 16 : (e == 2 ? 8 : 4)) : ((d == 0 || d > 128) && e == 4 ? 2 : 4);
}

// The bound of a query's lists from its seed: seed + 1, so that `key < bound`
// admits the seed row itself (the wave that owns it scans it again); an open
// seed (KEY_NONE) stays open.
__device__ __forceinline__ uint64_t seed_bound(cu64 *seed)
{
    const uint64_t s = *seed;
    return s + (s != WVG_KEY_NONE ? 1ull : 0ull);
}

// The screen's constants (the bound at the top of the file) and operand types.
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short shortx4 __attribute__((ext_vector_type(4)));
constexpr int QS_D = 128;                   // the screened form's dimension
constexpr double QS_C = 0x1p-7 + 0x1p-15 + QS_D * 0x1p-21;
constexpr float QS_G = 0x1p-15f;
constexpr int QS_QROW = QS_D * 2 / 16 + 1;  // uint4 per query of the LDS image: 256 B + 16 B (the four
                                            // queries a ds_read_b128 fetches then lie in different banks)
constexpr int QS_FROW = QS_D / 4 + 1;       // f4v per query of the fp32 LDS image: 512 B + 16 B (lanes that read
                                            // different queries at one chunk then lie in different banks)

__device__ __forceinline__ shortx4 bf16_of(float4 x)  // two v_cvt_pk_bf16_f32: round to nearest even
{
    const bf16x2 lo = __builtin_convertvector(f2v{x.x, x.y}, bf16x2), hi = __builtin_convertvector(f2v{x.z, x.w}, bf16x2);
    return __builtin_bit_cast(shortx4, make_uint2(__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi)));
}

// The query side of the screen, by one wave: the query's bf16 image and
// {Nq2, K1q, K2q, Cq = Nq2 - K2q} from the double square sum.  A non-finite
// query ends in NaN or infinite constants (Cq = inf - inf), which fold.
__device__ __forceinline__ void screen_query_side(const QShareArgs &a, uint32_t q, cf4 *qj, int lane)
{
    const int c = lane & (QS_D / 4 - 1);
    const f4v v = qj[c];
    double ss = lane < QS_D / 4
                    ? (double)v.x * (double)v.x + (double)v.y * (double)v.y + (double)v.z * (double)v.z + (double)v.w * (double)v.w
                    : 0.0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    if (a.screen == 2) {
        // The scan reads the corpus's shadow (qshare_shadow_body): the query as an MFMA fragment in
        // screen_qfrag_kernel's layout -- fragment (q / 16, kb), lane l = query q % 16 at l & 15, elements
        // 32 kb + 8 (l >> 4) .. + 7, so lane i < 16 of this wave converts elements 8 i .. 8 i + 7 (round to
        // nearest even, as the rows') -- and K3c-L2's constants of the same fp64 square sum.
        if (lane < QS_D / 8) {
            const f4v lo = qj[2 * lane], hi = qj[2 * lane + 1];
            const shortx4 blo = bf16_of(make_float4(lo.x, lo.y, lo.z, lo.w)), bhi = bf16_of(make_float4(hi.x, hi.y, hi.z, hi.w));
            const uint2 wl = __builtin_bit_cast(uint2, blo), wh = __builtin_bit_cast(uint2, bhi);
            reinterpret_cast<uint4 *>(a.qbf)[((size_t)(q >> 4) * 4 + (lane >> 2)) * 64 + (lane & 3) * 16 + (q & 15)] =
                make_uint4(wl.x, wl.y, wh.x, wh.y);
        }
        if (lane == 0) {
            float K1, K2, C;
            screen_l2_query_consts(ss, QS_D, K1, K2, C);
            a.qconst[q] = make_float4(K1, K2, C, 0.0f);
        }
        return;
    }
    if (lane < QS_D / 4)
        reinterpret_cast<shortx4 *>(a.qbf)[(size_t)q * (QS_D / 4) + c] = bf16_of(make_float4(v.x, v.y, v.z, v.w));
    if (lane == 0) {
        const double nq = __builtin_sqrt(ss) * (1.0 + 1e-6);
        const double k1 = (2.0 * QS_C * nq + 0x1p-60) * (1.0 + 0x1p-20);
        const double k2 = (double)QS_G * ss + 0x1p-60 * nq + 0x1p-100;
        a.qconst[q] = make_float4((float)ss, (float)k1, (float)k2, (float)(ss - k2));
    }
}

// The prologue of a shared-row launch.  The grid zeroes the ready words; then
// one WAVE scores one (sample tile, query) pair: workgroup b holds tile b % T of
// the first T = a.seed_tiles tiles of the range and the queries PRO_WAVES (b / T)
// + wave, so the queries of a tile meet in one workgroup and the tile comes from
// HBM once (T % 8 == 0 puts the workgroups of one tile on one XCD's L2).  The
// wave loads its whole tile at once -- behind no mask, allow word or query: a
// tile of the range is memory whatever its mask says -- runs the scan's chain
// (chunk_update2 in chunk order, avx256_reduce2, wrap_metric, lane_key with the
// scan's validity word: the keys are the scan's bit for bit), sorts its 64 keys
// and publishes the first min(k, 64) of them to pro.lists[q][tile] in the
// hand-off form of pass_combine_publish (agent-scope stores, the storing wave's
// drain); after the workgroup's barrier one agent-scope add tells the
// workgroup's arrival at pro.arrivals[c], c = its query block mod PRO_COUNTERS.
// A pair with an empty mask (a dead tile, an allow word of zero, a tile past the
// range, FILT: query q's sample is the rows of valid & allow_q) publishes
// KEY_NONE throughout and arrives like any other.  Nobody waits: the workgroup
// that arrives last at counter c -- its add returns T x (query blocks of class c)
// - 1 -- puts the counter back to zero for the next call and merges the queries
// of class c's blocks, wave w the w-th query of each (up to 128 queries: every
// wave one query, PRO_COUNTERS workgroups merging side by side), a lane per list
// as merge_lists_body reads them (agent-scope loads, as merge_lists_ready; up to
// PRO_CHUNK keys per lane in flight, since a dependent load per key was most of
// the merge's time), and writes seeds[q]: the sample's k-th smallest key,
// KEY_NONE with fewer than k live rows.  Every other workgroup exits.  The
// counters lie in the workspace's status block (QSharePro).
// Without a sample (seed_tiles = 0, d = 768) T = 1 and every seed is opened.
constexpr int SEED_WAVES = 16;  // qshare_open_seed_kernel's workgroup
constexpr int PRO_WAVES = 8;    // two waves per SIMD: 256 registers, the tile's 128 and the chain beside them
constexpr int PRO_CHUNK = 12;   // keys of a list a merging lane loads at once (48 KiB of LDS for the workgroup)

// Query q's allow word of tile t: wave-uniform, and no word outside [0, stride) is read.
__device__ __forceinline__ uint64_t allow_word(cu64 *aq, uint64_t stride, uint64_t t0, uint64_t t)
{
    const uint64_t w = t - t0;
    return w < stride ? aq[w] : 0ull;
}

template <int METRIC, int D, int E, bool FILT>
__device__ __forceinline__ void qshare_seed_body(const QShareArgs &a, const QSharePro &pro, const QShareFilt &f,
                                                 uint32_t bdim, uint32_t gdim)
{
    static_assert(D % 32 == 0 && D > 0 && !is_abs_or_neq<METRIC>, "shared rows: fixed D, the AVX2 chains");
    constexpr int NC = D / 4;
    constexpr bool WHOLE = D <= 128;  // the tile in registers at once; larger rows in blocks of 32 floats
    const uint64_t nready = (uint64_t)a.nq * a.groups;
    for (uint64_t i = (uint64_t)blockIdx.x * bdim + threadIdx.x; i < nready; i += (uint64_t)gdim * bdim)
        a.ready[i] = 0u;
    const int lane = threadIdx.x & 63, wave = wave_id();
    const uint32_t T = a.seed_tiles ? a.seed_tiles : 1u;  // gridDim.x == T * ceil(nq / PRO_WAVES)
    const uint32_t ti = blockIdx.x % T, q = blockIdx.x / T * PRO_WAVES + (uint32_t)wave;
    const bool hasq = q < a.nq;  // wave-uniform
    const uint64_t ntiles = a.tile_end - a.tile_begin;
    const uint64_t ns = a.seed_tiles < ntiles ? a.seed_tiles : ntiles;
    const uint64_t t = a.tile_begin + ti;
    const bool score = hasq && ti < ns;  // wave-uniform
    cf4 *qj = (cf4 *)a.queries + (size_t)(hasq ? q : 0u) * (a.qpitch / 4);
    const float4 *rp = reinterpret_cast<const float4 *>(a.data) + (size_t)t * NC * 64 + lane;
    float4 xs[WHOLE ? NC : 1];
    if constexpr (WHOLE) {
        if (score) {  // default policy: the scan reads them again
#pragma unroll
            for (int c = 0; c < NC; c++) xs[c] = rp[(size_t)c * 64];
        }
    }
    if constexpr (METRIC == WVG_M_L2 && D == QS_D) {
        if (a.screen) {  // the scan screens: its query side, by the query's wave of tile 0, under the row loads
#ifdef WVG_TOOLS
            if (threadIdx.x == 0 && blockIdx.x == 0) a.screen_count[0] = a.screen_count[1] = 0ull;
#endif
            if (ti == 0 && hasq) screen_query_side(a, q, qj, lane);
        }
    }
    if (ns == 0) {  // grid-uniform: no sample, every seed open
        if (hasq && lane == 0) a.seeds[q] = WVG_KEY_NONE;
        return;
    }
    uint64_t key = WVG_KEY_NONE;
    if (score) {
        uint64_t m = ((cu64 *)a.valid)[t];
        if constexpr (FILT) m &= allow_word((cu64 *)f.allow + (size_t)q * f.stride, f.stride, f.t0, t);
        if (m != 0ull) {  // wave-uniform
            f2v acc[4][4];
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int p = 0; p < 4; p++) acc[r][p] = f2v{0.0f, 0.0f};
            if constexpr (WHOLE) {
#pragma unroll
                for (int c = 0; c < NC; c++) chunk_update2<METRIC>(acc, c & 7, qj[c], xs[c]);
            } else {
#pragma unroll 2
                for (int b = 0; b < D / 32; b++) {
                    float4 xb[8];
#pragma unroll
                    for (int cc = 0; cc < 8; cc++) xb[cc] = rp[(size_t)(b * 8 + cc) * 64];
#pragma unroll
                    for (int cc = 0; cc < 8; cc++) chunk_update2<METRIC>(acc, cc, qj[b * 8 + cc], xb[cc]);
                }
            }
            key = lane_key(m, wrap_metric(a.metric, avx256_reduce2(acc)), t, lane);
            sort64(key);
        }
    }
    const uint32_t kk = a.k < 64u ? a.k : 64u;  // a tile holds 64 keys
    if (hasq && (uint32_t)lane < kk)
        __hip_atomic_store((gu64 *)(pro.lists + ((size_t)q * T + ti) * kk + lane), key, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its own list
    __shared__ uint32_t last_sh;
    __shared__ uint64_t stage[PRO_WAVES][PRO_CHUNK][64];  // the merge's keys, lane by lane
    __syncthreads();
    const uint32_t nqb = (a.nq + PRO_WAVES - 1) / PRO_WAVES, qb = blockIdx.x / T, cls = qb % PRO_COUNTERS;
    gu32 *ctr = (gu32 *)pro.arrivals + cls;
    if (threadIdx.x == 0) {  // class cls: the query blocks cls, cls + PRO_COUNTERS, ... with T workgroups each
        const uint32_t want = T * ((nqb - cls + PRO_COUNTERS - 1) / PRO_COUNTERS);
        last_sh = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == want - 1u;
    }
    __syncthreads();
    if (!last_sh) return;  // workgroup-uniform: only the class's last arriver goes on, and it waits for nobody
    if (threadIdx.x == 0) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t mq = cls * PRO_WAVES + (uint32_t)wave; mq < a.nq; mq += PRO_COUNTERS * PRO_WAVES) {
        WaveTopK<E> tk;
        tk.init((int)a.k);
        for (uint32_t g0 = 0; g0 < T; g0 += 64) {
            const uint32_t list = g0 + lane;
            const bool have = list < T;
            const gu64 *lp = (const gu64 *)(pro.lists + ((size_t)mq * T + (have ? list : 0u)) * kk);
            for (uint32_t r0 = 0; r0 < kk; r0 += PRO_CHUNK) {
                uint64_t c[PRO_CHUNK];
#pragma unroll
                for (int i = 0; i < PRO_CHUNK; i++)
                    c[i] = have && r0 + i < kk ? __hip_atomic_load(lp + r0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                               : WVG_KEY_NONE;
                // through LDS (the lane's own words): one rolled loop offers them, tk's code stands once
#pragma unroll
                for (int i = 0; i < PRO_CHUNK; i++) stage[wave][i][lane] = c[i];
                const uint32_t n = kk - r0 < (uint32_t)PRO_CHUNK ? kk - r0 : (uint32_t)PRO_CHUNK;
                bool stop = false;
#pragma unroll 1
                for (uint32_t i = 0; i < n; i++) {
                    const uint64_t key = stage[wave][i][lane];
                    if (r0 + i > 0 && __ballot(key < tk.tau) == 0ull) {  // sorted lists: the rest cannot enter
                        stop = true;
                        break;
                    }
                    tk.offer(key);
                }
                if (stop) break;
            }
        }
        if (lane == 0) a.seeds[mq] = tk.tau;  // element k - 1, KEY_NONE while the list is not full
    }
}

template <int METRIC, int D, int E>
__global__ __launch_bounds__(PRO_WAVES * 64) void qshare_seed_kernel(QShareArgs a, QSharePro pro)
{
    qshare_seed_body<METRIC, D, E, false>(a, pro, QShareFilt{}, blockDim.x, gridDim.x);
}

template <int METRIC, int D, int E>
__global__ __launch_bounds__(PRO_WAVES * 64) void qshare_seed_filt_kernel(QShareArgs a, QSharePro pro, QShareFilt f)
{
    qshare_seed_body<METRIC, D, E, true>(a, pro, f, blockDim.x, gridDim.x);
}

// The prologue without a sample (the runtime-dimension form runs unseeded): the
// ready words zeroed, every seed open.
__global__ __launch_bounds__(SEED_WAVES * 64) void qshare_open_seed_kernel(QShareArgs a)
{
    const uint64_t nready = (uint64_t)a.nq * a.groups;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nready; i += (uint64_t)gridDim.x * blockDim.x)
        a.ready[i] = 0u;
    if (threadIdx.x == 0) a.seeds[blockIdx.x] = WVG_KEY_NONE;  // gridDim.x == nq
}

// The end of a pass: every wave leaves its QP lists in LDS, then wave w merges
// the SCAN_WAVES lists of the pass's queries w, w + SCAN_WAVES, ... and publishes
// each as group_combine_publish does (write-through stores, the storing wave's
// own drain, then the list's ready word).  Keys are unique, so the merge order
// does not change a list.
// FRESH: the lane's addresses are formed here and not held in registers through
// the scan (the screened form has none to spare).
template <int E, int QP, bool FRESH = false>
__device__ __forceinline__ void pass_combine_publish(WaveTopK<E> (&tk)[QP], uint32_t nqp, uint32_t k, uint64_t *partials,
                                                     uint32_t *ready, size_t list0, uint32_t G, bool more)
{
    __shared__ uint64_t psh[QP][SCAN_WAVES][64 * E];
    int lane = threadIdx.x & 63;
    if constexpr (FRESH) asm volatile("" : "+v"(lane));
    const int wave = wave_id();
#pragma unroll
    for (int j = 0; j < QP; j++)
#pragma unroll
        for (int e = 0; e < E; e++) psh[j][wave][e * 64 + lane] = tk[j].l[e];
    __syncthreads();
    for (uint32_t j = (uint32_t)wave; j < nqp; j += SCAN_WAVES) {
        uint64_t l[E];
#pragma unroll
        for (int e = 0; e < E; e++) l[e] = psh[j][0][e * 64 + lane];
#pragma unroll
        for (int w = 1; w < SCAN_WAVES; w++) {
            uint64_t o[E];
#pragma unroll
            for (int e = 0; e < E; e++) o[e] = psh[j][w][e * 64 + lane];
            merge_lists<E>(l, o);
        }
        const size_t li = list0 + (size_t)j * G;
        uint64_t *out = partials + li * k;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t i = e * 64 + lane;
            if (i < k) __hip_atomic_store((gu64 *)(out + i), l[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store((gu32 *)(ready + li), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (more) __syncthreads();  // psh is reused by the next pass
}

// The screen of one tile (the bound at the top of the file): per lane, the
// queries of the pass that must be scored exactly on the lane's row (bit j =
// query j; 0 for a dead lane).  xs = the lane's row, qsh = the pass's bf16
// queries (QS_QROW uint4 each), kq = their {Nq2, K1q, K2q, Cq}, m = the tile's
// validity word.  32 k-steps x 4 query groups of MFMAs; a ds_read_b128 per group
// feeds two k-steps.
// FILT: mq[j] = the tile's validity word & query j's allow word (subsets of m).  A query whose
// mq[j] is empty is skipped (wave-uniform) and bit j survives only on the lanes of mq[j]: the
// scalar word is the lanes' condition where the query is combined, no per-lane copy of it is held.
template <int QP, bool FILT>
__device__ __forceinline__ uint32_t screen_tile(const float4 (&xs)[QS_D / 4], const uint4 *qsh, cf4 *kq,
                                                const WaveTopK<1> (&tk)[QP], uint32_t nqp, uint64_t m,
                                                const uint64_t (&mq)[FILT ? QP : 1], int lane)
{
    static_assert(QP == 16, "four query groups of four");
    f2v n2a = {0.0f, 0.0f}, n2b = {0.0f, 0.0f};
    floatx4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; g++) acc[g] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    const uint4 *ql = qsh + (lane & 3) * QS_QROW;
#pragma unroll
    for (int c = 0; c < QS_D / 4; c += 2) {
        uint4 aq[4];
#pragma unroll
        for (int g = 0; g < 4; g++) aq[g] = ql[g * 4 * QS_QROW + c / 2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const float4 x = xs[c + h];
            const f2v xlo = {x.x, x.y}, xhi = {x.z, x.w};
            n2a = __builtin_elementwise_fma(xlo, xlo, n2a);
            n2b = __builtin_elementwise_fma(xhi, xhi, n2b);
            const shortx4 b = bf16_of(x);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const uint2 w = h ? make_uint2(aq[g].z, aq[g].w) : make_uint2(aq[g].x, aq[g].y);
                acc[g] = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(__builtin_bit_cast(shortx4, w), b, acc[g], 0, 0, 0);
            }
        }
    }
    const f2v n2 = n2a + n2b;
    const float nx2 = n2.x + n2.y;
    const float nx = __builtin_amdgcn_sqrtf(nx2) * (1.0f + 0x1p-16f);
    const float bx = nx2 * (1.0f - QS_G);
    uint32_t adm = 0u;
#pragma unroll
    for (int j = 0; j < QP; j++) {
        if ((uint32_t)j < nqp && (!FILT || mq[FILT ? j : 0] != 0ull)) {  // wave-uniform
            const f4v k = kq[j];
            const float t = __builtin_fmaf(-2.0f, acc[j >> 2][j & 3], bx + k.w);
            const float lower = __builtin_fmaf(-k.y, nx, t);
            const float tau_dist = wvg_unord_f32((uint32_t)(tk[j].tau >> 32));  // NaN for an open tau
            bool skip = lower > tau_dist && lower < __builtin_inff();
            // (the scalar word as the lanes' condition: one scalar AND with the compare's mask)
            if constexpr (FILT) skip = skip || !__builtin_amdgcn_inverse_ballot_w64(mq[FILT ? j : 0]);
            adm |= skip ? 0u : 1u << j;
        }
    }
    if constexpr (FILT) return adm;
    return ((m >> lane) & 1ull) ? adm : 0u;
}

// The allow words of tile t for the nqp queries of a pass (al = the pass's first query's row): one
// window test for the pass, then a scalar load per query.
template <int QP>
__device__ __forceinline__ void pass_allow_words(uint64_t (&aw)[QP], cu64 *al, uint64_t stride, uint64_t t0, uint64_t t,
                                                 uint32_t nqp)
{
    const uint64_t w = t - t0;
    const bool in = w < stride;  // wave-uniform
#pragma unroll
    for (int j = 0; j < QP; j++) aw[j] = in && (uint32_t)j < nqp ? al[(size_t)j * stride + w] : 0ull;
}

// SCREEN: the bf16 screen per tile, then rounds of the exact chain per admitted row (WHOLE, L2, d = 128, E = 1).
// FILT: per tile and query j of the pass mq[j] = valid & query j's allow word (QShareFilt); a tile
// whose mq[j] are all empty is skipped before its row loads, and query j's keys come from the lanes of mq[j].
template <int METRIC, int D, int E, bool WHOLE, bool SCREEN, bool FILT>
__device__ __forceinline__ void qshare_scan_body(const QShareArgs &a, const QShareFilt &f)
{
    static_assert(D % 32 == 0 && D >= 0 && !is_abs_or_neq<METRIC>, "shared rows: fixed D (0 = a.dim), the AVX2 chains");
    static_assert(!SCREEN || (WHOLE && METRIC == WVG_M_L2 && D == QS_D && E == 1), "the screened form");
    static_assert(D > 0 || !WHOLE, "the runtime dimension takes the block shape");
    constexpr int QP = qshare_qp(D, E, WHOLE);
    constexpr int NC = D / 4;
    const int nb = D ? D / 32 : (int)(a.dim >> 5);  // 32-float blocks of a row
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
    static_assert(!SCREEN || QP * 16 == SCAN_WAVES * 64, "the LDS image copy: one thread per (query, 16 bytes)");
    __shared__ uint4 qsh[SCREEN ? QP * QS_QROW : 1];  // SCREEN: the pass's bf16 queries
    __shared__ f4v qfsh[SCREEN ? QP * QS_FROW : 1];   // SCREEN: the pass's fp32 queries (the rounds' operands)
#ifdef WVG_TOOLS
    // SCREEN, of this wave: (query, tile) pairs with an admitted row, all (query, tile) pairs, rounds;
    // of this lane: admitted (query, row) pairs
    uint32_t n_fold = 0, n_pairs = 0, n_rounds = 0, n_adm = 0;
#endif
    for (uint32_t q0 = 0, pass = 0; q0 < a.nq; q0 += QP, pass++) {
        const uint32_t nqp = a.nq - q0 < (uint32_t)QP ? a.nq - q0 : (uint32_t)QP;  // queries of this pass
        const bool rev = ((a.reverse + pass) & 1u) != 0;  // serpentine over the passes
        // seeds: written by the prologue launch, read-only here (wave-uniform scalar loads)
        cu64 *sd = (cu64 *)a.seeds + q0;
        WaveTopK<E> tk[QP];
#pragma unroll
        for (int j = 0; j < QP; j++) tk[j].init_bounded((int)a.k, (uint32_t)j < nqp ? seed_bound(sd + j) : WVG_KEY_NONE);
        cf4 *qb = (cf4 *)a.queries + (size_t)q0 * qstride;
        if constexpr (SCREEN) {  // the pass's bf16 queries into LDS, thread = (query, 16 bytes); zero past nqp
            uint32_t tid = threadIdx.x;
            asm volatile("" : "+v"(tid));  // the per-thread addresses are formed here, not held in registers through the scan
            const uint32_t tq = tid >> 4, part = tid & 15;
            const uint4 *src = reinterpret_cast<const uint4 *>(a.qbf) + (size_t)q0 * (QS_D * 2 / 16);
            qsh[tq * QS_QROW + part] = tq < nqp ? src[tid] : make_uint4(0u, 0u, 0u, 0u);  // 16 parts per query
            // and the fp32 queries, two chunks per thread: thread = (query, chunk), (query + QP / 2, chunk)
            const f4v *srcf = reinterpret_cast<const f4v *>(a.queries) + (size_t)q0 * qstride;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint32_t fq = (tid >> 5) + h * (QP / 2), fc = tid & 31;
                qfsh[fq * QS_FROW + fc] = fq < nqp ? srcf[(size_t)fq * qstride + fc] : f4v{0.0f, 0.0f, 0.0f, 0.0f};
            }
            __syncthreads();  // (the last pass's readers are past pass_combine_publish's barriers)
        }
        uint64_t m_next = n ? valid[rev ? t1 - 1 : t0] : 0ull;
        // FILT: the pass's allow words of the next tile, prefetched with m_next (0 past nqp)
        cu64 *al = FILT ? (cu64 *)f.allow + (size_t)q0 * f.stride : nullptr;
        uint64_t aw_next[FILT ? QP : 1], mq[FILT ? QP : 1];
        if constexpr (FILT) {
            if (n) pass_allow_words<QP>(aw_next, al, f.stride, f.t0, rev ? t1 - 1 : t0, nqp);
        }
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t t = rev ? t1 - 1 - i : t0 + i;
            const uint64_t m = m_next;
            uint64_t many = m;
            if constexpr (FILT) {
                many = 0ull;
#pragma unroll
                for (int j = 0; j < QP; j++) {
                    mq[j] = m & aw_next[j];
                    many |= mq[j];
                }
            }
            if (i + 1 < n) {  // scalar prefetch of the next mask
                m_next = valid[rev ? t - 1 : t + 1];
                if constexpr (FILT) pass_allow_words<QP>(aw_next, al, f.stride, f.t0, rev ? t - 1 : t + 1, nqp);
            }
            if (many == 0ull) continue;  // wave-uniform: nothing live (FILT: and allowed for a query of the pass) in this tile
            const float4 *rp = data + (size_t)t * (D ? NC : (int)(a.dim >> 2)) * 64 + lane;
            if constexpr (WHOLE) {
                float4 xs[NC];
                if (i >= split) {
#pragma unroll
                    for (int c = 0; c < NC; c++) xs[c] = ld_stream<false>(rp + (size_t)c * 64);
                } else {
#pragma unroll
                    for (int c = 0; c < NC; c++) xs[c] = ld_stream<true>(rp + (size_t)c * 64);
                }
                if constexpr (SCREEN) {
                    // Row-level admission: the lane's mask of queries whose lower bound on its row does
                    // not exceed tau, then rounds of the exact chain -- a lane scores its own row against
                    // one of its own admitted queries per round, the query chunks read from LDS.
                    uint32_t adm = screen_tile<QP, FILT>(xs, qsh, (cf4 *)a.qconst + q0, tk, nqp, m, mq, lane);
#ifdef WVG_TOOLS
                    n_pairs += nqp;
                    n_adm += (uint32_t)__builtin_popcount(adm);
                    {
                        uint32_t any = 0u;
#pragma unroll
                        for (int j = 0; j < QP; j++) any |= __ballot(((adm >> j) & 1u) != 0u) != 0ull ? 1u << j : 0u;
                        n_fold += (uint32_t)__builtin_popcount(any);
                    }
#endif
                    while (true) {
                        const uint64_t took_any = __ballot(adm != 0u);  // the lanes that score a pair in this round
                        if (took_any == 0ull) break;  // wave-uniform
#ifdef WVG_TOOLS
                        n_rounds++;
#endif
                        const bool has = adm != 0u;
                        const uint32_t jl = has ? (uint32_t)__builtin_ctz(adm) : 0u;  // the lane's lowest admitted query
                        adm &= adm - 1u;
                        const f4v *ql = qfsh + jl * QS_FROW;
                        f2v acc[4][4];
#pragma unroll
                        for (int r = 0; r < 4; r++)
#pragma unroll
                            for (int p = 0; p < 4; p++) acc[r][p] = f2v{0.0f, 0.0f};
                        // (a read-ahead of two or four chunks written out here spills: the kernel sits at 255 registers)
#pragma unroll
                        for (int c = 0; c < NC; c++) chunk_update2<METRIC>(acc, c & 7, ql[c], xs[c]);
                        const uint64_t key = lane_key(m, wrap_metric(a.metric, avx256_reduce2(acc)), t, lane);
#pragma unroll
                        for (int j = 0; j < QP; j++) {
                            const uint64_t took = __ballot(jl == (uint32_t)j) & took_any;
                            if (took != 0ull)  // wave-uniform: some lane took query j in this round
                                tk[j].offer_bounded(((took >> lane) & 1ull) ? key : WVG_KEY_NONE,
                                                    [&] { return seed_bound(sd + j); });
                        }
                    }
                } else {
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
                            const uint32_t jn = (uint32_t)j + 1 < nqp ? j + 1 : j;
                            cf4 *qnext = qb + (size_t)jn * qstride;
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
                            tk[j].offer_bounded(lane_key(FILT ? mq[FILT ? j : 0] : m, wrap_metric(a.metric, avx256_reduce2(acc)), t, lane),
                                                [&] { return seed_bound(sd + j); });
                        }
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
                for (int b = 0; b < (D ? D / 32 : nb); b++) {
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
                float sum[QP];
#pragma unroll
                for (int j = 0; j < QP; j++) sum[j] = 0.0f;
                if constexpr (D == 0) {
                    // The rest of the AVX2 order (row_dot_or_l2_generic): each leftover 8-float block goes
                    // into accumulator row 0 (chunk positions 0 and 1), then four last elements one by one
                    // through scalar_update into the query's sum, which avx256_reduce adds last.
                    int c = nb * 8;
                    for (const int c4 = (int)(a.dim >> 2) & ~1; c < c4; c += 2) {
                        const float4 *p0 = rp + (size_t)c * 64, *p1 = p0 + 64;
                        const float4 x0 = dflt ? ld_stream<false>(p0) : ld_stream<true>(p0);
                        const float4 x1 = dflt ? ld_stream<false>(p1) : ld_stream<true>(p1);
#pragma unroll
                        for (int j = 0; j < QP; j++) {
                            chunk_update2<METRIC>(acc[j], 0, qj[j][c], x0);
                            chunk_update2<METRIC>(acc[j], 1, qj[j][c + 1], x1);
                        }
                    }
                    if (a.dim & 4u) {  // wave-uniform
                        const float4 x = dflt ? ld_stream<false>(rp + (size_t)c * 64) : ld_stream<true>(rp + (size_t)c * 64);
#pragma unroll
                        for (int j = 0; j < QP; j++) {
                            const f4v q = qj[j][c];
                            scalar_update<METRIC>(sum[j], q.x, x.x);
                            scalar_update<METRIC>(sum[j], q.y, x.y);
                            scalar_update<METRIC>(sum[j], q.z, x.z);
                            scalar_update<METRIC>(sum[j], q.w, x.w);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < QP; j++)
                    if ((uint32_t)j < nqp)
                        tk[j].offer_bounded(lane_key(FILT ? mq[FILT ? j : 0] : m, wrap_metric(a.metric, avx256_reduce2(acc[j], sum[j])), t, lane),
                                            [&] { return seed_bound(sd + j); });
            }
        }
#ifdef WVG_TOOLS
        if (a.seq_combine) {  // A/B: the queries combined one after another, wave 0 merging
#pragma unroll
            for (int j = 0; j < QP; j++) {
                if ((uint32_t)j < nqp) {  // workgroup-uniform
                    const size_t li = (size_t)(q0 + j) * G + blockIdx.x;
                    group_combine_publish<E, SCAN_WAVES>(tk[j], a.partials + li * a.k, nullptr, a.ready + li, 1u);
                }
            }
            continue;
        }
#endif
        pass_combine_publish<E, QP, SCREEN>(tk, nqp, a.k, a.partials, a.ready, (size_t)q0 * G + blockIdx.x, G, q0 + QP < a.nq);
    }
#ifdef WVG_TOOLS
    if constexpr (SCREEN) {  // two adds per wave: word 0 = (query, tile) pairs with an admitted row (low half)
                             // and all (query, tile) pairs (high half); word 1 = admitted (query, row) pairs
                             // (low half) and rounds (high half)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n_adm += __shfl_xor(n_adm, off);
        if (lane == 0 && n_pairs) {
            atomicAdd((unsigned long long *)a.screen_count, ((unsigned long long)n_pairs << 32) | n_fold);
            atomicAdd((unsigned long long *)a.screen_count + 1, ((unsigned long long)n_rounds << 32) | n_adm);
        }
    }
#endif
}

// (two waves per SIMD -- at most 256 registers -- so one wave's tile loads run under the other's folds)
template <int METRIC, int D, int E, bool WHOLE>
__global__ __launch_bounds__(SCAN_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_f32_qshare_kernel(
    QShareArgs a)
{
    qshare_scan_body<METRIC, D, E, WHOLE, false, false>(a, QShareFilt{});
}

template <int METRIC, int D, int E, bool WHOLE>
__global__ __launch_bounds__(SCAN_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_f32_qshare_filt_kernel(
    QShareArgs a, QShareFilt f)
{
    qshare_scan_body<METRIC, D, E, WHOLE, false, true>(a, f);
}

// The runtime-dimension block form (D = 0: every dimension qshare_supported admits but 128 and 768):
// a.dim >> 5 blocks, then the tail of the AVX2 order; 4 queries per pass, 2 at E = 4.
template <int METRIC, int E>
__global__ __launch_bounds__(SCAN_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_f32_qshare_dyn_kernel(
    QShareArgs a)
{
    qshare_scan_body<METRIC, 0, E, false, false, false>(a, QShareFilt{});
}

template <int METRIC, int E>
__global__ __launch_bounds__(SCAN_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_f32_qshare_dyn_filt_kernel(
    QShareArgs a, QShareFilt f)
{
    qshare_scan_body<METRIC, 0, E, false, false, true>(a, f);
}

// The screened form: L2, d = 128, k <= 64, whole rows.
__global__ __launch_bounds__(SCAN_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_f32_qshare_screen_kernel(
    QShareArgs a)
{
    qshare_scan_body<WVG_M_L2, QS_D, 1, true, true, false>(a, QShareFilt{});
}

__global__ __launch_bounds__(SCAN_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_f32_qshare_screen_filt_kernel(
    QShareArgs a, QShareFilt f)
{
    qshare_scan_body<WVG_M_L2, QS_D, 1, true, true, true>(a, f);
}

// The shadow-fed screened scan (scan_f32_qshare_shadow_kernel; QShareArgs::screen = 2).  The coverage,
// grid, row ranges, serpentine, seeds, lists, combine and mergers are the screened form's.  What differs is
// what a tile costs in memory: the fp32-screened kernel loads the lane's whole 512-byte row only to round
// it to bf16 and sum its squares, and about 3 rows of 64 ever use their fp32 values.  A corpus that has a
// bf16 shadow (shadow_frag_kernel's fragments and shadow_norm_kernel's norm bounds, kept current by
// ensure_shadow) already holds both results, so a tile is 16 fragments of 1 KiB (one 16-byte load per lane
// each, [kb 0..3][rg 0..3]) and 256 B of norms, and the fp32 values are gathered from a.data for admitted
// (query, row) pairs only.
//
// The operands: v_mfma_f32_16x16x32_bf16 with A = the pass's query fragment of k-block kb (held in 16
// registers for the pass), B = the tile's row fragment (kb, rg); four k-blocks chained into acc[rg].  The
// result register r of lane l is the dot of query 4 (l >> 4) + r with row 16 rg + (l & 15): a lane holds
// FOUR QUERIES x FOUR ROWS.  (Rows as A would give a lane one query and 16 rows: 16 norms and h terms per
// lane instead of 4, against 12 constants instead of 3 -- about the same registers -- but a lane's 16 rows
// x its query's allow word would need a per-lane 64-bit select of the 16 words; here the live mask of pair
// (rg, r) is one scalar word per pair, built from the 16-bit fields of the validity / allow words.)
// Admission bit 4 rg + r of the lane = that pair.
//
// The bound is K3c-L2's (wvg_screen.hip, "K3c-L2"), on exactly its operands: the stored fragments, the
// stored norm bounds Nx, and K1 / K2 / Cq from screen_l2_query_consts:
//   h = (Nx Nx) hg,  E1 = fma(Nx, K1q, K2q),  u = (s - h) + E1,  lower = max(Cq - 2 u, 0) <= r.
// Two things carry over unchanged.  The accumulation: K3c-L2's s is one v_mfma_f32_16x16x32_bf16 chain
// over the row's k-blocks in ascending order from a zero accumulator (screen_body's acc[mq][nr]), which is
// what acc[rg] is here -- four k-blocks at d = 128; its (b) covers the bf16 operands and that fp32
// accumulation whichever operand is A.  (a) is about r, the same AVX2-order chain (chunk_update2 is
// chunk_update on pairs).  The special values: a row with Nx > 2^60 (inf: a NaN / inf row) gets h = NaN; a
// query with Nq > 2^56 or not finite gets K1 = +inf, Cq = -inf; a NaN or infinite s makes u NaN or
// infinite.  Each ends in lower = NaN (taken as -inf, sc_lower_l2's rule), -inf, 0 or +inf, and a pair is
// skipped only if lower > tau_dist && lower < +inf with tau_dist NaN for an open tau: all of these admit.
// Results do not depend on the bound's slack (the argument at the top of the file holds for any sound
// bound): a pair that is not admitted holds no key below tau.
//
// The rounds are the screened form's with the row fetched on demand: a lane takes its lowest admitted pair
// (rg, r), loads row 16 rg + (l & 15) of tile t from a.data -- 32 chunks 1 KiB apart, default policy, only
// lanes that hold a pair -- and runs the unchanged chain against query 4 (l >> 4) + r from the fp32 LDS
// image; the key is built from (t, row).  A pair belongs to exactly one lane, so keys stay unique; a lane
// with two pairs on one row loads it twice (the second read hits cache).
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ bf16x8 ld_frag(const uint4 *p)
{
    if constexpr (NT) return __builtin_bit_cast(bf16x8, __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p)));
    else return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4 *>(p));
}

// Lanes (g, i) <- bit i of the 16-bit field rg of word[g]: the live rows 16 rg + i of a lane's pair.
__device__ __forceinline__ uint64_t field16(uint64_t w, int rg) { return (w >> (16 * rg)) & 0xFFFFull; }

template <bool FILT>
__device__ __forceinline__ void qshare_shadow_body(const QShareArgs &a, const QShareFilt &f)
{
    constexpr int QP = 16, NC = QS_D / 4;
    const uint32_t G = a.groups;
    if (blockIdx.x >= G) {  // the mergers, as qshare_scan_body's
        const uint32_t nm = gridDim.x - G;
        for (uint32_t q = blockIdx.x - G; q < a.nq; q += nm) {
            const bool got = merge_lists_ready<1, SCAN_WAVES>(
                a.partials + (size_t)q * G * a.k, a.ready + (size_t)q * G, 1u, G, a.k, a.wait_limit, a.id_base,
                a.ids ? a.ids + (size_t)q * a.k : nullptr, a.dists ? a.dists + (size_t)q * a.k : nullptr,
                a.counts ? a.counts + q : nullptr, nullptr, 0u);
            if (!got) {
                if (threadIdx.x == 0) atomicOr(a.status, WVG_STATUS_MERGE_TIMEOUT);
                fill_empty_body(a.ids, a.dists, a.counts, q, q + 1, a.k);
            }
            __syncthreads();
        }
        return;
    }
    const int lane = threadIdx.x & 63;
    const uint64_t ntiles = a.tile_end - a.tile_begin, total = (uint64_t)G * SCAN_WAVES;
    const uint64_t gw = (uint64_t)blockIdx.x * SCAN_WAVES + wave_id();
    const uint64_t t0 = a.tile_begin + ntiles * gw / total, t1 = a.tile_begin + ntiles * (gw + 1) / total;
    const uint64_t n = t1 - t0;
    const uint64_t split = a.cache_tail256 ? n - ((n * a.cache_tail256) >> 8) : (a.plain ? 0 : n);
    const float4 *data = reinterpret_cast<const float4 *>(a.data);
    const uint4 *shadow = reinterpret_cast<const uint4 *>(a.shadow);
    cu64 *valid = (cu64 *)a.valid;
    const uint32_t qstride = a.qpitch / 4;
    const float hg = a.hg;
    __shared__ f4v qfsh[QP * QS_FROW];  // the pass's fp32 queries (the rounds' operands)
#ifdef WVG_TOOLS
    uint32_t n_fold = 0, n_pairs = 0, n_rounds = 0, n_adm = 0;  // as qshare_scan_body's
#endif
    for (uint32_t q0 = 0, pass = 0; q0 < a.nq; q0 += QP, pass++) {
        const uint32_t nqp = a.nq - q0 < (uint32_t)QP ? a.nq - q0 : (uint32_t)QP;
        const bool rev = ((a.reverse + pass) & 1u) != 0;
        cu64 *sd = (cu64 *)a.seeds + q0;
        WaveTopK<1> tk[QP];
#pragma unroll
        for (int j = 0; j < QP; j++) tk[j].init_bounded((int)a.k, (uint32_t)j < nqp ? seed_bound(sd + j) : WVG_KEY_NONE);
        {  // the fp32 queries into LDS, two chunks per thread: thread = (query, chunk), (query + QP / 2, chunk)
            uint32_t tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
            const f4v *srcf = reinterpret_cast<const f4v *>(a.queries) + (size_t)q0 * qstride;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const uint32_t fq = (tid >> 5) + h * (QP / 2), fc = tid & 31;
                qfsh[fq * QS_FROW + fc] = fq < nqp ? srcf[(size_t)fq * qstride + fc] : f4v{0.0f, 0.0f, 0.0f, 0.0f};
            }
            __syncthreads();  // (the last pass's readers are past pass_combine_publish's barriers)
        }
        // the pass's query fragments and the lane's four queries' constants; a query past nqp is never
        // admitted (its fragment column and constants may hold anything: an MFMA result depends on its own
        // row and column only)
        const uint32_t jg = (uint32_t)(lane >> 4) * 4;
        bf16x8 qa[4];
        float k1[4], k2[4], cq[4];
        {
            const uint4 *qf = reinterpret_cast<const uint4 *>(a.qbf) + (size_t)(q0 >> 4) * 4 * 64 + lane;
#pragma unroll
            for (int kb = 0; kb < 4; kb++) qa[kb] = ld_frag<false>(qf + kb * 64);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float4 c = jg + r < nqp ? a.qconst[q0 + jg + r] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                k1[r] = c.x;
                k2[r] = c.y;
                cq[r] = c.z;
            }
        }
        uint64_t qlive[4];  // lanes whose query 4 (l >> 4) + r is one of the pass
#pragma unroll
        for (int r = 0; r < 4; r++) {
            qlive[r] = 0ull;
#pragma unroll
            for (int g = 0; g < 4; g++) qlive[r] |= (uint32_t)(4 * g + r) < nqp ? 0xFFFFull << (16 * g) : 0ull;
        }
        uint64_t m_next = n ? valid[rev ? t1 - 1 : t0] : 0ull;
        cu64 *al = FILT ? (cu64 *)f.allow + (size_t)q0 * f.stride : nullptr;
        uint64_t aw_next[FILT ? QP : 1], mq[FILT ? QP : 1];
        if constexpr (FILT) {
            if (n) pass_allow_words<QP>(aw_next, al, f.stride, f.t0, rev ? t1 - 1 : t0, nqp);
        }
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t t = rev ? t1 - 1 - i : t0 + i;
            const uint64_t m = m_next;
            uint64_t many = m;
            if constexpr (FILT) {
                many = 0ull;
#pragma unroll
                for (int j = 0; j < QP; j++) {
                    mq[j] = m & aw_next[j];
                    many |= mq[j];
                }
            }
            if (i + 1 < n) {  // scalar prefetch of the next mask
                m_next = valid[rev ? t - 1 : t + 1];
                if constexpr (FILT) pass_allow_words<QP>(aw_next, al, f.stride, f.t0, rev ? t - 1 : t + 1, nqp);
            }
            if (many == 0ull) continue;  // wave-uniform: nothing live (FILT: and allowed) in this tile
            const uint4 *sp = shadow + (size_t)t * (16 * 64) + lane;
            bf16x8 xb[4][4];
            if (i >= split) {
#pragma unroll
                for (int fr = 0; fr < 16; fr++) xb[fr >> 2][fr & 3] = ld_frag<false>(sp + fr * 64);
            } else {
#pragma unroll
                for (int fr = 0; fr < 16; fr++) xb[fr >> 2][fr & 3] = ld_frag<true>(sp + fr * 64);
            }
            float nx[4];
#pragma unroll
            for (int rg = 0; rg < 4; rg++) nx[rg] = a.norms[(size_t)t * 64 + 16 * rg + (lane & 15)];
            // tau of the lane's four queries, as a distance (NaN for an open tau)
            float taud[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                uint32_t hi = (uint32_t)(tk[r].tau >> 32);
#pragma unroll
                for (int g = 1; g < 4; g++) hi = (lane >> 4) == g ? (uint32_t)(tk[4 * g + r].tau >> 32) : hi;
                taud[r] = wvg_unord_f32(hi);
            }
            floatx4 acc[4];
#pragma unroll
            for (int rg = 0; rg < 4; rg++) acc[rg] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int kb = 0; kb < 4; kb++)
#pragma unroll
                for (int rg = 0; rg < 4; rg++)
                    acc[rg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[kb], xb[kb][rg], acc[rg], 0, 0, 0);
            uint32_t adm = 0u;
#pragma unroll
            for (int rg = 0; rg < 4; rg++) {
                const float nrm = nx[rg];
                const float h = nrm <= 0x1p60f ? (nrm * nrm) * hg : __builtin_nanf("");
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    // the pair's live lanes: row 16 rg + i valid (FILT: and allowed by query 4 g + r), the query in the pass
                    uint64_t live;
                    if constexpr (FILT) {
                        live = field16(mq[r], rg) | field16(mq[4 + r], rg) << 16 | field16(mq[8 + r], rg) << 32 |
                               field16(mq[12 + r], rg) << 48;  // (mq[j] = 0 past nqp)
                    } else {
                        live = (field16(m, rg) * 0x0001000100010001ull) & qlive[r];
                    }
                    if (live == 0ull) continue;  // wave-uniform
                    const float e1 = __builtin_fmaf(nrm, k1[r], k2[r]);
                    const float u = (acc[rg][r] - h) + e1;
                    float lower = cq[r] - 2.0f * u;
                    lower = lower != lower ? -__builtin_inff() : __builtin_fmaxf(lower, 0.0f);
                    const bool skip = (lower > taud[r] && lower < __builtin_inff()) || !__builtin_amdgcn_inverse_ballot_w64(live);
                    adm |= skip ? 0u : 1u << (4 * rg + r);
                }
            }
#ifdef WVG_TOOLS
            n_pairs += nqp;
            n_adm += (uint32_t)__builtin_popcount(adm);
            {  // (query, tile) pairs with an admitted row: query 4 g + r over the lanes of group g
                uint32_t any = 0u;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const uint64_t b = __ballot((adm & (0x1111u << r)) != 0u);
#pragma unroll
                    for (int g = 0; g < 4; g++) any |= ((b >> (16 * g)) & 0xFFFFull) != 0ull ? 1u << (4 * g + r) : 0u;
                }
                n_fold += (uint32_t)__builtin_popcount(any);
            }
#endif
            const float4 *tp = data + (size_t)t * NC * 64 + (lane & 15);
            while (true) {
                const uint64_t took_any = __ballot(adm != 0u);  // the lanes that score a pair in this round
                if (took_any == 0ull) break;  // wave-uniform
#ifdef WVG_TOOLS
                n_rounds++;
#endif
                const bool has = adm != 0u;
                const uint32_t b = has ? (uint32_t)__builtin_ctz(adm) : 0u;  // the lane's lowest admitted pair
                adm &= adm - 1u;
                const uint32_t jl = jg + (b & 3u), row = (b >> 2) * 16 + (uint32_t)(lane & 15);
                uint64_t key = WVG_KEY_NONE;
                if (has) {  // only lanes that hold a pair load
                    const f4v *ql = qfsh + jl * QS_FROW;
                    const float4 *xr = tp + (b >> 2) * 16;
                    f2v c2[4][4];
#pragma unroll
                    for (int r = 0; r < 4; r++)
#pragma unroll
                        for (int p = 0; p < 4; p++) c2[r][p] = f2v{0.0f, 0.0f};
                    // The row streams through a ring of RING chunks: the first RING requested before the chain
                    // starts, chunk c + RING as chunk c is consumed.  (Written as xr[c] inside the chain the
                    // loads came out one at a time, each waited for -- 32 memory latencies per round; the
                    // whole row at once spills beside the lists.)
                    constexpr int RING = 16;
                    float4 x[RING];
#pragma unroll
                    for (int c = 0; c < RING; c++) x[c] = xr[(size_t)c * 64];
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        chunk_update2<WVG_M_L2>(c2, c & 7, ql[c], x[c % RING]);
                        if (c + RING < NC) x[c % RING] = xr[(size_t)(c + RING) * 64];
                    }
                    key =wvg_make_key(wrap_metric(a.metric, avx256_reduce2(c2)), (uint32_t)(t * 64 + row));
                }
#pragma unroll
                for (int j = 0; j < QP; j++) {
                    const uint64_t took = __ballot(has && jl == (uint32_t)j);
                    if (took != 0ull)  // wave-uniform: some lane took query j in this round
                        tk[j].offer_bounded(((took >> lane) & 1ull) ? key : WVG_KEY_NONE, [&] { return seed_bound(sd + j); });
                }
            }
        }
        pass_combine_publish<1, QP, true>(tk, nqp, a.k, a.partials, a.ready, (size_t)q0 * G + blockIdx.x, G, q0 + QP < a.nq);
    }
#ifdef WVG_TOOLS
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_adm += __shfl_xor(n_adm, off);
    if (lane == 0 && n_pairs) {
        atomicAdd((unsigned long long *)a.screen_count, ((unsigned long long)n_pairs << 32) | n_fold);
        atomicAdd((unsigned long long *)a.screen_count + 1, ((unsigned long long)n_rounds << 32) | n_adm);
    }
#endif
}

// (two waves per SIMD, as the screened form; profiles/r21/qshare_shadow/)
__global__ __launch_bounds__(SCAN_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_f32_qshare_shadow_kernel(
    QShareArgs a)
{
    qshare_shadow_body<false>(a, QShareFilt{});
}

__global__ __launch_bounds__(SCAN_WAVES * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_f32_qshare_shadow_filt_kernel(
    QShareArgs a, QShareFilt f)
{
    qshare_shadow_body<true>(a, f);
}

// Which corpora the kernel covers, its queries per pass and its grid.
// (dim % 4: device search's own condition.  dim = 4 stays out: below 8 elements the reference returns the
// scalar sum without the reduction tree, and a -0.0 sum would differ.)
bool qshare_supported(int metric, uint32_t dim, int order512)
{
    return (metric == WVG_M_L2 || metric == WVG_M_DOT || metric == WVG_M_COSINE) && dim % 4 == 0 && dim >= 8 &&
           !order512;
}

// The kernels' D of a corpus: 128 and 768 have fixed forms, 0 = the runtime-dimension form.
static int qshare_fixed_dim(uint32_t dim)
{
#ifdef WVG_TOOLS
    if (tuning().qshare == 3) return 0;  // A/B: the runtime-dimension form at d = 128 and 768 too
#endif
    return dim == 128 || dim == 768 ? (int)dim : 0;
}

static bool qshare_whole(uint32_t dim)
{
#ifdef WVG_TOOLS
    if (tuning().qshare == 2) return false;  // A/B: the block shape at d = 128 too
#endif
    return qshare_fixed_dim(dim) == 128;
}

uint32_t qshare_queries_per_pass(uint32_t dim, uint32_t k)
{
    const int e = k <= 64 ? 1 : (k <= 128 ? 2 : 4);
    return (uint32_t)qshare_qp(qshare_fixed_dim(dim), e, qshare_whole(dim));
}

// Two 4-wave workgroups per CU (the kernels stay within 256 registers), every wave at least one tile.
uint32_t qshare_groups(uint64_t ntiles, int num_cus)
{
    const uint64_t g = std::min<uint64_t>((uint64_t)num_cus * 2, (ntiles + SCAN_WAVES - 1) / SCAN_WAVES);
    return (uint32_t)std::max<uint64_t>(g, 1);
}

// Seeding pays where a wave's range is short (at most qshare_seed_tpw tiles per
// wave; with long ranges the lists' start-up is nothing beside the scan) and the
// scan is bound by the VALU: at d = 768 a pass is bound by HBM, the start-up
// hides under the loads and the sample costs 6x the reads (1M x 768, 16
// queries: launch 1789 -> 1799 us, prologue 145 us), so only d = 128 is seeded.
constexpr uint64_t QSHARE_SEED_FLOOR = 32;
uint32_t qshare_seed_tiles(uint32_t dim, uint64_t ntiles, uint32_t groups)
{
    const Tuning &t = tuning();
    if (t.qshare_seed <= 0 || dim != 128 || groups == 0) return 0;
    if (ntiles / ((uint64_t)groups * SCAN_WAVES) > (uint64_t)t.qshare_seed_tpw) return 0;
    // Every sample tile has a wave of its own, so the prologue's time hardly grows with the sample; its reads
    // do.  Up to QSHARE_SEED_FLOOR tiles are sampled whatever the range (the sample of before); beyond that
    // the sample stays within 1 / qshare_seed_share of the range.
    const uint64_t share = std::max<uint64_t>(QSHARE_SEED_FLOOR, ntiles / (uint64_t)std::max(t.qshare_seed_share, 1));
    return (uint32_t)std::min({(uint64_t)t.qshare_seed, share, ntiles});
}

// The screened form runs where seeding runs, for L2 with k <= 64 and whole rows:
// dot / cosine, k > 64, d = 768 and unseeded shapes are at or near their memory
// floor or start with open lists, where everything folds anyway.
bool qshare_screened(int metric, uint32_t dim, uint32_t k, uint32_t seed_tiles)
{
    return tuning().qshare_screen != 0 && metric == WVG_M_L2 && dim == (uint32_t)QS_D && k <= 64 && seed_tiles > 0 &&
           qshare_whole(dim);
}

template <int METRIC, int E>
static hipError_t launch_seed_e(const QShareArgs &a, const QSharePro &pro, hipStream_t s, const QShareFilt *f)
{
    if (a.dim != 128 && a.dim != 768) {  // no sample and no screen at the other dimensions
        if (a.seed_tiles || a.screen) return hipErrorInvalidValue;
        hipLaunchKernelGGL(qshare_open_seed_kernel, dim3(a.nq), dim3(SEED_WAVES * 64), 0, s, a);
        return hipGetLastError();
    }
    if (a.seed_tiles && (!pro.lists || !pro.arrivals)) return hipErrorInvalidValue;
    // a workgroup per sample tile and block of PRO_WAVES queries (one block of queries without a sample)
    const uint64_t nwg = (uint64_t)(a.seed_tiles ? a.seed_tiles : 1u) * ((a.nq + PRO_WAVES - 1) / PRO_WAVES);
    if (nwg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    dim3 grid((uint32_t)nwg), block(PRO_WAVES * 64);
    if (f) {
        if (a.dim == 128)
            hipLaunchKernelGGL((qshare_seed_filt_kernel<METRIC, 128, E>), grid, block, 0, s, a, pro, *f);
        else
            hipLaunchKernelGGL((qshare_seed_filt_kernel<METRIC, 768, E>), grid, block, 0, s, a, pro, *f);
    } else if (a.dim == 128) {
        hipLaunchKernelGGL((qshare_seed_kernel<METRIC, 128, E>), grid, block, 0, s, a, pro);
    } else {
        hipLaunchKernelGGL((qshare_seed_kernel<METRIC, 768, E>), grid, block, 0, s, a, pro);
    }
    return hipGetLastError();
}

hipError_t launch_qshare_seed(const QShareArgs &a, const QSharePro &pro, hipStream_t s, const QShareFilt *f)
{
    if (!qshare_supported(a.metric, a.dim, 0) || a.nq == 0) return hipErrorInvalidValue;
    auto go = [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        if (a.k <= 64) return launch_seed_e<MM, 1>(a, pro, s, f);
        if (a.k <= 128) return launch_seed_e<MM, 2>(a, pro, s, f);
        return launch_seed_e<MM, 4>(a, pro, s, f);
    };
    return a.metric == WVG_M_L2 ? go(MetricTag<WVG_M_L2>{}) : go(MetricTag<WVG_M_DOT>{});
}

template <int METRIC, int E>
static hipError_t launch_qshare_e(const QShareArgs &a, uint32_t mergers, hipStream_t s, const QShareFilt *f)
{
    dim3 grid(a.groups + mergers), block(SCAN_WAVES * 64);
    if (a.screen) {
        if (METRIC != WVG_M_L2 || E != 1 || a.dim != QS_D || !a.qbf || !a.qconst) return hipErrorInvalidValue;
        if (a.screen == 2) {  // fed from the corpus's shadow
            if (!a.shadow || !a.norms) return hipErrorInvalidValue;
            if (f)
                launch_timed(scan_f32_qshare_shadow_filt_kernel, grid, block, 0, s, a, *f);
            else
                launch_timed(scan_f32_qshare_shadow_kernel, grid, block, 0, s, a);
            return hipGetLastError();
        }
        if (f)
            launch_timed(scan_f32_qshare_screen_filt_kernel, grid, block, 0, s, a, *f);
        else
            launch_timed(scan_f32_qshare_screen_kernel, grid, block, 0, s, a);
        return hipGetLastError();
    }
    if (qshare_fixed_dim(a.dim) == 0) {  // the runtime-dimension form
        if (f)
            launch_timed((scan_f32_qshare_dyn_filt_kernel<METRIC, E>), grid, block, 0, s, a, *f);
        else
            launch_timed((scan_f32_qshare_dyn_kernel<METRIC, E>), grid, block, 0, s, a);
        return hipGetLastError();
    }
    if (f) {  // the filtered forms: whole rows at d = 128, blocks at d = 768
        if (a.dim == 128)
            launch_timed((scan_f32_qshare_filt_kernel<METRIC, 128, E, true>), grid, block, 0, s, a, *f);
        else if (a.dim == 768)
            launch_timed((scan_f32_qshare_filt_kernel<METRIC, 768, E, false>), grid, block, 0, s, a, *f);
        else
            return hipErrorInvalidValue;
        return hipGetLastError();
    }
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

hipError_t launch_scan_f32_qshare(const QShareArgs &a, uint32_t mergers, hipStream_t s, const QShareFilt *f)
{
    if (!qshare_supported(a.metric, a.dim, 0) || mergers == 0) return hipErrorInvalidValue;
    auto go = [&](auto M) -> hipError_t {
        constexpr int MM = decltype(M)::value;
        if (a.k <= 64) return launch_qshare_e<MM, 1>(a, mergers, s, f);
        if (a.k <= 128) return launch_qshare_e<MM, 2>(a, mergers, s, f);
        return launch_qshare_e<MM, 4>(a, mergers, s, f);
    };
    return a.metric == WVG_M_L2 ? go(MetricTag<WVG_M_L2>{}) : go(MetricTag<WVG_M_DOT>{});
}

}  // namespace wvg

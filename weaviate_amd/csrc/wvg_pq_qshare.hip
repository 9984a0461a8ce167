// wvg_pq_qshare.hip -- the shared-row query stream of PQ corpora
// (wvg_search_device_pipelined[_filtered] on a WVG_KIND_PQ corpus, nq >= 2).
//
// K8 / K8b / K8e (wvg_pq.hip) give every (query, row range) a workgroup of its own: a
// batch of nq queries fetches the codes nq times, builds nq LUT images per range and
// repeats the address work of every lookup per query.  Here a wave loads a 64-row tile
// of codes once and scores it against every query of its pass: the grid is (row ranges,
// passes), pass p serves queries [p Q, min(nq, (p + 1) Q)), each with a WaveTopK of its
// own in registers.  The workgroup's LDS image holds the pass's Q LUTs side by side:
// entry (s, c) is the Q floats lut_0[s][c] .. lut_{Q-1}[s][c], so ONE address and ONE
// ds_read_b64 (Q = 2) / ds_read_b128 (Q = 4) per (row, segment) return the terms of all
// Q queries.  Each query's sum is the reference's sequential fp32 sum in segment order
// from float32(0), then Wrap (CH/product_quantization.go:85-104, 352-361): the results
// are those of nq separate K8 scans bit for bit.  Two plain launches, this scan and
// launch_merge_lists; no workgroup waits for another.  Tiled layout as K8:
// [tile][chunk][lane] uint4, lane = row, m = 32 rows rotated (pq_rotated).
#include "wvg_internal.hpp"
#include "wvg_rowdist.hpp"
#include "wvg_topk.hpp"

namespace wvg {

typedef float f32x2q __attribute__((ext_vector_type(2)));
typedef float f32x4q __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4q __attribute__((ext_vector_type(4)));

// Code loads: the default cache policy (PLAIN) or non-temporal.  A template argument, not a run-time
// branch (wvg_bq_qshare.hip: the compiler merges the two arms of such a branch and drops the hint).
template <bool PLAIN>
__device__ __forceinline__ uint4 ld_pq_codes(const uint4 *p)
{
    if constexpr (PLAIN) {
        return *p;
    } else {
        const u32x4q v = __builtin_nontemporal_load(reinterpret_cast<const u32x4q *>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    }
}

// Query j's allow word of tile t (PQShareArgs: word t - allow_t0, zero outside the window).
__device__ __forceinline__ uint64_t pq_qshare_allow(const PQShareArgs &a, uint32_t q, uint64_t t)
{
    const uint64_t w = t - a.allow_t0;
    return w < a.allow_stride ? a.allow[(size_t)q * a.allow_stride + w] : 0ull;
}

// ---- the rotated form: m = 32, ks = 256, Q = 4 ----------------------------------------------------
// K8b's schedule (wvg_pq.hip): lane l (x = l mod 32) reads segment (x + j) mod 32 at step j, so the
// lanes of a wave are on 32 different segments at every step, and works on two rows at once: during
// the pass over (cur, nxt) it finishes cur's row (segments x .. 31, steps 0 .. 31 - x) into A and
// starts nxt's row (segments 0 .. x - 1, steps 32 - x .. 31) into B, so both sums run in segment order.
// Rows are stored rotated by slot mod 32 = x: step j's code is stored byte j of cur's row (x + j < 32)
// or of nxt's row -- one v_bfi per dword with a per-lane byte mask merges the two rows.
//
// Image: entry (c, s) -- 16 bytes, the four queries' lut[s][c] -- at byte
//     (s >> 4) << 16 | c << 8 | (s & 15) << 4,
// segments 0-15 in the lower 64 KiB and 16-31 in the upper.  The 16-byte bank quad of a read is
// (addr / 16) mod 16 = s mod 16, and each of ds_read_b128's lane groups holds 16 lanes whose x + j mod 16
// are all different, so the reads are conflict-free whatever the codes are.  The three address bytes
// come from ONE v_perm_b32: byte 1 is the code (a byte of the merged code word), bytes 0 and 2 are
// ((x + j) & 15) << 4 and ((x + j) >> 4) & 1, per-lane constants kept two steps to a register.
//
// Routing: whether step j belongs to A or to B depends on the lane only through x + j < 32, i.e.
// x < 32 - j: for a given j a CONSTANT lane mask.  The two packed adds into A run with the execution
// mask narrowed to that mask, the two into B with the rest; a lane that is off keeps its accumulator
// untouched, so every accumulator sees exactly its own terms in order: no +0.0 terms, no selects.
constexpr uint32_t PQ_ROT_IMG_BYTES = 32u * 256u * 16u;

// The mask is the same 32 bits for both halves of the wave, an instruction literal (MK: lanes with
// x < 32 - j).  The execution mask the block was entered with is put back at its end.
template <uint32_t MK>
__device__ __forceinline__ void rot_step_add(f32x2q &a0, f32x2q &a1, f32x2q &b0, f32x2q &b1, const f32x4q v)
{
    const f32x2q v0 = {v.x, v.y}, v1 = {v.z, v.w};
    uint64_t sv;
    asm("s_mov_b64 %[sv], exec\n\t"
        "s_and_b32 exec_lo, exec_lo, %[mk]\n\t"
        "s_and_b32 exec_hi, exec_hi, %[mk]\n\t"
        "v_pk_add_f32 %[a0], %[a0], %[v0]\n\t"
        "v_pk_add_f32 %[a1], %[a1], %[v1]\n\t"
        "s_xor_b64 exec, exec, %[sv]\n\t"
        "v_pk_add_f32 %[b0], %[b0], %[v0]\n\t"
        "v_pk_add_f32 %[b1], %[b1], %[v1]\n\t"
        "s_mov_b64 exec, %[sv]"
        : [a0] "+v"(a0), [a1] "+v"(a1), [b0] "+v"(b0), [b1] "+v"(b1), [sv] "=&s"(sv)
        : [v0] "v"(v0), [v1] "v"(v1), [mk] "n"(MK)
        : "scc");
}

// lanes with x < 32 - j, x = lane mod 32 (one half of the wave)
constexpr uint32_t rot_amask(int j) { return j == 0 ? 0xFFFFFFFFu : ((1u << (32 - j)) - 1u); }

// steps J .. JE - 1 of a batch that began at step J0: v[J - J0] into (A, B)
template <int J0, int J, int JE, int NB>
__device__ __forceinline__ void rot_batch_add(f32x2q &a0, f32x2q &a1, f32x2q &b0, f32x2q &b1, const f32x4q (&v)[NB])
{
    rot_step_add<rot_amask(J)>(a0, a1, b0, b1, v[J - J0]);
    if constexpr (J + 1 < JE) rot_batch_add<J0, J + 1, JE, NB>(a0, a1, b0, b1, v);
}

// batch H of the 32 steps: its NB reads all in flight, then their adds in step order
template <int H, int NB>
__device__ __forceinline__ void rot_batch(f32x2q &a0, f32x2q &a1, f32x2q &b0, f32x2q &b1, const char *imgb,
                                          const uint32_t (&kc)[16], const uint32_t (&win)[8])
{
    f32x4q v[NB];
#pragma unroll
    for (int jj = 0; jj < NB; jj++) {
        const int j = H * NB + jj;
        const uint32_t sel = 0x0C000000u | ((uint32_t)(5 + 2 * (j & 1)) << 16) | ((uint32_t)(j & 3) << 8) |
                             (uint32_t)(4 + 2 * (j & 1));
        const uint32_t off = __builtin_amdgcn_perm(kc[j >> 1], win[j >> 2], sel);
        v[jj] = *reinterpret_cast<const f32x4q *>(imgb + off);
    }
    rot_batch_add<H * NB, H * NB, H * NB + NB, NB>(a0, a1, b0, b1, v);
    if constexpr ((H + 1) * NB < 32) rot_batch<H + 1, NB>(a0, a1, b0, b1, imgb, kc, win);
}

// ---- the kernel -----------------------------------------------------------------------------------
// E: 64-key registers per list (k <= 64 E).  ROT: the rotated form above (Q = 4), else the generic
// form: any m, ks <= 256, partial chunks; all lanes on the same segment, the image in segment order
// (entry (s, c) at float (s ks + c) Q), bank conflicts accepted; m = 32 rows (ks < 256) un-rotated
// through pq32_window.  FILT: per-query allow words.  PLAIN: ld_pq_codes.
// Queries of the last pass that do not exist (j >= nqp) have +0.0 image entries and are never offered.
// No global store inside the scan loop (WaveTopK::offer_dist_emit explains what one costs).
template <int E, bool ROT, int Q, bool FILT, bool PLAIN>
__global__ __launch_bounds__(PQ_QSHARE_WAVES * 64) void scan_pq_qshare_kernel(PQShareArgs a)
{
    static_assert(Q == 2 || Q == 4, "8- or 16-byte image entries");
    static_assert(!ROT || Q == 4, "the rotated form has 16-byte entries");
    extern __shared__ __attribute__((aligned(16))) float img[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t rng = blockIdx.x, G = gridDim.x, q0 = blockIdx.y * Q;
    const uint32_t nqp = min((uint32_t)Q, a.nq - q0);  // queries of this pass (>= 1: gridDim.y = ceil(nq / Q))
    const bool rev = ((a.reverse + blockIdx.y) & 1u) != 0u;  // one direction per pass
    const uint32_t m = ROT ? 32u : a.m, ks = ROT ? 256u : a.ks;
    const float *gl = a.luts + (size_t)q0 * a.lpitch;
    // the pass's image: thread i reads the Q queries' entry i (coalesced per query) and writes it once
    for (uint32_t i = threadIdx.x; i < m * ks; i += PQ_QSHARE_WAVES * 64) {
        float v[Q];
#pragma unroll
        for (int j = 0; j < Q; j++) v[j] = (uint32_t)j < nqp ? gl[(size_t)j * a.lpitch + i] : 0.0f;
        uint32_t off;  // in floats
        if constexpr (ROT) {
            const uint32_t s = i >> 8, c = i & 255u;
            off = ((s >> 4) << 14) | (c << 6) | ((s & 15u) << 2);
        } else {
            off = i * Q;
        }
        if constexpr (Q == 4)
            *reinterpret_cast<f32x4q *>(img + off) = f32x4q{v[0], v[1], v[2], v[3]};
        else
            *reinterpret_cast<f32x2q *>(img + off) = f32x2q{v[0], v[1]};
    }
    __syncthreads();
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
    // live rows of tile t some query of the pass may take (wave-uniform)
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
    // first i' >= i whose tile has such a row (n if none), its word in w
    auto next_live = [&](uint64_t i, uint64_t &w) {
        for (; i < n; ++i) {
            w = live_word(tile_of(i));
            if (w) break;
        }
        return i;
    };
    // the tile's sums to the lists of the queries that take a row of it
    auto offer_all = [&](const float (&sum)[Q], uint64_t t, uint64_t live) {
#pragma unroll
        for (int j = 0; j < Q; j++) {
            if ((uint32_t)j < nqp) {
                uint64_t mq = live;
                if constexpr (FILT) mq &= pq_qshare_allow(a, q0 + j, t);
                if (mq) tk[j].offer_dist_fast(wrap_metric(a.metric, sum[j]), (uint32_t)(t * 64 + lane), mq);
            }
        }
    };
    if constexpr (ROT) {
        const uint32_t x = (uint32_t)lane & 31u;
        uint32_t nmask[8];  // bytes taken from the next tile's row: stored byte b with b + x >= 32
#pragma unroll
        for (int w = 0; w < 8; w++) {
            uint32_t mk = 0u;
#pragma unroll
            for (int bb = 0; bb < 4; bb++) mk |= (4u * w + bb + x >= 32u) ? (0xFFu << (8 * bb)) : 0u;
            nmask[w] = mk;
        }
        uint32_t kc[16];  // address bytes 0 and 2 of steps 2i (low half) and 2i + 1 (high half)
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t sa = (x + 2u * i) & 31u, sb = (x + 2u * i + 1u) & 31u;
            kc[i] = ((sa & 15u) << 4) | ((sa >> 4) << 8) | ((sb & 15u) << 20) | ((sb >> 4) << 24);
        }
        const char *imgb = reinterpret_cast<const char *>(img);
        // The chain of live tiles L_0 .. L_{c-1}: pass i has cur = L_{i-1} and nxt = L_i ("no tile" = zero
        // codes, whose lookups land on code 0 and whose sums nobody takes); pass i offers cur's rows.
        uint32_t cur[8], nxt[8];
#pragma unroll
        for (int w = 0; w < 8; w++) cur[w] = 0u;
        f32x2q a0 = {0.0f, 0.0f}, a1 = {0.0f, 0.0f}, b0 = {0.0f, 0.0f}, b1 = {0.0f, 0.0f};
        uint64_t m_cur = 0, m_nxt = 0, t_cur = 0;
        bool have_cur = false;
        uint64_t i = next_live(0, m_nxt);
        while (have_cur || i < n) {
            const bool have_nxt = i < n;
            const uint64_t t_nxt = have_nxt ? tile_of(i) : 0;
            if (have_nxt) {
                const uint4 *rp = data + (size_t)t_nxt * 2 * 64 + lane;
                const uint4 lo = ld_pq_codes<PLAIN>(rp), hi = ld_pq_codes<PLAIN>(rp + 64);
                nxt[0] = lo.x; nxt[1] = lo.y; nxt[2] = lo.z; nxt[3] = lo.w;
                nxt[4] = hi.x; nxt[5] = hi.y; nxt[6] = hi.z; nxt[7] = hi.w;
            } else {
#pragma unroll
                for (int w = 0; w < 8; w++) nxt[w] = 0u;
            }
            uint32_t win[8];
#pragma unroll
            for (int w = 0; w < 8; w++) win[w] = (nxt[w] & nmask[w]) | (cur[w] & ~nmask[w]);
            rot_batch<0, 8>(a0, a1, b0, b1, imgb, kc, win);  // (8 reads in flight before their adds)
            if (have_cur) {
                const float sum[Q] = {a0.x, a0.y, a1.x, a1.y};
                offer_all(sum, t_cur, m_cur);
            }
            a0 = b0;
            a1 = b1;
            b0 = f32x2q{0.0f, 0.0f};
            b1 = f32x2q{0.0f, 0.0f};
#pragma unroll
            for (int w = 0; w < 8; w++) cur[w] = nxt[w];
            have_cur = have_nxt;
            t_cur = t_nxt;
            m_cur = m_nxt;
            if (have_nxt) i = next_live(i + 1, m_nxt);
        }
    } else {
        const uint32_t nch = a.nchunks;
        // one (row, segment) lookup: the Q queries' terms from one read
        auto add_seg = [&](float (&sum)[Q], uint32_t s, uint32_t code) {
            const float *e = img + ((size_t)s * ks + code) * Q;
            if constexpr (Q == 4) {
                const f32x4q v = *reinterpret_cast<const f32x4q *>(e);
                sum[0] = sum[0] + v.x;
                sum[1] = sum[1] + v.y;
                sum[2] = sum[2] + v.z;
                sum[3] = sum[3] + v.w;
            } else {
                const f32x2q v = *reinterpret_cast<const f32x2q *>(e);
                sum[0] = sum[0] + v.x;
                sum[1] = sum[1] + v.y;
            }
        };
        uint64_t live = 0;
        for (uint64_t i = next_live(0, live); i < n; i = next_live(i + 1, live)) {
            const uint64_t t = tile_of(i);
            const uint4 *rp = data + (size_t)t * nch * 64 + lane;
            float sum[Q];
#pragma unroll
            for (int j = 0; j < Q; j++) sum[j] = 0.0f;
            if (pq_rotated(m)) {  // stored rotated by slot mod 32: back to segment order
                const uint4 lo = ld_pq_codes<PLAIN>(rp), hi = ld_pq_codes<PLAIN>(rp + 64);
                const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                uint32_t o[8];
                pq32_window(w, (32u - ((uint32_t)lane & 31u)) & 31u, o);
#pragma unroll
                for (int s = 0; s < 32; s++) add_seg(sum, (uint32_t)s, (o[s >> 2] >> (8 * (s & 3))) & 0xFFu);
            } else {
                for (uint32_t c = 0; c < nch; c++) {
                    const uint4 xw = ld_pq_codes<PLAIN>(rp + (size_t)c * 64);
                    const uint32_t ws[4] = {xw.x, xw.y, xw.z, xw.w};
#pragma unroll
                    for (int b = 0; b < 16; b++) {
                        const uint32_t s = c * 16 + b;
                        if (s < m) add_seg(sum, s, (ws[b >> 2] >> (8 * (b & 3))) & 0xFFu);
                    }
                }
            }
            offer_all(sum, t, live);
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
static bool pq_qshare_rot(uint32_t m, uint32_t ks) { return m == 32 && ks == 256; }

template <int E>
static uint32_t pq_qshare_q_e(uint32_t m, uint32_t ks)
{
    const size_t one = (size_t)m * ks * 4;
    if (pq_qshare_rot(m, ks) && fits_lds<&scan_pq_qshare_kernel<E, true, 4, false, false>>(PQ_ROT_IMG_BYTES)) return 4;
    if (fits_lds<&scan_pq_qshare_kernel<E, false, 4, false, false>>(4 * one)) return 4;
    if (fits_lds<&scan_pq_qshare_kernel<E, false, 2, false, false>>(2 * one)) return 2;
    return 1;
}

// Queries per pass: the largest of {4, 2} whose image (Q m ks 4 bytes) fits one workgroup's LDS beside the
// kernel's own static LDS (group_combine_store's buffer, 8 KiB x E), as the code object of the kernel
// that would be launched states it; 1 = no shared scan (at ks = 256: m >= 96).  A slice-wise image
// for those is not built.
uint32_t pq_qshare_queries_per_pass(uint32_t m, uint32_t ks, uint32_t k)
{
    if (m == 0 || ks == 0 || ks > 256 || k == 0 || k > 256) return 1;
    return k <= 64 ? pq_qshare_q_e<1>(m, ks) : k <= 128 ? pq_qshare_q_e<2>(m, ks) : pq_qshare_q_e<4>(m, ks);
}

// Row ranges of a shared-row PQ scan of ntiles tiles: one 16-wave workgroup per CU at most -- what a
// 128 KiB image lets a CU hold, so a pass is one round of workgroups -- and at least two tiles per
// wave where the corpus has them.
uint32_t pq_qshare_groups(uint64_t ntiles, int num_cus)
{
    const uint64_t cap = (uint64_t)std::max(num_cus, 1);
    return (uint32_t)std::min<uint64_t>(cap, std::max<uint64_t>(1, ntiles / (2 * PQ_QSHARE_WAVES)));
}

template <int E, bool ROT, int Q>
static void launch_pq_qshare_f(const PQShareArgs &a, dim3 grid, uint32_t lds, hipStream_t s)
{
    const dim3 block(PQ_QSHARE_WAVES * 64);
    if (a.allow) {
        if (a.plain)
            launch_timed((scan_pq_qshare_kernel<E, ROT, Q, true, true>), grid, block, lds, s, a);
        else
            launch_timed((scan_pq_qshare_kernel<E, ROT, Q, true, false>), grid, block, lds, s, a);
    } else {
        if (a.plain)
            launch_timed((scan_pq_qshare_kernel<E, ROT, Q, false, true>), grid, block, lds, s, a);
        else
            launch_timed((scan_pq_qshare_kernel<E, ROT, Q, false, false>), grid, block, lds, s, a);
    }
}

template <int E>
static hipError_t launch_pq_qshare_e(const PQShareArgs &a, uint32_t groups, hipStream_t s)
{
    const uint32_t qpp = pq_qshare_q_e<E>(a.m, a.ks);
    if (qpp < 2) return hipErrorInvalidValue;
    const uint32_t passes = (a.nq + qpp - 1) / qpp;
    if (passes > 65535u) return hipErrorInvalidValue;
    const dim3 grid(groups, passes);
    const uint32_t lds = qpp * a.m * a.ks * 4;
    if (qpp == 4 && pq_qshare_rot(a.m, a.ks) && a.nchunks == 2 &&
        fits_lds<&scan_pq_qshare_kernel<E, true, 4, false, false>>(PQ_ROT_IMG_BYTES))
        launch_pq_qshare_f<E, true, 4>(a, grid, PQ_ROT_IMG_BYTES, s);
    else if (qpp == 4)
        launch_pq_qshare_f<E, false, 4>(a, grid, lds, s);
    else
        launch_pq_qshare_f<E, false, 2>(a, grid, lds, s);
    return hipGetLastError();
}

hipError_t launch_scan_pq_qshare(const PQShareArgs &a, uint32_t groups, hipStream_t s)
{
    if (a.k == 0 || a.k > 256 || a.nq == 0 || groups == 0 || a.m == 0 || a.ks == 0 || a.ks > 256 ||
        a.nchunks != pq_chunks(a.m))
        return hipErrorInvalidValue;
    if (a.k <= 64) return launch_pq_qshare_e<1>(a, groups, s);
    if (a.k <= 128) return launch_pq_qshare_e<2>(a, groups, s);
    return launch_pq_qshare_e<4>(a, groups, s);
}

}  // namespace wvg

// wvg_pq_mfma.hip -- K8m: batched PQ ADC search on the bf16 matrix cores
// (option batch_screen = 6; DESIGN section 5, "K8m"), and K8m-S, its form for codebooks beyond LDS
// (option batch_screen = 7; below, above pqs_screen_kernel).
//
// For l2-squared the real-valued ADC distance of query q to a row with codes c is
//     sum_s |q_s - C_s[c_s]|^2 = |q|^2 + |x^|^2 - 2 q.x^,   x^ = the row decoded from the codebook,
// so Q x X^T is a GEMM and the only per-(query, row) work; the decode is per row and shared by the
// whole query block.  The GEMM runs in bf16 as a screen with K3c-L2's proven bound (below, above
// PqmArgs); the survivors are rescored with K8's own sum over the call's LUTs, so ids, distance
// bits, counts and padding are the default route's.
//
// Layout.  The codebook's bf16 image (round to nearest even), [segment][code][dsub], is built once
// per call and staged by every workgroup into LDS, next to its query block's B fragments (64 queries
// x dim bf16 in MFMA operand order).  Code bytes stay in the corpus's tiles ([tile][chunk][row] x
// 16 B; m = 32 rows rotated by their slot, pq_rotated) and never pass through LDS: for the 16-row
// MFMA tile mt of a 64-row tile, lane (r = lane % 16, g = lane / 16) loads the chunks of row
// 16 mt + r, and for K block kb of v_mfma_f32_16x16x32_bf16 gathers its 8 A elements 32 kb + 8 g ..
// + 7 of the decoded row from the image: two centroids (one ds_read_b64 each) at dsub = 4, one
// (ds_read_b128) at dsub = 8.  Each gathered fragment feeds the block's four query tiles.
//
// Work split.  Grid = row ranges x query blocks, one 4-wave workgroup per CU.  A step is 256 rows:
// wave w scores tile 4 step + w against the 64 queries, 4 row tiles x 4 query tiles of fp32
// accumulators; the next tile's code chunks and this tile's row norms are loaded before the MFMAs.
// Survivors claim a position in the (range, query) pool with one LDS atomic; pools, compaction
// (sc_compact), dropped bounds and the flag rule are K3c-W's, and so is the collect kernel.
// Per call, before the screen: the image and a per-centroid fp64 square-sum table (pqm_prep_kernel),
// every slot's norm upper bound from that table and the maximum over live rows (pqm_norms_kernel:
// one pass over the code bytes, no per-corpus state), the queries' fragments and constants
// (pqm_qconst_kernel).  After it: collect, pqm_rescore_keys_kernel, the key merge, and K8's generic
// scan for the flagged queries.  Every count, bound and flag is (re)initialised by these kernels.
#include "wvg_internal.hpp"
#include "wvg_screen_pool.hpp"

namespace wvg {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int PQM_WAVES = 4;
constexpr int PQM_QB = 64, PQM_NT = PQM_QB / 16;  // queries per workgroup, their 16-query MFMA tiles
constexpr int PQM_NCH = 4;                        // 16-byte code chunks per row held in registers: m <= 64

// The bound.  r = the fp32 value K8 returns: the sequential sum over the m segments of go_step's
// entries (per element diff = fl(q - c), fl(diff diff), fl(sum + .) over dsub elements).  D =
// |q - x^|^2 in real numbers, x^ the decoded row (the fp32 centroids); s = the bf16 MFMA dot of
// (bf16(q), bf16(x^)) -- the image is the element-wise bf16 of the centroids; Nq, Nx the norm upper
// bounds (sqrt of the fp64 square sum, (1 + 1e-6)).
//   (a) every rounding of r's chain is relative to a sum of non-negative terms, and a path through
//       it has 3 (the difference, counted twice by its square, and the square) + dsub (a segment's
//       adds) + m (the adds over segments) of them: D (1 - c_a) - 2^-130 <= r <= D (1 + c_a) +
//       2^-130 with c_a = (m + dsub + 6) 2^-24 (the second-order terms: (m + dsub)^2 2^-48 < 3
//       2^-24 for m + dsub <= 2^12; underflowing squares: <= d 2^-149 in all); D <= 2 (Nq^2 + Nx^2).
//   (b) |q.x^ - s| <= E1 = fma(Nx, K1q, K2q): K3c's constants with d (bf16 operands, the MFMA's
//       fp32 accumulation over d products).
//   (c) the combine h = fl(fl(Nx Nx) hg), w = fl(s - h), u = fl(w + E1), lower = fl(Cq - 2 u): three
//       roundings, in all <= 2^-21 (Nq^2 + Nx^2), as in K3c-L2.
// With alpha = 2 c_a + 2^-21 = (2 (m + dsub) + 20) 2^-24 (pq_mfma_alpha), hg and Cq are K3c-L2's at
// that alpha, and its obligations hold unchanged for every (query, row):
//   (a) lower <= r;   (b) r <= lower + 2 E_tot, E_tot = 2 E1 + beta (Nq^2 + Nx^2) + 2^-99, beta =
//   alpha + 2^-18;   (c) E_tot <= Emax_q = E_tot at the largest Nx of a live row (monotone in Nx).
// So tau = (k-th smallest lower) + 2 Emax_q bounds the k-th exact distance, and u < sigma_q
// (sc_sigma_l2, rounded down) proves lower > tau: one compare per element, a superset test.
// Non-finite and huge values never skip a row: a centroid that is NaN, inf or above 2^60 in norm
// gives its rows Nx = +inf or > 2^60, hence h = NaN and u = NaN; a query with Nq > 2^56 or a NaN
// gets K1 = +inf, Cq = -inf.  Both fail "u < sigma", take the per-element path with lower = -inf
// and are rescored exactly (in practice their pools overflow and the query is rescanned).
struct PqmArgs {
    const u32x4 *data;
    const uint64_t *valid, *allow;
    uint64_t allow_words, allow_t0, tile_begin, tile_end;
    uint32_t nch, m, ks, dim, rot;  // rot: rows stored rotated by slot mod 32 (m = 32)
    uint32_t nq, k, ranges, nqb, P;
    float hg;                       // (1 - (alpha + 2^-18)) / 2, rounded down
    const uint4 *image;             // [m][ks][dsub] bf16
    const uint4 *qfrag;             // [nqb][dim / 32][PQM_NT][64] x 16 B
    const float *norms;             // [(tile_end - tile_begin) * 64] Nx
    const float *k1, *k2, *cq, *emax;  // [nqb * 64]
    uint64_t *pools;                // [nq][ranges][P]
    uint32_t *pcnt, *pdrop;         // [nq][ranges]
    uint32_t *gbound;               // [nq]
};

// The codebook image and the per-centroid fp64 square sums; the call's bounds, maximum and flag count.
__global__ __launch_bounds__(256) void pqm_prep_kernel(const float *centers, uint32_t mks, uint32_t dsub, __bf16 *image,
                                                       double *sq, uint32_t *gbound, uint32_t nq, uint32_t *nmax,
                                                       uint32_t *nflag)
{
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g < mks) {
        double ss = 0.0;
        for (uint32_t e = 0; e < dsub; e++) {
            const float x = centers[(size_t)g * dsub + e];
            image[(size_t)g * dsub + e] = (__bf16)x;  // round to nearest even
            ss += (double)x * x;
        }
        sq[g] = ss;
    }
    if (g < nq) gbound[g] = 0xFFFFFFFFu;
    if (g == 0) {
        *nmax = 0;
        *nflag = 0;
    }
}

// Nx of every slot of [tile_begin, tile_end): the fp64 sum of the row's centroids' square sums,
// rounded up past the float cast (norm_upper); the maximum over live rows into *nmax.
__global__ __launch_bounds__(256) void pqm_norms_kernel(const u32x4 *data, uint32_t nch, uint32_t m, uint32_t ks,
                                                        uint32_t rot, const double *sq, const uint64_t *valid,
                                                        uint64_t tile_begin, uint64_t n, float *norms, uint32_t *nmax)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    float nv = 0.f;
    if (i < n) {
        const uint64_t slot = tile_begin * 64 + i;
        const u32x4 *rp = data + (slot >> 6) * nch * 64 + (slot & 63);
        double ss = 0.0;
        for (uint32_t c = 0; c < nch; c++) {
            const u32x4 x = rp[(size_t)c * 64];
            for (uint32_t b = 0; b < 16; b++) {
                const uint32_t p = 16 * c + b, s = rot ? (p + (uint32_t)slot) & 31u : p;  // stored byte p = code[s]
                const uint32_t code = min((x[b >> 2] >> (8 * (b & 3))) & 0xFFu, ks - 1);
                if (s < m) ss += sq[(size_t)s * ks + code];
            }
        }
        nv = norm_upper(ss);
        norms[i] = nv;
        if (!((valid[slot >> 6] >> (slot & 63)) & 1ull)) nv = 0.f;
    }
    // the wave's maximum, then one atomic (non-negative floats order as their bits)
    uint32_t b = __float_as_uint(nv);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) b = max(b, (uint32_t)__shfl_xor((int)b, off));
    if ((threadIdx.x & 63) == 0 && b) atomicMax(nmax, b);
}

// One wave per query of the padded batch: its bf16 B fragments in MFMA order (lane (col, g) of
// fragment (kb, nt) holds elements 32 kb + 8 g .. + 7 of query 16 nt + col; zeros for padding
// queries) and K1q, K2q, Cq, Emax_q as screen_qconst_l2_kernel computes them, at this route's alpha.
__global__ __launch_bounds__(256) void pqm_qconst_kernel(const float *q, uint32_t nq, uint32_t qpitch, uint32_t dim,
                                                         uint32_t nq_pad, double alpha, const uint32_t *nmax,
                                                         uint4 *qfrag, float *k1, float *k2, float *emax, float *cq)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq_pad) return;
    const uint32_t KB = dim / 32, qb = qi / PQM_QB, nt = (qi % PQM_QB) / 16, col = qi % 16;
    for (uint32_t idx = lane; idx < KB * 4; idx += 64) {
        const uint32_t kb = idx >> 2, g = idx & 3u;
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = (__bf16)(qi < nq ? q[(size_t)qi * qpitch + 32 * kb + 8 * g + e] : 0.0f);
        qfrag[(((size_t)qb * KB + kb) * PQM_NT + nt) * 64 + 16 * g + col] = *reinterpret_cast<const uint4 *>(&o);
    }
    double ss = 0.0;
    if (qi < nq)
        for (uint32_t i = lane; i < dim; i += 64) {
            const double x = q[(size_t)qi * qpitch + i];
            ss += x * x;
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    if (lane) return;
    float K1, K2, C;
    const float nq_up = screen_l2_query_consts(ss, dim, alpha, K1, K2, C);
    const double beta = alpha + 0x1p-18;
    const float nm = __uint_as_float(*nmax);
    const double e1 = __builtin_fmaf(nm, K1, K2);
    float E = (float)((2.0 * e1 + beta * ((double)nq_up * nq_up + (double)nm * nm) + 0x1p-99) * (1.0 + 0x1p-20));
    if (qi >= nq) K1 = K2 = C = E = 0.f;
    k1[qi] = K1;
    k2[qi] = K2;
    emax[qi] = E;
    cq[qi] = C;
}

__device__ __forceinline__ uint64_t pqm_tile_mask(const PqmArgs &a, uint64_t t)
{
    uint64_t m = a.valid[t];
    if (a.allow) {
        const uint64_t w = t - a.allow_t0;
        m &= w < a.allow_words ? a.allow[w] : 0ull;
    }
    return m;
}

template <int DSUB>
__global__ __launch_bounds__(PQM_WAVES * 64) void pqm_screen_kernel(PqmArgs a)
{
    constexpr int NT = PQM_NT, QB = PQM_QB;
    constexpr int KPC = DSUB == 4 ? 2 : 4;  // K blocks per 16-code chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t KB = a.dim / 32, img_bytes = a.dim * a.ks * 2, frag_vecs = KB * NT * 64;
    const bf16x8 *bl = reinterpret_cast<const bf16x8 *>(smem + img_bytes);
    float *ck1 = reinterpret_cast<float *>(smem + img_bytes + (size_t)frag_vecs * 16);  // [64] each
    float *ck2 = ck1 + QB, *ccq = ck2 + QB, *cem = ccq + QB;
    float *sig = cem + QB;    // u-space threshold of tadm
    float *tadm = sig + QB;   // what a wave admits: min(tau_q, the pool's dropped bound)
    float *wtau = tadm + QB;  // the query's valid bound tau_q
    uint32_t *cnt = reinterpret_cast<uint32_t *>(wtau + QB), *wdrop = cnt + QB, *flag = wdrop + QB;  // flag[2] by step parity

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the query blocks of one row range side by side on one XCD (K5 COS's order) where the ranges deal over the 8 XCDs
    uint32_t rng, qb;
    if (a.ranges % 8u == 0) {
        const uint32_t kk = blockIdx.x >> 3;
        rng = (kk / a.nqb) * 8u + (blockIdx.x & 7u);
        qb = kk % a.nqb;
    } else {
        rng = blockIdx.x / a.nqb;
        qb = blockIdx.x % a.nqb;
    }
    const uint32_t q0 = qb * QB, P = a.P, K = a.k, ks = a.ks;
    {
        uint4 *li = reinterpret_cast<uint4 *>(smem);
        for (uint32_t i = tid; i < img_bytes / 16; i += PQM_WAVES * 64) li[i] = a.image[i];
        uint4 *lf = reinterpret_cast<uint4 *>(smem + img_bytes);
        const uint4 *gf = a.qfrag + (size_t)qb * frag_vecs;
        for (uint32_t i = tid; i < frag_vecs; i += PQM_WAVES * 64) lf[i] = gf[i];
        if (tid < (uint32_t)QB) {
            const bool live = q0 + tid < a.nq;  // a padding query admits nothing
            ck1[tid] = a.k1[q0 + tid];
            ck2[tid] = a.k2[q0 + tid];
            ccq[tid] = a.cq[q0 + tid];
            cem[tid] = a.emax[q0 + tid];
            sig[tid] = live ? -__builtin_inff() : __builtin_inff();
            tadm[tid] = live ? __builtin_inff() : -__builtin_inff();
            wtau[tid] = __builtin_inff();
            cnt[tid] = 0;
            wdrop[tid] = 0xFFFFFFFFu;
        }
        if (tid < 2) flag[tid] = 0;
    }
    __syncthreads();

    // Compaction (workgroup-uniform entry): wave w takes queries w, w + 4, ... whose pool passed P - 256
    // (last: every query; the kept count, the dropped bound and tau_q are the range's output).
    auto compact = [&](bool last, uint32_t par) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the pools' stores
        __threadfence_block();
        __syncthreads();
        if (tid == 0) flag[par] = 0;
        for (uint32_t ql = wave; ql < (uint32_t)QB; ql += PQM_WAVES) {
            const uint32_t q = q0 + ql;
            if (q >= a.nq) break;
            const uint32_t raw = cnt[ql];
            if (!last && raw <= P - 256) continue;
            float t = wtau[ql];
            uint32_t kept = 0;
            if (raw > 0) {
                const uint64_t r = sc_compact(a.pools + ((size_t)q * a.ranges + rng) * P, min(raw, P), K, P - 256,
                                              cem[ql], 0, t, (lds_u32 *)(wdrop + ql));
                kept = (uint32_t)(r >> 32) & 0x7FFFFFFFu;
                t = __uint_as_float((uint32_t)r);
            }
            if (lane == 0) {
                if (raw > P) wdrop[ql] = 0;  // keys lost past the pool (never, by the step rule): always flagged
                const uint32_t dr = wdrop[ql];
                const float wt = dr == 0xFFFFFFFFu ? t : fminf(t, wvg_unord_f32(dr));  // (ord 0: NaN, fminf keeps t)
                cnt[ql] = kept;
                wtau[ql] = t;
                tadm[ql] = wt;
                sig[ql] = sc_sigma_l2(wt, ccq[ql]);
                if (last) {
                    a.pcnt[(size_t)q * a.ranges + rng] = kept;
                    a.pdrop[(size_t)q * a.ranges + rng] = dr;
                    if (t < __builtin_inff()) atomicMin(a.gbound + q, wvg_ord_f32(t));
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the packed pools
        __threadfence_block();
        __syncthreads();
    };

    const uint64_t ntiles = a.tile_end - a.tile_begin, nsteps = (ntiles + 3) / 4;
    const uint64_t s0 = nsteps * rng / a.ranges, s1 = nsteps * (rng + 1) / a.ranges;
    const uint32_t nch = a.nch, col = lane & 15u, g = lane >> 4;
    // the code chunks of rows 16 mt + col of tile T, mt = 0 .. 3
    auto load_rows = [&](uint64_t T, u32x4 (&dst)[4][PQM_NCH]) {
        const u32x4 *p = a.data + (size_t)T * nch * 64 + col;
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
            for (int c = 0; c < PQM_NCH; c++)
                if ((uint32_t)c < nch) dst[mt][c] = p[(size_t)c * 64 + 16 * mt];
    };
    u32x4 cur[4][PQM_NCH] = {}, nxt[4][PQM_NCH] = {};
    bool have = false;  // nxt holds this step's tile (loaded under the previous tile's MFMAs)
    for (uint64_t step = s0; step < s1; ++step) {
        const uint32_t par = (uint32_t)(step & 1ull);
        const uint64_t T = a.tile_begin + 4 * step + wave;
        const uint64_t mask = T < a.tile_end ? pqm_tile_mask(a, T) : 0ull;  // wave-uniform
        if (mask != 0ull) {
            if (have) {
#pragma unroll
                for (int mt = 0; mt < 4; mt++)
#pragma unroll
                    for (int c = 0; c < PQM_NCH; c++) cur[mt][c] = nxt[mt][c];
            } else {
                load_rows(T, cur);
            }
            have = step + 1 < s1 && T + 4 < a.tile_end;
            if (have) load_rows(T + 4, nxt);
            // the rows' norm bounds: element i of nv[mt] is row 16 mt + 4 g + i
            f32x4 nv[4];
            {
                const f32x4 *np = reinterpret_cast<const f32x4 *>(a.norms + (T - a.tile_begin) * 64) + g;
#pragma unroll
                for (int mt = 0; mt < 4; mt++) nv[mt] = np[4 * mt];
            }
            if (a.rot) {  // m = 32: back to segment order (stored byte b = code[(b + slot) mod 32])
#pragma unroll
                for (int mt = 0; mt < 4; mt++) {
                    const uint32_t w[8] = {cur[mt][0].x, cur[mt][0].y, cur[mt][0].z, cur[mt][0].w,
                                           cur[mt][1].x, cur[mt][1].y, cur[mt][1].z, cur[mt][1].w};
                    uint32_t o[8];
                    pq32_window(w, (32u - ((16u * mt + col) & 31u)) & 31u, o);
                    cur[mt][0] = u32x4{o[0], o[1], o[2], o[3]};
                    cur[mt][1] = u32x4{o[4], o[5], o[6], o[7]};
                }
            }
            f32x4 acc[4][NT];
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
#pragma unroll
                for (int nt = 0; nt < NT; nt++) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < PQM_NCH; c++) {
#pragma unroll
                for (int j = 0; j < KPC; j++) {
                    const uint32_t kb = (uint32_t)(KPC * c + j);
                    if (kb >= KB) break;  // (dim % 32 == 0: whole K blocks; the codes past m are never read)
                    bf16x8 b[NT];
#pragma unroll
                    for (int nt = 0; nt < NT; nt++) b[nt] = bl[(kb * NT + nt) * 64 + lane];
#pragma unroll
                    for (int mt = 0; mt < 4; mt++) {
                        const u32x4 cw = cur[mt][c];
                        bf16x8 af;
                        if constexpr (DSUB == 4) {
                            // segments 16 c + 8 j + 2 g, + 1: the chunk's bytes 8 j + 2 g, + 1
                            const uint64_t half = j ? ((uint64_t)cw.w << 32) | cw.z : ((uint64_t)cw.y << 32) | cw.x;
                            const uint32_t hw = (uint32_t)(half >> (16u * g)) & 0xFFFFu;
                            const uint32_t seg = 16u * c + 8u * j + 2u * g;
                            const uint32_t c0 = min(hw & 0xFFu, ks - 1), c1 = min(hw >> 8, ks - 1);
                            u32x2 lo = *reinterpret_cast<const u32x2 *>(smem + ((size_t)seg * ks + c0) * 8);
                            u32x2 hi = *reinterpret_cast<const u32x2 *>(smem + ((size_t)(seg + 1) * ks + c1) * 8);
                            const u32x4 v = {lo.x, lo.y, hi.x, hi.y};
                            af = *reinterpret_cast<const bf16x8 *>(&v);
                        } else {
                            // segment 16 c + 4 j + g: the chunk's byte 4 j + g
                            const uint32_t wj = j == 0 ? cw.x : (j == 1 ? cw.y : (j == 2 ? cw.z : cw.w));
                            const uint32_t seg = 16u * c + 4u * j + g;
                            const uint32_t c0 = min((wj >> (8u * g)) & 0xFFu, ks - 1);
                            af = *reinterpret_cast<const bf16x8 *>(smem + ((size_t)seg * ks + c0) * 16);
                        }
#pragma unroll
                        for (int nt = 0; nt < NT; nt++)
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b[nt], acc[mt][nt], 0, 0, 0);
                    }
                }
            }
            // epilogue: element i of acc[mt][nt] is row 16 mt + 4 g + i against query 16 nt + col;
            // u = (s - h) + E1, one compare against sigma_q (NaN: never below it)
            f32x4 hx[4];
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                    hx[mt][i] = nv[mt][i] <= 0x1p60f ? (nv[mt][i] * nv[mt][i]) * a.hg : __builtin_nanf("");
            float k1r[NT], k2r[NT], sgr[NT];
            bool any = false;
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                k1r[nt] = ck1[16 * nt + col];
                k2r[nt] = ck2[16 * nt + col];
                sgr[nt] = sig[16 * nt + col];
#pragma unroll
                for (int mt = 0; mt < 4; mt++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const float u = (acc[mt][nt][i] - hx[mt][i]) + __builtin_fmaf(nv[mt][i], k1r[nt], k2r[nt]);
                        any |= !(u < sgr[nt]);
                    }
            }
            if (__ballot(any) != 0ull) {
#pragma unroll
                for (int nt = 0; nt < NT; nt++) {
                    const uint32_t ql = 16u * nt + col;
                    if (q0 + ql >= a.nq) continue;
#pragma unroll
                    for (int mt = 0; mt < 4; mt++) {
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const float u = (acc[mt][nt][i] - hx[mt][i]) + __builtin_fmaf(nv[mt][i], k1r[nt], k2r[nt]);
                            const uint32_t row = 16u * mt + 4u * g + (uint32_t)i;
                            if (!(u < sgr[nt]) && ((mask >> row) & 1ull)) {
                                const float lower = sc_lower_l2(u, ccq[ql]);
                                if (!(lower > tadm[ql])) {
                                    const uint32_t pos = atomicAdd(&cnt[ql], 1u);
                                    if (pos < P)
                                        a.pools[((size_t)(q0 + ql) * a.ranges + rng) * P + pos] =
                                            ((uint64_t)wvg_ord_f32(lower) << 32) | (uint32_t)(T * 64 + row);
                                    if (pos + 256 >= P) flag[par] = 1u;
                                }
                            }
                        }
                    }
                }
            }
        } else {
            have = false;
        }
        __syncthreads();
        if (flag[par] != 0u) compact(false, par);  // the same word for every wave: all compact or none
    }
    compact(true, 0);
}

// ---- K8m-S: codebooks beyond LDS (option batch_screen = 7; DESIGN section 5, "K8m-S") ---------------------
// The image and the query fragments pass through LDS in K slices of 64 dimensions (two K blocks): a slice's
// image is ks * 128 contiguous bytes of [segment][code][dsub], its fragments 8 KiB of [nqb][dim / 32][NT][64],
// and two slices are resident (slice s + 1 arrives by global_load_lds under the MFMAs of slice s; one
// barrier per slice).  A workgroup takes its range in blocks of 8 tiles (512 rows); wave w owns tiles
// 2 w, 2 w + 1 of the block and carries their 2 x 4 x 4 f32x4 accumulators (128 AGPRs) through every slice.
// (Four tiles per wave, 256 accumulator registers, did not compile without a private segment: DESIGN.)  The
// code chunk of a slice (dsub 4: one chunk per slice; dsub 8: one per two slices) is loaded into registers one
// chunk ahead; a block's first chunk -- both chunks of rotated rows (m = 32, un-rotated at the head of the
// block) -- arrives in LDS under the previous block's last chunk, so nothing stays in registers across the
// epilogue.  The block's row norms are staged into LDS during slice 0.
//
// The bound.  Each accumulator is the C operand of its row tile's MFMAs in slice order, K block by K block:
// the same fp32 chain over the d products as K8m's single K loop, nothing summed in another order and K never
// split across waves.  So (b) above PqmArgs (K1q / K2q at d) holds as written, and with pq_mfma_alpha(m, dsub)
// -- general in m -- so do (a), (c) and the three obligations.  PqmArgs serves both kernels: `ranges` are
// K8m-S's block ranges here, every other field means what it means to K8m.
//
// The pools' step rule (a query's pool gains at most 256 keys between two compaction checks) is kept by
// running the epilogue tile by tile: one tile per wave (256 rows per workgroup), then the barrier and the
// flag check, twice per block.
constexpr int PQS_TPW = 2;                                // tiles per wave and block
constexpr int PQS_TB = PQM_WAVES * PQS_TPW;               // tiles per block
constexpr uint32_t PQS_IMG = 32u << 10;                   // a slice's image at ks = 256
constexpr uint32_t PQS_BUF = PQS_IMG + (8u << 10);        // + its 64 queries' fragments
constexpr uint32_t PQS_NORMS = 2 * PQS_BUF;               // the block's row norms
constexpr uint32_t PQS_CODES = PQS_NORMS + PQS_TB * 64 * 4;  // the block's first chunk (rotated rows: both)
constexpr uint32_t PQS_TAIL = PQS_CODES + 2 * PQS_TB * 64 * 16;  // K8m's tail (PQM_TAIL)
constexpr uint32_t PQS_LDS = PQS_TAIL + PQM_TAIL;
constexpr uint32_t PQS_MAX_DIM = 2048;  // the largest dim taken: K1q's constant and alpha are checked up to it

template <int DSUB, bool ROT>
__global__ __launch_bounds__(PQM_WAVES * 64) void pqs_screen_kernel(PqmArgs a)
{
    constexpr int NT = PQM_NT, QB = PQM_QB, TPW = PQS_TPW;
    constexpr int SPC = DSUB == 4 ? 1 : 2;  // slices per 16-code chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *lnorm = reinterpret_cast<float *>(smem + PQS_NORMS);
    uint4 *lcodes = reinterpret_cast<uint4 *>(smem + PQS_CODES);
    float *ck1 = reinterpret_cast<float *>(smem + PQS_TAIL);  // [64] each, as in K8m
    float *ck2 = ck1 + QB, *ccq = ck2 + QB, *cem = ccq + QB;
    float *sig = cem + QB, *tadm = sig + QB, *wtau = tadm + QB;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(wtau + QB), *wdrop = cnt + QB, *flag = wdrop + QB;  // flag[2] by tile parity

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint32_t rng, qb;  // K8m's block order
    if (a.ranges % 8u == 0) {
        const uint32_t kk = blockIdx.x >> 3;
        rng = (kk / a.nqb) * 8u + (blockIdx.x & 7u);
        qb = kk % a.nqb;
    } else {
        rng = blockIdx.x / a.nqb;
        qb = blockIdx.x % a.nqb;
    }
    const uint32_t q0 = qb * QB, P = a.P, K = a.k, ks = a.ks, nch = a.nch;
    const uint32_t S = a.dim / 64, slice_img = ks * 128u, nu_img = (slice_img + 1023u) / 1024u;
    const uint32_t col = lane & 15u, g = lane >> 4;
    const uint4 *gimg = a.image + lane;
    const uint4 *gfr = a.qfrag + (size_t)qb * (a.dim / 32) * NT * 64 + lane;
    // slice s into buffer s & 1, in 1 KiB units dealt over the waves (a unit = one wave-wide 16-byte load)
    auto stage = [&](uint32_t s) {
        unsigned char *dst = smem + (s & 1u) * PQS_BUF;
        for (uint32_t u = wave; u < nu_img + 8u; u += PQM_WAVES) {
            if (u < nu_img) {
                if (u * 1024u + lane * 16u < slice_img)  // (ks % 8 != 0: the last unit is partial)
                    __builtin_amdgcn_global_load_lds(gimg + ((size_t)s * slice_img + u * 1024u) / 16,
                                                     reinterpret_cast<uint4 *>(dst + u * 1024u), 16, 0, 0);
            } else {
                const uint32_t v = u - nu_img;
                __builtin_amdgcn_global_load_lds(gfr + ((size_t)s * 8 + v) * 64,
                                                 reinterpret_cast<uint4 *>(dst + PQS_IMG + v * 1024u), 16, 0, 0);
            }
        }
    };
    const uint64_t nblk = (a.tile_end - a.tile_begin + PQS_TB - 1) / PQS_TB;
    const uint64_t b0 = nblk * rng / a.ranges, b1 = nblk * (rng + 1) / a.ranges;
    // chunk 0 (rotated rows: chunks 0 and 1) of the wave's tiles of block blk, a row per lane; each wave
    // reads back only what it loaded.  (A tile past the end reads the range's last tile instead: its mask is 0
    // and nothing of it is kept.)
    auto stage_codes = [&](uint64_t blk) {
#pragma unroll
        for (int t = 0; t < TPW; t++) {
            const uint64_t T = min(a.tile_begin + PQS_TB * blk + TPW * wave + t, a.tile_end - 1);
#pragma unroll
            for (int c = 0; c < (ROT ? 2 : 1); c++)
                __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint4 *>(a.data) + ((size_t)T * nch + c) * 64 + lane,
                                                 lcodes + (PQS_TB * c + TPW * wave + t) * 64, 16, 0, 0);
        }
    };
    if (b0 < b1) {
        stage(0);
        stage_codes(b0);
    }
    if (tid < (uint32_t)QB) {
        const bool live = q0 + tid < a.nq;  // a padding query admits nothing
        ck1[tid] = a.k1[q0 + tid];
        ck2[tid] = a.k2[q0 + tid];
        ccq[tid] = a.cq[q0 + tid];
        cem[tid] = a.emax[q0 + tid];
        sig[tid] = live ? -__builtin_inff() : __builtin_inff();
        tadm[tid] = live ? __builtin_inff() : -__builtin_inff();
        wtau[tid] = __builtin_inff();
        cnt[tid] = 0;
        wdrop[tid] = 0xFFFFFFFFu;
    }
    if (tid < 2) flag[tid] = 0;
    __syncthreads();

    // K8m's compaction, word for word
    auto compact = [&](bool last, uint32_t par) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the pools' stores
        __threadfence_block();
        __syncthreads();
        if (tid == 0) flag[par] = 0;
        for (uint32_t ql = wave; ql < (uint32_t)QB; ql += PQM_WAVES) {
            const uint32_t q = q0 + ql;
            if (q >= a.nq) break;
            const uint32_t raw = cnt[ql];
            if (!last && raw <= P - 256) continue;
            float t = wtau[ql];
            uint32_t kept = 0;
            if (raw > 0) {
                const uint64_t r = sc_compact(a.pools + ((size_t)q * a.ranges + rng) * P, min(raw, P), K, P - 256,
                                              cem[ql], 0, t, (lds_u32 *)(wdrop + ql));
                kept = (uint32_t)(r >> 32) & 0x7FFFFFFFu;
                t = __uint_as_float((uint32_t)r);
            }
            if (lane == 0) {
                if (raw > P) wdrop[ql] = 0;  // keys lost past the pool (never, by the step rule): always flagged
                const uint32_t dr = wdrop[ql];
                const float wt = dr == 0xFFFFFFFFu ? t : fminf(t, wvg_unord_f32(dr));
                cnt[ql] = kept;
                wtau[ql] = t;
                tadm[ql] = wt;
                sig[ql] = sc_sigma_l2(wt, ccq[ql]);
                if (last) {
                    a.pcnt[(size_t)q * a.ranges + rng] = kept;
                    a.pdrop[(size_t)q * a.ranges + rng] = dr;
                    if (t < __builtin_inff()) atomicMin(a.gbound + q, wvg_ord_f32(t));
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the packed pools
        __threadfence_block();
        __syncthreads();
    };

    // chunk c of rows 16 mt + col of the wave's tiles of block blk
    auto load_chunk = [&](uint64_t blk, uint32_t c, u32x4 (&dst)[TPW][4]) {
#pragma unroll
        for (int t = 0; t < TPW; t++) {
            const uint64_t T = min(a.tile_begin + PQS_TB * blk + TPW * wave + t, a.tile_end - 1);
            const u32x4 *p = a.data + ((size_t)T * nch + c) * 64 + col;
#pragma unroll
            for (int mt = 0; mt < 4; mt++) dst[t][mt] = p[16 * mt];
        }
    };
    for (uint64_t blk = b0; blk < b1; ++blk) {
        const uint64_t T0 = a.tile_begin + PQS_TB * blk + TPW * wave;
        uint64_t mask[TPW];
#pragma unroll
        for (int t = 0; t < TPW; t++) mask[t] = T0 + t < a.tile_end ? pqm_tile_mask(a, T0 + t) : 0ull;  // wave-uniform
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // slice 0 and the first chunk (this wave's own loads)
        u32x4 cur[TPW][4], hi[TPW][4] = {};
#pragma unroll
        for (int t = 0; t < TPW; t++)
#pragma unroll
            for (int mt = 0; mt < 4; mt++) {
                const uint4 x = lcodes[(TPW * wave + t) * 64 + 16 * mt + col];
                cur[t][mt] = u32x4{x.x, x.y, x.z, x.w};
                if constexpr (ROT) {
                    const uint4 y = lcodes[(PQS_TB + TPW * wave + t) * 64 + 16 * mt + col];
                    hi[t][mt] = u32x4{y.x, y.y, y.z, y.w};
                }
            }
        if constexpr (ROT) {  // m = 32: back to segment order (stored byte b = code[(b + slot) mod 32])
#pragma unroll
            for (int t = 0; t < TPW; t++)
#pragma unroll
                for (int mt = 0; mt < 4; mt++) {
                    const uint32_t w[8] = {cur[t][mt].x, cur[t][mt].y, cur[t][mt].z, cur[t][mt].w,
                                           hi[t][mt].x, hi[t][mt].y, hi[t][mt].z, hi[t][mt].w};
                    uint32_t o[8];
                    pq32_window(w, (32u - ((16u * mt + col) & 31u)) & 31u, o);
                    cur[t][mt] = u32x4{o[0], o[1], o[2], o[3]};
                    hi[t][mt] = u32x4{o[4], o[5], o[6], o[7]};
                }
        }
        f32x4 acc[TPW][4][NT];
#pragma unroll
        for (int t = 0; t < TPW; t++)
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
#pragma unroll
                for (int nt = 0; nt < NT; nt++) acc[t][mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();  // slice 0 is whole
        for (uint32_t c = 0; c < nch; c++) {
            u32x4 nxt[TPW][4] = {};
            if (c + 1 == nch && blk + 1 < b1) stage_codes(blk + 1);  // (read back after this block's epilogue)
            if constexpr (ROT) {
#pragma unroll
                for (int t = 0; t < TPW; t++)
#pragma unroll
                    for (int mt = 0; mt < 4; mt++) nxt[t][mt] = hi[t][mt];
            } else if (c + 1 < nch) {
                load_chunk(blk, c + 1, nxt);  // under this chunk's MFMAs
            }
#pragma unroll
            for (int h = 0; h < SPC; h++) {
                const uint32_t s = SPC * c + h;
                if (s >= S) break;  // (a half-filled last chunk at dsub = 8)
                if (s + 1 < S) stage(s + 1);
                if (s == 0) {  // every wave is past the previous block's epilogue: the norms of this one
#pragma unroll
                    for (int t = 0; t < TPW; t++)
                        if (T0 + t < a.tile_end)
                            __builtin_amdgcn_global_load_lds(a.norms + (T0 + t - a.tile_begin) * 64 + lane,
                                                             lnorm + (TPW * wave + t) * 64, 4, 0, 0);
                }
                const unsigned char *ib = smem + (s & 1u) * PQS_BUF;
                const bf16x8 *bl = reinterpret_cast<const bf16x8 *>(ib + PQS_IMG);
#pragma unroll
                for (int kbl = 0; kbl < 2; kbl++) {
                    bf16x8 b[NT];
#pragma unroll
                    for (int nt = 0; nt < NT; nt++) b[nt] = bl[(kbl * NT + nt) * 64 + lane];
#pragma unroll
                    for (int t = 0; t < TPW; t++) {
                        if (mask[t] == 0ull) continue;
                        bf16x8 af[4];
#pragma unroll
                        for (int mt = 0; mt < 4; mt++) {
                            const u32x4 cw = cur[t][mt];
                            if constexpr (DSUB == 4) {
                                // the slice's segments 8 kbl + 2 g, + 1: the chunk's bytes 8 kbl + 2 g, + 1
                                const uint64_t half = kbl ? ((uint64_t)cw.w << 32) | cw.z : ((uint64_t)cw.y << 32) | cw.x;
                                const uint32_t hw = (uint32_t)(half >> (16u * g)) & 0xFFFFu;
                                const uint32_t seg = 8u * kbl + 2u * g;
                                const uint32_t c0 = min(hw & 0xFFu, ks - 1), c1 = min(hw >> 8, ks - 1);
                                u32x2 lo = *reinterpret_cast<const u32x2 *>(ib + ((size_t)seg * ks + c0) * 8);
                                u32x2 hi = *reinterpret_cast<const u32x2 *>(ib + ((size_t)(seg + 1) * ks + c1) * 8);
                                const u32x4 v = {lo.x, lo.y, hi.x, hi.y};
                                af[mt] = *reinterpret_cast<const bf16x8 *>(&v);
                            } else {
                                // the slice's segment 4 kbl + g: the chunk's byte 8 h + 4 kbl + g
                                const uint32_t wj = h == 0 ? (kbl == 0 ? cw.x : cw.y) : (kbl == 0 ? cw.z : cw.w);
                                const uint32_t seg = 4u * kbl + g;
                                const uint32_t c0 = min((wj >> (8u * g)) & 0xFFu, ks - 1);
                                af[mt] = *reinterpret_cast<const bf16x8 *>(ib + ((size_t)seg * ks + c0) * 16);
                            }
                        }
#pragma unroll
                        for (int mt = 0; mt < 4; mt++)
#pragma unroll
                            for (int nt = 0; nt < NT; nt++)
                                acc[t][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mt], b[nt], acc[t][mt][nt], 0, 0, 0);
                    }
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // slice s + 1, the norms, the next chunk
                __syncthreads();                                   // and buffer s & 1 is free
            }
#pragma unroll
            for (int t = 0; t < TPW; t++)
#pragma unroll
                for (int mt = 0; mt < 4; mt++) cur[t][mt] = nxt[t][mt];
        }
        if (blk + 1 < b1) stage(0);  // the next block's first slice under this block's epilogue
        // K8m's epilogue, a tile at a time: element i of acc[t][mt][nt] is row 16 mt + 4 g + i of tile T0 + t
        // against query 16 nt + col
#pragma unroll
        for (uint32_t t = 0; t < (uint32_t)TPW; t++) {
            const uint32_t par = t & 1u;
            const uint64_t m_t = mask[t];
            if (m_t != 0ull) {
                // tile t's accumulators against query tile nt (t is wave-uniform)
                auto take = [&](int nt, f32x4 (&e)[4]) {
#pragma unroll
                    for (int mt = 0; mt < 4; mt++) e[mt] = acc[t][mt][nt];
                };
                f32x4 nv[4], hx[4];
#pragma unroll
                for (int mt = 0; mt < 4; mt++) {
                    nv[mt] = *reinterpret_cast<const f32x4 *>(lnorm + (TPW * wave + t) * 64 + 16 * mt + 4 * g);
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        hx[mt][i] = nv[mt][i] <= 0x1p60f ? (nv[mt][i] * nv[mt][i]) * a.hg : __builtin_nanf("");
                }
                float k1r[NT], k2r[NT], sgr[NT];
                bool any = false;
#pragma unroll
                for (int nt = 0; nt < NT; nt++) {
                    k1r[nt] = ck1[16 * nt + col];
                    k2r[nt] = ck2[16 * nt + col];
                    sgr[nt] = sig[16 * nt + col];
                    f32x4 e[4];
                    take(nt, e);
#pragma unroll
                    for (int mt = 0; mt < 4; mt++)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const float u = (e[mt][i] - hx[mt][i]) + __builtin_fmaf(nv[mt][i], k1r[nt], k2r[nt]);
                            any |= !(u < sgr[nt]);
                        }
                }
                if (__ballot(any) != 0ull) {
#pragma unroll
                    for (int nt = 0; nt < NT; nt++) {
                        const uint32_t ql = 16u * nt + col;
                        if (q0 + ql >= a.nq) continue;
                        f32x4 e[4];
                        take(nt, e);
#pragma unroll
                        for (int mt = 0; mt < 4; mt++) {
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                const float u =
                                    (e[mt][i] - hx[mt][i]) + __builtin_fmaf(nv[mt][i], k1r[nt], k2r[nt]);
                                const uint32_t row = 16u * mt + 4u * g + (uint32_t)i;
                                if (!(u < sgr[nt]) && ((m_t >> row) & 1ull)) {
                                    const float lower = sc_lower_l2(u, ccq[ql]);
                                    if (!(lower > tadm[ql])) {
                                        const uint32_t pos = atomicAdd(&cnt[ql], 1u);
                                        if (pos < P)
                                            a.pools[((size_t)(q0 + ql) * a.ranges + rng) * P + pos] =
                                                ((uint64_t)wvg_ord_f32(lower) << 32) | (uint32_t)((T0 + t) * 64 + row);
                                        if (pos + 256 >= P) flag[par] = 1u;
                                    }
                                }
                            }
                        }
                    }
                }
            }
            __syncthreads();
            if (flag[par] != 0u) compact(false, par);  // the same word for every wave: all compact or none
        }
    }
    compact(true, 0);
}

// The exact rescore, in place: every kept (query, slot) gets K8's sum -- the call's LUT entries of
// the row's codes added in segment order (pq_row_sum) -- as its key.
__global__ __launch_bounds__(256) void pqm_rescore_keys_kernel(const uint4 *data, uint32_t nch, uint32_t m, uint32_t ks,
                                                               const float *luts, uint64_t *keys, uint32_t ncand,
                                                               uint64_t total)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const uint64_t key = keys[i];
    if (key == WVG_KEY_NONE) return;
    const uint32_t slot = (uint32_t)key;
    const float *lut = luts + (i / ncand) * (size_t)m * ks;
    const float sum = pq_row_sum(data + (size_t)(slot >> 6) * nch * 64 + (slot & 63), nch, m, ks, lut, slot);
    keys[i] = wvg_make_key(sum, slot);  // (l2-squared: Wrap is the identity)
}

// ---- host side ---------------------------------------------------------------------------------------------
bool pq_mfma_supported(uint32_t dim, uint32_t m, uint32_t ks, uint32_t k)
{
    if (dim == 0 || m == 0 || ks == 0 || ks > 256 || k == 0 || k > 256 || dim % 32 != 0 || dim % m != 0) return false;
    const uint32_t dsub = dim / m;
    if ((dsub != 4 && dsub != 8) || m > 16 * PQM_NCH) return false;
    return (size_t)dim * ks * 2 + (size_t)dim * 2 * PQM_QB + PQM_TAIL <= WVG_LDS_BYTES;
}

// K8m-S takes what K8m refuses for its image size or segment count: whole 64-dimension slices, any m.
bool pq_mfma_slice_supported(uint32_t dim, uint32_t m, uint32_t ks, uint32_t k)
{
    if (dim == 0 || m == 0 || ks == 0 || ks > 256 || k == 0 || k > 256 || dim % 64 != 0 || dim % m != 0 ||
        dim > PQS_MAX_DIM)
        return false;
    const uint32_t dsub = dim / m;
    return (dsub == 4 || dsub == 8) && !pq_mfma_supported(dim, m, ks, k);
}

static uint32_t pqm_pool(uint32_t k) { return screen_wide_pool(k); }

uint32_t pq_mfma_ranges(uint32_t nq, uint32_t k, uint64_t ntiles, int num_cus)
{
    const uint32_t nqb = (nq + PQM_QB - 1) / PQM_QB;
    const uint64_t nsteps = (ntiles + 3) / 4;
    // one workgroup per CU; a range of at least 8 steps (2048 rows), as K5m's
    uint64_t r = std::max<uint64_t>(1, (uint64_t)num_cus / nqb);
    r = std::min(r, std::max<uint64_t>(1, nsteps / 8));
    // the pools of all workgroups within 256 MiB
    const uint64_t per_range = (uint64_t)nqb * PQM_QB * pqm_pool(k) * 8;
    r = std::min<uint64_t>(r, (256ull << 20) / per_range);
    if (r >= 8) r -= r % 8;  // whole rounds over the 8 XCDs: the co-scheduled block order
    return (uint32_t)r;      // 0: the batch's pools do not fit (the caller keeps its route)
}

uint32_t pq_mfma_slice_ranges(uint32_t nq, uint32_t k, uint64_t ntiles, int num_cus)
{
    const uint32_t nqb = (nq + PQM_QB - 1) / PQM_QB;
    const uint64_t nblk = (ntiles + PQS_TB - 1) / PQS_TB;
    // one workgroup per CU; a range of at least 4 blocks (2048 rows, as K8m's)
    uint64_t r = std::max<uint64_t>(1, (uint64_t)num_cus / nqb);
    r = std::min(r, std::max<uint64_t>(1, nblk / 4));
    // the pools of all workgroups within 256 MiB, as pq_mfma_ranges
    const uint64_t per_range = (uint64_t)nqb * PQM_QB * pqm_pool(k) * 8;
    r = std::min<uint64_t>(r, (256ull << 20) / per_range);
    if (r >= 8) r -= r % 8;
    return (uint32_t)r;
}

PqMfmaWs pq_mfma_ws(uint32_t nq, uint32_t k, uint32_t dim, uint32_t m, uint32_t ks, uint32_t ranges, uint64_t ntiles)
{
    const size_t nq_pad = (size_t)(nq + PQM_QB - 1) / PQM_QB * PQM_QB;
    PqMfmaWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off = (off + bytes + 255) / 256 * 256;
        return at;
    };
    w.pools = take((size_t)nq * ranges * pqm_pool(k) * 8);
    w.norms = take((size_t)ntiles * 64 * 4);
    w.image = take((size_t)dim * ks * 2);
    w.sq = take((size_t)m * ks * 8);
    w.qfrag = take(nq_pad * dim * 2);
    w.k1 = take(nq_pad * 4);
    w.k2 = take(nq_pad * 4);
    w.em = take(nq_pad * 4);
    w.cq = take(nq_pad * 4);
    w.gb = take((size_t)nq * 4);
    w.nmax = take(4);
    w.pcnt = take((size_t)nq * ranges * 4);
    w.pdrop = take((size_t)nq * ranges * 4);
    w.fl = take((size_t)nq * 4);
    w.nf = take(4);
    w.fbp = take((size_t)nq * PQM_FB_GROUPS * k * 8);
    w.total = off;
    return w;
}

// The screen's dynamic LDS is above the default limit: raised once per process, outside any launch (so a
// first call that is being captured only launches).
void pq_mfma_prepare()
{
    static const bool attr =
        hipFuncSetAttribute(reinterpret_cast<const void *>(&pqm_screen_kernel<4>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)WVG_LDS_BYTES) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&pqm_screen_kernel<8>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)WVG_LDS_BYTES) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&pqs_screen_kernel<4, false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)PQS_LDS) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&pqs_screen_kernel<8, false>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)PQS_LDS) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&pqs_screen_kernel<8, true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)PQS_LDS) == hipSuccess;
    (void)attr;
}

hipError_t launch_pq_mfma(const PqMfmaLaunch &L, uint64_t *ids, float *dists, uint32_t *counts, hipStream_t s)
{
    const ScanArgs &sa = L.scan;
    const uint32_t nq = sa.nq, k = sa.k, m = sa.pq_m, ks = sa.pq_ks;
    const bool slice = pq_mfma_slice_supported(L.dim, m, ks, k);  // (never where K8m applies)
    if (!(slice || pq_mfma_supported(L.dim, m, ks, k)) || L.ranges == 0 || nq == 0 || sa.tile_end <= sa.tile_begin ||
        sa.nchunks != pq_chunks(m) || sa.metric != WVG_M_L2)
        return hipErrorInvalidValue;
    const uint32_t dsub = L.dim / m, nqb = (nq + PQM_QB - 1) / PQM_QB, nq_pad = nqb * PQM_QB, P = pqm_pool(k);
    const uint64_t ntiles = sa.tile_end - sa.tile_begin;
    const uint32_t lds = L.dim * ks * 2 + L.dim * 2 * PQM_QB + PQM_TAIL;
    const PqMfmaWs w = pq_mfma_ws(nq, k, L.dim, m, ks, L.ranges, ntiles);
    const double alpha = pq_mfma_alpha(m, dsub);
    PqmArgs a{};
    a.data = reinterpret_cast<const u32x4 *>(sa.data);
    a.valid = sa.valid;
    a.allow = sa.allow;
    a.allow_words = sa.allow_words;
    a.allow_t0 = sa.allow_t0;
    a.tile_begin = sa.tile_begin;
    a.tile_end = sa.tile_end;
    a.nch = sa.nchunks;
    a.m = m;
    a.ks = ks;
    a.dim = L.dim;
    a.rot = pq_rotated(m) ? 1u : 0u;
    a.nq = nq;
    a.k = k;
    a.ranges = L.ranges;
    a.nqb = nqb;
    a.P = P;
    a.hg = screen_l2_hg_alpha(alpha);
    a.image = reinterpret_cast<const uint4 *>(L.ws + w.image);
    a.qfrag = reinterpret_cast<const uint4 *>(L.ws + w.qfrag);
    a.norms = reinterpret_cast<const float *>(L.ws + w.norms);
    a.k1 = reinterpret_cast<const float *>(L.ws + w.k1);
    a.k2 = reinterpret_cast<const float *>(L.ws + w.k2);
    a.cq = reinterpret_cast<const float *>(L.ws + w.cq);
    a.emax = reinterpret_cast<const float *>(L.ws + w.em);
    a.pools = reinterpret_cast<uint64_t *>(L.ws + w.pools);
    a.pcnt = reinterpret_cast<uint32_t *>(L.ws + w.pcnt);
    a.pdrop = reinterpret_cast<uint32_t *>(L.ws + w.pdrop);
    a.gbound = reinterpret_cast<uint32_t *>(L.ws + w.gb);
    uint32_t *nmax = reinterpret_cast<uint32_t *>(L.ws + w.nmax), *nflag = reinterpret_cast<uint32_t *>(L.ws + w.nf);
    uint32_t *flist = reinterpret_cast<uint32_t *>(L.ws + w.fl);
    double *sq = reinterpret_cast<double *>(L.ws + w.sq);
    hipLaunchKernelGGL(pqm_prep_kernel, dim3((std::max(m * ks, nq) + 255) / 256), dim3(256), 0, s, L.centers, m * ks, dsub,
                       reinterpret_cast<__bf16 *>(L.ws + w.image), sq, a.gbound, nq, nmax, nflag);
    hipLaunchKernelGGL(pqm_norms_kernel, dim3((unsigned)((ntiles * 64 + 255) / 256)), dim3(256), 0, s, a.data, a.nch, m, ks,
                       a.rot, sq, a.valid, a.tile_begin, ntiles * 64, reinterpret_cast<float *>(L.ws + w.norms), nmax);
    hipLaunchKernelGGL(pqm_qconst_kernel, dim3(nq_pad / 4), dim3(256), 0, s, L.queries, nq, L.qpitch, L.dim, nq_pad, alpha,
                       nmax, reinterpret_cast<uint4 *>(L.ws + w.qfrag), reinterpret_cast<float *>(L.ws + w.k1),
                       reinterpret_cast<float *>(L.ws + w.k2), reinterpret_cast<float *>(L.ws + w.em),
                       reinterpret_cast<float *>(L.ws + w.cq));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    pq_mfma_prepare();
    // (rotated rows, m = 32, reach K8m-S at dsub = 8 only: at dsub = 4 their image is K8m's)
    if (slice && a.rot) launch_timed((pqs_screen_kernel<8, true>), dim3(a.ranges * a.nqb), dim3(PQM_WAVES * 64), PQS_LDS, s, a);
    else if (slice && dsub == 4) launch_timed((pqs_screen_kernel<4, false>), dim3(a.ranges * a.nqb), dim3(PQM_WAVES * 64), PQS_LDS, s, a);
    else if (slice) launch_timed((pqs_screen_kernel<8, false>), dim3(a.ranges * a.nqb), dim3(PQM_WAVES * 64), PQS_LDS, s, a);
    else if (dsub == 4) launch_timed((pqm_screen_kernel<4>), dim3(a.ranges * a.nqb), dim3(PQM_WAVES * 64), lds, s, a);
    else launch_timed((pqm_screen_kernel<8>), dim3(a.ranges * a.nqb), dim3(PQM_WAVES * 64), lds, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = launch_collect_pools(a.pools, a.pcnt, a.pdrop, nq, L.ranges, P, k, a.emax, flist, nflag, a.gbound, s);
    if (e != hipSuccess) return e;
    const uint32_t ncand = L.ranges * P;
    const uint64_t total = (uint64_t)nq * ncand;
    hipLaunchKernelGGL(pqm_rescore_keys_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const uint4 *>(sa.data), a.nch, m, ks, reinterpret_cast<const float *>(sa.queries),
                       a.pools, ncand, total);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = launch_merge_keys(a.pools, nq, ncand, k, sa.id_base, ids, dists, counts, s);
    if (e != hipSuccess) return e;
    // the flagged queries: K8's sums over the whole range, their results replace the screened ones
    ScanArgs f = sa;
    f.nq = 1;
    f.cosched = 0;
    f.reverse = 0;
    uint64_t *fbp = reinterpret_cast<uint64_t *>(L.ws + w.fbp);
    e = launch_scan_pq_qlist(f, fbp, (int)PQM_FB_GROUPS, flist, nflag, std::min<uint32_t>(nq, 8), s);
    if (e != hipSuccess) return e;
    return launch_merge_lists_qlist(fbp, nq, PQM_FB_GROUPS, k, k, sa.id_base, ids, dists, counts, flist, nflag, s);
}

}  // namespace wvg

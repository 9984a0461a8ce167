// wvg_bq_mfma.hip -- K5m: batched BQ Hamming search on the int8 matrix cores
// (option batch_screen = 5; DESIGN section 5, "K5m").
//
// Hamming distance as a dot product: for a row bit a in {0, 1} and a query bit
// b, with s = +1 where b = 0 and s = -1 where b = 1,
//     hamming(a, b) = sum a * s + popcount(b).
// v_mfma_i32_16x16x64_i8 computes sum a * s exactly in int32, so the
// accumulator plus the query's popcount IS the distance: no shadow, no error
// bound, no rescore.  Keys are K5's ((ordered float distance) << 32 | slot),
// exact and totally ordered.
//
// Layout.  Rows stay in the corpus's tiles ([tile][chunk][row] x 16 B) and
// never pass through LDS: for the 16-row MFMA tile m of a 64-row tile, lane
// (r = lane % 16, g = lane / 16) loads the 16-byte chunk 4 c' + g of row
// 16 m + r (four 256-byte segments per wave load) and expands its four dwords
// w into the eight A fragments (w >> t) & 0x01010101, t = 0 .. 7: byte j of
// dword i of fragment t is bit 32 i + 8 j + t of the chunk.  The prologue
// (bqm_image_kernel) writes the queries' +-1 bytes with the same bit-to-byte
// mapping in B-fragment order, [query block][c'][t][query tile][lane] x 16 B,
// and every workgroup stages its query block's image into LDS once.  Chunks
// past the row's last (nchunks % 4 != 0) are zero A fragments; padding bits are
// 0 in the rows, so whatever the image holds there adds nothing.
//
// Work split.  Grid = row ranges x query blocks, one 4-wave workgroup per CU
// (the image fills LDS).  A step is 256 rows: wave w scores tile 4 step + w
// against the whole query block, MT = 4 row tiles x NT = QB / 16 query tiles
// of int32 accumulators.  Survivors (accumulator <= the lane's per-column
// threshold, live in the validity / allow word, key below the query's bound
// key) claim a position in the (workgroup, query) pool with one LDS atomic and
// store their key; a pool that passes P - 256 at a step boundary is compacted
// by the whole workgroup (block-parity flag words, as K3c-W): the k smallest
// keys stay and the k-th becomes the query's bound key.  The range's last
// compaction writes the kept keys to partials [nq][ranges][k]; the host
// launches the merge.
#include "wvg_internal.hpp"

namespace wvg {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int BQM_WAVES = 4;
constexpr int BQM_KEYS = 768 / 64;  // keys per lane of a compaction: P <= 768
// the bounds, counts, thresholds and the two flag words behind the image
constexpr uint32_t BQM_TAIL = 64 * 8 + 64 * 4 + 64 * 4 + 16;

struct BqmArgs {
    const u32x4 *data;
    const uint64_t *valid, *allow;
    uint64_t allow_words, allow_t0, tile_begin, tile_end;
    uint32_t nchunks, c4;  // 16-byte chunks per row; groups of four chunks
    uint32_t nq, k, ranges, nqb, P;
    const u32x4 *image;    // [nqb][c4][8][NT][64]
    const int32_t *pc;     // [nqb * QB] popcounts (0 for padding queries)
    uint64_t *pools;       // [ranges][nqb * QB][P]
    uint64_t *partials;    // [nq][ranges][k]
};

// The query image and popcounts: one 64-thread block per (query block, c', t, query tile).
__global__ __launch_bounds__(64) void bqm_image_kernel(const uint64_t *codes, uint32_t qpitch, uint32_t words,
                                                       uint32_t nq, uint32_t c4, uint32_t nt, u32x4 *image, int32_t *pc)
{
    const uint32_t lane = threadIdx.x, cq = lane & 15u, g = lane >> 4;
    uint32_t b = blockIdx.x;
    const uint32_t tile = b % nt;
    b /= nt;
    const uint32_t t = b & 7u;
    b >>= 3;
    const uint32_t cp = b % c4, qb = b / c4;
    const uint32_t q = (qb * nt + tile) * 16u + cq;
    u32x4 out = {0u, 0u, 0u, 0u};
    if (q < nq) {
        const uint64_t *src = codes + (size_t)q * qpitch;
        const uint32_t w0 = 2u * (4u * cp + g);
        const uint64_t lo = w0 < words ? src[w0] : 0ull, hi = w0 + 1 < words ? src[w0 + 1] : 0ull;
        const uint32_t dw[4] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
        // a set bit -> the byte 0xFF (-1), a clear one -> 0x01
        out.x = 0x01010101u + ((dw[0] >> t) & 0x01010101u) * 0xFEu;
        out.y = 0x01010101u + ((dw[1] >> t) & 0x01010101u) * 0xFEu;
        out.z = 0x01010101u + ((dw[2] >> t) & 0x01010101u) * 0xFEu;
        out.w = 0x01010101u + ((dw[3] >> t) & 0x01010101u) * 0xFEu;
    }
    image[(size_t)blockIdx.x * 64 + lane] = out;
    if (cp == 0 && t == 0 && g == 0) {
        int32_t n = 0;
        if (q < nq)
            for (uint32_t w = 0; w < words; w++) n += __popcll(codes[(size_t)q * qpitch + w]);
        pc[(qb * nt + tile) * 16u + cq] = n;
    }
}

__device__ __forceinline__ uint64_t bqm_tile_mask(const BqmArgs &a, uint64_t t)
{
    uint64_t m = a.valid[t];
    if (a.allow) {
        const uint64_t w = t - a.allow_t0;
        m &= w < a.allow_words ? a.allow[w] : 0ull;
    }
    return m;
}

template <int NT>
__global__ __launch_bounds__(BQM_WAVES * 64) void scan_bq_mfma_kernel(BqmArgs a)
{
    constexpr int QB = NT * 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t img_vecs = a.c4 * 8u * NT * 64u;
    const u32x4 *img = reinterpret_cast<const u32x4 *>(smem);
    uint64_t *bound = reinterpret_cast<uint64_t *>(smem + (size_t)img_vecs * 16);  // [64] admit only keys below
    uint32_t *cnt = reinterpret_cast<uint32_t *>(bound + 64);                       // [64] the pools' fill counts
    int32_t *thr = reinterpret_cast<int32_t *>(cnt + 64);                           // [64] on the raw accumulator
    uint32_t *flag = reinterpret_cast<uint32_t *>(thr + 64);                        // [2] by step parity

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
    const uint32_t q0 = qb * QB, P = a.P, K = a.k;
    {
        const u32x4 *gi = a.image + (size_t)qb * img_vecs;
        u32x4 *li = reinterpret_cast<u32x4 *>(smem);
        for (uint32_t i = tid; i < img_vecs; i += BQM_WAVES * 64) li[i] = gi[i];
        if (tid < 64) {
            bound[tid] = WVG_KEY_NONE;
            cnt[tid] = 0;
            thr[tid] = q0 + tid < a.nq ? 0x7FFFFFFF : (int32_t)0x80000000;  // a padding query admits nothing
        }
        if (tid < 2) flag[tid] = 0;
    }
    const uint32_t col = lane & 15u, g = lane >> 4;
    int32_t pcr[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) pcr[nt] = a.pc[q0 + 16 * nt + col];
    uint64_t *pools = a.pools + ((size_t)rng * a.nqb + qb) * QB * P;
    __syncthreads();

    // Compaction (workgroup-uniform entry): wave w takes queries w, w + 4, ... whose pool passed P - 256
    // (last: every query; the kept keys are the range's list).
    auto compact = [&](bool last, uint32_t par) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the pools' stores
        __threadfence_block();
        __syncthreads();
        if (tid == 0) flag[par] = 0;
        for (uint32_t ql = wave; ql < (uint32_t)QB; ql += BQM_WAVES) {
            const uint32_t q = q0 + ql;
            if (q >= a.nq) break;
            const uint32_t raw = cnt[ql];
            if (!last && raw <= P - 256) continue;
            const uint32_t n = min(raw, P);
            uint64_t *pool = pools + (size_t)ql * P;
            uint64_t key[BQM_KEYS];
#pragma unroll
            for (int i = 0; i < BQM_KEYS; i++) {
                const uint32_t j = 64u * i + lane;
                key[i] = j < n ? __hip_atomic_load(pool + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : WVG_KEY_NONE;
            }
            uint64_t kth = WVG_KEY_NONE;
            if (n >= K) {  // the K-th smallest key: the largest v with fewer than K keys below it (keys are distinct)
                uint64_t v = 0;
                for (int bit = 63; bit >= 0; bit--) {
                    const uint64_t c = v | (1ull << bit);
                    uint32_t below = 0;
#pragma unroll
                    for (int i = 0; i < BQM_KEYS; i++) below += (uint32_t)__popcll(__ballot(key[i] < c));
                    if (below < K) v = c;
                }
                kth = v;
            }
            uint32_t kept = 0;
#pragma unroll
            for (int i = 0; i < BQM_KEYS; i++) {
                const bool keep = key[i] != WVG_KEY_NONE && key[i] <= kth;
                const uint64_t bal = __ballot(keep);
                const uint32_t at = kept + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                if (keep) {
                    if (last)
                        a.partials[((size_t)q * a.ranges + rng) * K + at] = key[i];
                    else
                        pool[at] = key[i];
                }
                kept += (uint32_t)__popcll(bal);
            }
            if (last) {
                for (uint32_t i = kept + lane; i < K; i += 64) a.partials[((size_t)q * a.ranges + rng) * K + i] = WVG_KEY_NONE;
            } else if (lane == 0) {
                cnt[ql] = kept;
                if (kth != WVG_KEY_NONE) {  // from here on only keys below the k-th are admitted
                    bound[ql] = kth;
                    thr[ql] = (int32_t)wvg_unord_f32((uint32_t)(kth >> 32)) - a.pc[q];
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the packed pools
        __threadfence_block();
        __syncthreads();
    };

    const uint64_t ntiles = a.tile_end - a.tile_begin, nsteps = (ntiles + 3) / 4;
    const uint64_t s0 = nsteps * rng / a.ranges, s1 = nsteps * (rng + 1) / a.ranges;
    const uint32_t nch = a.nchunks, C4 = a.c4;
    // chunk 4 cp + g of rows 16 m + (lane % 16) of tile T, m = 0 .. 3 (zeros past the row's last chunk)
    auto load_rows = [&](uint64_t T, uint32_t cp, u32x4 (&dst)[4]) {
        const uint32_t ch = 4u * cp + g;
        const u32x4 *p = a.data + ((size_t)T * nch + ch) * 64 + col;
#pragma unroll
        for (int m = 0; m < 4; m++) dst[m] = ch < nch ? p[16 * m] : u32x4{0u, 0u, 0u, 0u};
    };
    u32x4 cur[4] = {}, nxt[4] = {};
    bool have = false;  // nxt holds this step's first chunk group (loaded under the previous tile's MFMAs)
    for (uint64_t step = s0; step < s1; ++step) {
        const uint32_t par = (uint32_t)(step & 1ull);
        const uint64_t T = a.tile_begin + 4 * step + wave;
        const uint64_t mask = T < a.tile_end ? bqm_tile_mask(a, T) : 0ull;  // wave-uniform
        if (mask != 0ull) {
            if (have) {
#pragma unroll
                for (int m = 0; m < 4; m++) cur[m] = nxt[m];
            } else {
                load_rows(T, 0, cur);
            }
            i32x4 acc[4][NT];
#pragma unroll
            for (int m = 0; m < 4; m++)
#pragma unroll
                for (int nt = 0; nt < NT; nt++) acc[m][nt] = i32x4{0, 0, 0, 0};
            for (uint32_t cp = 0; cp < C4; cp++) {
                // the next chunk group -- or the next step's first -- under this one's MFMAs
                if (cp + 1 < C4)
                    load_rows(T, cp + 1, nxt);
                else if (step + 1 < s1 && T + 4 < a.tile_end)
                    load_rows(T + 4, 0, nxt);
                const u32x4 *bp = img + (size_t)cp * 8 * NT * 64 + lane;
#pragma unroll
                for (int t = 0; t < 8; t++) {
                    i32x4 b[NT];
#pragma unroll
                    for (int nt = 0; nt < NT; nt++) b[nt] = (i32x4)bp[(t * NT + nt) * 64];
#pragma unroll
                    for (int m = 0; m < 4; m++) {
                        const i32x4 af = (i32x4)((cur[m] >> (uint32_t)t) & 0x01010101u);
#pragma unroll
                        for (int nt = 0; nt < NT; nt++)
                            acc[m][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, b[nt], acc[m][nt], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int m = 0; m < 4; m++) cur[m] = nxt[m];
            }
            have = step + 1 < s1 && T + 4 < a.tile_end;
            // epilogue: element i of acc[m][nt] is row 16 m + 4 g + i against query 16 nt + col
            int32_t th[NT];
            bool any = false;
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                th[nt] = thr[16 * nt + col];
#pragma unroll
                for (int m = 0; m < 4; m++)
                    any |= acc[m][nt].x <= th[nt] || acc[m][nt].y <= th[nt] || acc[m][nt].z <= th[nt] ||
                           acc[m][nt].w <= th[nt];
            }
            if (__ballot(any) != 0ull) {
#pragma unroll
                for (int nt = 0; nt < NT; nt++) {
                    const uint32_t ql = 16u * nt + col;
#pragma unroll
                    for (int m = 0; m < 4; m++) {
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int32_t s = acc[m][nt][i];
                            const uint32_t row = 16u * m + 4u * g + (uint32_t)i;
                            if (s <= th[nt] && ((mask >> row) & 1ull)) {
                                const uint64_t key = wvg_make_key((float)(s + pcr[nt]), (uint32_t)(T * 64 + row));
                                if (key < bound[ql]) {
                                    const uint32_t pos = atomicAdd(&cnt[ql], 1u);
                                    if (pos < P) pools[(size_t)ql * P + pos] = key;
                                    if (pos + 1 > P - 256) flag[par] = 1u;
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

// ---- host side ---------------------------------------------------------------------------------------------
bool bq_mfma_supported(uint32_t dim, uint32_t k) { return dim > 0 && dim <= 4096 && k > 0 && k <= 256; }

uint32_t bq_mfma_qblock(uint32_t dim) { return dim <= 2048 ? 64u : 32u; }

uint32_t bq_mfma_pool(uint32_t k) { return 2 * (k > 64 ? k : 64) + 256; }

uint32_t bq_mfma_ranges(uint32_t nq, uint32_t k, uint32_t dim, uint64_t ntiles, int num_cus)
{
    const uint32_t QB = bq_mfma_qblock(dim), nqb = (nq + QB - 1) / QB;
    const uint64_t nsteps = (ntiles + 3) / 4;
    // one workgroup per CU; a range of at least 8 steps (2048 rows), so that its last compaction and its list
    // in the merge are a small share of it
    uint64_t r = std::max<uint64_t>(1, (uint64_t)num_cus / nqb);
    r = std::min(r, std::max<uint64_t>(1, nsteps / 8));
    // the pools of all workgroups within 256 MiB
    const uint64_t per_range = (uint64_t)nqb * QB * bq_mfma_pool(k) * 8;
    r = std::min<uint64_t>(r, (256ull << 20) / per_range);
    if (r >= 8) r -= r % 8;  // whole rounds over the 8 XCDs: the co-scheduled block order
    return (uint32_t)r;      // 0: the batch's pools do not fit (the caller keeps K5)
}

BqMfmaWs bq_mfma_ws(uint32_t nq, uint32_t k, uint32_t dim, uint32_t ranges)
{
    const uint32_t QB = bq_mfma_qblock(dim), nqb = (nq + QB - 1) / QB, c4 = (bq_chunks(dim) + 3) / 4;
    BqMfmaWs w;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off = (off + bytes + 255) / 256 * 256;
        return at;
    };
    w.part = take((size_t)nq * ranges * k * 8);
    w.pools = take((size_t)ranges * nqb * QB * bq_mfma_pool(k) * 8);
    w.image = take((size_t)nqb * c4 * 8 * (QB / 16) * 1024);
    w.pc = take((size_t)nqb * QB * 4);
    w.total = off;
    return w;
}

template <int NT>
static hipError_t launch_bqm(const BqmArgs &a, uint32_t lds, hipStream_t s)
{
    static const bool attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&scan_bq_mfma_kernel<NT>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(128 * 1024 + BQM_TAIL)) == hipSuccess;
    (void)attr;
    launch_timed((scan_bq_mfma_kernel<NT>), dim3(a.ranges * a.nqb), dim3(BQM_WAVES * 64), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_bq_mfma(const BqMfmaLaunch &L, hipStream_t s)
{
    if (!bq_mfma_supported(L.dim, L.k) || L.ranges == 0 || L.nq == 0) return hipErrorInvalidValue;
    const uint32_t QB = bq_mfma_qblock(L.dim), NT = QB / 16, nqb = (L.nq + QB - 1) / QB;
    const uint32_t c4 = (L.nchunks + 3) / 4;
    const uint32_t lds = c4 * 8 * NT * 1024 + BQM_TAIL;
    if (L.nchunks != bq_chunks(L.dim) || lds > WVG_LDS_BYTES) return hipErrorInvalidValue;
    const BqMfmaWs w = bq_mfma_ws(L.nq, L.k, L.dim, L.ranges);
    BqmArgs a{};
    a.data = reinterpret_cast<const u32x4 *>(L.data);
    a.valid = L.valid;
    a.allow = L.allow;
    a.allow_words = L.allow_words;
    a.allow_t0 = L.allow_t0;
    a.tile_begin = L.tile_begin;
    a.tile_end = L.tile_end;
    a.nchunks = L.nchunks;
    a.c4 = c4;
    a.nq = L.nq;
    a.k = L.k;
    a.ranges = L.ranges;
    a.nqb = nqb;
    a.P = bq_mfma_pool(L.k);
    a.image = reinterpret_cast<const u32x4 *>(L.ws + w.image);
    a.pc = reinterpret_cast<const int32_t *>(L.ws + w.pc);
    a.pools = reinterpret_cast<uint64_t *>(L.ws + w.pools);
    a.partials = reinterpret_cast<uint64_t *>(L.ws + w.part);
    hipLaunchKernelGGL(bqm_image_kernel, dim3(nqb * c4 * 8 * NT), dim3(64), 0, s, L.qcodes, L.qpitch, bq_words(L.dim),
                       L.nq, c4, NT, reinterpret_cast<u32x4 *>(L.ws + w.image),
                       reinterpret_cast<int32_t *>(L.ws + w.pc));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return NT == 4 ? launch_bqm<4>(a, lds, s) : launch_bqm<2>(a, lds, s);
}

}  // namespace wvg

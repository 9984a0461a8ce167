// wvg_screen_pool.hpp -- what the screens that keep lower bounds in survivor pools share: the
// l2-squared lower bound and thresholds (K3c-L2), tau from a k-th lower bound, and the pool
// compaction (K3c-W, wvg_screen.hip; K8m, wvg_pq_mfma.hip).  Device code only.
#pragma once
#include "wvg_internal.hpp"

namespace wvg {

// tau from the k-th smallest lower bound of a list: every one of those k rows
// has its exact distance <= lower + 2 E <= lower_k + 2 Emax.  Not a number
// (-inf + inf: a non-finite query) means no bound: +inf.
__device__ __forceinline__ float sc_tau_k(float lower_k, float emax, int cosine)
{
    const float t = lower_k + 2.0f * emax * (1.0f + 0x1p-10f) + (cosine ? 0x1p-20f : 0.0f);
    return t == t ? t : __builtin_inff();
}

// The l2-squared forms (K3c-L2).  u = (s - h) + E; the lower bound of
// the distance is Cq - 2 u, clamped at 0 (the exact chain sums squares).  NaN
// (a non-finite or huge row or query) -> -inf: always a candidate.
__device__ __forceinline__ float sc_lower_l2(float u, float cq)
{
    const float l = cq - 2.0f * u;
    if (l != l) return -__builtin_inff();
    return __builtin_fmaxf(l, 0.0f);
}

// u-space threshold of a distance threshold tau: at or below the real
// (Cq - tau) / 2, so u < sigma proves Cq - 2 u > tau (a superset test).
__device__ __forceinline__ float sc_sigma_l2(float tau, float cq)
{
    if (!(tau < __builtin_inff())) return -__builtin_inff();
    const float d = cq - tau;
    const float s = __builtin_fmaf(-0x1p-22f, __builtin_fabsf(d), 0.5f * d) - 0x1p-120f;
    return s == s ? s : -__builtin_inff();
}
// (sc_tau_k's dot form, cosine = 0, is the l2-squared one too: k-th lower + 2 Emax_q.)

__device__ __forceinline__ float key_lower(uint64_t key) { return wvg_unord_f32((uint32_t)(key >> 32)); }

// The compaction of one query's pool (a wave; wave-uniform arguments): the k-th smallest lower
// bound of its n <= 768 keys tightens the query's bound t, and every key with lower <= t stays (not
// only k of them: a dropped key at or below the final tau may be a row of the exact top-k), packed
// at the pool's front.  More than cap such keys (the pool must take another row block): only those
// below the (cap + 1)-th smallest lower bound x stay, and *drop keeps the minimum of every such x --
// the smallest lower bound the pool ever let go.  (A later x can be above an earlier one: the fast
// check admits on u >= sigma, and sigma's rounding slack lets a key slightly above the admission
// bound in.)  x is no bound of a distance: the caller admits nothing above min(t, *drop) from here
// on, up to that slack, and collect flags the query if its final tau reaches *drop (K3c's rule for
// a full list).  Returns (truncated << 63) | (kept << 32) | bits of t.  Out of line, and what it
// returns is in registers or LDS: the main loop keeps its allocation, nothing goes through a stack.
constexpr int SW_PMAX = 768;  // 2 * max(k, 64) + 256 at k = 256: 12 keys per lane
typedef __attribute__((address_space(3))) uint32_t lds_u32;
__device__ __attribute__((noinline)) inline uint64_t sc_compact(uint64_t *pool, uint32_t n, uint32_t K, uint32_t cap,
                                                                float emax, int cosine, float t, lds_u32 *drop)
{
    const uint32_t lane = threadIdx.x & 63;
    uint64_t key[SW_PMAX / 64];
#pragma unroll
    for (int i = 0; i < SW_PMAX / 64; i++) {
        const uint32_t j = 64u * i + lane;
        key[i] = j < n ? pool[j] : WVG_KEY_NONE;
    }
    // the R-th smallest ordered lower bound (R <= n) = the largest v with fewer than R values below it, bit by bit
    auto rth = [&](uint32_t R) {
        uint32_t v = 0;
        for (int bit = 31; bit >= 0; bit--) {
            const uint32_t c = v | (1u << bit);
            int below = 0;
#pragma unroll
            for (int i = 0; i < SW_PMAX / 64; i++) below += (uint32_t)(key[i] >> 32) < c;
            for (int off = 32; off > 0; off >>= 1) below += __shfl_xor(below, off);
            if ((uint32_t)below < R) v = c;
        }
        return v;
    };
    if (n >= K) t = fminf(t, sc_tau_k(wvg_unord_f32(rth(K)), emax, cosine));
    uint32_t within = 0;
#pragma unroll
    for (int i = 0; i < SW_PMAX / 64; i++)
        within += (uint32_t)__popcll(__ballot(key[i] != WVG_KEY_NONE && key_lower(key[i]) <= t));
    const bool trunc = within > cap;
    uint32_t x = 0xFFFFFFFFu;
    if (trunc) {
        x = rth(cap + 1);
        if (lane == 0) *drop = min((uint32_t)*drop, x);
    }
    uint32_t kept = 0;
#pragma unroll
    for (int i = 0; i < SW_PMAX / 64; i++) {
        const bool keep = key[i] != WVG_KEY_NONE && (trunc ? (uint32_t)(key[i] >> 32) < x : key_lower(key[i]) <= t);
        const uint64_t bal = __ballot(keep);
        if (keep) pool[kept + __popcll(bal & ((1ull << lane) - 1ull))] = key[i];
        kept += (uint32_t)__popcll(bal);
    }
    return ((uint64_t)trunc << 63) | ((uint64_t)kept << 32) | __float_as_uint(t);
}

}  // namespace wvg

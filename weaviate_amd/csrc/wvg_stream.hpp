// wvg_stream.hpp -- device pieces shared by the query-stream kernels
// (wvg_scan.hip: scan_f32_stream_kernel; wvg_qshare.hip: scan_f32_qshare_kernel):
// the in-launch hand-off of a workgroup's list and the merge of a query's lists
// as they arrive.
#pragma once

#include "wvg_internal.hpp"
#include "wvg_topk.hpp"

namespace wvg {

// Wave index as a wave-uniform (SGPR) value, so per-wave loops, the tile mask
// loads and the skip branch are scalar.
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }

// The merge's end: the WAVES waves' lists tree-merged in LDS, wave 0 writes
// ids / dists / count, or the tagged records (rec) for a host-read result.
// rec (host-read results, see StreamJob::records): entry i goes to rec[i] as ONE
// 16-byte store {id lo, id hi, dist bits, tag}, then the header {count, tag}
// at rec[k] -- the host accepts only entries carrying its call's tag.
template <int E, int WAVES>
__device__ __forceinline__ void merge_finish(WaveTopK<E> &tk, uint32_t k, uint64_t id_base, uint64_t *ids,
                                             float *dists, uint32_t *count, uint4 *rec, uint32_t tag, bool sys_release)
{
    __shared__ uint64_t msh[WAVES][64 * E];
    const int lane = threadIdx.x & 63, wave = wave_id();
#pragma unroll
    for (int e = 0; e < E; e++) msh[wave][e * 64 + lane] = tk.l[e];
    for (int step = 1; step < WAVES; step <<= 1) {
        __syncthreads();
        if ((wave & (2 * step - 1)) == 0) {
            uint64_t o[E];
#pragma unroll
            for (int e = 0; e < E; e++) o[e] = msh[wave + step][e * 64 + lane];
            merge_lists<E>(tk.l, o);
#pragma unroll
            for (int e = 0; e < E; e++) msh[wave][e * 64 + lane] = tk.l[e];
        }
    }
    if (wave != 0) return;
    uint32_t cnt = 0;
#pragma unroll
    for (int e = 0; e < E; e++) {
        const uint32_t i = e * 64 + lane;
        const uint64_t key = tk.l[e];
        const bool live = i < k && key != WVG_KEY_NONE;
        cnt += (uint32_t)__popcll(__ballot(live));
        if (i < k) {
            const uint64_t id = live ? id_base + (key & 0xFFFFFFFFull) : WVG_KEY_NONE;
            const float dv = live ? wvg_unord_f32((uint32_t)(key >> 32)) : __builtin_inff();
            if (rec)  // {slot, tag, dist, tag}: each 8-byte half carries the tag (the host adds id_base)
                rec[i] = make_uint4(live ? (uint32_t)key : 0xFFFFFFFFu, tag, __float_as_uint(dv), tag);
            else {
                ids[i] = id;
                dists[i] = dv;
            }
        }
    }
    if (rec) {
        if (lane == 0)
            __hip_atomic_store(reinterpret_cast<uint64_t *>(rec + k), ((uint64_t)tag << 32) | cnt, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    // sys_release (tools A/B of the round-4 polled layout): a system-scope release between
    // the ids / dists stores and the count the host polls
    if (sys_release) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    if (lane == 0 && count) *count = cnt;
}

constexpr int MERGE_WAVES = 8;  // waves of a phase-2 merge workgroup

// Phase-2 merge body for one query (merge_keys_kernel, wvg_scan.hip; merge_group_kernel, wvg_group.hip): WAVES waves read
// `nlists` ascending lists transposed, then tree-merge in LDS; wave 0 writes.
// rec (host-read results, see StreamJob::records): entry i goes to rec[i] as ONE
// 16-byte store {id lo, id hi, dist bits, tag}, then the header {count, tag}
// at rec[k] -- the host accepts only entries carrying its call's tag.
template <int E, int WAVES>
__device__ __forceinline__ void merge_lists_body(const uint64_t *src, uint32_t nlists, uint32_t list_len, uint32_t k,
                                                 uint64_t id_base, uint64_t *ids, float *dists, uint32_t *count,
                                                 uint4 *rec = nullptr, uint32_t tag = 0, bool sys_release = false)
{
    const int lane = threadIdx.x & 63, wave = wave_id();
    WaveTopK<E> tk;
    tk.init((int)k);
    for (uint32_t g0 = (uint32_t)wave * 64; g0 < nlists; g0 += WAVES * 64) {
        const uint32_t list = g0 + lane;
        const uint64_t *lp = src + (size_t)list * list_len;
        // four entries per lane in flight at a time (independent loads): a one-query
        // merge sits on the launch's critical path, where one dependent load per entry
        // (~1 us each from L2) was most of its time
        bool done = false;
        for (uint32_t r0 = 0; r0 < list_len && !done; r0 += 4) {
            uint64_t c4[4];
#pragma unroll
            for (int i = 0; i < 4; i++)
                c4[i] = (r0 + i < list_len && list < nlists) ? lp[r0 + i] : WVG_KEY_NONE;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t r = r0 + (uint32_t)i;
                if (r >= list_len) break;
                if (list_len > 1 && r > 0 && __ballot(c4[i] < tk.tau) == 0ull) {  // sorted lists: done
                    done = true;
                    break;
                }
                tk.offer(c4[i]);
            }
        }
    }
    merge_finish<E, WAVES>(tk, k, id_base, ids, dists, count, rec, tag, sys_release);
}

__device__ __forceinline__ uint64_t lane_key(uint64_t m, float dist, uint64_t t, int lane)
{
    return ((m >> lane) & 1ull) ? wvg_make_key(dist, (uint32_t)(t * 64 + lane)) : WVG_KEY_NONE;
}

typedef __attribute__((address_space(1))) uint32_t gu32;
typedef __attribute__((address_space(1))) uint64_t gu64;

// The query-stream merge of one query as its lists ARRIVE (StreamJob::ready):
// scan workgroup g stores its list sc1, drains it, then sc1-stores `tag` into
// ready[g]; lane l of merge wave w owns list g = 64 w + l (+ 64 WAVES ...),
// polls its ready word (sc1 load) and, once it matches, reads the list with sc1
// loads (MI355X_MICROARCH.md correctness boundaries: the valid hand-off form
// without an acquire) and offers it to the wave's top-k -- lists that arrive
// early are merged while the scan's stragglers still run, so after the last
// arrival only its own list is left to read.  False after `limit` ticks of
// s_memrealtime without every list.
template <int E, int WAVES>
__device__ __forceinline__ bool merge_lists_ready(const uint64_t *src, const uint32_t *ready, uint32_t tag,
                                                  uint32_t nlists, uint32_t k, uint64_t limit, uint64_t id_base,
                                                  uint64_t *ids, float *dists, uint32_t *count, uint4 *rec,
                                                  uint32_t rtag)
{
    __shared__ int ok_sh;
    const int lane = threadIdx.x & 63, wave = wave_id();
    WaveTopK<E> tk;
    tk.init((int)k);
    const uint64_t start = __builtin_amdgcn_s_memrealtime();
    bool ok = true;
    for (uint32_t g0 = (uint32_t)wave * 64; g0 < nlists && ok; g0 += WAVES * 64) {
        const uint32_t list = g0 + lane;
        bool done = list >= nlists;
        const gu64 *lp = (const gu64 *)(src + (size_t)list * k);
        while (true) {
            const bool rdy = !done && __hip_atomic_load((const gu32 *)(ready + list), __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT) == tag;
            if (__ballot(rdy)) {
                for (uint32_t r0 = 0; r0 < k; r0 += 4) {
                    uint64_t c4[4];
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        c4[i] = rdy && r0 + i < k ? __hip_atomic_load(lp + r0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                                  : WVG_KEY_NONE;
                    bool stop = false;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t r = r0 + (uint32_t)i;
                        if (r >= k) break;
                        if (r > 0 && __ballot(c4[i] < tk.tau) == 0ull) {  // sorted lists: the rest cannot enter
                            stop = true;
                            break;
                        }
                        tk.offer(c4[i]);
                    }
                    if (stop) break;
                }
                done = done || rdy;
            }
            if (__ballot(!done) == 0ull) break;
            if (__builtin_amdgcn_s_memrealtime() - start > limit) {
                ok = false;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    if (threadIdx.x == 0) ok_sh = 1;
    __syncthreads();
    if (!ok && lane == 0) ok_sh = 0;
    __syncthreads();
    if (!ok_sh) return false;
    merge_finish<E, WAVES>(tk, k, id_base, ids, dists, count, rec, rtag, false);
    return true;
}

// Empty results for queries [q0, nq): ids KEY_NONE, dists +inf, counts 0
// (what the host path's write_empty returns for an empty corpus / slab).
__device__ __forceinline__ void fill_empty_body(uint64_t *ids, float *dists, uint32_t *counts, uint32_t q0,
                                                uint32_t nq, uint32_t k)
{
    const uint64_t n = (uint64_t)(nq - q0) * k, off = (uint64_t)q0 * k;
    for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) {
        if (ids) ids[off + i] = WVG_KEY_NONE;
        if (dists) dists[off + i] = __builtin_inff();
    }
    if (counts)
        for (uint32_t q = q0 + threadIdx.x; q < nq; q += blockDim.x) counts[q] = 0;
}

// group_combine_store with write-through stores, then the storing wave drains
// and publishes one arrival (in-launch hand-off, cdna_hip_programming.md §6
// Guideline 16, form R1: agent-scope relaxed atomic stores = sc1, s_waitcnt
// vmcnt(0), then the ready word or the arrival counter; no release fence, so no
// L2 writeback per list).
template <int E, int WAVES>
__device__ __forceinline__ void group_combine_publish(WaveTopK<E> &tk, uint64_t *out, uint32_t *arrivals,
                                                      uint32_t *ready = nullptr, uint32_t tag = 0)
{
    __shared__ uint64_t sh[WAVES][64 * E];
    const int lane = threadIdx.x & 63;
    const int wave = wave_id();
#pragma unroll
    for (int e = 0; e < E; e++) sh[wave][e * 64 + lane] = tk.l[e];
    __syncthreads();
    // pairwise tree, as group_combine_store
#pragma unroll
    for (int half = WAVES / 2; half >= 2; half /= 2) {
        if (wave < half) {
            uint64_t o[E];
#pragma unroll
            for (int e = 0; e < E; e++) o[e] = sh[wave + half][e * 64 + lane];
            merge_lists<E>(tk.l, o);
#pragma unroll
            for (int e = 0; e < E; e++) sh[wave][e * 64 + lane] = tk.l[e];
        }
        __syncthreads();
    }
    if (wave == 0) {
        if (WAVES > 1) {
            uint64_t o[E];
#pragma unroll
            for (int e = 0; e < E; e++) o[e] = sh[1][e * 64 + lane];
            merge_lists<E>(tk.l, o);
        }
#pragma unroll
        for (int e = 0; e < E; e++) {
            const int i = e * 64 + lane;
            if (i < tk.k) __hip_atomic_store((gu64 *)(out + i), tk.l[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            if (ready)  // StreamJob::ready: this list's own flag
                __hip_atomic_store((gu32 *)ready, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                __hip_atomic_fetch_add((gu32 *)arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();  // sh is reused by the next query
}

}  // namespace wvg

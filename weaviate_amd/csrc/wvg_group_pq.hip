// wvg_group_pq.hip -- the PQ kernels of wvg_search_group (wvg_group.hip): nq
// PQ flat searches, query i against a tenant of its own with a codebook of its
// own, as one LUT launch, one scan launch and the grouped merge launch.
//
//  1. pq_lut_group_kernel: DistanceLookUpTable of every query against its own
//     tenant's codebook (CH/product_quantization.go:85-104), entry (q, seg, c) =
//     go_step(metric, q_seg, centers_q[seg][c], ds) -- pq_lut_kernel's entries,
//     the codebook pointer read per query from the call's table.
//  2. scan_pq_group_kernel<E, NC, GL>: workgroup b takes items[b] (GroupItem, a
//     run of tiles of one query's tenant).  Its waves load their first live
//     tiles' codes, then move the query's LUT global -> LDS (16 bytes per lane,
//     global_load_lds, 1 KiB units dealt over the waves: no VGPR round trip), so
//     the first HBM latency sits under the staging; one barrier; then K8's loop
//     (wvg_pq.hip): lane = row, the next live tile's codes (non-temporal) in
//     flight while this tile's m lookups are gathered and summed in segment
//     order, Wrap, K8's keys, WaveTopK<E>, group_combine_store into the item's
//     list.  GL: the LUT stays in global memory / L2 (no staging, no barrier).
//     Roofline: HBM / Infinity Cache for the codes, the LDS gather for the sums
//     (random codes: bank conflicts, as K8); the LUT staging is the fixed cost
//     per item that the item rule (group_pq_item_tiles) amortizes.
#include <algorithm>
#include <map>
#include <mutex>

#include "wvg_host.hpp"
#include "wvg_rowdist.hpp"
#include "wvg_stream.hpp"
#include "wvg_topk.hpp"

namespace wvg {

typedef __attribute__((address_space(1))) const float gfl;
typedef __attribute__((address_space(1))) const uint4 ggu4;
typedef unsigned int gpq_u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void pq_lut_group_kernel(GroupPqArgs a)
{
    const uint32_t qi = blockIdx.y;
    cgq *d = (cgq *)a.desc + qi;
    if (d->nlists == 0) return;  // nothing live or allowed: no scan reads this LUT
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.m * a.ks) return;
    const float *centers = (const float *)(gfl *)(uintptr_t)((cgu64 *)a.centers)[qi];
    const uint32_t seg = r / a.ks, c = r % a.ks;
    a.luts[(size_t)qi * a.lpitch + r] = go_step(a.metric, a.queries + (size_t)qi * a.qpitch + (size_t)seg * a.ds,
                                                centers + ((size_t)seg * a.ks + c) * a.ds, a.ds);
}

// Workgroup size by what the LUT leaves of a CU's 160 KiB: up to four chunks
// per row (m <= 64: a LUT of at most 64 KiB at ks = 256) two or more
// workgroups share a CU, so 8 waves each; above it, and in the generic form,
// one workgroup owns the CU and brings K8's 16 waves.
constexpr int gpq_waves(int nc) { return nc >= 1 && nc <= 4 ? 8 : 16; }

__device__ __forceinline__ uint4 gpq_ld_codes(const uint4 *p)
{
    const gpq_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const gpq_u32x4 *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ uint32_t gpq_byte(const uint4 &v, int b)
{
    const int w = b >> 2;
    const uint32_t word = w == 0 ? v.x : (w == 1 ? v.y : (w == 2 ? v.z : v.w));
    return (word >> (8 * (b & 3))) & 0xFFu;
}

template <int E, int NC, bool GL>
__global__ __launch_bounds__(gpq_waves(NC) * 64) void scan_pq_group_kernel(GroupPqArgs a)
{
    static_assert(!GL || NC == 0, "the global-LUT form is the generic kernel's");
    constexpr int WV = gpq_waves(NC);
    extern __shared__ __attribute__((aligned(16))) float lut[];
    cgi *ip = (cgi *)a.items + blockIdx.x;
    const uint32_t qi = ip->query, range = ip->range;
    const uint64_t i0 = ip->t0, i1 = ip->t1;
    cgq *d = (cgq *)a.desc + qi;
    cgu64 *valid = (cgu64 *)d->valid;
    const bool filtered = d->filtered != 0;
    cgu64 *allow = (cgu64 *)a.allow + d->allow_off;
    const uint64_t allow_words = d->allow_words, allow_t0 = d->allow_t0;
    const uint4 *data = (const uint4 *)(ggu4 *)d->data;
    const float *glut = a.luts + (size_t)qi * a.lpitch;
    const uint32_t ks = a.ks;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)wave_id();
    // the item's tiles split over the waves as K1 splits a workgroup's (wave_range)
    const uint64_t n_item = i1 - i0;
    const uint64_t t0 = i0 + n_item * wave / WV, t1 = i0 + n_item * (wave + 1) / WV;
    // The query's LUT into LDS: unit u = bytes [1024 u, 1024 (u + 1)), one wave-wide 16-byte transfer,
    // lane l writing its 16 bytes at 16 l of the unit; lpitch is a multiple of 4 floats, so only whole
    // 16-byte pieces exist and the last unit is cut by lane.
    auto stage = [&]() {
        const uint32_t bytes = a.lpitch * 4u;
        const uint4 *src = reinterpret_cast<const uint4 *>(glut) + lane;
        unsigned char *dst = reinterpret_cast<unsigned char *>(lut);
        for (uint32_t u = wave; u * 1024u < bytes; u += WV)
            if (u * 1024u + (uint32_t)lane * 16u < bytes)
                __builtin_amdgcn_global_load_lds(src + (size_t)u * 64, reinterpret_cast<uint4 *>(dst + u * 1024u), 16, 0, 0);
    };
    WaveTopK<E> tk;
    tk.init((int)a.k);
    if constexpr (NC > 0) {
        constexpr int M = 16 * NC;
        auto next_live = [&](uint64_t t, uint64_t &msk) {  // next tile at or after t with a live allowed row
            for (; t < t1; ++t) {
                msk = group_tile_mask(valid, allow, filtered, allow_words, allow_t0, t);
                if (msk) break;
            }
            return t;
        };
        uint64_t m_cur = 0, m_nxt = 0;
        uint64_t t = next_live(t0, m_cur);
        uint4 cur[NC], nxt[NC];
        if (t < t1) {
            const uint4 *rp = data + (size_t)t * NC * 64 + lane;
#pragma unroll
            for (int c = 0; c < NC; c++) cur[c] = gpq_ld_codes(rp + (size_t)c * 64);
        }
        stage();  // behind the first tile's code loads, in the same queue
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's transfers (and its codes) have landed
        __syncthreads();                                   // and so have every other wave's
        while (t < t1) {
            const uint64_t tn = next_live(t + 1, m_nxt);
            if (tn < t1) {
                const uint4 *rp = data + (size_t)tn * NC * 64 + lane;
#pragma unroll
                for (int c = 0; c < NC; c++) nxt[c] = gpq_ld_codes(rp + (size_t)c * 64);
            }
            uint4 uc[NC];  // codes in segment order (m = 32 rows are stored rotated: pq_rotated)
            if constexpr (M == 32) {
                const uint32_t w[8] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y, cur[1].z, cur[1].w};
                uint32_t o[8];
                pq32_window(w, (32u - ((uint32_t)lane & 31u)) & 31u, o);
                uc[0] = make_uint4(o[0], o[1], o[2], o[3]);
                uc[1] = make_uint4(o[4], o[5], o[6], o[7]);
            } else {
#pragma unroll
                for (int c = 0; c < NC; c++) uc[c] = cur[c];
            }
            // a chunk's 16 lookups are independent ds_reads; the adds run in segment order
            float sum = 0.0f;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                float v[16];
#pragma unroll
                for (int b = 0; b < 16; b++) v[b] = lut[(uint32_t)(c * 16 + b) * ks + gpq_byte(uc[c], b)];
#pragma unroll
                for (int b = 0; b < 16; b++) sum = sum + v[b];
            }
            const float dist = wrap_metric(a.metric, sum);
            tk.offer(((m_cur >> lane) & 1ull) ? wvg_make_key(dist, (uint32_t)(t * 64 + lane)) : WVG_KEY_NONE);
#pragma unroll
            for (int c = 0; c < NC; c++) cur[c] = nxt[c];
            t = tn;
            m_cur = m_nxt;
        }
    } else {
        if constexpr (!GL) {
            stage();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        const uint32_t nch = a.nchunks, m = a.m;
        for (uint64_t t = t0; t < t1; ++t) {
            const uint64_t msk = group_tile_mask(valid, allow, filtered, allow_words, allow_t0, t);
            if (msk == 0ull) continue;  // wave-uniform
            const uint4 *rp = data + (size_t)t * nch * 64 + lane;
            const float sum = GL ? pq_row_sum(rp, nch, m, ks, glut, (uint64_t)lane)
                                 : pq_row_sum(rp, nch, m, ks, lut, (uint64_t)lane);
            const float dist = wrap_metric(a.metric, sum);
            tk.offer(((msk >> lane) & 1ull) ? wvg_make_key(dist, (uint32_t)(t * 64 + lane)) : WVG_KEY_NONE);
        }
    }
    group_combine_store<E, WV>(tk, a.partials + ((size_t)d->list0 + range) * a.k);
}

hipError_t launch_pq_lut_group(const GroupPqArgs &a, uint32_t nq, hipStream_t s)
{
    const uint32_t per_q = a.m * a.ks;
    if (nq == 0 || per_q == 0) return hipSuccess;
    hipLaunchKernelGGL(pq_lut_group_kernel, dim3((per_q + 255) / 256, nq), dim3(256), 0, s, a);
    return hipGetLastError();
}

// Resident workgroups per CU of a form, as the runtime counts them from the
// kernel's registers and LDS; asked once per (kernel, LUT size).
static int gpq_resident(void (*kernel)(GroupPqArgs), int waves, uint32_t lds)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, uint32_t>, int> known;
    std::lock_guard<std::mutex> g(mu);
    const auto key = std::make_pair(reinterpret_cast<const void *>(kernel), lds);
    auto it = known.find(key);
    if (it != known.end()) return it->second;
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, reinterpret_cast<const void *>(kernel), waves * 64, lds) != hipSuccess) {
        (void)hipGetLastError();
        n = 1;
    }
    n = std::max(n, 1);
    known[key] = n;
    return n;
}

// The LDS form while the LUT (lpitch floats) fits beside the instantiation's
// own static LDS -- group_combine_store's buffer, waves x 64 E keys: 4 / 8 /
// 16 KiB for 8 waves, 8 / 16 / 32 KiB for 16 -- in a workgroup's 160 KiB
// (fits_lds).  At ks = 256 the generic kernel's LDS form ends at m = 152 / 144 /
// 128 for E = 1 / 2 / 4, K8's own limits (launch_pq_k8); every fixed-NC form
// fits (m <= 128).  Above it: the generic kernel's global-LUT form.
template <int E, int NC>
static void gpq_form_nc(GroupPqForm &f, uint32_t lut_bytes)
{
    f.e = E;
    f.nc = NC;
    f.waves = gpq_waves(NC);
    if (fits_lds<&scan_pq_group_kernel<E, NC, false>>(lut_bytes)) {
        f.kernel = &scan_pq_group_kernel<E, NC, false>;
        f.lds = lut_bytes;
        return;
    }
    if constexpr (NC == 0) {
        f.kernel = &scan_pq_group_kernel<E, 0, true>;
        f.gl = true;
        f.lds = 0;
    }
}

template <int E>
static GroupPqForm gpq_form_e(uint32_t m, uint32_t ks)
{
    GroupPqForm f;
    const uint32_t lut_bytes = (uint32_t)align_up((size_t)m * ks, 4) * 4u;
    switch (m % 16 == 0 ? m / 16 : 0) {  // whole chunks only: a partial chunk is the generic form's
    case 1: gpq_form_nc<E, 1>(f, lut_bytes); break;
    case 2: gpq_form_nc<E, 2>(f, lut_bytes); break;
    case 4: gpq_form_nc<E, 4>(f, lut_bytes); break;
    case 6: gpq_form_nc<E, 6>(f, lut_bytes); break;
    case 8: gpq_form_nc<E, 8>(f, lut_bytes); break;
    default: break;
    }
    if (!f.kernel) gpq_form_nc<E, 0>(f, lut_bytes);
    f.per_cu = gpq_resident(f.kernel, f.waves, f.lds);
    return f;
}

GroupPqForm group_pq_form(uint32_t m, uint32_t ks, uint32_t k)
{
    if (k <= 64) return gpq_form_e<1>(m, ks);
    if (k <= 128) return gpq_form_e<2>(m, ks);
    return gpq_form_e<4>(m, ks);
}

// The PQ item rule.  T = max(floor, ceil(total_tiles / (CUs x S))).  The floor
// pays for the staging: an LDS-form item holds at least Tuning::group_pq_floor
// (c = 1) x its LUT's bytes in code bytes (a tile is nchunks KiB of codes: 16
// tiles at ks = 256 with m a multiple of 16) and never fewer than two tiles per
// wave; the global-LUT form stages nothing and keeps only the two tiles per
// wave.  The ceiling term spreads a large call as S = Tuning::
// group_pq_items_per_cu (1) items per CU -- not per resident workgroup: the
// workgroups of a CU share its LDS pipe, which the gather saturates, so a second
// resident item only adds its staging ("Grouped PQ search
// over tenants", has the A/B).  A tenant of at most T tiles is one item.
uint32_t group_pq_item_tiles(uint64_t total_tiles, int num_cus, const GroupPqForm &f, uint32_t m, uint32_t ks)
{
    const int s = tuning().group_pq_items_per_cu;
    const uint64_t per = (uint64_t)std::max(num_cus, 1) * (uint64_t)(s > 0 ? s : 2 * std::max(f.per_cu, 1));
    uint64_t floor_t = 2ull * (uint64_t)f.waves;
    if (!f.gl) {
        const uint64_t c = (uint64_t)std::max(tuning().group_pq_floor, 1);
        const uint64_t tile_bytes = (uint64_t)pq_chunks(m) * 1024ull;
        floor_t = std::max<uint64_t>(floor_t, (c * (uint64_t)m * ks * 4ull + tile_bytes - 1) / tile_bytes);
    }
    const uint64_t t = std::max(floor_t, (total_tiles + per - 1) / per);
    return (uint32_t)std::min<uint64_t>(t, 0xFFFFFFFFull);
}

hipError_t launch_scan_pq_group(const GroupPqArgs &a, const GroupPqForm &f, uint32_t nitems, hipStream_t s)
{
    if (nitems == 0) return hipSuccess;
    launch_timed(f.kernel, dim3(nitems), dim3(f.waves * 64), f.lds, s, a);
    return hipGetLastError();
}

}  // namespace wvg

// wvg_group.hip -- wvg_search_group: nq flat.SearchByVector calls
// (V/flat/index.go:307-334), query i against a corpus of its own -- the shards
// of a multi-tenant class, where a query names exactly one tenant
// (adapters/repos/db/index.go:1516-1539, 1554-1565) -- as one scan launch and
// one merge launch, one copy in and one copy out.
//
// The host writes a descriptor per query (GroupQuery: the corpus's rows and
// validity words, its allow window, its lists) and a table of work items
// (GroupItem: a run of at most T tiles of one query's corpus,
// group_item_tiles).  Scan workgroup b takes items[b]: its four waves split the
// item's tiles (lane = row), fold each row with K1's chains (wvg_rowdist.hpp,
// the calls of scan_tiles, wvg_scan.hip) into K1's keys and leave one k-list
// per item.  Merge workgroup q merges query q's lists with merge_lists_body.
// The second launch starts after the first by stream order: neither kernel
// polls or waits for anything.
// Roofline: HBM / Infinity Cache, the sum of the scanned tenants' bytes.
#include <algorithm>
#include <mutex>
#include <shared_mutex>

#include "wvg_host.hpp"
#include "wvg_rowdist.hpp"
#include "wvg_stream.hpp"
#include "wvg_topk.hpp"

namespace wvg {

// The tables, the queries, the validity words and the allow windows are written
// before the launch and by nobody during it, and every index into them is
// wave-uniform: read through the constant address space they are scalar loads
// and the pointers, tile ranges and masks stay in SGPRs.  The pointers a
// descriptor holds are global ones; saying so keeps the row loads global_load
// (a pointer loaded from memory is a flat one to the compiler).
typedef __attribute__((address_space(4))) const GroupQuery cgq;
typedef __attribute__((address_space(4))) const GroupItem cgi;
typedef __attribute__((address_space(4))) const uint64_t cgu64;
typedef __attribute__((address_space(4))) const float4 cgf4;
typedef __attribute__((address_space(1))) const float4 ggf4;

// Mask of live, allowed rows of tile t (tile_mask of wvg_scan.hip on the descriptor's scalars).
__device__ __forceinline__ uint64_t group_tile_mask(cgu64 *valid, cgu64 *allow, bool filtered, uint64_t allow_words,
                                                    uint64_t allow_t0, uint64_t t)
{
    uint64_t m = valid[t];
    if (filtered) {
        const uint64_t w = t - allow_t0;  // allow[0] is tile allow_t0's word
        m &= w < allow_words ? allow[w] : 0ull;
    }
    return m;
}

template <int METRIC, int D, int E>
__global__ __launch_bounds__(SCAN_WAVES * 64) void scan_f32_group_kernel(GroupArgs a)
{
    cgi *ip = (cgi *)a.items + blockIdx.x;
    const uint32_t qi = ip->query, range = ip->range;
    const uint64_t i0 = ip->t0, i1 = ip->t1;
    cgq *d = (cgq *)a.desc + qi;
    cgu64 *valid = (cgu64 *)d->valid;
    const bool filtered = d->filtered != 0;
    cgu64 *allow = (cgu64 *)a.allow + d->allow_off;
    const uint64_t allow_words = d->allow_words, allow_t0 = d->allow_t0;
    const float4 *data = (const float4 *)(ggf4 *)d->data;
    const float4 *q4 = (const float4 *)((cgf4 *)a.queries + (size_t)qi * (a.qpitch / 4));
    const int lane = threadIdx.x & 63;
    // the item's tiles split over the waves as K1 splits a workgroup's (wave_range)
    const uint64_t n_item = i1 - i0, w = (uint64_t)wave_id();
    const uint64_t t0 = i0 + n_item * w / SCAN_WAVES, t1 = i0 + n_item * (w + 1) / SCAN_WAVES;
    const uint64_t n = t1 - t0;
    WaveTopK<E> tk;
    tk.init((int)a.k);
    // scan_tiles (wvg_scan.hip) with the default cache policy: one tile's loads in flight per
    // wave, tiles with no live / allowed row skipped without touching their rows
    uint64_t m_next = n ? group_tile_mask(valid, allow, filtered, allow_words, allow_t0, t0) : 0ull;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t t = t0 + i;
        const uint64_t m = m_next;
        if (i + 1 < n) m_next = group_tile_mask(valid, allow, filtered, allow_words, allow_t0, t + 1);  // scalar prefetch
        if (m == 0ull) continue;  // wave-uniform
        const float4 *rp = data + (size_t)t * a.nchunks * 64 + lane;
        float r;
        if (a.order512)  // wave-uniform: the AVX-512 kernels' order (generic length)
            r = row_dist_512<METRIC, 64>(rp, q4, (int)a.dim);
        else if constexpr (D > 0)
            r = row_dot_or_l2_fixed<METRIC, D, 64, false>(rp, q4);
        else
            r = row_dot_or_l2_generic<METRIC, 64>(rp, q4, (int)a.dim);
        tk.offer(lane_key(m, wrap_metric(a.metric, r), t, lane));
    }
    group_combine_store<E, SCAN_WAVES>(tk, a.partials + ((size_t)d->list0 + range) * a.k);
}

template <int E>
__global__ __launch_bounds__(MERGE_WAVES * 64) void merge_group_kernel(const GroupQuery *desc, const uint64_t *partials,
                                                                       uint32_t k, uint64_t *ids, float *dists,
                                                                       uint32_t *counts)
{
    const uint32_t q = blockIdx.x;
    cgq *d = (cgq *)desc + q;
    const uint32_t nlists = d->nlists;
    if (nlists == 0) {  // nothing live or allowed: wvg_search's empty result
        fill_empty_body(ids, dists, counts, q, q + 1, k);
        return;
    }
    merge_lists_body<E, MERGE_WAVES>(partials + (size_t)d->list0 * k, nlists, k, k, d->id_base, ids + (size_t)q * k,
                                     dists + (size_t)q * k, counts + q);
}

template <int METRIC, int E>
static hipError_t launch_group_e(const GroupArgs &a, uint32_t nitems, hipStream_t s)
{
    dim3 grid(nitems), block(SCAN_WAVES * 64);
    switch (a.dim) {  // K1's fixed row lengths (launch_f32_e, wvg_scan.hip)
    case 128: launch_timed((scan_f32_group_kernel<METRIC, 128, E>), grid, block, 0, s, a); break;
    case 768: launch_timed((scan_f32_group_kernel<METRIC, 768, E>), grid, block, 0, s, a); break;
    case 1536: launch_timed((scan_f32_group_kernel<METRIC, 1536, E>), grid, block, 0, s, a); break;
    default: launch_timed((scan_f32_group_kernel<METRIC, 0, E>), grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}

template <int METRIC>
static hipError_t launch_group_m(const GroupArgs &a, uint32_t nitems, hipStream_t s)
{
    if (a.k <= 64) return launch_group_e<METRIC, 1>(a, nitems, s);
    if (a.k <= 128) return launch_group_e<METRIC, 2>(a, nitems, s);
    return launch_group_e<METRIC, 4>(a, nitems, s);
}

hipError_t launch_scan_f32_group(const GroupArgs &a, uint32_t nitems, hipStream_t s)
{
    if (nitems == 0) return hipSuccess;
    return with_metric(a.metric, [&](auto M) { return launch_group_m<decltype(M)::value>(a, nitems, s); });
}

hipError_t launch_merge_group(const GroupQuery *desc, const uint64_t *partials, uint32_t nq, uint32_t k, uint64_t *ids,
                              float *dists, uint32_t *counts, hipStream_t s)
{
    if (nq == 0) return hipSuccess;
    dim3 grid(nq), block(MERGE_WAVES * 64);
    if (k <= 64)
        hipLaunchKernelGGL((merge_group_kernel<1>), grid, block, 0, s, desc, partials, k, ids, dists, counts);
    else if (k <= 128)
        hipLaunchKernelGGL((merge_group_kernel<2>), grid, block, 0, s, desc, partials, k, ids, dists, counts);
    else
        hipLaunchKernelGGL((merge_group_kernel<4>), grid, block, 0, s, desc, partials, k, ids, dists, counts);
    return hipGetLastError();
}

// The item rule.  A call's `total_tiles` (the sum of its queries' tile ranges)
// are cut into items of at most T tiles,
//   T = max(2 * SCAN_WAVES, ceil(total_tiles / (GROUP_ITEMS_PER_SLOT * slots))),
// slots = 2 x the CUs: the L2 and dot forms of the scan kernel need 173-237
// VGPRs, two waves per SIMD, so two 4-wave workgroups are resident per CU.  A query of n
// tiles gets ceil(n / T) items whose bounds are tile_begin + n * r / nlists:
// near-equal, none above T; a tenant of at most T tiles is one item.  The floor
// keeps K1's two tiles per wave (below it the combine and the list store
// outweigh the rows); the ceiling term gives a large call about two items per
// resident workgroup, so the last ones level the CUs.
constexpr uint64_t GROUP_ITEMS_PER_SLOT = 2;
uint32_t group_item_tiles(uint64_t total_tiles, int num_cus)
{
    const uint64_t per = GROUP_ITEMS_PER_SLOT * 2 * (uint64_t)std::max(num_cus, 1);
    const uint64_t t = std::max<uint64_t>(2 * SCAN_WAVES, (total_tiles + per - 1) / per);
    return (uint32_t)std::min<uint64_t>(t, 0xFFFFFFFFull);
}

}  // namespace wvg

using namespace wvg;

extern "C" {

int wvg_search_group(wvg_corpus *const *corpora, const float *queries, uint32_t nq, uint32_t k,
                     const uint64_t *const *allow_bits, const uint64_t *allow_words, uint64_t *out_ids,
                     float *out_dists, uint32_t *out_counts)
{
    if (nq == 0) return WVG_OK;
    if (!corpora) return fail(WVG_ERR_INVALID, "null corpora");
    if (!queries) return fail(WVG_ERR_INVALID, "null queries");
    for (uint32_t i = 0; i < nq; i++) {
        const wvg_corpus *c = corpora[i], *c0 = corpora[0];
        const std::string at = "corpora[" + std::to_string(i) + "]";
        if (!c || !c->ctx) return fail(WVG_ERR_INVALID, at + " is null");
        if (c->ctx != c0->ctx) return fail(WVG_ERR_INVALID, at + " belongs to another context than corpora[0]");
        if (c->dim != c0->dim) return fail(WVG_ERR_INVALID, at + " differs from corpora[0] in dim");
        if (c->metric != c0->metric) return fail(WVG_ERR_INVALID, at + " differs from corpora[0] in metric");
        if (allow_bits && allow_bits[i] && !allow_words)
            return fail(WVG_ERR_INVALID, "allow_bits[" + std::to_string(i) + "] without allow_words");
    }
    for (uint32_t i = 0; i < nq; i++)
        if (corpora[i]->kind != WVG_KIND_F32)
            return fail(WVG_ERR_UNSUPPORTED, "corpora[" + std::to_string(i) + "] is not an F32 corpus (grouped search: F32 only)");
    if (k > MAX_K) return fail(WVG_ERR_UNSUPPORTED, "grouped search: k above 256");
    wvg_corpus *c0 = corpora[0];
    wvg_ctx *ctx = c0->ctx;
    WVG_HIP(hipSetDevice(ctx->device));

    // Shared locks of the distinct corpora in ascending address order: with a
    // writer-preferring shared_mutex, calls that took overlapping sets in
    // different orders while writers wait could deadlock; one order cannot.
    // Held until the results are on the host (as search_batch holds its one).
    std::vector<wvg_corpus *> uniq(corpora, corpora + nq);
    std::sort(uniq.begin(), uniq.end(), std::less<wvg_corpus *>());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    std::vector<std::shared_lock<std::shared_mutex>> locks;
    locks.reserve(uniq.size());
    for (wvg_corpus *c : uniq) locks.emplace_back(c->rw);

    if (k == 0) {  // as wvg_search: counts 0, nothing else to write
        write_empty(nq, 0, out_ids, out_dists, out_counts);
        return WVG_OK;
    }

    // the plan: per query its tile range and allow window, then the items
    std::vector<GroupQuery> desc(nq);
    std::vector<const uint64_t *> win(nq, nullptr);  // the caller's words of each window
    uint64_t total_tiles = 0, allow_total = 0;
    for (uint32_t i = 0; i < nq; i++) {
        const wvg_corpus *c = corpora[i];
        const uint64_t *allow = allow_bits ? allow_bits[i] : nullptr;
        GroupQuery &d = desc[i];
        d = GroupQuery{};
        d.data = c->d_data;
        d.valid = c->d_valid;
        d.id_base = c->id_base;
        uint64_t tb = 0, te = 0;
        if (!allow_tile_range(c, allow, allow ? allow_words[i] : 0, tb, te)) continue;  // nlists stays 0
        d.tile_begin = tb;
        d.tile_end = te;
        if (allow) {
            d.filtered = 1;
            d.allow_off = allow_total;
            d.allow_words = te - tb;
            d.allow_t0 = tb;
            win[i] = allow + c->id_base / 64 + tb;
            allow_total += te - tb;
        }
        total_tiles += te - tb;
    }
    if (total_tiles == 0) {
        write_empty(nq, k, out_ids, out_dists, out_counts);
        return WVG_OK;
    }
    const uint64_t T = group_item_tiles(total_tiles, ctx->num_cus);
    uint64_t nlists_total = 0;
    for (uint32_t i = 0; i < nq; i++) {
        GroupQuery &d = desc[i];
        const uint64_t n = d.tile_end - d.tile_begin;
        if (nlists_total + (n + T - 1) / T > 0x7FFFFFFFull) return fail(WVG_ERR_UNSUPPORTED, "grouped search: too many work items");
        d.list0 = (uint32_t)nlists_total;
        d.nlists = (uint32_t)((n + T - 1) / T);
        nlists_total += d.nlists;
    }
    const uint32_t nitems = (uint32_t)nlists_total;

    SlotGuard g(ctx);
    int rc = ctx->acquire(&g.slot);
    if (rc) return rc;
    const uint32_t qpitch = f32_chunks(c0->dim) * 4;
    // device scratch: the input block [queries | descriptors | items | allow windows], the lists, the results
    Carver in;
    const size_t i_q = in.take((size_t)nq * qpitch * 4);
    const size_t i_desc = in.take((size_t)nq * sizeof(GroupQuery));
    const size_t i_items = in.take((size_t)nitems * sizeof(GroupItem));
    const size_t i_allow = in.take((size_t)allow_total * 8);
    const size_t in_b = in.off;
    Carver cv;
    const size_t o_in = cv.take(in_b);
    const size_t o_part = cv.take((size_t)nitems * k * 8);
    const size_t o_ids = cv.take((size_t)nq * k * 8);
    const size_t o_d = cv.take((size_t)nq * k * 4);
    const size_t o_cnt = cv.take((size_t)nq * 4);
    const size_t out_b = o_cnt + (size_t)nq * 4 - o_ids;
    void *base = nullptr;
    rc = g.slot->device_scratch(cv.off, &base);
    if (rc) return rc;
    char *b = (char *)base;
    hipStream_t s = g.slot->stream;
    void *pinned = nullptr;
    rc = g.slot->host_pinned(in_b + align_up(out_b, 64), &pinned);
    if (rc) return rc;
    char *hin = (char *)pinned, *hout = hin + in_b;

    // queries as stage_queries / prepare_queries_host prepare them for an F32 corpus
    {
        std::vector<float> qf;
        std::vector<uint64_t> qb;
        uint32_t qp = 0;
        prepare_queries_host(c0, queries, nq, qf, qb, qp);
        std::memcpy(hin + i_q, qf.data(), (size_t)nq * qpitch * 4);
    }
    GroupItem *items = reinterpret_cast<GroupItem *>(hin + i_items);
    for (uint32_t i = 0, at = 0; i < nq; i++) {
        const GroupQuery &d = desc[i];
        const uint64_t n = d.tile_end - d.tile_begin;
        for (uint32_t r = 0; r < d.nlists; r++, at++)
            items[at] = GroupItem{i, r, (uint32_t)(d.tile_begin + n * r / d.nlists),
                                  (uint32_t)(d.tile_begin + n * (r + 1) / d.nlists)};
        if (win[i]) std::memcpy(hin + i_allow + d.allow_off * 8, win[i], d.allow_words * 8);
    }
    std::memcpy(hin + i_desc, desc.data(), (size_t)nq * sizeof(GroupQuery));

    WVG_HIP(hipMemcpyAsync(b + o_in, hin, in_b, hipMemcpyHostToDevice, s));
    GroupArgs a{};
    a.desc = reinterpret_cast<const GroupQuery *>(b + o_in + i_desc);
    a.items = reinterpret_cast<const GroupItem *>(b + o_in + i_items);
    a.queries = reinterpret_cast<const float *>(b + o_in + i_q);
    a.allow = reinterpret_cast<const uint64_t *>(b + o_in + i_allow);
    a.partials = reinterpret_cast<uint64_t *>(b + o_part);
    a.qpitch = qpitch;
    a.k = k;
    a.dim = c0->dim;
    a.nchunks = c0->nchunks;
    a.metric = c0->metric;
    a.order512 = ctx->order512;
    {
        ProfArm arm(ctx);  // wvg_profile_*: the scan dispatch's own events
        if (arm.rc) return arm.rc;
        WVG_HIP(launch_scan_f32_group(a, nitems, s));
    }
    WVG_HIP(launch_merge_group(a.desc, a.partials, nq, k, (uint64_t *)(b + o_ids), (float *)(b + o_d),
                               (uint32_t *)(b + o_cnt), s));
    WVG_HIP(hipMemcpyAsync(hout, b + o_ids, out_b, hipMemcpyDeviceToHost, s));
    WVG_HIP(hipStreamSynchronize(s));
    if (out_ids) std::memcpy(out_ids, hout, (size_t)nq * k * 8);
    if (out_dists) std::memcpy(out_dists, hout + (o_d - o_ids), (size_t)nq * k * 4);
    if (out_counts) std::memcpy(out_counts, hout + (o_cnt - o_ids), (size_t)nq * 4);
    return WVG_OK;
}

}  // extern "C"

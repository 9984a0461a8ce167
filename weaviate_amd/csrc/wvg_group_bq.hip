// wvg_group_bq.hip -- wvg_search_group_bq_rescore / _bq_candidates: nq
// flat.searchByVectorBQ calls (V/flat/index.go:347-389), query i against a
// tenant of its own (adapters/repos/db/index.go:1516-1539, 1554-1565), as three
// launches whatever nq is.  The result is the reference heap's own
// (findTopVectorsCached, index.go:456-506; the pop loop and the k-heap fed in
// pop order, :368-385), as wvg_search_bq_rescore's (wvg_replay.hip).
//
// The exact flow of a lone corpus records per wave against the wave's own
// running R-th distance; a grouped work item gives a wave ~128 rows, which with
// R = 200 would record every row.  So the grouped flow has kernels of its own:
//  1. scan_bq_group_kernel: workgroup b takes items[b] (GroupItem, the item rule
//     of wvg_group.hip) and stores each row's Hamming distance as a u16 into its
//     query's distance strip (slot - 64 * tile_begin).  No top-k.  Roofline:
//     HBM / Infinity Cache, the scanned tenants' code bytes (2 B written per
//     16-192 B read).
//  2. bq_group_filter_kernel: one workgroup per query walks the strip in docID
//     order, 256 rows at a time, with an LDS histogram of the live distances
//     seen so far.  T at a chunk's start = the R-th smallest of them (+inf below
//     R rows); the chunk's live rows with d < T are appended, in slot order, to
//     the query's record list.  T is an upper bound of the heap's threshold
//     T_i for every row i of the chunk (T_i is the R-th smallest over a longer
//     prefix), so the records are a superset of the rows insertToHeap accepts,
//     and replaying a superset in docID order reproduces the heap
//     (wvg_replay.hip "How").  A record list holds its window's rows: nothing
//     overflows, no rerun.
//  3. rescore_group_kernel: the popped candidates' exact distances from their
//     tenant's float rows (rescore_keys_kernel's arithmetic, the rows from the
//     query's own F32 corpus).
// Host: one copy in; totals + a head of records per query back (queries beyond
// the head: one more round); the R-heap replay; candidates in; distances back;
// the k-heap.  Launches, copies and syncs do not depend on nq.
#include <algorithm>
#include <mutex>
#include <shared_mutex>

#include "wvg_host.hpp"
#include "wvg_rowdist.hpp"

namespace wvg {

// Descriptors, items, masks and query codes: written before the launch, indexed
// wave-uniformly -- scalar loads through the constant address space (wvg_group.hip).
typedef __attribute__((address_space(4))) const GroupQuery cgq;
typedef __attribute__((address_space(4))) const GroupItem cgi;
typedef __attribute__((address_space(4))) const uint64_t cgu64;
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) const u64x2 ggx2;

struct GroupBqArgs {
    const GroupQuery *desc;   // [nq]; list0 = the query's first tile in the strips / records
    const GroupItem *items;   // [gridDim.x]
    const uint64_t *qcodes;   // [nq][qpitch] query code words
    const uint64_t *allow;    // the call's allow windows, back to back
    uint16_t *strips;         // [total tiles][64] Hamming distances
    uint32_t qpitch, nchunks;
};

constexpr int GBQ_WAVES = 4;
constexpr uint32_t GBQ_PAD = 0xFFFFFFFFu;  // slot of a padding candidate

__device__ __forceinline__ uint64_t gbq_tile_mask(cgu64 *valid, cgu64 *allow, bool filtered, uint64_t allow_words,
                                                  uint64_t allow_t0, uint64_t t)
{
    uint64_t m = valid[t];
    if (filtered) {
        const uint64_t w = t - allow_t0;  // allow[0] is tile allow_t0's word
        m &= w < allow_words ? allow[w] : 0ull;
    }
    return m;
}

// K5's body (XOR + popcount over the tile's 16-byte chunks, lane = row) on a work
// item; fixed NCH keeps the next live tile's chunks in flight while the current
// one is reduced.  Tiles with no live allowed row are neither loaded nor written.
template <int NCH>
__global__ __launch_bounds__(GBQ_WAVES * 64) void scan_bq_group_kernel(GroupBqArgs a)
{
    cgi *ip = (cgi *)a.items + blockIdx.x;
    const uint32_t qi = ip->query;
    const uint64_t i0 = ip->t0, i1 = ip->t1;
    cgq *d = (cgq *)a.desc + qi;
    cgu64 *valid = (cgu64 *)d->valid;
    const bool filtered = d->filtered != 0;
    cgu64 *allow = (cgu64 *)a.allow + d->allow_off;
    const uint64_t allow_words = d->allow_words, allow_t0 = d->allow_t0;
    const u64x2 *data = (const u64x2 *)(ggx2 *)d->data;
    cgu64 *q = (cgu64 *)a.qcodes + (size_t)qi * a.qpitch;
    const uint64_t tb = d->tile_begin;
    uint16_t *strip = a.strips + (size_t)d->list0 * 64;
    const int lane = threadIdx.x & 63;
    const uint64_t n_item = i1 - i0, w = (uint64_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t t0 = i0 + n_item * w / GBQ_WAVES, t1 = i0 + n_item * (w + 1) / GBQ_WAVES;
    if constexpr (NCH > 0) {
        auto next_live = [&](uint64_t t) {  // next tile at or after t with a live allowed row (wave-uniform)
            for (; t < t1; ++t)
                if (gbq_tile_mask(valid, allow, filtered, allow_words, allow_t0, t)) break;
            return t;
        };
        uint64_t t = next_live(t0);
        u64x2 cur[NCH], nxt[NCH];
        if (t < t1) {
            const u64x2 *rp = data + (size_t)t * NCH * 64 + lane;
#pragma unroll
            for (int c = 0; c < NCH; c++) cur[c] = rp[(size_t)c * 64];
        }
        while (t < t1) {
            const uint64_t tn = next_live(t + 1);
            if (tn < t1) {
                const u64x2 *rp = data + (size_t)tn * NCH * 64 + lane;
#pragma unroll
                for (int c = 0; c < NCH; c++) nxt[c] = rp[(size_t)c * 64];
            }
            uint32_t tot = 0;
#pragma unroll
            for (int c = 0; c < NCH; c++)
                tot += (uint32_t)__popcll(cur[c].x ^ q[2 * c]) + (uint32_t)__popcll(cur[c].y ^ q[2 * c + 1]);
            strip[(size_t)(t - tb) * 64 + lane] = (uint16_t)tot;
#pragma unroll
            for (int c = 0; c < NCH; c++) cur[c] = nxt[c];
            t = tn;
        }
    } else {
        const uint32_t nch = a.nchunks;
        for (uint64_t t = t0; t < t1; ++t) {
            if (gbq_tile_mask(valid, allow, filtered, allow_words, allow_t0, t) == 0ull) continue;  // wave-uniform
            const u64x2 *rp = data + (size_t)t * nch * 64 + lane;
            uint32_t tot = 0;
            for (uint32_t c = 0; c < nch; c++) {
                const u64x2 x = rp[(size_t)c * 64];
                tot += (uint32_t)__popcll(x.x ^ q[2 * c]) + (uint32_t)__popcll(x.y ^ q[2 * c + 1]);
            }
            strip[(size_t)(t - tb) * 64 + lane] = (uint16_t)tot;
        }
    }
}

// One workgroup per query; wave w of chunk c holds tile tile_begin + 4c + w, lane = row.
// hist[b] = live allowed rows of the earlier chunks at distance b.  v = the smallest bin
// whose cumulative count reaches R (nbins = +inf: fewer than R rows so far), cnt = the count
// at or below v (while v = nbins: every row so far); both uniform over the workgroup.
// Records: keys (ordered distance << 32 | slot), the first `head` of a query in heads
// [nq][head], the rest at their position in the query's part of rec.
__global__ __launch_bounds__(GBQ_WAVES * 64) void bq_group_filter_kernel(const GroupQuery *desc, const uint64_t *allow_blk,
                                                                         const uint16_t *strips, uint32_t R,
                                                                         uint32_t nbins, uint32_t head, uint64_t *rec,
                                                                         uint64_t *heads, uint32_t *totals)
{
    extern __shared__ uint32_t hist[];  // [nbins]
    __shared__ uint32_t wkeep[GBQ_WAVES], wle[GBQ_WAVES];
    const uint32_t qi = blockIdx.x;
    cgq *d = (cgq *)desc + qi;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (d->nlists == 0) {  // nothing live or allowed
        if (threadIdx.x == 0) totals[qi] = 0u;
        return;
    }
    cgu64 *valid = (cgu64 *)d->valid;
    const bool filtered = d->filtered != 0;
    cgu64 *allow = (cgu64 *)allow_blk + d->allow_off;
    const uint64_t allow_words = d->allow_words, allow_t0 = d->allow_t0;
    const uint64_t tb = d->tile_begin, te = d->tile_end;
    const uint16_t *strip = strips + (size_t)d->list0 * 64;
    uint64_t *rq = rec + (size_t)d->list0 * 64;
    uint64_t *hq = heads + (size_t)qi * head;
    for (uint32_t i = threadIdx.x; i < nbins; i += GBQ_WAVES * 64) hist[i] = 0u;
    __syncthreads();
    uint32_t v = nbins, cnt = 0, out = 0;
    auto find_v = [&]() {  // the first bin whose cumulative count reaches R, from scratch (every wave the same)
        uint32_t base = 0;
        v = nbins;
        for (uint32_t b0 = 0; b0 < nbins; b0 += 64) {
            const uint32_t b = b0 + (uint32_t)lane;
            uint32_t c = b < nbins ? hist[b] : 0u;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {  // inclusive prefix sum over the 64 lanes
                const uint32_t o = (uint32_t)__shfl_up((int)c, off, 64);
                if (lane >= off) c += o;
            }
            const uint64_t hit = __ballot(base + c >= R);
            if (hit) {
                const int l = __builtin_ctzll(hit);
                v = b0 + (uint32_t)l;
                cnt = base + (uint32_t)__shfl((int)c, l, 64);
                return;
            }
            base += (uint32_t)__shfl((int)c, 63, 64);
        }
        cnt = base;
    };
    const uint64_t nchunk = (te - tb + GBQ_WAVES - 1) / GBQ_WAVES;
    auto load = [&](uint64_t c, uint64_t &m, uint32_t &dd) {
        const uint64_t t = tb + c * GBQ_WAVES + (uint64_t)wave;
        m = t < te ? gbq_tile_mask(valid, allow, filtered, allow_words, allow_t0, t) : 0ull;
        dd = m ? (uint32_t)strip[(size_t)(t - tb) * 64 + lane] : 0u;  // dead tiles were never written
    };
    uint64_t m = 0, mn = 0;
    uint32_t dist = 0, dn = 0;
    load(0, m, dist);
    for (uint64_t c = 0; c < nchunk; c++) {
        if (c + 1 < nchunk) load(c + 1, mn, dn);  // the next chunk's words while this one is counted
        dist = min(dist, nbins - 1);
        const bool live = (m >> lane) & 1ull;
        const bool keep = live && dist < v;  // v = nbins: every live row
        const uint64_t kb = __ballot(keep), lb = __ballot(live && dist <= v);
        if (live) atomicAdd(&hist[dist], 1u);
        if (lane == 0) {
            wkeep[wave] = (uint32_t)__popcll(kb);
            wle[wave] = (uint32_t)__popcll(lb);
        }
        __syncthreads();
        uint32_t before = 0, kt = 0, lt = 0;
#pragma unroll
        for (int w = 0; w < GBQ_WAVES; w++) {
            const uint32_t kw = wkeep[w];
            before += w < wave ? kw : 0u;
            kt += kw;
            lt += wle[w];
        }
        if (keep) {
            const uint32_t pos = out + before +
                                 __builtin_amdgcn_mbcnt_hi((uint32_t)(kb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kb, 0u));
            const uint32_t slot = (uint32_t)((tb + c * GBQ_WAVES + (uint64_t)wave) * 64 + (uint64_t)lane);
            const uint64_t key = wvg_make_key((float)dist, slot);
            if (pos < head) hq[pos] = key;
            else rq[pos] = key;
        }
        out += kt;
        cnt += lt;
        if (v == nbins) {
            if (cnt >= R) find_v();
        } else {
            while (v > 0 && cnt - hist[v] >= R) {  // (uniform: every lane reads the same words)
                cnt -= hist[v];
                --v;
            }
        }
        __syncthreads();  // the next chunk's atomics and counts after every read of this one's
        m = mn;
        dist = dn;
    }
    if (threadIdx.x == 0) totals[qi] = out;
}

// Exact distances of the popped candidates (the rescore loop, V/flat/index.go:375-385):
// cand[j] = query << 32 | slot, each query's run padded to a multiple of 64 with GBQ_PAD
// slots, so a workgroup serves one query; out[j] = the ordered distance bits.
template <int METRIC>
__global__ __launch_bounds__(64) void rescore_group_kernel(int metric, const float4 *q4, uint32_t qpitch,
                                                           const void *const *fdata, uint32_t dim, uint32_t nchunks,
                                                           const uint64_t *cand, uint32_t *out, int o512)
{
    const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
    const uint64_t e = cand[j];
    const uint32_t qi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(e >> 32));
    const uint32_t slot = (uint32_t)e;
    uint32_t res = 0xFFFFFFFFu;
    if (slot != GBQ_PAD) {
        const float4 *tiled = (const float4 *)fdata[qi];
        const float4 *rp = tiled + ((size_t)(slot >> 6) * nchunks) * 64 + (slot & 63);
        const float4 *q = q4 + (size_t)qi * (qpitch / 4);
        res = wvg_ord_f32(wrap_metric(metric, row_dist<METRIC, 64>(rp, q, (int)dim, o512)));
    }
    out[j] = res;
}

static hipError_t launch_scan_bq_group(const GroupBqArgs &a, uint32_t nitems, hipStream_t s)
{
    if (nitems == 0) return hipSuccess;
    dim3 grid(nitems), block(GBQ_WAVES * 64);
    switch (a.nchunks) {  // K5's chunk counts (launch_bq_ec, wvg_bq.hip)
    case 1: launch_timed((scan_bq_group_kernel<1>), grid, block, 0, s, a); break;    // d <= 128
    case 6: launch_timed((scan_bq_group_kernel<6>), grid, block, 0, s, a); break;    // d = 768
    case 12: launch_timed((scan_bq_group_kernel<12>), grid, block, 0, s, a); break;  // d = 1536
    default: launch_timed((scan_bq_group_kernel<0>), grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}

constexpr uint32_t GBQ_MAX_DIM = 8192;  // the filter's histogram: dim + 1 bins of LDS, 32 KiB

static hipError_t launch_bq_group_filter(const GroupBqArgs &a, uint32_t nq, uint32_t R, uint32_t head, uint64_t *rec,
                                         uint64_t *heads, uint32_t *totals, hipStream_t s)
{
    const uint32_t nbins = 128u * a.nchunks + 1;  // distances are 0 .. 128 * nchunks (padding bits are equal)
    hipLaunchKernelGGL(bq_group_filter_kernel, dim3(nq), dim3(GBQ_WAVES * 64), (size_t)nbins * 4, s, a.desc, a.allow,
                       a.strips, R, nbins, head, rec, heads, totals);
    return hipGetLastError();
}

static hipError_t launch_rescore_group(int metric, const float *q, uint32_t qpitch, const void *const *fdata,
                                       uint32_t dim, uint32_t nchunks, const uint64_t *cand, uint64_t ncand,
                                       uint32_t *out, int o512, hipStream_t s)
{
    if (ncand == 0) return hipSuccess;
    with_metric(metric, [&](auto M) {
        hipLaunchKernelGGL((rescore_group_kernel<decltype(M)::value>), dim3((unsigned)(ncand / 64)), dim3(64), 0, s,
                           metric, reinterpret_cast<const float4 *>(q), qpitch, fdata, dim, nchunks, cand, out, o512);
    });
    return hipGetLastError();
}

// Records per query copied back with the totals.  The filter keeps about
// R (1 + ln(n / R)) x 1.1 rows of an n-row tenant (1086 of 10k at
// R = 200), so 8 R covers tenants up to ~500 R rows in the first round; never more than
// the largest window, and the block stays within 32 MiB.
static uint32_t group_bq_head(uint32_t nq, uint32_t R, uint64_t max_rows)
{
    uint64_t h = std::max<uint64_t>(1024, 8ull * R);
    h = std::min(h, max_rows);
    h = std::min<uint64_t>(h, ((uint64_t)32 << 20) / 8 / nq);
    return (uint32_t)std::max<uint64_t>(h, 64);
}

// f(0) .. f(nq - 1), the queries' independent host work: on the host pool from four queries on
// (waking the pool costs about what one query's replay does, so fewer run on the caller).
static void for_queries(uint32_t nq, const std::function<void(uint32_t)> &f)
{
    if (nq >= 4) return parallel_for(nq, f);
    for (uint32_t i = 0; i < nq; i++) f(i);
}

// Both entry points: f32 null = the candidates themselves ([nq][R], pop order).
static int group_bq_flow(wvg_corpus *const *bq, wvg_corpus *const *f32, const float *queries, uint32_t nq, uint32_t k,
                         uint32_t R, const uint64_t *const *allow_bits, const uint64_t *allow_words, uint64_t *out_ids,
                         float *out_dists, uint32_t *out_counts)
{
    if (nq == 0) return WVG_OK;
    if (!bq) return fail(WVG_ERR_INVALID, "null bq corpora");
    if (!queries) return fail(WVG_ERR_INVALID, "null queries");
    for (uint32_t i = 0; i < nq; i++) {
        const wvg_corpus *c = bq[i], *c0 = bq[0];
        const std::string at = "bq[" + std::to_string(i) + "]";
        if (!c || !c->ctx) return fail(WVG_ERR_INVALID, at + " is null");
        if (c->ctx != c0->ctx) return fail(WVG_ERR_INVALID, at + " belongs to another context than bq[0]");
        if (c->kind != WVG_KIND_BQ) return fail(WVG_ERR_INVALID, at + " is not a BQ corpus");
        if (c->dim != c0->dim) return fail(WVG_ERR_INVALID, at + " differs from bq[0] in dim");
        if (c->metric != c0->metric) return fail(WVG_ERR_INVALID, at + " differs from bq[0] in metric");
        if (tiles_of(c->high_water) * 64 > 0xFFFFFFFFull) return fail(WVG_ERR_UNSUPPORTED, at + " holds too many rows");
        if (f32) {
            const wvg_corpus *f = f32[i];
            const std::string fat = "f32[" + std::to_string(i) + "]";
            if (!f || !f->ctx) return fail(WVG_ERR_INVALID, fat + " is null");
            if (f->ctx != c0->ctx) return fail(WVG_ERR_INVALID, fat + " belongs to another context than bq[0]");
            if (f->kind != WVG_KIND_F32) return fail(WVG_ERR_INVALID, fat + " is not an F32 corpus");
            if (f->dim != c0->dim) return fail(WVG_ERR_INVALID, fat + " differs from bq[0] in dim");
            if (f->metric != c0->metric) return fail(WVG_ERR_INVALID, fat + " differs from bq[0] in metric");
            if (f->id_base != c->id_base) return fail(WVG_ERR_INVALID, fat + " differs from " + at + " in id_base");
            if (f->capacity < tiles_of(c->high_water) * 64)  // the rescore reads the candidates' slots of f
                return fail(WVG_ERR_INVALID, fat + " holds fewer rows than " + at);
        }
        if (allow_bits && allow_bits[i] && !allow_words)
            return fail(WVG_ERR_INVALID, "allow_bits[" + std::to_string(i) + "] without allow_words");
    }
    wvg_corpus *c0 = bq[0];
    wvg_ctx *ctx = c0->ctx;
    if (!ctx->opt.heap_replay)
        return fail(WVG_ERR_UNSUPPORTED, "grouped BQ search returns the reference heap's result only (heap_replay = 0)");
    if (c0->dim > GBQ_MAX_DIM) return fail(WVG_ERR_UNSUPPORTED, "grouped BQ search: dim above 8192");
    WVG_HIP(hipSetDevice(ctx->device));

    // Shared locks of the distinct corpora, BQ and F32 together, in ascending address
    // order (wvg_search_group: one global order cannot deadlock against waiting writers),
    // held until the results are on the host.
    std::vector<wvg_corpus *> uniq(bq, bq + nq);
    if (f32) uniq.insert(uniq.end(), f32, f32 + nq);
    std::sort(uniq.begin(), uniq.end(), std::less<wvg_corpus *>());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    std::vector<std::shared_lock<std::shared_mutex>> locks;
    locks.reserve(uniq.size());
    for (wvg_corpus *c : uniq) locks.emplace_back(c->rw);

    const uint32_t W = f32 ? k : R;  // output width
    if (W == 0 || R == 0) {          // counts 0, nothing else to write
        write_empty(nq, 0, out_ids, out_dists, out_counts);
        return WVG_OK;
    }

    // the plan: per query its tile range and allow window (wvg_search_group's), then the items
    std::vector<GroupQuery> desc(nq);
    std::vector<const uint64_t *> win(nq, nullptr);
    uint64_t total_tiles = 0, allow_total = 0, max_rows = 0, cand_cap = 0;
    for (uint32_t i = 0; i < nq; i++) {
        const wvg_corpus *c = bq[i];
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
        max_rows = std::max(max_rows, (te - tb) * 64);
        cand_cap += align_up(std::min<uint64_t>(R, (te - tb) * 64), 64);
    }
    if (total_tiles == 0) {
        write_empty(nq, W, out_ids, out_dists, out_counts);
        return WVG_OK;
    }
    if (total_tiles > 0x7FFFFFFFull) return fail(WVG_ERR_UNSUPPORTED, "grouped BQ search: too many rows in one call");
    const uint64_t T = group_item_tiles(total_tiles, ctx->num_cus);
    uint64_t nitems64 = 0, tile_at = 0;
    for (uint32_t i = 0; i < nq; i++) {
        GroupQuery &d = desc[i];
        const uint64_t n = d.tile_end - d.tile_begin;
        d.list0 = (uint32_t)tile_at;  // the query's first tile in the strips and the records
        d.nlists = (uint32_t)((n + T - 1) / T);
        tile_at += n;
        nitems64 += d.nlists;
    }
    const uint32_t nitems = (uint32_t)nitems64;
    const uint32_t head = group_bq_head(nq, R, max_rows);

    SlotGuard g(ctx);
    int rc = ctx->acquire(&g.slot);
    if (rc) return rc;
    const uint32_t qpb = bq_chunks(c0->dim) * 2, qpf = f32_chunks(c0->dim) * 4;
    // the input block [query codes | float queries | descriptors | items | allow windows | float row pointers]
    Carver in;
    const size_t i_qb = in.take((size_t)nq * qpb * 8);
    const size_t i_qf = in.take(f32 ? (size_t)nq * qpf * 4 : 0);
    const size_t i_desc = in.take((size_t)nq * sizeof(GroupQuery));
    const size_t i_items = in.take((size_t)nitems * sizeof(GroupItem));
    const size_t i_allow = in.take((size_t)allow_total * 8);
    const size_t i_fdata = in.take(f32 ? (size_t)nq * sizeof(void *) : 0);
    const size_t in_b = in.off;
    const size_t tot_b = align_up((size_t)nq * 4, 256), back_b = tot_b + (size_t)nq * head * 8;
    const size_t cand_b = f32 ? (size_t)cand_cap * 8 : 0, resc_b = f32 ? (size_t)cand_cap * 4 : 0;
    Carver cv;
    const size_t o_in = cv.take(in_b);
    const size_t o_strip = cv.take((size_t)total_tiles * 64 * 2);
    const size_t o_rec = cv.take((size_t)total_tiles * 64 * 8);
    const size_t o_back = cv.take(back_b);  // totals [nq], then the heads [nq][head]
    const size_t o_cand = cv.take(cand_b);
    const size_t o_resc = cv.take(resc_b);
    void *base = nullptr;
    rc = g.slot->device_scratch(cv.off, &base);
    if (rc) return rc;
    char *b = (char *)base;
    hipStream_t s = g.slot->stream;
    // pinned staging, reserved whole before the first copy; pieces above STAGE_MAX stay pageable
    Staging st;
    rc = st.reserve(g.slot, align_up(in_b, 64) + stage_bytes(back_b) + stage_bytes(cand_b) + stage_bytes(resc_b));
    if (rc) return rc;
    char *hin = st.take(in_b);
    std::vector<char> big_back(back_b > STAGE_MAX ? back_b : 0), big_cand(cand_b > STAGE_MAX ? cand_b : 0),
        big_resc(resc_b > STAGE_MAX ? resc_b : 0);
    char *hback = back_b <= STAGE_MAX ? st.take(back_b) : big_back.data();
    char *hcand = cand_b <= STAGE_MAX ? st.take(cand_b) : big_cand.data();
    char *hresc = resc_b <= STAGE_MAX ? st.take(resc_b) : big_resc.data();

    {
        std::vector<float> qf;
        std::vector<uint64_t> qb;
        uint32_t qp = 0;
        prepare_queries_host(c0, queries, nq, qf, qb, qp);  // the query codes (normalized first for cosine)
        std::memcpy(hin + i_qb, qb.data(), (size_t)nq * qpb * 8);
        if (f32) {
            prepare_queries_host(f32[0], queries, nq, qf, qb, qp);
            std::memcpy(hin + i_qf, qf.data(), (size_t)nq * qpf * 4);
        }
    }
    GroupItem *items = reinterpret_cast<GroupItem *>(hin + i_items);
    for (uint32_t i = 0, at = 0; i < nq; i++) {
        const GroupQuery &d = desc[i];
        const uint64_t n = d.tile_end - d.tile_begin;
        for (uint32_t r = 0; r < d.nlists; r++, at++)
            items[at] = GroupItem{i, r, (uint32_t)(d.tile_begin + n * r / d.nlists),
                                  (uint32_t)(d.tile_begin + n * (r + 1) / d.nlists)};
        if (win[i]) std::memcpy(hin + i_allow + d.allow_off * 8, win[i], d.allow_words * 8);
        if (f32) reinterpret_cast<const void **>(hin + i_fdata)[i] = f32[i]->d_data;
    }
    std::memcpy(hin + i_desc, desc.data(), (size_t)nq * sizeof(GroupQuery));

    WVG_HIP(hipMemcpyAsync(b + o_in, hin, in_b, hipMemcpyHostToDevice, s));
    GroupBqArgs a{};
    a.desc = reinterpret_cast<const GroupQuery *>(b + o_in + i_desc);
    a.items = reinterpret_cast<const GroupItem *>(b + o_in + i_items);
    a.qcodes = reinterpret_cast<const uint64_t *>(b + o_in + i_qb);
    a.allow = reinterpret_cast<const uint64_t *>(b + o_in + i_allow);
    a.strips = reinterpret_cast<uint16_t *>(b + o_strip);
    a.qpitch = qpb;
    a.nchunks = c0->nchunks;
    {
        ProfArm arm(ctx);  // wvg_profile_*: the scan dispatch's own events
        if (arm.rc) return arm.rc;
        WVG_HIP(launch_scan_bq_group(a, nitems, s));
    }
    WVG_HIP(launch_bq_group_filter(a, nq, R, head, (uint64_t *)(b + o_rec), (uint64_t *)(b + o_back + tot_b),
                                   (uint32_t *)(b + o_back), s));
    WVG_HIP(hipMemcpyAsync(hback, b + o_back, back_b, hipMemcpyDeviceToHost, s));
    WVG_HIP(hipStreamSynchronize(s));
    const uint32_t *tot = reinterpret_cast<const uint32_t *>(hback);
    const uint64_t *heads = reinterpret_cast<const uint64_t *>(hback + tot_b);
    // queries whose records exceed the head: the rest of each in one more round
    std::vector<uint64_t> rest_at(nq, 0);
    uint64_t rest_n = 0;
    for (uint32_t i = 0; i < nq; i++) {
        if ((uint64_t)tot[i] > (desc[i].tile_end - desc[i].tile_begin) * 64)
            return fail(WVG_ERR_DEVICE, "grouped BQ search: record count beyond the window");
        rest_at[i] = rest_n;
        if (tot[i] > head) rest_n += tot[i] - head;
    }
    std::vector<uint64_t> rest(rest_n);
    if (rest_n) {
        for (uint32_t i = 0; i < nq; i++)
            if (tot[i] > head)
                WVG_HIP(hipMemcpyAsync(rest.data() + rest_at[i], b + o_rec + ((size_t)desc[i].list0 * 64 + head) * 8,
                                       (size_t)(tot[i] - head) * 8, hipMemcpyDeviceToHost, s));
        WVG_HIP(hipStreamSynchronize(s));
    }
    std::vector<std::vector<GoItem>> pops(nq);
    // findTopVectorsCached into a heap of R and the pop loop, per query: ~1.1k heap operations
    // each (36 us on one host core at R = 200), the call's longest serial part, so on the pool
    for_queries(nq, [&](uint32_t i) {
        const uint32_t n = tot[i];
        std::vector<GoItem> rows(n);
        for (uint32_t j = 0; j < n; j++) {
            const uint64_t key = j < head ? heads[(size_t)i * head + j] : rest[rest_at[i] + (j - head)];
            rows[j] = GoItem{(uint32_t)key, wvg_unord_f32((uint32_t)(key >> 32))};
        }
        replay_rows(rows.data(), n, R, pops[i]);
    });
    if (!f32) {  // the candidates themselves, in pop order
        for (uint32_t q = 0; q < nq; q++) {
            const std::vector<GoItem> &v = pops[q];
            for (uint32_t i = 0; i < R; i++) {
                const bool has = i < v.size();
                if (out_ids) out_ids[(size_t)q * R + i] = has ? bq[q]->id_base + v[i].id : WVG_KEY_NONE;
                if (out_dists) out_dists[(size_t)q * R + i] = has ? v[i].dist : INFINITY;
            }
            if (out_counts) out_counts[q] = (uint32_t)v.size();
        }
        return WVG_OK;
    }
    // the rescore loop (index.go:368-385): exact distances of the popped slots on the
    // device, inserted into a heap of k in pop order on the host
    uint64_t *ck = reinterpret_cast<uint64_t *>(hcand);
    std::vector<uint64_t> cand_at(nq, 0);
    uint64_t ncand = 0;
    for (uint32_t q = 0; q < nq; q++) {
        cand_at[q] = ncand;
        for (const GoItem &it : pops[q]) ck[ncand++] = ((uint64_t)q << 32) | (uint32_t)it.id;
        while (ncand % 64) ck[ncand++] = ((uint64_t)q << 32) | GBQ_PAD;
    }
    if (ncand > cand_cap) return fail(WVG_ERR_DEVICE, "grouped BQ search: more candidates than planned");
    const uint32_t *resc = reinterpret_cast<const uint32_t *>(hresc);
    if (ncand) {
        WVG_HIP(hipMemcpyAsync(b + o_cand, ck, (size_t)ncand * 8, hipMemcpyHostToDevice, s));
        WVG_HIP(launch_rescore_group(c0->metric, (const float *)(b + o_in + i_qf), qpf,
                                     (const void *const *)(b + o_in + i_fdata), c0->dim, f32[0]->nchunks,
                                     (const uint64_t *)(b + o_cand), ncand, (uint32_t *)(b + o_resc), ctx->order512, s));
        WVG_HIP(hipMemcpyAsync(hresc, b + o_resc, (size_t)ncand * 4, hipMemcpyDeviceToHost, s));
        WVG_HIP(hipStreamSynchronize(s));
    }
    for_queries(nq, [&](uint32_t q) {
        std::vector<uint64_t> ids(std::min<size_t>(k, pops[q].size()));
        std::vector<float> dists(ids.size());
        GoMaxHeap h(ids.size());
        for (size_t i = 0; i < pops[q].size(); i++)
            insert_to_heap(h, k, bq[q]->id_base + pops[q][i].id, wvg_unord_f32(resc[cand_at[q] + i]));
        const size_t cnt = extract_heap(h, ids.data(), dists.data());
        for (uint32_t i = 0; i < k; i++) {
            if (out_ids) out_ids[(size_t)q * k + i] = i < cnt ? ids[i] : WVG_KEY_NONE;
            if (out_dists) out_dists[(size_t)q * k + i] = i < cnt ? dists[i] : INFINITY;
        }
        if (out_counts) out_counts[q] = (uint32_t)cnt;
    });
    return WVG_OK;
}

}  // namespace wvg

using namespace wvg;

extern "C" {

int wvg_search_group_bq_rescore(wvg_corpus *const *bq, wvg_corpus *const *f32, const float *queries, uint32_t nq,
                                uint32_t k, uint32_t rescore_limit, const uint64_t *const *allow_bits,
                                const uint64_t *allow_words, uint64_t *out_ids, float *out_dists, uint32_t *out_counts)
{
    if (nq == 0) return WVG_OK;
    if (!f32) return fail(WVG_ERR_INVALID, "null f32 corpora");
    const uint32_t R = std::max(rescore_limit, k);  // searchTimeRescore (V/flat/index.go:297-305)
    return group_bq_flow(bq, f32, queries, nq, k, R, allow_bits, allow_words, out_ids, out_dists, out_counts);
}

int wvg_search_group_bq_candidates(wvg_corpus *const *bq, const float *queries, uint32_t nq, uint32_t rescore_limit,
                                   const uint64_t *const *allow_bits, const uint64_t *allow_words, uint64_t *out_ids,
                                   float *out_dists, uint32_t *out_counts)
{
    return group_bq_flow(bq, nullptr, queries, nq, rescore_limit, rescore_limit, allow_bits, allow_words, out_ids,
                         out_dists, out_counts);
}

}  // extern "C"

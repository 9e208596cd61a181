// srl_color_cloud.hip -- the colour voxel map's product on the device for gfx950: the coloured cloud of lioOptimization::pubColorPoints
// (src/lioOptimization.cpp:1210-1241), threadPubColorPoints (:1243-1344) and saveColorPoints (:1386-1426).  All three walk the registered
// list, leave out a point iff N_rgb < pub_point_minimum_views and pack position and colour of the others into a pcl::PointXYZRGB; they
// differ in the range and the direction of the walk.  A filter and a pack over state that already lies in HBM: a deterministic function of
// the stored position, N_rgb and rgb (and, for the `since` option, last_observe_time), bit for bit and reproducible.
//
//   k_cloud_flags   range element e is registered index first + e, or first + n - 1 - e walking down: registered entry -> pool position
//                   -> N_rgb, and last_observe_time only where `since` can leave a point out; writes the flag word.  The two counters
//                   (below the views, stale) leave through srl_wg_totals (srl_wg_totals.h).  A workgroup is 1 024 threads with one
//                   element each up to 131 072 elements and eight each beyond: the ticket is an atomic on one address at agent scope
//                   and costs about 30 ns per workgroup, one after the other ("Cost of the cloud export")
//   k_scan_small    the flags in walk order (srl_scan: one, two or three levels); the sink gathers the kept point's 12 position bytes and
//                   6 colour bytes and writes the record as ONE 16-byte store, and its registered index.  The two-level gather is the
//                   sink's, not the scan's input: in the one-launch regime the scan re-reads everything in front of its tile
// A map never rendered has no colour state: the kernels take a null state pointer for "N_rgb 0, colour 0, time 0" and nothing is allocated.
#include "srl_ctx.h"
#include "srl_color_map.h"
#include "srl_frame_scratch.h"

#include <cmath>
#include <cstring>
#include <limits>

static_assert(sizeof(srl_color_cloud_point) == 16, "srl_color_cloud_point is 16 bytes on both sides of the C-ABI: x y z and the rgb word");
static_assert(sizeof(srl_color_cloud_opts) == 16 && sizeof(srl_color_cloud_totals) == 32, "options and totals of the cloud export");

namespace {

enum { CC_BELOW, CC_STALE, CC_N };
#define SRL_CTOT_PUBLISHED 4            // (an int behind the two totals and the ticket; the scan's sink writes it on every call)
#define SRL_CTOT_BYTES 64
#define SRL_CLOUD_ITEMS 8
#define SRL_CLOUD_STAGE_BYTES ((size_t)1 << 20)

struct CloudWalk {
    const int *reg;                      // registered list: pool position per point_index
    long long first;
    int n, reverse;
    __device__ __forceinline__ long long index(int e) const { return reverse ? first + (long long)(n - 1 - e) : first + (long long)e; }
};

// workgroup b owns elements [b BLOCK ITEMS, (b + 1) BLOCK ITEMS): ITEMS coalesced rounds of BLOCK elements
template <int BLOCK, int ITEMS>
__global__ void __launch_bounds__(BLOCK) k_cloud_flags(CloudWalk W, const SrlColorState *state, int minimum_views, int use_since, double since, int *flags,
                                                       unsigned long long *cpart, unsigned long long *ctot) {
    unsigned c[CC_N] = {0, 0};
#pragma unroll
    for (int u = 0; u < ITEMS; u++) {
        const long long e64 = (long long)blockIdx.x * (BLOCK * ITEMS) + u * BLOCK + threadIdx.x;
        if (e64 < W.n) {
            const int e = (int)e64;
            int n_rgb = 0;
            long long p = 0;
            if (state) { p = W.reg[W.index(e)]; n_rgb = state[p].n_rgb; }
            int keep = 1;
            if (n_rgb < minimum_views) {                                      // :1221, :1281, :1404
                c[CC_BELOW]++; keep = 0;
            } else if (use_since) {
                const double t = state ? state[p].last_observe_time : 0.0;
                if (t < since) { c[CC_STALE]++; keep = 0; }
            }
            flags[e] = keep;
        }
    }
    srl_wg_totals<CC_N, BLOCK>(c, cpart, ctot);
}

struct CloudRecordSink {
    CloudWalk W;
    const SrlColorPoint *pool;
    const SrlColorState *state;
    uint4 *out;                          // srl_color_cloud_point, written whole
    int *index_out;                      // or null
    int *published;
    __device__ void operator()(int e, int keep, int excl) const {
        if (keep) {
            const long long i = W.index(e);
            const int p = W.reg[i];
            const SrlColorPoint &pt = pool[p];
            // b, g, r, a from the low byte: r = (uint8_t) rgb[2], g = (uint8_t) rgb[1], b = (uint8_t) rgb[0] (:1228-1230); a = 255
            unsigned word = 0xFF000000u;
            if (state) {
                const short *c = state[p].rgb;
                word |= ((unsigned)c[0] & 0xFFu) | (((unsigned)c[1] & 0xFFu) << 8) | (((unsigned)c[2] & 0xFFu) << 16);
            }
            out[excl] = make_uint4(__float_as_uint(pt.x), __float_as_uint(pt.y), __float_as_uint(pt.z), word);
            if (index_out) index_out[excl] = (int)i;
        }
        if (e == W.n - 1) *published = excl + keep;
    }
};

}  // namespace

extern "C" void srl_color_cloud_opts_default(srl_color_cloud_opts *o) {
    if (!o) return;
    o->minimum_views = 1;                  // config/r3live.yaml:76 (the class default, parameters.h:106, is 3)
    o->reverse = 0;
    o->since = -std::numeric_limits<double>::infinity();
}

extern "C" int srl_color_map_export_cloud(srl_ctx *ctx, int64_t first, int64_t count, const srl_color_cloud_opts *opts, srl_color_cloud_point *out,
                                          int32_t *point_index, int64_t capacity, srl_color_cloud_totals *totals) {
    if (totals) std::memset(totals, 0, sizeof *totals);
    if (!ctx || !opts || first < 0 || capacity < 0 || std::isnan(opts->since)) return SRL_ERR_BAD_ARG;
    { const int rc = srl_color_need_map_one_rank(ctx); if (rc) return rc; }
    SrlColorMap *cm = ctx->color;
    if (first > cm->num_registered || (count >= 0 && count > cm->num_registered - first)) { ctx->err = "cloud: the range ends beyond the registered list"; return SRL_ERR_BAD_ARG; }
    if (count < 0) count = cm->num_registered - first;      // to the end of the list as it is now
    if (count > (int64_t)1 << 27) { ctx->err = "cloud: a range of more than 2^27 points (export it in pieces)"; return SRL_ERR_UNSUPPORTED; }
    SRL_DISARM(ctx);                      // a waiting launch holds a workgroup on every compute unit
    if (count == 0) return SRL_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    const int n = (int)count;
    const bool want_index = point_index != nullptr;
    const double since = opts->since;
    const int use_since = since > -std::numeric_limits<double>::infinity() ? 1 : 0;      // at -inf no time lies below it: the word is not read
    const CloudWalk W = {cm->d_reg, (long long)first, n, opts->reverse ? 1 : 0};
    const int items = n <= SRL_SCAN_SMALL_MAX ? 1 : SRL_CLOUD_ITEMS;      // elements per thread (see k_cloud_flags above)
    const unsigned nblocks = (unsigned)(((long long)n + 1024 * items - 1) / (1024 * items));

    { const int rc = srl_wg_totals_reserve(ctx, cm->cloud_tot, SRL_CTOT_BYTES / 8, CC_N, nblocks); if (rc) return rc; }
    DevBuf b_flag, b_sc, b_out, b_idx;
    HIPCHK(ctx, b_flag.alloc(ctx, (size_t)n * sizeof(int)));
    HIPCHK(ctx, b_sc.alloc(ctx, srl_scan_scratch_ints(n) * 4));
    HIPCHK(ctx, b_out.alloc(ctx, (size_t)n * sizeof(srl_color_cloud_point)));
    if (want_index) HIPCHK(ctx, b_idx.alloc(ctx, (size_t)n * sizeof(int)));
    unsigned long long *ctot = cm->cloud_tot.d_tot, *cpart = cm->cloud_tot.d_rows;
    int *published_d = reinterpret_cast<int *>(ctot + SRL_CTOT_PUBLISHED);
    if (items == 1)
        hipLaunchKernelGGL((k_cloud_flags<1024, 1>), dim3(nblocks), dim3(1024), 0, st, W, (const SrlColorState *)cm->d_state, (int)opts->minimum_views, use_since,
                           since, b_flag.as<int>(), cpart, ctot);
    else
        hipLaunchKernelGGL((k_cloud_flags<1024, SRL_CLOUD_ITEMS>), dim3(nblocks), dim3(1024), 0, st, W, (const SrlColorState *)cm->d_state, (int)opts->minimum_views,
                           use_since, since, b_flag.as<int>(), cpart, ctot);
    HIPCHK(ctx, hipGetLastError());
    srl_scan(SrlIntArrayIn{b_flag.as<int>()},
             CloudRecordSink{W, cm->d_pool, cm->d_state, b_out.as<uint4>(), want_index ? b_idx.as<int>() : nullptr, published_d}, n, b_sc.as<int>(), st);
    HIPCHK(ctx, hipGetLastError());

    // one wait for the totals, then one DMA of exactly `published` records (and one of as many indices)
    { const int rc = ensure_host_scratch(ctx, SRL_CTOT_BYTES); if (rc) return rc; }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch, ctot, SRL_CTOT_BYTES, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    unsigned long long h_tot[CC_N];
    int h_pub = 0;
    std::memcpy(h_tot, ctx->h_scratch, sizeof h_tot);
    std::memcpy(&h_pub, ctx->h_scratch + 8 * SRL_CTOT_PUBLISHED, sizeof h_pub);
    const int64_t published = h_pub;
    if (totals) {
        totals->scanned = n; totals->published = published;
        totals->below_views = (int64_t)h_tot[CC_BELOW]; totals->stale = (int64_t)h_tot[CC_STALE];
    }
    if (published < 0 || published + (int64_t)h_tot[CC_BELOW] + (int64_t)h_tot[CC_STALE] != (int64_t)n) { ctx->err = "cloud: the counters do not add up (internal)"; return SRL_ERR_HIP; }
    if ((!out && !want_index) || published == 0) return SRL_OK;
    if (capacity < published) { ctx->err = "cloud: capacity below the number of published points (totals->published)"; return SRL_ERR_BAD_ARG; }
    const size_t rec_bytes = out ? (size_t)published * sizeof(srl_color_cloud_point) : 0, idx_bytes = want_index ? (size_t)published * sizeof(int32_t) : 0;
    // a small cloud leaves through the page-locked scratch and a host copy; a larger one goes straight to the caller, as the reports of
    // bulk loads do.  Measured: 0.4 MB 70 us staged against 72 straight, 4 MB 315 against 137, 19 MB 1 350 against 498
    const bool staged = rec_bytes + idx_bytes <= SRL_CLOUD_STAGE_BYTES;
    if (staged) { const int rc = ensure_host_scratch(ctx, rec_bytes + idx_bytes); if (rc) return rc; }
    if (out) HIPCHK(ctx, hipMemcpyAsync(staged ? (void *)ctx->h_scratch : (void *)out, b_out.p, rec_bytes, hipMemcpyDeviceToHost, st));
    if (want_index) HIPCHK(ctx, hipMemcpyAsync(staged ? (void *)(ctx->h_scratch + rec_bytes) : (void *)point_index, b_idx.p, idx_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (staged) {
        if (out) std::memcpy(out, ctx->h_scratch, rec_bytes);
        if (want_index) std::memcpy(point_index, ctx->h_scratch + rec_bytes, idx_bytes);
    }
    return SRL_OK;
}

// srl_color_select.hip -- the colour voxel map's second consumer on the device for gfx950: rgbMapTracker::selectPointsForProjection
// (src/rgbMapTracker.cpp:45-152), called through refreshPointsForProjection (:26-43).  The candidates -- the last point of every listed
// voxel, or the whole registered list -- are projected (project3dPointInThisImage, shared with the render: srl_color_project.h), and one
// point per coarse image cell survives: the loop keeps `(float) depth` of a cell's last setter and candidate i takes the cell iff the cell
// is empty or (double) stored > depth_i.
//
// The loop is a function of ranks.  f(d) = (float) d is monotone, so the stored value in front of candidate i is the minimum of f over the
// cell's earlier candidates; with M the minimum of f over the whole cell
//     the holder is the LAST i with d_i < (double) M if there is one, otherwise the FIRST i with f(d_i) == M
// (the first candidate with f == M always sets; after it the cell holds M and exactly the candidates below M set).  Depths are >= 0, so
// float bit patterns order like unsigned integers: three integer atomics per cell and no sort.
//
//   k_select_tails   one thread per pool point appended since the last selection: a point in its voxel's highest slot files its position
//                    as the voxel's tail (points.back()); the layout has no such word and the insertion stays as it is
//   k_select_lookup  list mode, one thread per list entry: voxel -> tail position, or -1 for a key the map does not hold; the scan behind
//                    it compacts the known entries: candidate i is the i-th KNOWN entry (the reference's empty block takes no index)
//   k_select_cells   (a) one thread per participating candidate (i % skip_step == 0): depth, the two depth tests, the projection, the
//                    cell key; the cell is found or claimed in an epoch-tagged table that is never cleared (srl_frame_scratch.h) and its
//                    float minimum lowered.  The minimum only falls: the word is read first and the atomic issued only where it would
//                    change it.  The four counters leave through srl_wg_totals (srl_wg_totals.h)
//   k_select_file    (b) candidates with f(d) == M file their index: atomicMax among d < M, atomicMin among the others
//   k_scan_small     (c) the holder flag in index order; the sink writes the records
// The companion words are {0xFFFFFFFF - call counter, value} and only ever lowered: a word of an earlier call loses against the first
// write of this one, nothing is reset per call.
#include "srl_ctx.h"
#include "srl_color_map.h"
#include "srl_color_project.h"
#include "srl_frame_scratch.h"
#include "srl_hash.h"

#include <algorithm>
#include <cmath>
#include <cstring>

static_assert(sizeof(srl_color_selected) == 32, "srl_color_selected is 32 bytes on both sides of the C-ABI");

namespace {

#define SRL_SEL_NONE 0xFFFFFFFFu
enum { SC_FAR, SC_NEAR, SC_BEHIND, SC_OUTSIDE, SC_N };

struct SelectArgs {
    SrlCamArgs C;
    double min_dis, min_depth, max_depth;
    long long base_u, base_v, span_v;      // cell = (u - base_u) * span_v + (v - base_v): below 2^45 for every accepted image and margin
    int skip;
    int m_hi;                              // participating candidates the host can bound (the grid); the device knows the number
};

__global__ void k_select_tails(long long first, long long P, const SrlColorPoint *pool, const SrlColorVoxel *vox, int *tail) {
    const long long p = first + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const SrlColorPoint pt = pool[p];
    if ((unsigned)pt.slot + 1u == vox[pt.voxel].count) tail[pt.voxel] = (int)p;
}

__global__ void k_select_lookup(const int *voxels_xyz, int n, const SrlColorSlot *vtab, unsigned vmask, const int *tail, int *tail_of_entry) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int v = srl_color_find_voxel(vtab, vmask, voxels_xyz[(size_t)e * 3], voxels_xyz[(size_t)e * 3 + 1], voxels_xyz[(size_t)e * 3 + 2]);
    tail_of_entry[e] = v >= 0 ? tail[v] : -1;              // a voxel of the map holds at least one point (NumPoints() > 0)
}
struct SelectKnownIn {
    const int *tail_of_entry;
    __device__ int operator()(int e) const { return tail_of_entry[e] >= 0 ? 1 : 0; }
};
struct SelectKnownSink {
    const int *tail_of_entry;
    int *cand, *counters;
    int n;
    __device__ void operator()(int e, int known, int excl) const {
        if (known) cand[excl] = tail_of_entry[e];
        if (e == n - 1) counters[0] = excl + known;          // candidates
    }
};

// participating candidates of C candidates
__device__ __forceinline__ int select_participating(int C, int skip) { return (int)(((long long)C + skip - 1) / skip); }

// (a)
__global__ void __launch_bounds__(256) k_select_cells(const int *cand, const int *counters, int C_host, const SrlColorPoint *pool, SelectArgs A,
                                                      unsigned long long *keyw, unsigned long long *minw, unsigned mask, unsigned epoch16, unsigned tag,
                                                      unsigned *slot_out, double *depth_out, float *uv_out, unsigned long long *spart, unsigned long long *stot) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int m = select_participating(counters ? counters[0] : C_host, A.skip);
    unsigned c[SC_N] = {0, 0, 0, 0};
    if (j < A.m_hi) {
        unsigned slot = SRL_SEL_NONE;
        if (j < m) {
            const SrlColorPoint pt = pool[cand[(size_t)j * A.skip]];
            const double px = (double)pt.x, py = (double)pt.y, pz = (double)pt.z;      // getPosition(): position.cast<double>()
            const double depth = srl_color_depth(A.C, px, py, pz);
            if (depth > A.max_depth) {
                c[SC_FAR] = 1;
            } else if (depth < A.min_depth) {
                c[SC_NEAR] = 1;
            } else {
                double u_f, v_f;
                const int outcome = srl_color_project(A.C, px, py, pz, &u_f, &v_f);
                if (outcome == SRL_PROJ_BEHIND) {
                    c[SC_BEHIND] = 1;
                } else if (outcome == SRL_PROJ_OUTSIDE) {
                    c[SC_OUTSIDE] = 1;
                } else {
                    // u = std::round(u_f / minimum_dis) * minimum_dis into an int (:116-117): FP64 quotient, half away from zero, FP64 product, truncation
                    const int u = (int)(round(u_f / A.min_dis) * A.min_dis), v = (int)(round(v_f / A.min_dis) * A.min_dis);
                    const unsigned long long cell = ((unsigned long long)((long long)u - A.base_u) * (unsigned long long)A.span_v +
                                                     (unsigned long long)((long long)v - A.base_v)) & SRL_KEY48_MASK;
                    slot = srl_epoch_claim(keyw, mask, epoch16, cell, srl_hash_key(cell));
                    const unsigned long long want = ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint((float)depth);
                    if (minw[slot] > want) atomicMin(&minw[slot], want);      // a plain read: an older value is a larger one, never a missed update (an
                                                                               // agent-scope atomic load here measured no faster: DESIGN.md section 5)
                    depth_out[j] = depth;
                    uv_out[(size_t)j * 2] = (float)u_f; uv_out[(size_t)j * 2 + 1] = (float)v_f;      // cv::Point2f(u_f, v_f)
                }
            }
        }
        slot_out[j] = slot;
    }
    srl_wg_totals<SC_N, 256>(c, spart, stot);
}

// (b)
__global__ void __launch_bounds__(256) k_select_file(const int *counters, int C_host, int skip, const unsigned *slot_of, const double *depth_of,
                                                     const unsigned long long *minw, unsigned long long *lastw, unsigned long long *firstw, unsigned tag) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= select_participating(counters ? counters[0] : C_host, skip)) return;
    const unsigned slot = slot_of[j];
    if (slot == SRL_SEL_NONE) return;
    const double d = depth_of[j];
    const unsigned M = (unsigned)minw[slot];                 // of this call: this candidate lowered it itself
    if (__float_as_uint((float)d) != M) return;
    const unsigned i = (unsigned)j * (unsigned)skip;
    if (d < (double)__uint_as_float(M)) {
        const unsigned long long want = ((unsigned long long)tag << 32) | (unsigned long long)(0xFFFFFFFFu - i);
        if (lastw[slot] > want) atomicMin(&lastw[slot], want);
    } else {
        const unsigned long long want = ((unsigned long long)tag << 32) | (unsigned long long)i;
        if (firstw[slot] > want) atomicMin(&firstw[slot], want);
    }
}

// (c)
struct SelectHolderIn {
    const unsigned *slot_of;
    const unsigned long long *lastw, *firstw;
    unsigned tag, skip;
    __device__ int operator()(int j) const {
        const unsigned slot = slot_of[j];
        if (slot == SRL_SEL_NONE) return 0;
        const unsigned i = (unsigned)j * skip;
        const unsigned long long l = lastw[slot];
        if ((unsigned)(l >> 32) == tag) return 0xFFFFFFFFu - (unsigned)l == i ? 1 : 0;
        const unsigned long long f = firstw[slot];
        return ((unsigned)(f >> 32) == tag && (unsigned)f == i) ? 1 : 0;
    }
};
struct SelectRecordSink {
    const int *cand;
    const SrlColorPoint *pool;
    const float *uv;
    srl_color_selected *out;
    int out_cap, skip, n;
    int *counters;
    __device__ void operator()(int j, int holder, int excl) const {
        if (holder && excl < out_cap) {
            const int i = j * skip, p = cand[i];
            const SrlColorPoint pt = pool[p];
            srl_color_selected o;
            o.index = i; o.pool = p; o.point_index = pt.reg;
            o.x = pt.x; o.y = pt.y; o.z = pt.z;
            o.u = uv[(size_t)j * 2]; o.v = uv[(size_t)j * 2 + 1];
            out[excl] = o;
        }
        if (j == n - 1) counters[1] = excl + holder;         // selected
    }
};

unsigned select_pow2(unsigned long long v) { unsigned p = 1024; while (p < v && p < 0x80000000u) p <<= 1; return p; }

// the voxels' tails follow the pool: a sweep over what was appended since the last selection
int select_tails(srl_ctx *ctx, SrlColorMap *cm) {
    hipStream_t st = ctx->stream;
    if (cm->tail_cap < cm->vox_cap) {
        // grown by copy, as the voxel array is: voxel numbers stay, so the tails swept so far stay valid
        int *grown = nullptr;
        HIPCHK(ctx, hipMalloc((void **)&grown, (size_t)cm->vox_cap * sizeof(int)));
        if (cm->d_tail) {
            const hipError_t e = hipMemcpyAsync(grown, cm->d_tail, (size_t)cm->tail_cap * sizeof(int), hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) (void)hipFree(grown);
            HIPCHK(ctx, e);
            HIPCHK(ctx, hipStreamSynchronize(st));
            HIPCHK(ctx, hipFree(cm->d_tail));
        }
        cm->d_tail = grown;
        cm->tail_cap = cm->vox_cap;
    }
    const long long fresh = cm->num_points - cm->tail_swept;
    if (fresh > 0) {
        hipLaunchKernelGGL(k_select_tails, dim3((unsigned)((fresh + 255) / 256)), dim3(256), 0, st, cm->tail_swept, cm->num_points, cm->d_pool, cm->d_vox, cm->d_tail);
        HIPCHK(ctx, hipGetLastError());
        cm->tail_swept = cm->num_points;
    }
    return SRL_OK;
}

}  // namespace

void srl_color_select_free(SrlColorMap *cm) {
    if (cm->d_tail) hipFree(cm->d_tail);
    if (cm->d_sel_last) hipFree(cm->d_sel_last);
    if (cm->d_sel_first) hipFree(cm->d_sel_first);
    srl_epoch_table_free(cm->sel_cells);
    cm->d_tail = nullptr; cm->d_sel_last = nullptr; cm->d_sel_first = nullptr;
    cm->tail_cap = 0; cm->tail_swept = 0; cm->sel_words_cap = 0;
}

extern "C" void srl_color_select_opts_default(srl_color_select_opts *o) {
    if (!o) return;
    o->minimum_dis = 10.0;                 // rgbMapTracker.cpp:36
    o->skip_step = 1;
    o->use_all_points = 0;
    o->minimum_depth = 0.1;                // rgbMapTracker.cpp:9-10
    o->maximum_depth = 200;
}

extern "C" int srl_color_map_select(srl_ctx *ctx, const srl_color_camera *cam, int image_rows, int image_cols, const int32_t *voxels_xyz, int n_voxels,
                                    const srl_color_select_opts *opts, srl_color_selected *out, int64_t capacity, srl_color_select_totals *totals) {
    if (totals) std::memset(totals, 0, sizeof *totals);
    if (!ctx || !cam || !opts || n_voxels < 0 || (n_voxels > 0 && !voxels_xyz) || capacity < 0) return SRL_ERR_BAD_ARG;
    if (!std::isfinite(opts->minimum_dis) || !(opts->minimum_dis > 0.0) || opts->minimum_dis > 65536.0 || opts->skip_step < 1 ||
        std::isnan(opts->minimum_depth) || std::isnan(opts->maximum_depth)) {
        ctx->err = "select: minimum_dis finite in (0, 65536], skip_step >= 1, depth limits not NaN";
        return SRL_ERR_BAD_ARG;
    }
    if (image_rows < 2 || image_cols < 2 || (int64_t)image_rows * image_cols > SRL_COLOR_IMAGE_MAX_PIXELS) { ctx->err = "select: image size"; return SRL_ERR_BAD_ARG; }
    if (!srl_color_cam_finite(cam)) { ctx->err = "select: camera must be finite"; return SRL_ERR_BAD_ARG; }
    if (!(cam->fov_margin >= -4.0 && cam->fov_margin < 0.5)) { ctx->err = "select: fov_margin must lie in [-4, 0.5)"; return SRL_ERR_BAD_ARG; }
    SelectArgs A;
    if (!srl_color_cam_args(cam, image_rows, image_cols, &A.C)) { ctx->err = "select: camera pose is not finite"; return SRL_ERR_BAD_ARG; }
    { const int rc = srl_color_need_map_one_rank(ctx); if (rc) return rc; }
    SrlColorMap *cm = ctx->color;

    const bool list_mode = !opts->use_all_points && n_voxels > 0;      // (!use_all_points) && boxes_recent_hitted.size() (:74)
    const int skip = opts->skip_step;
    SRL_DISARM(ctx);                      // a waiting launch holds a workgroup on every compute unit
    if (cm->vtab_cap == 0 || (!list_mode && cm->num_registered == 0)) {      // a map nothing was ever inserted into: every key is unknown
        if (totals && list_mode) totals->unknown = n_voxels;
        return SRL_OK;
    }
    if (!list_mode && cm->num_registered > 0x7FFFFFFFll) { ctx->err = "select: more registered points than an int index holds"; return SRL_ERR_UNSUPPORTED; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    // the cells: keys lie within minimum_dis / 2 (and a rounding) of the accepted u, v
    const double md = opts->minimum_dis;
    A.min_dis = md; A.min_depth = opts->minimum_depth; A.max_depth = opts->maximum_depth; A.skip = skip;
    const long long top_u = (long long)std::ceil(A.C.u_hi + md / 2) + 2, top_v = (long long)std::ceil(A.C.v_hi + md / 2) + 2;
    A.base_u = (long long)std::floor(A.C.u_lo - md / 2) - 2; A.base_v = (long long)std::floor(A.C.v_lo - md / 2) - 2;
    const long long span_u = std::max<long long>(top_u - A.base_u + 1, 1);
    A.span_v = std::max<long long>(top_v - A.base_v + 1, 1);
    const double quot_u = std::max(std::floor((A.C.u_hi - A.C.u_lo) / md), 0.0) + 3.0, quot_v = std::max(std::floor((A.C.v_hi - A.C.v_lo) / md), 0.0) + 3.0;
    const double cells_d = std::min((double)span_u, quot_u) * std::min((double)A.span_v, quot_v);      // distinct keys the accepted points can form

    const int C_hi = list_mode ? n_voxels : (int)cm->num_registered;
    const int m_hi = (int)(((long long)C_hi + skip - 1) / skip);
    A.m_hi = m_hi;
    const unsigned long long cells_hi = cells_d < (double)m_hi ? (unsigned long long)cells_d : (unsigned long long)m_hi;      // ... and as many records at most
    const unsigned cap2 = select_pow2(2ull * cells_hi);

    const unsigned nblocks = (unsigned)((m_hi + 255) / 256);
    { const int rc = srl_wg_totals_reserve(ctx, cm->select_tot, SC_N + 1, SC_N, nblocks); if (rc) return rc; }
    { const int rc = srl_epoch_table_begin(ctx, cm->sel_cells, cap2, true); if (rc) return rc; }
    if (cm->sel_words_cap != cm->sel_cells.cap || cm->sel_cells.counter32 == 1) {      // the companions follow the table and the wrap of its counter (srl_epoch_table_begin has just cleared its own words)
        if (cm->sel_words_cap != cm->sel_cells.cap) {
            HIPCHK(ctx, hipStreamSynchronize(st));
            if (cm->d_sel_last) { HIPCHK(ctx, hipFree(cm->d_sel_last)); cm->d_sel_last = nullptr; }
            if (cm->d_sel_first) { HIPCHK(ctx, hipFree(cm->d_sel_first)); cm->d_sel_first = nullptr; }
            cm->sel_words_cap = 0;
            HIPCHK(ctx, hipMalloc((void **)&cm->d_sel_last, (size_t)cm->sel_cells.cap * 8));
            HIPCHK(ctx, hipMalloc((void **)&cm->d_sel_first, (size_t)cm->sel_cells.cap * 8));
            cm->sel_words_cap = cm->sel_cells.cap;
        }
        HIPCHK(ctx, hipMemsetAsync(cm->d_sel_last, 0xFF, (size_t)cm->sel_words_cap * 8, st));
        HIPCHK(ctx, hipMemsetAsync(cm->d_sel_first, 0xFF, (size_t)cm->sel_words_cap * 8, st));
    }
    const unsigned tag = 0xFFFFFFFFu - cm->sel_cells.counter32;

    DevBuf b_list, b_entry, b_cand, b_cnt, b_slot, b_depth, b_uv, b_out, b_sc;
    HIPCHK(ctx, b_cnt.alloc(ctx, 64));                               // [0] candidates (list mode) [1] selected
    HIPCHK(ctx, b_slot.alloc(ctx, (size_t)m_hi * 4));
    HIPCHK(ctx, b_depth.alloc(ctx, (size_t)m_hi * 8));
    HIPCHK(ctx, b_uv.alloc(ctx, (size_t)m_hi * 8));
    HIPCHK(ctx, b_out.alloc(ctx, (size_t)cells_hi * sizeof(srl_color_selected)));
    HIPCHK(ctx, b_sc.alloc(ctx, srl_scan_scratch_ints(std::max(C_hi, m_hi)) * 4));
    int *cnt = b_cnt.as<int>();
    const int *cand = cm->d_reg;
    const int *d_C = nullptr;
    if (list_mode) {
        { const int rc = select_tails(ctx, cm); if (rc) return rc; }
        { const int rc = srl_color_upload_list(ctx, voxels_xyz, n_voxels, b_list); if (rc) return rc; }
        HIPCHK(ctx, b_entry.alloc(ctx, (size_t)n_voxels * 4));
        HIPCHK(ctx, b_cand.alloc(ctx, (size_t)n_voxels * 4));
        hipLaunchKernelGGL(k_select_lookup, dim3((n_voxels + 255) / 256), dim3(256), 0, st, b_list.as<int>(), n_voxels, cm->d_vtab, cm->vtab_cap - 1, cm->d_tail,
                           b_entry.as<int>());
        HIPCHK(ctx, hipGetLastError());
        srl_scan(SelectKnownIn{b_entry.as<int>()}, SelectKnownSink{b_entry.as<int>(), b_cand.as<int>(), cnt, n_voxels}, n_voxels, b_sc.as<int>(), st);
        HIPCHK(ctx, hipGetLastError());
        cand = b_cand.as<int>();
        d_C = cnt;
    }
    hipLaunchKernelGGL(k_select_cells, dim3(nblocks), dim3(256), 0, st, cand, d_C, C_hi, cm->d_pool, A, cm->sel_cells.keyw, cm->sel_cells.minw, cap2 - 1,
                       cm->sel_cells.epoch16, tag, b_slot.as<unsigned>(), b_depth.as<double>(), b_uv.as<float>(), cm->select_tot.d_rows, cm->select_tot.d_tot);
    hipLaunchKernelGGL(k_select_file, dim3(nblocks), dim3(256), 0, st, d_C, C_hi, skip, b_slot.as<unsigned>(), b_depth.as<double>(), cm->sel_cells.minw,
                       cm->d_sel_last, cm->d_sel_first, tag);
    HIPCHK(ctx, hipGetLastError());
    srl_scan(SelectHolderIn{b_slot.as<unsigned>(), cm->d_sel_last, cm->d_sel_first, tag, (unsigned)skip},
             SelectRecordSink{cand, cm->d_pool, b_uv.as<float>(), b_out.as<srl_color_selected>(), (int)cells_hi, skip, m_hi, cnt}, m_hi, b_sc.as<int>(), st);
    HIPCHK(ctx, hipGetLastError());

    // one wait for the totals, then one DMA of exactly `selected` records
    { const int rc = ensure_host_scratch(ctx, 128); if (rc) return rc; }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch, cm->select_tot.d_tot, SC_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch + 64, cnt, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    unsigned long long h_tot[SC_N];
    int h_cnt[2];
    std::memcpy(h_tot, ctx->h_scratch, sizeof h_tot);
    std::memcpy(h_cnt, ctx->h_scratch + 64, sizeof h_cnt);
    const int C = list_mode ? h_cnt[0] : C_hi;
    const int64_t selected = h_cnt[1];
    if (totals) {
        totals->candidates = C; totals->visited = ((int64_t)C + skip - 1) / skip;
        totals->far = (int64_t)h_tot[SC_FAR]; totals->near = (int64_t)h_tot[SC_NEAR]; totals->behind = (int64_t)h_tot[SC_BEHIND]; totals->outside = (int64_t)h_tot[SC_OUTSIDE];
        totals->selected = selected; totals->unknown = list_mode ? (int64_t)n_voxels - C : 0;
    }
    if (selected > (int64_t)cells_hi) { ctx->err = "select: more holders than cells (internal)"; return SRL_ERR_HIP; }
    if (!out || selected == 0) return SRL_OK;
    if (capacity < selected) { ctx->err = "select: capacity below the number of selected points (totals->selected)"; return SRL_ERR_BAD_ARG; }
    const size_t bytes = (size_t)selected * sizeof(srl_color_selected);
    { const int rc = ensure_host_scratch(ctx, bytes); if (rc) return rc; }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch, b_out.p, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    std::memcpy(out, ctx->h_scratch, bytes);
    return SRL_OK;
}

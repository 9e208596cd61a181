// srl_color_render.hip -- the colour voxel map's first consumer on the device for gfx950: rgbMapTracker::renderPointsInRecentVoxel /
// threadRenderPointsInVoxel (src/rgbMapTracker.cpp:176-237).  For every point of every listed voxel: project3dPointInThisImage
// (src/lioOptimization.cpp:142-199, if2dPointsAvailable :48-60), the sub-pixel colour getSubPixel<cv::Vec3b> (:71-97) and
// rgbPoint::updateRgb (src/cloudMap.cpp:59-100).  Every operation is an IEEE operation in the reference's order (-ffp-contract=off,
// sums of three as (a0 + a1) + a2), so the state is held to the bar of the rest of this tree: bitwise.
//
//   k_render_mark    one thread per list entry: the key is looked up in the map's voxel table and the voxel's mark word,
//                    (render epoch << 16) | occurrences, is raised by the entries of the wave that name it -- a word of another epoch IS
//                    zero occurrences, nothing is cleared per call
//   k_render_points  one thread per POOL point: 24-byte record, 4-byte mark gather; an unmarked point leaves at once, a marked one runs
//                    the loop body `occurrences` times and rewrites its 40-byte state record.  The six counters leave through
//                    srl_wg_totals (srl_wg_totals.h)
// The sweep is linear in the map, not in the list: it needs no per-voxel point index (the layout forbids a cap-sized one).
//
// OpenCV's Vec3b arithmetic decides the colour's bits: `double * Vec3b` is a Vec3b of saturate_cast<uchar>(w * pixel)
// = round to nearest, ties to even (cvRound = lrint), clamped to 0 ... 255; `Vec3b + Vec3b` saturates; the four terms are added left to
// right; the channels become doubles only then.
#include "srl_ctx.h"
#include "srl_color_map.h"
#include "srl_color_project.h"
#include "srl_image_prep.h"
#include "srl_hash.h"
#include "host/srl_la.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

struct RenderArgs {
    SrlCamArgs C;                      // the pose, the intrinsics and the bounds of the field of view (srl_color_project.h)
    double obs_time;
    int rows, cols;
};
enum { RC_LISTED, RC_BEHIND, RC_OUTSIDE, RC_GATED, RC_FIRST, RC_UPDATED, RC_N };
#define SRL_RTOT_UNKNOWN (RC_N + 1)   // behind the ticket: the two words the mark kernel counts in, since allocation
#define SRL_RTOT_OVERFLOW (RC_N + 2)
#define SRL_RTOT_WORDS (RC_N + 3)

__global__ void k_render_mark(const int *voxels_xyz, int n, const SrlColorSlot *vtab, unsigned vmask, unsigned *mark, unsigned epoch, unsigned long long *rtot) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int v = -1;
    if (e < n) {
        v = srl_color_find_voxel(vtab, vmask, voxels_xyz[(size_t)e * 3], voxels_xyz[(size_t)e * 3 + 1], voxels_xyz[(size_t)e * 3 + 2]);
        if (v < 0) atomicAdd(&rtot[SRL_RTOT_UNKNOWN], 1ull);
    }
    // the entries of a wave that name one voxel add their number in ONE compare-and-swap: with one per entry a list that names a voxel
    // tens of thousands of times retries n^2 / 2 times on one word (seconds for the 65 535 a mark word counts).  The sum of what was added
    // never passes 0xFFFF, so a list is flagged exactly when it names a voxel more often than that, whatever the order of the waves
    unsigned long long pending = __ballot(v >= 0);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int lv = __shfl(v, leader);
        const unsigned long long same = __ballot(v == lv);
        pending &= ~same;
        if (lane == leader) {                 // (the wave meets again behind this block: `pending` and the ballots stay those of the whole wave)
            const unsigned add = (unsigned)__popcll(same);
            unsigned old = mark[lv];
            for (;;) {
                const unsigned have = (old >> 16) == epoch ? (old & 0xFFFFu) : 0u;
                if (have + add > 0xFFFFu) { atomicAdd(&rtot[SRL_RTOT_OVERFLOW], 1ull); break; }
                const unsigned prev = atomicCAS(&mark[lv], old, (epoch << 16) | (have + add));
                if (prev == old) break;
                old = prev;
            }
        }
    }
}

// (short) of a double as the reference's x86-64 build does it: cvttsd2si to 32 bits (the "integer indefinite" 0x80000000 outside the
// range), low 16 bits
__device__ __forceinline__ short render_short(double x) {
    const int t = (x > -2147483649.0 && x < 2147483648.0) ? (int)x : (int)0x80000000u;
    return (short)t;
}

__global__ void __launch_bounds__(256) k_render_points(long long P, const SrlColorPoint *pool, const unsigned *mark, unsigned epoch, SrlColorState *state,
                                                       const unsigned char *img, RenderArgs A, unsigned long long overflow_before, unsigned long long *rpart,
                                                       unsigned long long *rtot) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned c[RC_N] = {0, 0, 0, 0, 0, 0};
    // a list that names one voxel more than 65 535 times: the mark kernel has flagged it, nothing is rendered
    const bool refused = rtot[SRL_RTOT_OVERFLOW] != overflow_before;
    if (p < P && !refused) {
        const SrlColorPoint pt = pool[p];
        const unsigned w = mark[pt.voxel];
        if ((w >> 16) == epoch) {
            const unsigned mult = w & 0xFFFFu;
            c[RC_LISTED] = mult;
            const double px = (double)pt.x, py = (double)pt.y, pz = (double)pt.z;
            double u, v;
            const int outcome = srl_color_project(A.C, px, py, pz, &u, &v);
            if (outcome == SRL_PROJ_BEHIND) {
                c[RC_BEHIND] = mult;
            } else {
                if (outcome == SRL_PROJ_OUTSIDE) {
                    c[RC_OUTSIDE] = mult;
                } else {
                    const double d = srl_color_depth(A.C, px, py, pz);
                    // the test above leaves 1 <= floor < cols (rows)
                    int byte[3];
                    srl_color_sub_pixel(img, A.rows, A.cols, v, u, byte);
                    const double col[3] = {(double)byte[0], (double)byte[1], (double)byte[2]};
                    SrlColorState s = state[p];
                    bool changed = false;
                    for (unsigned it = 0; it < mult; ++it) {
                        if (s.observe_distance != 0 && (d > s.observe_distance * 1.2)) { ++c[RC_GATED]; continue; }
                        changed = true;
                        if (s.n_rgb == 0) {
                            s.last_observe_time = A.obs_time;
                            s.observe_distance = d;
#pragma unroll
                            for (int k = 0; k < 3; k++) { s.rgb[k] = render_short(round(col[k])); s.cov_rgb[k] = (float)15.0; }
                            s.n_rgb = 1;
                            ++c[RC_FIRST];
                            continue;
                        }
#pragma unroll
                        for (int k = 0; k < 3; k++) {
                            float cv = (float)((double)s.cov_rgb[k] + 0.1 * (A.obs_time - s.last_observe_time));
                            const double old_sigma = (double)cv;
                            cv = (float)sqrt(1.0 / (1.0 / (double)(cv * cv) + 1.0 / (15.0 * 15.0)));
                            s.cov_rgb[k] = cv;
                            s.rgb[k] = render_short((double)(cv * cv) * ((double)s.rgb[k] / (old_sigma * old_sigma) + col[k] / (15.0 * 15.0)));
                        }
                        if (d < s.observe_distance) s.observe_distance = d;
                        s.last_observe_time = A.obs_time;
                        s.n_rgb = (short)(s.n_rgb + 1);
                        ++c[RC_UPDATED];
                    }
                    if (changed) state[p] = s;
                }
            }
        }
    }
    srl_wg_totals<RC_N, 256>(c, rpart, rtot);
}

// srl_color_registered_rgb
__global__ void k_render_reg_gather(const int *reg_list, long long first, int count, const SrlColorState *state, SrlColorState *out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    out[t] = state[reg_list[first + t]];
}

void split_state(const SrlColorState &s, size_t at, int16_t *rgb, int16_t *n_rgb, float *cov, double *dist, double *time) {
    if (rgb) { rgb[at * 3] = s.rgb[0]; rgb[at * 3 + 1] = s.rgb[1]; rgb[at * 3 + 2] = s.rgb[2]; }
    if (n_rgb) n_rgb[at] = s.n_rgb;
    if (cov) { cov[at * 3] = s.cov_rgb[0]; cov[at * 3 + 1] = s.cov_rgb[1]; cov[at * 3 + 2] = s.cov_rgb[2]; }
    if (dist) dist[at] = s.observe_distance;
    if (time) time[at] = s.last_observe_time;
}

}  // namespace

int srl_color_state_reserve(srl_ctx *ctx, SrlColorMap *cm) {
    if (!cm->render_on || cm->state_cap >= cm->pool_cap) return SRL_OK;
    SrlColorState *ns = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&ns, cm->pool_cap * sizeof(SrlColorState)));
    const size_t used = cm->d_state ? (size_t)cm->num_points : 0;
    if (used > 0) HIPCHK(ctx, hipMemcpyAsync(ns, cm->d_state, used * sizeof(SrlColorState), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ns + used, 0, (cm->pool_cap - used) * sizeof(SrlColorState), ctx->stream));      // rgbPoint::reset()
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (cm->d_state) HIPCHK(ctx, hipFree(cm->d_state));
    cm->d_state = ns;
    cm->state_cap = cm->pool_cap;
    return SRL_OK;
}

void srl_color_render_free(SrlColorMap *cm) {
    if (cm->img_pending && cm->img_ev) hipEventSynchronize(cm->img_ev);
    if (cm->d_state) hipFree(cm->d_state);
    if (cm->d_mark) hipFree(cm->d_mark);
    cm->img.release();
    if (cm->img_ev) hipEventDestroy(cm->img_ev);
    cm->d_state = nullptr; cm->d_mark = nullptr; cm->img_ev = nullptr;
}

extern "C" int srl_color_image_upload(srl_ctx *ctx, const uint8_t *bgr, int rows, int cols, int64_t row_stride_bytes) {
    if (!ctx || !bgr || rows < 2 || cols < 2 || (int64_t)rows * cols > SRL_COLOR_IMAGE_MAX_PIXELS || row_stride_bytes < (int64_t)cols * 3) return SRL_ERR_BAD_ARG;
    { const int rc = srl_color_need_map_one_rank(ctx); if (rc) return rc; }
    SrlColorMap *cm = ctx->color;
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t row_bytes = (size_t)cols * 3, bytes = row_bytes * (size_t)rows;
    if (!cm->img_ev) HIPCHK(ctx, hipEventCreateWithFlags(&cm->img_ev, hipEventDisableTiming));
    if (cm->img_pending) { HIPCHK(ctx, hipEventSynchronize(cm->img_ev)); cm->img_pending = false; }      // the staging block is free again
    { const int rc = cm->img.reserve(ctx, bytes, bytes); if (rc) return rc; }
    cm->img_rows = 0; cm->img_cols = 0;
    { const int rc = cm->img.upload(ctx, bgr, rows, row_bytes, row_stride_bytes); if (rc) return rc; }
    HIPCHK(ctx, hipEventRecord(cm->img_ev, ctx->stream));
    cm->img_pending = true;
    cm->render_on = true;                 // from here on the colour state exists and follows the pool
    { const int rc = srl_color_state_reserve(ctx, cm); if (rc) return rc; }
    cm->img_rows = rows; cm->img_cols = cols;
    return SRL_OK;
}

// srl_image_prepare's hand-over: what srl_color_image_upload leaves, with the image already on the device (the caller has made the
// upload's refusals; the copy is ordered on the context's stream behind the kernels that wrote d_bgr and in front of the next render)
int srl_color_image_install(srl_ctx *ctx, const unsigned char *d_bgr, int rows, int cols) {
    SrlColorMap *cm = ctx->color;
    const size_t bytes = (size_t)cols * 3 * (size_t)rows;
    { const int rc = cm->img.reserve(ctx, 0, bytes); if (rc) return rc; }
    cm->img_rows = 0; cm->img_cols = 0;
    HIPCHK(ctx, hipMemcpyAsync(cm->img.d, d_bgr, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    cm->render_on = true;
    { const int rc = srl_color_state_reserve(ctx, cm); if (rc) return rc; }
    cm->img_rows = rows; cm->img_cols = cols;
    return SRL_OK;
}

extern "C" int srl_color_map_render(srl_ctx *ctx, const srl_color_camera *cam, const int32_t *voxels_xyz, int n_voxels, double obs_time,
                                    srl_color_render_totals *totals) {
    if (totals) std::memset(totals, 0, sizeof *totals);
    if (!ctx || !cam || n_voxels < 0 || (n_voxels > 0 && !voxels_xyz)) return SRL_ERR_BAD_ARG;
    {
        const bool finite = std::isfinite(obs_time) && srl_color_cam_finite(cam);
        if (!finite) { ctx->err = "render: camera and observation time must be finite"; return SRL_ERR_BAD_ARG; }
        if (!(cam->fov_margin > 0.0)) { ctx->err = "render: fov_margin must be > 0 (at 0 an integral u = cols - 1 reads one pixel past the row)"; return SRL_ERR_BAD_ARG; }
    }
    { const int rc = srl_color_need_map(ctx); if (rc) return rc; }
    SrlColorMap *cm = ctx->color;
    if (cm->img_rows == 0) { ctx->err = "no image uploaded (srl_color_image_upload)"; return SRL_ERR_NO_SWEEP; }
    { const int rc = srl_color_one_rank(ctx); if (rc) return rc; }
    if (n_voxels == 0) return SRL_OK;
    SRL_DISARM(ctx);                      // a waiting launch holds a workgroup on every compute unit
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    // refreshPoseForProjection (lioOptimization.cpp:201-205) and the bounds of if2dPointsAvailable (:55-56)
    RenderArgs A;
    A.rows = cm->img_rows; A.cols = cm->img_cols; A.obs_time = obs_time;
    if (!srl_color_cam_args(cam, A.rows, A.cols, &A.C)) { ctx->err = "render: camera pose is not finite"; return SRL_ERR_BAD_ARG; }
    const long long P = cm->num_points;
    const unsigned nblocks = (unsigned)((P + 255) / 256);
    if (cm->vtab_cap == 0) {              // a map nothing was ever inserted into: every key is unknown
        if (totals) totals->unknown = n_voxels;
        return SRL_OK;
    }
    { const int rc = srl_wg_totals_reserve(ctx, cm->render_tot, SRL_RTOT_WORDS, RC_N, nblocks); if (rc) return rc; }
    if (cm->mark_cap < cm->vox_cap) {
        if (cm->d_mark) { HIPCHK(ctx, hipStreamSynchronize(st)); HIPCHK(ctx, hipFree(cm->d_mark)); cm->d_mark = nullptr; cm->mark_cap = 0; }
        HIPCHK(ctx, hipMalloc((void **)&cm->d_mark, (size_t)cm->vox_cap * sizeof(unsigned)));
        HIPCHK(ctx, hipMemsetAsync(cm->d_mark, 0, (size_t)cm->vox_cap * sizeof(unsigned), st));
        cm->mark_cap = cm->vox_cap;
    }
    if (++cm->render_epoch > 0xFFFFu) {
        cm->render_epoch = 1;
        HIPCHK(ctx, hipMemsetAsync(cm->d_mark, 0, (size_t)cm->mark_cap * sizeof(unsigned), st));
    }
    { const int rc = srl_color_state_reserve(ctx, cm); if (rc) return rc; }
    DevBuf b_list;
    { const int rc = srl_color_upload_list(ctx, voxels_xyz, n_voxels, b_list); if (rc) return rc; }
    hipLaunchKernelGGL(k_render_mark, dim3((n_voxels + 255) / 256), dim3(256), 0, st, b_list.as<int>(), n_voxels, cm->d_vtab, cm->vtab_cap - 1, cm->d_mark,
                       cm->render_epoch, cm->render_tot.d_tot);
    HIPCHK(ctx, hipGetLastError());
    if (nblocks > 0) {
        hipLaunchKernelGGL(k_render_points, dim3(nblocks), dim3(256), 0, st, P, cm->d_pool, cm->d_mark, cm->render_epoch, cm->d_state, cm->img.d, A,
                           cm->overflow_seen, cm->render_tot.d_rows, cm->render_tot.d_tot);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch, cm->render_tot.d_tot, SRL_RTOT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    cm->img_pending = false;
    unsigned long long h[SRL_RTOT_WORDS];
    std::memcpy(h, ctx->h_scratch, sizeof h);
    const unsigned long long unknown = h[SRL_RTOT_UNKNOWN] - cm->unknown_seen, overflow = h[SRL_RTOT_OVERFLOW] - cm->overflow_seen;
    cm->unknown_seen = h[SRL_RTOT_UNKNOWN]; cm->overflow_seen = h[SRL_RTOT_OVERFLOW];
    if (overflow) { ctx->err = "render: the list names one voxel more than 65 535 times (nothing was rendered)"; return SRL_ERR_UNSUPPORTED; }
    if (totals) {
        if (nblocks > 0) {
            totals->listed = (int64_t)h[RC_LISTED]; totals->behind = (int64_t)h[RC_BEHIND]; totals->outside = (int64_t)h[RC_OUTSIDE];
            totals->gated = (int64_t)h[RC_GATED]; totals->first = (int64_t)h[RC_FIRST]; totals->updated = (int64_t)h[RC_UPDATED];
        }
        totals->unknown = (int64_t)unknown;
    }
    return SRL_OK;
}

extern "C" int srl_color_map_download_rgb(srl_ctx *ctx, int16_t *rgb, int16_t *n_rgb, float *cov_rgb, double *observe_distance, double *last_observe_time,
                                          int64_t max_points) {
    if (!ctx) return SRL_ERR_BAD_ARG;
    const SrlColorMap *cm = ctx->color;
    if (!cm) return SRL_ERR_NO_MAP;
    const int V = cm->num_voxels;
    const long long P = cm->num_points;
    if (max_points < P) return SRL_ERR_BAD_ARG;
    if (P == 0) return SRL_OK;
    if (!cm->d_state) {                   // never rendered: every point is as rgbPoint::reset() left it
        const SrlColorState zero = {};
        for (long long p = 0; p < P; p++) split_state(zero, (size_t)p, rgb, n_rgb, cov_rgb, observe_distance, last_observe_time);
        return SRL_OK;
    }
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<SrlColorVoxel> vox((size_t)V);
    std::vector<SrlColorPoint> pool((size_t)P);
    std::vector<SrlColorState> state((size_t)P);
    HIPCHK(ctx, hipMemcpyAsync(vox.data(), cm->d_vox, (size_t)V * sizeof(SrlColorVoxel), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(pool.data(), cm->d_pool, (size_t)P * sizeof(SrlColorPoint), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(state.data(), cm->d_state, (size_t)P * sizeof(SrlColorState), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<long long> first((size_t)V + 1, 0);
    for (int v = 0; v < V; v++) first[(size_t)v + 1] = first[v] + vox[v].count;
    if (first[V] != P) { ctx->err = "colour map: voxel counts and point pool disagree"; return SRL_ERR_HIP; }
    for (long long p = 0; p < P; p++) {
        const SrlColorPoint &pt = pool[(size_t)p];
        split_state(state[(size_t)p], (size_t)(first[pt.voxel] + pt.slot), rgb, n_rgb, cov_rgb, observe_distance, last_observe_time);      // voxel after voxel, slot order
    }
    return SRL_OK;
}

extern "C" int srl_color_registered_rgb(srl_ctx *ctx, int64_t first, int count, int16_t *rgb, int16_t *n_rgb, float *cov_rgb, double *observe_distance,
                                        double *last_observe_time) {
    if (!ctx || first < 0 || count < 0) return SRL_ERR_BAD_ARG;
    const SrlColorMap *cm = ctx->color;
    if (!cm) return SRL_ERR_NO_MAP;
    if (first + count > cm->num_registered) return SRL_ERR_BAD_ARG;
    if (count == 0) return SRL_OK;
    if (!cm->d_state) {
        const SrlColorState zero = {};
        for (int t = 0; t < count; t++) split_state(zero, (size_t)t, rgb, n_rgb, cov_rgb, observe_distance, last_observe_time);
        return SRL_OK;
    }
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf b_out;
    HIPCHK(ctx, b_out.alloc(ctx, (size_t)count * sizeof(SrlColorState)));
    { const int rc = ensure_host_scratch(ctx, (size_t)count * sizeof(SrlColorState)); if (rc) return rc; }
    hipLaunchKernelGGL(k_render_reg_gather, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, cm->d_reg, (long long)first, count, cm->d_state,
                       b_out.as<SrlColorState>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch, b_out.p, (size_t)count * sizeof(SrlColorState), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const SrlColorState *s = reinterpret_cast<const SrlColorState *>(ctx->h_scratch);
    for (int t = 0; t < count; t++) split_state(s[t], (size_t)t, rgb, n_rgb, cov_rgb, observe_distance, last_observe_time);
    return SRL_OK;
}

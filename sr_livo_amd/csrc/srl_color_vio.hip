// srl_color_vio.hip -- the colour voxel map's consumers between the selection and the render of a frame, on the device for gfx950: the
// per-point loops of imageProcessing::vioEsikf (src/imageProcessing.cpp:308-349, reprojection, 11 states) and imageProcessing::vioPhotometric
// (:463-518, photometric, 6 states) with cloudFrame::getRgb(u, v, 0, &dx, &dy) (src/lioOptimization.cpp:99-140), and the products H^T H,
// H^T r over them.  Every operation is an IEEE operation in the reference's order (-ffp-contract=off, sums of three as (a0 + a1) + a2, the
// zeros of J_u_pc and of the skew matrix multiplied and added as a coefficient-wise matrix product does), so a point's rows are held to the
// bar of the rest of this tree: bitwise.  The contract is written out in include/srlivo_hip.h.
//
//   k_vio_rows   one thread per listed point: its 24 doubles and its acc_residual term go into the workgroup's LDS block (256 x 25 doubles),
//                from where they leave to `rows` in whole lines.  The 78 sums (66 of the upper triangle of H^T H, 11 of H^T r, acc_residual)
//                are formed from that block in a fixed order: every wave walks its 64 points in list order, one sum per lane and round; the
//                four waves are combined through LDS as (w0 + w1) + (w2 + w3); one row per workgroup and a ticket as in srl_wg_totals.h, but
//                the kernel keeps its own epilogue: the last workgroup adds the rows up in INDEX order, one thread per word, which is
//                what makes the FP64 sums a function of the list alone.  No floating-point atomics.
#include "srl_ctx.h"
#include "srl_color_map.h"
#include "srl_color_project.h"

#include <cmath>
#include <cstring>

static_assert(sizeof(srl_color_vio_point) == 40, "srl_color_vio_point is 40 bytes on both sides of the C-ABI");
static_assert(sizeof(srl_color_vio_sums) == (121 + 11 + 1) * 8 + 5 * 8, "srl_color_vio_sums: 133 doubles and 5 counts");

namespace {

#define VIO_STRIDE 25                  // 24 doubles of a point's rows and its acc_residual term; odd in 8-byte words: the lanes' writes spread over the banks
#define VIO_PAIRS 66                   // upper triangle of 11 x 11
#define VIO_SUMS 78                    // + 11 of H^T r + acc_residual
#define VIO_COUNTS 80                  // words 80 ... 84 of a row: used, few_views, behind, outside, unknown
#define VIO_ROW_WORDS 88
#define VIO_TICKET 88
enum { VC_N = 5 };

struct VioArgs {
    SrlCamArgs C;                      // the pose and the intrinsics (srl_color_project.h); the bounds of the field of view are not read
    double time_td;
    double Rt[9];                      // R_imu_camera.transpose(), row-major
    int mode, estimate_extrinsic, estimate_intrinsic;
    int rows, cols;                    // of the uploaded image (photometric mode)
    int n;
    long long P;
};

// (a, b) of the upper triangle, row after row
__constant__ unsigned char c_pair_a[VIO_PAIRS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3,
                                                  3, 3, 3, 3, 3, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 6, 6, 6, 6, 6, 7, 7, 7, 7, 8, 8, 8, 9, 9, 10};
__constant__ unsigned char c_pair_b[VIO_PAIRS] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 2, 3, 4, 5, 6, 7, 8, 9, 10, 3, 4, 5,
                                                  6, 7, 8, 9, 10, 4, 5, 6, 7, 8, 9, 10, 5, 6, 7, 8, 9, 10, 6, 7, 8, 9, 10, 7, 8, 9, 10, 8, 9, 10, 9, 10, 10};

// getHuberLoss(residual, 1.0) (imageProcessing.cpp:202-216): residual / 1.0 and sqrt(1.0) change no bit
__device__ __forceinline__ double vio_huber(double residual) {
    return residual < 1.0 ? 1.0 : (2 * sqrt(residual) - 1.0) / residual;
}
// one row of a coefficient-wise product with a 3 x 3 matrix M (row-major): out[k] = (j[0] M[0][k] + j[1] M[1][k]) + j[2] M[2][k]
__device__ __forceinline__ void vio_row_times(const double j[3], const double *M, double out[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = (j[0] * M[k] + j[1] * M[3 + k]) + j[2] * M[6 + k];
}

// one point of the list; writes its rows and its acc_residual term (row[24]) and returns its outcome
__device__ __forceinline__ int vio_point(const srl_color_vio_point &q, const SrlColorPoint *pool, const SrlColorState *state, const unsigned char *img,
                                         const VioArgs &A, double *row) {
    if (q.pool < 0 || (long long)q.pool >= A.P) return SRL_VIO_UNKNOWN;
    const bool photometric = A.mode == SRL_VIO_PHOTOMETRIC;
    SrlColorState s = {};
    if (photometric) {
        if (state) s = state[q.pool];
        if (s.n_rgb < 3) return SRL_VIO_FEW_VIEWS;                             // :465
    }
    const SrlColorPoint pt = pool[q.pool];
    const double px = (double)pt.x, py = (double)pt.y, pz = (double)pt.z;      // getPosition(): position.cast<double>()
    double x, y, z;
    srl_color_to_camera(A.C, px, py, pz, &x, &y, &z);
    if (z < 0.001) return SRL_VIO_BEHIND;
    const double u = (A.C.fx * x / z + A.C.cx) + A.time_td * q.vel_u, v = (A.C.fy * y / z + A.C.cy) + A.time_td * q.vel_v;
    const double J0[3] = {A.C.fx / z, 0.0, -(A.C.fx * x) / (z * z)}, J1[3] = {0.0, A.C.fy / z, -(A.C.fy * y) / (z * z)};      // J_u_pc
    const double S[9] = {0.0, -z, y, z, 0.0, -x, -y, x, 0.0};                  // numType::skewSymmetric(point_camera)

    if (!photometric) {
        const double du = u - q.match_u, dv = v - q.match_v;
        const double residual = sqrt(du * du + dv * dv);
        const double huber = vio_huber(residual);
        row[24] = residual;
        row[11] = du * huber; row[23] = dv * huber;
        row[0] = q.vel_u * huber; row[12] = q.vel_v * huber;
        if (A.estimate_extrinsic) {
            const double N0[3] = {-J0[0], -J0[1], -J0[2]}, N1[3] = {-J1[0], -J1[1], -J1[2]};
            double a[3];
            vio_row_times(J0, S, a);     row[1] = a[0] * huber;  row[2] = a[1] * huber;  row[3] = a[2] * huber;
            vio_row_times(N0, A.Rt, a);  row[4] = a[0] * huber;  row[5] = a[1] * huber;  row[6] = a[2] * huber;
            vio_row_times(J1, S, a);     row[13] = a[0] * huber; row[14] = a[1] * huber; row[15] = a[2] * huber;
            vio_row_times(N1, A.Rt, a);  row[16] = a[0] * huber; row[17] = a[1] * huber; row[18] = a[2] * huber;
        }
        if (A.estimate_intrinsic) {      // J_u_K = [x/z 0 1 0; 0 y/z 0 1]
            row[7] = x / z * huber;  row[8] = 0.0 * huber;      row[9] = 1.0 * huber;  row[10] = 0.0 * huber;
            row[19] = 0.0 * huber;   row[20] = y / z * huber;   row[21] = 0.0 * huber; row[22] = 1.0 * huber;
        }
        return SRL_VIO_USED;
    }

    // the footprint of getRgb's 17 samples: columns floor(u) - 4 ... floor(u) + 5, rows likewise; nothing is clamped
    // (u + bias may round up to an integer, so that floor(u + bias) = floor(u) + bias + 1: the neighbour one past the footprint then has
    // weight exactly 0 and srl_color_sub_pixel's clamp to the last row / column is what keeps that read inside the image)
    const double fu = floor(u), fv = floor(v);
    if (!(isfinite(u) && isfinite(v) && fu - 4.0 >= 0.0 && fu + 5.0 <= (double)(A.cols - 1) && fv - 4.0 >= 0.0 && fv + 5.0 <= (double)(A.rows - 1)))
        return SRL_VIO_OUTSIDE;
    int obs[3], smp[3];
    srl_color_sub_pixel(img, A.rows, A.cols, v, u, obs);
    float left[3] = {0.f, 0.f, 0.f}, right[3] = {0.f, 0.f, 0.f}, down[3] = {0.f, 0.f, 0.f}, up[3] = {0.f, 0.f, 0.f};
    float pixel_dif = 0.f;
#pragma unroll 1
    for (int bias = 1; bias < 5; bias++) {          // ssd = 5; kept a loop: unrolled, the 192 byte loads of 16 samples are all in flight at once
        srl_color_sub_pixel(img, A.rows, A.cols, v, u - bias, smp);
        left[0] += (float)smp[0]; left[1] += (float)smp[1]; left[2] += (float)smp[2];
        srl_color_sub_pixel(img, A.rows, A.cols, v, u + bias, smp);
        right[0] += (float)smp[0]; right[1] += (float)smp[1]; right[2] += (float)smp[2];
        srl_color_sub_pixel(img, A.rows, A.cols, v - bias, u, smp);
        down[0] += (float)smp[0]; down[1] += (float)smp[1]; down[2] += (float)smp[2];
        srl_color_sub_pixel(img, A.rows, A.cols, v + bias, u, smp);
        up[0] += (float)smp[0]; up[1] += (float)smp[1]; up[2] += (float)smp[2];
        pixel_dif += (float)(2 * bias);
    }
    double res[3], info[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        info[k] = 1.0 / (double)s.cov_rgb[k];
        res[k] = (double)obs[k] - (double)s.rgb[k];
    }
    const double huber = vio_huber(sqrt((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2]));
    const double r0 = res[0] * huber, r1 = res[1] * huber, r2 = res[2] * huber;
    row[24] = ((r0 * info[0]) * r0 + (r1 * info[1]) * r1) + (r2 * info[2]) * r2;
    row[6] = r0; row[14] = r1; row[22] = r2;
    row[7] = info[0]; row[15] = info[1]; row[23] = info[2];
    if (A.estimate_extrinsic) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double dx = (double)(right[k] - left[k]) / (double)pixel_dif, dy = (double)(up[k] - down[k]) / (double)pixel_dif;
            const double Jc[3] = {dx * J0[0] + dy * J1[0], dx * J0[1] + dy * J1[1], dx * J0[2] + dy * J1[2]};      // J_color_u * J_u_pc
            const double Nc[3] = {-Jc[0], -Jc[1], -Jc[2]};
            double a[3];
            vio_row_times(Jc, S, a);     row[k * 8] = a[0] * huber;     row[k * 8 + 1] = a[1] * huber; row[k * 8 + 2] = a[2] * huber;
            vio_row_times(Nc, A.Rt, a);  row[k * 8 + 3] = a[0] * huber; row[k * 8 + 4] = a[1] * huber; row[k * 8 + 5] = a[2] * huber;
        }
    }
    return SRL_VIO_USED;
}

__global__ void __launch_bounds__(256) k_vio_rows(const srl_color_vio_point *points, const SrlColorPoint *pool, const SrlColorState *state,
                                                  const unsigned char *img, VioArgs A, double *rows_out, unsigned char *outcome_out,
                                                  unsigned long long *vpart, unsigned long long *vtot) {
    __shared__ double s_rows[256 * VIO_STRIDE];
    __shared__ double s_wave[4][VIO_COUNTS];
    __shared__ unsigned s_cnt[4][VC_N];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i = blockIdx.x * 256 + tid;
    double *row = s_rows + tid * VIO_STRIDE;
#pragma unroll
    for (int k = 0; k < VIO_STRIDE; k++) row[k] = 0.0;
    unsigned c[VC_N] = {0, 0, 0, 0, 0};
    if (i < A.n) {
        const int outcome = vio_point(points[i], pool, state, img, A, row);
#pragma unroll
        for (int k = 0; k < VC_N; k++) c[k] = outcome == k ? 1u : 0u;
        if (outcome_out) outcome_out[i] = (unsigned char)outcome;
    }
#pragma unroll
    for (int k = 0; k < VC_N; k++) {
        const unsigned v = srl_wave_sum(c[k]);
        if (lane == 0) s_cnt[wv][k] = v;
    }
    __syncthreads();
    if (rows_out) {
        for (int idx = tid; idx < 256 * 24; idx += 256) {
            const int p = idx / 24, k = idx - p * 24;
            const int at = blockIdx.x * 256 + p;
            if (at < A.n) rows_out[(size_t)at * 24 + k] = s_rows[p * VIO_STRIDE + k];
        }
    }
    // the wave's 64 points in list order, one sum per lane and round
    const bool photometric = A.mode == SRL_VIO_PHOTOMETRIC;
    const int rs = photometric ? 8 : 12, ncol = photometric ? 6 : 11;
    const double *mine = s_rows + wv * 64 * VIO_STRIDE;
    for (int comp = lane; comp < VIO_SUMS; comp += 64) {
        double sum = 0.0;
        if (comp == VIO_SUMS - 1) {
            for (int p = 0; p < 64; p++) sum += mine[p * VIO_STRIDE + 24];
        } else {
            const int a = comp < VIO_PAIRS ? c_pair_a[comp] : comp - VIO_PAIRS;
            const int b = comp < VIO_PAIRS ? c_pair_b[comp] : ncol;            // the r column follows the H columns
            if (a < ncol && b <= ncol && (comp >= VIO_PAIRS || b < ncol)) {
                for (int p = 0; p < 64; p++) {
                    const double *r = mine + p * VIO_STRIDE;
                    double t;
                    if (photometric) t = ((r[a] * r[7]) * r[b] + (r[8 + a] * r[15]) * r[8 + b]) + (r[16 + a] * r[23]) * r[16 + b];
                    else t = r[a] * r[b] + r[rs + a] * r[rs + b];
                    sum += t;
                }
            }
        }
        s_wave[wv][comp] = sum;
    }
    __syncthreads();
    // one row per workgroup, then the ticket
    unsigned long long *my_row = vpart + (size_t)blockIdx.x * VIO_ROW_WORDS;
    if (tid < VIO_SUMS) my_row[tid] = (unsigned long long)__double_as_longlong((s_wave[0][tid] + s_wave[1][tid]) + (s_wave[2][tid] + s_wave[3][tid]));
    else if (tid >= VIO_COUNTS && tid < VIO_COUNTS + VC_N) {
        const int k = tid - VIO_COUNTS;
        my_row[tid] = (unsigned long long)((s_cnt[0][k] + s_cnt[1][k]) + (s_cnt[2][k] + s_cnt[3][k]));
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(&vtot[VIO_TICKET], 1ull) == (unsigned long long)gridDim.x - 1ull ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    // the last workgroup: one thread per word over the rows in index order
    if (tid < VIO_SUMS) {
        double sum = 0.0;
        for (unsigned b = 0; b < gridDim.x; b++)
            sum += __longlong_as_double((long long)__hip_atomic_load(&vpart[(size_t)b * VIO_ROW_WORDS + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        vtot[tid] = (unsigned long long)__double_as_longlong(sum);
    } else if (tid >= VIO_COUNTS && tid < VIO_COUNTS + VC_N) {
        unsigned long long sum = 0;
        for (unsigned b = 0; b < gridDim.x; b++) sum += __hip_atomic_load(&vpart[(size_t)b * VIO_ROW_WORDS + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        vtot[tid] = sum;
    }
    if (tid == 0) vtot[VIO_TICKET] = 0ull;
}

}  // namespace

extern "C" int srl_color_map_vio_rows(srl_ctx *ctx, const srl_color_vio_args *args, const srl_color_vio_point *points, int n, srl_color_vio_sums *sums,
                                      double *rows, uint8_t *outcome) {
    if (sums) std::memset(sums, 0, sizeof *sums);
    if (!ctx || !args || !sums || n < 0 || n > SRL_COLOR_VIO_MAX_POINTS || (n > 0 && !points)) return SRL_ERR_BAD_ARG;
    if (args->mode != SRL_VIO_REPROJECTION && args->mode != SRL_VIO_PHOTOMETRIC) { ctx->err = "vio rows: mode is neither reprojection nor photometric"; return SRL_ERR_BAD_ARG; }
    srl_color_camera cam = args->cam;
    cam.fov_margin = 0.0;                 // ignored
    {
        bool finite = std::isfinite(args->time_td) && srl_color_cam_finite(&cam);
        for (int k = 0; k < 9; k++) finite = finite && std::isfinite(args->R_imu_camera[k]);
        if (!finite) { ctx->err = "vio rows: camera, time_td and R_imu_camera must be finite"; return SRL_ERR_BAD_ARG; }
    }
    { const int rc = srl_color_need_map(ctx); if (rc) return rc; }
    SrlColorMap *cm = ctx->color;
    const bool photometric = args->mode == SRL_VIO_PHOTOMETRIC;
    if (photometric && cm->img_rows == 0) { ctx->err = "no image uploaded (srl_color_image_upload)"; return SRL_ERR_NO_SWEEP; }
    { const int rc = srl_color_one_rank(ctx); if (rc) return rc; }
    VioArgs A;
    A.rows = photometric ? cm->img_rows : 0; A.cols = photometric ? cm->img_cols : 0;
    if (!srl_color_cam_args(&cam, A.rows, A.cols, &A.C)) { ctx->err = "vio rows: camera pose is not finite"; return SRL_ERR_BAD_ARG; }
    if (n == 0) return SRL_OK;
    SRL_DISARM(ctx);                      // a waiting launch holds a workgroup on every compute unit
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    A.time_td = args->time_td;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) A.Rt[r * 3 + c] = args->R_imu_camera[c * 3 + r];
    A.mode = args->mode; A.estimate_extrinsic = args->estimate_extrinsic ? 1 : 0; A.estimate_intrinsic = args->estimate_intrinsic ? 1 : 0;
    A.n = n; A.P = cm->num_points;

    const unsigned nblocks = (unsigned)((n + 255) / 256);
    // rows for the longest list at once, as before: the buffer never grows behind a synchronisation
    { const int rc = srl_wg_totals_reserve(ctx, cm->vio_tot, VIO_TICKET + 1, VIO_ROW_WORDS, SRL_COLOR_VIO_MAX_POINTS / 256); if (rc) return rc; }

    // page-locked scratch: the row of sums, the list, then the outcomes and the rows
    const size_t at_points = 1024, at_outcome = at_points + (size_t)n * sizeof(srl_color_vio_point);
    const size_t at_rows = (at_outcome + (size_t)n + 63) / 64 * 64, total = at_rows + (rows ? (size_t)n * 24 * sizeof(double) : 0);
    { const int rc = ensure_host_scratch(ctx, total); if (rc) return rc; }
    DevBuf b_points, b_rows, b_outcome;
    HIPCHK(ctx, b_points.alloc(ctx, (size_t)n * sizeof(srl_color_vio_point)));
    if (rows) HIPCHK(ctx, b_rows.alloc(ctx, (size_t)n * 24 * sizeof(double)));
    if (outcome) HIPCHK(ctx, b_outcome.alloc(ctx, (size_t)n));
    std::memcpy(ctx->h_scratch + at_points, points, (size_t)n * sizeof(srl_color_vio_point));
    HIPCHK(ctx, hipMemcpyAsync(b_points.p, ctx->h_scratch + at_points, (size_t)n * sizeof(srl_color_vio_point), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_vio_rows, dim3(nblocks), dim3(256), 0, st, b_points.as<srl_color_vio_point>(), cm->d_pool, cm->d_state, cm->img.d, A,
                       rows ? b_rows.as<double>() : nullptr, outcome ? b_outcome.as<unsigned char>() : nullptr, cm->vio_tot.d_rows, cm->vio_tot.d_tot);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch, cm->vio_tot.d_tot, VIO_ROW_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (outcome) HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch + at_outcome, b_outcome.p, (size_t)n, hipMemcpyDeviceToHost, st));
    if (rows) HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch + at_rows, b_rows.p, (size_t)n * 24 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (photometric) cm->img_pending = false;

    double h_sum[VIO_SUMS];
    unsigned long long h_cnt[VC_N];
    std::memcpy(h_sum, ctx->h_scratch, sizeof h_sum);
    std::memcpy(h_cnt, ctx->h_scratch + VIO_COUNTS * sizeof(unsigned long long), sizeof h_cnt);
    int comp = 0;
    for (int a = 0; a < 11; a++)
        for (int b = a; b < 11; b++, comp++) { sums->HtH[a * 11 + b] = h_sum[comp]; sums->HtH[b * 11 + a] = h_sum[comp]; }
    for (int a = 0; a < 11; a++) sums->Htr[a] = h_sum[VIO_PAIRS + a];
    sums->acc_residual = h_sum[VIO_SUMS - 1];
    sums->used = (int64_t)h_cnt[SRL_VIO_USED]; sums->few_views = (int64_t)h_cnt[SRL_VIO_FEW_VIEWS]; sums->behind = (int64_t)h_cnt[SRL_VIO_BEHIND];
    sums->outside = (int64_t)h_cnt[SRL_VIO_OUTSIDE]; sums->unknown = (int64_t)h_cnt[SRL_VIO_UNKNOWN];
    if (outcome) std::memcpy(outcome, ctx->h_scratch + at_outcome, (size_t)n);
    if (rows) std::memcpy(rows, ctx->h_scratch + at_rows, (size_t)n * 24 * sizeof(double));
    return SRL_OK;
}

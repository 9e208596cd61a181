// srl_color_project.h -- internal: what the consumers of the colour voxel map share (srl_color_render.hip, srl_color_select.hip,
// srl_color_vio.hip): cloudFrame::refreshPoseForProjection (src/lioOptimization.cpp:201-205) on the host, project3dPointInThisImage
// (:142-199) with if2dPointsAvailable (:48-60), |p - t_world_camera| and the sub-pixel colour getSubPixel<cv::Vec3b> (:71-97) on the device.  Every operation is an IEEE
// operation in the reference's order (-ffp-contract=off, sums of three as (a0 + a1) + a2).
#pragma once
#include "srl_ctx.h"
#include "srl_color_map.h"
#include "srl_hash.h"
#include "host/srl_la.h"

#include <cmath>

struct SrlCamArgs {
    double R[9], t_cw[3], t_wc[3];     // q_camera_world.toRotationMatrix(), t_camera_world, t_world_camera
    double fx, fy, cx, cy;
    double u_lo, u_hi, v_lo, v_hi;     // m cols + 1, (1 - m) cols, m rows + 1, (1 - m) rows
};

// false: a camera value is not finite
inline bool srl_color_cam_finite(const srl_color_camera *cam) {
    bool finite = std::isfinite(cam->fx) && std::isfinite(cam->fy) && std::isfinite(cam->cx) && std::isfinite(cam->cy) && std::isfinite(cam->fov_margin);
    for (int k = 0; k < 4; k++) finite = finite && std::isfinite(cam->q_world_camera[k]);
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(cam->t_world_camera[k]);
    return finite;
}
// refreshPoseForProjection and the bounds of if2dPointsAvailable (:55-56); false: the inverted pose is not finite
inline bool srl_color_cam_args(const srl_color_camera *cam, int rows, int cols, SrlCamArgs *A) {
    const srl::Quat q(cam->q_world_camera[0], cam->q_world_camera[1], cam->q_world_camera[2], cam->q_world_camera[3]);
    const srl::Quat q_cw = q.inverse();
    const srl::Mat3 R = q_cw.toRotationMatrix();
    const srl::Vec3 t_wc = srl::vec3(cam->t_world_camera[0], cam->t_world_camera[1], cam->t_world_camera[2]);
    const srl::Vec3 t_cw = (-R) * t_wc;
    for (int k = 0; k < 9; k++) A->R[k] = R.a[k];
    for (int k = 0; k < 3; k++) { A->t_cw[k] = t_cw[k]; A->t_wc[k] = t_wc[k]; }
    for (int k = 0; k < 12; k++) if (!std::isfinite(k < 9 ? A->R[k] : A->t_cw[k - 9])) return false;
    A->fx = cam->fx; A->fy = cam->fy; A->cx = cam->cx; A->cy = cam->cy;
    const double m = cam->fov_margin;
    A->u_lo = m * cols + 1; A->u_hi = (1 - m) * cols;
    A->v_lo = m * rows + 1; A->v_hi = (1 - m) * rows;
    return true;
}

#if defined(__HIPCC__)
enum { SRL_PROJ_OK = 0, SRL_PROJ_BEHIND = 1, SRL_PROJ_OUTSIDE = 2 };
// R_camera_world p + t_camera_world
__device__ __forceinline__ void srl_color_to_camera(const SrlCamArgs &A, double px, double py, double pz, double *xc, double *yc, double *zc) {
    *xc = ((A.R[0] * px + A.R[1] * py) + A.R[2] * pz) + A.t_cw[0];
    *yc = ((A.R[3] * px + A.R[4] * py) + A.R[5] * pz) + A.t_cw[1];
    *zc = ((A.R[6] * px + A.R[7] * py) + A.R[8] * pz) + A.t_cw[2];
}
// project3dPointInThisImage(p, u, v, nullptr, 1.0); u, v are written unless the point is behind the camera
__device__ __forceinline__ int srl_color_project(const SrlCamArgs &A, double px, double py, double pz, double *u_out, double *v_out) {
    double xc, yc, zc;
    srl_color_to_camera(A, px, py, pz, &xc, &yc, &zc);
    if (zc < 0.001) return SRL_PROJ_BEHIND;
    const double u = (xc * A.fx / zc + A.cx) * 1.0, v = (yc * A.fy / zc + A.cy) * 1.0;
    *u_out = u; *v_out = v;
    if (!((u >= A.u_lo) && (ceil(u) < A.u_hi) && (v >= A.v_lo) && (ceil(v) < A.v_hi))) return SRL_PROJ_OUTSIDE;
    return SRL_PROJ_OK;
}
// (p - t_world_camera).norm()
__device__ __forceinline__ double srl_color_depth(const SrlCamArgs &A, double px, double py, double pz) {
    const double dx = px - A.t_wc[0], dy = py - A.t_wc[1], dz = pz - A.t_wc[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}
// saturate_cast<uchar>(w * pixel): cvRound = round to nearest even, then the clamp (w in [0, 1]: the clamp is there for the letter)
__device__ __forceinline__ int srl_color_sat8(double w, int pixel) {
    const int r = (int)rint(w * (double)pixel);
    return r < 0 ? 0 : (r > 255 ? 255 : r);
}
__device__ __forceinline__ int srl_color_add8(int a, int b) { const int s = a + b; return s > 255 ? 255 : s; }
// getSubPixel<cv::Vec3b>(img, row, col, 0): per channel the saturating 8-bit sum, left to right, of four individually rounded bytes
// (SURVEY.md App. C).  The caller keeps 0 <= floor(row) < rows and 0 <= floor(col) < cols; the neighbour past the last row / column is
// read from the last one: the clamps only ever move a neighbour of weight 0
__device__ __forceinline__ void srl_color_sub_pixel(const unsigned char *img, int rows, int cols, double row, double col, int out[3]) {
    const int r0 = (int)floor(row), c0 = (int)floor(col);
    const double fr = row - (double)r0, fc = col - (double)c0;
    const int r1 = r0 + 1 < rows ? r0 + 1 : rows - 1, c1 = c0 + 1 < cols ? c0 + 1 : cols - 1;
    const double w00 = (1.0 - fr) * (1.0 - fc), w10 = fr * (1.0 - fc), w01 = (1.0 - fr) * fc, w11 = fr * fc;
    const unsigned char *q00 = img + ((size_t)r0 * cols + c0) * 3, *q10 = img + ((size_t)r1 * cols + c0) * 3;
    const unsigned char *q01 = img + ((size_t)r0 * cols + c1) * 3, *q11 = img + ((size_t)r1 * cols + c1) * 3;
#pragma unroll
    for (int k = 0; k < 3; k++)
        out[k] = srl_color_add8(srl_color_add8(srl_color_add8(srl_color_sat8(w00, q00[k]), srl_color_sat8(w10, q10[k])), srl_color_sat8(w01, q01[k])),
                                srl_color_sat8(w11, q11[k]));
}
#endif

// srl_color_project.h -- internal: what the consumers of the colour voxel map share (srl_color_render.hip, srl_color_select.hip):
// cloudFrame::refreshPoseForProjection (src/lioOptimization.cpp:201-205) on the host, project3dPointInThisImage (:142-199) with
// if2dPointsAvailable (:48-60) and |p - t_world_camera| on the device.  Every operation is an IEEE
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
// project3dPointInThisImage(p, u, v, nullptr, 1.0); u, v are written unless the point is behind the camera
__device__ __forceinline__ int srl_color_project(const SrlCamArgs &A, double px, double py, double pz, double *u_out, double *v_out) {
    const double xc = ((A.R[0] * px + A.R[1] * py) + A.R[2] * pz) + A.t_cw[0];
    const double yc = ((A.R[3] * px + A.R[4] * py) + A.R[5] * pz) + A.t_cw[1];
    const double zc = ((A.R[6] * px + A.R[7] * py) + A.R[8] * pz) + A.t_cw[2];
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
#endif

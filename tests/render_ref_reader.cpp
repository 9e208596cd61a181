// tests/render_ref_reader.cpp -- test-side driver of two pieces of the reference's own translation units that the harness of oracle/
// does not export: rgbPoint::updateRgb (src/cloudMap.cpp:59-100) and cloudFrame::refreshPoseForProjection + project3dPointInThisImage
// (src/lioOptimization.cpp:142-205).  tests/test_render_checker_reference.py compiles this file into its temporary directory against
// the include arrangement of oracle/Makefile's `refpath` target and links it to oracle/_ref/libref_path.so, in the manner of
// tests/color_ref_reader.cpp.  It holds no code of the reference; it only calls it and reads the private fields of rgbPoint.
//
// The standard headers come first: `#define private public` in front of <sstream> does not compile.
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>
#include <Eigen/Core>
#include <Eigen/Dense>

#define private public
#define protected public
#include "lioOptimization.h"
#undef private
#undef protected

extern "C" {

// One rgbPoint driven through n observations.  in: n x 5 doubles (colour 0, 1, 2, distance, time).  After every step: the return value,
// rgb[3], N_rgb (int32 x 5 per step), cov_rgb (float x 3 per step), observe_distance and last_observe_time (double x 2 per step).
void rrr_update_rgb(int n, const double *in, int32_t *out_int, float *out_cov, double *out_dbl) {
    rgbPoint pt(Eigen::Vector3d(1.0, 2.0, 3.0));
    const Eigen::Vector3d sigma(15, 15, 15);                 // image_obs_cov (rgbMapTracker.cpp:176, :208)
    for (int k = 0; k < n; ++k) {
        const double *o = in + (size_t)k * 5;
        const int r = pt.updateRgb(Eigen::Vector3d(o[0], o[1], o[2]), o[3], sigma, o[4]);
        out_int[(size_t)k * 5] = r;
        for (int i = 0; i < 3; ++i) { out_int[(size_t)k * 5 + 1 + i] = pt.rgb[i]; out_cov[(size_t)k * 3 + i] = pt.cov_rgb(i); }
        out_int[(size_t)k * 5 + 4] = pt.N_rgb;
        out_dbl[(size_t)k * 2] = pt.observe_distance;
        out_dbl[(size_t)k * 2 + 1] = pt.last_observe_time;
    }
}

// A cloudFrame whose state carries the camera (q as w, x, y, z; t; fx, fy, cx, cy; fov_margin) and the image size; every point (FP32
// positions, as a voxelBlock holds them) goes through getPosition()'s cast and project3dPointInThisImage(p, u, v, nullptr, 1.0).
// pose_out: q_camera_world (w, x, y, z) and t_camera_world as refreshPoseForProjection left them.
void rrr_project(const double *cam12, int rows, int cols, int n, const float *xyz, double *uv, uint8_t *accept, double *pose_out) {
    state st;
    st.q_world_camera = Eigen::Quaterniond(cam12[0], cam12[1], cam12[2], cam12[3]);
    st.t_world_camera = Eigen::Vector3d(cam12[4], cam12[5], cam12[6]);
    st.fx = cam12[7]; st.fy = cam12[8]; st.cx = cam12[9]; st.cy = cam12[10];
    st.fov_margin = cam12[11];
    std::vector<point3D> none;
    cloudFrame frame(none, &st);
    frame.image_rows = rows;
    frame.image_cols = cols;
    frame.refreshPoseForProjection();
    pose_out[0] = st.q_camera_world.w(); pose_out[1] = st.q_camera_world.x(); pose_out[2] = st.q_camera_world.y(); pose_out[3] = st.q_camera_world.z();
    for (int i = 0; i < 3; ++i) pose_out[4 + i] = st.t_camera_world(i);
    for (int k = 0; k < n; ++k) {
        const Eigen::Vector3f pos(xyz[(size_t)k * 3], xyz[(size_t)k * 3 + 1], xyz[(size_t)k * 3 + 2]);
        const Eigen::Vector3d p = pos.cast<double>();         // rgbPoint::getPosition()
        double u = 0.0, v = 0.0;
        accept[k] = frame.project3dPointInThisImage(p, u, v, nullptr, 1.0) ? 1 : 0;
        uv[(size_t)k * 2] = u; uv[(size_t)k * 2 + 1] = v;
    }
    frame.p_state = nullptr;                                  // the state is this function's, not the frame's
}

}  // extern "C"

// tests/select_ref_reader.cpp -- test-side driver of the pieces of rgbMapTracker::selectPointsForProjection (src/rgbMapTracker.cpp:45-152)
// that can be compiled against the stand-ins of oracle/: the function itself cannot (the include mirror shadows rgbMapTracker and the
// stand-in OpenCV has no Point2f).  The reference's own Hash_map_2d<int, int> / Hash_map_2d<int, float> (include/utility.h:143-) hold the
// mask, cloudFrame::project3dPointInThisImage (src/lioOptimization.cpp:142-199) projects, Eigen's norm() gives the depth; the mask update
// between them is written out here.  tests/test_select_checker_reference.py compiles this file into its temporary directory against the
// include arrangement of oracle/Makefile's `refpath` target and links it to oracle/_ref/libref_path.so, in the manner of
// tests/render_ref_reader.cpp.  What it holds of its own is a restatement of the loop's two steps the
// library cannot be asked for -- the key formation (round(u_f / minimum_dis) * minimum_dis into an int) and the mask condition with its two
// assignments, which follow rgbMapTracker.cpp:116-119 and :133-134 statement by statement on purpose; everything else is a call.
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

#include "lioOptimization.h"

extern "C" {

// cam12: q_world_camera (w, x, y, z), t_world_camera, fx, fy, cx, cy, fov_margin.  xyz: the candidates' FP32 positions in order.
// outcome per candidate: 255 not visited (the skip step), 1 beyond maximum_depth, 2 nearer than minimum_depth, 3 refused by the
// projection, 0 accepted -- then key (u, v) and depth are written; holder: 1 for the final holder of a cell.  Returns the number of cells.
int srr_select(const double *cam12, int rows, int cols, int n, const float *xyz, double minimum_dis, int skip_step, double minimum_depth, double maximum_depth,
               uint8_t *outcome, int32_t *key, double *depth_out, uint8_t *holder) {
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
    Hash_map_2d<int, int> mask_index;
    Hash_map_2d<int, float> mask_depth;
    int u, v;
    double u_f, v_f;
    std::memset(outcome, 255, (size_t)n);
    std::memset(holder, 0, (size_t)n);
    for (int point_index = 0; point_index < n; point_index += skip_step) {
        const Eigen::Vector3f pos(xyz[(size_t)point_index * 3], xyz[(size_t)point_index * 3 + 1], xyz[(size_t)point_index * 3 + 2]);
        const Eigen::Vector3d point_world = pos.cast<double>();        // rgbPoint::getPosition()
        const double depth = (point_world - st.t_world_camera).norm();
        if (depth > maximum_depth) { outcome[point_index] = 1; continue; }
        if (depth < minimum_depth) { outcome[point_index] = 2; continue; }
        if (!frame.project3dPointInThisImage(point_world, u_f, v_f, nullptr, 1.0)) { outcome[point_index] = 3; continue; }
        u = std::round(u_f / minimum_dis) * minimum_dis;
        v = std::round(v_f / minimum_dis) * minimum_dis;
        outcome[point_index] = 0;
        key[(size_t)point_index * 2] = u; key[(size_t)point_index * 2 + 1] = v;
        depth_out[point_index] = depth;
        if ((!mask_depth.if_exist(u, v)) || mask_depth.m_map_2d_hash_map[u][v] > depth) {
            mask_index.m_map_2d_hash_map[u][v] = point_index;
            mask_depth.m_map_2d_hash_map[u][v] = (float)depth;
        }
    }
    int cells = 0;
    for (auto &col : mask_index.m_map_2d_hash_map)
        for (auto &cell : col.second) { holder[cell.second] = 1; ++cells; }
    frame.p_state = nullptr;                                           // the state is this function's, not the frame's
    return cells;
}

}  // extern "C"

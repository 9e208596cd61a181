// tests/track_ref_reader.cpp -- test-side driver of the pieces of opticalFlowTracker::updateAndAppendTrackPoints
// (src/opticalFlowTracker.cpp:13-102) that can be compiled against the stand-ins of oracle/: the function itself cannot (it needs
// OpenCV's Point2f and the include mirror shadows the vision stage).  The reference's own Hash_map_2d<int, float> (include/utility.h:143-)
// holds the occupancy mask, cloudFrame::project3dPointInThisImage (src/lioOptimization.cpp:142-199) projects, Eigen's norm() gives the
// error and the depth the mask stores; the loops' remaining statements are restated here line by line, on purpose.
// tests/test_track_checker_reference.py compiles this file into its temporary directory against the include arrangement of
// oracle/Makefile's `refpath` target and links it to oracle/_ref/libref_path.so, in the manner of tests/select_ref_reader.cpp.
// The map keyed by pointer is a list walked in the caller's order with an id per element (the id stands for the pointer: `find` is a
// search by id); an element's is_out_lier_count travels with it.
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

// cam12: q_world_camera (w, x, y, z), t_world_camera, fx, fy, cx, cy, fov_margin.  Tracked element i: id_t[i], FP32 position xyz_t, pixel
// uv_t (two floats), count_t (is_out_lier_count on entry).  Out per tracked element: state_t 0 kept / 1 kept with the count raised /
// 2 erased, count_out, error_out.  Candidate j: id_c[j], xyz_c.  Out per candidate: state_c 1 found in the map (:69-73), 0 added (uv_c
// written: the two casts to float), 3 refused by the projection, 4 cell occupied, 6 not reached (behind the break).  Returns the size of
// the map behind the second loop.
int trr_update(const double *cam12, int rows, int cols, double mini_distance, unsigned int maximum_tracked_points, int n, const int32_t *id_t, const float *xyz_t,
               const float *uv_t, const int32_t *count_t, uint8_t *state_t, int32_t *count_out, double *error_out, int nc, const int32_t *id_c,
               const float *xyz_c, uint8_t *state_c, float *uv_c) {
    state st;
    st.q_world_camera = Eigen::Quaterniond(cam12[0], cam12[1], cam12[2], cam12[3]);
    st.t_world_camera = Eigen::Vector3d(cam12[4], cam12[5], cam12[6]);
    st.fx = cam12[7]; st.fy = cam12[8]; st.cx = cam12[9]; st.cy = cam12[10];
    st.fov_margin = cam12[11];
    std::vector<point3D> none;
    cloudFrame frame(none, &st);
    cloudFrame *p_frame = &frame;
    frame.image_rows = rows;
    frame.image_cols = cols;
    frame.refreshPoseForProjection();

    double u_d, v_d;
    int u_i, v_i;
    double max_allow_reproject_error = 2.0 * p_frame->image_cols / 320.0;
    Hash_map_2d<int, float> map_2d_points_occupied;
    std::map<int32_t, int> in_map;                                         // id -> present (the keys of map_rgb_points_in_last_image_pose)

    for (int i = 0; i < n; i++) {
        Eigen::Vector3d point_3d = Eigen::Vector3f(xyz_t[(size_t)i * 3], xyz_t[(size_t)i * 3 + 1], xyz_t[(size_t)i * 3 + 2]).cast<double>();
        int is_out_lier_count = count_t[i];
        bool res = p_frame->project3dPointInThisImage(point_3d, u_d, v_d, nullptr, 1.0);
        u_i = std::round(u_d / mini_distance) * mini_distance;
        v_i = std::round(v_d / mini_distance) * mini_distance;
        double error = Eigen::Vector2d(u_d - uv_t[(size_t)i * 2], v_d - uv_t[(size_t)i * 2 + 1]).norm();
        error_out[i] = error;
        state_t[i] = 0;
        if (error > max_allow_reproject_error) {
            is_out_lier_count++;
            state_t[i] = 1;
            if ((is_out_lier_count > 1) || (error > max_allow_reproject_error * 2)) {
                is_out_lier_count = 0;
                count_out[i] = is_out_lier_count;
                state_t[i] = 2;
                continue;
            }
        } else {
            is_out_lier_count = 0;
        }
        count_out[i] = is_out_lier_count;
        in_map[id_t[i]] = 1;
        if (res) {
            double depth = (point_3d - p_frame->p_state->t_world_camera).norm();
            if (map_2d_points_occupied.if_exist(u_i, v_i) == false) {
                map_2d_points_occupied.insert(u_i, v_i, depth);
            }
        }
    }

    std::memset(state_c, 6, (size_t)nc);
    for (int i = 0; i < nc; i++) {
        if (in_map.find(id_c[i]) != in_map.end()) {
            state_c[i] = 1;
            continue;
        }
        Eigen::Vector3d point_3d = Eigen::Vector3f(xyz_c[(size_t)i * 3], xyz_c[(size_t)i * 3 + 1], xyz_c[(size_t)i * 3 + 2]).cast<double>();
        bool res = p_frame->project3dPointInThisImage(point_3d, u_d, v_d, nullptr, 1.0);
        u_i = std::round(u_d / mini_distance) * mini_distance;
        v_i = std::round(v_d / mini_distance) * mini_distance;
        state_c[i] = 3;
        if (res) {
            double depth = (point_3d - p_frame->p_state->t_world_camera).norm();
            state_c[i] = 4;
            if (map_2d_points_occupied.if_exist(u_i, v_i) == false) {
                map_2d_points_occupied.insert(u_i, v_i, depth);
                in_map[id_c[i]] = 1;
                uv_c[(size_t)i * 2] = (float)u_d; uv_c[(size_t)i * 2 + 1] = (float)v_d;      // cv::Point2f(u_d, v_d)
                state_c[i] = 0;
            }
        }
        if (in_map.size() >= maximum_tracked_points) {
            break;
        }
    }
    frame.p_state = nullptr;                                               // the state is this function's, not the frame's
    return (int)in_map.size();
}

}  // extern "C"

// tests/color_ref_reader.cpp -- test-side reader of what the reference's own addPointsToMap leaves behind for the rendering side:
// lioOptimization::color_voxel_map, hashmap_3d_points, voxels_recent_visited_temp (include/lioOptimization.h:275-291, private) and
// img_pro->map_tracker->rgb_points_vec.  The harness of oracle/ runs the reference's translation units but exports none of these;
// tests/test_color_checker_reference.py compiles this file into its temporary directory against the same include arrangement as
// oracle/Makefile's `refpath` target and reads the node behind ref_node_lio_ptr().  Nothing of it is built by build() or committed as
// a binary; it holds no code of the reference.
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

static const lioOptimization &L(const void *p) { return *static_cast<const lioOptimization *>(p); }

extern "C" {

// voxels, stored points, registered points, grid cells
void crr_sizes(const void *lio, int64_t out[4]) {
    lioOptimization &l = const_cast<lioOptimization &>(L(lio));
    int64_t pts = 0;
    for (auto it = l.color_voxel_map.begin(); it != l.color_voxel_map.end(); ++it) pts += it->second.NumPoints();
    out[0] = (int64_t)l.color_voxel_map.size();
    out[1] = pts;
    out[2] = (int64_t)l.img_pro->map_tracker->rgb_points_vec.size();
    out[3] = (int64_t)l.hashmap_3d_points.total_size();
}

// the map in the container's iteration order: keys (V x 3), counts (V), last_visited_time (V), and the points voxel after voxel in slot
// order (P x 3, the FP32 the block holds)
void crr_map(const void *lio, int16_t *keys, int32_t *counts, double *times, float *xyz) {
    lioOptimization &l = const_cast<lioOptimization &>(L(lio));
    size_t v = 0, p = 0;
    for (auto it = l.color_voxel_map.begin(); it != l.color_voxel_map.end(); ++it, ++v) {
        keys[3 * v] = it->first.x; keys[3 * v + 1] = it->first.y; keys[3 * v + 2] = it->first.z;
        voxelBlock &block = it.value();
        counts[v] = block.NumPoints();
        times[v] = block.last_visited_time;
        for (int s = 0; s < block.NumPoints(); ++s, ++p) {
            const Eigen::Vector3d q = block.points[s].getPosition();
            xyz[3 * p] = (float)q[0]; xyz[3 * p + 1] = (float)q[1]; xyz[3 * p + 2] = (float)q[2];
        }
    }
}

// rgb_points_vec in order: position, and the voxel and slot the pointer points into (-1 when it points into no block of the map)
void crr_registered(const void *lio, double size_voxel_map, float *xyz, int16_t *keys, int32_t *slot) {
    lioOptimization &l = const_cast<lioOptimization &>(L(lio));
    const std::vector<rgbPoint *> &vec = l.img_pro->map_tracker->rgb_points_vec;
    for (size_t i = 0; i < vec.size(); ++i) {
        const Eigen::Vector3d q = vec[i]->getPosition();
        xyz[3 * i] = (float)q[0]; xyz[3 * i + 1] = (float)q[1]; xyz[3 * i + 2] = (float)q[2];
        const short kx = static_cast<short>(q[0] / size_voxel_map), ky = static_cast<short>(q[1] / size_voxel_map), kz = static_cast<short>(q[2] / size_voxel_map);
        keys[3 * i] = kx; keys[3 * i + 1] = ky; keys[3 * i + 2] = kz;
        slot[i] = -1;
        auto it = l.color_voxel_map.find(voxel(kx, ky, kz));
        if (it != l.color_voxel_map.end()) {
            voxelBlock &block = it.value();
            for (int s = 0; s < block.NumPoints(); ++s) if (&block.points[s] == vec[i]) slot[i] = s;
        }
    }
}

// hashmap_3d_points: every cell (x, y, z) and the index in rgb_points_vec of the point it holds (-1: none of them)
int64_t crr_grid(const void *lio, int64_t *cells, int32_t *index, int64_t capacity) {
    lioOptimization &l = const_cast<lioOptimization &>(L(lio));
    const std::vector<rgbPoint *> &vec = l.img_pro->map_tracker->rgb_points_vec;
    std::unordered_map<const rgbPoint *, int32_t> at;
    for (size_t i = 0; i < vec.size(); ++i) at[vec[i]] = (int32_t)i;
    int64_t n = 0;
    for (auto &a : l.hashmap_3d_points.m_map_3d_hash_map)
        for (auto &b : a.second)
            for (auto &c : b.second) {
                if (n < capacity) {
                    cells[3 * n] = a.first; cells[3 * n + 1] = b.first; cells[3 * n + 2] = c.first;
                    auto f = at.find(c.second);
                    index[n] = f == at.end() ? -1 : f->second;
                }
                ++n;
            }
    return n;
}

// voxels_recent_visited_temp (to_rendering = false in the harness's call: the list accumulates)
int64_t crr_visited(const void *lio, int32_t *out, int64_t capacity) {
    const std::vector<voxelId> &v = L(lio).voxels_recent_visited_temp;
    for (size_t i = 0; i < v.size() && (int64_t)i < capacity; ++i) { out[3 * i] = v[i].kx; out[3 * i + 1] = v[i].ky; out[3 * i + 2] = v[i].kz; }
    return (int64_t)v.size();
}

}  // extern "C"

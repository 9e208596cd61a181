// tests/cloud_export_ref_reader.cpp -- test-side driver of the pieces of the reference that its three coloured-cloud loops are made of:
// lioOptimization::pubColorPoints (src/lioOptimization.cpp:1210-1241), threadPubColorPoints (:1243-1344) and saveColorPoints (:1386-1426).
// The functions themselves cannot be compiled against the stand-ins of oracle/ (they need ROS publishers, pcl::toROSMsg and the PCD
// writer).  What can be asked of the reference's own translation units is: rgbPoint's constructor (src/cloudMap.cpp:5-9), updateRgb
// (:59-100), which brings every point to its state, getPosition() (:26-29), getRgb() (:41-44) and the public N_rgb.
// tests/test_cloud_export_checker_reference.py compiles this file into its temporary directory against the include arrangement of
// oracle/Makefile's `refpath` target and links it to oracle/_ref/libref_path.so, in the manner of tests/render_ref_reader.cpp.  What it
// holds of its own is the loops' index arithmetic -- `i = 0; i < size; i++` (:1217, :1275), `i = size - 1; i > 0; i--` (:1398) and the
// topic counter (:1295-1316, :1319-1336) -- restated by hand around those calls, statement by statement on purpose; the comparison with
// N_rgb and the six assignments follow :1221-1230 / :1281-1292 / :1404-1416.  The record is the stand-in pcl::PointXYZRGB's fields packed
// as x y z and b, g, r, a; the stand-in is not PCL, and `a` is set to the 255 of PCL's constructor here.
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

namespace {
struct Record { float x, y, z; uint8_t b, g, r, a; };
static_assert(sizeof(Record) == 16, "16 bytes");

void pack(const pcl::PointXYZRGB &q, Record *out) {
    out->x = q.x; out->y = q.y; out->z = q.z;
    out->b = q.b; out->g = q.g; out->r = q.r; out->a = 255;
}
}  // namespace

extern "C" {

// n points: xyz (FP32, as a voxelBlock hands them to the constructor); obs_start[n + 1] into obs (5 doubles each: colour 0, 1, 2,
// distance, time): point k is brought to its state by updateRgb over obs[obs_start[k] .. obs_start[k + 1]).
// which: 0 pubColorPoints, 1 threadPubColorPoints (topic_sizes / n_topics receive the sizes of the topics sent with
// number_of_points_per_topic points per topic), 2 saveColorPoints.  Returns the number of records; index[k] = i of record k.
long cer_cloud(int n, const float *xyz, const int64_t *obs_start, const double *obs, int which, int pub_point_minimum_views,
               int number_of_points_per_topic, Record *records, int32_t *index, int32_t *topic_sizes, int32_t *n_topics) {
    const Eigen::Vector3d sigma(15, 15, 15);                 // image_obs_cov (rgbMapTracker.cpp:176, :208)
    std::vector<rgbPoint *> rgb_points_vec;
    for (int k = 0; k < n; ++k) {
        rgbPoint *pt = new rgbPoint(Eigen::Vector3d(xyz[(size_t)k * 3], xyz[(size_t)k * 3 + 1], xyz[(size_t)k * 3 + 2]));
        for (int64_t j = obs_start[k]; j < obs_start[k + 1]; ++j) {
            const double *o = obs + (size_t)j * 5;
            pt->updateRgb(Eigen::Vector3d(o[0], o[1], o[2]), o[3], sigma, o[4]);
        }
        rgb_points_vec.push_back(pt);
    }
    long point_count = 0;
    if (which == 0) {
        for (int i = 0; i < rgb_points_vec.size(); i++) {                                     // :1217
            rgbPoint *p_point = rgb_points_vec[i];
            if (p_point->N_rgb < pub_point_minimum_views) continue;
            pcl::PointXYZRGB rgb_point;
            rgb_point.x = p_point->getPosition()[0];
            rgb_point.y = p_point->getPosition()[1];
            rgb_point.z = p_point->getPosition()[2];
            rgb_point.r = p_point->getRgb()[2];
            rgb_point.g = p_point->getRgb()[1];
            rgb_point.b = p_point->getRgb()[0];
            pack(rgb_point, records + point_count);
            index[point_count++] = i;
        }
    } else if (which == 1) {
        int points_size = rgb_points_vec.size();
        int pub_index_size = 0;
        int cur_topic_index = 0;
        for (int i = 0; i < points_size; i++) {                                               // :1275
            int N_rgb = rgb_points_vec[i]->N_rgb;
            if (N_rgb < pub_point_minimum_views) continue;
            pcl::PointXYZRGB q;
            q.x = rgb_points_vec[i]->getPosition()[0];
            q.y = rgb_points_vec[i]->getPosition()[1];
            q.z = rgb_points_vec[i]->getPosition()[2];
            q.r = rgb_points_vec[i]->getRgb()[2];
            q.g = rgb_points_vec[i]->getRgb()[1];
            q.b = rgb_points_vec[i]->getRgb()[0];
            pack(q, records + point_count);
            index[point_count++] = i;
            pub_index_size++;
            if (pub_index_size == number_of_points_per_topic) {                               // :1297
                topic_sizes[cur_topic_index] = number_of_points_per_topic;
                pub_index_size = 0;
                cur_topic_index++;
            }
        }
        topic_sizes[cur_topic_index] = pub_index_size;                                        // :1319, :1334
        cur_topic_index++;
        *n_topics = cur_topic_index;
    } else {
        long point_size = rgb_points_vec.size();
        for (long i = point_size - 1; i > 0; i--) {                                           // :1398
            int N_rgb = rgb_points_vec[i]->N_rgb;
            if (N_rgb < pub_point_minimum_views) continue;
            pcl::PointXYZRGB q;
            q.x = rgb_points_vec[i]->getPosition()[0];
            q.y = rgb_points_vec[i]->getPosition()[1];
            q.z = rgb_points_vec[i]->getPosition()[2];
            q.r = rgb_points_vec[i]->getRgb()[2];
            q.g = rgb_points_vec[i]->getRgb()[1];
            q.b = rgb_points_vec[i]->getRgb()[0];
            pack(q, records + point_count);
            index[point_count++] = (int32_t)i;
        }
    }
    for (rgbPoint *p : rgb_points_vec) delete p;
    return point_count;
}

}  // extern "C"

// lioOptimization.h (host mirror) -- the reference's class surface for the LIO scan-matching path
// (include/lioOptimization.h:334-357: optimize / buildPlaneResiduals / updateIEKF /
// computeNeighborhoodDistribution / searchNeighbors / addPointToMap / addPointsToMap / removePointsFarFromLocation / mapSize),
// forwarding through the C-ABI of include/srlivo_hip.h to the gfx950 kernels.  ROS I/O, sensor
// decoding and the vision stage of the reference class are out of scope.
#pragma once
#include "../../../include/srlivo_hip.h"
#include "cloudMap.h"
#include "eskfEstimator.h"
#include "parameters.h"
#include "state.h"
#include "utility.h"

#include <functional>
#include <string>
#include <vector>

// When Eigen is on the include path (the reference's own build: CMakeLists.txt:51) the members whose signatures carry
// Eigen types -- computeNeighborhoodDistribution and searchNeighbors, include/lioOptimization.h:340-343, and
// removePointsFarFromLocation, :355 -- are ALSO
// declared with exactly those types, so call sites written against the reference header compile unchanged.  They convert
// at the boundary and forward to the srl:: versions (the image this was built in has no Eigen: tests/stub_eigen holds the
// minimal stand-in the signature test compiles against).  -DSRL_NO_EIGEN switches the block off.
#if defined(__has_include) && !defined(SRL_NO_EIGEN)
#if __has_include(<Eigen/Core>)
#include <Eigen/Core>
#include <Eigen/StdVector>
#define SRL_HAVE_EIGEN 1
#endif
#endif

namespace srlivo {

extern srl::Vec3 G;        // include/utility.h:43 (written by updateIEKF, optimize.cpp:260)
extern double G_norm;      // include/utility.h:44

class cloudFrame {         // include/lioOptimization.h:80-92 (LIO members only)
public:
    double time_sweep_begin = 0, time_sweep_end = 0;
    double time_frame_begin = 0, time_frame_end = 0;
    int id = 0;            // the index in all_cloud_frame
    int sub_id = 0;
    int frame_id = 0;
    double offset_begin = 0, offset_end = 0, dt_offset = 0;
    state *p_state = nullptr;
    std::vector<point3D> point_frame;
    bool success = true;
    cloudFrame(std::vector<point3D> &point_frame_, state *p_state_) : p_state(p_state_), point_frame(point_frame_) {}
};

struct Neighborhood {      // include/lioOptimization.h:127-137
    srl::Vec3 center = srl::Vec3::Zero();
    srl::Vec3 normal = srl::Vec3::Zero();
    srl::Mat3 covariance = srl::Mat3::Identity();
    double a2D = 1.0;
};

#ifdef SRL_HAVE_EIGEN
struct NeighborhoodEigen {  // include/lioOptimization.h:127-137 with the reference's member types
    Eigen::Vector3d center = Eigen::Vector3d::Zero();
    Eigen::Vector3d normal = Eigen::Vector3d::Zero();
    Eigen::Matrix3d covariance = Eigen::Matrix3d::Identity();
    double a2D = 1.0;
};
#endif

struct optimizeSummary {   // include/lioOptimization.h:181-188
    bool success = false;
    int num_residuals_used = 0;
    std::string error_log;
};

struct iterationLog {      // ours: per-ESIKF-iteration tap for the parity tests
    srl_normal_eq neq;
    srl::Vec17 d_x;
};

// source of the per-iteration normal equations: the HIP backend by default; an external provider lets
// the identical host update run on equations reduced elsewhere (multi-process CPU tests).
typedef int (*normal_eq_provider)(const srl_frame *frame, const srl_icp_opts *opts, srl_normal_eq *out, void *user);

void subSampleFrame(std::vector<point3D> &frame, double size_voxel);                                     // utility.cpp:167-186
void gridSampling(const std::vector<point3D> &frame, std::vector<point3D> &keypoints, double size_voxel_subsampling);  // utility.cpp:188-201

class lioOptimization {
public:
    // device >= 0: creates the HIP context (throws std::runtime_error when no GPU -- there is no CPU path).
    // device < 0 : host-only object, usable solely with setNormalEqProvider().
    explicit lioOptimization(int device);
    ~lioOptimization();
    lioOptimization(const lioOptimization &) = delete;
    lioOptimization &operator=(const lioOptimization &) = delete;

    // ---- reference surface (include/lioOptimization.h:334-357) ----
    optimizeSummary optimize(cloudFrame *p_frame, const icpOptions &cur_icp_options, double sample_voxel_size);
    optimizeSummary buildPlaneResiduals(const icpOptions &cur_icp_options, voxelHashMap &voxel_map_temp,
                                        std::vector<point3D> &keypoints, std::vector<planeParam> &plane_residuals,
                                        cloudFrame *p_frame, double &loss_sum);
    optimizeSummary updateIEKF(const icpOptions &cur_icp_options, voxelHashMap &voxel_map_temp,
                               std::vector<point3D> &keypoints, cloudFrame *p_frame);
    Neighborhood computeNeighborhoodDistribution(const std::vector<srl::Vec3> &points);
    std::vector<srl::Vec3> searchNeighbors(voxelHashMap &map, const srl::Vec3 &point, int nb_voxels_visited,
                                           double size_voxel_map, int max_num_neighbors, int threshold_voxel_capacity = 1,
                                           std::vector<voxel> *voxels = nullptr);
#ifdef SRL_HAVE_EIGEN
    // the reference's own signatures (include/lioOptimization.h:340-343), forwarding to the two members above
    NeighborhoodEigen computeNeighborhoodDistribution(const std::vector<Eigen::Vector3d, Eigen::aligned_allocator<Eigen::Vector3d>> &points) {
        std::vector<srl::Vec3> p(points.size());
        for (size_t i = 0; i < points.size(); i++) p[i] = srl::vec3(points[i][0], points[i][1], points[i][2]);
        const Neighborhood nb = computeNeighborhoodDistribution(p);
        NeighborhoodEigen out;
        for (int i = 0; i < 3; i++) { out.center[i] = nb.center[i]; out.normal[i] = nb.normal[i]; for (int j = 0; j < 3; j++) out.covariance(i, j) = nb.covariance(i, j); }
        out.a2D = nb.a2D;
        return out;
    }
    std::vector<Eigen::Vector3d, Eigen::aligned_allocator<Eigen::Vector3d>> searchNeighbors(voxelHashMap &map, const Eigen::Vector3d &point,
            int nb_voxels_visited, double size_voxel_map, int max_num_neighbors, int threshold_voxel_capacity = 1, std::vector<voxel> *voxels = nullptr) {
        const std::vector<srl::Vec3> r = searchNeighbors(map, srl::vec3(point[0], point[1], point[2]), nb_voxels_visited, size_voxel_map,
                                                         max_num_neighbors, threshold_voxel_capacity, voxels);
        std::vector<Eigen::Vector3d, Eigen::aligned_allocator<Eigen::Vector3d>> out(r.size());
        for (size_t i = 0; i < r.size(); i++) out[i] = Eigen::Vector3d(r[i][0], r[i][1], r[i][2]);
        return out;
    }
#endif
    void addPointToMap(voxelHashMap &map, const srl::Vec3 &point, double voxel_size, int max_num_points_in_voxel,
                       double min_distance_points, int min_num_points, cloudFrame *p_frame);
    void addPointsToMap(voxelHashMap &map, cloudFrame *p_frame, double voxel_size, int max_num_points_in_voxel,
                        double min_distance_points, int min_num_points = 0, bool to_rendering = false);
    // lioOptimization.cpp:556-572: srl_map_remove_far (the survivors are renumbered in creation order)
    void removePointsFarFromLocation(voxelHashMap &map, const srl::Vec3 &location, double distance);
#ifdef SRL_HAVE_EIGEN
    // the reference's own signature (include/lioOptimization.h:355), so that the node's call at lioOptimization.cpp:1032 compiles as written
    void removePointsFarFromLocation(voxelHashMap &map, const Eigen::Vector3d &location, double distance) {
        removePointsFarFromLocation(map, srl::vec3(location[0], location[1], location[2]), distance);
    }
#endif
    size_t mapSize(const voxelHashMap &map);

    // stateInitialization (lioOptimization.cpp:895-990): pose prior of the next frame from the last two frames of
    // all_cloud_frame (constant velocity), the filter (INIT_IMU once initial_flag is set) or the last pose.
    void stateInitialization(state *cur_state);
    int index_frame = 1;                                                 // lioOptimization.cpp:355
    enum StateInitialization { INIT_IMU = 0, INIT_CONSTANT_VELOCITY = 1 };   // include/utility.h:88-92
    int initialization = INIT_IMU;                                      // odometry_options.initialization (both yaml: "imu")

    // sweep reconstruction (lioOptimization.cpp:786-893).  The per-point math of distortFrameByConstant/-ByImu and
    // transformAllImuPoint runs on the device over the whole cut sweep (srl_frame_undistort); the two std::shuffle calls
    // (one default-seeded mt19937_64) run on the host over index arrays; subSampleFrame's grouping and tr1 iteration
    // order run on the device (srl_frame_subsample), and the surviving points become the resident frame
    // (srl_frame_take_subsampled), so optimizeResident(p_frame, ...) and commitFrame() need no further upload.
    // point_frame of the returned frame is filled from the device results (m points, not the n of the sweep).
    // device_subsample = false: the grouping on the host over the n-point downloads and srl_frame_take (the same bits;
    // kept to compare the two in one process, srl_lio_set_device_subsample).
    void makePointTimestamp(std::vector<point3D> &sweep, double time_begin, double time_end);
    cloudFrame *buildFrame(std::vector<point3D> &cut_sweep, state *cur_state, double timestamp_begin, double timestamp_offset);
    bool device_subsample = true;
    // The sweep of the next buildFrame is the resident cut of the device point queue (srl_points_cut), not cut_sweep: the time rewrite and
    // the undistortion run on it where it lies (srl_frame_undistort_cut), the device sub-sample follows unchanged, and the point3D time
    // fields of the kept points come back through srl_frame_point_times.  Set for one measurement by srl_lio_run_measurement_queued.
    bool sweep_from_queue = false;
    // cloudProcessing's options as srl_livox_decode reads them (setN_SCANS, setTimeUnit, setBlind, setPointFilterNum), and what
    // lioOptimization::livoxHandler (lioOptimization.cpp:593-601) and cloudProcessing::livoxHandler keep between messages
    srl_livox_opts lidar_options = {};                                   // (the reference has no defaults for three of the four)
    bool lidar_options_set = false;
    // ... and as srl_pc2_decode reads them for lioOptimization::standardCloudHandler (:583-591): setLidarType and setScanRate come with them.
    // Both handlers share the two times below and the queue, as they share cloud_pro and point_buffer upstream.
    srl_pc2_opts pc2_options = {};
    bool pc2_options_set = false;
    double last_time_lidar = -1.0;                                       // lioOptimization.cpp:383
    double last_end_time = -1.0;                                         // cloudProcessing.cpp:9
    // optimize() on the frame buildFrame left resident in HBM
    optimizeSummary optimizeBuiltFrame(cloudFrame *p_frame, const icpOptions &cur_icp_options, double sample_voxel_size,
                                       std::vector<int> *keypoint_index = nullptr);
    std::vector<imuState> imu_states;                                    // lioOptimization.h:263
    bool point_time_enable = true;                                       // cloud_pro->isPointTimeEnable()
    enum MotionCompensation { IMU = 0, CONSTANT_VELOCITY = 1 };          // include/utility.h:82-86
    int motion_compensation = CONSTANT_VELOCITY;                         // odometry_options (parameters.h:84)
    double init_voxel_size = 0.2, voxel_size = 0.5;                      // parameters.h:62,70
    int init_num_frames = 20;                                            // parameters.h:66

    // ---- ROS-free replay driver: the LIO part of run() / process() / stateEstimation() ----
    // (lioOptimization.cpp:1427-1584, :1036-1133, :991-1034).  Image / rendering / publishing / file output are out
    // of scope; recordSinglePose's rows are kept in `trajectory` instead of pose.txt.
    struct imuSample { double time; srl::Vec3 acc, gyr; };
    struct Measurement {
        double time_frame = 0;                         // measurement.time_image
        std::vector<imuSample> imu;                    // measurement.imu_measurements
        std::vector<point3D> lidar_points;             // raw_point, point (= raw_point), timestamp
        double time_sweep_begin = 0, time_sweep_offset = 0;   // measurement.time_sweep
    };
    struct poseRecord { double time; srl::Vec3 translation; srl::Quat rotation; };
    // returns false while the filter is still initialising (no frame processed)
    bool runMeasurement(Measurement &measurement, optimizeSummary *summary = nullptr);
    void process(std::vector<point3D> &cut_sweep, double timestamp_begin, double timestamp_offset, optimizeSummary *summary = nullptr);
    optimizeSummary stateEstimation(cloudFrame *p_frame);
    // the camera half of process() (lioOptimization.cpp:1053-1086), between stateEstimation (whatever its summary says: the reference does not look at it) and the sliding window: the
    // frame is the newest of all_cloud_frame.  Empty unless a caller with an image sets it for one measurement (srl_lio_run_measurement_image)
    std::function<void(cloudFrame *)> camera_half;
    void releaseFrames();
    icpOptions optimize_options;                                         // odometry_options.optimize_options
    double init_sample_voxel_size = 1.0, sample_voxel_size = 1.5;        // parameters.h:64,72
    int num_for_initialization = 10;                                     // parameters.h:68
    int max_num_points_in_voxel = 20;                                    // parameters.h:76
    double min_distance_points = 0.1;                                    // parameters.h:78
    bool download_frame_points = true;       // fill point3D::point of the frame after the device commit
    std::vector<poseRecord> trajectory;
    std::vector<imuMeas> imu_meas;
    double current_time = -1, last_time_frame = -1, dt_sum = 0;         // lioOptimization.cpp:353-357
    int last_frame_keypoints = 0, last_frame_points = 0, last_points_added = 0;
    // points_world (include/lioOptimization.h:262; filled by addPointToPcl at lioOptimization.cpp:429, published as cloud_world at :552-553):
    // the points the last addPointsToMap / commitFrame APPENDED to voxels that already existed, in frame order, as pcl::PointXYZI payloads.
    // Cleared at the start of both; filled only while the switch is on (srl_map_insert_report / srl_frame_commit_report, which are
    // synchronous: with the switch off process() keeps its deferred commit).  The reference clears the cloud after publishing it; here
    // it stays until the next insertion so that the caller can publish it.
    std::vector<srl_cloud_point> points_world;
    void setCollectPointsWorld(bool on) { collect_points_world = on; }
    // The colour half of addPointsToMap (lioOptimization.cpp:538-539: addPointToColorMap for every add_point_step-th point), opt-in: once
    // setColorMapOptions has created the device colour map (srl_color_map_create with mapOptions, parameters.h:98-106), addPointsToMap and
    // commitFrame run srl_color_map_insert behind the LiDAR insertion -- commitFrame on the world points it left in HBM -- and keep the
    // lists of lioOptimization.cpp:523-550 as the reference does, `to_rendering` included.  color_stored: the records of the last
    // insertion (which point went to which voxel and slot, and under which index it was registered), for the caller's own rgbPoint
    // objects.  Without the options: exactly the LiDAR insertion.  The calls are synchronous.
    struct voxelId { int kx, ky, kz; };                                  // cloudMap.h:88
    void setColorMapOptions(const srl_color_opts &o);
    bool colorMapEnabled() const { return color_map_enabled; }
    double time_last_process = -1e5;                                     // img_pro->time_last_process (imageProcessing.cpp:6; the vision stage's, set by the caller)
    bool to_rendering = false;                                           // include/lioOptimization.h: what stateEstimation hands to addPointsToMap (:1027)
    double commit_time_sweep_end = 0.0;                                  // p_frame->time_sweep_end of the frame commitFrame inserts (stateEstimation sets it)
    std::vector<voxelId> voxels_recent_visited_temp;                     // include/lioOptimization.h:291
    std::vector<voxelId> voxels_recent_visited;                          // img_pro->map_tracker->voxels_recent_visited (rgbMapTracker.h:38)
    int number_of_new_visited_voxel = 0;                                 // rgbMapTracker.h:52
    std::vector<srl_color_stored> color_stored;
    srl_color_totals color_totals = {0, 0, 0, 0};
    // rgbMapTracker::renderPointsInRecentVoxel (rgbMapTracker.cpp:219-237) on the device colour map (srl_color_map_render): the image the
    // caller uploaded with srl_color_image_upload is rendered into the points of voxels_recent_visited, the list addPointsToMap filled
    // under `to_rendering`.  Neither list is changed.  render_totals: what the pass did (updated = the reference's render_point_count).
    void renderPointsInRecentVoxel(const srl_color_camera &camera, double obs_time);
    srl_color_render_totals render_totals = {0, 0, 0, 0, 0, 0, 0};
    // rgbMapTracker::selectPointsForProjection (rgbMapTracker.cpp:45-152) on the device colour map (srl_color_map_select) over
    // voxels_recent_visited: one point per coarse image cell, the nearest by the reference's float depth mask, with its pixel position --
    // what the optical-flow tracker takes.  refreshPointsForProjection (:26-43): the same with (10.0, 1), nothing when the frame has no
    // image size, the result kept as points_for_projection (the reference's points_rgb_vec_for_projection).  select_totals: the last call's.
    double minimum_depth_for_projection = 0.1;                           // rgbMapTracker.cpp:9
    double maximum_depth_for_projection = 200;                           // rgbMapTracker.cpp:10
    std::vector<srl_color_selected> selectPointsForProjection(const srl_color_camera &camera, int rows, int cols, double minimum_dis = 10.0, int skip_step = 1,
                                                              bool use_all_points = false);
    void refreshPointsForProjection(const srl_color_camera &camera, int rows, int cols);
    std::vector<srl_color_selected> points_for_projection;
    srl_color_select_totals select_totals = {0, 0, 0, 0, 0, 0, 0, 0};
    size_t select_capacity = 0;                                          // records the one call per frame has room for: 1.5 x the most selected so far
    // The publishers' coloured cloud on the device colour map (srl_color_map_export_cloud): a point is left out iff N_rgb < minimum_views
    // (map_options.pub_point_minimum_views).  pubColorPoints (lioOptimization.cpp:1210-1241; the same cloud threadPubColorPoints cuts into
    // topics, :1243-1344): the whole registered list, ascending.  saveColorPoints (:1386-1426): its loop is `for (i = size - 1; i > 0; i--)`
    // (:1398) -- descending, index 0 never saved: the range [1, size) reversed.  point_index (optional) receives the registered index of
    // every record.  ROS messages, topics, sleeping and the PCD file stay with the caller.  cloud_totals: the last call's.  Both return a
    // view of the object's own buffers, valid until the next of these calls.  The buffers keep the size of the largest cloud so far and
    // half as much again (one device call per cloud; only a call that publishes more than that is asked a second time) and are not
    // touched between calls, so that a publisher that runs every frame pays for the records it receives and for nothing else.
    struct colorCloudView { const srl_color_cloud_point *points; const int32_t *point_index /* or nullptr */; size_t size; };
    colorCloudView pubColorPoints(int minimum_views, bool with_point_index = false);
    colorCloudView saveColorPoints(int minimum_views, bool with_point_index = false);
    std::vector<srl_color_cloud_point> color_cloud;                      // the buffers: records [0, cloud_totals.published) are the last cloud
    std::vector<int32_t> color_cloud_index;
    // the call beneath both, into the caller's arrays (which = 0 pub, 1 save); returns the status of srl_color_map_export_cloud
    int colorCloud(int which, int minimum_views, srl_color_cloud_point *out, int32_t *point_index, int64_t capacity);
    srl_color_cloud_totals cloud_totals = {0, 0, 0, 0};
    // threadPubColorPoints' topic schedule (:1262-1342) as a pure function with the state the thread carries from round to round: for P
    // published points P / number_of_points_per_topic full topics, then one remainder topic that is always sent, also when it is empty;
    // if the topics sent in the round are >= 45 both ints are multiplied by 1.5 and truncated (:1338-1342).  Returns the topic sizes.
    int number_of_points_per_topic = 1000;                               // :1247
    int sleep_time_after_pub = 10;                                       // :1246
    int64_t colorTopicCount(int64_t published) const { return published / number_of_points_per_topic + 1; }
    std::vector<int32_t> colorTopicSizes(int64_t published);
    bool collectPointsWorld() const { return collect_points_world; }

    // ---- ours ----
    // pin a sweep in HBM (bench: inputs resident before the timed region): solveIEKF() then runs on it.  updateIEKF()
    // with a keypoint vector always uploads that vector and releases the pin.
    int residentSweep(const double *raw_xyz, int n);
    // upload the NEXT sweep on the copy stream while solveIEKF() works on the current one; swapSweep() makes it the pinned one
    int prefetchSweep(const double *raw_xyz, int n);
    int swapSweep();
    // ... the same upload issued by the next solveIEKF() beside the kernel of its first pass (srl_lio_prefetch_sweep_during_solve)
    void prefetchSweepDuringSolve(const double *raw_xyz, int n) { pending_prefetch_raw = raw_xyz; pending_prefetch_n = n; pending_prefetch_rc = 0; }
    bool sweepPinned(int n) const { return sweep_pinned && resident_n == n; }
    // updateIEKF on the sweep already resident in HBM (no keypoint vector needed)
    optimizeSummary solveIEKF(const icpOptions &cur_icp_options, cloudFrame *p_frame);
    void releaseSweep() { sweep_pinned = false; resident_n = -1; }
    // frame-resident form of optimize(): the raw frame is uploaded once, keypoints are selected on the device with
    // the prior pose of p_frame->p_state (same set and order as gridSampling on transformPoint-ed points), the
    // ESIKF runs on them in place.  Returns the keypoints' frame indices through keypoint_index (optional).
    optimizeSummary optimizeResident(cloudFrame *p_frame, const double *frame_raw, int n, const icpOptions &cur_icp_options,
                                     double sample_voxel_size, std::vector<int> *keypoint_index = nullptr);
    // transformPoint over the uploaded frame with p_state's pose + addPointsToMap, all on the device
    // (want_added = false: the insertion is only enqueued -- srl_frame_commit with num_added = NULL -- and -1 is returned)
    int commitFrame(const state *p_state, double voxel_size, int max_num_points_in_voxel, double min_distance_points,
                    int min_num_points, double *world_out = nullptr, bool want_added = true);
    void setNormalEqProvider(normal_eq_provider fn, void *user) { provider = fn; provider_user = user; }
    srl_ctx *context() { return voxel_map.ctx; }

    // members the path reads (lioOptimization.h:216-228,249,274); public for replay drivers
    eskfEstimator *eskf_pro = nullptr;
    voxelHashMap voxel_map;
    srl::Mat3 R_imu_lidar = srl::Mat3::Identity();
    srl::Vec3 t_imu_lidar = srl::Vec3::Zero();
    double laser_point_cov = 0.001;                    // lioOptimization.cpp:364
    std::vector<cloudFrame *> all_cloud_frame;

    bool record_iterations = false;
    std::vector<iterationLog> iteration_log;
    int last_num_iterations = 0;
    int last_num_observed = 0;         // eskf_pro->observe() calls of the last solve (optimize.cpp:253): 0 = p_state / G were never written (:255-261)
    int last_solve_launches = 0;       // passes (= association kernel launches) of the last solve

private:
    int normalEquations(const icpOptions &o, cloudFrame *p_frame, srl_normal_eq &neq, void (*while_running)(void *) = nullptr, void *user = nullptr);
    void fillFrame(cloudFrame *p_frame, srl_frame &f) const;
    normal_eq_provider provider = nullptr;
    void *provider_user = nullptr;
    int resident_n = -1;
    int prefetched_n = -1;
    const double *pending_prefetch_raw = nullptr;      // prefetchSweepDuringSolve: issued by the next solve's first pass
    int pending_prefetch_n = -1;
    int pending_prefetch_rc = 0;
    bool sweep_pinned = false;
    bool collect_points_world = false;
    bool color_map_enabled = false;
    void colorInsert(const double *world_xyz, int n, double time_sweep_end, bool rendering);
};

}  // namespace srlivo

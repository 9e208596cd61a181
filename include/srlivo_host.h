/*
 * srlivo_host.h -- C handles onto the C++ host mirror (sr_livo_amd/csrc/host/: lioOptimization,
 * eskfEstimator, cloudMap types with the reference's member names).  A C++ consumer (the ROS node)
 * includes the mirror headers directly; these handles exist so that non-C++ harnesses (the Python
 * parity tests and bench.py, via ctypes) drive exactly the same C++ code.  Exported by
 * libsrlivo_hip.so next to the kernel-level ABI of srlivo_hip.h.
 */
#ifndef SRLIVO_HOST_H
#define SRLIVO_HOST_H

#include "srlivo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srl_lio srl_lio;

/* device >= 0: lioOptimization on the HIP backend (fails with SRL_ERR_NO_DEVICE without a GPU).
 * device <  0: host-only object; only srl_lio_update_iekf_provided() may be used on it. */
int      srl_lio_create(int device, srl_lio **out);
int      srl_lio_destroy(srl_lio *lio);
srl_ctx *srl_lio_ctx(srl_lio *lio);                         /* the context behind voxel_map (NULL if host-only) */
const char *srl_lio_last_error(srl_lio *lio);

/* members of class lioOptimization the path reads (lioOptimization.h:221,227-228) */
int srl_lio_set_extrinsics(srl_lio *lio, const double R_il[9], const double t_il[3]);
int srl_lio_set_laser_point_cov(srl_lio *lio, double cov);
/* srl_lio_last_solve_launches: kernel launches the last solve enqueued for its passes (one per ESIKF iteration; with armed launches
 * all but the first are enqueued ahead of time, include/srlivo_hip.h). */
int srl_lio_last_solve_launches(srl_lio *lio, int *launches);
/* eskfEstimator::observe() calls of the last solve (src/optimize.cpp:253).  0 = every pass ran into the step guard (:248-251) or
 * failed before it: the reference then never wrote p_frame->p_state, G, G_norm (:255-261) -- a binding must not either. */
int srl_lio_last_solve_observed(srl_lio *lio, int *observed);

/* eskfEstimator accessors (eskfEstimator.h:74-108).  state = p(3) q(wxyz,4) v(3) ba(3) bg(3) g(3) */
int srl_lio_eskf_get_state(srl_lio *lio, double s[19]);
int srl_lio_eskf_set_state(srl_lio *lio, const double s[19]);
int srl_lio_eskf_get_cov(srl_lio *lio, double P[289]);
int srl_lio_eskf_set_cov(srl_lio *lio, const double P[289]);
int srl_lio_eskf_set_noise(srl_lio *lio, double acc_cov, double gyr_cov, double b_acc_cov, double b_gyr_cov);
int srl_lio_eskf_init_imu(srl_lio *lio, const double acc0[3], const double gyr0[3]);
int srl_lio_eskf_scale_init_cov(srl_lio *lio);
int srl_lio_eskf_predict(srl_lio *lio, double dt, const double acc1[3], const double gyr1[3]);
int srl_lio_eskf_observe(srl_lio *lio, const double dx[17]);

/* lioOptimization::addPointsToMap / mapSize (lioOptimization.h:347-357) on the device map */
int srl_lio_add_points_to_map(srl_lio *lio, const double *world_xyz, int n, double voxel_size,
                              int max_num_points_in_voxel, double min_distance_points, int min_num_points);
int srl_lio_map_size(srl_lio *lio, int64_t *num_points);
/* lioOptimization::removePointsFarFromLocation (lioOptimization.cpp:556-572) on the device map: srl_map_remove_far.  The reference
 * calls it right after addPointsToMap in stateEstimation (lioOptimization.cpp:1032, commented out in the shipped node); a caller of
 * srl_lio_run_measurement does the same with srl_lio_remove_points_far_from_location(lio, result.state + 4, max_distance) after every
 * processed, successful measurement. */
int srl_lio_remove_points_far_from_location(srl_lio *lio, const double location[3], double distance);
/* points_world (include/lioOptimization.h:262): the cloud addPointsToMap publishes as cloud_world (lioOptimization.cpp:552-553) -- the
 * points the last insertion of this handle (srl_lio_add_points_to_map, srl_lio_commit_frame, the commit inside srl_lio_run_measurement)
 * appended to voxels that already existed, see srl_map_insert_report.  Off by default; while on, those insertions go through the
 * synchronous report calls (a commit with num_added == NULL is then not deferred).  srl_lio_points_world copies the records out: *n is
 * their number; capacity 0 asks for the number alone, a smaller non-zero capacity is SRL_ERR_BAD_ARG.  The cloud stays until the next
 * insertion.  A host-only handle has no map: SRL_ERR_NO_DEVICE with *n = 0. */
int srl_lio_set_collect_points_world(srl_lio *lio, int on);
int srl_lio_points_world(srl_lio *lio, srl_cloud_point *out, int capacity, int *n);
/* The colour half of addPointsToMap (lioOptimization.cpp:538-539, addPointToColorMap :448-518), opt-in.  srl_lio_set_color_map_options
 * creates the device colour map (srl_color_map_create; opts NULL = srl_color_opts_default); from then on every insertion of this handle
 * also runs srl_color_map_insert behind the LiDAR insertion -- the commits on the world points they left in HBM -- and keeps
 * voxels_recent_visited_temp, voxels_recent_visited and number_of_new_visited_voxel as lioOptimization.cpp:523-550 do.  Without it the
 * handle behaves exactly as before.  srl_lio_set_color_times: img_pro->time_last_process (imageProcessing.cpp:6: -1e5 until the vision
 * stage processes a frame), p_frame->time_sweep_end of the frame the next srl_lio_commit_frame inserts (srl_lio_run_measurement takes the
 * frame's own), and the `to_rendering` flag stateEstimation passes (:1027).  srl_lio_add_points_to_map_at: srl_lio_add_points_to_map
 * with the frame's time_sweep_end and to_rendering as arguments.  srl_lio_color_visited copies a list out (which = 0:
 * voxels_recent_visited_temp, 1: voxels_recent_visited; int32 x 3 per voxel; capacity in voxels, 0 asks for the number alone) and
 * number_of_new_visited_voxel; srl_lio_color_stored the records of the last insertion.  A host-only handle: SRL_ERR_NO_DEVICE. */
int srl_lio_set_color_map_options(srl_lio *lio, const srl_color_opts *opts);
int srl_lio_set_color_times(srl_lio *lio, double time_last_process, double commit_time_sweep_end, int to_rendering);
int srl_lio_add_points_to_map_at(srl_lio *lio, const double *world_xyz, int n, double voxel_size, int max_num_points_in_voxel,
                                 double min_distance_points, int min_num_points, double time_sweep_end, int to_rendering);
int srl_lio_color_visited(srl_lio *lio, int which, int32_t *out_xyz, int capacity, int *n, int *number_of_new_visited_voxel);
int srl_lio_color_stored(srl_lio *lio, srl_color_stored *out, int capacity, int *n);
/* rgbMapTracker::renderPointsInRecentVoxel (rgbMapTracker.cpp:219-237): srl_color_map_render of the image last uploaded with
 * srl_color_image_upload(srl_lio_ctx(lio), ...) into the points of voxels_recent_visited (the list an insertion with to_rendering set
 * left; repeats included).  totals (optional) is zeroed first.  NULL lio or camera: SRL_ERR_BAD_ARG; a host-only handle:
 * SRL_ERR_NO_DEVICE; otherwise the codes of srl_color_map_render. */
int srl_lio_render_points_in_recent_voxel(srl_lio *lio, const srl_color_camera *camera, double obs_time, srl_color_render_totals *totals);
/* rgbMapTracker::selectPointsForProjection (rgbMapTracker.cpp:45-152): srl_color_map_select over voxels_recent_visited with the object's
 * minimum_depth_for_projection / maximum_depth_for_projection (0.1, 200).  refresh != 0: refreshPointsForProjection (:26-43) -- the
 * parameters (10.0, 1, list mode) whatever is passed, SRL_OK with *n = 0 at once when rows or cols is 0, and the result kept by the object
 * as points_for_projection.  *n = the number of records; capacity 0 asks for the number (and the totals) alone, a smaller capacity than
 * *n is SRL_ERR_BAD_ARG.  NULL lio, camera or n: SRL_ERR_BAD_ARG; a host-only handle: SRL_ERR_NO_DEVICE; otherwise the codes of
 * srl_color_map_select. */
int srl_lio_select_points_for_projection(srl_lio *lio, const srl_color_camera *camera, int rows, int cols, double minimum_dis, int skip_step,
                                         int use_all_points, int refresh, srl_color_selected *out, int capacity, int *n,
                                         srl_color_select_totals *totals);
/* The coloured cloud of the publishers (srl_color_map_export_cloud with since = -inf).  which = 0: pubColorPoints
 * (lioOptimization.cpp:1210-1241) and the cloud threadPubColorPoints cuts into topics (:1243-1344): the whole registered list, ascending.
 * which = 1: saveColorPoints (:1386-1426), whose loop is `for (i = size - 1; i > 0; i--)` (:1398): descending, and index 0 is never
 * saved -- the range [1, size) reversed.  *n = the number of records; out and point_index (optional) take them; capacity 0 asks for the
 * number and the totals alone, a smaller capacity than *n is SRL_ERR_BAD_ARG with both filled.  NULL lio or n, which outside 0 ... 1,
 * capacity < 0 or capacity > 0 without out: SRL_ERR_BAD_ARG; a host-only handle: SRL_ERR_NO_DEVICE, never a host loop; otherwise the codes
 * of srl_color_map_export_cloud. */
int srl_lio_color_cloud(srl_lio *lio, int which, int minimum_views, srl_color_cloud_point *out, int32_t *point_index, int64_t capacity,
                        int64_t *n, srl_color_cloud_totals *totals);
/* The same cloud without a copy of the caller's: *points (and *point_index, when with_point_index is set) point into buffers the object
 * keeps -- *n records, valid until the next srl_lio_color_cloud_view of this handle or its destruction.  The buffers hold the largest
 * cloud so far and half as much again and are not touched between calls: one device call per cloud, a second one only for a cloud
 * larger than the buffers.  Errors of the device call arrive as SRL_ERR_HIP with the message of srl_lio_last_error. */
int srl_lio_color_cloud_view(srl_lio *lio, int which, int minimum_views, int with_point_index, const srl_color_cloud_point **points,
                             const int32_t **point_index, int64_t *n, srl_color_cloud_totals *totals);
/* threadPubColorPoints' topic schedule (:1262-1342) as a function of the number of published points, with the two ints the thread carries
 * from round to round kept by the object: number_of_points_per_topic = 1000 and sleep_time_after_pub = 10 (microseconds) at the start.
 * One round: published / number_of_points_per_topic full topics, then one remainder topic that is always sent, also when it is empty
 * (:1319-1336); if the number of topics sent is >= 45 both ints are multiplied by 1.5 and truncated (:1338-1342) for the NEXT round.
 * sizes[0 .. *n_topics) are the topic sizes in order: the caller slices the one cloud srl_lio_color_cloud(which = 0) gave.  A capacity
 * below *n_topics leaves the carried state as it was (0: SRL_OK, the number alone; else SRL_ERR_BAD_ARG).  Pure host logic: works on a
 * host-only handle.  srl_lio_color_topic_state reads the carried ints (each output optional). */
int srl_lio_color_topic_sizes(srl_lio *lio, int64_t published, int32_t *sizes, int capacity, int *n_topics);
int srl_lio_color_topic_state(srl_lio *lio, int *number_of_points_per_topic, int *sleep_time_after_pub);
/* Where lioOptimization::buildFrame sub-samples the cut sweep (subSampleFrame, lioOptimization.cpp:838-846): on = 1 (the default) on the
 * device (srl_frame_subsample + srl_frame_take_subsampled; the host runs the two shuffles on index arrays and downloads m points), 0 = on the
 * host over the n-point downloads of srl_frame_undistort and srl_frame_take.  Both give the same frame bit for bit. */
int srl_lio_set_device_subsample(srl_lio *lio, int on);
/* srl_map_probe_checksum over the world points the last srl_lio_commit_frame left in HBM (the frame the node inserts next) */
int srl_lio_probe_checksum_of_committed_frame(srl_lio *lio, int stride, double voxel_size, uint64_t *checksum, int32_t *num_voxels);

/* keep a sweep resident in HBM for the next srl_lio_update_iekf (pass raw_xyz = NULL there) */
int srl_lio_resident_sweep(srl_lio *lio, const double *raw_xyz, int n);
/* srl_sweep_prefetch / srl_sweep_swap behind the handle: upload the next sweep while srl_lio_update_iekf (raw_xyz = NULL)
 * solves the current one; the swapped-in sweep becomes the resident one. */
int srl_lio_prefetch_sweep(srl_lio *lio, const double *raw_xyz, int n);
int srl_lio_swap_sweep(srl_lio *lio);
/* The same prefetch, issued BY the next srl_lio_update_iekf while the kernel of its first pass is in flight (a node receives sweep k + 1
 * during the solve of sweep k, src/lioOptimization.cpp:1003-1027): the host time of the upload call (a memcpy enqueue and two event
 * records, ~5 us) then lies beside the association kernel instead of between two solves.  raw_xyz must stay valid and untouched until that
 * solve has returned (page-locked memory: until srl_sweep_wait / the first result on the swapped-in sweep, as for srl_sweep_prefetch). */
int srl_lio_prefetch_sweep_during_solve(srl_lio *lio, const double *raw_xyz, int n);

/* lioOptimization::updateIEKF (optimize.cpp:133-314).
 * state_io: p_frame->p_state = q(wxyz) t v ba bg (16 doubles) in/out; t_last = previous frame's
 * translation; log (optional): per iteration HtH(36) Hth(6) d_x(17) num_residuals loss = 61 doubles.
 * Returns SRL_OK with *iters >= 1, or SRL_ERR_NOT_ENOUGH_RESIDUALS / SRL_ERR_NAN_PLANARITY / ... */
int srl_lio_update_iekf(srl_lio *lio, const srl_icp_opts *opts, const double *raw_xyz, int n,
                        double state_io[16], const double t_last[3], int frame_id, double *log,
                        int max_log_iters, int *iters, int *num_residuals_used);

/* same update, the per-iteration normal equations coming from `provider` (multi-process CPU tests of
 * the sharded host logic; never used by the product path). */
typedef int (*srl_normal_eq_provider)(const srl_frame *frame, const srl_icp_opts *opts, srl_normal_eq *out, void *user);
/* The body of a node's loop over a stream of sweeps (src/lioOptimization.cpp:1003-1027: one optimize() per sweep) as ONE call, for replay
 * and benchmark loops whose own language would otherwise sit between the calls: reset the filter to the given prior (eskf_state[19],
 * eskf_cov[289]; NULL: keep what the filter holds), register the upload of the NEXT sweep with the solve (next_raw_xyz / next_n; NULL: none),
 * solve the resident sweep of n keypoints (srl_lio_update_iekf with raw_xyz = NULL), and make the next sweep the resident one
 * (srl_lio_swap_sweep; only when one was given).  Same statuses as the calls it stands for; the first failure is returned. */
int srl_lio_stream_step(srl_lio *lio, const srl_icp_opts *opts, const double eskf_state[19], const double eskf_cov[289], int n, double state_io[16],
                        const double t_last[3], int frame_id, const double *next_raw_xyz, int next_n, int *iters, int *num_residuals_used);

int srl_lio_update_iekf_provided(srl_lio *lio, const srl_icp_opts *opts, srl_normal_eq_provider provider,
                                 void *user, int n, double state_io[16], const double t_last[3], int frame_id,
                                 double *log, int max_log_iters, int *iters, int *num_residuals_used);

/* lioOptimization::optimize (optimize.cpp:428-448): gridSampling -> updateIEKF -> re-transform.
 * frame_raw / frame_world: point3D::raw_point / ::point of p_frame->point_frame (n x 3 each);
 * frame_world is overwritten with the re-transformed points on success; keypoint_index (optional,
 * capacity n) receives the indices gridSampling selected, in keypoint order. */
int srl_lio_optimize(srl_lio *lio, const srl_icp_opts *opts, double sample_voxel_size, const double *frame_raw,
                     double *frame_world, int n, double state_io[16], const double t_last[3], int frame_id,
                     int32_t *keypoint_index, int *num_keypoints, int *iters, int *num_residuals_used);

/* eskfEstimator::tryInit (eskfEstimator.cpp:43-118): imu_meas as t (n), gyr (n x 3), acc (n x 3).
 * *initialized: 1 initialised by this call (initial_flag set), 0 wait for more, -1 / -2 gyro / accel variance too large.
 * get_init_stats: mean_gyr, mean_acc, gyr_cov, acc_cov, num_init_meas, initial_flag (14 doubles).
 * initial_flag is process-global, as in the reference (utility.cpp:11). */
int srl_lio_eskf_try_init(srl_lio *lio, const double *t, const double *gyr, const double *acc, int n, int *initialized);
int srl_lio_eskf_get_init_stats(srl_lio *lio, double out[14]);
int srl_lio_set_initial_flag(srl_lio *lio, int flag);
/* G_norm is process-global as well (utility.cpp:14: 9.81): the first processed frame of a replay writes the norm of the filter's gravity
 * back into it (lioOptimization.cpp:1024) and the next initialisation scales its gravity by it, so a second replay in one process
 * starts from another value than the first.  A harness that compares replays bit for bit sets it before each.  g_norm must be finite
 * and positive. */
int srl_lio_set_g_norm(srl_lio *lio, double g_norm);
/* lioOptimization::stateInitialization (lioOptimization.cpp:895-990): pose prior (q wxyz, t) of frame index_frame from
 * prev2 / prev1 = poses of all_cloud_frame[size-2] / [size-1]; initialization: 0 INIT_IMU, 1 INIT_CONSTANT_VELOCITY. */
int srl_lio_state_initialization(srl_lio *lio, int index_frame, int initialization, const double prev2[7],
                                 const double prev1[7], double out[7]);

/* ---- ROS-free replay driver: the LIO part of lioOptimization::run()'s loop body (lioOptimization.cpp:1427-1584):
 * tryInit while the filter is uninitialised; afterwards IMU propagation (predict per sample, imu_states), then
 * process() = stateInitialization -> buildFrame (device undistortion) -> stateEstimation (device keypoints, ESIKF,
 * device map insert) and the sliding window.  One call = one `Measurements` element: time_frame = time_image,
 * IMU samples (time, linear_acceleration, angular_velocity), the cut sweep (sensor-frame points + absolute point
 * timestamps) and time_sweep = (begin, offset).  srl_odometry_opts carries the odometryOptions fields the path
 * reads (parameters.h:58-88) plus the IMU noise parameters (setAccCov ...) and isPointTimeEnable(). */
typedef struct srl_odometry_opts {
    double init_voxel_size, init_sample_voxel_size;
    int init_num_frames, num_for_initialization;
    double voxel_size, sample_voxel_size;
    int max_num_points_in_voxel;
    double min_distance_points;
    int motion_compensation;          /* include/utility.h:82-86: 0 IMU, 1 CONSTANT_VELOCITY */
    int initialization;               /* include/utility.h:88-92: 0 INIT_IMU, 1 INIT_CONSTANT_VELOCITY */
    int point_time_enable;
    double acc_cov, gyr_cov, b_acc_cov, b_gyr_cov;
    srl_icp_opts icp;
} srl_odometry_opts;
typedef struct srl_replay_result {
    int processed;                    /* 0: the call only fed tryInit */
    int initialized;                  /* initial_flag after the call */
    int index_frame;                  /* after the call */
    int success, num_residuals_used, iterations;
    int frame_points, keypoints, points_added;
    double state[16];                 /* p_state of the frame: q wxyz, t, v, ba, bg */
} srl_replay_result;
int srl_lio_set_odometry_options(srl_lio *lio, const srl_odometry_opts *opts);
int srl_lio_run_measurement(srl_lio *lio, double time_frame, const double *imu_t, const double *imu_acc,
                            const double *imu_gyr, int n_imu, const double *pts_raw, const double *pts_timestamp,
                            int n_pts, double time_sweep_begin, double time_sweep_offset, srl_replay_result *out);
/* point3D::raw_point / ::point / ::imu_point of the newest frame in all_cloud_frame (any pointer may be NULL) */
int srl_lio_last_frame(srl_lio *lio, int capacity, double *raw_point, double *point, double *imu_point, int *n);

/* The point side of the node on the device point queue (srlivo_hip.h: srl_livox_decode, srl_points_cut, srl_frame_undistort_cut).
 * srl_lio_set_lidar_options: cloudProcessing's N_SCANS, time_unit_scale (srl_time_unit_scale), blind and point_filter_num; refused like
 *   srl_livox_decode refuses them.
 * srl_lio_feed_livox: lioOptimization::livoxHandler (lioOptimization.cpp:593-601): the message is decoded into the handle's queue;
 *   last_time_lidar = header_stamp, and cloud_pro->last_end_time follows the report (a message without a valid point leaves it as it
 *   was).  The reference asserts header_stamp > last_time_lidar; here such a message is refused with SRL_ERR_BAD_ARG and nothing is queued,
 *   as is a feed before the options are set.
 * srl_lio_points_info: srl_points_info plus the two times above (every output optional; the two times are written even when the queue does
 *   not exist yet and the call returns SRL_ERR_NO_SWEEP).
 * srl_lio_run_measurement_queued: srl_lio_run_measurement with the sweep cut from the queue at time_cut (while (front().timestamp <
 *   time_cut) pop, lioOptimization.cpp:719-723 / :759-763) in place of pts_raw / pts_timestamp: the cut points are rewritten, undistorted and
 *   sub-sampled where they lie, and only the kept points' fields come back.  The same results bit for bit as srl_lio_run_measurement on
 *   the same points.  Needs srl_lio_set_device_subsample(1) and voxel_size > 0: otherwise SRL_ERR_UNSUPPORTED and the queue is left uncut.
 *   An empty cut is the reference's "no lidar points, no Measurements element": SRL_OK, out->processed = 0, nothing changes (the IMU
 *   samples are not consumed either).  There is no _image twin yet: srl_lio_run_measurement_image's body is not a forward. */
int srl_lio_set_lidar_options(srl_lio *lio, const srl_livox_opts *opts);
int srl_lio_feed_livox(srl_lio *lio, const srl_livox_point *points, int point_num, double header_stamp, srl_livox_report *report);
int srl_lio_points_info(srl_lio *lio, int *size, double *front_timestamp, double *back_timestamp, double *last_time_lidar, double *last_end_time);
int srl_lio_run_measurement_queued(srl_lio *lio, double time_frame, const double *imu_t, const double *imu_acc, const double *imu_gyr, int n_imu,
                                   double time_cut, double time_sweep_begin, double time_sweep_offset, srl_replay_result *out);
/* The same for the spinning LiDARs (srlivo_hip.h: srl_pc2_decode).
 * srl_lio_set_pc2_options: cloudProcessing's lidar_type, N_SCANS, SCAN_RATE, point_filter_num, time_unit_scale and blind; refused like
 *   srl_pc2_decode refuses them (n_scans and scan_rate are looked at by the yaw branch alone, and refused there).
 * srl_lio_feed_pointcloud2: lioOptimization::standardCloudHandler (lioOptimization.cpp:583-591): the message is decoded with the handle's
 *   last_end_time into the handle's queue; last_time_lidar = header_stamp, and last_end_time follows the report (an empty message leaves
 *   it as it was).  header_stamp <= last_time_lidar (the reference's assert) and a feed before the options are set: SRL_ERR_BAD_ARG,
 *   nothing queued.  The two times and the queue are the ones srl_lio_feed_livox uses: both feeds keep one FIFO.
 *   report->given_offset_time is cloudProcessing::isPointTimeEnable(): what the caller puts into srl_odometry_opts.point_time_enable. */
int srl_lio_set_pc2_options(srl_lio *lio, const srl_pc2_opts *opts);
int srl_lio_feed_pointcloud2(srl_lio *lio, const void *data, size_t data_bytes, const srl_pc2_layout *layout, double header_stamp,
                             srl_pc2_report *report);

/* Frame-resident form of optimize() + the map update that follows it in stateEstimation
 * (lioOptimization.cpp:1027,1051): the raw frame (n x 3) is uploaded once; keypoints are selected on the device
 * from point = R(q)(R_il raw + t_il) + t with the PRIOR pose in state_io (what point3D::point holds when
 * optimize() is entered, lioOptimization.cpp:981-1001 -> utility.cpp:314-318) -- same keypoints, same order as
 * gridSampling -- and the ESIKF runs on them in place.  srl_lio_commit_frame then re-transforms the frame with
 * `state` (optimize.cpp:441-445) and inserts it (addPointsToMap) without the points leaving HBM;
 * world_out (n x 3, optional) receives point3D::point. */
int srl_lio_optimize_resident(srl_lio *lio, const srl_icp_opts *opts, double sample_voxel_size, const double *frame_raw,
                              int n, double state_io[16], const double t_last[3], int frame_id, int32_t *keypoint_index,
                              int *num_keypoints, int *iters, int *num_residuals_used);
int srl_lio_commit_frame(srl_lio *lio, const double state[16], double voxel_size, int max_num_points_in_voxel,
                         double min_distance_points, int min_num_points, double *world_out, int *num_added /* or NULL: see srl_frame_commit */);

/* ------------------------------------------------------------------ the camera ESIKF (csrc/host/imageProcessing.{h,cpp})
 * imageProcessing::vioEsikf (imageProcessing.cpp:220-380) and vioPhotometric (:402-552) with both updateCameraParameters, setInitialCov
 * and the 11 x 11 covariance, on the camera state the handle keeps (csrc/host/cameraState.h).  Each iteration's per-point loop is ONE
 * srl_color_map_vio_rows on the handle's device (srlivo_hip.h); the solve uses its sums: A = HtH + (J0 P J0^T w)^-1, K r = A^-1 Htr,
 * K H = A^-1 HtH -- the reference forms the 11 x 2N gain K explicitly, the one algebraic difference.  Everything else is the
 * reference's statements: the < 10 points gates, both convergence breaks, acc_residual / total_point_size, cam_measurement_weight from
 * number_of_new_visited_voxel, the final covariance update with K H and `solution` of the last iteration (zero when the loop broke at
 * the gate).  The tracked list is map_rgb_points_in_last_image_pose in the caller's order and n, its length, is also taken as
 * total_point_size: the reference reads that from map_rgb_points_in_cur_image_pose.size() (:247, :413), so the two maps are assumed to
 * have one size, as they do behind removeOutlierUsingRansacPnp.
 * The camera state travels as 31 doubles: time_td, R_imu_camera (9, row-major), t_imu_camera (3), fx fy cx cy, q_world_camera
 * (w x y z), t_world_camera (3), rotation (w x y z), translation (3). */
#define SRL_LIO_CAMERA_STATE_DOUBLES 31
int srl_lio_vio_set_options(srl_lio *lio, int num_iterations, int estimate_intrinsic, int estimate_extrinsic, const double camera_intrinsic[9],
                            const double R_imu_camera[9], const double t_imu_camera[3]);
int srl_lio_vio_set_camera_state(srl_lio *lio, const double *state31);
int srl_lio_vio_get_camera_state(srl_lio *lio, double *state31);
int srl_lio_vio_set_initial_cov(srl_lio *lio);                    /* setInitialCov (:65-72) */
int srl_lio_vio_set_cov(srl_lio *lio, const double *cov121);      /* row-major */
int srl_lio_vio_get_cov(srl_lio *lio, double *cov121);
/* replaces the measurement pass (tests feed recorded sums through it); NULL puts the device's back.  Returns a srl_status. */
typedef int (*srl_vio_rows_provider)(const srl_color_vio_args *args, const srl_color_vio_point *points, int n, srl_color_vio_sums *sums, void *user);
int srl_lio_vio_set_rows_provider(srl_lio *lio, srl_vio_rows_provider fn, void *user);
/* *accepted = what the reference's function returns (0: fewer than 10 tracked points, nothing done).  *iterations = the number of
 * updateCameraParameters calls; states (optional, capacity x 31 doubles) takes the camera state behind each of the first `capacity`.
 * *used = num_used_point_count of the last iteration.  NULL lio, accepted or (n > 0) tracked, n < 0: SRL_ERR_BAD_ARG; a host-only handle
 * without a provider: SRL_ERR_NO_DEVICE, never a host loop; otherwise what the measurement pass returned. */
int srl_lio_vio_esikf(srl_lio *lio, const srl_color_vio_point *tracked, int n, int number_of_new_visited_voxel, int *accepted, int *iterations,
                      int *used, double *states, int capacity);
int srl_lio_vio_photometric(srl_lio *lio, const srl_color_vio_point *tracked, int n, int number_of_new_visited_voxel, int *accepted,
                            int *iterations, int *used, double *states, int capacity);

/* class LKOpticalFlowKernel of the host mirror (csrc/host/lkpyramid.h; lkpyramid.cpp:627-795): the reference's constructor arguments
 * (cv::Size winSize, maxLevel, cv::TermCriteria {type, maxCount, epsilon}, flags, minEigThreshold) with setTerminationCriteria's clamping
 * (:670-682: without COUNT 30 steps, else 0 ... 100; without EPS 0.01, else 0 ... 10), and trackImage on a raw gray buffer, which is
 * srl_flow_track_image of srlivo_hip.h on ctx with those values (the device tracker is created at the first image and owned by the
 * handle).  ctx may be NULL: the handle then answers srl_lk_get, and srl_lk_track_image returns the C-ABI's SRL_ERR_BAD_ARG -- there is
 * no host loop.  srl_lk_get: the level count (as lowered by the first image) and the clamped criteria; NULL outputs are skipped. */
typedef struct srl_lk srl_lk;
int srl_lk_create(srl_ctx *ctx, int win_width, int win_height, int max_level, int criteria_type, int max_count, double epsilon, int flags,
                  double min_eig_threshold, srl_lk **out);
int srl_lk_destroy(srl_lk *lk);
int srl_lk_get(srl_lk *lk, int *max_level, int *max_count, double *epsilon);
int srl_lk_track_image(srl_lk *lk, const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, const float *prev_xy, int n,
                       float *next_xy, uint8_t *status, int *n_tracked);

/* class opticalFlowTracker of the host mirror (csrc/host/opticalFlowTracker.h; opticalFlowTracker.cpp:13-323) without OpenCV: the
 * bookkeeping between srl_color_map_select, srl_flow_track_image, srl_color_map_vio_rows and srl_color_map_track_update in the loop
 * of imageProcessing::process (imageProcessing.cpp:137-161).  State is kept by pool position (srl_color_selected.pool); wherever the
 * reference iterates a std::map keyed by pointer value the mirror iterates by ASCENDING POOL POSITION: last_tracked_points / old_ids,
 * the point lists handed to the PnP provider, srl_oft_pose_map and srl_oft_tracked_for_vio.  ctx may be NULL for a handle whose flow
 * and update go through providers.  Providers return a srl_status; NULL puts the default back:
 *   flow         srl_flow_track_image's arguments without the context; default: the handle's LKOpticalFlowKernel on ctx (21 x 21, 3
 *                levels, COUNT + EPS 10 / 0.05), whose first image -- srl_oft_init's -- is only stored
 *   fundamental  the mask of the caller's cv::findFundamentalMat(last, cur, FM_RANSAC, 1.0, 0.997, status), n bytes; no default:
 *                srl_oft_track_image with 30 or more points and none set is SRL_ERR_BAD_ARG
 *   pnp          the inlier list of the caller's cv::solvePnPRansac (n x 3 floats, n x 2 floats -> indices); a status other than SRL_OK
 *                stands for the cv::Exception the reference catches (*accepted = 0); no default: with 10 or more points and none set
 *                SRL_ERR_BAD_ARG
 *   update       srl_color_map_track_update's arguments without the context and the outcome arrays; default: that call on ctx
 * srl_oft_use_device_consensus (the reference's setIntrinsic, :104-109, plus its two cv:: calls) installs as the fundamental and the PnP
 * provider this library's own estimators on the handle's context: srl_consensus_fundamental and srl_consensus_pnp (srlivo_hip.h) with
 * the intrinsics fx, fy, cx, cy and the options given (NULL: srl_consensus_opts_default of either model).  They are NOT OpenCV's
 * results; they stand in because the reference reads only the mask / inlier list, which in OpenCV depends on its private generator.
 * A handle made with a NULL ctx: SRL_ERR_NO_DEVICE; intrinsics or options srl_consensus_* would refuse: their status (SRL_ERR_BAD_ARG;
 * a context with more than one rank: SRL_ERR_UNSUPPORTED), nothing installed -- the rules are theirs and are asked of them.  A provider set later with srl_oft_set_fundamental_provider / srl_oft_set_pnp_provider replaces it.  While it is in
 * place a failing device call is the status of srl_oft_track_image / srl_oft_remove_outlier_using_ransac_pnp, never the "caught
 * cv::Exception" path.  Without this call (and without providers) both steps refuse as before.  srl_oft_last_consensus: the result
 * record of the handle's last device call, which = 0 fundamental, 1 PnP (zeros before the first).
 * srl_oft_use_prepared_image(oft, on): with on != 0 srl_oft_init and srl_oft_track_image ignore their gray argument (NULL included: it is
 * no longer the empty image) and the default flow step calls srl_flow_track_prepared on the handle's context, i.e. tracks on the gray
 * image the last srl_image_prepare left on the device; the caller prepares every frame before it tracks.  Without the opt-in nothing
 * changes; a flow provider still takes precedence (and is handed the arguments as given).  A handle made with a NULL ctx:
 * SRL_ERR_NO_DEVICE.
 * srl_oft_init = init (:188-197) on rgb_points_vec / points_2d_vec as selection records; srl_oft_track_image = trackImage (:111-186):
 * gray == NULL is the empty image, fewer than 30 points only move the time, *n_cur = map_rgb_points_in_cur_image_pose.size();
 * image_rows / image_cols are the frame's (if2dPointsAvailable(x, y, 1.0, 0.05)); rejectErrorTrackingPoints is not built (the reference
 * switches it off with distance = -20).  srl_oft_remove_outlier_using_ransac_pnp (:267-323): *accepted = its return value.
 * srl_oft_update_and_append_track_points (:13-102): candidates = points_rgb_vec_for_projection as the selection returned it; a point
 * that left the set flagged comes back flagged.  srl_oft_pose_map: which = 0 map_rgb_points_in_last_image_pose, 1 ..._cur_...; out
 * may be NULL (the size alone), flagged = is_out_lier_count.  srl_oft_tracked_for_vio: the list srl_color_map_vio_rows takes. */
typedef struct srl_oft srl_oft;
typedef int (*srl_oft_flow_provider)(const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, const float *prev_xy, int n, float *next_xy,
                                     uint8_t *status, void *user);
typedef int (*srl_oft_fundamental_provider)(const float *last_xy, const float *cur_xy, int n, uint8_t *status, void *user);
typedef int (*srl_oft_pnp_provider)(const float *xyz, const float *uv, int n, int32_t *inliers, int *n_inliers, void *user);
typedef int (*srl_oft_update_provider)(const srl_color_camera *cam, int image_rows, int image_cols, const srl_color_track_point *tracked, int n,
                                       const int32_t *candidates, int n_candidates, const srl_color_track_opts *opts, srl_color_track_point *out,
                                       int64_t capacity, srl_color_track_totals *totals, void *user);
int srl_oft_create(srl_ctx *ctx, srl_oft **out);
int srl_oft_destroy(srl_oft *oft);
int srl_oft_set_maximum_tracked_points(srl_oft *oft, int maximum_tracked_points);
int srl_oft_set_flow_provider(srl_oft *oft, srl_oft_flow_provider fn, void *user);
int srl_oft_set_fundamental_provider(srl_oft *oft, srl_oft_fundamental_provider fn, void *user);
int srl_oft_set_pnp_provider(srl_oft *oft, srl_oft_pnp_provider fn, void *user);
int srl_oft_set_update_provider(srl_oft *oft, srl_oft_update_provider fn, void *user);
int srl_oft_use_device_consensus(srl_oft *oft, const double *fx_fy_cx_cy, const srl_consensus_opts *fundamental /* NULL = default */,
                                 const srl_consensus_opts *pnp /* NULL = default */);
int srl_oft_last_consensus(srl_oft *oft, int which /* 0 fundamental, 1 pnp */, srl_consensus_result *out);
int srl_oft_use_prepared_image(srl_oft *oft, int on);
int srl_oft_set_track_points(srl_oft *oft, const srl_color_selected *records, int n);
int srl_oft_init(srl_oft *oft, const srl_color_selected *records, int n, const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes,
                 double time_sweep_end);
int srl_oft_track_image(srl_oft *oft, const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, double time_sweep_end, int image_rows,
                        int image_cols, int *n_cur);
int srl_oft_remove_outlier_using_ransac_pnp(srl_oft *oft, int if_remove_outlier, int *accepted);
int srl_oft_update_and_append_track_points(srl_oft *oft, const srl_color_camera *cam, int image_rows, int image_cols,
                                           const srl_color_selected *candidates, int n_candidates, double mini_distance,
                                           srl_color_track_totals *totals /* or NULL */);
int srl_oft_sizes(srl_oft *oft, int *last_pose, int *cur_pose, int *last_tracked, int *flagged);
int srl_oft_times(srl_oft *oft, double *last_image_time, double *current_image_time);
int srl_oft_pose_map(srl_oft *oft, int which, srl_color_track_point *out, int capacity, int *n);
int srl_oft_tracked_for_vio(srl_oft *oft, srl_color_vio_point *out, int capacity, int *n);

/* ------------------------------------------------------------------ one camera frame end to end (csrc/host/imageProcessing.{h,cpp})
 * imageProcessing::process (imageProcessing.cpp:89-164), statement by statement, on the camera state the handle keeps
 * (srl_lio_vio_set_camera_state / _get_camera_state) and on an opticalFlowTracker, an image preparer and the colour-map bookkeeping
 * the handle owns.  A frame runs, in this order:
 *   first data (:91-111)   image_scale_factor = image_width image_resize_ratio / cols of the frame; the four intrinsics of
 *                          srl_lio_vio_set_options divided by it, for good; the preparer created at (int)(image_height / scale) rows x
 *                          (int)(image_width / scale) columns with them and the distortion coefficients (srl_image_prep_create); the
 *                          tracker's setIntrinsic = srl_oft_use_device_consensus with them; maximum_tracked_points and the depth limits
 *                          handed on
 *   prepare (:113-125)     srl_image_prepare_resized iff fabs(image_resize_ratio - 1.0) > 1e-6, else srl_image_prepare; the tracker
 *                          follows on the prepared gray image (srl_oft_use_prepared_image)
 *   first data (:127-135)  the selection with minimum_dis = track_windows_size / scale, skip 1, and init
 *   every frame (:137-163) trackImage; removeOutlierUsingRansacPnp; vioEsikf and vioPhotometric, both only when PnP accepted; the
 *                          render with obs_time = time_sweep_end and the camera as the two updates left it; updatePoseForProjection
 *                          with a margin of -0.4; refreshPointsForProjection (nothing on a frame_id it has refreshed for already);
 *                          updateAndAppendTrackPoints with track_windows_size / scale; time_last_process = time_sweep_end, which the
 *                          handle's next colour insertion reads -- srl_lio_set_color_times is not needed on this path.
 * image_rows / image_cols of every projection test are the RAW frame's, as in the reference (lioOptimization.cpp:1080-1081); the render
 * tests against the prepared image it reads.  The colour map must exist (srl_lio_set_color_map_options).
 * Every step that leaves the mirror goes through a table of step functions whose defaults are the device calls named above;
 * srl_lio_image_set_steps replaces any of them (NULL members keep the default; a NULL table puts every default back) so that a test
 * can record order, gates and arguments without a device.  A step returns a srl_status; a failing step ends the frame with that
 * status and no later step runs; *out holds what the frame reached.  The frame may be offered again: of the first data nothing is done
 * twice (the intrinsics are scaled once, the preparer is created once, the consensus setup runs once), and the first selection and init
 * run until they have succeeded.  A replaced fundamental or pnp step holds from the first frame on, also behind the default consensus
 * setup; a member that goes back to NULL gets the device call back.  select: write at most `capacity` records and set *n; with *n >
 * capacity return SRL_ERR_BAD_ARG and the call is repeated with room for *n.
 * SRL_ERR_BAD_ARG: NULL lio or image, rows or cols < 1, a stride below a row, options never set.  A host-only handle with a step left
 * at its default: SRL_ERR_NO_DEVICE, never a host loop.  A context of more than one rank: SRL_ERR_UNSUPPORTED (the preparer's and
 * the consensus calls' own refusal).
 * srl_lio_image_oft: the handle's tracker, for the srl_oft_* read-backs (owned by the handle; NULL lio: NULL).
 * srl_lio_image_candidates: points_rgb_vec_for_projection as the last refresh left it (capacity 0 asks for the number alone). */
typedef struct srl_image_process_opts {
    int32_t image_width, image_height;          /* setImageWidth / setImageHeight */
    double image_resize_ratio;                  /* imageProcessing.cpp:11: 1.0 */
    double dist[5];                             /* camera_dist_coeffs: k1 k2 p1 p2 k3 */
    double track_windows_size;                  /* :15: 40 */
    int32_t maximum_tracked_points, reserved;   /* :14: 300 */
    double tracker_minimum_depth, tracker_maximum_depth;      /* :17-18: 0.1, 200 */
} srl_image_process_opts;
typedef struct srl_image_process_result {
    int32_t first_data, prepared_rows, prepared_cols;
    int32_t tracked_after_flow, tracked_after_pnp, pnp_accepted;      /* map_rgb_points_in_cur_image_pose.size() behind either step */
    int32_t esikf_accepted, esikf_iterations, esikf_used;
    int32_t photometric_accepted, photometric_iterations, photometric_used;
    int32_t refreshed_candidates, reserved;
    double image_scale_factor;
    srl_color_render_totals render;
    srl_color_track_totals track;
} srl_image_process_result;
typedef struct srl_image_process_steps {
    void *user;
    int (*prep_create)(const srl_image_prep_opts *opts, void *user);
    int (*prepare)(const uint8_t *raw_bgr, int rows, int cols, int64_t row_stride_bytes, int resized, void *user);
    int (*consensus_setup)(const double *fx_fy_cx_cy, void *user);
    int (*select)(const srl_color_camera *cam, int image_rows, int image_cols, const srl_color_select_opts *opts, int refresh, srl_color_selected *out,
                  int capacity, int *n, void *user);
    srl_oft_flow_provider flow;
    srl_oft_fundamental_provider fundamental;
    srl_oft_pnp_provider pnp;
    srl_vio_rows_provider rows;
    int (*render)(const srl_color_camera *cam, double obs_time, srl_color_render_totals *totals, void *user);
    srl_oft_update_provider track_update;
} srl_image_process_steps;
void srl_image_process_opts_default(srl_image_process_opts *o);      /* the reference's constructor values; width, height, dist 0 */
int srl_lio_image_set_options(srl_lio *lio, const srl_image_process_opts *opts);
int srl_lio_image_set_steps(srl_lio *lio, const srl_image_process_steps *steps);
int srl_lio_image_process(srl_lio *lio, const uint8_t *raw_bgr, int rows, int cols, int64_t row_stride_bytes, double time_sweep_end, int frame_id,
                          srl_image_process_result *out /* or NULL */);
srl_oft *srl_lio_image_oft(srl_lio *lio);
int srl_lio_image_candidates(srl_lio *lio, srl_color_selected *out, int capacity, int *n);
int srl_lio_image_time_last_process(srl_lio *lio, double *time_last_process);
/* srl_lio_run_measurement with the measurement's camera frame: lioOptimization::process (lioOptimization.cpp:1037-1086) with to_rendering
 * set.  raw_bgr == NULL: no image -- exactly srl_lio_run_measurement, whatever the other image arguments hold.  Otherwise the sweep is
 * inserted into the colour map with to_rendering, and behind stateEstimation, before the sliding window moves:
 *   :1053-1071  fx fy cx cy, R_imu_camera and t_imu_camera of the handle's camera state are set from the configured values
 *               (srl_lio_vio_set_options; the intrinsics as process's first data scaled them) while all_cloud_frame.size() < 3 and
 *               otherwise left as the frame before left them, camera updates included;
 *   :1073-1075  rotation and translation are the frame's, q_world_camera = rotation R_imu_camera, t_world_camera = rotation t_imu_camera
 *               + translation;
 *   :1077-1083  srl_lio_image_process's frame with time_sweep_end and frame_id of the sweep; *image_out (optional) is its record.
 * The camera frame also runs behind a stateEstimation that failed (the reference's process does not look at the summary, :1049-1083;
 * the sweep is then in neither map and the pose is the prior), and *image_out is its record.  Returns the first failure: the arguments',
 * srl_lio_run_measurement's (SRL_ERR_NOT_ENOUGH_RESIDUALS included), then the camera frame's.  A measurement that only feeds the filter's
 * initialisation runs no camera frame. */
int srl_lio_run_measurement_image(srl_lio *lio, double time_frame, const double *imu_t, const double *imu_acc, const double *imu_gyr, int n_imu,
                                  const double *pts_raw, const double *pts_timestamp, int n_pts, double time_sweep_begin, double time_sweep_offset,
                                  const uint8_t *raw_bgr, int rows, int cols, int64_t row_stride_bytes, srl_replay_result *out,
                                  srl_image_process_result *image_out /* or NULL */);
/* Compressed camera frames: lioOptimization::compressedImageHandler (lioOptimization.cpp:640-664: toCvCopy(msg, BGR8) of a
 * sensor_msgs/CompressedImage) followed by process.  srl_lio_image_process_jpeg is srl_lio_image_process on a baseline JPEG stream: rows
 * and cols -- for image_scale_factor and for every projection test -- come from srl_jpeg_parse (host only: no device is asked for them),
 * and the prepare step becomes the JPEG step, whose default is srl_image_prepare_jpeg: the stream is entropy-decoded on the host, the
 * frame is built on the device and prepared where it lies; the resize runs whenever the frame's size differs from the preparer's, so
 * image_resize_ratio only sets the preparer's size here.  Every other statement is srl_lio_image_process's, one body for both.
 * srl_lio_image_set_jpeg_step replaces the step (NULL: the default again); it is not a member of srl_image_process_steps, whose layout
 * stays as it is, and survives srl_lio_image_set_steps.  A host-only handle with the step at its default: SRL_ERR_NO_DEVICE, as for the
 * table's members.  SRL_ERR_BAD_ARG: NULL lio or bytes, n < 2, options never set; a stream srl_jpeg_parse refuses returns its status
 * (SRL_ERR_BAD_ARG or SRL_ERR_UNSUPPORTED) before any step runs, *out zeroed.
 * srl_lio_run_measurement_image_jpeg is srl_lio_run_measurement_image with the frame given as such a stream (bytes == NULL: no image). */
typedef int (*srl_image_jpeg_step)(const uint8_t *bytes, int64_t n, void *user);
int srl_lio_image_set_jpeg_step(srl_lio *lio, srl_image_jpeg_step fn, void *user);
int srl_lio_image_process_jpeg(srl_lio *lio, const uint8_t *bytes, int64_t n, double time_sweep_end, int frame_id, srl_image_process_result *out /* or NULL */);
int srl_lio_run_measurement_image_jpeg(srl_lio *lio, double time_frame, const double *imu_t, const double *imu_acc, const double *imu_gyr, int n_imu,
                                       const double *pts_raw, const double *pts_timestamp, int n_pts, double time_sweep_begin, double time_sweep_offset,
                                       const uint8_t *bytes, int64_t n, srl_replay_result *out, srl_image_process_result *image_out /* or NULL */);

/* lioOptimization::searchNeighbors / computeNeighborhoodDistribution single-call forms */
int srl_lio_search_neighbors(srl_lio *lio, const double point[3], int nb_voxels_visited, double size_voxel_map,
                             int max_num_neighbors, int threshold_voxel_capacity, double *out_xyz /* K x 3 */,
                             int16_t *out_voxels /* K x 3 or NULL */, int *num_found);
int srl_lio_neighborhood(srl_lio *lio, const double *pts, int n, double center[3], double normal[3],
                         double cov[9], double *a2D);

/* lioOptimization::buildPlaneResiduals, signature-compatible form (materialises the residual list):
 * outputs for the accepted residuals in order: raw_point(3) norm_vector(3) jacobians(6) norm_offset
 * distance weight = 15 doubles each, capacity max_out rows. */
int srl_lio_build_plane_residuals(srl_lio *lio, const srl_icp_opts *opts, const double *raw_xyz, int n,
                                  const double state[16], const double t_last[3], int frame_id,
                                  double *out_rows, int max_out, int *num_out, double *loss_sum,
                                  int *success, double *keypoint_world /* n x 3 or NULL */);

/* gridSampling (utility.cpp:188-201) alone: indices of the selected points, in output order */
int srl_grid_sampling(const double *world_xyz, int n, double size_voxel, int32_t *index_out, int *num_out);
/* debug / parity hook: iteration order of the std::tr1::unordered_map<voxel, ...> of subSampleFrame (utility.cpp:169-185) after
 * inserting n DISTINCT voxel keys in the given order, by the flat replay of the container's bucket moves that
 * srl_frame_select_keypoints uses (csrc/host/tr1_order.h; no container is built).  order_out[r] = index of the r-th element. */
int srl_debug_tr1_order(const int16_t *keys_xyz, int n, int32_t *order_out);
/* ... and the same order computed the way the DEVICE does it for frames that fit (csrc/host/tr1_relation.h: the container's iteration
 * order as a relation between two elements -- no replay; the functions the kernels call, compiled for the host). */
int srl_debug_tr1_order_by_relation(const int16_t *keys_xyz, int n, int32_t *order_out);

#ifdef __cplusplus
}
#endif
#endif

// imageProcessing.h (host mirror) -- the camera ESIKF of class imageProcessing (include/imageProcessing.h, src/imageProcessing.cpp:
// setInitialCov :65-72, vioEsikf :220-380, vioPhotometric :402-552, both updateCameraParameters :382-400, :554-566) without ROS and
// without OpenCV.  The per-point loops of the two updates are one call each iteration (srl_color_map_vio_rows, or a provider with its
// signature); what surrounds them is written statement by statement.  One algebraic difference: the reference forms the 11 x 2N gain K
// explicitly; here A = HtH + (J0 P J0^T w)^-1, K r = A^-1 Htr and K H = A^-1 HtH come from the call's sums.
// Optical flow is lkpyramid.h of this directory and the tracker's bookkeeping opticalFlowTracker.h; PnP / RANSAC (srl_consensus_*) and the
// undistortion and equalisation of the image (srl_image_prepare) are the device library's own specified operations, not OpenCV's.
// process (:89-164) joins them: one camera frame from the raw image to the topped-up track set, statement by statement, every step
// that leaves the mirror taken from a table of step functions (processSteps) whose defaults are the device calls.
#pragma once
#include "../../../include/srlivo_host.h"
#include "cameraState.h"
#include "opticalFlowTracker.h"
#include "srl_la.h"

#include <functional>
#include <string>
#include <vector>

#define SRL_VIO_INIT_COV (0.0001)      // include/imageProcessing.h:22

namespace srlivo {

// what process reads of its cloudFrame (lioOptimization.cpp:1079-1081): the raw image, its size, the sweep's end and the frame's number
struct imageFrame {
    const uint8_t *rgb_image = nullptr;
    const uint8_t *jpeg = nullptr;                         // compressedImageHandler's frame: a baseline JPEG stream instead of rgb_image;
    int64_t jpeg_bytes = 0;                                // image_rows / image_cols are then what srl_jpeg_parse read from it
    int image_rows = 0, image_cols = 0;
    int64_t row_stride_bytes = 0;
    double time_sweep_end = 0.0;
    int frame_id = 0;
};

// The steps of process that leave the mirror, each returning a srl_status; a failing step ends the frame with its status.  The flow, the
// two consensus calls and the track-update are the providers of the opticalFlowTracker the object works on, the measurement pass is
// `rows`; the rest is here.  The handle (srl_host_capi.cpp) fills in the device calls, a test its recording stand-ins.
struct processSteps {
    std::function<int(const srl_image_prep_opts &)> prepCreate;                                      // initUndistortRectifyMap (:103): srl_image_prep_create
    std::function<int(const uint8_t *raw, int rows, int cols, int64_t stride, bool resized)> prepare;      // :113-125: srl_image_prepare(_resized)
    std::function<int(const uint8_t *bytes, int64_t n)> prepareJpeg;                                  // the same for a frame that came compressed: srl_image_prepare_jpeg
    std::function<int(const double *fx_fy_cx_cy)> consensusSetup;                                     // setIntrinsic (:106): useDeviceConsensus
    // selectPointsForProjection (:131) and, with refresh set, the one inside refreshPointsForProjection (:159)
    std::function<int(const srl_color_camera &, int rows, int cols, const srl_color_select_opts &, bool refresh, std::vector<srl_color_selected> &)> select;
    std::function<int(const srl_color_camera &, double obs_time, srl_color_render_totals &)> render;      // renderPointsInRecentVoxel (:155)
};

class imageProcessing {
public:
    using RowsProvider = std::function<int(const srl_color_vio_args *, const srl_color_vio_point *, int, srl_color_vio_sums *)>;

    srl::Mat<11, 11> covariance;
    int num_iterations = 2;                              // imageProcessing.cpp:20
    double cam_measurement_weight = 1e-3;                // :22
    bool ifEstimateCameraIntrinsic = true, ifEstimateExtrinsic = true;      // :24-25
    srl::Mat3 camera_intrinsic = srl::Mat3::Identity();
    srl::Mat3 R_imu_camera = srl::Mat3::Identity();
    srl::Vec3 t_imu_camera = srl::Vec3::Zero();
    RowsProvider rows;                                   // the measurement pass of one iteration
    int status = 0;                                      // the provider's last status (SRL_OK, or what stopped an update)
    std::vector<cameraState> iterations;                 // the state behind every updateCameraParameters of the last update
    int last_used = 0;                                   // num_used_point_count of the last iteration

    imageProcessing() { setInitialCov(); }
    void setInitialCov();
    // tracked: map_rgb_points_in_last_image_pose in the caller's order; total_point_size (map_rgb_points_in_cur_image_pose.size() in the
    // reference, :247, :413) is taken as its length: the two maps are assumed to have one size
    bool vioEsikf(cameraState &st, const srl_color_vio_point *tracked, int n, int number_of_new_visited_voxel);
    bool vioPhotometric(cameraState &st, const srl_color_vio_point *tracked, int n, int number_of_new_visited_voxel);
    void updateCameraParameters(cameraState &st, const srl::Mat<11, 1> &d_x);
    void updateCameraParameters(cameraState &st, const srl::Mat<6, 1> &d_x);

    // ---- process (:89-164) and what it reads (:6-27)
    int image_width = 0, image_height = 0;               // setImageWidth / setImageHeight
    double image_resize_ratio = 1.0;                     // :11
    double image_scale_factor = 1.0;                     // :12
    double camera_dist_coeffs[5] = {0, 0, 0, 0, 0};      // k1 k2 p1 p2 k3
    int maximum_tracked_points = 300;                    // :14
    double track_windows_size = 40;                      // :15
    double tracker_minimum_depth = 0.1, tracker_maximum_depth = 200;      // :17-18
    bool first_data = true;                              // :27
    int first_data_stage = 0;                            // what of :91-111 is done for good: 1 the scale, the intrinsics and the preparer, 2 the consensus setup
    double time_last_process = -1e5;                     // :6
    int prepared_rows = 0, prepared_cols = 0;            // cv::Size(image_width / image_scale_factor, image_height / image_scale_factor)
    opticalFlowTracker *op_tracker = nullptr;            // the handle's
    processSteps steps;
    // map_tracker: the depth limits (:109-110), p_cloud_frame as updatePoseForProjection leaves it (rgbMapTracker.cpp:154-174),
    // updated_frame_index (:16) and points_rgb_vec_for_projection
    double minimum_depth_for_projection = 0.1, maximum_depth_for_projection = 200;
    srl_color_camera projection_camera = {};
    int projection_rows = 0, projection_cols = 0, projection_frame_id = 0, updated_frame_index = -1;
    std::vector<srl_color_selected> points_for_projection;
    // one frame on the camera state st.  number_of_new_visited_voxel: map_tracker's, as the last insertion left it.  Returns a
    // srl_status: SRL_OK, or what the first failing step returned (later steps are not run); *result is filled as far as the frame got
    int process(cameraState &st, const imageFrame &frame, int number_of_new_visited_voxel, srl_image_process_result *result);

private:
    int measure(const cameraState &st, int mode, const srl_color_vio_point *tracked, int n, srl_color_vio_sums *sums);
};

}  // namespace srlivo

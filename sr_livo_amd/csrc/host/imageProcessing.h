// imageProcessing.h (host mirror) -- the camera ESIKF of class imageProcessing (include/imageProcessing.h, src/imageProcessing.cpp:
// setInitialCov :65-72, vioEsikf :220-380, vioPhotometric :402-552, both updateCameraParameters :382-400, :554-566) without ROS and
// without OpenCV.  The per-point loops of the two updates are one call each iteration (srl_color_map_vio_rows, or a provider with its
// signature); what surrounds them is written statement by statement.  One algebraic difference: the reference forms the 11 x 2N gain K
// explicitly; here A = HtH + (J0 P J0^T w)^-1, K r = A^-1 Htr and K H = A^-1 HtH come from the call's sums.
// Optical flow is lkpyramid.h of this directory and the tracker's bookkeeping opticalFlowTracker.h; PnP / RANSAC (srl_consensus_*) and the
// undistortion and equalisation of the image (srl_image_prepare) are the device library's own specified operations, not OpenCV's.
#pragma once
#include "../../../include/srlivo_hip.h"
#include "cameraState.h"
#include "srl_la.h"

#include <functional>
#include <string>
#include <vector>

#define SRL_VIO_INIT_COV (0.0001)      // include/imageProcessing.h:22

namespace srlivo {

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

private:
    int measure(const cameraState &st, int mode, const srl_color_vio_point *tracked, int n, srl_color_vio_sums *sums);
};

}  // namespace srlivo

// opticalFlowTracker.h (host mirror) -- class opticalFlowTracker (include/opticalFlowTracker.h, src/opticalFlowTracker.cpp) without
// OpenCV: the bookkeeping that ties srl_color_map_select, srl_flow_track_image, srl_color_map_vio_rows and
// srl_color_map_track_update into the loop of imageProcessing::process (imageProcessing.cpp:137-161).  The optical flow and
// updateAndAppendTrackPoints are one device call each (or a provider with its signature).  cv::findFundamentalMat and
// cv::solvePnPRansac are reached through providers: the caller's own OpenCV, or -- after useDeviceConsensus -- this library's consensus
// estimators on the handle's context (srl_consensus_fundamental, srl_consensus_pnp).  Those are NOT OpenCV's results and claim no
// parity with them; they stand in soundly because the reference reads only the inlier mask / list of either call, and OpenCV's own
// mask depends on its private random generator.  With neither, both steps refuse.
//
// State is kept by POOL POSITION (srl_color_selected.pool) where the reference keys by rgbPoint pointer: wherever it iterates a
// std::map keyed by pointer value -- an order that is not reproducible -- the mirror iterates by ascending pool position
// (updateLastTrackingVectorAndIds, removeOutlierUsingRansacPnp's lists, trackedForVio).  What the reference keeps inside the rgbPoint is
// kept here per pool position: image_velocity (zero for a point no trackImage accepted yet; the reference leaves it uninitialised) and
// is_out_lier_count, as the sparse set of positions whose count is 1 -- a point that left the set flagged comes back flagged, which is
// overlaid on the points srl_color_map_track_update adds (it returns them with flag 0).
//
// The velocity statement (:167) is `(cur - last) / frame_time_diff` on cv::Point2f: written here as OpenCV's operators read -- the
// difference of two Point2f in float, Point_<float> / double as saturate_cast<float>((double) x / b), i.e. a double quotient rounded to
// float.  Nothing in this tree can confirm OpenCV's Point_ operators: there is no OpenCV on the machines this is built and tested on,
// and the stand-in headers of the tests are not OpenCV.
//
// rejectErrorTrackingPoints (:213-245) is not built: the reference's own call passes distance = -20, which switches it off (:173), and
// its loop erases the element it then increments.  The images the reference clones (old_image, old_gray) live in the device tracker.
#pragma once
#include "../../../include/srlivo_hip.h"
#include "lkpyramid.h"

#include <array>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <vector>

namespace srlivo {

class opticalFlowTracker {
public:
    // srl_flow_track_image without the context; returns a srl_status
    using FlowProvider = std::function<int(const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, const float *prev_xy, int n, float *next_xy,
                                           uint8_t *status)>;
    // the mask of cv::findFundamentalMat(last, cur, FM_RANSAC, 1.0, 0.997, status): n bytes
    using FundamentalProvider = std::function<int(const float *last_xy, const float *cur_xy, int n, uint8_t *status)>;
    // the inlier list of cv::solvePnPRansac(points_3d, points_2d, intrinsic, ..., 200, 1.5, 0.99, status): indices into the n points; a
    // status other than SRL_OK stands for the cv::Exception the reference catches
    using PnpProvider = std::function<int(const float *xyz, const float *uv, int n, int32_t *inliers, int *n_inliers)>;
    // srl_color_map_track_update without the context and the outcome arrays
    using UpdateProvider = std::function<int(const srl_color_camera *cam, int image_rows, int image_cols, const srl_color_track_point *tracked, int n,
                                             const int32_t *candidates, int n_candidates, const srl_color_track_opts *opts, srl_color_track_point *out,
                                             int64_t capacity, srl_color_track_totals *totals)>;

    explicit opticalFlowTracker(srl_ctx *ctx);

    int maximum_tracked_points = 300;                                       // :10
    std::map<int32_t, Point2f> map_rgb_points_in_last_image_pose, map_rgb_points_in_cur_image_pose;
    std::vector<Point2f> last_tracked_points, cur_tracked_points;
    std::vector<int32_t> rgb_points_ptr_vec_in_last_image;                  // pool positions
    std::vector<int> old_ids;
    std::map<int32_t, std::array<double, 2>> image_velocity;               // rgbPoint::image_velocity
    std::set<int32_t> out_lier_flagged;                                     // rgbPoint::is_out_lier_count == 1
    std::map<int32_t, std::array<float, 3>> position;                       // getPosition() of every point the set has held (stored FP32)
    double last_image_time = 0.0, current_image_time = 0.0;
    unsigned image_idx = 0;
    srl_color_track_totals update_totals = {};                              // of the last updateAndAppendTrackPoints
    int status = 0;                                                         // the last provider's or device call's srl_status

    FlowProvider flow;                                                      // default: the object's LKOpticalFlowKernel on ctx
    FundamentalProvider fundamental;                                        // none: trackImage refuses with SRL_ERR_BAD_ARG
    PnpProvider pnp;                                                        // none: removeOutlierUsingRansacPnp refuses with SRL_ERR_BAD_ARG
    UpdateProvider update;                                                  // default: srl_color_map_track_update on ctx
    // useDeviceConsensus: setIntrinsic (:104-109) plus the two cv:: calls on ctx.  A provider set later replaces it.  While it is in
    // place a failing PnP call is a failure of the handle (status), not the cv::Exception the reference catches
    bool pnp_is_device = false;
    double intrinsic[4] = {0.0, 0.0, 0.0, 0.0};                             // fx, fy, cx, cy
    srl_consensus_opts consensus_opts[2] = {};                              // [0] fundamental, [1] PnP
    srl_consensus_result last_consensus[2] = {};                            // of the last device call of either kind (zeros: none yet)
    int useDeviceConsensus(const double *fx_fy_cx_cy, const srl_consensus_opts *fundamental_opts, const srl_consensus_opts *pnp_opts);
    // usePreparedImage: init and trackImage ignore their gray argument (NULL included) and the default flow step tracks on the image
    // srl_image_prepare left on ctx (srl_flow_track_prepared).  A flow provider still takes precedence and gets the arguments as given
    bool use_prepared_image = false;
    int usePreparedImage(bool on);

    // :188-197; records: rgb_points_vec with points_2d_vec (pool, position, u, v).  false: a call refused or failed (status)
    bool init(const srl_color_selected *records, int n, const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, double time_sweep_end);
    void setTrackPoints(const srl_color_selected *records, int n);          // :199-211
    void updateLastTrackingVectorAndIds();                                  // :247-265
    // :111-186; gray == nullptr is the reference's empty image.  image_rows / image_cols: the frame's (if2dPointsAvailable)
    bool trackImage(const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, double time_sweep_end, int image_rows, int image_cols);
    // :267-323; *accepted = what the reference's function returns
    bool removeOutlierUsingRansacPnp(int if_remove_ourlier, bool *accepted);
    // :13-102; candidates: points_rgb_vec_for_projection as the selection returned it
    bool updateAndAppendTrackPoints(const srl_color_camera *cam, int image_rows, int image_cols, const srl_color_selected *candidates, int n_candidates,
                                    double mini_distance);
    // map_rgb_points_in_last_image_pose with each point's image_velocity, as vioEsikf and vioPhotometric read them
    std::vector<srl_color_vio_point> trackedForVio() const;

private:
    srl_ctx *ctx;
    std::unique_ptr<LKOpticalFlowKernel> lk_optical_flow_kernel;
    int flowCall(const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, const std::vector<Point2f> &last, std::vector<Point2f> &cur,
                 std::vector<uint8_t> &st);
};

}  // namespace srlivo

// the C handle of include/srlivo_host.h (srl_oft_*): opticalFlowTracker.cpp, and opticalFlowTrackerDevice.cpp for the two functions
// that reach srl_consensus_* -- a translation unit of their own, so that the mirror links without the device library
struct srl_oft {
    srlivo::opticalFlowTracker t;
    explicit srl_oft(srl_ctx *ctx) : t(ctx) {}
};

// lkpyramid.h (host mirror) -- class LKOpticalFlowKernel (include/lkpyramid.h, src/lkpyramid.cpp:627-795) without OpenCV: the
// reference's constructor arguments, its setTerminationCriteria clamping (:670-682) and trackImage (:755-795) on a raw gray buffer.  The
// pyramid, the derivative and the track are one call on the device (srl_flow_track_image, csrc/srl_flow.hip); nothing of them is
// computed here and there is no host loop to fall back to.  The object owns the context's one device tracker, which it creates at
// the first image with the clamped criteria.  findFundamentalMat stays with the caller; the rest of
// opticalFlowTracker is opticalFlowTracker.h of this directory.
#pragma once
#include "../../../include/srlivo_hip.h"

#include <cstdint>
#include <functional>
#include <vector>

namespace srlivo {

struct Size { int width = 0, height = 0; };
struct Point2f { float x = 0.f, y = 0.f; };
struct TermCriteria {
    enum { COUNT = 1, MAX_ITER = COUNT, EPS = 2 };
    int type = COUNT + EPS;
    int maxCount = 30;
    double epsilon = 0.01;
};

class LKOpticalFlowKernel {
public:
    LKOpticalFlowKernel(srl_ctx *ctx, Size winSize_ = Size{21, 21}, int maxLevel_ = 3, TermCriteria criteria_ = TermCriteria(), int flags_ = 0,
                        double minEigThreshold_ = 1e-4);
    ~LKOpticalFlowKernel();
    LKOpticalFlowKernel(const LKOpticalFlowKernel &) = delete;
    LKOpticalFlowKernel &operator=(const LKOpticalFlowKernel &) = delete;

    Size getWinSize() const { return lk_win_size; }
    int getMaxLevel() const { return maxLevel; }
    TermCriteria getTermCriteria() const { return terminate_criteria; }
    int getFlags() const { return flags; }
    double getMinEigThreshold() const { return minEigThreshold; }
    // as in the reference the argument is not read: the member is clamped in place
    void setTerminationCriteria(TermCriteria &crit);

    // curr_tracked_pts = last_tracked_pts on the first image (status untouched, 0 returned); otherwise every point's new position and
    // status, and the number of status == 1.  -1 when the device call refused or failed: last_status then holds its srl_status.
    int trackImage(const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, const std::vector<Point2f> &last_tracked_pts,
                   std::vector<Point2f> &curr_tracked_pts, std::vector<uint8_t> &status);
    int last_status = 0;
    // when set, stands where trackImage calls srl_flow_track_image: the image is then whatever the hook tracks on, and gray, rows, cols and
    // the stride are not read (opticalFlowTracker::usePreparedImage: srl_flow_track_prepared on ctx).  It returns a srl_status.
    std::function<int(const float *prev_xy, int n, float *next_xy, uint8_t *status, int *n_tracked)> device_track;

private:
    srl_ctx *ctx;
    bool created = false, seen_image_ = false;
    Size lk_win_size;
    int maxLevel;
    TermCriteria terminate_criteria;
    int flags;
    double minEigThreshold;
};

}  // namespace srlivo

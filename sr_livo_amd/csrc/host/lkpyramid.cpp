// lkpyramid.cpp (host mirror) -- see lkpyramid.h.  The C handle of include/srlivo_host.h (srl_lk_*) is at the end of this file.
#include "lkpyramid.h"
#include "../../../include/srlivo_hip_debug.h"
#include "../../../include/srlivo_host.h"

#include <algorithm>
#include <cstring>
#include <new>

namespace srlivo {

LKOpticalFlowKernel::LKOpticalFlowKernel(srl_ctx *ctx_, Size winSize_, int maxLevel_, TermCriteria criteria_, int flags_, double minEigThreshold_)
    : ctx(ctx_), lk_win_size(winSize_), maxLevel(maxLevel_), terminate_criteria(criteria_), flags(flags_), minEigThreshold(minEigThreshold_) {
    setTerminationCriteria(terminate_criteria);
}

LKOpticalFlowKernel::~LKOpticalFlowKernel() {
    if (created) srl_flow_destroy(ctx);
}

void LKOpticalFlowKernel::setTerminationCriteria(TermCriteria &) {      // lkpyramid.cpp:670-682
    if ((terminate_criteria.type & TermCriteria::COUNT) == 0)
        terminate_criteria.maxCount = 30;
    else
        terminate_criteria.maxCount = std::min(std::max(terminate_criteria.maxCount, 0), 100);

    if ((terminate_criteria.type & TermCriteria::EPS) == 0)
        terminate_criteria.epsilon = 0.01;
    else
        terminate_criteria.epsilon = std::min(std::max(terminate_criteria.epsilon, 0.), 10.);
}

int LKOpticalFlowKernel::trackImage(const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, const std::vector<Point2f> &last_tracked_pts,
                                    std::vector<Point2f> &curr_tracked_pts, std::vector<uint8_t> &status) {
    static_assert(sizeof(Point2f) == 2 * sizeof(float), "a vector of Point2f is n x 2 floats");
    if (last_tracked_pts.size() > (size_t)SRL_FLOW_MAX_POINTS) { last_status = SRL_ERR_BAD_ARG; return -1; }
    if (!created) {
        if (lk_win_size.width != lk_win_size.height) { last_status = SRL_ERR_UNSUPPORTED; return -1; }
        srl_flow_opts o;
        srl_flow_opts_default(&o);
        o.win = lk_win_size.width; o.max_level = maxLevel; o.max_count = terminate_criteria.maxCount;
        o.epsilon = terminate_criteria.epsilon; o.min_eig_threshold = minEigThreshold;
        last_status = srl_flow_create(ctx, &o);
        if (last_status != SRL_OK) return -1;
        created = true;
    }
    const int n = (int)last_tracked_pts.size();
    std::vector<Point2f> next(last_tracked_pts.size());
    std::vector<uint8_t> st(last_tracked_pts.size(), 1);
    int n_tracked = 0, L = maxLevel;
    // n == 0: the arrays may be NULL
    if (device_track)
        last_status = device_track(n ? &last_tracked_pts[0].x : nullptr, n, n ? &next[0].x : nullptr, n ? st.data() : nullptr, &n_tracked);
    else
        last_status = srl_flow_track_image(ctx, gray, rows, cols, row_stride_bytes, n ? &last_tracked_pts[0].x : nullptr, n, n ? &next[0].x : nullptr,
                                           n ? st.data() : nullptr, &n_tracked);
    if (last_status != SRL_OK) return -1;
    const bool first = !seen_image_;
    seen_image_ = true;
    if (srl_flow_levels(ctx, &L) == SRL_OK) maxLevel = L;      // trackImage assigns the lowered level count back (:758)
    curr_tracked_pts = next;
    if (first) return 0;                                     // :762-773: status is not touched
    status = st;
    return n_tracked;
}

}  // namespace srlivo

struct srl_lk { srlivo::LKOpticalFlowKernel k; };

extern "C" {
int srl_lk_create(srl_ctx *ctx, int win_width, int win_height, int max_level, int criteria_type, int max_count, double epsilon, int flags,
                  double min_eig_threshold, srl_lk **out) {
    if (out) *out = nullptr;
    if (!out) return SRL_ERR_BAD_ARG;
    srlivo::TermCriteria c;
    c.type = criteria_type; c.maxCount = max_count; c.epsilon = epsilon;
    srl_lk *h = new (std::nothrow) srl_lk{{ctx, srlivo::Size{win_width, win_height}, max_level, c, flags, min_eig_threshold}};
    if (!h) return SRL_ERR_BAD_ARG;
    *out = h;
    return SRL_OK;
}
int srl_lk_destroy(srl_lk *h) { delete h; return SRL_OK; }
int srl_lk_get(srl_lk *h, int *max_level, int *max_count, double *epsilon) {
    if (!h) return SRL_ERR_BAD_ARG;
    if (max_level) *max_level = h->k.getMaxLevel();
    if (max_count) *max_count = h->k.getTermCriteria().maxCount;
    if (epsilon) *epsilon = h->k.getTermCriteria().epsilon;
    return SRL_OK;
}
int srl_lk_track_image(srl_lk *h, const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, const float *prev_xy, int n, float *next_xy,
                       uint8_t *status, int *n_tracked) {
    if (n_tracked) *n_tracked = 0;
    if (!h || n < 0 || n > SRL_FLOW_MAX_POINTS || (n > 0 && (!prev_xy || !next_xy || !status))) return SRL_ERR_BAD_ARG;
    std::vector<srlivo::Point2f> last((size_t)n), cur;
    std::vector<uint8_t> st;
    if (n) std::memcpy(&last[0].x, prev_xy, (size_t)n * 2 * sizeof(float));
    const int rc = h->k.trackImage(gray, rows, cols, row_stride_bytes, last, cur, st);
    if (rc < 0) return h->k.last_status;
    if (n) std::memcpy(next_xy, &cur[0].x, (size_t)n * 2 * sizeof(float));
    if (n && st.size() == (size_t)n) std::memcpy(status, st.data(), (size_t)n);
    if (n_tracked) *n_tracked = rc;
    return SRL_OK;
}
}

// opticalFlowTrackerDevice.cpp (host mirror) -- the opt-ins of opticalFlowTracker.h: this library's consensus estimators
// (srl_consensus_fundamental, srl_consensus_pnp) in the place of cv::findFundamentalMat and cv::solvePnPRansac, and the prepared image
// (srl_image_prepare) in the place of the caller's gray image, with their C functions of include/srlivo_host.h.  Apart from
// opticalFlowTracker.cpp and lkpyramid.cpp so that they link against no more of the device library than before.
#include "opticalFlowTracker.h"
#include "../../../include/srlivo_host.h"

#include <cstring>

namespace srlivo {

int opticalFlowTracker::useDeviceConsensus(const double *fx_fy_cx_cy, const srl_consensus_opts *fundamental_opts, const srl_consensus_opts *pnp_opts) {
    if (!ctx) return SRL_ERR_NO_DEVICE;
    if (!fx_fy_cx_cy) return SRL_ERR_BAD_ARG;
    srl_consensus_opts o[2];
    srl_consensus_opts_default(&o[0], SRL_CONSENSUS_FUNDAMENTAL);
    srl_consensus_opts_default(&o[1], SRL_CONSENSUS_PNP);
    if (fundamental_opts) o[0] = *fundamental_opts;
    if (pnp_opts) o[1] = *pnp_opts;
    // The rules for options and intrinsics are srl_consensus_*'s own and live there only: a call on no points applies them and ends before
    // a device is touched (SRL_OK with an empty consensus), so whatever it refuses is refused here, with its status, and nothing installed.
    {
        int none = 0;
        int rc = srl_consensus_fundamental(ctx, nullptr, nullptr, 0, &o[0], nullptr, nullptr);
        if (rc == SRL_OK) rc = srl_consensus_pnp(ctx, nullptr, nullptr, 0, fx_fy_cx_cy, &o[1], nullptr, &none, nullptr);
        if (rc != SRL_OK) return rc;
    }
    for (int k = 0; k < 4; k++) intrinsic[k] = fx_fy_cx_cy[k];
    consensus_opts[0] = o[0]; consensus_opts[1] = o[1];
    fundamental = [this](const float *last_xy, const float *cur_xy, int n, uint8_t *st) {
        return srl_consensus_fundamental(ctx, last_xy, cur_xy, n, &consensus_opts[0], st, &last_consensus[0]);
    };
    pnp = [this](const float *xyz, const float *uv, int n, int32_t *inliers, int *n_inliers) {
        return srl_consensus_pnp(ctx, xyz, uv, n, intrinsic, &consensus_opts[1], inliers, n_inliers, &last_consensus[1]);
    };
    pnp_is_device = true;
    return SRL_OK;
}

int opticalFlowTracker::usePreparedImage(bool on) {
    if (!ctx) return SRL_ERR_NO_DEVICE;
    use_prepared_image = on;
    if (on) {
        srl_ctx *c = ctx;
        lk_optical_flow_kernel->device_track = [c](const float *prev_xy, int n, float *next_xy, uint8_t *st, int *n_tracked) {
            return srl_flow_track_prepared(c, prev_xy, n, next_xy, st, n_tracked);
        };
    } else {
        lk_optical_flow_kernel->device_track = nullptr;
    }
    return SRL_OK;
}

}  // namespace srlivo

extern "C" {
int srl_oft_use_device_consensus(srl_oft *h, const double *fx_fy_cx_cy, const srl_consensus_opts *fundamental, const srl_consensus_opts *pnp) {
    if (!h) return SRL_ERR_BAD_ARG;
    return h->t.useDeviceConsensus(fx_fy_cx_cy, fundamental, pnp);
}
int srl_oft_use_prepared_image(srl_oft *h, int on) {
    if (!h) return SRL_ERR_BAD_ARG;
    return h->t.usePreparedImage(on != 0);
}
int srl_oft_last_consensus(srl_oft *h, int which, srl_consensus_result *out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (!h || !out || (which != 0 && which != 1)) return SRL_ERR_BAD_ARG;
    *out = h->t.last_consensus[which];
    return SRL_OK;
}
}

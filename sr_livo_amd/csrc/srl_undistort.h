// srl_undistort.h -- internal: what srl_frame_undistort (srl_frame_kernels.hip) and srl_frame_undistort_cut (srl_points.hip) share, so that
// the sweep cut from the device point queue goes through the SAME kernel, argument set-up and interval walk as a sweep the host hands over.
#pragma once
#include "srl_ctx.h"

// the undistorted sweep's blocks (d_corr_in, d_corr_rel, d_corr_imu, d_corr_raw, d_corr_seg) hold n points; grow-only
int srl_corr_reserve(srl_ctx *ctx, int n);
// k_undistort over d_corr_in / d_corr_rel / d_corr_seg / d_corr_imu -> d_corr_imu, d_corr_raw, enqueued on the context's stream.
// d_states: the n_states records on the device; imu_states: the same on the host (the constant-velocity end poses and the inverse of the
// last one are prepared there)
int srl_undistort_launch(srl_ctx *ctx, int n, const double *d_states, const srl_imu_state *imu_states, int n_states, double time_frame_begin,
                         int motion_compensation, const double R_il[9], const double t_il[3]);

// The interval walk of distortFrameByImu (utility.cpp:247-305), sequential in the point order: a point that fits the current interval
// advances the point cursor, one that does not advances the interval -- and a point no later interval fits stops everything behind it.
// seg[i] = interval of point i, -1 = never reached.
inline void srl_imu_interval_walk(const double *relative_time_ms, int n, const srl_imu_state *imu_states, int n_states, double time_frame_begin, int *seg) {
    for (int i = 0; i < n; i++) seg[i] = -1;
    int iter = 0;
    for (int k = 0; k + 1 < n_states; k++) {
        const double tb = imu_states[k].timestamp, te = imu_states[k + 1].timestamp;
        while (iter != n) {
            const double time_point = time_frame_begin + relative_time_ms[iter] / 1000.0;
            if (time_point > tb - 1e-6 && time_point < te + 1e-6) seg[iter++] = k;
            else break;
        }
    }
}

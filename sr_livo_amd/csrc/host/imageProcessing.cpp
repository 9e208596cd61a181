// imageProcessing.cpp (host mirror) -- see imageProcessing.h.  Line numbers are those of src/imageProcessing.cpp.
#include "imageProcessing.h"
#include "utility.h"

#include <algorithm>
#include <cmath>

namespace srlivo {

namespace {
const int minimum_iteration_points = 10;                 // :218

// (HtH + prior^-1)^-1 applied to Htr and to HtH: K residual_vec and K H_mat of :361 / :528 without the explicit K
template <int N>
bool solve_from_sums(const srl::Mat<N, N> &HtH, const srl::Mat<N, 1> &Htr, const srl::Mat<N, N> &prior, srl::Mat<N, 1> &Kr, srl::Mat<N, N> &KH) {
    srl::Mat<N, N> prior_inv, A_inv;
    if (!srl::inverse<N>(prior, prior_inv)) return false;
    if (!srl::inverse<N>(HtH + prior_inv, A_inv)) return false;
    Kr = A_inv * Htr;
    KH = A_inv * HtH;
    return true;
}
void follow_pose(cameraState &st) {                      // :396-399; refreshPoseForProjection (:399) is part of every measurement pass
    st.q_world_camera = srl::Quat::fromRotationMatrix(st.rotation.toRotationMatrix() * st.R_imu_camera);
    st.t_world_camera = st.rotation.toRotationMatrix() * st.t_imu_camera + st.translation;
}
}  // namespace

void imageProcessing::setInitialCov() {                  // :65-72
    covariance = srl::Mat<11, 11>::Identity() * SRL_VIO_INIT_COV;
    covariance(0, 0) = 0.00001;
    covariance.setBlock<6, 6>(1, 1, srl::Mat<6, 6>::Identity() * 1e-3);
    covariance.setBlock<4, 4>(7, 7, srl::Mat<4, 4>::Identity() * 1e-3);
}

int imageProcessing::measure(const cameraState &st, int mode, const srl_color_vio_point *tracked, int n, srl_color_vio_sums *sums) {
    srl_color_vio_args a = {};
    a.cam.q_world_camera[0] = st.q_world_camera.w; a.cam.q_world_camera[1] = st.q_world_camera.x;
    a.cam.q_world_camera[2] = st.q_world_camera.y; a.cam.q_world_camera[3] = st.q_world_camera.z;
    for (int k = 0; k < 3; k++) a.cam.t_world_camera[k] = st.t_world_camera[k];
    a.cam.fx = st.fx; a.cam.fy = st.fy; a.cam.cx = st.cx; a.cam.cy = st.cy;
    a.time_td = st.time_td;
    for (int k = 0; k < 9; k++) a.R_imu_camera[k] = st.R_imu_camera.a[k];
    a.mode = mode;
    a.estimate_extrinsic = ifEstimateExtrinsic ? 1 : 0;
    a.estimate_intrinsic = ifEstimateCameraIntrinsic ? 1 : 0;
    status = rows ? rows(&a, tracked, n, sums) : SRL_ERR_NO_DEVICE;
    return status;
}

bool imageProcessing::vioEsikf(cameraState &st, const srl_color_vio_point *tracked, int n, int number_of_new_visited_voxel) {
    iterations.clear();
    status = SRL_OK;
    if (!ifEstimateCameraIntrinsic) {                    // :224-230
        st.fx = camera_intrinsic(0, 0); st.fy = camera_intrinsic(1, 1);
        st.cx = camera_intrinsic(0, 2); st.cy = camera_intrinsic(1, 2);
    }
    if (!ifEstimateExtrinsic) { st.R_imu_camera = R_imu_camera; st.t_imu_camera = t_imu_camera; }      // :232-236
    typedef srl::Mat<11, 11> M11;
    typedef srl::Mat<11, 1> V11;
    V11 solution = V11::Zero(), d_x = V11::Zero();
    M11 KH = M11::Zero();
    const int total_point_size = n;                      // :247
    if (total_point_size < minimum_iteration_points) return false;

    const double t_predict = st.time_td;                 // :259-265
    const srl::Vec3 p_predict = st.t_imu_camera;
    const srl::Quat q_predict = srl::Quat::fromRotationMatrix(st.R_imu_camera);
    const double fx_predict = st.fx, fy_predict = st.fy, cx_predict = st.cx, cy_predict = st.cy;
    int num_used_point_count = 0;
    double acc_residual = 0, last_acc_residual = 3e8;
    cam_measurement_weight = std::max(0.001, std::min(5.0 / number_of_new_visited_voxel, 0.01));      // :272

    for (int iter_count = 0; iter_count < num_iterations; iter_count++) {
        solution = V11::Zero(); KH = M11::Zero(); d_x = V11::Zero();      // :282-287: H_mat, solution, K set to zero
        const double d_t = st.time_td - t_predict;       // :289-296
        const srl::Vec3 d_p = st.t_imu_camera - p_predict;
        const srl::Quat d_q = q_predict.inverse() * srl::Quat::fromRotationMatrix(st.R_imu_camera);
        const srl::Vec3 d_so3 = numType::quatToSo3(d_q);
        d_x(0) = d_t;
        for (int k = 0; k < 3; k++) { d_x(1 + k) = d_so3[k]; d_x(4 + k) = d_p[k]; }
        d_x(7) = st.fx - fx_predict; d_x(8) = st.fy - fy_predict; d_x(9) = st.cx - cx_predict; d_x(10) = st.cy - cy_predict;

        srl_color_vio_sums sums;                         // :308-349
        if (measure(st, SRL_VIO_REPROJECTION, tracked, n, &sums) != SRL_OK) return false;
        num_used_point_count = (int)sums.used;
        last_used = num_used_point_count;
        acc_residual = sums.acc_residual;
        acc_residual /= total_point_size;                // :351
        if (num_used_point_count < minimum_iteration_points) break;      // :353-356

        M11 J_zero = M11::Identity();                    // :358-359
        J_zero.setBlock<3, 3>(1, 1, srl::Mat3::Identity() - 0.5 * numType::skewSymmetric(srl::vec3(d_x(1), d_x(2), d_x(3))));
        M11 HtH;
        V11 Htr, Kr;
        for (int k = 0; k < 121; k++) HtH.a[k] = sums.HtH[k];
        for (int k = 0; k < 11; k++) Htr.a[k] = sums.Htr[k];
        if (!solve_from_sums<11>(HtH, Htr, J_zero * covariance * J_zero.transpose() * cam_measurement_weight, Kr, KH)) { status = SRL_ERR_BAD_ARG; return false; }
        solution = -Kr - (M11::Identity() - KH) * J_zero * d_x;      // :362
        updateCameraParameters(st, solution);            // :364
        iterations.push_back(st);
        if (std::fabs(acc_residual - last_acc_residual) < 0.01) break;      // :366-369
        last_acc_residual = acc_residual;
    }
    M11 J_k = M11::Identity();                           // :374-377
    J_k.setBlock<3, 3>(1, 1, srl::Mat3::Identity() - 0.5 * numType::skewSymmetric(srl::vec3(solution(1), solution(2), solution(3))));
    covariance = J_k * (M11::Identity() - KH) * covariance * J_k.transpose();
    return true;
}

void imageProcessing::updateCameraParameters(cameraState &st, const srl::Mat<11, 1> &d_x) {      // :382-400
    st.time_td += d_x(0);
    srl::Quat q_imu_camera = srl::Quat::fromRotationMatrix(st.R_imu_camera);
    q_imu_camera = (q_imu_camera * numType::so3ToQuat(srl::vec3(d_x(1), d_x(2), d_x(3)))).normalized();
    st.R_imu_camera = q_imu_camera.toRotationMatrix();
    st.t_imu_camera = st.t_imu_camera + srl::vec3(d_x(4), d_x(5), d_x(6));
    st.fx += d_x(7); st.fy += d_x(8); st.cx += d_x(9); st.cy += d_x(10);
    follow_pose(st);
}

bool imageProcessing::vioPhotometric(cameraState &st, const srl_color_vio_point *tracked, int n, int number_of_new_visited_voxel) {
    iterations.clear();
    status = SRL_OK;
    typedef srl::Mat<6, 6> M6;
    typedef srl::Mat<6, 1> V6;
    V6 solution = V6::Zero(), d_x = V6::Zero();
    M6 KH = M6::Zero();
    const int total_point_size = n;                      // :413
    if (total_point_size < minimum_iteration_points) return false;
    const srl::Vec3 p_predict = st.t_imu_camera;         // :427-428
    const srl::Quat q_predict = srl::Quat::fromRotationMatrix(st.R_imu_camera);
    int num_used_point_count = 0;
    double acc_residual = 0, last_acc_residual = 3e8;
    cam_measurement_weight = std::max(0.001, std::min(5.0 / number_of_new_visited_voxel, 0.01));      // :435

    for (int iter_count = 0; iter_count < num_iterations; iter_count++) {
        solution = V6::Zero(); KH = M6::Zero(); d_x = V6::Zero();         // :445-452
        const srl::Vec3 d_p = st.t_imu_camera - p_predict;                 // :454-459
        const srl::Quat d_q = q_predict.inverse() * srl::Quat::fromRotationMatrix(st.R_imu_camera);
        const srl::Vec3 d_so3 = numType::quatToSo3(d_q);
        for (int k = 0; k < 3; k++) { d_x(k) = d_so3[k]; d_x(3 + k) = d_p[k]; }

        srl_color_vio_sums sums;                         // :463-518
        if (measure(st, SRL_VIO_PHOTOMETRIC, tracked, n, &sums) != SRL_OK) return false;
        num_used_point_count = (int)sums.used;
        last_used = num_used_point_count;
        acc_residual = sums.acc_residual;
        if (num_used_point_count < minimum_iteration_points) break;      // :520-523

        M6 J_zero = M6::Identity();                      // :525-526
        J_zero.setBlock<3, 3>(0, 0, srl::Mat3::Identity() - 0.5 * numType::skewSymmetric(srl::vec3(d_x(0), d_x(1), d_x(2))));
        M6 HtH;
        V6 Htr, Kr;
        for (int i = 0; i < 6; i++) { Htr(i) = sums.Htr[i]; for (int j = 0; j < 6; j++) HtH(i, j) = sums.HtH[i * 11 + j]; }
        const M6 cov6 = covariance.block<6, 6>(1, 1);
        if (!solve_from_sums<6>(HtH, Htr, J_zero * cov6 * J_zero.transpose() * cam_measurement_weight, Kr, KH)) { status = SRL_ERR_BAD_ARG; return false; }
        solution = -Kr - (M6::Identity() - KH) * J_zero * d_x;      // :529
        updateCameraParameters(st, solution);            // :531
        iterations.push_back(st);
        if ((acc_residual / total_point_size) < 10) break;                 // :533-536
        if (std::fabs(acc_residual - last_acc_residual) < 0.01) break;     // :538-541
        last_acc_residual = acc_residual;
    }
    M6 J_k = M6::Identity();                             // :546-549
    J_k.setBlock<3, 3>(0, 0, srl::Mat3::Identity() - 0.5 * numType::skewSymmetric(srl::vec3(solution(0), solution(1), solution(2))));
    const M6 cov6 = covariance.block<6, 6>(1, 1);
    covariance.setBlock<6, 6>(1, 1, J_k * (M6::Identity() - KH) * cov6 * J_k.transpose());
    return true;
}

namespace {
srl_color_camera camera_of(const cameraState &st, double fov_margin) {
    srl_color_camera c;
    c.q_world_camera[0] = st.q_world_camera.w; c.q_world_camera[1] = st.q_world_camera.x;
    c.q_world_camera[2] = st.q_world_camera.y; c.q_world_camera[3] = st.q_world_camera.z;
    for (int k = 0; k < 3; k++) c.t_world_camera[k] = st.t_world_camera[k];
    c.fx = st.fx; c.fy = st.fy; c.cx = st.cx; c.cy = st.cy;
    c.fov_margin = fov_margin;
    return c;
}
const double frame_fov_margin = 0.005;                   // state.cpp:25: the margin of every p_frame->p_state
}  // namespace

int imageProcessing::process(cameraState &st, const imageFrame &frame, int number_of_new_visited_voxel, srl_image_process_result *result) {      // :89-164
    srl_image_process_result r = {};
    auto leave = [&](int rc) { status = rc; if (result) *result = r; return rc; };
    if (!op_tracker || !steps.prepCreate || !steps.prepare || !steps.consensusSetup || !steps.select || !steps.render) return leave(SRL_ERR_NO_DEVICE);
    if (frame.jpeg && !steps.prepareJpeg) return leave(SRL_ERR_NO_DEVICE);
    if ((!frame.rgb_image && !frame.jpeg) || frame.image_rows < 1 || frame.image_cols < 1) return leave(SRL_ERR_BAD_ARG);
    r.first_data = first_data ? 1 : 0;

    // :91-111.  The reference has no failing step; here one may fail, and the frame is then offered again.  So nothing of the first
    // data is done twice: the scale, the size and the scaled intrinsics are committed once, with the preparer (first_data_stage 1), the
    // consensus setup once behind them (2), and first_data itself falls behind init as in the reference
    if (first_data && first_data_stage < 1) {
        if (image_width < 1 || image_height < 1 || !(image_resize_ratio > 0.0)) return leave(SRL_ERR_BAD_ARG);
        const double scale = image_width * image_resize_ratio / frame.image_cols;
        const double fx = camera_intrinsic(0, 0) / scale, cx = camera_intrinsic(0, 2) / scale;
        const double fy = camera_intrinsic(1, 1) / scale, cy = camera_intrinsic(1, 2) / scale;
        srl_image_prep_opts po;
        srl_image_prep_opts_default(&po);
        po.cols = (int)(image_width / scale);            // cv::Size(int, int) of two doubles
        po.rows = (int)(image_height / scale);
        po.fx = fx; po.fy = fy; po.cx = cx; po.cy = cy;
        for (int k = 0; k < 5; k++) po.dist[k] = camera_dist_coeffs[k];
        { const int rc = steps.prepCreate(po); if (rc != SRL_OK) return leave(rc); }                  // :103
        image_scale_factor = scale;                      // :93-98
        camera_intrinsic(0, 0) = fx; camera_intrinsic(0, 2) = cx; camera_intrinsic(1, 1) = fy; camera_intrinsic(1, 2) = cy;
        prepared_rows = po.rows; prepared_cols = po.cols;
        first_data_stage = 1;
    }
    if (first_data && first_data_stage < 2) {
        const double k4[4] = {camera_intrinsic(0, 0), camera_intrinsic(1, 1), camera_intrinsic(0, 2), camera_intrinsic(1, 2)};
        { const int rc = steps.consensusSetup(k4); if (rc != SRL_OK) return leave(rc); }              // :106
        op_tracker->maximum_tracked_points = maximum_tracked_points;                                  // :107
        minimum_depth_for_projection = tracker_minimum_depth;                                         // :109-110
        maximum_depth_for_projection = tracker_maximum_depth;
        first_data_stage = 2;
    }
    r.prepared_rows = prepared_rows; r.prepared_cols = prepared_cols; r.image_scale_factor = image_scale_factor;

    {                                                    // :113-125: the resize iff the ratio says so, then remap, gray + CLAHE, YCrCb
        const bool resized = std::fabs(image_resize_ratio - 1.0) > 1e-6;
        // (a compressed frame is decoded on the way, and resized whenever its size is not the preparer's)
        const int rc = frame.jpeg ? steps.prepareJpeg(frame.jpeg, frame.jpeg_bytes)
                                  : steps.prepare(frame.rgb_image, frame.image_rows, frame.image_cols, frame.row_stride_bytes, resized);
        if (rc != SRL_OK) return leave(rc);
    }

    const srl_color_camera cam_in = camera_of(st, frame_fov_margin);
    if (first_data) {                                    // :127-135
        const srl_color_select_opts so = {track_windows_size / image_scale_factor, 1, 0, minimum_depth_for_projection, maximum_depth_for_projection};
        std::vector<srl_color_selected> rgb_points_vec_temp;
        { const int rc = steps.select(cam_in, frame.image_rows, frame.image_cols, so, false, rgb_points_vec_temp); if (rc != SRL_OK) return leave(rc); }
        if (!op_tracker->init(rgb_points_vec_temp.data(), (int)rgb_points_vec_temp.size(), nullptr, prepared_rows, prepared_cols, prepared_cols,
                              frame.time_sweep_end))
            return leave(op_tracker->status);
        first_data = false;
    }

    // :137 (distance = -20 switches rejectErrorTrackingPoints off: not built)
    if (!op_tracker->trackImage(nullptr, prepared_rows, prepared_cols, prepared_cols, frame.time_sweep_end, frame.image_rows, frame.image_cols))
        return leave(op_tracker->status);
    r.tracked_after_flow = (int)op_tracker->map_rgb_points_in_cur_image_pose.size();

    bool enough_points = true;                           // :139-145
    {
        bool accepted = false;
        if (!op_tracker->removeOutlierUsingRansacPnp(1, &accepted)) return leave(op_tracker->status);
        if (!accepted) enough_points = false;
    }
    r.tracked_after_pnp = (int)op_tracker->map_rgb_points_in_cur_image_pose.size();
    r.pnp_accepted = enough_points ? 1 : 0;

    if (enough_points) {                                 // :149-150
        const std::vector<srl_color_vio_point> tracked = op_tracker->trackedForVio();
        const bool res_esikf = vioEsikf(st, tracked.data(), (int)tracked.size(), number_of_new_visited_voxel);
        if (status != SRL_OK) return leave(status);
        r.esikf_accepted = res_esikf ? 1 : 0; r.esikf_iterations = (int)iterations.size(); r.esikf_used = last_used;
    }
    if (enough_points) {                                 // :152-153
        const std::vector<srl_color_vio_point> tracked = op_tracker->trackedForVio();
        const bool res_photometric = vioPhotometric(st, tracked.data(), (int)tracked.size(), number_of_new_visited_voxel);
        if (status != SRL_OK) return leave(status);
        r.photometric_accepted = res_photometric ? 1 : 0; r.photometric_iterations = (int)iterations.size(); r.photometric_used = last_used;
    }

    const srl_color_camera cam_out = camera_of(st, frame_fov_margin);      // the camera as the two updates left it
    { const int rc = steps.render(cam_out, frame.time_sweep_end, r.render); if (rc != SRL_OK) return leave(rc); }      // :155

    projection_camera = camera_of(st, -0.4);             // :157 updatePoseForProjection(p_frame, -0.4)
    projection_rows = frame.image_rows; projection_cols = frame.image_cols; projection_frame_id = frame.frame_id;

    if (!(projection_cols == 0 || projection_rows == 0) && projection_frame_id != updated_frame_index) {      // :159, rgbMapTracker.cpp:26-43
        const srl_color_select_opts so = {10.0, 1, 0, minimum_depth_for_projection, maximum_depth_for_projection};
        std::vector<srl_color_selected> temp;
        { const int rc = steps.select(projection_camera, projection_rows, projection_cols, so, true, temp); if (rc != SRL_OK) return leave(rc); }
        points_for_projection.swap(temp);
        updated_frame_index = projection_frame_id;
    }
    r.refreshed_candidates = (int)points_for_projection.size();

    // :161 (the reference's last argument, 1000000, is a parameter its function never reads)
    const bool topped = op_tracker->updateAndAppendTrackPoints(&cam_out, frame.image_rows, frame.image_cols, points_for_projection.data(),
                                                               (int)points_for_projection.size(), track_windows_size / image_scale_factor);
    r.track = op_tracker->update_totals;
    if (!topped) return leave(op_tracker->status);

    time_last_process = frame.time_sweep_end;            // :163
    return leave(SRL_OK);
}

void imageProcessing::updateCameraParameters(cameraState &st, const srl::Mat<6, 1> &d_x) {      // :554-566
    srl::Quat q_imu_camera = srl::Quat::fromRotationMatrix(st.R_imu_camera);
    q_imu_camera = (q_imu_camera * numType::so3ToQuat(srl::vec3(d_x(0), d_x(1), d_x(2)))).normalized();
    st.R_imu_camera = q_imu_camera.toRotationMatrix();
    st.t_imu_camera = st.t_imu_camera + srl::vec3(d_x(3), d_x(4), d_x(5));
    follow_pose(st);
}

}  // namespace srlivo

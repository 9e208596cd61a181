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

void imageProcessing::updateCameraParameters(cameraState &st, const srl::Mat<6, 1> &d_x) {      // :554-566
    srl::Quat q_imu_camera = srl::Quat::fromRotationMatrix(st.R_imu_camera);
    q_imu_camera = (q_imu_camera * numType::so3ToQuat(srl::vec3(d_x(0), d_x(1), d_x(2)))).normalized();
    st.R_imu_camera = q_imu_camera.toRotationMatrix();
    st.t_imu_camera = st.t_imu_camera + srl::vec3(d_x(3), d_x(4), d_x(5));
    follow_pose(st);
}

}  // namespace srlivo

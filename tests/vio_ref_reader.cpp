// tests/vio_ref_reader.cpp -- test-side driver of the pieces of imageProcessing::vioEsikf (src/imageProcessing.cpp:220-380) and
// vioPhotometric (:402-552) that can be compiled against the stand-ins of oracle/.  imageProcessing.cpp itself cannot be compiled here:
// the include mirror of oracle/Makefile's `refpath` target shadows imageProcessing.h and there is no OpenCV (optical flow, PnP).  So the
// reader CALLS the reference's own pieces and writes out the loop statements between those calls:
//   cloudFrame::getRgb(u, v, 0, &dx, &dy) with its getSubPixel<cv::Vec3b> (src/lioOptimization.cpp:71-140), cloudFrame::
//   refreshPoseForProjection (:201-205), numType::skewSymmetric, quatToSo3 and so3ToQuat (include/utility.h), rgbPoint::getPosition, getRgb
//   and getCovRgb (src/cloudMap.cpp) on points whose private colour fields are set from the test's map (updateRgb, which makes them, is
//   pinned by tests/render_ref_reader.cpp), and the stand-in Eigen of oracle/ref_shim for every matrix statement, the literal solve with
//   the explicit gain K (:358-377, :525-549) included.
// getRgb needs pixels and the stand-in cv::Mat of oracle/ref_shim has none, so tests/test_vio_checker_reference.py compiles the
// reference's src/lioOptimization.cpp once more into this reader's library with tests/stub_opencv in front of oracle/ref_shim on the include
// path (a cv::Mat that views the caller's bytes, OpenCV's saturating byte arithmetic), links with -Bsymbolic so that this copy's
// cloudFrame is the one the reader uses, and takes everything else from oracle/_ref/libref_path.so as tests/select_ref_reader.cpp does.
// The stand-in Eigen has no RowMajor fixed matrices: J_u_pc, J_u_K and J_color_u are plain (column-major) matrices filled by the same
// comma initialisers and block assignments; storage order changes no coefficient and no sum.  The comparison therefore pins the contract
// to the STAND-IN's evaluation order (coefficient-wise products, terms added left to right).  With real Eigen the one block whose order
// is not forced is J_color_pc * R_imu_camera^T, which has three-term sums (every other product has at most two non-zero terms per
// entry); its order cannot be verified on a machine without Eigen.
// The three departures of the contract (include/srlivo_hip.h) are written here as guards in front of the reference's statements: the
// list's order, `unknown` / `behind` / `outside` points left out.  It holds no code of the reference.
//
// The standard headers come first: `#define private public` in front of <sstream> does not compile.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>
#include <Eigen/Core>
#include <Eigen/Dense>

#define private public
#define protected public
#include "lioOptimization.h"
#undef private
#undef protected

namespace {

double huber_loss(double residual, double outlier_threshold = 1.0) {      // getHuberLoss (:202-216) is a free function of the file that cannot be compiled
    double scale = 1.0;
    if (residual / outlier_threshold < 1.0) scale = 1.0;
    else scale = (2 * sqrt(residual) / sqrt(outlier_threshold) - 1.0) / residual;
    return scale;
}

struct Tracked {                        // one entry of the caller's list
    int known;                          // 0: a pool position the map does not hold
    rgbPoint *point;
    Eigen::Vector2d match, velocity;
};

// state31: time_td, R_imu_camera (9, row-major), t_imu_camera (3), fx fy cx cy, q_world_camera (w x y z), t_world_camera (3), rotation (w x y z), translation (3)
void state_from(const double *s, state &st) {
    st.time_td = s[0];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) st.R_imu_camera(r, c) = s[1 + r * 3 + c];
    st.t_imu_camera = Eigen::Vector3d(s[10], s[11], s[12]);
    st.fx = s[13]; st.fy = s[14]; st.cx = s[15]; st.cy = s[16];
    st.q_world_camera = Eigen::Quaterniond(s[17], s[18], s[19], s[20]);
    st.t_world_camera = Eigen::Vector3d(s[21], s[22], s[23]);
    st.rotation = Eigen::Quaterniond(s[24], s[25], s[26], s[27]);
    st.translation = Eigen::Vector3d(s[28], s[29], s[30]);
}
void state_to(const state &st, double *s) {
    s[0] = st.time_td;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) s[1 + r * 3 + c] = st.R_imu_camera(r, c);
    for (int i = 0; i < 3; ++i) { s[10 + i] = st.t_imu_camera(i); s[21 + i] = st.t_world_camera(i); s[28 + i] = st.translation(i); }
    s[13] = st.fx; s[14] = st.fy; s[15] = st.cx; s[16] = st.cy;
    s[17] = st.q_world_camera.w(); s[18] = st.q_world_camera.x(); s[19] = st.q_world_camera.y(); s[20] = st.q_world_camera.z();
    s[24] = st.rotation.w(); s[25] = st.rotation.x(); s[26] = st.rotation.y(); s[27] = st.rotation.z();
}

struct Scene {
    state st;
    std::vector<point3D> none;
    cloudFrame *frame = nullptr;
    std::vector<rgbPoint *> points;
    std::vector<Tracked> tracked;
    ~Scene() {
        if (frame) { frame->p_state = nullptr; frame->rgb_image.release(); delete frame; }
        for (rgbPoint *p : points) delete p;
    }
};

// list: n x (known, x, y, z as FP32 bits are passed separately), see vrr_* below
void build_scene(Scene &S, const double *state31, const uint8_t *img, int rows, int cols, int n, const int32_t *known, const float *xyz, const int16_t *rgb,
                 const float *cov, const int16_t *n_rgb, const double *match_vel) {
    state_from(state31, S.st);
    S.frame = new cloudFrame(S.none, &S.st);
    S.frame->image_rows = rows; S.frame->image_cols = cols;
    S.frame->rgb_image.rows = rows; S.frame->rgb_image.cols = cols; S.frame->rgb_image.data = const_cast<uint8_t *>(img);
    S.frame->refreshPoseForProjection();
    for (int k = 0; k < n; ++k) {
        const Eigen::Vector3f pos(xyz[(size_t)k * 3], xyz[(size_t)k * 3 + 1], xyz[(size_t)k * 3 + 2]);
        rgbPoint *p = new rgbPoint(pos.cast<double>());      // stores the FP32 position back: the cast is exact
        for (int i = 0; i < 3; ++i) { p->rgb[i] = rgb[(size_t)k * 3 + i]; p->cov_rgb(i) = cov[(size_t)k * 3 + i]; }
        p->N_rgb = n_rgb[k];
        p->image_velocity = Eigen::Vector2d(match_vel[(size_t)k * 4 + 2], match_vel[(size_t)k * 4 + 3]);
        S.points.push_back(p);
        Tracked t;
        t.known = known[k]; t.point = p;
        t.match = Eigen::Vector2d(match_vel[(size_t)k * 4], match_vel[(size_t)k * 4 + 1]);
        t.velocity = p->image_velocity;
        S.tracked.push_back(t);
    }
}

// the loop of :308-349 over the list; H_mat (2 total x 11), residual_vec.  outcome / where per list entry (where: the point_idx it took, or -1)
void esikf_loop(Scene &S, bool ifEstimateExtrinsic, bool ifEstimateCameraIntrinsic, Eigen::MatrixXd &H_mat, Eigen::VectorXd &residual_vec, double &acc_residual,
                int &num_used_point_count, uint8_t *outcome, int *where) {
    cloudFrame *p_frame = S.frame;
    Eigen::Vector3d point_world, point_camera;
    Eigen::Vector2d pixel_match, pixel_projection, pixel_velocity;
    int point_idx = -1;
    for (size_t it = 0; it < S.tracked.size(); ++it) {
        if (where) where[it] = -1;
        if (!S.tracked[it].known) { if (outcome) outcome[it] = 4; continue; }
        point_world = S.tracked[it].point->getPosition();
        pixel_velocity = S.tracked[it].point->image_velocity;
        pixel_match = S.tracked[it].match;
        point_camera = p_frame->p_state->q_camera_world.toRotationMatrix() * point_world + p_frame->p_state->t_camera_world;
        if (point_camera(2) < 0.001) { if (outcome) outcome[it] = 2; continue; }
        pixel_projection = Eigen::Vector2d(p_frame->p_state->fx * point_camera(0) / point_camera(2) + p_frame->p_state->cx,
                                           p_frame->p_state->fy * point_camera(1) / point_camera(2) + p_frame->p_state->cy) + p_frame->p_state->time_td * pixel_velocity;
        double residual = (pixel_projection - pixel_match).norm();
        double huber = huber_loss(residual);
        point_idx++;
        acc_residual += residual;
        residual_vec.block<2, 1>(point_idx * 2, 0) = (pixel_projection - pixel_match) * huber;
        num_used_point_count++;
        Eigen::Matrix<double, 2, 3> J_u_pc;
        J_u_pc << p_frame->p_state->fx / point_camera.z(), 0, -(p_frame->p_state->fx * point_camera.x()) / (point_camera.z() * point_camera.z()),
            0, p_frame->p_state->fy / point_camera.z(), -(p_frame->p_state->fy * point_camera.y()) / (point_camera.z() * point_camera.z());
        Eigen::Matrix<double, 2, 4> J_u_K;
        J_u_K << point_camera.x() / point_camera.z(), 0, 1, 0, 0, point_camera.y() / point_camera.z(), 0, 1;
        H_mat.block<2, 1>(point_idx * 2, 0) = pixel_velocity * huber;
        if (ifEstimateExtrinsic) {
            H_mat.block<2, 3>(point_idx * 2, 1) = J_u_pc * numType::skewSymmetric(point_camera) * huber;
            H_mat.block<2, 3>(point_idx * 2, 4) = -J_u_pc * p_frame->p_state->R_imu_camera.transpose() * huber;
        }
        if (ifEstimateCameraIntrinsic) H_mat.block<2, 4>(point_idx * 2, 7) = J_u_K * huber;
        if (outcome) outcome[it] = 0;
        if (where) where[it] = point_idx;
    }
}

// the loop of :463-518
void photometric_loop(Scene &S, bool ifEstimateExtrinsic, Eigen::MatrixXd &H_mat, Eigen::VectorXd &residual_vec, Eigen::MatrixXd &R_mat_inv, double &acc_residual,
                      int &num_used_point_count, uint8_t *outcome, int *where) {
    cloudFrame *p_frame = S.frame;
    Eigen::Vector3d point_world, point_camera;
    Eigen::Vector2d pixel_projection, pixel_velocity;
    int point_idx = -1;
    for (size_t it = 0; it < S.tracked.size(); ++it) {
        if (where) where[it] = -1;
        if (!S.tracked[it].known) { if (outcome) outcome[it] = 4; continue; }
        if (S.tracked[it].point->N_rgb < 3) { if (outcome) outcome[it] = 1; continue; }
        point_world = S.tracked[it].point->getPosition();
        pixel_velocity = S.tracked[it].point->image_velocity;
        point_camera = p_frame->p_state->q_camera_world.toRotationMatrix() * point_world + p_frame->p_state->t_camera_world;
        if (point_camera(2) < 0.001) { if (outcome) outcome[it] = 2; continue; }
        pixel_projection = Eigen::Vector2d(p_frame->p_state->fx * point_camera(0) / point_camera(2) + p_frame->p_state->cx,
                                           p_frame->p_state->fy * point_camera(1) / point_camera(2) + p_frame->p_state->cy) + p_frame->p_state->time_td * pixel_velocity;
        {   // the footprint of getRgb's 17 samples
            const double u = pixel_projection(0), v = pixel_projection(1);
            const bool inside = std::isfinite(u) && std::isfinite(v) && std::floor(u) - 4 >= 0 && std::floor(u) + 5 <= p_frame->image_cols - 1 &&
                                std::floor(v) - 4 >= 0 && std::floor(v) + 5 <= p_frame->image_rows - 1;
            if (!inside) { if (outcome) outcome[it] = 3; continue; }
        }
        point_idx++;
        Eigen::Vector3d point_color = S.tracked[it].point->getRgb();
        Eigen::Matrix3d point_rgb_info = Eigen::Matrix3d::Zero();
        Eigen::Matrix3d point_rgb_cov = S.tracked[it].point->getCovRgb();
        for (int i = 0; i < 3; i++) {
            point_rgb_info(i, i) = 1.0 / point_rgb_cov(i, i);
            R_mat_inv(point_idx * 3 + i, point_idx * 3 + i) = point_rgb_info(i, i);
        }
        Eigen::Vector3d obs_color_dx, obs_color_dy;
        Eigen::Vector3d obs_color = p_frame->getRgb(pixel_projection(0), pixel_projection(1), 0, &obs_color_dx, &obs_color_dy);
        Eigen::Vector3d residual = obs_color - point_color;
        double huber = huber_loss(residual.norm());
        residual *= huber;
        residual_vec.block<3, 1>(point_idx * 3, 0) = (obs_color - point_color) * huber;
        acc_residual += (residual.transpose() * point_rgb_info * residual)(0, 0);      // the stand-in has no 1 x 1 -> scalar conversion
        Eigen::Matrix<double, 3, 2> J_color_u;
        J_color_u.block<3, 1>(0, 0) = obs_color_dx;
        J_color_u.block<3, 1>(0, 1) = obs_color_dy;
        num_used_point_count++;
        Eigen::Matrix<double, 2, 3> J_u_pc;
        J_u_pc << p_frame->p_state->fx / point_camera.z(), 0, -(p_frame->p_state->fx * point_camera.x()) / (point_camera.z() * point_camera.z()),
            0, p_frame->p_state->fy / point_camera.z(), -(p_frame->p_state->fy * point_camera.y()) / (point_camera.z() * point_camera.z());
        Eigen::Matrix3d J_color_pc = J_color_u * J_u_pc;
        if (ifEstimateExtrinsic) {
            H_mat.block<3, 3>(point_idx * 3, 0) = J_color_pc * numType::skewSymmetric(point_camera) * huber;
            H_mat.block<3, 3>(point_idx * 3, 3) = -J_color_pc * p_frame->p_state->R_imu_camera.transpose() * huber;
        }
        if (outcome) outcome[it] = 0;
        if (where) where[it] = point_idx;
    }
}

void update_camera_11(Scene &S, const Eigen::VectorXd &d_x) {      // :382-400
    state *p_state = S.frame->p_state;
    p_state->time_td += d_x(0);
    Eigen::Quaterniond q_imu_camera = Eigen::Quaterniond(p_state->R_imu_camera);
    q_imu_camera = (q_imu_camera * numType::so3ToQuat(Eigen::Vector3d(d_x(1), d_x(2), d_x(3)))).normalized();
    p_state->R_imu_camera = q_imu_camera.toRotationMatrix();
    p_state->t_imu_camera += Eigen::Vector3d(d_x(4), d_x(5), d_x(6));
    p_state->fx += d_x(7); p_state->fy += d_x(8); p_state->cx += d_x(9); p_state->cy += d_x(10);
    p_state->q_world_camera = Eigen::Quaterniond(p_state->rotation.toRotationMatrix() * p_state->R_imu_camera);
    p_state->t_world_camera = p_state->rotation.toRotationMatrix() * p_state->t_imu_camera + p_state->translation;
    S.frame->refreshPoseForProjection();
}
void update_camera_6(Scene &S, const Eigen::VectorXd &d_x) {       // :554-566
    state *p_state = S.frame->p_state;
    Eigen::Quaterniond q_imu_camera = Eigen::Quaterniond(p_state->R_imu_camera);
    q_imu_camera = (q_imu_camera * numType::so3ToQuat(Eigen::Vector3d(d_x(0), d_x(1), d_x(2)))).normalized();
    p_state->R_imu_camera = q_imu_camera.toRotationMatrix();
    p_state->t_imu_camera += Eigen::Vector3d(d_x(3), d_x(4), d_x(5));
    p_state->q_world_camera = Eigen::Quaterniond(p_state->rotation.toRotationMatrix() * p_state->R_imu_camera);
    p_state->t_world_camera = p_state->rotation.toRotationMatrix() * p_state->t_imu_camera + p_state->translation;
    S.frame->refreshPoseForProjection();
}

const int minimum_iteration_points = 10;

}  // namespace

extern "C" {

// One iteration's loop.  mode 0: reprojection, rows_out n x 24 as 2 x (11 H, r); mode 1: photometric, 3 x (6 H, r, info).
void vrr_rows(const double *state31, const uint8_t *img, int rows, int cols, int mode, int est_ext, int est_int, int n, const int32_t *known, const float *xyz,
              const int16_t *rgb, const float *cov, const int16_t *n_rgb, const double *match_vel, double *rows_out, uint8_t *outcome) {
    Scene S;
    build_scene(S, state31, img, rows, cols, n, known, xyz, rgb, cov, n_rgb, match_vel);
    std::vector<int> where(n);
    double acc = 0; int used = 0;
    std::memset(rows_out, 0, (size_t)n * 24 * sizeof(double));
    if (mode == 0) {
        Eigen::MatrixXd H_mat; Eigen::VectorXd residual_vec;
        H_mat.resize(n * 2, 11); residual_vec.resize(n * 2, 1); H_mat.setZero(); residual_vec.setZero();
        esikf_loop(S, est_ext != 0, est_int != 0, H_mat, residual_vec, acc, used, outcome, where.data());
        for (int k = 0; k < n; ++k) if (where[k] >= 0)
            for (int i = 0; i < 2; ++i) { for (int c = 0; c < 11; ++c) rows_out[(size_t)k * 24 + i * 12 + c] = H_mat(where[k] * 2 + i, c); rows_out[(size_t)k * 24 + i * 12 + 11] = residual_vec(where[k] * 2 + i); }
    } else {
        Eigen::MatrixXd H_mat, R_mat_inv; Eigen::VectorXd residual_vec;
        H_mat.resize(n * 3, 6); residual_vec.resize(n * 3, 1); R_mat_inv.resize(n * 3, n * 3); H_mat.setZero(); residual_vec.setZero(); R_mat_inv.setZero();
        photometric_loop(S, est_ext != 0, H_mat, residual_vec, R_mat_inv, acc, used, outcome, where.data());
        for (int k = 0; k < n; ++k) if (where[k] >= 0)
            for (int i = 0; i < 3; ++i) {
                const int r = where[k] * 3 + i;
                for (int c = 0; c < 6; ++c) rows_out[(size_t)k * 24 + i * 8 + c] = H_mat(r, c);
                rows_out[(size_t)k * 24 + i * 8 + 6] = residual_vec(r); rows_out[(size_t)k * 24 + i * 8 + 7] = R_mat_inv(r, r);
            }
    }
}

// vioEsikf (mode 0) or vioPhotometric (mode 1) with the explicit K.  state31 and cov121 (row-major) are read and written; states_out takes
// the state behind each of the first `capacity` updateCameraParameters.  Returns what the reference's function returns.
int vrr_update(double *state31, double *cov121, const uint8_t *img, int rows, int cols, int mode, int est_ext, int est_int, int num_iterations,
               int number_of_new_visited_voxel, int n, const int32_t *known, const float *xyz, const int16_t *rgb, const float *cov, const int16_t *n_rgb,
               const double *match_vel, double *states_out, int capacity, int *iterations, int *used_out) {
    *iterations = 0; *used_out = 0;
    Scene S;
    build_scene(S, state31, img, rows, cols, n, known, xyz, rgb, cov, n_rgb, match_vel);
    state *p_state = S.frame->p_state;
    const int N = mode == 0 ? 11 : 6, per = mode == 0 ? 2 : 3;
    Eigen::MatrixXd covariance(11, 11);
    for (int r = 0; r < 11; ++r) for (int c = 0; c < 11; ++c) covariance(r, c) = cov121[r * 11 + c];
    Eigen::MatrixXd H_mat, R_mat_inv, K;
    Eigen::VectorXd solution(N), residual_vec, d_x(N);
    int total_point_size = n;
    if (total_point_size < minimum_iteration_points) return 0;
    H_mat.resize(total_point_size * per, N); residual_vec.resize(total_point_size * per, 1); K.resize(N, total_point_size * per);
    if (mode == 1) R_mat_inv.resize(total_point_size * 3, total_point_size * 3);
    double t_predict = p_state->time_td;
    Eigen::Vector3d p_predict = p_state->t_imu_camera;
    Eigen::Quaterniond q_predict = Eigen::Quaterniond(p_state->R_imu_camera);
    double fx_predict = p_state->fx, fy_predict = p_state->fy, cx_predict = p_state->cx, cy_predict = p_state->cy;
    int num_used_point_count = 0;
    double acc_residual = 0, last_acc_residual = 3e8;
    const double cam_measurement_weight = std::max(0.001, std::min(5.0 / number_of_new_visited_voxel, 0.01));
    const Eigen::MatrixXd I_N = Eigen::MatrixXd::Identity(N, N);
    const int at = mode == 0 ? 1 : 0;
    for (int iter_count = 0; iter_count < num_iterations; iter_count++) {
        acc_residual = 0;
        H_mat.setZero(); solution.setZero(); residual_vec.setZero(); K.setZero(); d_x.setZero();
        if (mode == 1) R_mat_inv.setZero();
        Eigen::Vector3d d_p = p_state->t_imu_camera - p_predict;
        Eigen::Quaterniond d_q = q_predict.inverse() * Eigen::Quaterniond(p_state->R_imu_camera);
        Eigen::Vector3d d_so3 = numType::quatToSo3(d_q);
        if (mode == 0) {
            d_x(0) = p_state->time_td - t_predict;
            for (int i = 0; i < 3; ++i) { d_x(1 + i) = d_so3(i); d_x(4 + i) = d_p(i); }
            d_x(7) = p_state->fx - fx_predict; d_x(8) = p_state->fy - fy_predict; d_x(9) = p_state->cx - cx_predict; d_x(10) = p_state->cy - cy_predict;
        } else {
            for (int i = 0; i < 3; ++i) { d_x(i) = d_so3(i); d_x(3 + i) = d_p(i); }
        }
        num_used_point_count = 0;
        if (mode == 0) {
            esikf_loop(S, est_ext != 0, est_int != 0, H_mat, residual_vec, acc_residual, num_used_point_count, nullptr, nullptr);
            acc_residual /= total_point_size;
        } else {
            photometric_loop(S, est_ext != 0, H_mat, residual_vec, R_mat_inv, acc_residual, num_used_point_count, nullptr, nullptr);
        }
        *used_out = num_used_point_count;
        if (num_used_point_count < minimum_iteration_points) break;
        Eigen::MatrixXd J_zero = Eigen::MatrixXd::Identity(N, N);
        J_zero.block<3, 3>(at, at) = Eigen::Matrix3d::Identity() - 0.5 * numType::skewSymmetric(Eigen::Vector3d(d_x(at), d_x(at + 1), d_x(at + 2)));
        if (mode == 0) {
            K = (H_mat.transpose() * H_mat + (J_zero * covariance * J_zero.transpose() * cam_measurement_weight).inverse()).inverse() * H_mat.transpose();
        } else {
            Eigen::MatrixXd cov6(6, 6);
            for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) cov6(r, c) = covariance(1 + r, 1 + c);
            K = (H_mat.transpose() * R_mat_inv * H_mat + (J_zero * cov6 * J_zero.transpose() * cam_measurement_weight).inverse()).inverse() * H_mat.transpose() * R_mat_inv;
        }
        solution = -K * residual_vec - (I_N - K * H_mat) * J_zero * d_x;
        if (mode == 0) update_camera_11(S, solution); else update_camera_6(S, solution);
        if (*iterations < capacity) state_to(*p_state, states_out + (size_t)*iterations * 31);
        ++*iterations;
        if (mode == 1 && (acc_residual / total_point_size) < 10) break;
        if (fabs(acc_residual - last_acc_residual) < 0.01) break;
        last_acc_residual = acc_residual;
    }
    Eigen::MatrixXd J_k = Eigen::MatrixXd::Identity(N, N);
    J_k.block<3, 3>(at, at) = Eigen::Matrix3d::Identity() - 0.5 * numType::skewSymmetric(Eigen::Vector3d(solution(at), solution(at + 1), solution(at + 2)));
    if (mode == 0) {
        covariance = J_k * (I_N - K * H_mat) * covariance * J_k.transpose();
    } else {
        Eigen::MatrixXd cov6(6, 6);
        for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) cov6(r, c) = covariance(1 + r, 1 + c);
        cov6 = J_k * (I_N - K * H_mat) * cov6 * J_k.transpose();
        for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) covariance(1 + r, 1 + c) = cov6(r, c);
    }
    for (int r = 0; r < 11; ++r) for (int c = 0; c < 11; ++c) cov121[r * 11 + c] = covariance(r, c);
    state_to(*p_state, state31);
    return 1;
}

}  // extern "C"

// srl_host_capi.cpp -- C handles (include/srlivo_host.h) onto the C++ host mirror, so that ctypes
// harnesses drive the same lioOptimization / eskfEstimator code a C++ consumer links.
#include "../../../include/srlivo_host.h"
#include "imageProcessing.h"
#include "lioOptimization.h"
#include "tr1_order.h"
#include "tr1_relation.h"

#include <cmath>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>

using namespace srlivo;

struct srl_lio {
    lioOptimization *lio = nullptr;
    std::string err;
    state prev_state, cur_state;
    imageProcessing vio;                      // the camera ESIKF and the camera state it works on
    cameraState camera;
    srl_vio_rows_provider vio_provider = nullptr;
    void *vio_user = nullptr;
    // imageProcessing::process: the tracker it works on (made at the first frame) and the step table as given
    srl_oft *oft = nullptr;
    srl_image_process_steps image_steps = {};
    srl_image_jpeg_step jpeg_step = nullptr;  // the prepare step of a compressed frame (not a member of the table: its layout stays)
    void *jpeg_user = nullptr;
    bool image_options_set = false;
};

namespace {

int status_from_exception(srl_lio *h, const std::exception &e) {
    h->err = e.what();
    if (h->err == "error") return SRL_ERR_NAN_PLANARITY;   // optimize.cpp:348-350
    return SRL_ERR_HIP;
}

void state_from(const double s[16], state &st) {
    st.rotation = srl::Quat(s[0], s[1], s[2], s[3]);
    st.translation = srl::vec3(s[4], s[5], s[6]);
    st.velocity = srl::vec3(s[7], s[8], s[9]);
    st.ba = srl::vec3(s[10], s[11], s[12]);
    st.bg = srl::vec3(s[13], s[14], s[15]);
}
void state_to(const state &st, double s[16]) {
    s[0] = st.rotation.w; s[1] = st.rotation.x; s[2] = st.rotation.y; s[3] = st.rotation.z;
    for (int i = 0; i < 3; i++) { s[4 + i] = st.translation[i]; s[7 + i] = st.velocity[i]; s[10 + i] = st.ba[i]; s[13 + i] = st.bg[i]; }
}

// builds the two-frame window updateIEKF needs: all_cloud_frame[id-1] (previous) and the current frame
struct FrameWindow {
    std::vector<point3D> no_points;
    cloudFrame prev, cur;
    srl_lio *owner;
    std::vector<cloudFrame *> saved;          // the replay driver's own window, put back on exit
    ~FrameWindow() { owner->lio->all_cloud_frame.swap(saved); }
    FrameWindow(srl_lio *h, const double state_io[16], const double t_last[3], int frame_id, std::vector<point3D> &pts)
        : prev(no_points, &h->prev_state), cur(pts, &h->cur_state), owner(h) {
        saved.swap(h->lio->all_cloud_frame);
        h->prev_state = state();
        h->prev_state.translation = srl::vec3(t_last[0], t_last[1], t_last[2]);
        state_from(state_io, h->cur_state);
        prev.id = 0; prev.frame_id = frame_id - 1;
        cur.id = 1; cur.frame_id = frame_id;
        h->lio->all_cloud_frame.clear();
        h->lio->all_cloud_frame.push_back(&prev);
        h->lio->all_cloud_frame.push_back(&cur);
    }
};

void write_log(const lioOptimization &L, double *log, int max_log_iters) {
    if (!log) return;
    const int m = std::min<int>((int)L.iteration_log.size(), max_log_iters);
    for (int i = 0; i < m; i++) {
        double *row = log + (size_t)i * 61;
        std::memcpy(row, L.iteration_log[i].neq.HtH, 36 * sizeof(double));
        std::memcpy(row + 36, L.iteration_log[i].neq.Hth, 6 * sizeof(double));
        for (int a = 0; a < 17; a++) row[42 + a] = L.iteration_log[i].d_x[a];
        row[59] = (double)L.iteration_log[i].neq.num_residuals;
        row[60] = L.iteration_log[i].neq.loss_sum;
    }
}

int run_update(srl_lio *h, const srl_icp_opts *opts, std::vector<point3D> &keypoints, double state_io[16],
               const double t_last[3], int frame_id, double *log, int max_log_iters, int *iters, int *num_res,
               bool resident = false) {
    FrameWindow w(h, state_io, t_last, frame_id, keypoints);
    h->lio->record_iterations = (log != nullptr);
    const icpOptions o = icpOptions::fromAbi(*opts);
    optimizeSummary s;
    try {
        s = resident ? h->lio->solveIEKF(o, &w.cur) : h->lio->updateIEKF(o, h->lio->voxel_map, keypoints, &w.cur);
    } catch (const std::exception &e) {
        // the NaN throw of optimize.cpp:348-350 leaves p_frame->p_state as the passes before it wrote it (:255-259): hand that back too
        h->lio->all_cloud_frame.clear();
        state_to(h->cur_state, state_io);
        if (iters) *iters = h->lio->last_num_iterations;
        return status_from_exception(h, e);
    }
    h->lio->all_cloud_frame.clear();
    state_to(h->cur_state, state_io);
    write_log(*h->lio, log, max_log_iters);
    if (iters) *iters = h->lio->last_num_iterations;
    if (num_res) *num_res = s.num_residuals_used;
    if (!s.success) { h->err = s.error_log; return SRL_ERR_NOT_ENOUGH_RESIDUALS; }
    return SRL_OK;
}

}  // namespace

extern "C" {

int srl_lio_create(int device, srl_lio **out) {
    if (!out) return SRL_ERR_BAD_ARG;
    *out = nullptr;
    srl_lio *h = new (std::nothrow) srl_lio();
    if (!h) return SRL_ERR_HIP;
    try {
        h->lio = new lioOptimization(device);
    } catch (const std::exception &) {
        delete h;
        return SRL_ERR_NO_DEVICE;
    }
    *out = h;
    return SRL_OK;
}

int srl_lio_destroy(srl_lio *h) {
    if (!h) return SRL_OK;
    delete h->oft;                            // its device tracker lives on the context lio owns
    delete h->lio;
    delete h;
    return SRL_OK;
}

srl_ctx *srl_lio_ctx(srl_lio *h) { return h ? h->lio->context() : nullptr; }
const char *srl_lio_last_error(srl_lio *h) { return h ? h->err.c_str() : "null handle"; }

int srl_lio_set_extrinsics(srl_lio *h, const double R_il[9], const double t_il[3]) {
    if (!h || !R_il || !t_il) return SRL_ERR_BAD_ARG;
    for (int i = 0; i < 9; i++) h->lio->R_imu_lidar.a[i] = R_il[i];
    for (int i = 0; i < 3; i++) h->lio->t_imu_lidar.a[i] = t_il[i];
    return SRL_OK;
}
int srl_lio_set_laser_point_cov(srl_lio *h, double cov) { if (!h) return SRL_ERR_BAD_ARG; h->lio->laser_point_cov = cov; return SRL_OK; }
int srl_lio_last_solve_observed(srl_lio *h, int *observed) {
    if (!h || !observed) return SRL_ERR_BAD_ARG;
    *observed = h->lio->last_num_observed;
    return SRL_OK;
}
int srl_lio_last_solve_launches(srl_lio *h, int *launches) { if (!h || !launches) return SRL_ERR_BAD_ARG; *launches = h->lio->last_solve_launches; return SRL_OK; }

int srl_lio_eskf_get_state(srl_lio *h, double s[19]) {
    if (!h || !s) return SRL_ERR_BAD_ARG;
    eskfEstimator *e = h->lio->eskf_pro;
    const srl::Vec3 p = e->getTranslation(), v = e->getVelocity(), ba = e->getBa(), bg = e->getBg(), g = e->getGravity();
    const srl::Quat q = e->getRotation();
    for (int i = 0; i < 3; i++) { s[i] = p[i]; s[7 + i] = v[i]; s[10 + i] = ba[i]; s[13 + i] = bg[i]; s[16 + i] = g[i]; }
    s[3] = q.w; s[4] = q.x; s[5] = q.y; s[6] = q.z;
    return SRL_OK;
}
int srl_lio_eskf_set_state(srl_lio *h, const double s[19]) {
    if (!h || !s) return SRL_ERR_BAD_ARG;
    eskfEstimator *e = h->lio->eskf_pro;
    e->setTranslation(srl::vec3(s[0], s[1], s[2]));
    e->setRotation(srl::Quat(s[3], s[4], s[5], s[6]));
    e->setVelocity(srl::vec3(s[7], s[8], s[9]));
    e->setBa(srl::vec3(s[10], s[11], s[12]));
    e->setBg(srl::vec3(s[13], s[14], s[15]));
    e->setGravity(srl::vec3(s[16], s[17], s[18]));
    return SRL_OK;
}
int srl_lio_eskf_get_cov(srl_lio *h, double P[289]) {
    if (!h || !P) return SRL_ERR_BAD_ARG;
    const srl::Mat17 c = h->lio->eskf_pro->getCovariance();
    std::memcpy(P, c.a, sizeof c.a);
    return SRL_OK;
}
int srl_lio_eskf_set_cov(srl_lio *h, const double P[289]) {
    if (!h || !P) return SRL_ERR_BAD_ARG;
    srl::Mat17 c;
    std::memcpy(c.a, P, sizeof c.a);
    h->lio->eskf_pro->setCovariance(c);
    return SRL_OK;
}
int srl_lio_eskf_set_noise(srl_lio *h, double acc_cov, double gyr_cov, double b_acc_cov, double b_gyr_cov) {
    if (!h) return SRL_ERR_BAD_ARG;
    eskfEstimator *e = h->lio->eskf_pro;
    e->setAccCov(acc_cov); e->setGyrCov(gyr_cov); e->setBiasAccCov(b_acc_cov); e->setBiasGyrCov(b_gyr_cov);
    e->useScaleCovAsCov();
    e->initializeNoise();
    return SRL_OK;
}
int srl_lio_eskf_init_imu(srl_lio *h, const double acc0[3], const double gyr0[3]) {
    if (!h || !acc0 || !gyr0) return SRL_ERR_BAD_ARG;
    h->lio->eskf_pro->initializeImuData(srl::vec3(acc0[0], acc0[1], acc0[2]), srl::vec3(gyr0[0], gyr0[1], gyr0[2]));
    return SRL_OK;
}
int srl_lio_eskf_scale_init_cov(srl_lio *h) { if (!h) return SRL_ERR_BAD_ARG; h->lio->eskf_pro->scaleInitialCovariance(); return SRL_OK; }
int srl_lio_eskf_predict(srl_lio *h, double dt, const double acc1[3], const double gyr1[3]) {
    if (!h || !acc1 || !gyr1) return SRL_ERR_BAD_ARG;
    h->lio->eskf_pro->predict(dt, srl::vec3(acc1[0], acc1[1], acc1[2]), srl::vec3(gyr1[0], gyr1[1], gyr1[2]));
    return SRL_OK;
}
int srl_lio_eskf_observe(srl_lio *h, const double dx[17]) {
    if (!h || !dx) return SRL_ERR_BAD_ARG;
    srl::Vec17 d;
    std::memcpy(d.a, dx, sizeof d.a);
    h->lio->eskf_pro->observe(d);
    return SRL_OK;
}

int srl_lio_add_points_to_map(srl_lio *h, const double *world_xyz, int n, double voxel_size, int max_num_points_in_voxel,
                              double min_distance_points, int min_num_points) {
    if (!h || n < 0 || (n > 0 && !world_xyz)) return SRL_ERR_BAD_ARG;
    std::vector<point3D> pts((size_t)n);
    for (int k = 0; k < n; k++) pts[k].point = srl::vec3(world_xyz[(size_t)k * 3], world_xyz[(size_t)k * 3 + 1], world_xyz[(size_t)k * 3 + 2]);
    state st;
    cloudFrame frame(pts, &st);
    try {
        h->lio->addPointsToMap(h->lio->voxel_map, &frame, voxel_size, max_num_points_in_voxel, min_distance_points, min_num_points, false);
    } catch (const std::exception &e) { return status_from_exception(h, e); }
    return SRL_OK;
}
int srl_lio_map_size(srl_lio *h, int64_t *num_points) {
    if (!h || !num_points) return SRL_ERR_BAD_ARG;
    try { *num_points = (int64_t)h->lio->mapSize(h->lio->voxel_map); }
    catch (const std::exception &e) { return status_from_exception(h, e); }
    return SRL_OK;
}
int srl_lio_remove_points_far_from_location(srl_lio *h, const double location[3], double distance) {
    if (!h || !location) return SRL_ERR_BAD_ARG;
    try { h->lio->removePointsFarFromLocation(h->lio->voxel_map, srl::vec3(location[0], location[1], location[2]), distance); }
    catch (const std::exception &e) { return status_from_exception(h, e); }
    return SRL_OK;
}

int srl_lio_set_collect_points_world(srl_lio *h, int on) {
    if (!h) return SRL_ERR_BAD_ARG;
    h->lio->setCollectPointsWorld(on != 0);
    return SRL_OK;
}
int srl_lio_points_world(srl_lio *h, srl_cloud_point *out, int capacity, int *n) {
    if (n) *n = 0;
    if (!h || !n || capacity < 0 || (capacity > 0 && !out)) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) { h->err = "host-only handle: no device map, no points_world"; return SRL_ERR_NO_DEVICE; }
    const std::vector<srl_cloud_point> &pw = h->lio->points_world;
    *n = (int)pw.size();
    if ((int)pw.size() > capacity) return capacity == 0 ? SRL_OK : SRL_ERR_BAD_ARG;     // capacity 0: the size query
    if (!pw.empty()) std::memcpy(out, pw.data(), pw.size() * sizeof(srl_cloud_point));
    return SRL_OK;
}

int srl_lio_set_color_map_options(srl_lio *h, const srl_color_opts *opts) {
    if (!h) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) { h->err = "host-only handle: no device, no colour map"; return SRL_ERR_NO_DEVICE; }
    srl_color_opts o;
    if (opts) o = *opts; else srl_color_opts_default(&o);
    try { h->lio->setColorMapOptions(o); }
    catch (const std::exception &e) { return status_from_exception(h, e); }
    return SRL_OK;
}
int srl_lio_set_color_times(srl_lio *h, double time_last_process, double commit_time_sweep_end, int to_rendering) {
    if (!h) return SRL_ERR_BAD_ARG;
    h->lio->time_last_process = time_last_process;
    h->lio->commit_time_sweep_end = commit_time_sweep_end;
    h->lio->to_rendering = to_rendering != 0;
    return SRL_OK;
}
int srl_lio_add_points_to_map_at(srl_lio *h, const double *world_xyz, int n, double voxel_size, int max_num_points_in_voxel, double min_distance_points,
                                 int min_num_points, double time_sweep_end, int to_rendering) {
    if (!h || n < 0 || (n > 0 && !world_xyz)) return SRL_ERR_BAD_ARG;
    std::vector<point3D> pts((size_t)n);
    for (int k = 0; k < n; k++) pts[k].point = srl::vec3(world_xyz[(size_t)k * 3], world_xyz[(size_t)k * 3 + 1], world_xyz[(size_t)k * 3 + 2]);
    state st;
    cloudFrame frame(pts, &st);
    frame.time_sweep_end = time_sweep_end;
    try {
        h->lio->addPointsToMap(h->lio->voxel_map, &frame, voxel_size, max_num_points_in_voxel, min_distance_points, min_num_points, to_rendering != 0);
    } catch (const std::exception &e) { return status_from_exception(h, e); }
    return SRL_OK;
}
int srl_lio_color_visited(srl_lio *h, int which, int32_t *out_xyz, int capacity, int *n, int *number_of_new_visited_voxel) {
    if (n) *n = 0;
    if (number_of_new_visited_voxel) *number_of_new_visited_voxel = 0;
    if (!h || !n || which < 0 || which > 1 || capacity < 0 || (capacity > 0 && !out_xyz)) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) { h->err = "host-only handle: no device, no colour map"; return SRL_ERR_NO_DEVICE; }
    const auto &list = which == 0 ? h->lio->voxels_recent_visited_temp : h->lio->voxels_recent_visited;
    *n = (int)list.size();
    if (number_of_new_visited_voxel) *number_of_new_visited_voxel = h->lio->number_of_new_visited_voxel;
    if ((int)list.size() > capacity) return capacity == 0 ? SRL_OK : SRL_ERR_BAD_ARG;
    for (size_t k = 0; k < list.size(); k++) { out_xyz[k * 3] = list[k].kx; out_xyz[k * 3 + 1] = list[k].ky; out_xyz[k * 3 + 2] = list[k].kz; }
    return SRL_OK;
}
int srl_lio_color_stored(srl_lio *h, srl_color_stored *out, int capacity, int *n) {
    if (n) *n = 0;
    if (!h || !n || capacity < 0 || (capacity > 0 && !out)) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) { h->err = "host-only handle: no device, no colour map"; return SRL_ERR_NO_DEVICE; }
    const std::vector<srl_color_stored> &cs = h->lio->color_stored;
    *n = (int)cs.size();
    if ((int)cs.size() > capacity) return capacity == 0 ? SRL_OK : SRL_ERR_BAD_ARG;
    if (!cs.empty()) std::memcpy(out, cs.data(), cs.size() * sizeof(srl_color_stored));
    return SRL_OK;
}

int srl_lio_render_points_in_recent_voxel(srl_lio *h, const srl_color_camera *camera, double obs_time, srl_color_render_totals *totals) {
    if (totals) std::memset(totals, 0, sizeof *totals);
    if (!h || !camera) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) { h->err = "host-only handle: no device, no colour map"; return SRL_ERR_NO_DEVICE; }
    try { h->lio->renderPointsInRecentVoxel(*camera, obs_time); }
    catch (const std::exception &e) { return status_from_exception(h, e); }
    if (totals) *totals = h->lio->render_totals;
    return SRL_OK;
}

int srl_lio_select_points_for_projection(srl_lio *h, const srl_color_camera *camera, int rows, int cols, double minimum_dis, int skip_step, int use_all_points,
                                         int refresh, srl_color_selected *out, int capacity, int *n, srl_color_select_totals *totals) {
    if (n) *n = 0;
    if (totals) std::memset(totals, 0, sizeof *totals);
    if (!h || !camera || !n || capacity < 0 || (capacity > 0 && !out)) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) { h->err = "host-only handle: no device, no colour map"; return SRL_ERR_NO_DEVICE; }
    std::vector<srl_color_selected> mine;
    const std::vector<srl_color_selected> *rec = &mine;
    try {
        if (refresh) {
            if (rows == 0 || cols == 0) return SRL_OK;                   // refreshPointsForProjection returns at once: nothing is selected, nothing kept
            h->lio->refreshPointsForProjection(*camera, rows, cols);
            rec = &h->lio->points_for_projection;
        } else {
            mine = h->lio->selectPointsForProjection(*camera, rows, cols, minimum_dis, skip_step, use_all_points != 0);
        }
    } catch (const std::exception &e) { return status_from_exception(h, e); }
    *n = (int)rec->size();
    if (totals) *totals = h->lio->select_totals;
    if ((int)rec->size() > capacity) return capacity == 0 ? SRL_OK : SRL_ERR_BAD_ARG;
    if (!rec->empty()) std::memcpy(out, rec->data(), rec->size() * sizeof(srl_color_selected));
    return SRL_OK;
}

int srl_lio_color_cloud(srl_lio *h, int which, int minimum_views, srl_color_cloud_point *out, int32_t *point_index, int64_t capacity, int64_t *n,
                        srl_color_cloud_totals *totals) {
    if (n) *n = 0;
    if (totals) std::memset(totals, 0, sizeof *totals);
    if (!h || !n || which < 0 || which > 1 || capacity < 0 || (capacity > 0 && !out)) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) { h->err = "host-only handle: no device, no colour map"; return SRL_ERR_NO_DEVICE; }      // never a host loop
    int rc;
    try { rc = h->lio->colorCloud(which, minimum_views, capacity > 0 ? out : nullptr, capacity > 0 ? point_index : nullptr, capacity); }
    catch (const std::exception &e) { return status_from_exception(h, e); }
    *n = h->lio->cloud_totals.published;
    if (totals) *totals = h->lio->cloud_totals;
    if (rc != SRL_OK) h->err = srl_last_error(h->lio->context());
    return rc;
}

int srl_lio_color_cloud_view(srl_lio *h, int which, int minimum_views, int with_point_index, const srl_color_cloud_point **points,
                             const int32_t **point_index, int64_t *n, srl_color_cloud_totals *totals) {
    if (n) *n = 0;
    if (points) *points = nullptr;
    if (point_index) *point_index = nullptr;
    if (totals) std::memset(totals, 0, sizeof *totals);
    if (!h || !n || !points || which < 0 || which > 1 || (with_point_index && !point_index)) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) { h->err = "host-only handle: no device, no colour map"; return SRL_ERR_NO_DEVICE; }
    try {
        const lioOptimization::colorCloudView v = which == 0 ? h->lio->pubColorPoints(minimum_views, with_point_index != 0)
                                                             : h->lio->saveColorPoints(minimum_views, with_point_index != 0);
        *points = v.points; *n = (int64_t)v.size;
        if (point_index) *point_index = v.point_index;
    } catch (const std::exception &e) { return status_from_exception(h, e); }
    if (totals) *totals = h->lio->cloud_totals;
    return SRL_OK;
}

int srl_lio_color_topic_sizes(srl_lio *h, int64_t published, int32_t *sizes, int capacity, int *n_topics) {
    if (n_topics) *n_topics = 0;
    if (!h || !n_topics || published < 0 || capacity < 0 || (capacity > 0 && !sizes)) return SRL_ERR_BAD_ARG;
    const int64_t topics = h->lio->colorTopicCount(published);
    if (topics > 0x7FFFFFFF) return SRL_ERR_BAD_ARG;
    *n_topics = (int)topics;
    if (topics > capacity) return capacity == 0 ? SRL_OK : SRL_ERR_BAD_ARG;      // the carried state stays as it was
    const std::vector<int32_t> s = h->lio->colorTopicSizes(published);
    std::memcpy(sizes, s.data(), s.size() * sizeof(int32_t));
    return SRL_OK;
}
int srl_lio_color_topic_state(srl_lio *h, int *number_of_points_per_topic, int *sleep_time_after_pub) {
    if (!h) return SRL_ERR_BAD_ARG;
    if (number_of_points_per_topic) *number_of_points_per_topic = h->lio->number_of_points_per_topic;
    if (sleep_time_after_pub) *sleep_time_after_pub = h->lio->sleep_time_after_pub;
    return SRL_OK;
}

int srl_lio_set_device_subsample(srl_lio *h, int on) {
    if (!h) return SRL_ERR_BAD_ARG;
    h->lio->device_subsample = on != 0;
    return SRL_OK;
}

int srl_lio_probe_checksum_of_committed_frame(srl_lio *h, int stride, double voxel_size, uint64_t *checksum, int32_t *num_voxels) {
    if (!h || !checksum) return SRL_ERR_BAD_ARG;
    srl_ctx *ctx = h->lio->context();
    if (!ctx) return SRL_ERR_NO_DEVICE;
    int rc = srl_map_probe_checksum(ctx, nullptr, 0, stride, voxel_size, checksum);
    if (rc == SRL_OK && num_voxels) rc = srl_map_size(ctx, nullptr, num_voxels);
    return rc;
}

int srl_lio_resident_sweep(srl_lio *h, const double *raw_xyz, int n) {
    if (!h || n < 0 || (n > 0 && !raw_xyz)) return SRL_ERR_BAD_ARG;
    return h->lio->residentSweep(raw_xyz, n);
}

int srl_lio_prefetch_sweep(srl_lio *h, const double *raw_xyz, int n) {
    if (!h || n < 0 || (n > 0 && !raw_xyz)) return SRL_ERR_BAD_ARG;
    return h->lio->prefetchSweep(raw_xyz, n);
}
int srl_lio_prefetch_sweep_during_solve(srl_lio *h, const double *raw_xyz, int n) {
    if (!h || n < 0 || (n > 0 && !raw_xyz)) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) return SRL_ERR_NO_DEVICE;
    h->lio->prefetchSweepDuringSolve(raw_xyz, n);
    return SRL_OK;
}
int srl_lio_swap_sweep(srl_lio *h) {
    if (!h) return SRL_ERR_BAD_ARG;
    return h->lio->swapSweep();
}

int srl_lio_update_iekf(srl_lio *h, const srl_icp_opts *opts, const double *raw_xyz, int n, double state_io[16],
                        const double t_last[3], int frame_id, double *log, int max_log_iters, int *iters,
                        int *num_residuals_used) {
    if (!h || !opts || !state_io || !t_last || n < 0) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) { h->err = "host-only handle: use srl_lio_update_iekf_provided"; return SRL_ERR_NO_DEVICE; }
    h->lio->setNormalEqProvider(nullptr, nullptr);
    std::vector<point3D> keypoints;
    if (raw_xyz) {
        h->lio->releaseSweep();
        keypoints.resize((size_t)n);
        for (int k = 0; k < n; k++) keypoints[k].raw_point = srl::vec3(raw_xyz[(size_t)k * 3], raw_xyz[(size_t)k * 3 + 1], raw_xyz[(size_t)k * 3 + 2]);
        return run_update(h, opts, keypoints, state_io, t_last, frame_id, log, max_log_iters, iters, num_residuals_used);
    }
    if (!h->lio->sweepPinned(n)) { h->err = "no resident sweep of this size"; return SRL_ERR_NO_SWEEP; }
    return run_update(h, opts, keypoints, state_io, t_last, frame_id, log, max_log_iters, iters, num_residuals_used, true);
}

int srl_lio_stream_step(srl_lio *h, const srl_icp_opts *opts, const double eskf_state[19], const double eskf_cov[289], int n, double state_io[16],
                        const double t_last[3], int frame_id, const double *next_raw_xyz, int next_n, int *iters, int *num_residuals_used) {
    if (!h || !opts || !state_io || !t_last || n < 0 || next_n < 0) return SRL_ERR_BAD_ARG;
    int rc = SRL_OK;
    if (eskf_state && (rc = srl_lio_eskf_set_state(h, eskf_state)) != SRL_OK) return rc;
    if (eskf_cov && (rc = srl_lio_eskf_set_cov(h, eskf_cov)) != SRL_OK) return rc;
    if (next_raw_xyz && (rc = srl_lio_prefetch_sweep_during_solve(h, next_raw_xyz, next_n)) != SRL_OK) return rc;
    if ((rc = srl_lio_update_iekf(h, opts, nullptr, n, state_io, t_last, frame_id, nullptr, 0, iters, num_residuals_used)) != SRL_OK) return rc;
    return next_raw_xyz ? srl_lio_swap_sweep(h) : SRL_OK;
}

int srl_lio_update_iekf_provided(srl_lio *h, const srl_icp_opts *opts, srl_normal_eq_provider provider, void *user, int n,
                                 double state_io[16], const double t_last[3], int frame_id, double *log, int max_log_iters,
                                 int *iters, int *num_residuals_used) {
    if (!h || !opts || !provider || !state_io || !t_last || n < 0) return SRL_ERR_BAD_ARG;
    (void)n;
    h->lio->setNormalEqProvider(provider, user);
    std::vector<point3D> keypoints;
    int rc = run_update(h, opts, keypoints, state_io, t_last, frame_id, log, max_log_iters, iters, num_residuals_used, true);
    h->lio->setNormalEqProvider(nullptr, nullptr);
    return rc;
}

int srl_lio_optimize(srl_lio *h, const srl_icp_opts *opts, double sample_voxel_size, const double *frame_raw,
                     double *frame_world, int n, double state_io[16], const double t_last[3], int frame_id,
                     int32_t *keypoint_index, int *num_keypoints, int *iters, int *num_residuals_used) {
    if (!h || !opts || !frame_raw || !frame_world || !state_io || !t_last || n < 0) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) return SRL_ERR_NO_DEVICE;
    h->lio->setNormalEqProvider(nullptr, nullptr);
    std::vector<point3D> pts((size_t)n);
    for (int k = 0; k < n; k++) {
        pts[k].raw_point = srl::vec3(frame_raw[(size_t)k * 3], frame_raw[(size_t)k * 3 + 1], frame_raw[(size_t)k * 3 + 2]);
        pts[k].point = srl::vec3(frame_world[(size_t)k * 3], frame_world[(size_t)k * 3 + 1], frame_world[(size_t)k * 3 + 2]);
        pts[k].index_frame = k;
    }
    if (keypoint_index || num_keypoints) {
        std::vector<point3D> kp;
        gridSampling(pts, kp, sample_voxel_size);
        if (num_keypoints) *num_keypoints = (int)kp.size();
        if (keypoint_index) for (size_t i = 0; i < kp.size(); i++) keypoint_index[i] = kp[i].index_frame;
    }
    FrameWindow w(h, state_io, t_last, frame_id, pts);
    const icpOptions o = icpOptions::fromAbi(*opts);
    optimizeSummary s;
    try {
        s = h->lio->optimize(&w.cur, o, sample_voxel_size);
    } catch (const std::exception &e) {
        h->lio->all_cloud_frame.clear();
        return status_from_exception(h, e);
    }
    h->lio->all_cloud_frame.clear();
    state_to(h->cur_state, state_io);
    if (iters) *iters = h->lio->last_num_iterations;
    if (num_residuals_used) *num_residuals_used = s.num_residuals_used;
    if (!s.success) { h->err = s.error_log; return SRL_ERR_NOT_ENOUGH_RESIDUALS; }
    for (int k = 0; k < n; k++) for (int d = 0; d < 3; d++) frame_world[(size_t)k * 3 + d] = w.cur.point_frame[k].point[d];
    return SRL_OK;
}

int srl_lio_eskf_try_init(srl_lio *h, const double *t, const double *gyr, const double *acc, int n, int *initialized) {
    if (!h || n < 0 || (n > 0 && (!t || !gyr || !acc))) return SRL_ERR_BAD_ARG;
    std::vector<imuMeas> meas((size_t)n);
    for (int i = 0; i < n; i++) {
        meas[i].first = t[i];
        meas[i].second.first = srl::vec3(gyr[3 * i], gyr[3 * i + 1], gyr[3 * i + 2]);
        meas[i].second.second = srl::vec3(acc[3 * i], acc[3 * i + 1], acc[3 * i + 2]);
    }
    const int r = h->lio->eskf_pro->tryInit(meas);
    if (initialized) *initialized = r;
    return SRL_OK;
}
int srl_lio_eskf_get_init_stats(srl_lio *h, double out[14]) {
    if (!h || !out) return SRL_ERR_BAD_ARG;
    const eskfEstimator *e = h->lio->eskf_pro;
    const srl::Vec3 v[4] = {e->getMeanGyr(), e->getMeanAcc(), e->getGyrCov(), e->getAccCov()};
    for (int k = 0; k < 4; k++) for (int d = 0; d < 3; d++) out[3 * k + d] = v[k][d];
    out[12] = (double)e->getNumInitMeas();
    out[13] = initial_flag ? 1.0 : 0.0;
    return SRL_OK;
}
int srl_lio_set_initial_flag(srl_lio *h, int flag) {
    if (!h) return SRL_ERR_BAD_ARG;
    initial_flag = flag != 0;
    return SRL_OK;
}
int srl_lio_set_g_norm(srl_lio *h, double g_norm) {
    if (!h || !(g_norm > 0.0) || !std::isfinite(g_norm)) return SRL_ERR_BAD_ARG;
    G_norm = g_norm;
    return SRL_OK;
}
int srl_lio_state_initialization(srl_lio *h, int index_frame, int initialization, const double prev2[7], const double prev1[7],
                                 double out[7]) {
    if (!h || !out || (index_frame > 2 && (!prev2 || !prev1))) return SRL_ERR_BAD_ARG;
    state s2, s1, cur;
    if (index_frame > 2) {
        s2.rotation = srl::Quat(prev2[0], prev2[1], prev2[2], prev2[3]); s2.translation = srl::vec3(prev2[4], prev2[5], prev2[6]);
        s1.rotation = srl::Quat(prev1[0], prev1[1], prev1[2], prev1[3]); s1.translation = srl::vec3(prev1[4], prev1[5], prev1[6]);
    }
    std::vector<point3D> none;
    cloudFrame f2(none, &s2), f1(none, &s1);
    std::vector<cloudFrame *> saved;
    saved.swap(h->lio->all_cloud_frame);
    h->lio->all_cloud_frame.push_back(&f2);
    h->lio->all_cloud_frame.push_back(&f1);
    const int saved_index = h->lio->index_frame, saved_init = h->lio->initialization;
    h->lio->index_frame = index_frame;
    h->lio->initialization = initialization;
    h->lio->stateInitialization(&cur);
    h->lio->all_cloud_frame.swap(saved);
    h->lio->index_frame = saved_index;
    h->lio->initialization = saved_init;
    out[0] = cur.rotation.w; out[1] = cur.rotation.x; out[2] = cur.rotation.y; out[3] = cur.rotation.z;
    for (int d = 0; d < 3; d++) out[4 + d] = cur.translation[d];
    return SRL_OK;
}

// ---- ROS-free replay driver
int srl_lio_set_odometry_options(srl_lio *h, const srl_odometry_opts *o) {
    if (!h || !o) return SRL_ERR_BAD_ARG;
    lioOptimization &L = *h->lio;
    L.init_voxel_size = o->init_voxel_size; L.init_sample_voxel_size = o->init_sample_voxel_size;
    L.init_num_frames = o->init_num_frames; L.num_for_initialization = o->num_for_initialization;
    L.voxel_size = o->voxel_size; L.sample_voxel_size = o->sample_voxel_size;
    L.max_num_points_in_voxel = o->max_num_points_in_voxel; L.min_distance_points = o->min_distance_points;
    L.motion_compensation = o->motion_compensation; L.initialization = o->initialization;
    L.point_time_enable = o->point_time_enable != 0;
    L.optimize_options = icpOptions::fromAbi(o->icp);
    L.eskf_pro->setAccCov(o->acc_cov); L.eskf_pro->setGyrCov(o->gyr_cov);
    L.eskf_pro->setBiasAccCov(o->b_acc_cov); L.eskf_pro->setBiasGyrCov(o->b_gyr_cov);
    return SRL_OK;
}

int srl_lio_run_measurement(srl_lio *h, double time_frame, const double *imu_t, const double *imu_acc, const double *imu_gyr,
                            int n_imu, const double *pts_raw, const double *pts_timestamp, int n_pts, double time_sweep_begin,
                            double time_sweep_offset, srl_replay_result *out) {
    if (!h || n_imu < 0 || n_pts < 0 || (n_imu > 0 && (!imu_t || !imu_acc || !imu_gyr)) || (n_pts > 0 && (!pts_raw || !pts_timestamp)))
        return SRL_ERR_BAD_ARG;
    lioOptimization &L = *h->lio;
    lioOptimization::Measurement m;
    m.time_frame = time_frame; m.time_sweep_begin = time_sweep_begin; m.time_sweep_offset = time_sweep_offset;
    m.imu.resize((size_t)n_imu);
    for (int i = 0; i < n_imu; i++) {
        m.imu[i].time = imu_t[i];
        m.imu[i].acc = srl::vec3(imu_acc[3 * i], imu_acc[3 * i + 1], imu_acc[3 * i + 2]);
        m.imu[i].gyr = srl::vec3(imu_gyr[3 * i], imu_gyr[3 * i + 1], imu_gyr[3 * i + 2]);
    }
    m.lidar_points.resize((size_t)n_pts);
    for (int i = 0; i < n_pts; i++) {
        point3D &p = m.lidar_points[i];
        p.raw_point = srl::vec3(pts_raw[3 * (size_t)i], pts_raw[3 * (size_t)i + 1], pts_raw[3 * (size_t)i + 2]);
        p.point = p.raw_point;                                   // cloudProcessing.cpp:143
        p.timestamp = pts_timestamp[i];
    }
    optimizeSummary s;
    bool processed = false;
    if (out) std::memset(out, 0, sizeof *out);
    try {
        if (initial_flag && !L.context()) return SRL_ERR_NO_DEVICE;
        processed = L.runMeasurement(m, &s);
    } catch (const std::exception &e) { return status_from_exception(h, e); }
    if (out) {
        out->processed = processed ? 1 : 0;
        out->initialized = initial_flag ? 1 : 0;
        out->index_frame = L.index_frame;
        if (processed) {
            out->success = s.success ? 1 : 0;
            out->num_residuals_used = s.num_residuals_used;
            out->iterations = L.last_num_iterations;
            out->frame_points = L.last_frame_points;
            out->keypoints = L.last_frame_keypoints;
            out->points_added = L.last_points_added;
            const state *st = L.all_cloud_frame.back()->p_state;
            state_to(*st, out->state);
        }
    }
    if (processed && !s.success) { h->err = s.error_log; return SRL_ERR_NOT_ENOUGH_RESIDUALS; }
    return SRL_OK;
}

// ---- the point side of the node: Livox messages into the device point queue, sweeps cut from it
int srl_lio_set_lidar_options(srl_lio *h, const srl_livox_opts *o) {
    if (!h || !o) return SRL_ERR_BAD_ARG;
    if (o->point_filter_num < 1 || o->n_scans < 0 || !(o->time_unit_scale > 0.0) || std::isinf(o->time_unit_scale) || std::isnan(o->blind)) return SRL_ERR_BAD_ARG;
    h->lio->lidar_options = *o;
    h->lio->lidar_options_set = true;
    return SRL_OK;
}

int srl_lio_feed_livox(srl_lio *h, const srl_livox_point *points, int point_num, double header_stamp, srl_livox_report *report) {
    if (report) { std::memset(report, 0, sizeof *report); report->last_end_time = report->first_timestamp = report->last_timestamp = std::nan(""); }
    if (!h || point_num < 0 || (point_num > 0 && !points)) return SRL_ERR_BAD_ARG;
    lioOptimization &L = *h->lio;
    if (!L.lidar_options_set) { h->err = "srl_lio_feed_livox: no options (srl_lio_set_lidar_options)"; return SRL_ERR_BAD_ARG; }
    // lioOptimization.cpp:595: assert(msg->header.stamp.toSec() > last_time_lidar) -- here a refusal, and nothing is queued
    if (!(header_stamp > L.last_time_lidar)) { h->err = "srl_lio_feed_livox: a message that is not newer than the last one"; return SRL_ERR_BAD_ARG; }
    srl_ctx *ctx = L.context();
    if (!ctx) { h->err = "host-only handle: no device, no point queue"; return SRL_ERR_NO_DEVICE; }
    srl_livox_report r;
    const int rc = srl_livox_decode(ctx, points, point_num, header_stamp, &L.lidar_options, &r);
    if (rc != SRL_OK) { h->err = srl_last_error(ctx); return rc; }
    L.last_time_lidar = header_stamp;                              // :600
    if (r.valid > 0) L.last_end_time = r.last_end_time;            // cloudProcessing.cpp:213 (no valid point: .back() of an empty vector upstream; kept here)
    if (report) *report = r;
    return SRL_OK;
}

// ---- ... and PointCloud2 messages of the spinning LiDARs into the same queue
int srl_lio_set_pc2_options(srl_lio *h, const srl_pc2_opts *o) {
    if (!h || !o) return SRL_ERR_BAD_ARG;
    if (o->lidar_type < 2 || o->lidar_type > 4 || o->point_filter_num < 1 || !(o->time_unit_scale > 0.0) || std::isinf(o->time_unit_scale) || std::isnan(o->blind))
        return SRL_ERR_BAD_ARG;
    h->lio->pc2_options = *o;          // (scan_rate and n_scans matter in the yaw branch alone: srl_pc2_decode refuses them there)
    h->lio->pc2_options_set = true;
    return SRL_OK;
}

int srl_lio_feed_pointcloud2(srl_lio *h, const void *data, size_t data_bytes, const srl_pc2_layout *layout, double header_stamp, srl_pc2_report *report) {
    if (report) { std::memset(report, 0, sizeof *report); report->last_end_time = report->first_timestamp = report->last_timestamp = std::nan(""); }
    if (!h || !data || !layout) return SRL_ERR_BAD_ARG;
    lioOptimization &L = *h->lio;
    if (!L.pc2_options_set) { h->err = "srl_lio_feed_pointcloud2: no options (srl_lio_set_pc2_options)"; return SRL_ERR_BAD_ARG; }
    // lioOptimization.cpp:585: assert(msg->header.stamp.toSec() > last_time_lidar) -- here a refusal, and nothing is queued
    if (!(header_stamp > L.last_time_lidar)) { h->err = "srl_lio_feed_pointcloud2: a message that is not newer than the last one"; return SRL_ERR_BAD_ARG; }
    srl_ctx *ctx = L.context();
    if (!ctx) { h->err = "host-only handle: no device, no point queue"; return SRL_ERR_NO_DEVICE; }
    srl_pc2_report r;
    const int rc = srl_pc2_decode(ctx, data, data_bytes, layout, header_stamp, L.last_end_time, &L.pc2_options, &r);
    if (rc != SRL_OK) { h->err = srl_last_error(ctx); return rc; }
    L.last_time_lidar = header_stamp;                              // :590
    if (r.points > 0) L.last_end_time = r.last_end_time;           // cloudProcessing.cpp:322 / :432 / :541 (an empty message returns before it)
    if (report) *report = r;
    return SRL_OK;
}

int srl_lio_points_info(srl_lio *h, int *size, double *front_timestamp, double *back_timestamp, double *last_time_lidar, double *last_end_time) {
    if (!h) return SRL_ERR_BAD_ARG;
    lioOptimization &L = *h->lio;
    if (last_time_lidar) *last_time_lidar = L.last_time_lidar;
    if (last_end_time) *last_end_time = L.last_end_time;
    srl_ctx *ctx = L.context();
    if (!ctx) { h->err = "host-only handle: no device, no point queue"; return SRL_ERR_NO_DEVICE; }
    const int rc = srl_points_info(ctx, size, front_timestamp, back_timestamp);
    if (rc != SRL_OK) h->err = srl_last_error(ctx);
    return rc;
}

int srl_lio_run_measurement_queued(srl_lio *h, double time_frame, const double *imu_t, const double *imu_acc, const double *imu_gyr, int n_imu,
                                   double time_cut, double time_sweep_begin, double time_sweep_offset, srl_replay_result *out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (!h || n_imu < 0 || (n_imu > 0 && (!imu_t || !imu_acc || !imu_gyr)) || std::isnan(time_cut)) return SRL_ERR_BAD_ARG;
    lioOptimization &L = *h->lio;
    srl_ctx *ctx = L.context();
    if (!ctx) { h->err = "host-only handle: no device, no point queue"; return SRL_ERR_NO_DEVICE; }
    if (!(L.device_subsample && L.voxel_size > 0)) {
        h->err = "srl_lio_run_measurement_queued needs the device sub-sample (srl_lio_set_device_subsample(1), voxel_size > 0)";
        return SRL_ERR_UNSUPPORTED;                                // the queue is left uncut
    }
    srl_points_cut_report cut;
    int rc = srl_points_cut(ctx, time_cut, &cut);
    if (rc != SRL_OK) { h->err = srl_last_error(ctx); return rc; }
    if (cut.count == 0) return SRL_OK;                             // lioOptimization.cpp:730 / :770: no lidar points, no Measurements element
    L.sweep_from_queue = true;
    rc = srl_lio_run_measurement(h, time_frame, imu_t, imu_acc, imu_gyr, n_imu, nullptr, nullptr, 0, time_sweep_begin, time_sweep_offset, out);
    L.sweep_from_queue = false;
    return rc;
}

int srl_lio_last_frame(srl_lio *h, int capacity, double *raw_point, double *point, double *imu_point, int *n) {
    if (!h || !n) return SRL_ERR_BAD_ARG;
    if (h->lio->all_cloud_frame.empty()) { *n = 0; return SRL_OK; }
    const std::vector<point3D> &f = h->lio->all_cloud_frame.back()->point_frame;
    *n = (int)f.size();
    const int m = std::min(capacity, *n);
    for (int k = 0; k < m; k++)
        for (int d = 0; d < 3; d++) {
            if (raw_point) raw_point[(size_t)k * 3 + d] = f[k].raw_point[d];
            if (point) point[(size_t)k * 3 + d] = f[k].point[d];
            if (imu_point) imu_point[(size_t)k * 3 + d] = f[k].imu_point[d];
        }
    return SRL_OK;
}

int srl_lio_optimize_resident(srl_lio *h, const srl_icp_opts *opts, double sample_voxel_size, const double *frame_raw, int n,
                              double state_io[16], const double t_last[3], int frame_id, int32_t *keypoint_index,
                              int *num_keypoints, int *iters, int *num_residuals_used) {
    if (!h || !opts || (n > 0 && !frame_raw) || !state_io || !t_last || n < 0) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) return SRL_ERR_NO_DEVICE;
    h->lio->setNormalEqProvider(nullptr, nullptr);
    std::vector<point3D> none;
    FrameWindow w(h, state_io, t_last, frame_id, none);
    const icpOptions o = icpOptions::fromAbi(*opts);
    optimizeSummary s;
    std::vector<int> kidx;
    try {
        s = h->lio->optimizeResident(&w.cur, frame_raw, n, o, sample_voxel_size, keypoint_index || num_keypoints ? &kidx : nullptr);
    } catch (const std::exception &e) {
        h->lio->all_cloud_frame.clear();
        state_to(h->cur_state, state_io);
        if (iters) *iters = h->lio->last_num_iterations;
        return status_from_exception(h, e);
    }
    h->lio->all_cloud_frame.clear();
    if (num_keypoints) *num_keypoints = (int)kidx.size();
    if (keypoint_index) for (size_t i = 0; i < kidx.size(); i++) keypoint_index[i] = kidx[i];
    state_to(h->cur_state, state_io);
    if (iters) *iters = h->lio->last_num_iterations;
    if (num_residuals_used) *num_residuals_used = s.num_residuals_used;
    if (!s.success) { h->err = s.error_log; return SRL_ERR_NOT_ENOUGH_RESIDUALS; }
    return SRL_OK;
}

int srl_lio_commit_frame(srl_lio *h, const double state[16], double voxel_size, int max_num_points_in_voxel,
                         double min_distance_points, int min_num_points, double *world_out, int *num_added) {
    if (!h || !state) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) return SRL_ERR_NO_DEVICE;
    srlivo::state st;
    state_from(state, st);
    try {
        const int added = h->lio->commitFrame(&st, voxel_size, max_num_points_in_voxel, min_distance_points, min_num_points, world_out, num_added != nullptr);
        if (num_added) *num_added = added;
    } catch (const std::exception &e) { return status_from_exception(h, e); }
    return SRL_OK;
}

int srl_lio_search_neighbors(srl_lio *h, const double point[3], int nb_voxels_visited, double size_voxel_map,
                             int max_num_neighbors, int threshold_voxel_capacity, double *out_xyz, int16_t *out_voxels,
                             int *num_found) {
    if (!h || !point || !out_xyz || !num_found) return SRL_ERR_BAD_ARG;
    try {
        std::vector<voxel> vox;
        const auto nb = h->lio->searchNeighbors(h->lio->voxel_map, srl::vec3(point[0], point[1], point[2]), nb_voxels_visited,
                                                size_voxel_map, max_num_neighbors, threshold_voxel_capacity, out_voxels ? &vox : nullptr);
        *num_found = (int)nb.size();
        for (size_t i = 0; i < nb.size(); i++) {
            for (int d = 0; d < 3; d++) out_xyz[i * 3 + d] = nb[i][d];
            if (out_voxels) { out_voxels[i * 3] = vox[i].x; out_voxels[i * 3 + 1] = vox[i].y; out_voxels[i * 3 + 2] = vox[i].z; }
        }
    } catch (const std::exception &e) { return status_from_exception(h, e); }
    return SRL_OK;
}

int srl_lio_neighborhood(srl_lio *h, const double *pts, int n, double center[3], double normal[3], double cov[9], double *a2D) {
    if (!h || !pts || n <= 0) return SRL_ERR_BAD_ARG;
    std::vector<srl::Vec3> P((size_t)n);
    for (int i = 0; i < n; i++) P[i] = srl::vec3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
    try {
        const Neighborhood nb = h->lio->computeNeighborhoodDistribution(P);
        for (int d = 0; d < 3; d++) { if (center) center[d] = nb.center[d]; if (normal) normal[d] = nb.normal[d]; }
        if (cov) std::memcpy(cov, nb.covariance.a, 9 * sizeof(double));
        if (a2D) *a2D = nb.a2D;
    } catch (const std::exception &e) { return status_from_exception(h, e); }
    return SRL_OK;
}

int srl_lio_build_plane_residuals(srl_lio *h, const srl_icp_opts *opts, const double *raw_xyz, int n, const double st[16],
                                  const double t_last[3], int frame_id, double *out_rows, int max_out, int *num_out,
                                  double *loss_sum, int *success, double *keypoint_world) {
    if (!h || !opts || !raw_xyz || !st || !t_last || n < 0) return SRL_ERR_BAD_ARG;
    if (!h->lio->context()) return SRL_ERR_NO_DEVICE;
    std::vector<point3D> keypoints((size_t)n);
    for (int k = 0; k < n; k++) keypoints[k].raw_point = srl::vec3(raw_xyz[(size_t)k * 3], raw_xyz[(size_t)k * 3 + 1], raw_xyz[(size_t)k * 3 + 2]);
    double state_io[16];
    std::memcpy(state_io, st, sizeof state_io);
    FrameWindow w(h, state_io, t_last, frame_id, keypoints);
    const icpOptions o = icpOptions::fromAbi(*opts);
    std::vector<planeParam> pr;
    double loss = 0.0;
    optimizeSummary s;
    try {
        s = h->lio->buildPlaneResiduals(o, h->lio->voxel_map, keypoints, pr, &w.cur, loss);
    } catch (const std::exception &e) {
        h->lio->all_cloud_frame.clear();
        return status_from_exception(h, e);
    }
    h->lio->all_cloud_frame.clear();
    if (num_out) *num_out = (int)pr.size();
    if (loss_sum) *loss_sum = loss;
    if (success) *success = s.success ? 1 : 0;
    if (out_rows)
        for (int i = 0; i < (int)pr.size() && i < max_out; i++) {
            double *r = out_rows + (size_t)i * 15;
            for (int d = 0; d < 3; d++) { r[d] = pr[i].raw_point[d]; r[3 + d] = pr[i].norm_vector[d]; }
            for (int c = 0; c < 6; c++) r[6 + c] = pr[i].jacobians(0, c);
            r[12] = pr[i].norm_offset; r[13] = pr[i].distance; r[14] = pr[i].weight;
        }
    if (keypoint_world) for (int k = 0; k < n; k++) for (int d = 0; d < 3; d++) keypoint_world[(size_t)k * 3 + d] = keypoints[k].point[d];
    return SRL_OK;
}

int srl_grid_sampling(const double *world_xyz, int n, double size_voxel, int32_t *index_out, int *num_out) {
    if (n < 0 || (n > 0 && !world_xyz) || !num_out) return SRL_ERR_BAD_ARG;
    std::vector<point3D> pts((size_t)n), kp;
    for (int k = 0; k < n; k++) { pts[k].point = srl::vec3(world_xyz[(size_t)k * 3], world_xyz[(size_t)k * 3 + 1], world_xyz[(size_t)k * 3 + 2]); pts[k].index_frame = k; }
    gridSampling(pts, kp, size_voxel);
    *num_out = (int)kp.size();
    if (index_out) for (size_t i = 0; i < kp.size(); i++) index_out[i] = kp[i].index_frame;
    return SRL_OK;
}

// debug / parity hook: iteration order of std::tr1::unordered_map<voxel, ...> after inserting the given DISTINCT voxel keys
// in order, computed by the flat replay of host/tr1_order.h (what srl_frame_select_keypoints uses); order_out[r] = index
// into keys of the r-th element.  tests compare it with the real container (srl_grid_sampling).
int srl_debug_tr1_order(const int16_t *keys_xyz, int n, int32_t *order_out) {
    if (n < 0 || (n > 0 && (!keys_xyz || !order_out))) return SRL_ERR_BAD_ARG;
    std::vector<std::size_t> h((size_t)n);
    for (int i = 0; i < n; i++) h[(size_t)i] = std::hash<voxel>()(voxel(keys_xyz[3 * i], keys_xyz[3 * i + 1], keys_xyz[3 * i + 2]));
    std::vector<int> out((size_t)n);
    srl::Tr1Order::order(h.data(), n, out.data());
    for (int i = 0; i < n; i++) order_out[i] = out[(size_t)i];
    return SRL_OK;
}

// debug / parity hook: the same order from the RELATION of host/tr1_relation.h, by the steps of the device ordering of
// srl_frame_select_keypoints (bucket of every element at the final level -> exclusive scan over the bucket counts -> rank among the
// elements sharing a bucket), with the very functions the kernels call, compiled for the host.  No bucket-size limit here.
int srl_debug_tr1_order_by_relation(const int16_t *keys_xyz, int n, int32_t *order_out) {
    if (n < 0 || (n > 0 && (!keys_xyz || !order_out))) return SRL_ERR_BAD_ARG;
    if (n == 0) return SRL_OK;
    std::vector<unsigned long long> h((size_t)n);
    for (int i = 0; i < n; i++) h[(size_t)i] = (unsigned long long)std::hash<voxel>()(voxel(keys_xyz[3 * i], keys_xyz[3 * i + 1], keys_xyz[3 * i + 2]));
    SrlTr1Sched S;
    std::memset(&S, 0, sizeof S);
    S.steps = srl::Tr1Order::export_schedule(n, S.first, S.nb, SRL_TR1_MAX_STEPS);
    if (S.steps < 0) return SRL_ERR_UNSUPPORTED;
    const int G = srl_tr1_level(&S, (unsigned)n);
    const unsigned nb = S.nb[G];
    std::vector<std::vector<unsigned>> members(nb);
    for (int e = 0; e < n; e++) members[(size_t)(h[(size_t)e] % nb)].push_back((unsigned)e);
    size_t start = 0;
    for (unsigned b = 0; b < nb; b++) {
        const std::vector<unsigned> &m = members[b];
        for (size_t j = 0; j < m.size(); j++) {
            size_t rank = 0;
            for (size_t i = 0; i < m.size(); i++)
                if (i != j && srl_tr1_before(&S, h.data(), G, m[i], m[j])) ++rank;
            order_out[start + rank] = (int32_t)m[j];
        }
        start += m.size();
    }
    return SRL_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ the camera ESIKF
namespace {
void camera_state_to(const cameraState &c, double *s) {
    s[0] = c.time_td;
    for (int k = 0; k < 9; k++) s[1 + k] = c.R_imu_camera.a[k];
    for (int k = 0; k < 3; k++) { s[10 + k] = c.t_imu_camera[k]; s[21 + k] = c.t_world_camera[k]; s[28 + k] = c.translation[k]; }
    s[13] = c.fx; s[14] = c.fy; s[15] = c.cx; s[16] = c.cy;
    s[17] = c.q_world_camera.w; s[18] = c.q_world_camera.x; s[19] = c.q_world_camera.y; s[20] = c.q_world_camera.z;
    s[24] = c.rotation.w; s[25] = c.rotation.x; s[26] = c.rotation.y; s[27] = c.rotation.z;
}
void camera_state_from(const double *s, cameraState &c) {
    c.time_td = s[0];
    for (int k = 0; k < 9; k++) c.R_imu_camera.a[k] = s[1 + k];
    for (int k = 0; k < 3; k++) { c.t_imu_camera[k] = s[10 + k]; c.t_world_camera[k] = s[21 + k]; c.translation[k] = s[28 + k]; }
    c.fx = s[13]; c.fy = s[14]; c.cx = s[15]; c.cy = s[16];
    c.q_world_camera = srl::Quat(s[17], s[18], s[19], s[20]);
    c.rotation = srl::Quat(s[24], s[25], s[26], s[27]);
}
int vio_update(srl_lio *h, bool photometric, const srl_color_vio_point *tracked, int n, int number_of_new_visited_voxel, int *accepted, int *iterations,
               int *used, double *states, int capacity) {
    if (accepted) *accepted = 0;
    if (iterations) *iterations = 0;
    if (used) *used = 0;
    if (!h || !accepted || n < 0 || (n > 0 && !tracked) || capacity < 0 || (capacity > 0 && !states)) return SRL_ERR_BAD_ARG;
    srl_ctx *ctx = h->lio->context();
    if (!h->vio_provider && !ctx) { h->err = "host-only handle: no device, no measurement pass"; return SRL_ERR_NO_DEVICE; }
    if (h->vio_provider) {
        srl_lio *self = h;
        h->vio.rows = [self](const srl_color_vio_args *a, const srl_color_vio_point *p, int m, srl_color_vio_sums *s) { return self->vio_provider(a, p, m, s, self->vio_user); };
    } else {
        h->vio.rows = [ctx](const srl_color_vio_args *a, const srl_color_vio_point *p, int m, srl_color_vio_sums *s) { return srl_color_map_vio_rows(ctx, a, p, m, s, nullptr, nullptr); };
    }
    const bool ok = photometric ? h->vio.vioPhotometric(h->camera, tracked, n, number_of_new_visited_voxel)
                                : h->vio.vioEsikf(h->camera, tracked, n, number_of_new_visited_voxel);
    if (h->vio.status != SRL_OK) { h->err = "the measurement pass of the camera ESIKF failed"; return h->vio.status; }
    *accepted = ok ? 1 : 0;
    if (iterations) *iterations = (int)h->vio.iterations.size();
    if (used) *used = h->vio.last_used;
    for (int k = 0; k < capacity && k < (int)h->vio.iterations.size(); k++) camera_state_to(h->vio.iterations[k], states + (size_t)k * SRL_LIO_CAMERA_STATE_DOUBLES);
    return SRL_OK;
}
}  // namespace

extern "C" {
int srl_lio_vio_set_options(srl_lio *h, int num_iterations, int estimate_intrinsic, int estimate_extrinsic, const double camera_intrinsic[9],
                            const double R_imu_camera[9], const double t_imu_camera[3]) {
    if (!h || num_iterations < 0) return SRL_ERR_BAD_ARG;
    h->vio.num_iterations = num_iterations;
    h->vio.ifEstimateCameraIntrinsic = estimate_intrinsic != 0;
    h->vio.ifEstimateExtrinsic = estimate_extrinsic != 0;
    if (camera_intrinsic) for (int k = 0; k < 9; k++) h->vio.camera_intrinsic.a[k] = camera_intrinsic[k];
    if (R_imu_camera) for (int k = 0; k < 9; k++) h->vio.R_imu_camera.a[k] = R_imu_camera[k];
    if (t_imu_camera) for (int k = 0; k < 3; k++) h->vio.t_imu_camera[k] = t_imu_camera[k];
    return SRL_OK;
}
int srl_lio_vio_set_camera_state(srl_lio *h, const double *s) { if (!h || !s) return SRL_ERR_BAD_ARG; camera_state_from(s, h->camera); return SRL_OK; }
int srl_lio_vio_get_camera_state(srl_lio *h, double *s) { if (!h || !s) return SRL_ERR_BAD_ARG; camera_state_to(h->camera, s); return SRL_OK; }
int srl_lio_vio_set_initial_cov(srl_lio *h) { if (!h) return SRL_ERR_BAD_ARG; h->vio.setInitialCov(); return SRL_OK; }
int srl_lio_vio_set_cov(srl_lio *h, const double *c) { if (!h || !c) return SRL_ERR_BAD_ARG; for (int k = 0; k < 121; k++) h->vio.covariance.a[k] = c[k]; return SRL_OK; }
int srl_lio_vio_get_cov(srl_lio *h, double *c) { if (!h || !c) return SRL_ERR_BAD_ARG; for (int k = 0; k < 121; k++) c[k] = h->vio.covariance.a[k]; return SRL_OK; }
int srl_lio_vio_set_rows_provider(srl_lio *h, srl_vio_rows_provider fn, void *user) { if (!h) return SRL_ERR_BAD_ARG; h->vio_provider = fn; h->vio_user = user; return SRL_OK; }
int srl_lio_vio_esikf(srl_lio *h, const srl_color_vio_point *tracked, int n, int number_of_new_visited_voxel, int *accepted, int *iterations, int *used,
                      double *states, int capacity) {
    return vio_update(h, false, tracked, n, number_of_new_visited_voxel, accepted, iterations, used, states, capacity);
}
int srl_lio_vio_photometric(srl_lio *h, const srl_color_vio_point *tracked, int n, int number_of_new_visited_voxel, int *accepted, int *iterations, int *used,
                            double *states, int capacity) {
    return vio_update(h, true, tracked, n, number_of_new_visited_voxel, accepted, iterations, used, states, capacity);
}
}  // extern "C"

// ------------------------------------------------------------------ one camera frame end to end (imageProcessing::process)
namespace {
// the handle's step table as imageProcessing::process and the tracker take it: a member the caller gave, or the device call.
// jpeg: the frame comes compressed, so its own prepare step is needed too
int image_install_steps(srl_lio *h, bool jpeg) {
    srl_ctx *ctx = h->lio->context();
    const srl_image_process_steps S = h->image_steps;
    void *user = S.user;
    const bool all = S.prep_create && S.prepare && S.consensus_setup && S.select && S.flow && S.fundamental && S.pnp && (S.rows || h->vio_provider) &&
                     S.render && S.track_update;
    if (!ctx && !(all && (!jpeg || h->jpeg_step))) { h->err = "host-only handle: no device for the steps of imageProcessing::process left at their defaults"; return SRL_ERR_NO_DEVICE; }
    if (!h->oft) h->oft = new srl_oft(ctx);
    opticalFlowTracker &t = h->oft->t;
    lioOptimization *L = h->lio;
    h->vio.op_tracker = &t;
    processSteps &P = h->vio.steps;
    if (S.prep_create) P.prepCreate = [S, user](const srl_image_prep_opts &o) { return S.prep_create(&o, user); };
    else P.prepCreate = [ctx](const srl_image_prep_opts &o) { return srl_image_prep_create(ctx, &o); };
    if (S.prepare) P.prepare = [S, user](const uint8_t *raw, int rows, int cols, int64_t stride, bool resized) { return S.prepare(raw, rows, cols, stride, resized ? 1 : 0, user); };
    else P.prepare = [ctx](const uint8_t *raw, int rows, int cols, int64_t stride, bool resized) {
        return resized ? srl_image_prepare_resized(ctx, raw, rows, cols, stride, nullptr) : srl_image_prepare(ctx, raw, rows, cols, stride, nullptr);
    };
    if (h->jpeg_step) { const srl_image_jpeg_step fn = h->jpeg_step; void *ju = h->jpeg_user; P.prepareJpeg = [fn, ju](const uint8_t *b, int64_t n) { return fn(b, n, ju); }; }
    else if (ctx) P.prepareJpeg = [ctx](const uint8_t *b, int64_t n) { return srl_image_prepare_jpeg(ctx, b, n, nullptr); };
    else P.prepareJpeg = nullptr;
    // The tracker's two consensus providers: the device's estimators on the intrinsics k (useDeviceConsensus installs both), then the
    // caller's on top where the table has them.  ONE function, run behind the consensus setup of the first data and again by every later
    // install, so that a replaced step holds from the first frame on and a member that went back to NULL gets the device call back.
    // (pnp_is_device: a failing step ends the frame with its status, it is not the cv::Exception the reference catches)
    const auto consensus_providers = [S, user, &t](const double *k) {
        if (!(S.fundamental && S.pnp)) { const int rc = t.useDeviceConsensus(k, nullptr, nullptr); if (rc != SRL_OK) return rc; }
        if (S.fundamental) t.fundamental = [S, user](const float *l, const float *c, int n, uint8_t *st) { return S.fundamental(l, c, n, st, user); };
        if (S.pnp) { t.pnp = [S, user](const float *xyz, const float *uv, int n, int32_t *in, int *nin) { return S.pnp(xyz, uv, n, in, nin, user); }; t.pnp_is_device = true; }
        return (int)SRL_OK;
    };
    P.consensusSetup = [S, user, consensus_providers](const double *k) {
        if (S.consensus_setup) { const int rc = S.consensus_setup(k, user); if (rc != SRL_OK) return rc; }
        return consensus_providers(k);
    };
    if (h->vio.first_data_stage >= 2) {
        const double k[4] = {h->vio.camera_intrinsic(0, 0), h->vio.camera_intrinsic(1, 1), h->vio.camera_intrinsic(0, 2), h->vio.camera_intrinsic(1, 2)};
        const int rc = consensus_providers(k);
        if (rc != SRL_OK) return rc;
    }
    if (S.select)
        P.select = [S, user](const srl_color_camera &cam, int rows, int cols, const srl_color_select_opts &o, bool refresh, std::vector<srl_color_selected> &out) {
            out.resize(4096);
            int n = 0;
            int rc = S.select(&cam, rows, cols, &o, refresh ? 1 : 0, out.data(), (int)out.size(), &n, user);
            if (rc == SRL_ERR_BAD_ARG && n > (int)out.size()) {
                out.resize((size_t)n);
                rc = S.select(&cam, rows, cols, &o, refresh ? 1 : 0, out.data(), (int)out.size(), &n, user);
            }
            if (rc == SRL_OK && (n < 0 || n > (int)out.size())) rc = SRL_ERR_BAD_ARG;
            out.resize(rc == SRL_OK ? (size_t)n : 0);
            return rc;
        };
    else
        P.select = [h, L](const srl_color_camera &cam, int rows, int cols, const srl_color_select_opts &o, bool refresh, std::vector<srl_color_selected> &out) {
            L->minimum_depth_for_projection = o.minimum_depth; L->maximum_depth_for_projection = o.maximum_depth;
            try {
                out = L->selectPointsForProjection(cam, rows, cols, o.minimum_dis, o.skip_step, o.use_all_points != 0);
                if (refresh) L->points_for_projection = out;
            } catch (const std::exception &e) { return status_from_exception(h, e); }
            return (int)SRL_OK;
        };
    if (S.render) P.render = [S, user](const srl_color_camera &cam, double obs_time, srl_color_render_totals &tot) { return S.render(&cam, obs_time, &tot, user); };
    else
        P.render = [h, L](const srl_color_camera &cam, double obs_time, srl_color_render_totals &tot) {
            try { L->renderPointsInRecentVoxel(cam, obs_time); } catch (const std::exception &e) { return status_from_exception(h, e); }
            tot = L->render_totals;
            return (int)SRL_OK;
        };
    // the tracker's providers
    if (S.flow) {
        t.flow = [S, user](const uint8_t *g, int r, int c, int64_t s, const float *p, int n, float *x, uint8_t *st) { return S.flow(g, r, c, s, p, n, x, st, user); };
        t.use_prepared_image = true;                                       // a NULL gray is the prepared image, not the empty one
    } else {
        t.flow = nullptr;
        const int rc = t.usePreparedImage(true);
        if (rc != SRL_OK) return rc;
    }
    if (S.track_update)
        t.update = [S, user](const srl_color_camera *cam, int r, int c, const srl_color_track_point *tr, int n, const int32_t *cand, int nc,
                             const srl_color_track_opts *o, srl_color_track_point *out, int64_t cap, srl_color_track_totals *tot) {
            return S.track_update(cam, r, c, tr, n, cand, nc, o, out, cap, tot, user);
        };
    else t.update = nullptr;
    if (S.rows) h->vio.rows = [S, user](const srl_color_vio_args *a, const srl_color_vio_point *p, int m, srl_color_vio_sums *s) { return S.rows(a, p, m, s, user); };
    else if (h->vio_provider) {
        srl_lio *self = h;
        h->vio.rows = [self](const srl_color_vio_args *a, const srl_color_vio_point *p, int m, srl_color_vio_sums *s) { return self->vio_provider(a, p, m, s, self->vio_user); };
    } else h->vio.rows = [ctx](const srl_color_vio_args *a, const srl_color_vio_point *p, int m, srl_color_vio_sums *s) { return srl_color_map_vio_rows(ctx, a, p, m, s, nullptr, nullptr); };
    return SRL_OK;
}
}  // namespace

extern "C" {
void srl_image_process_opts_default(srl_image_process_opts *o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->image_resize_ratio = 1.0; o->track_windows_size = 40; o->maximum_tracked_points = 300;      // imageProcessing.cpp:11-18
    o->tracker_minimum_depth = 0.1; o->tracker_maximum_depth = 200;
}
int srl_lio_image_set_options(srl_lio *h, const srl_image_process_opts *o) {
    if (!h || !o || o->image_width < 1 || o->image_height < 1 || !(o->image_resize_ratio > 0.0) || !(o->track_windows_size > 0.0)) return SRL_ERR_BAD_ARG;
    imageProcessing &v = h->vio;
    v.image_width = o->image_width; v.image_height = o->image_height; v.image_resize_ratio = o->image_resize_ratio;
    for (int k = 0; k < 5; k++) v.camera_dist_coeffs[k] = o->dist[k];
    v.track_windows_size = o->track_windows_size; v.maximum_tracked_points = o->maximum_tracked_points;
    v.tracker_minimum_depth = o->tracker_minimum_depth; v.tracker_maximum_depth = o->tracker_maximum_depth;
    h->image_options_set = true;
    return SRL_OK;
}
int srl_lio_image_set_steps(srl_lio *h, const srl_image_process_steps *steps) {
    if (!h) return SRL_ERR_BAD_ARG;
    if (steps) h->image_steps = *steps; else h->image_steps = srl_image_process_steps();
    return SRL_OK;
}
}  // extern "C"

namespace {
// srl_lio_image_process and srl_lio_image_process_jpeg behind their argument checks: f holds the image, raw or compressed, and its size
int image_process_frame(srl_lio *h, imageFrame f, double time_sweep_end, int frame_id, srl_image_process_result *out) {
    if (!h->image_options_set) { h->err = "srl_lio_image_process: no options (srl_lio_image_set_options)"; return SRL_ERR_BAD_ARG; }
    { const int rc = image_install_steps(h, f.jpeg != nullptr); if (rc != SRL_OK) return rc; }
    f.time_sweep_end = time_sweep_end; f.frame_id = frame_id;
    int rc;
    try { rc = h->vio.process(h->camera, f, h->lio->number_of_new_visited_voxel, out); }
    catch (const std::exception &e) { return status_from_exception(h, e); }
    if (rc == SRL_OK) h->lio->time_last_process = h->vio.time_last_process;      // what the next colour insertion reads; a frame that did not finish moves nothing
    if (rc != SRL_OK && h->lio->context()) { const char *m = srl_last_error(h->lio->context()); if (m && *m) h->err = m; }
    return rc;
}
// a compressed frame: its size from the stream's header alone (no device)
int jpeg_frame(srl_lio *h, const uint8_t *bytes, int64_t n, imageFrame *f) {
    srl_jpeg_info ji;
    const int rc = srl_jpeg_parse(bytes, n, &ji);
    if (rc != SRL_OK) { h->err = rc == SRL_ERR_UNSUPPORTED ? "JPEG: outside what srl_jpeg_parse accepts" : "JPEG: malformed header"; return rc; }
    f->jpeg = bytes; f->jpeg_bytes = n; f->image_rows = ji.rows; f->image_cols = ji.cols;
    return SRL_OK;
}
}  // namespace

extern "C" {
int srl_lio_image_process(srl_lio *h, const uint8_t *raw_bgr, int rows, int cols, int64_t row_stride_bytes, double time_sweep_end, int frame_id,
                          srl_image_process_result *out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (!h || !raw_bgr || rows < 1 || cols < 1 || row_stride_bytes < (int64_t)cols * 3) return SRL_ERR_BAD_ARG;
    imageFrame f;
    f.rgb_image = raw_bgr; f.image_rows = rows; f.image_cols = cols; f.row_stride_bytes = row_stride_bytes;
    return image_process_frame(h, f, time_sweep_end, frame_id, out);
}
int srl_lio_image_set_jpeg_step(srl_lio *h, srl_image_jpeg_step fn, void *user) {
    if (!h) return SRL_ERR_BAD_ARG;
    h->jpeg_step = fn; h->jpeg_user = fn ? user : nullptr;
    return SRL_OK;
}
int srl_lio_image_process_jpeg(srl_lio *h, const uint8_t *bytes, int64_t n, double time_sweep_end, int frame_id, srl_image_process_result *out) {
    if (out) std::memset(out, 0, sizeof *out);
    if (!h || !bytes || n < 2) return SRL_ERR_BAD_ARG;
    if (!h->image_options_set) { h->err = "srl_lio_image_process_jpeg: no options (srl_lio_image_set_options)"; return SRL_ERR_BAD_ARG; }
    imageFrame f;
    { const int rc = jpeg_frame(h, bytes, n, &f); if (rc != SRL_OK) return rc; }
    return image_process_frame(h, f, time_sweep_end, frame_id, out);
}
srl_oft *srl_lio_image_oft(srl_lio *h) {
    if (!h) return nullptr;
    if (!h->oft) h->oft = new srl_oft(h->lio->context());
    return h->oft;
}
int srl_lio_image_candidates(srl_lio *h, srl_color_selected *out, int capacity, int *n) {
    if (n) *n = 0;
    if (!h || !n || capacity < 0 || (capacity > 0 && !out)) return SRL_ERR_BAD_ARG;
    const std::vector<srl_color_selected> &c = h->vio.points_for_projection;
    *n = (int)c.size();
    if ((int)c.size() > capacity) return capacity == 0 ? SRL_OK : SRL_ERR_BAD_ARG;
    if (!c.empty()) std::memcpy(out, c.data(), c.size() * sizeof(srl_color_selected));
    return SRL_OK;
}
}  // extern "C"

namespace {
// srl_lio_run_measurement_image and its _jpeg twin behind their argument checks: `frame` holds the image, raw or compressed, and its size
int run_measurement_frame(srl_lio *h, double time_frame, const double *imu_t, const double *imu_acc, const double *imu_gyr, int n_imu,
                          const double *pts_raw, const double *pts_timestamp, int n_pts, double time_sweep_begin, double time_sweep_offset,
                          const imageFrame &frame, srl_replay_result *out, srl_image_process_result *image_out) {
    if (!h->image_options_set) { h->err = "srl_lio_run_measurement_image: no options (srl_lio_image_set_options)"; return SRL_ERR_BAD_ARG; }
    { const int rc = image_install_steps(h, frame.jpeg != nullptr); if (rc != SRL_OK) return rc; }
    lioOptimization &L = *h->lio;
    int image_rc = SRL_OK;
    std::string image_err;
    L.camera_half = [&](cloudFrame *p_frame) {
        cameraState &c = h->camera;
        if (L.all_cloud_frame.size() < 3) {               // :1053-1061
            c.fx = h->vio.camera_intrinsic(0, 0); c.fy = h->vio.camera_intrinsic(1, 1);
            c.cx = h->vio.camera_intrinsic(0, 2); c.cy = h->vio.camera_intrinsic(1, 2);
            c.R_imu_camera = h->vio.R_imu_camera; c.t_imu_camera = h->vio.t_imu_camera;
        }                                                 // :1062-1071: else the frame's before, which the handle's camera state still holds
        c.rotation = p_frame->p_state->rotation; c.translation = p_frame->p_state->translation;
        c.q_world_camera = srl::Quat::fromRotationMatrix(c.rotation.toRotationMatrix() * c.R_imu_camera);      // :1073-1074
        c.t_world_camera = c.rotation.toRotationMatrix() * c.t_imu_camera + c.translation;
        imageFrame f = frame;                             // :1077-1083
        f.time_sweep_end = p_frame->time_sweep_end; f.frame_id = p_frame->frame_id;
        try { image_rc = h->vio.process(c, f, L.number_of_new_visited_voxel, image_out); }
        catch (const std::exception &e) { image_rc = SRL_ERR_HIP; image_err = e.what(); }
        if (image_rc == SRL_OK) L.time_last_process = h->vio.time_last_process;
    };
    const bool rendering_before = L.to_rendering;
    L.to_rendering = true;
    const int rc = srl_lio_run_measurement(h, time_frame, imu_t, imu_acc, imu_gyr, n_imu, pts_raw, pts_timestamp, n_pts, time_sweep_begin, time_sweep_offset, out);
    L.to_rendering = rendering_before;
    L.camera_half = nullptr;
    if (rc != SRL_OK) return rc;
    if (image_rc != SRL_OK) {
        const char *m = L.context() ? srl_last_error(L.context()) : "";
        h->err = !image_err.empty() ? image_err : (m && *m ? m : "the camera frame of srl_lio_run_measurement_image failed");
    }
    return image_rc;
}
}  // namespace

extern "C" {
int srl_lio_run_measurement_image(srl_lio *h, double time_frame, const double *imu_t, const double *imu_acc, const double *imu_gyr, int n_imu,
                                  const double *pts_raw, const double *pts_timestamp, int n_pts, double time_sweep_begin, double time_sweep_offset,
                                  const uint8_t *raw_bgr, int rows, int cols, int64_t row_stride_bytes, srl_replay_result *out,
                                  srl_image_process_result *image_out) {
    if (image_out) std::memset(image_out, 0, sizeof *image_out);
    if (!raw_bgr) return srl_lio_run_measurement(h, time_frame, imu_t, imu_acc, imu_gyr, n_imu, pts_raw, pts_timestamp, n_pts, time_sweep_begin, time_sweep_offset, out);
    if (out) std::memset(out, 0, sizeof *out);
    if (!h || rows < 1 || cols < 1 || row_stride_bytes < (int64_t)cols * 3) return SRL_ERR_BAD_ARG;
    imageFrame f;
    f.rgb_image = raw_bgr; f.image_rows = rows; f.image_cols = cols; f.row_stride_bytes = row_stride_bytes;
    return run_measurement_frame(h, time_frame, imu_t, imu_acc, imu_gyr, n_imu, pts_raw, pts_timestamp, n_pts, time_sweep_begin, time_sweep_offset, f, out, image_out);
}
int srl_lio_run_measurement_image_jpeg(srl_lio *h, double time_frame, const double *imu_t, const double *imu_acc, const double *imu_gyr, int n_imu,
                                       const double *pts_raw, const double *pts_timestamp, int n_pts, double time_sweep_begin, double time_sweep_offset,
                                       const uint8_t *bytes, int64_t n, srl_replay_result *out, srl_image_process_result *image_out) {
    if (image_out) std::memset(image_out, 0, sizeof *image_out);
    if (!bytes) return srl_lio_run_measurement(h, time_frame, imu_t, imu_acc, imu_gyr, n_imu, pts_raw, pts_timestamp, n_pts, time_sweep_begin, time_sweep_offset, out);
    if (out) std::memset(out, 0, sizeof *out);
    if (!h || n < 2) return SRL_ERR_BAD_ARG;
    if (!h->image_options_set) { h->err = "srl_lio_run_measurement_image_jpeg: no options (srl_lio_image_set_options)"; return SRL_ERR_BAD_ARG; }
    imageFrame f;
    { const int rc = jpeg_frame(h, bytes, n, &f); if (rc != SRL_OK) return rc; }
    return run_measurement_frame(h, time_frame, imu_t, imu_acc, imu_gyr, n_imu, pts_raw, pts_timestamp, n_pts, time_sweep_begin, time_sweep_offset, f, out, image_out);
}
int srl_lio_image_time_last_process(srl_lio *h, double *time_last_process) {
    if (!h || !time_last_process) return SRL_ERR_BAD_ARG;
    *time_last_process = h->lio->time_last_process;
    return SRL_OK;
}
}  // extern "C"

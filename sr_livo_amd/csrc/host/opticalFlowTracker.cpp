// opticalFlowTracker.cpp (host mirror) -- see opticalFlowTracker.h.  The C handle of include/srlivo_host.h (srl_oft_*) is at the end;
// useDeviceConsensus and its two C functions are opticalFlowTrackerDevice.cpp.
#include "opticalFlowTracker.h"
#include "../../../include/srlivo_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

namespace srlivo {

namespace {
// reduce_vector (include/utility.h): the elements whose status is set, in order
template <class T>
void reduce_vector(std::vector<T> &v, const std::vector<uint8_t> &status) {
    size_t j = 0;
    for (size_t i = 0; i < v.size(); i++)
        if (status[i]) v[j++] = v[i];
    v.resize(j);
}
// cloudFrame::if2dPointsAvailable(u, v, scale, fov_mar) with fov_mar > 0 (lioOptimization.cpp:48-60)
bool if2dPointsAvailable(double u, double v, double scale, double fov_mar, int image_rows, int image_cols) {
    const double used_fov_margin = fov_mar;
    return (u / scale >= (used_fov_margin * image_cols + 1)) && (std::ceil(u / scale) < ((1 - used_fov_margin) * image_cols)) &&
           (v / scale >= (used_fov_margin * image_rows + 1)) && (std::ceil(v / scale) < ((1 - used_fov_margin) * image_rows));
}
}  // namespace

opticalFlowTracker::opticalFlowTracker(srl_ctx *ctx_) : ctx(ctx_) {
    TermCriteria criteria;                                                  // :5-8
    criteria.type = TermCriteria::COUNT + TermCriteria::EPS; criteria.maxCount = 10; criteria.epsilon = 0.05;
    lk_optical_flow_kernel.reset(new LKOpticalFlowKernel(ctx, Size{21, 21}, 3, criteria, 8 /* cv_OPTFLOW_LK_GET_MIN_EIGENVALS */));
    maximum_tracked_points = 300;
}

int opticalFlowTracker::flowCall(const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, const std::vector<Point2f> &last, std::vector<Point2f> &cur,
                                 std::vector<uint8_t> &st) {
    const int n = (int)last.size();
    if (flow) {
        cur.assign(last.size(), Point2f());
        st.assign(last.size(), 1);
        return flow(gray, rows, cols, row_stride_bytes, n ? &last[0].x : nullptr, n, n ? &cur[0].x : nullptr, n ? st.data() : nullptr);
    }
    st.assign(last.size(), 1);                                              // (the tracker's first image leaves the status untouched)
    return lk_optical_flow_kernel->trackImage(gray, rows, cols, row_stride_bytes, last, cur, st) < 0 ? lk_optical_flow_kernel->last_status : SRL_OK;
}

void opticalFlowTracker::updateLastTrackingVectorAndIds() {
    int idx = 0;
    last_tracked_points.clear();
    rgb_points_ptr_vec_in_last_image.clear();
    old_ids.clear();
    for (auto it = map_rgb_points_in_last_image_pose.begin(); it != map_rgb_points_in_last_image_pose.end(); it++) {      // ascending pool position
        rgb_points_ptr_vec_in_last_image.push_back(it->first);
        last_tracked_points.push_back(it->second);
        old_ids.push_back(idx);
        idx++;
    }
}

void opticalFlowTracker::setTrackPoints(const srl_color_selected *records, int n) {
    map_rgb_points_in_last_image_pose.clear();
    for (int i = 0; i < n; i++) {
        map_rgb_points_in_last_image_pose[records[i].pool] = Point2f{records[i].u, records[i].v};
        position[records[i].pool] = {records[i].x, records[i].y, records[i].z};
    }
    updateLastTrackingVectorAndIds();
}

bool opticalFlowTracker::init(const srl_color_selected *records, int n, const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, double time_sweep_end) {
    setTrackPoints(records, n);
    current_image_time = time_sweep_end;
    last_image_time = current_image_time;
    std::vector<uint8_t> st;
    status = flowCall(gray, rows, cols, row_stride_bytes, last_tracked_points, cur_tracked_points, st);
    return status == SRL_OK;
}

bool opticalFlowTracker::trackImage(const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, double time_sweep_end, int image_rows, int image_cols) {
    status = SRL_OK;
    current_image_time = time_sweep_end;
    map_rgb_points_in_cur_image_pose.clear();
    if (!gray && !use_prepared_image) return true;                          // cur_image.empty()

    std::vector<uint8_t> st;
    cur_tracked_points = last_tracked_points;
    if (last_tracked_points.size() < 30) {
        last_image_time = current_image_time;
        return true;
    }
    if (!fundamental) { status = SRL_ERR_BAD_ARG; return false; }           // the caller's cv::findFundamentalMat: there is none to default to

    status = flowCall(gray, rows, cols, row_stride_bytes, last_tracked_points, cur_tracked_points, st);
    if (status != SRL_OK) return false;
    reduce_vector(last_tracked_points, st);
    reduce_vector(old_ids, st);
    reduce_vector(cur_tracked_points, st);

    const int n = (int)last_tracked_points.size();
    st.assign((size_t)n, 0);
    status = fundamental(n ? &last_tracked_points[0].x : nullptr, n ? &cur_tracked_points[0].x : nullptr, n, n ? st.data() : nullptr);
    if (status != SRL_OK) return false;
    reduce_vector(last_tracked_points, st);
    reduce_vector(old_ids, st);
    reduce_vector(cur_tracked_points, st);

    map_rgb_points_in_cur_image_pose.clear();
    const double frame_time_diff = (current_image_time - last_image_time);
    for (unsigned i = 0; i < last_tracked_points.size(); i++) {
        if (if2dPointsAvailable(cur_tracked_points[i].x, cur_tracked_points[i].y, 1.0, 0.05, image_rows, image_cols)) {
            const int32_t rgb_point = rgb_points_ptr_vec_in_last_image[old_ids[i]];
            map_rgb_points_in_cur_image_pose[rgb_point] = cur_tracked_points[i];
            Point2f point_image_velocity;
            if (frame_time_diff < 1e-5) {
                point_image_velocity = Point2f{(float)1e-3, (float)1e-3};
            } else {
                // cv::Point2f - cv::Point2f in float, then Point_<float> / double: a double quotient rounded to float (see the header)
                const Point2f d{cur_tracked_points[i].x - last_tracked_points[i].x, cur_tracked_points[i].y - last_tracked_points[i].y};
                point_image_velocity = Point2f{(float)((double)d.x / frame_time_diff), (float)((double)d.y / frame_time_diff)};
            }
            image_velocity[rgb_point] = {(double)point_image_velocity.x, (double)point_image_velocity.y};
        }
    }
    // (rejectErrorTrackingPoints: not built, see the header)
    last_tracked_points = cur_tracked_points;
    updateLastTrackingVectorAndIds();
    image_idx++;
    last_image_time = current_image_time;
    return true;
}

bool opticalFlowTracker::removeOutlierUsingRansacPnp(int if_remove_ourlier, bool *accepted) {
    status = SRL_OK;
    *accepted = false;
    std::vector<float> points_3d, points_2d;
    std::vector<int32_t> map_ptr;
    for (auto it = map_rgb_points_in_cur_image_pose.begin(); it != map_rgb_points_in_cur_image_pose.end(); it++) {      // ascending pool position
        map_ptr.push_back(it->first);
        const std::array<float, 3> &p = position[it->first];               // cv::Point3f of getPosition(): the stored floats
        points_3d.insert(points_3d.end(), {p[0], p[1], p[2]});
        points_2d.insert(points_2d.end(), {it->second.x, it->second.y});
    }
    if (map_ptr.size() < 10) return true;
    if (!pnp) { status = SRL_ERR_BAD_ARG; return false; }                   // the caller's cv::solvePnPRansac
    const int n = (int)map_ptr.size();
    std::vector<int32_t> inliers((size_t)n);
    int n_inliers = 0;
    {
        const int rc = pnp(points_3d.data(), points_2d.data(), n, inliers.data(), &n_inliers);
        if (rc != SRL_OK && pnp_is_device) { status = rc; return false; }  // the device's estimator throws nothing: its failure is the handle's
        if (rc != SRL_OK) return true;                                      // the caught cv::Exception: return 0
    }
    if (n_inliers < 0 || n_inliers > n) { status = SRL_ERR_BAD_ARG; return false; }
    for (int i = 0; i < n_inliers; i++)
        if (inliers[i] < 0 || inliers[i] >= n) { status = SRL_ERR_BAD_ARG; return false; }
    if (if_remove_ourlier) {
        map_rgb_points_in_last_image_pose.clear();
        map_rgb_points_in_cur_image_pose.clear();
        for (int i = 0; i < n_inliers; i++) {
            const int inlier_idx = inliers[i];
            const Point2f uv{points_2d[(size_t)inlier_idx * 2], points_2d[(size_t)inlier_idx * 2 + 1]};
            map_rgb_points_in_last_image_pose[map_ptr[inlier_idx]] = uv;
            map_rgb_points_in_cur_image_pose[map_ptr[inlier_idx]] = uv;
        }
    }
    updateLastTrackingVectorAndIds();
    *accepted = true;
    return true;
}

bool opticalFlowTracker::updateAndAppendTrackPoints(const srl_color_camera *cam, int image_rows, int image_cols, const srl_color_selected *candidates,
                                                    int n_candidates, double mini_distance) {
    std::vector<srl_color_track_point> tracked;
    for (const auto &e : map_rgb_points_in_last_image_pose)
        tracked.push_back(srl_color_track_point{e.first, e.second.x, e.second.y, out_lier_flagged.count(e.first) ? 1 : 0});
    std::vector<int32_t> cand((size_t)std::max(n_candidates, 0));
    for (int i = 0; i < n_candidates; i++) cand[i] = candidates[i].pool;
    srl_color_track_opts o;
    o.mini_distance = mini_distance; o.maximum_tracked_points = maximum_tracked_points; o.reserved = 0;
    const int n = (int)tracked.size();
    std::vector<srl_color_track_point> out(tracked.size() + (size_t)std::min<long long>(std::max(n_candidates, 0), std::max(maximum_tracked_points, 1)));
    update_totals = srl_color_track_totals();
    if (update)
        status = update(cam, image_rows, image_cols, n ? tracked.data() : nullptr, n, n_candidates > 0 ? cand.data() : nullptr, n_candidates, &o,
                        out.empty() ? nullptr : out.data(), (int64_t)out.size(), &update_totals);
    else
        status = srl_color_map_track_update(ctx, cam, image_rows, image_cols, n ? tracked.data() : nullptr, n, n_candidates > 0 ? cand.data() : nullptr,
                                            n_candidates, &o, out.empty() ? nullptr : out.data(), (int64_t)out.size(), nullptr, nullptr, &update_totals);
    if (status != SRL_OK) return false;
    const int64_t kept = update_totals.kept, added = update_totals.added;
    if (kept < 0 || added < 0 || kept + added > (int64_t)out.size()) { status = SRL_ERR_BAD_ARG; return false; }
    // the first loop left every tracked point's count at 0 unless it kept the point flagged
    for (const auto &t : tracked) out_lier_flagged.erase(t.pool);
    map_rgb_points_in_last_image_pose.clear();
    for (int64_t k = 0; k < kept; k++) {
        map_rgb_points_in_last_image_pose[out[k].pool] = Point2f{out[k].u, out[k].v};
        if (out[k].flagged) out_lier_flagged.insert(out[k].pool);
    }
    // an added point's count is what its rgbPoint held: 1 if it left the set flagged (out_lier_flagged still names it)
    std::map<int32_t, int> where;
    for (int i = n_candidates - 1; i >= 0; i--) where[candidates[i].pool] = i;
    for (int64_t k = kept; k < kept + added; k++) {
        map_rgb_points_in_last_image_pose[out[k].pool] = Point2f{out[k].u, out[k].v};
        const auto w = where.find(out[k].pool);
        if (w != where.end()) position[out[k].pool] = {candidates[w->second].x, candidates[w->second].y, candidates[w->second].z};
    }
    updateLastTrackingVectorAndIds();
    return true;
}

std::vector<srl_color_vio_point> opticalFlowTracker::trackedForVio() const {
    std::vector<srl_color_vio_point> out;
    for (const auto &e : map_rgb_points_in_last_image_pose) {
        srl_color_vio_point p;
        p.pool = e.first; p.pad = 0;
        p.match_u = (double)e.second.x; p.match_v = (double)e.second.y;
        const auto v = image_velocity.find(e.first);
        p.vel_u = v == image_velocity.end() ? 0.0 : v->second[0];
        p.vel_v = v == image_velocity.end() ? 0.0 : v->second[1];
        out.push_back(p);
    }
    return out;
}

}  // namespace srlivo

extern "C" {
int srl_oft_create(srl_ctx *ctx, srl_oft **out) {
    if (!out) return SRL_ERR_BAD_ARG;
    *out = new (std::nothrow) srl_oft(ctx);
    return *out ? SRL_OK : SRL_ERR_BAD_ARG;
}
int srl_oft_destroy(srl_oft *h) { delete h; return SRL_OK; }
int srl_oft_set_maximum_tracked_points(srl_oft *h, int maximum_tracked_points) {
    if (!h) return SRL_ERR_BAD_ARG;
    h->t.maximum_tracked_points = maximum_tracked_points;
    return SRL_OK;
}
int srl_oft_set_flow_provider(srl_oft *h, srl_oft_flow_provider fn, void *user) {
    if (!h) return SRL_ERR_BAD_ARG;
    if (fn) h->t.flow = [fn, user](const uint8_t *g, int r, int c, int64_t s, const float *p, int n, float *x, uint8_t *st) { return fn(g, r, c, s, p, n, x, st, user); };
    else h->t.flow = nullptr;
    return SRL_OK;
}
int srl_oft_set_fundamental_provider(srl_oft *h, srl_oft_fundamental_provider fn, void *user) {
    if (!h) return SRL_ERR_BAD_ARG;
    if (fn) h->t.fundamental = [fn, user](const float *l, const float *c, int n, uint8_t *st) { return fn(l, c, n, st, user); };
    else h->t.fundamental = nullptr;
    return SRL_OK;
}
int srl_oft_set_pnp_provider(srl_oft *h, srl_oft_pnp_provider fn, void *user) {
    if (!h) return SRL_ERR_BAD_ARG;
    if (fn) h->t.pnp = [fn, user](const float *xyz, const float *uv, int n, int32_t *in, int *nin) { return fn(xyz, uv, n, in, nin, user); };
    else h->t.pnp = nullptr;
    h->t.pnp_is_device = false;
    return SRL_OK;
}
int srl_oft_set_update_provider(srl_oft *h, srl_oft_update_provider fn, void *user) {
    if (!h) return SRL_ERR_BAD_ARG;
    if (fn)
        h->t.update = [fn, user](const srl_color_camera *cam, int r, int c, const srl_color_track_point *t, int n, const int32_t *cand, int nc,
                                 const srl_color_track_opts *o, srl_color_track_point *out, int64_t cap, srl_color_track_totals *tot) {
            return fn(cam, r, c, t, n, cand, nc, o, out, cap, tot, user);
        };
    else h->t.update = nullptr;
    return SRL_OK;
}
int srl_oft_set_track_points(srl_oft *h, const srl_color_selected *records, int n) {
    if (!h || n < 0 || (n > 0 && !records)) return SRL_ERR_BAD_ARG;
    h->t.setTrackPoints(records, n);
    return SRL_OK;
}
int srl_oft_init(srl_oft *h, const srl_color_selected *records, int n, const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, double time_sweep_end) {
    if (!h || n < 0 || (n > 0 && !records)) return SRL_ERR_BAD_ARG;
    return h->t.init(records, n, gray, rows, cols, row_stride_bytes, time_sweep_end) ? SRL_OK : h->t.status;
}
int srl_oft_track_image(srl_oft *h, const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, double time_sweep_end, int image_rows, int image_cols,
                        int *n_cur) {
    if (n_cur) *n_cur = 0;
    if (!h) return SRL_ERR_BAD_ARG;
    if (!h->t.trackImage(gray, rows, cols, row_stride_bytes, time_sweep_end, image_rows, image_cols)) return h->t.status;
    if (n_cur) *n_cur = (int)h->t.map_rgb_points_in_cur_image_pose.size();
    return SRL_OK;
}
int srl_oft_remove_outlier_using_ransac_pnp(srl_oft *h, int if_remove_outlier, int *accepted) {
    if (accepted) *accepted = 0;
    if (!h || !accepted) return SRL_ERR_BAD_ARG;
    bool ok = false;
    if (!h->t.removeOutlierUsingRansacPnp(if_remove_outlier, &ok)) return h->t.status;
    *accepted = ok ? 1 : 0;
    return SRL_OK;
}
int srl_oft_update_and_append_track_points(srl_oft *h, const srl_color_camera *cam, int image_rows, int image_cols, const srl_color_selected *candidates,
                                           int n_candidates, double mini_distance, srl_color_track_totals *totals) {
    if (totals) std::memset(totals, 0, sizeof *totals);
    if (!h || !cam || n_candidates < 0 || (n_candidates > 0 && !candidates)) return SRL_ERR_BAD_ARG;
    const bool ok = h->t.updateAndAppendTrackPoints(cam, image_rows, image_cols, candidates, n_candidates, mini_distance);
    if (totals) *totals = h->t.update_totals;
    return ok ? SRL_OK : h->t.status;
}
int srl_oft_sizes(srl_oft *h, int *last_pose, int *cur_pose, int *last_tracked, int *flagged) {
    if (!h) return SRL_ERR_BAD_ARG;
    if (last_pose) *last_pose = (int)h->t.map_rgb_points_in_last_image_pose.size();
    if (cur_pose) *cur_pose = (int)h->t.map_rgb_points_in_cur_image_pose.size();
    if (last_tracked) *last_tracked = (int)h->t.last_tracked_points.size();
    if (flagged) *flagged = (int)h->t.out_lier_flagged.size();
    return SRL_OK;
}
int srl_oft_times(srl_oft *h, double *last_image_time, double *current_image_time) {
    if (!h) return SRL_ERR_BAD_ARG;
    if (last_image_time) *last_image_time = h->t.last_image_time;
    if (current_image_time) *current_image_time = h->t.current_image_time;
    return SRL_OK;
}
int srl_oft_pose_map(srl_oft *h, int which, srl_color_track_point *out, int capacity, int *n) {
    if (n) *n = 0;
    if (!h || !n || capacity < 0 || (which != 0 && which != 1)) return SRL_ERR_BAD_ARG;
    const auto &m = which ? h->t.map_rgb_points_in_cur_image_pose : h->t.map_rgb_points_in_last_image_pose;
    *n = (int)m.size();
    if (!out) return SRL_OK;
    if ((size_t)capacity < m.size()) return SRL_ERR_BAD_ARG;
    int k = 0;
    for (const auto &e : m) out[k++] = srl_color_track_point{e.first, e.second.x, e.second.y, h->t.out_lier_flagged.count(e.first) ? 1 : 0};
    return SRL_OK;
}
int srl_oft_tracked_for_vio(srl_oft *h, srl_color_vio_point *out, int capacity, int *n) {
    if (n) *n = 0;
    if (!h || !n || capacity < 0) return SRL_ERR_BAD_ARG;
    const std::vector<srl_color_vio_point> v = h->t.trackedForVio();
    *n = (int)v.size();
    if (!out) return SRL_OK;
    if ((size_t)capacity < v.size()) return SRL_ERR_BAD_ARG;
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(srl_color_vio_point));
    return SRL_OK;
}
}

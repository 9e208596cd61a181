// track_host_san_main.cpp -- a stand-alone program over the host mirror's opticalFlowTracker (sr_livo_amd/csrc/host/opticalFlowTracker.cpp),
// built with -fsanitize=address,undefined by tests/test_track_host_san.py: the C handle's argument handling, the vectors that shrink and
// grow through trackImage, the PnP rebuild and the buffers handed to srl_color_map_track_update.  It makes no device call: the srl_flow_*
// entry points the mirror's LKOpticalFlowKernel uses and srl_color_map_track_update are stand-ins defined here.
#include "../sr_livo_amd/csrc/host/opticalFlowTracker.h"
#include "../include/srlivo_hip_debug.h"
#include "../include/srlivo_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static int g_first = 1, g_updates = 0, g_last_n = -1, g_last_nc = -1, g_flagged_in = 0;
static long long g_last_capacity = -1;

extern "C" {
void srl_flow_opts_default(srl_flow_opts *o) { o->win = 21; o->max_level = 3; o->max_count = 10; o->reserved = 0; o->epsilon = 0.05; o->min_eig_threshold = 1e-4; }
int srl_flow_create(srl_ctx *, const srl_flow_opts *) { g_first = 1; return SRL_OK; }
int srl_flow_destroy(srl_ctx *) { return SRL_OK; }
int srl_flow_levels(srl_ctx *, int *L) { *L = 3; return SRL_OK; }
// the first image is only stored; afterwards every point moves by (2, 1) and every third is lost
int srl_flow_track_image(srl_ctx *, const uint8_t *gray, int rows, int cols, int64_t stride, const float *prev, int n, float *next, uint8_t *status, int *n_tracked) {
    *n_tracked = 0;
    if (!gray || rows < 2 || cols < 2 || stride < cols) return SRL_ERR_BAD_ARG;
    if (g_first) { g_first = 0; if (n) std::memcpy(next, prev, (size_t)n * 2 * sizeof(float)); return SRL_OK; }
    for (int i = 0; i < n; i++) { next[2 * i] = prev[2 * i] + 2.f; next[2 * i + 1] = prev[2 * i + 1] + 1.f; status[i] = (uint8_t)(i % 3 != 0); *n_tracked += status[i]; }
    return SRL_OK;
}
// keeps every tracked point but the first, the second flagged; adds as many candidates as the capacity and the maximum allow
int srl_color_map_track_update(srl_ctx *, const srl_color_camera *, int, int, const srl_color_track_point *tracked, int n, const int32_t *cand, int nc,
                               const srl_color_track_opts *opts, srl_color_track_point *out, int64_t capacity, uint8_t *, uint8_t *, srl_color_track_totals *tot) {
    g_updates++; g_last_n = n; g_last_nc = nc; g_last_capacity = capacity; g_flagged_in = 0;
    std::memset(tot, 0, sizeof *tot);
    int64_t k = 0;
    for (int i = 0; i < n; i++) {
        g_flagged_in += tracked[i].flagged;
        if (i == 0) continue;
        out[k] = tracked[i]; out[k].flagged = i == 1 ? 1 : 0; k++;
    }
    tot->tracked_in = n; tot->kept = k; tot->flagged = n > 1 ? 1 : 0; tot->dropped = n ? 1 : 0; tot->candidates = nc;
    for (int j = 0; j < nc && k < capacity && k < opts->maximum_tracked_points; j++) { out[k++] = srl_color_track_point{cand[j], 5.f, 6.f, 0}; tot->added++; }
    return SRL_OK;
}
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static int all_ones(const float *, const float *, int n, uint8_t *status, void *) { if (n) std::memset(status, 1, (size_t)n); return SRL_OK; }
static int pnp_even(const float *, const float *, int n, int32_t *inliers, int *n_inliers, void *) {
    *n_inliers = 0;
    for (int i = 0; i < n; i += 2) inliers[(*n_inliers)++] = i;
    return SRL_OK;
}
static int pnp_bad(const float *, const float *, int n, int32_t *inliers, int *n_inliers, void *) { inliers[0] = n; *n_inliers = 1; return SRL_OK; }
static int pnp_throws(const float *, const float *, int, int32_t *, int *, void *) { return SRL_ERR_BAD_ARG; }

int main() {
    const int rows = 480, cols = 640;
    std::vector<uint8_t> gray((size_t)rows * cols, 9);
    std::vector<srl_color_selected> rec(90);
    for (int i = 0; i < 90; i++) {
        rec[i].index = i; rec[i].pool = 1000 - 7 * i; rec[i].point_index = i;
        rec[i].x = (float)i; rec[i].y = 1.f; rec[i].z = 2.f;
        rec[i].u = 60.f + 5.f * (float)i; rec[i].v = 50.f + 4.f * (float)i;
    }
    std::vector<srl_color_selected> fresh(rec);                              // candidates the set does not hold
    for (int i = 0; i < 90; i++) fresh[i].pool = 5000 + i;
    srl_color_camera cam;
    std::memset(&cam, 0, sizeof cam);
    cam.q_world_camera[0] = 1.0; cam.fx = cam.fy = 200.0; cam.cx = 320.0; cam.cy = 240.0; cam.fov_margin = 0.005;

    srl_oft *h = nullptr;
    CHECK(srl_oft_create(nullptr, nullptr) == SRL_ERR_BAD_ARG && srl_oft_create(nullptr, &h) == SRL_OK && h);
    int a = -1, b = -1, c = -1, d = -1, n = -1;
    CHECK(srl_oft_init(h, nullptr, 3, gray.data(), rows, cols, cols, 1.0) == SRL_ERR_BAD_ARG && srl_oft_init(h, rec.data(), -1, gray.data(), rows, cols, cols, 1.0) == SRL_ERR_BAD_ARG);
    CHECK(srl_oft_init(h, rec.data(), 20, nullptr, rows, cols, cols, 1.0) == SRL_ERR_BAD_ARG);                      // the flow's refusal comes through
    CHECK(srl_oft_init(h, rec.data(), 20, gray.data(), rows, cols, cols, 1.0) == SRL_OK);
    CHECK(srl_oft_sizes(h, &a, &b, &c, &d) == SRL_OK && a == 20 && b == 0 && c == 20 && d == 0);
    CHECK(srl_oft_track_image(h, gray.data(), rows, cols, cols, 1.5, rows, cols, &n) == SRL_OK && n == 0);          // fewer than 30
    CHECK(srl_oft_init(h, rec.data(), 90, gray.data(), rows, cols, cols, 2.0) == SRL_OK);
    CHECK(srl_oft_track_image(h, gray.data(), rows, cols, cols, 2.1, rows, cols, &n) == SRL_ERR_BAD_ARG && n == 0);  // no fundamental-matrix provider
    CHECK(srl_oft_set_fundamental_provider(h, all_ones, nullptr) == SRL_OK && srl_oft_set_fundamental_provider(nullptr, all_ones, nullptr) == SRL_ERR_BAD_ARG);
    CHECK(srl_oft_track_image(h, gray.data(), rows, cols, cols, 2.1, rows, cols, &n) == SRL_OK && n > 30 && n <= 60);
    const int n_cur = n;
    std::vector<srl_color_track_point> pm(90);
    CHECK(srl_oft_pose_map(h, 1, nullptr, 0, &n) == SRL_OK && n == n_cur && srl_oft_pose_map(h, 1, pm.data(), n_cur - 1, &n) == SRL_ERR_BAD_ARG);
    CHECK(srl_oft_pose_map(h, 1, pm.data(), 90, &n) == SRL_OK && n == n_cur && srl_oft_pose_map(h, 2, pm.data(), 90, &n) == SRL_ERR_BAD_ARG);
    for (int i = 1; i < n_cur; i++) CHECK(pm[i - 1].pool < pm[i].pool);
    std::vector<srl_color_vio_point> vio(90);
    CHECK(srl_oft_tracked_for_vio(h, vio.data(), 90, &n) == SRL_OK && n == 90 && srl_oft_tracked_for_vio(h, vio.data(), 3, &n) == SRL_ERR_BAD_ARG);
    int acc = -1;
    CHECK(srl_oft_remove_outlier_using_ransac_pnp(h, 1, &acc) == SRL_ERR_BAD_ARG && acc == 0);                         // no PnP provider
    CHECK(srl_oft_set_pnp_provider(h, pnp_throws, nullptr) == SRL_OK && srl_oft_remove_outlier_using_ransac_pnp(h, 1, &acc) == SRL_OK && acc == 0);
    CHECK(srl_oft_set_pnp_provider(h, pnp_bad, nullptr) == SRL_OK && srl_oft_remove_outlier_using_ransac_pnp(h, 1, &acc) == SRL_ERR_BAD_ARG);
    CHECK(srl_oft_set_pnp_provider(h, pnp_even, nullptr) == SRL_OK && srl_oft_remove_outlier_using_ransac_pnp(h, 1, &acc) == SRL_OK && acc == 1);
    const int inl = (n_cur + 1) / 2;
    CHECK(srl_oft_sizes(h, &a, &b, &c, &d) == SRL_OK && a == inl && b == inl && c == inl && d == 0);
    // the update through the default path (the stand-in): the buffers hold n + min(candidates, maximum)
    srl_color_track_totals tot;
    CHECK(srl_oft_update_and_append_track_points(h, nullptr, rows, cols, rec.data(), 90, 10.0, &tot) == SRL_ERR_BAD_ARG && tot.kept == 0);
    CHECK(srl_oft_update_and_append_track_points(h, &cam, rows, cols, nullptr, 90, 10.0, &tot) == SRL_ERR_BAD_ARG);
    CHECK(srl_oft_set_maximum_tracked_points(h, 40) == SRL_OK);
    CHECK(srl_oft_update_and_append_track_points(h, &cam, rows, cols, fresh.data(), 90, 10.0, &tot) == SRL_OK);
    CHECK(g_updates == 1 && g_last_n == inl && g_last_nc == 90 && g_last_capacity == inl + 40 && g_flagged_in == 0);
    CHECK(tot.kept == inl - 1 && tot.added == 40 - (inl - 1) && srl_oft_sizes(h, &a, &b, &c, &d) == SRL_OK && a == 40 && c == 40 && d == 1);
    CHECK(srl_oft_update_and_append_track_points(h, &cam, rows, cols, nullptr, 0, 10.0, nullptr) == SRL_OK && g_last_n == 40 && g_last_nc == 0 && g_flagged_in == 1);
    CHECK(srl_oft_set_maximum_tracked_points(h, -2) == SRL_OK && srl_oft_update_and_append_track_points(h, &cam, rows, cols, rec.data(), 1, 10.0, &tot) == SRL_OK);
    CHECK(g_last_capacity == 39 + 1 && tot.added == 0);
    CHECK(srl_oft_set_track_points(h, nullptr, 0) == SRL_OK && srl_oft_sizes(h, &a, &b, &c, &d) == SRL_OK && a == 0 && c == 0);
    CHECK(srl_oft_update_and_append_track_points(h, &cam, rows, cols, nullptr, 0, 10.0, &tot) == SRL_OK && g_last_n == 0 && g_last_capacity == 0);
    double t0 = 0, t1 = 0;
    CHECK(srl_oft_times(h, &t0, &t1) == SRL_OK && t0 == 2.1 && t1 == 2.1);
    CHECK(srl_oft_destroy(h) == SRL_OK && srl_oft_destroy(nullptr) == SRL_OK);
    std::puts("tracker host mirror: ok");
    return 0;
}

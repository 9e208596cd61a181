// flow_host_san_main.cpp -- a stand-alone program over the host mirror's LKOpticalFlowKernel (sr_livo_amd/csrc/host/lkpyramid.cpp), built
// with -fsanitize=address,undefined by tests/test_flow_host_san.py: criteria clamping, argument handling and what the object hands to the
// C-ABI.  It makes no device call: the four srl_flow_* entry points the mirror uses are recording stand-ins defined here.
#include "../sr_livo_amd/csrc/host/lkpyramid.h"
#include "../include/srlivo_hip_debug.h"
#include "../include/srlivo_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static srl_flow_opts g_opts;
static int g_creates = 0, g_destroys = 0, g_tracks = 0, g_last_n = -1, g_fail_track = 0, g_first = 1;
static const float *g_last_prev = nullptr;

extern "C" {
void srl_flow_opts_default(srl_flow_opts *o) { o->win = 21; o->max_level = 3; o->max_count = 10; o->reserved = 0; o->epsilon = 0.05; o->min_eig_threshold = 1e-4; }
int srl_flow_create(srl_ctx *, const srl_flow_opts *o) {
    if (o->win != 21) return SRL_ERR_UNSUPPORTED;
    g_opts = *o; g_creates++; g_first = 1;
    return SRL_OK;
}
int srl_flow_destroy(srl_ctx *) { g_destroys++; return SRL_OK; }
int srl_flow_levels(srl_ctx *, int *L) { *L = 2; return SRL_OK; }
// the first image of a tracker is only stored (next = prev); afterwards the stand-in "tracks" by adding (1, 2) and marks every second point
int srl_flow_track_image(srl_ctx *, const uint8_t *gray, int rows, int cols, int64_t stride, const float *prev, int n, float *next, uint8_t *status, int *n_tracked) {
    *n_tracked = 0;
    if (g_fail_track || !gray || rows < 2 || cols < 2 || stride < cols) return SRL_ERR_BAD_ARG;
    g_tracks++; g_last_n = n; g_last_prev = prev;
    if (g_first) { g_first = 0; if (n) std::memcpy(next, prev, (size_t)n * 2 * sizeof(float)); return SRL_OK; }
    for (int i = 0; i < n; i++) { next[2 * i] = prev[2 * i] + 1.f; next[2 * i + 1] = prev[2 * i + 1] + 2.f; status[i] = (uint8_t)(i & 1); *n_tracked += i & 1; }
    return SRL_OK;
}
}

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

int main() {
    using namespace srlivo;
    {   // clamping (lkpyramid.cpp:670-682)
        struct { int type, count; double eps; int want_count; double want_eps; } cases[] = {
            {3, 10, 0.05, 10, 0.05}, {3, 500, 50.0, 100, 10.0}, {3, -4, -1.0, 0, 0.0}, {2, 7, 0.3, 30, 0.3}, {1, 7, 0.3, 7, 0.01}, {0, 7, 0.3, 30, 0.01}};
        for (auto &c : cases) {
            TermCriteria t; t.type = c.type; t.maxCount = c.count; t.epsilon = c.eps;
            LKOpticalFlowKernel k(nullptr, Size{21, 21}, 3, t, 8, 1e-4);
            CHECK(k.getTermCriteria().maxCount == c.want_count && k.getTermCriteria().epsilon == c.want_eps);
            CHECK(k.getMaxLevel() == 3 && k.getFlags() == 8 && k.getWinSize().width == 21 && k.getMinEigThreshold() == 1e-4);
        }
        LKOpticalFlowKernel d(nullptr);
        CHECK(d.getTermCriteria().maxCount == 30 && d.getTermCriteria().epsilon == 0.01 && d.getMaxLevel() == 3);
        CHECK(g_creates == 0 && g_destroys == 0);      // an object that never saw an image owns no device tracker
    }
    std::vector<uint8_t> gray(40 * 64, 7);
    {   // first image, tracking, empty lists, refusals
        TermCriteria t; t.type = 3; t.maxCount = 500; t.epsilon = 0.05;
        LKOpticalFlowKernel k(nullptr, Size{21, 21}, 3, t, 8, 2e-4);
        std::vector<Point2f> last(5), cur;
        for (int i = 0; i < 5; i++) { last[i].x = (float)i; last[i].y = (float)(10 * i); }
        std::vector<uint8_t> status(2, 9);
        CHECK(k.trackImage(gray.data(), 40, 64, 64, last, cur, status) == 0);
        CHECK(g_creates == 1 && g_opts.win == 21 && g_opts.max_level == 3 && g_opts.max_count == 100 && g_opts.epsilon == 0.05 && g_opts.min_eig_threshold == 2e-4);
        CHECK(cur.size() == 5 && cur[4].x == 4.f && cur[4].y == 40.f && status.size() == 2 && status[0] == 9 && k.getMaxLevel() == 2);      // first image: status untouched
        CHECK(k.trackImage(gray.data(), 40, 64, 64, last, cur, status) == 2 && g_creates == 1 && g_last_n == 5);
        CHECK(status.size() == 5 && status[1] == 1 && status[2] == 0 && cur[4].x == 5.f && cur[4].y == 42.f);
        std::vector<Point2f> none;
        CHECK(k.trackImage(gray.data(), 40, 64, 64, none, cur, status) == 0 && g_last_n == 0 && g_last_prev == nullptr && cur.empty() && status.empty());
        CHECK(k.trackImage(nullptr, 40, 64, 64, last, cur, status) == -1 && k.last_status == SRL_ERR_BAD_ARG);
        CHECK(k.trackImage(gray.data(), 40, 64, 10, last, cur, status) == -1 && k.last_status == SRL_ERR_BAD_ARG);
        std::vector<Point2f> many((size_t)SRL_FLOW_MAX_POINTS + 1);
        const int tracks = g_tracks;
        CHECK(k.trackImage(gray.data(), 40, 64, 64, many, cur, status) == -1 && k.last_status == SRL_ERR_BAD_ARG && g_tracks == tracks);
    }
    CHECK(g_destroys == 1);
    {   // a window the device does not take: nothing is created, nothing destroyed
        LKOpticalFlowKernel k(nullptr, Size{15, 15});
        std::vector<Point2f> last(1), cur;
        std::vector<uint8_t> status;
        CHECK(k.trackImage(gray.data(), 40, 64, 64, last, cur, status) == -1 && k.last_status == SRL_ERR_UNSUPPORTED);
        LKOpticalFlowKernel r(nullptr, Size{21, 15});
        CHECK(r.trackImage(gray.data(), 40, 64, 64, last, cur, status) == -1 && r.last_status == SRL_ERR_UNSUPPORTED);
    }
    CHECK(g_destroys == 1 && g_creates == 1);
    {   // the C handle
        srl_lk *h = nullptr;
        CHECK(srl_lk_create(nullptr, 21, 21, 3, 3, 10, 0.05, 8, 1e-4, nullptr) == SRL_ERR_BAD_ARG);
        CHECK(srl_lk_create(nullptr, 21, 21, 3, 3, 10, 0.05, 8, 1e-4, &h) == SRL_OK && h);
        int L = 0, mc = 0; double eps = 0;
        CHECK(srl_lk_get(h, &L, &mc, &eps) == SRL_OK && L == 3 && mc == 10 && eps == 0.05 && srl_lk_get(h, nullptr, nullptr, nullptr) == SRL_OK);
        float prev[6] = {1, 2, 3, 4, 5, 6}, next[6] = {0};
        uint8_t st[3] = {9, 9, 9};
        int nt = 7;
        CHECK(srl_lk_track_image(h, gray.data(), 40, 64, 64, prev, 3, next, st, &nt) == SRL_OK && nt == 0 && next[5] == 6.f && st[0] == 9);
        CHECK(srl_lk_track_image(h, gray.data(), 40, 64, 64, prev, 3, next, st, &nt) == SRL_OK && nt == 1 && next[5] == 8.f && st[0] == 0 && st[1] == 1);
        CHECK(srl_lk_track_image(h, gray.data(), 40, 64, 64, nullptr, 0, nullptr, nullptr, &nt) == SRL_OK && nt == 0);
        CHECK(srl_lk_track_image(h, gray.data(), 40, 64, 64, nullptr, 3, next, st, &nt) == SRL_ERR_BAD_ARG);
        CHECK(srl_lk_track_image(h, gray.data(), 40, 64, 64, prev, -1, next, st, &nt) == SRL_ERR_BAD_ARG);
        g_fail_track = 1;
        CHECK(srl_lk_track_image(h, gray.data(), 40, 64, 64, prev, 3, next, st, &nt) == SRL_ERR_BAD_ARG && nt == 0);
        g_fail_track = 0;
        CHECK(srl_lk_destroy(h) == SRL_OK && srl_lk_destroy(nullptr) == SRL_OK && g_destroys == 2);
    }
    std::puts("flow host mirror: ok");
    return 0;
}

// image_process_san_main.cpp -- a stand-alone program over the host mirror's imageProcessing::process (sr_livo_amd/csrc/host/imageProcessing.cpp)
// with the tracker it works on (opticalFlowTracker.cpp, lkpyramid.cpp), for AddressSanitizer and UBSan: tests/test_image_process_host_san.py
// compiles it with -fsanitize=address,undefined and runs it.  Every step that leaves the mirror is a stub of this file; the few device entry
// points the three translation units name are defined here and never reached.  No device, no Python in the instrumented process.
#include "../sr_livo_amd/csrc/host/imageProcessing.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

extern "C" {
void srl_image_prep_opts_default(srl_image_prep_opts *o) { std::memset(o, 0, sizeof *o); o->clip_gray = 3.0; o->clip_color = 1.0; }
void srl_flow_opts_default(srl_flow_opts *o) { std::memset(o, 0, sizeof *o); o->win = 21; o->max_level = 3; o->max_count = 10; o->epsilon = 0.05; o->min_eig_threshold = 1e-4; }
int srl_flow_create(srl_ctx *, const srl_flow_opts *) { std::abort(); }
int srl_flow_destroy(srl_ctx *) { return SRL_OK; }
int srl_flow_levels(srl_ctx *, int *) { std::abort(); }
int srl_flow_track_image(srl_ctx *, const uint8_t *, int, int, int64_t, const float *, int, float *, uint8_t *, int *) { std::abort(); }
int srl_color_map_track_update(srl_ctx *, const srl_color_camera *, int, int, const srl_color_track_point *, int, const int32_t *, int, const srl_color_track_opts *,
                               srl_color_track_point *, int64_t, uint8_t *, uint8_t *, srl_color_track_totals *) { std::abort(); }
}

namespace {
using namespace srlivo;

struct Stubs {
    int prep_created = 0, setups = 0, prepared = 0, selections = 0, flows = 0, renders = 0, rows_calls = 0, updates = 0;
    int n_selected = 40, fundamental_keeps = -1, fail_prepare_once = 0, fail_init_once = 0;
    srl_image_prep_opts created = {};
    double k_setup[4] = {0, 0, 0, 0};
};

void install(imageProcessing &ip, opticalFlowTracker &t, Stubs &s) {
    ip.op_tracker = &t;
    ip.steps.prepCreate = [&s](const srl_image_prep_opts &o) { s.prep_created++; s.created = o; return (int)SRL_OK; };
    ip.steps.consensusSetup = [&s](const double *k) { s.setups++; for (int i = 0; i < 4; i++) s.k_setup[i] = k[i]; return (int)SRL_OK; };
    ip.steps.prepare = [&s](const uint8_t *raw, int rows, int cols, int64_t stride, bool) {
        s.prepared++;
        if (s.fail_prepare_once) { s.fail_prepare_once = 0; return (int)SRL_ERR_UNSUPPORTED; }
        unsigned sum = 0;                                    // every byte of every row the caller handed over is readable
        for (int r = 0; r < rows; r++) for (int c = 0; c < 3 * cols; c++) sum += raw[(size_t)r * (size_t)stride + c];
        return sum == 0xFFFFFFFFu ? (int)SRL_ERR_BAD_ARG : (int)SRL_OK;
    };
    ip.steps.select = [&s](const srl_color_camera &, int, int, const srl_color_select_opts &, bool, std::vector<srl_color_selected> &out) {
        s.selections++;
        out.resize((size_t)s.n_selected);
        for (int k = 0; k < s.n_selected; k++) {
            srl_color_selected &r = out[(size_t)k];
            r.index = k; r.pool = 3 * k + 1; r.point_index = k;
            r.x = 0.1f * k; r.y = 0.2f * k; r.z = 5.0f;
            r.u = 12.0f + 2.0f * (k % 40); r.v = 14.0f + 9.0f * (k / 40);
        }
        return (int)SRL_OK;
    };
    ip.steps.render = [&s](const srl_color_camera &, double, srl_color_render_totals &tot) { s.renders++; tot.listed = 7; return (int)SRL_OK; };
    ip.rows = [&s](const srl_color_vio_args *, const srl_color_vio_point *, int n, srl_color_vio_sums *sums) {
        s.rows_calls++;
        std::memset(sums, 0, sizeof *sums);
        sums->used = n;
        return (int)SRL_OK;
    };
    t.use_prepared_image = true;
    t.flow = [&s](const uint8_t *, int, int, int64_t, const float *prev, int n, float *next, uint8_t *st) {
        s.flows++;
        if (s.fail_init_once) { s.fail_init_once = 0; return (int)SRL_ERR_UNSUPPORTED; }
        for (int i = 0; i < n; i++) { next[2 * i] = prev[2 * i] + 2.0f; next[2 * i + 1] = prev[2 * i + 1] + 1.0f; st[i] = 1; }
        return (int)SRL_OK;
    };
    t.fundamental = [&s](const float *, const float *, int n, uint8_t *st) {
        for (int i = 0; i < n; i++) st[i] = (s.fundamental_keeps < 0 || i < s.fundamental_keeps) ? 1 : 0;
        return (int)SRL_OK;
    };
    t.pnp = [](const float *, const float *, int n, int32_t *in, int *nin) { for (int i = 0; i < n; i++) in[i] = i; *nin = n; return (int)SRL_OK; };
    t.update = [&s](const srl_color_camera *, int, int, const srl_color_track_point *tracked, int n, const int32_t *, int nc, const srl_color_track_opts *,
                    srl_color_track_point *out, int64_t cap, srl_color_track_totals *tot) {
        s.updates++;
        if (cap < n) return (int)SRL_ERR_BAD_ARG;
        for (int i = 0; i < n; i++) out[i] = tracked[i];
        tot->tracked_in = n; tot->kept = n; tot->candidates = nc;
        return (int)SRL_OK;
    };
}

int scenario(int n_selected, int fundamental_keeps, bool fail_prepare, bool fail_init) {
    imageProcessing ip;
    opticalFlowTracker tracker(nullptr);
    Stubs s;
    s.n_selected = n_selected; s.fundamental_keeps = fundamental_keeps; s.fail_prepare_once = fail_prepare; s.fail_init_once = fail_init;
    install(ip, tracker, s);
    ip.camera_intrinsic = srl::Mat3::Identity();
    ip.camera_intrinsic(0, 0) = 95.0; ip.camera_intrinsic(1, 1) = 97.0; ip.camera_intrinsic(0, 2) = 52.5; ip.camera_intrinsic(1, 2) = 36.5;
    ip.image_width = 100; ip.image_height = 70; ip.image_resize_ratio = 0.5;
    cameraState st;
    st.fx = 95.0; st.fy = 97.0; st.cx = 52.5; st.cy = 36.5;
    const int rows = 74, cols = 106;
    const int64_t stride = 3 * cols + 13;
    std::vector<uint8_t> image((size_t)(rows - 1) * (size_t)stride + 3 * cols, (uint8_t)0xA5);      // ends with the last row's last byte
    imageFrame f;
    f.rgb_image = image.data(); f.image_rows = rows; f.image_cols = cols; f.row_stride_bytes = stride;
    const double scale = 100 * 0.5 / cols;
    srl_image_process_result r;
    int frame = 0;
    if (fail_prepare || fail_init) {                         // the first frame fails in its first data and is offered again
        f.time_sweep_end = 10.0; f.frame_id = ++frame;
        CHECK(ip.process(st, f, 20, &r) == SRL_ERR_UNSUPPORTED && r.first_data == 1 && ip.first_data && ip.time_last_process == -1e5);
        --frame;
    }
    for (int k = 0; k < 3; k++) {
        f.time_sweep_end = 10.0 + 0.1 * k; f.frame_id = ++frame;
        CHECK(ip.process(st, f, 20, &r) == SRL_OK);
        CHECK(r.first_data == (k == 0 ? 1 : 0) && r.image_scale_factor == scale && ip.time_last_process == f.time_sweep_end);
        CHECK(r.prepared_rows == (int)(70 / scale) && r.prepared_cols == (int)(100 / scale) && r.refreshed_candidates == n_selected);
        if (n_selected >= 30 && fundamental_keeps < 0) CHECK(r.pnp_accepted == 1 && r.esikf_accepted == 1 && r.photometric_accepted == 1);
        if (fundamental_keeps >= 0 && fundamental_keeps < 10) CHECK(r.pnp_accepted == 0 && r.esikf_iterations == 0);
    }
    // nothing of the first data was done twice
    CHECK(s.prep_created == 1 && s.setups == 1 && s.renders == 3 && s.updates == 3 && s.selections == 4 + (fail_init ? 1 : 0));
    CHECK(ip.camera_intrinsic(0, 0) == 95.0 / scale && ip.camera_intrinsic(1, 2) == 36.5 / scale && s.created.fx == 95.0 / scale && s.k_setup[3] == 36.5 / scale);
    CHECK(s.created.rows == (int)(70 / scale) && s.created.cols == (int)(100 / scale) && s.created.clip_gray == 3.0);
    return 0;
}
}  // namespace

int main() {
    if (scenario(40, -1, false, false)) return 1;            // the plain sequence
    if (scenario(40, -1, true, false)) return 1;             // a refused prepare on the first frame
    if (scenario(40, -1, false, true)) return 1;             // a failing init on the first frame
    if (scenario(40, 5, false, false)) return 1;             // five points behind the flow: PnP not accepted
    if (scenario(29, -1, false, false)) return 1;            // below trackImage's thirty
    if (scenario(5000, -1, false, false)) return 1;          // a selection of thousands, most of it outside the image
    if (scenario(0, -1, false, false)) return 1;             // nothing selected at all
    std::printf("image process host mirror: ok\n");
    return 0;
}

// srl_points.hip -- the step that PRODUCES the points: Livox messages decoded into a device point queue, sweeps cut from it at image
// times, and the cut undistorted without a visit to the host.
//   srl_livox_decode          cloudProcessing::livoxHandler (cloudProcessing.cpp:125-214), statement by statement: the 20-byte records go
//                             up once; stable sort of (offset_time, message index) over all 32 key bits (four 8-bit passes of
//                             srl_frame_scratch.h's radix pass: relative_time = double(offset) * scale is strictly monotone in the
//                             integer for a positive scale, so the integer IS the sort key) -> validity flags in sorted order -> scan
//                             (rank among the valid points; the modulo pick and the range test ride in its sink) -> scan over the
//                             survivors whose sink appends to the queue.  Sorting everything first and compacting the valid points
//                             afterwards is the same order as the reference's "collect, then sort" for a stable sort, and needs no
//                             count on the host between the two.  Ties keep message order: that is this library's SPECIFICATION --
//                             std::sort's order among equal keys is its library's own and cannot be reproduced.
//   the queue                 one SoA block (x | y | z | relative_time | timestamp, stride = capacity), head and size on the host,
//                             grown by doubling into a fresh block (which also compacts to the front)
//   srl_points_cut            while (front().timestamp < t) pop: a min-reduction over the indices that FAIL the test gives the prefix
//                             length (the queue need not be sorted across messages), then one kernel moves the prefix to the resident cut
//   srl_frame_undistort_cut   makePointTimestamp (lioOptimization.cpp:786-819) as flag + scan with the rewrite in the sink, the IMU
//                             interval of every point by rule instead of the sequential walk (see k_seg_rule), then the kernel of
//                             srl_frame_undistort (srl_undistort.h) on the blocks srl_frame_subsample / srl_frame_take read
// No floating-point atomic anywhere: the reductions are integer minima and maxima, so every call gives the same bytes.
// Built with -ffp-contract=off: every FP64 statement below is the reference's sequence of separately rounded operations.
#include "srl_ctx.h"
#include "srl_frame_scratch.h"
#include "srl_points_queue.h"
#include "srl_undistort.h"
#include "../../include/srlivo_hip_debug.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

static_assert(sizeof(srl_livox_point) == 20, "srl_livox_point is livox_ros_driver::CustomPoint in memory");
static_assert(sizeof(srl_livox_opts) == 32 && sizeof(srl_livox_report) == 40 && sizeof(srl_points_cut_report) == 16, "ABI structs of srlivo_hip.h");

namespace {

// minimum of v over the wave, folded into *w by one lane (v = 0xFFFFFFFF: nothing to report); every lane of the wave must call it
__device__ inline void d_wave_min_into(unsigned v, unsigned *w) {
    for (int d = 32; d >= 1; d >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, d));
    if ((threadIdx.x & 63) == 0 && v != 0xFFFFFFFFu) atomicMin(w, v);
}

__global__ void k_set_int(int *w, int v) { *w = v; }

// ---------------------------------------------------------------------------------------------------------------- decode
__global__ void k_livox_keys(const srl_livox_point *p, int n, unsigned *keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = p[i].offset_time;
}

// cloudProcessing.cpp:136-150 for message index i
__device__ inline bool d_livox_valid(const srl_livox_point *p, int i, int n_scans) {
    if (i < 1) return false;
    const srl_livox_point a = p[i], b = p[i - 1];
    if (!((int)a.line < n_scans)) return false;
    if ((double)fabsf(a.x) > 1e8 || (double)fabsf(a.y) > 1e8 || (double)fabsf(a.z) > 1e8) return false;
    if (!((double)a.x > 0.7)) return false;
    if ((double)a.x > 2.0 && (((a.tag & 0x03) != 0x00) || ((a.tag & 0x0C) != 0x00))) return false;
    return (double)fabsf(a.x - b.x) > 1e-7 || (double)fabsf(a.y - b.y) > 1e-7 || (double)fabsf(a.z - b.z) > 1e-7;
}
__global__ void k_livox_valid(const srl_livox_point *p, const unsigned *order, int n, int n_scans, int *flag) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) flag[j] = d_livox_valid(p, (int)order[j], n_scans) ? 1 : 0;
}
// scan over the validity flags in sorted order: the exclusive prefix is the point's position among the sorted valid points
struct SinkPick {
    const srl_livox_point *p;
    const unsigned *order;
    int n, pfn;
    double blind2;
    int *flag2, *words;
    __device__ void operator()(int j, int v, int excl) const {
        int keep = 0;
        if (v) {
            atomicMax(&words[W_LASTJ], j);                       // .back() of the sorted vector
            if ((excl + 1) % pfn == 0) {
                const srl_livox_point a = p[order[j]];
                const double x = (double)a.x, y = (double)a.y, z = (double)a.z;
                keep = (x * x + y * y) + z * z > blind2 ? 1 : 0;
            }
        }
        flag2[j] = keep;
        if (j == n - 1) words[W_VALID] = excl + v;
    }
};
struct SinkAppend {
    const srl_livox_point *p;
    const unsigned *order, *keys;      // sorted message indices and offsets
    int n;
    double scale, stamp;
    double *tail;                      // queue plane 0 at the first free record
    int stride;
    int *words;
    __device__ void operator()(int j, int v, int excl) const {
        if (v) {
            const srl_livox_point a = p[order[j]];
            const double rel = (double)keys[j] * scale;
            tail[(size_t)PL_X * stride + excl] = (double)a.x;
            tail[(size_t)PL_Y * stride + excl] = (double)a.y;
            tail[(size_t)PL_Z * stride + excl] = (double)a.z;
            tail[(size_t)PL_REL * stride + excl] = rel;
            tail[(size_t)PL_TS * stride + excl] = rel / 1000.0 + stamp;
        }
        if (j == n - 1) words[W_APPENDED] = excl + v;
    }
};
__global__ void k_livox_report(int *words, const unsigned *keys, double scale, double stamp, int pfn, const double *tail_ts) {
    srl_livox_report *r = reinterpret_cast<srl_livox_report *>(words + W_WORDS);
    const int valid = words[W_VALID], app = words[W_APPENDED];
    r->valid = valid; r->picked = valid / pfn; r->appended = app; r->reserved = 0;
    r->last_end_time = valid > 0 ? stamp + ((double)keys[words[W_LASTJ]] * scale) / 1000.0 : d_nan();
    r->first_timestamp = app > 0 ? tail_ts[0] : d_nan();
    r->last_timestamp = app > 0 ? tail_ts[app - 1] : d_nan();
}

// ---------------------------------------------------------------------------------------------------------------- cut
__global__ void k_cut_find(const double *ts, int s, double t, unsigned *w) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    d_wave_min_into(k < s && !(ts[k] < t) ? (unsigned)k : 0xFFFFFFFFu, w);
}
__global__ void k_cut_move(const double *front, int stride, int s, int *words, double *cut, int cut_stride) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = words[W_CUT];
    if (k < c)
        for (int pl = 0; pl < PL_COUNT; pl++) cut[(size_t)pl * cut_stride + k] = front[(size_t)pl * stride + k];
    if (k == 0) {
        srl_points_cut_report *r = reinterpret_cast<srl_points_cut_report *>(words + W_WORDS);
        r->count = c; r->reserved = 0;
        r->front_timestamp = c < s ? front[(size_t)PL_TS * stride + c] : d_nan();
    }
}

// ---------------------------------------------------------------------------------------------------------------- time rewrite
__global__ void k_rewrite_flag(const double *ts, int n0, double tb, double te, int enable, int *flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n0) return;
    const double t = ts[i];
    flag[i] = enable || !(t > te || t < tb) ? 1 : 0;          // lioOptimization.cpp:808-809
}
struct SinkRewrite {
    const double *cut;
    int cut_stride, n0, enable;
    double tb, delta_t;
    double *raw, *rel, *ts_out, *alpha_out;
    int *words;
    __device__ void operator()(int i, int v, int excl) const {
        if (v) {
            const double ts = cut[(size_t)PL_TS * cut_stride + i];
            double r = ts - tb;
            double alpha = r / delta_t;
            r = r * 1000.0;
            if (enable && alpha > 1.0) alpha = 1.0 - 1e-5;
            raw[(size_t)excl * 3] = cut[(size_t)PL_X * cut_stride + i];
            raw[(size_t)excl * 3 + 1] = cut[(size_t)PL_Y * cut_stride + i];
            raw[(size_t)excl * 3 + 2] = cut[(size_t)PL_Z * cut_stride + i];
            rel[excl] = r; ts_out[excl] = ts; alpha_out[excl] = alpha;
        }
        if (i == n0 - 1) words[W_N] = excl + v;
    }
};

// ---------------------------------------------------------------------------------------------------------------- IMU intervals by rule
// The walk of distortFrameByImu (srl_undistort.h) is a sequential loop.  Where the times t_i = time_begin + relative_i / 1000.0 and the state
// stamps are both non-decreasing it equals: k(i) = the smallest k with t_i < stamp[k + 1] + 1e-6, accepted iff t_i > stamp[k] - 1e-6; the
// first point without an accepted interval stops the walk, so it and every point behind it get -1.  (Intervals in front of k(i) cannot take
// the point: their upper test fails; the cursor cannot be past k(i): it sits at k(i - 1) <= k(i) because t_{i-1} <= t_i; and once the lower
// test fails at k(i) it fails at every later interval, whose lower stamp is no smaller.)  tests/test_livox_checker.py holds rule == walk.
__global__ void k_times_check(const double *rel, const int *words_n, int *words) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 1 && i < *words_n && !(rel[i - 1] <= rel[i])) words[W_NONMONO] = 1;
}
__global__ void k_seg_rule(const double *rel, const int *words_n, double tfb, const double *states, int n_states, int *seg, unsigned *fail) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned failed = 0xFFFFFFFFu;
    if (i < *words_n) {
        const double t = tfb + rel[i] / 1000.0;
        int k = -1;
        for (int kk = 0; kk + 1 < n_states; kk++)
            if (t < states[17 * (size_t)(kk + 1)] + 1e-6) {
                if (t > states[17 * (size_t)kk] - 1e-6) k = kk;
                break;
            }
        seg[i] = k;
        if (k < 0) failed = (unsigned)i;
    }
    d_wave_min_into(failed, fail);
}
__global__ void k_seg_stop(const int *words_n, const int *fail, int *seg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < *words_n && i >= *fail) seg[i] = -1;
}

__global__ void k_gather_times(const int *index, int m, const double *ts, const double *rel, const double *alpha, double *out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int i = index[k];
    out[k] = ts[i]; out[(size_t)m + k] = rel[i]; out[2 * (size_t)m + k] = alpha[i];
}

template <class T>
int grow_block(srl_ctx *ctx, T *&p, int &cap, int want, size_t per_record) {
    if (want <= cap) return SRL_OK;
    if (p) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(p)); p = nullptr; cap = 0; }
    const int grown = std::max(want, SRL_POINTS_QUEUE_MIN_CAP);
    HIPCHK(ctx, hipMalloc((void **)&p, (size_t)grown * per_record));
    cap = grown;
    return SRL_OK;
}

// count records of a PL_COUNT-plane block starting at `first` -> the caller's arrays
int download_records(srl_ctx *ctx, const double *first, int stride, int count, double *raw_xyz, double *relative_time, double *timestamp) {
    if (count == 0 || (!raw_xyz && !relative_time && !timestamp)) return SRL_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<double> h((size_t)count * PL_COUNT);
    for (int pl = 0; pl < PL_COUNT; pl++)
        HIPCHK(ctx, hipMemcpyAsync(h.data() + (size_t)pl * count, first + (size_t)pl * stride, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < count; k++) {
        if (raw_xyz) for (int d = 0; d < 3; d++) raw_xyz[(size_t)k * 3 + d] = h[(size_t)d * count + k];
        if (relative_time) relative_time[k] = h[(size_t)PL_REL * count + k];
        if (timestamp) timestamp[k] = h[(size_t)PL_TS * count + k];
    }
    return SRL_OK;
}

}  // namespace

extern "C" {

void srl_points_release(srl_ctx *ctx) {
    SrlPoints *P = ctx ? ctx->points : nullptr;
    if (!P) return;
    if (P->q) (void)hipFree(P->q);
    if (P->c) (void)hipFree(P->c);
    if (P->t) (void)hipFree(P->t);
    if (P->d_words) (void)hipFree(P->d_words);
    if (P->h_words) (void)hipHostFree(P->h_words);
    delete P;
    ctx->points = nullptr;
}

double srl_time_unit_scale(int unit) {
    float s;
    switch (unit) {                    // cloudProcessing.cpp:44-66 (SEC, MS, US, NS of cloudProcessing.h)
    case 0: s = 1.e3f; break;
    case 1: s = 1.f; break;
    case 2: s = 1.e-3f; break;
    case 3: s = 1.e-6f; break;
    default: s = 1.f; break;
    }
    return (double)s;
}

int srl_livox_decode(srl_ctx *ctx, const srl_livox_point *points, int point_num, double header_stamp, const srl_livox_opts *opts, srl_livox_report *report) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (report) { std::memset(report, 0, sizeof *report); report->last_end_time = report->first_timestamp = report->last_timestamp = nan; }
    if (!ctx || !opts || point_num < 0 || (point_num > 0 && !points)) return SRL_ERR_BAD_ARG;
    if (opts->point_filter_num < 1 || opts->n_scans < 0 || !(opts->time_unit_scale > 0.0) || std::isinf(opts->time_unit_scale) || std::isnan(opts->blind) ||
        std::isnan(header_stamp))
        return SRL_ERR_BAD_ARG;
    if (point_num > SRL_SCAN_MAX) { ctx->err = "a Livox message of more than 2^20 points"; return SRL_ERR_UNSUPPORTED; }
    if (ctx->nranks > 1) { ctx->err = "the point queue is not sharded"; return SRL_ERR_UNSUPPORTED; }
    SRL_DISARM(ctx);
    if (!ctx->points) ctx->points = new SrlPoints();
    SrlPoints &P = *ctx->points;
    const int n = point_num;
    if (n <= 1) return SRL_OK;         // point 0 is never output: no valid point
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = points_words(ctx, P);
    if (rc) return rc;
    const int pfn = opts->point_filter_num;
    rc = points_reserve(ctx, P, (n - 1) / pfn);        // picked <= valid / pfn <= (n - 1) / pfn
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    DevBuf b_pts, b_keys, b_ks, b_vs, b_tk, b_tv, b_flag, b_flag2, b_sc;
    HIPCHK(ctx, b_pts.alloc(ctx, (size_t)n * sizeof(srl_livox_point)));
    for (DevBuf *b : {&b_keys, &b_ks, &b_vs, &b_tk, &b_tv, &b_flag, &b_flag2}) HIPCHK(ctx, b->alloc(ctx, (size_t)n * 4));
    HIPCHK(ctx, b_sc.alloc(ctx, std::max(srl_radix_scratch_ints(n), srl_scan_scratch_ints(n)) * 4));
    const srl_livox_point *d_pts = b_pts.as<srl_livox_point>();
    HIPCHK(ctx, hipMemcpyAsync(b_pts.p, points, (size_t)n * sizeof(srl_livox_point), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_livox_keys, grid256(n), dim3(256), 0, st, d_pts, n, b_keys.as<unsigned>());
    // all 32 bits of the offset: four passes of eight (srl_radix_sort_pairs' pass arithmetic holds beyond the 27 bits its other users need)
    srl_radix_sort_pairs(b_keys.as<unsigned>(), nullptr, b_ks.as<unsigned>(), b_vs.as<unsigned>(), b_tk.as<unsigned>(), b_tv.as<unsigned>(), n, 32u, st, b_sc.as<int>());
    HIPCHK(ctx, hipMemsetAsync(P.d_words, 0xFF, SRL_POINTS_WORD_BYTES, st));
    hipLaunchKernelGGL(k_livox_valid, grid256(n), dim3(256), 0, st, d_pts, (const unsigned *)b_vs.as<unsigned>(), n, (int)opts->n_scans, b_flag.as<int>());
    const SinkPick pick = {d_pts, b_vs.as<unsigned>(), n, pfn, opts->blind * opts->blind, b_flag2.as<int>(), P.d_words};
    srl_scan(SrlIntArrayIn{b_flag.as<int>()}, pick, n, b_sc.as<int>(), st);
    double *tail = P.q + P.head + P.size;
    const SinkAppend app = {d_pts, b_vs.as<unsigned>(), b_ks.as<unsigned>(), n, opts->time_unit_scale, header_stamp, tail, P.cap, P.d_words};
    srl_scan(SrlIntArrayIn{b_flag2.as<int>()}, app, n, b_sc.as<int>(), st);
    hipLaunchKernelGGL(k_livox_report, dim3(1), dim3(1), 0, st, P.d_words, (const unsigned *)b_ks.as<unsigned>(), opts->time_unit_scale, header_stamp, pfn,
                       (const double *)(tail + (size_t)PL_TS * P.cap));
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(P.h_words, P.d_words, SRL_POINTS_WORD_BYTES, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    srl_livox_report r;
    std::memcpy(&r, P.h_words + W_WORDS * sizeof(int), sizeof r);
    if (r.appended < 0 || r.appended > (n - 1) / pfn) { ctx->err = "livox decode: the device reported an impossible count"; return SRL_ERR_HIP; }
    if (r.appended > 0) {
        if (P.size == 0) P.front_ts = r.first_timestamp;
        P.back_ts = r.last_timestamp;
        P.size += r.appended;
    }
    if (report) *report = r;
    return SRL_OK;
}

int srl_points_info(srl_ctx *ctx, int *size, double *front_timestamp, double *back_timestamp) {
    if (!ctx) return SRL_ERR_BAD_ARG;
    if (ctx->nranks > 1) return SRL_ERR_UNSUPPORTED;
    SRL_DISARM(ctx);
    if (!ctx->points) { ctx->err = "no point queue (srl_livox_decode first)"; return SRL_ERR_NO_SWEEP; }
    const SrlPoints &P = *ctx->points;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (size) *size = P.size;
    if (front_timestamp) *front_timestamp = P.size > 0 ? P.front_ts : nan;
    if (back_timestamp) *back_timestamp = P.size > 0 ? P.back_ts : nan;
    return SRL_OK;
}

int srl_points_clear(srl_ctx *ctx) {
    if (!ctx) return SRL_ERR_BAD_ARG;
    if (ctx->nranks > 1) return SRL_ERR_UNSUPPORTED;
    SRL_DISARM(ctx);
    if (!ctx->points) { ctx->err = "no point queue (srl_livox_decode first)"; return SRL_ERR_NO_SWEEP; }
    ctx->points->head = 0;
    ctx->points->size = 0;
    return SRL_OK;
}

int srl_points_cut(srl_ctx *ctx, double t, srl_points_cut_report *report) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (report) { report->count = 0; report->reserved = 0; report->front_timestamp = nan; }
    if (!ctx || std::isnan(t)) return SRL_ERR_BAD_ARG;
    if (ctx->nranks > 1) { ctx->err = "the point queue is not sharded"; return SRL_ERR_UNSUPPORTED; }
    SRL_DISARM(ctx);
    if (!ctx->points) { ctx->err = "no point queue (srl_livox_decode first)"; return SRL_ERR_NO_SWEEP; }
    SrlPoints &P = *ctx->points;
    const int s = P.size;
    if (s == 0) { P.cut_n = 0; return SRL_OK; }        // front() of an empty queue upstream; here: an empty cut
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = points_words(ctx, P);
    if (rc) return rc;
    P.cut_n = -1;
    rc = grow_block(ctx, P.c, P.cut_cap, s, PL_COUNT * sizeof(double));
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const double *front = P.q + P.head;
    hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, st, P.d_words + W_CUT, s);
    hipLaunchKernelGGL(k_cut_find, grid256(s), dim3(256), 0, st, front + (size_t)PL_TS * P.cap, s, t, reinterpret_cast<unsigned *>(P.d_words + W_CUT));
    hipLaunchKernelGGL(k_cut_move, grid256(s), dim3(256), 0, st, front, P.cap, s, P.d_words, P.c, P.cut_cap);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(P.h_words, P.d_words, SRL_POINTS_WORD_BYTES, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    srl_points_cut_report r;
    std::memcpy(&r, P.h_words + W_WORDS * sizeof(int), sizeof r);
    if (r.count < 0 || r.count > s) { ctx->err = "points cut: the device reported an impossible count"; return SRL_ERR_HIP; }
    P.cut_n = r.count;
    P.head += r.count;
    P.size -= r.count;
    if (P.size == 0) P.head = 0; else P.front_ts = r.front_timestamp;
    if (report) *report = r;
    return SRL_OK;
}

int srl_points_queue_download(srl_ctx *ctx, double *raw_xyz, double *relative_time, double *timestamp, int capacity, int *n) {
    if (n) *n = 0;
    if (!ctx || capacity < 0) return SRL_ERR_BAD_ARG;
    if (ctx->nranks > 1) return SRL_ERR_UNSUPPORTED;
    SRL_DISARM(ctx);
    if (!ctx->points) { ctx->err = "no point queue (srl_livox_decode first)"; return SRL_ERR_NO_SWEEP; }
    const SrlPoints &P = *ctx->points;
    if (n) *n = P.size;
    if (capacity < P.size) { ctx->err = "queue download: capacity below the queue's size"; return SRL_ERR_BAD_ARG; }
    return download_records(ctx, P.q + P.head, P.cap, P.size, raw_xyz, relative_time, timestamp);
}

int srl_points_cut_download(srl_ctx *ctx, double *raw_xyz, double *relative_time, double *timestamp, int capacity, int *n) {
    if (n) *n = 0;
    if (!ctx || capacity < 0) return SRL_ERR_BAD_ARG;
    if (ctx->nranks > 1) return SRL_ERR_UNSUPPORTED;
    SRL_DISARM(ctx);
    if (!ctx->points || ctx->points->cut_n < 0) { ctx->err = "no resident cut (srl_points_cut first)"; return SRL_ERR_NO_SWEEP; }
    const SrlPoints &P = *ctx->points;
    if (n) *n = P.cut_n;
    if (capacity < P.cut_n) { ctx->err = "cut download: capacity below the cut's size"; return SRL_ERR_BAD_ARG; }
    return download_records(ctx, P.c, P.cut_cap, P.cut_n, raw_xyz, relative_time, timestamp);
}

int srl_debug_points_fallbacks(srl_ctx *ctx, int64_t *count) {
    if (!ctx || !count) return SRL_ERR_BAD_ARG;
    *count = ctx->points ? ctx->points->fallbacks : 0;
    return SRL_OK;
}

int srl_frame_undistort_cut(srl_ctx *ctx, double time_begin, double time_end, int point_time_enable, const srl_imu_state *imu_states, int n_states,
                            int motion_compensation, const double R_il[9], const double t_il[3], int *n_out) {
    if (n_out) *n_out = 0;
    if (!ctx || !imu_states || n_states < 1 || !R_il || !t_il || std::isnan(time_begin) || std::isnan(time_end)) return SRL_ERR_BAD_ARG;
    if (motion_compensation != SRL_MC_IMU && motion_compensation != SRL_MC_CONSTANT_VELOCITY && motion_compensation != SRL_MC_NONE) return SRL_ERR_BAD_ARG;
    if (ctx->nranks > 1) { ctx->err = "the point queue is not sharded"; return SRL_ERR_UNSUPPORTED; }
    SRL_DISARM(ctx);
    if (!ctx->points || ctx->points->cut_n < 0) { ctx->err = "no resident cut (srl_points_cut first)"; return SRL_ERR_NO_SWEEP; }
    SrlPoints &P = *ctx->points;
    const int n0 = P.cut_n;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->corr_n = -1;
    ctx->sub_n = -1;
    ctx->corr_from_cut = false;
    int rc = srl_corr_reserve(ctx, n0);
    if (rc) return rc;
    if (n0 == 0) { ctx->corr_n = 0; ctx->corr_from_cut = true; return SRL_OK; }
    rc = points_words(ctx, P);
    if (rc) return rc;
    rc = grow_block(ctx, P.t, P.t_cap, n0, 2 * sizeof(double));
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    DevBuf b_flag, b_sc, b_states;
    HIPCHK(ctx, b_flag.alloc(ctx, (size_t)n0 * 4));
    HIPCHK(ctx, b_sc.alloc(ctx, srl_scan_scratch_ints(n0) * 4));
    HIPCHK(ctx, b_states.alloc(ctx, (size_t)n_states * sizeof(srl_imu_state)));
    HIPCHK(ctx, hipMemcpyAsync(b_states.p, imu_states, (size_t)n_states * sizeof(srl_imu_state), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(P.d_words, 0x7F, SRL_POINTS_WORD_BYTES, st));          // every word a large positive int (W_FAIL: "no point failed")
    HIPCHK(ctx, hipMemsetAsync(ctx->d_corr_imu, 0, (size_t)n0 * 24, st));
    const int enable = point_time_enable ? 1 : 0;
    hipLaunchKernelGGL(k_rewrite_flag, grid256(n0), dim3(256), 0, st, (const double *)(P.c + (size_t)PL_TS * P.cut_cap), n0, time_begin, time_end, enable, b_flag.as<int>());
    const SinkRewrite rw = {P.c, P.cut_cap, n0, enable, time_begin, time_end - time_begin, ctx->d_corr_in, ctx->d_corr_rel, P.t, P.t + P.t_cap, P.d_words};
    srl_scan(SrlIntArrayIn{b_flag.as<int>()}, rw, n0, b_sc.as<int>(), st);
    bool host_walk = false;
    if (motion_compensation == SRL_MC_IMU) {
        for (int k = 0; k + 1 < n_states; k++)
            if (!(imu_states[k].timestamp <= imu_states[k + 1].timestamp)) host_walk = true;
        if (!host_walk) {
            hipLaunchKernelGGL(k_times_check, grid256(n0), dim3(256), 0, st, (const double *)ctx->d_corr_rel, (const int *)(P.d_words + W_N), P.d_words);
            hipLaunchKernelGGL(k_seg_rule, grid256(n0), dim3(256), 0, st, (const double *)ctx->d_corr_rel, (const int *)(P.d_words + W_N), time_begin,
                               (const double *)b_states.as<double>(), n_states, ctx->d_corr_seg, reinterpret_cast<unsigned *>(P.d_words + W_FAIL));
            hipLaunchKernelGGL(k_seg_stop, grid256(n0), dim3(256), 0, st, (const int *)(P.d_words + W_N), (const int *)(P.d_words + W_FAIL), ctx->d_corr_seg);
        }
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(P.h_words, P.d_words, SRL_POINTS_WORD_BYTES, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const int *hw = reinterpret_cast<const int *>(P.h_words);
    const int n = hw[W_N];
    if (n < 0 || n > n0) { ctx->err = "undistort cut: the device reported an impossible count"; return SRL_ERR_HIP; }
    if (motion_compensation == SRL_MC_IMU && hw[W_NONMONO] == 1) host_walk = true;
    if (motion_compensation == SRL_MC_IMU && host_walk && n > 0) {
        // the guarded fallback: the walk itself, on the rewritten times, as srl_frame_undistort replays it
        P.fallbacks++;
        std::vector<double> rel((size_t)n);
        std::vector<int> seg((size_t)n);
        HIPCHK(ctx, hipMemcpyAsync(rel.data(), ctx->d_corr_rel, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        srl_imu_interval_walk(rel.data(), n, imu_states, n_states, time_begin, seg.data());
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_corr_seg, seg.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    if (n > 0) {
        rc = srl_undistort_launch(ctx, n, b_states.as<double>(), imu_states, n_states, time_begin, motion_compensation, R_il, t_il);
        if (rc) return rc;
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    ctx->corr_n = n;
    ctx->corr_from_cut = true;
    if (n_out) *n_out = n;
    return SRL_OK;
}

int srl_debug_undistorted_download(srl_ctx *ctx, double *uncorrected_xyz, double *imu_point, double *corrected_xyz, int32_t *interval, int capacity, int *n) {
    if (n) *n = 0;
    if (!ctx || capacity < 0) return SRL_ERR_BAD_ARG;
    if (ctx->nranks > 1) return SRL_ERR_UNSUPPORTED;
    SRL_DISARM(ctx);
    if (ctx->corr_n < 0) { ctx->err = "no undistorted sweep"; return SRL_ERR_NO_SWEEP; }
    const int m = ctx->corr_n;
    if (n) *n = m;
    if (capacity < m) { ctx->err = "undistorted download: capacity below the sweep's size"; return SRL_ERR_BAD_ARG; }
    if (m == 0) return SRL_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (uncorrected_xyz) HIPCHK(ctx, hipMemcpyAsync(uncorrected_xyz, ctx->d_corr_in, (size_t)m * 24, hipMemcpyDeviceToHost, st));
    if (imu_point) HIPCHK(ctx, hipMemcpyAsync(imu_point, ctx->d_corr_imu, (size_t)m * 24, hipMemcpyDeviceToHost, st));
    if (corrected_xyz) HIPCHK(ctx, hipMemcpyAsync(corrected_xyz, ctx->d_corr_raw, (size_t)m * 24, hipMemcpyDeviceToHost, st));
    if (interval) HIPCHK(ctx, hipMemcpyAsync(interval, ctx->d_corr_seg, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return SRL_OK;
}

int srl_frame_point_times(srl_ctx *ctx, const int32_t *index, int m, double *timestamp, double *relative_time, double *alpha_time) {
    if (!ctx || m < 0 || (m > 0 && !index)) return SRL_ERR_BAD_ARG;
    if (ctx->nranks > 1) return SRL_ERR_UNSUPPORTED;
    SRL_DISARM(ctx);
    if (!ctx->points || ctx->corr_n < 0 || !ctx->corr_from_cut) { ctx->err = "no sweep undistorted from a cut (srl_frame_undistort_cut first)"; return SRL_ERR_NO_SWEEP; }
    for (int k = 0; k < m; k++)
        if (index[k] < 0 || index[k] >= ctx->corr_n) { ctx->err = "point index out of range"; return SRL_ERR_BAD_ARG; }
    if (m == 0 || (!timestamp && !relative_time && !alpha_time)) return SRL_OK;
    const SrlPoints &P = *ctx->points;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf b_idx, b_out;
    HIPCHK(ctx, b_idx.alloc(ctx, (size_t)m * 4));
    HIPCHK(ctx, b_out.alloc(ctx, (size_t)m * 3 * sizeof(double)));
    HIPCHK(ctx, hipMemcpyAsync(b_idx.p, index, (size_t)m * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gather_times, grid256(m), dim3(256), 0, st, (const int *)b_idx.as<int>(), m, (const double *)P.t, (const double *)ctx->d_corr_rel,
                       (const double *)(P.t + P.t_cap), b_out.as<double>());
    HIPCHK(ctx, hipGetLastError());
    double *o = b_out.as<double>();
    if (timestamp) HIPCHK(ctx, hipMemcpyAsync(timestamp, o, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    if (relative_time) HIPCHK(ctx, hipMemcpyAsync(relative_time, o + m, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    if (alpha_time) HIPCHK(ctx, hipMemcpyAsync(alpha_time, o + 2 * (size_t)m, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return SRL_OK;
}

}  // extern "C"

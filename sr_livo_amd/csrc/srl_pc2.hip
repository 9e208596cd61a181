// srl_pc2.hip -- the second producer of the device point queue: sensor_msgs::PointCloud2 of the spinning LiDARs, decoded where the Livox
// records are (srl_points.hip), into the same FIFO.
//   srl_pc2_decode            cloudProcessing::process (cloudProcessing.cpp:100-123) with velodyneHandler (:325-433), ousterHandler (:216-323)
//                             and robosenseHandler (:435-542), statement by statement.  The message goes up once, as it is; every field is
//                             read where the layout says it lies (unaligned fields are assembled from bytes: RoboSense drivers put the
//                             double at offset 18).
//   given_offset_time = 1     time field -> order-preserving unsigned key -> stable sort of (key, message index) with srl_frame_scratch.h's
//                             radix passes -> flags in sorted order (the modulo pick, the blind test, timestamp > last_end_time) -> scan
//                             whose sink appends the five planes.  There is no validity filter in these handlers: every sorted position
//                             counts for the pick.
//   given_offset_time = 0     the yaw fallback for drivers without per-point time.  yaw = atan2(y, x) * 57.2957 IS COMPUTED ON THE HOST with
//                             libm (srl_pc2_layout.cpp) and uploaded beside the message: the reference's bits there are its libm's, and a
//                             device atan2 is a different function.  It is the one step that deliberately stays on the host.  On the
//                             device: the first point of every ring in message order by an integer atomicMin, relative_time and timestamp
//                             per point, a stable sort on the FP64 relative_time, the pick (no blind test in this branch), the append.
//   key maps                  uint32 t: itself.  float / double: -0.0 is rewritten to +0.0 (they compare equal under <), then all bits are
//                             flipped when the sign is set, else the sign bit is set: a < b as numbers <=> key(a) < key(b) as unsigned.
//                             A NaN key is refused (std::sort under < is undefined there).
//   64-bit keys               two stable 32-bit rounds, low word first; the high words are gathered through the first round's order
//                             between the rounds, and the second round carries that order as its values.
// Ties keep message order: this library's SPECIFICATION, as for Livox -- std::sort is not stable.  It weighs more here: every Ouster column
// shares one t, and in the yaw branch every ring's first point has relative_time 0.
// No floating-point atomic anywhere, and the two data-dependent refusals (a ring >= n_scans, a NaN key) are a word every offending thread
// sets to the same value: every call gives the same bytes.  The queue's size lives on the host: a refused call does not advance it.
// Built with -ffp-contract=off: every FP64 statement below is the reference's sequence of separately rounded operations.
#include "srl_ctx.h"
#include "srl_frame_scratch.h"
#include "srl_pc2_layout.h"
#include "srl_points_queue.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

static_assert(sizeof(srl_pc2_layout) == 40 && sizeof(srl_pc2_opts) == 32 && sizeof(srl_pc2_report) == 40, "ABI structs of srlivo_hip.h");
static_assert(W_WORDS * sizeof(int) + sizeof(srl_pc2_report) <= SRL_POINTS_WORD_BYTES, "the report record lies behind the words");

namespace {

// the message on the device, as srl_pc2_layout describes it
struct Pc2Msg {
    const unsigned char *data;
    unsigned width, point_step, row_step;
    int off_x, off_y, off_z, off_time, off_ring;
    int type;                          // SRL_LIDAR_VELO / _OUST / _ROBO
};
__device__ inline const unsigned char *d_point(const Pc2Msg &m, unsigned i) {
    return m.data + (size_t)(i / m.width) * m.row_step + (size_t)(i % m.width) * m.point_step;
}
// little-endian loads at any byte address: one aligned load where the address allows, else assembled from bytes (never a misaligned wide load)
__device__ inline unsigned d_ld16(const unsigned char *p) { return (unsigned)p[0] | ((unsigned)p[1] << 8); }
__device__ inline unsigned d_ld32(const unsigned char *p) {
    if (((size_t)p & 3u) == 0) return *reinterpret_cast<const unsigned *>(p);
    return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
}
__device__ inline unsigned long long d_ld64(const unsigned char *p) { return (unsigned long long)d_ld32(p) | ((unsigned long long)d_ld32(p + 4) << 32); }
__device__ inline unsigned d_ring(const Pc2Msg &m, const unsigned char *p) { return m.type == SRL_LIDAR_OUST ? (unsigned)p[m.off_ring] : d_ld16(p + m.off_ring); }
// the time field as the reference's expressions widen it: double(float time), double(uint32 t), the double timestamp
__device__ inline double d_time(const Pc2Msg &m, const unsigned char *p) {
    if (m.type == SRL_LIDAR_VELO) return (double)__uint_as_float(d_ld32(p + m.off_time));
    if (m.type == SRL_LIDAR_OUST) return (double)d_ld32(p + m.off_time);
    return __longlong_as_double((long long)d_ld64(p + m.off_time));
}
__device__ inline unsigned d_key_f32(unsigned u) {
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline unsigned long long d_key_f64(unsigned long long u) {
    if (u == 0x8000000000000000ull) u = 0ull;
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline bool d_nan_f32(unsigned u) { return (u & 0x7FFFFFFFu) > 0x7F800000u; }
__device__ inline bool d_nan_f64(unsigned long long u) { return (u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }

// ---------------------------------------------------------------------------------------------------------------- given_offset_time = 1
// sort keys of the time field by message index: lo (and hi for the double); a NaN time raises W_BAD
__global__ void k_pc2_time_keys(Pc2Msg m, int n, unsigned *lo, unsigned *hi, int *words) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned char *p = d_point(m, (unsigned)i);
    if (m.type == SRL_LIDAR_OUST) {
        lo[i] = d_ld32(p + m.off_time);
    } else if (m.type == SRL_LIDAR_VELO) {
        const unsigned u = d_ld32(p + m.off_time);
        if (d_nan_f32(u)) words[W_BAD] = 1;
        lo[i] = d_key_f32(u);
    } else {
        const unsigned long long u = d_ld64(p + m.off_time);
        if (d_nan_f64(u)) words[W_BAD] = 1;
        const unsigned long long k = d_key_f64(u);
        lo[i] = (unsigned)k;
        hi[i] = (unsigned)(k >> 32);
    }
}

// ---------------------------------------------------------------------------------------------------------------- given_offset_time = 0
// cloudProcessing.cpp:262-268: is_first[layer] in message order = the smallest message index of the ring
__global__ void k_pc2_ring_first(Pc2Msg m, int n, int n_scans, unsigned *first, int *words) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned ring = d_ring(m, d_point(m, (unsigned)i));
    if (ring >= (unsigned)n_scans) { words[W_BAD] = 1; return; }       // yaw_first_point[layer] out of bounds upstream
    atomicMin(&first[ring], (unsigned)i);
}
// :263-285 for message index i, and the sort key of its relative_time
__global__ void k_pc2_yaw_times(Pc2Msg m, int n, int n_scans, const unsigned *first, const double *yaw, double omega, double stamp, double *rel, double *ts,
                                unsigned *lo, unsigned *hi, int *words) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned ring = d_ring(m, d_point(m, (unsigned)i));
    double r = 0.0, t = 0.0;           // a ring's first point: relative_time = 0.0, and the timestamp point3D() starts with
    if (ring < (unsigned)n_scans) {
        const unsigned f = first[ring];
        if (f != (unsigned)i) {
            const double yaw_first = yaw[f], yaw_angle = yaw[i];
            if (yaw_angle <= yaw_first) r = (yaw_first - yaw_angle) / omega;
            else r = (yaw_first - yaw_angle + 360.0) / omega;
            t = r / 1000.0 + stamp;
        }
    }
    const unsigned long long u = (unsigned long long)__double_as_longlong(r);
    if (d_nan_f64(u)) words[W_BAD] = 1;
    const unsigned long long k = d_key_f64(u);
    rel[i] = r; ts[i] = t;
    lo[i] = (unsigned)k;
    hi[i] = (unsigned)(k >> 32);
}

__global__ void k_pc2_gather(const unsigned *src, const unsigned *order, int n, unsigned *dst) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) dst[j] = src[order[j]];
}

// ---------------------------------------------------------------------------------------------------------------- pick and append
// the record of sorted position j
struct Pc2Src {
    Pc2Msg m;
    const unsigned *order;             // sorted message indices
    int n;
    double scale, stamp;
    const double *rel, *ts;            // yaw branch: by message index; given branch: nullptr
};
struct Pc2Rec { double x, y, z, rel, ts; };
__device__ inline Pc2Rec d_pc2_record(const Pc2Src &s, int j) {
    const unsigned i = s.order[j];
    const unsigned char *p = d_point(s.m, i);
    Pc2Rec r;
    r.x = (double)__uint_as_float(d_ld32(p + s.m.off_x));
    r.y = (double)__uint_as_float(d_ld32(p + s.m.off_y));
    r.z = (double)__uint_as_float(d_ld32(p + s.m.off_z));
    if (s.rel) {
        r.rel = s.rel[i]; r.ts = s.ts[i];
    } else {
        const double t = d_time(s.m, p);
        // robosenseHandler :477: against .front() of the SORTED cloud
        if (s.m.type == SRL_LIDAR_ROBO) r.rel = (t - d_time(s.m, d_point(s.m, s.order[0]))) * s.scale;
        else r.rel = t * s.scale;
        r.ts = r.rel / 1000.0 + s.stamp;
    }
    return r;
}
__global__ void k_pc2_flag(Pc2Src s, int pfn, int use_blind, double blind2, double last_end_time, int *flag) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= s.n) return;
    int keep = 0;
    if (j % pfn == 0) {
        const Pc2Rec r = d_pc2_record(s, j);
        keep = (!use_blind || (r.x * r.x + r.y * r.y) + r.z * r.z > blind2) && r.ts > last_end_time ? 1 : 0;
    }
    flag[j] = keep;
}
struct SinkPc2Append {
    Pc2Src s;
    double *tail;                      // queue plane 0 at the first free record
    int stride;
    int *words;
    __device__ void operator()(int j, int v, int excl) const {
        if (v) {
            const Pc2Rec r = d_pc2_record(s, j);
            tail[(size_t)PL_X * stride + excl] = r.x;
            tail[(size_t)PL_Y * stride + excl] = r.y;
            tail[(size_t)PL_Z * stride + excl] = r.z;
            tail[(size_t)PL_REL * stride + excl] = r.rel;
            tail[(size_t)PL_TS * stride + excl] = r.ts;
        }
        if (j == s.n - 1) words[W_APPENDED] = excl + v;
    }
};
__global__ void k_pc2_report(int *words, Pc2Src s, int pfn, int given, const double *tail_ts) {
    srl_pc2_report *r = reinterpret_cast<srl_pc2_report *>(words + W_WORDS);
    const int app = words[W_APPENDED];
    const unsigned last = s.order[s.n - 1];
    // :237 / :346 / :456 (for ROBO the absolute timestamp, as the reference has it) and :307 / :417 / :526
    const double dt_last_point = given ? d_time(s.m, d_point(s.m, last)) * s.scale : s.rel[last];
    r->points = s.n; r->given_offset_time = given; r->picked = (s.n + pfn - 1) / pfn; r->appended = app;
    r->last_end_time = s.stamp + dt_last_point / 1000.0;
    r->first_timestamp = app > 0 ? tail_ts[0] : d_nan();
    r->last_timestamp = app > 0 ? tail_ts[app - 1] : d_nan();
}

}  // namespace

extern "C" int srl_pc2_decode(srl_ctx *ctx, const void *data, size_t data_bytes, const srl_pc2_layout *layout, double header_stamp, double last_end_time,
                              const srl_pc2_opts *opts, srl_pc2_report *report) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (report) { std::memset(report, 0, sizeof *report); report->last_end_time = report->first_timestamp = report->last_timestamp = nan; }
    if (!ctx || !layout || !opts || !data) return SRL_ERR_BAD_ARG;
    if (opts->point_filter_num < 1 || !(opts->time_unit_scale > 0.0) || std::isinf(opts->time_unit_scale) || std::isnan(opts->blind) || std::isnan(header_stamp) ||
        std::isnan(last_end_time))
        return SRL_ERR_BAD_ARG;
    if (srl_pc2_time_bytes(opts->lidar_type) == 0) return SRL_ERR_BAD_ARG;          // LIVOX has srl_livox_decode; anything else is no LiDAR of the reference
    uint64_t n64 = 0;
    if (srl_pc2_layout_check(layout, opts->lidar_type, data_bytes, &n64) != SRL_OK) return SRL_ERR_BAD_ARG;
    if (n64 > (uint64_t)SRL_SCAN_MAX) { ctx->err = "a PointCloud2 message of more than 2^20 points"; return SRL_ERR_UNSUPPORTED; }
    if (ctx->nranks > 1) { ctx->err = "the point queue is not sharded"; return SRL_ERR_UNSUPPORTED; }
    const int n = (int)n64, type = opts->lidar_type, pfn = opts->point_filter_num;
    const unsigned char *bytes = static_cast<const unsigned char *>(data);
    // the branch: the time field of the last point in message order, before any sort (:229, :338, :448)
    int given = 0;
    if (n > 0) {
        const unsigned char *p = bytes + srl_pc2_point_offset(*layout, (uint64_t)n - 1) + layout->off_time;
        if (type == SRL_LIDAR_VELO) { float t; std::memcpy(&t, p, 4); given = t > 0 ? 1 : 0; }
        else if (type == SRL_LIDAR_OUST) { uint32_t t; std::memcpy(&t, p, 4); given = t > 0 ? 1 : 0; }
        else { double t; std::memcpy(&t, p, 8); given = t > 0 ? 1 : 0; }
    }
    if (n > 0 && !given && (opts->scan_rate <= 0 || opts->n_scans < 1)) return SRL_ERR_BAD_ARG;
    SRL_DISARM(ctx);
    if (!ctx->points) ctx->points = new SrlPoints();
    SrlPoints &P = *ctx->points;
    if (n == 0) return SRL_OK;         // :224-227: the handler returns before it assigns last_end_time
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = points_words(ctx, P);
    if (rc) return rc;
    const int picked = (n + pfn - 1) / pfn;
    rc = points_reserve(ctx, P, picked);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    const bool wide = !given || type == SRL_LIDAR_ROBO;                // a 64-bit key
    const size_t msg_bytes = srl_pc2_point_offset(*layout, (uint64_t)n - 1) + layout->point_step;
    DevBuf b_msg, b_lo, b_hi, b_ks, b_vs, b_tk, b_tv, b_hi1, b_vs2, b_flag, b_sc, b_yaw, b_rel, b_ts, b_first;
    HIPCHK(ctx, b_msg.alloc(ctx, msg_bytes));
    for (DevBuf *b : {&b_lo, &b_ks, &b_vs, &b_tk, &b_tv, &b_flag}) HIPCHK(ctx, b->alloc(ctx, (size_t)n * 4));
    if (wide) for (DevBuf *b : {&b_hi, &b_hi1, &b_vs2}) HIPCHK(ctx, b->alloc(ctx, (size_t)n * 4));
    HIPCHK(ctx, b_sc.alloc(ctx, std::max(srl_radix_scratch_ints(n), srl_scan_scratch_ints(n)) * 4));
    HIPCHK(ctx, hipMemcpyAsync(b_msg.p, data, msg_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(P.d_words, 0, SRL_POINTS_WORD_BYTES, st));
    const Pc2Msg m = {b_msg.as<unsigned char>(), layout->width, layout->point_step, layout->row_step, layout->off_x, layout->off_y, layout->off_z, layout->off_time,
                      layout->off_ring, type};
    unsigned *lo = b_lo.as<unsigned>(), *hi = wide ? b_hi.as<unsigned>() : nullptr;
    std::vector<double> yaw;
    if (given) {
        hipLaunchKernelGGL(k_pc2_time_keys, grid256(n), dim3(256), 0, st, m, n, lo, hi, P.d_words);
    } else {
        // ring < n_scans and a ring is at most 16 bits wide: the table never needs more than 65 536 entries
        const int table = std::min(opts->n_scans, 65536);
        yaw.resize((size_t)n);
        rc = srl_pc2_yaw_angles(data, data_bytes, layout, yaw.data());
        if (rc) return rc;
        HIPCHK(ctx, b_yaw.alloc(ctx, (size_t)n * 8));
        HIPCHK(ctx, b_rel.alloc(ctx, (size_t)n * 8));
        HIPCHK(ctx, b_ts.alloc(ctx, (size_t)n * 8));
        HIPCHK(ctx, b_first.alloc(ctx, (size_t)table * 4));
        HIPCHK(ctx, hipMemcpyAsync(b_yaw.p, yaw.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemsetAsync(b_first.p, 0xFF, (size_t)table * 4, st));
        hipLaunchKernelGGL(k_pc2_ring_first, grid256(n), dim3(256), 0, st, m, n, (int)opts->n_scans, b_first.as<unsigned>(), P.d_words);
        hipLaunchKernelGGL(k_pc2_yaw_times, grid256(n), dim3(256), 0, st, m, n, (int)opts->n_scans, (const unsigned *)b_first.as<unsigned>(),
                           (const double *)b_yaw.as<double>(), 0.361 * opts->scan_rate, header_stamp, b_rel.as<double>(), b_ts.as<double>(), lo, hi, P.d_words);
    }
    // all 32 bits of a word: four passes of eight, as for the Livox offsets
    srl_radix_sort_pairs(lo, nullptr, b_ks.as<unsigned>(), b_vs.as<unsigned>(), b_tk.as<unsigned>(), b_tv.as<unsigned>(), n, 32u, st, b_sc.as<int>());
    const unsigned *order = b_vs.as<unsigned>();
    if (wide) {
        hipLaunchKernelGGL(k_pc2_gather, grid256(n), dim3(256), 0, st, (const unsigned *)hi, order, n, b_hi1.as<unsigned>());
        // the second round reads (high word, first round's order) and may write its sorted keys over the low words: they are done with
        srl_radix_sort_pairs(b_hi1.as<unsigned>(), order, lo, b_vs2.as<unsigned>(), b_tk.as<unsigned>(), b_tv.as<unsigned>(), n, 32u, st, b_sc.as<int>());
        order = b_vs2.as<unsigned>();
    }
    const Pc2Src src = {m, order, n, opts->time_unit_scale, header_stamp, given ? nullptr : b_rel.as<double>(), given ? nullptr : b_ts.as<double>()};
    hipLaunchKernelGGL(k_pc2_flag, grid256(n), dim3(256), 0, st, src, pfn, given, opts->blind * opts->blind, last_end_time, b_flag.as<int>());
    double *tail = P.q + P.head + P.size;
    const SinkPc2Append app = {src, tail, P.cap, P.d_words};
    srl_scan(SrlIntArrayIn{b_flag.as<int>()}, app, n, b_sc.as<int>(), st);
    hipLaunchKernelGGL(k_pc2_report, dim3(1), dim3(1), 0, st, P.d_words, src, pfn, given, (const double *)(tail + (size_t)PL_TS * P.cap));
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(P.h_words, P.d_words, SRL_POINTS_WORD_BYTES, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    int bad;
    std::memcpy(&bad, P.h_words + W_BAD * sizeof(int), sizeof bad);
    if (bad) {
        ctx->err = given ? "PointCloud2 decode: a NaN time (no order under <)" : "PointCloud2 decode: a ring >= n_scans or a NaN relative_time";
        return SRL_ERR_BAD_ARG;        // the records written behind the queue's back are not part of it: the size did not move
    }
    srl_pc2_report r;
    std::memcpy(&r, P.h_words + W_WORDS * sizeof(int), sizeof r);
    if (r.appended < 0 || r.appended > picked) { ctx->err = "PointCloud2 decode: the device reported an impossible count"; return SRL_ERR_HIP; }
    if (r.appended > 0) {
        if (P.size == 0) P.front_ts = r.first_timestamp;
        P.back_ts = r.last_timestamp;
        P.size += r.appended;
    }
    if (report) *report = r;
    return SRL_OK;
}

// srl_consensus.hip -- consensus outlier rejection of the camera tracker on the device for gfx950: a deterministic hypothesis-parallel
// RANSAC for the two places where the reference calls OpenCV and reads nothing but the inlier set,
//   cv::findFundamentalMat(last, cur, FM_RANSAC, 1.0, 0.997, status)         (opticalFlowTracker.cpp:144)  -> srl_consensus_fundamental
//   cv::solvePnPRansac(points_3d, points_2d, intrinsic, ..., 200, 1.5, 0.99)  (opticalFlowTracker.cpp:295)  -> srl_consensus_pnp
// These are NOT OpenCV's results: OpenCV's masks depend on its private generator.  What is specified here instead (include/srlivo_hip.h)
// is a function of (inputs, options) alone, checkable by its properties.
//
//   k_cons_prep   one workgroup: the list of usable points (every coordinate finite) in ascending order by ordered ballot compaction, and,
//                 for the fundamental model, Hartley's normalisation of both views (centroid, sqrt 2 / mean distance), computed ONCE: the
//                 sums are per-thread strided partial sums folded by a fixed tree in LDS (no floating-point atomics: same bits every call).
//   k_cons_hyp    one LANE per hypothesis.  The lane draws its minimal sample with the counter-based generator of srl_consensus_math.h:
//                   draw(seed, h, k, m) = (mix64(((seed << 32) | h) * 0x9E3779B97F4A7C15 + (k + 1) * 0xBF58476D1CE4E5B9) >> 32) * m >> 32,
//                 mix64 = the splitmix64 finaliser; k = 0, 1, ... and a draw that repeats an earlier position is rejected (64 draws at most).
//                 Positions index the usable list, so a non-finite point is never sampled.  Then the minimal problem in FP64:
//                 fundamental: 7-point -- the 7 x 9 system of the normalised points reduced by Gauss-Jordan elimination with complete pivoting
//                   (the lanes' systems interleaved in LDS, 81 doubles a lane: runtime-indexed rows never sit in registers), its two null
//                   vectors, the cubic det(a F1 + (1 - a) F2) = 0, up to 3 real roots, each de-normalised and scaled to unit Frobenius norm;
//                 PnP: P3P -- Grunert's quartic (Haralick et al. 1994) on bearings normalised by the intrinsics, every real root refined on
//                   the three distance equations; all of up to 4 solutions with positive depth at the three points are kept as R, t.
//                 A degenerate sample yields no model; every model slot carries a validity flag.
//   k_cons_score  one WAVE per candidate model (model = hypothesis * slots + slot), four to a workgroup.  The points are staged through LDS in
//                 chunks of 1024 (each point once per workgroup); lanes stride over a chunk and the count grows by popcount(ballot).
//   k_cons_pick   one workgroup: the valid model with the largest count, ties to the lowest model index; it is scored again by the same
//                 function, which writes the n-byte mask, the ascending inlier list (ordered ballot compaction) and the result record.
// No stage waits for the host: the four kernels and the copies are enqueued back to back, and the workspace (one device block, one
// page-locked block, sized for the limits) is allocated at the context's first call and freed with the context.
//
// Bounds: k_cons_hyp writes models [0, H * slots), flags likewise, samples [0, 8 H): the workspace holds SRL_CONSENSUS_MAX_HYPOTHESES * 4
// models.  The compactions write at most as many entries as points flagged, <= n <= SRL_CONSENSUS_MAX_POINTS.  LDS of k_cons_hyp<F>:
// 64 lanes x 81 doubles, lane-interleaved (element e of lane l at [e * 64 + l]).
#include "srl_ctx.h"
#include "../../include/srlivo_hip_debug.h"
#include "srl_consensus_math.h"

#include <cmath>
#include <cstring>

#define CONS_F SRL_CONSENSUS_FUNDAMENTAL
#define CONS_P SRL_CONSENSUS_PNP
#define CONS_CHUNK 1024                    // points staged per LDS chunk by k_cons_score
#define CONS_MAX_SLOTS 4

struct SrlConsensus {
    char *d_block = nullptr, *h_block = nullptr;
    // device
    float *d_pts = nullptr;                // MAX_POINTS x 5
    int *d_usable = nullptr;               // MAX_POINTS
    double *d_norm = nullptr;              // 8: mx1, my1, s1, mx2, my2, s2, -, -
    int *d_nusable = nullptr;              // 2
    double *d_models = nullptr;            // MAX_HYPOTHESES x 4 x 12
    int *d_flags = nullptr;                // MAX_HYPOTHESES x 4: validity, then (k_cons_score) the count, -1 = no model
    int *d_samples = nullptr;              // MAX_HYPOTHESES x 8
    unsigned char *d_mask = nullptr;       // MAX_POINTS
    int *d_list = nullptr;                 // MAX_POINTS
    srl_consensus_result *d_res = nullptr;
    // page-locked
    float *h_pts = nullptr;
    unsigned char *h_mask = nullptr;
    int *h_list = nullptr;
    srl_consensus_result *h_res = nullptr;
    // the last call that ran on the workspace (srl_debug_consensus_download): its model (-1: none yet), hypotheses and points
    int last_model = -1, last_H = 0, last_n = 0;
};

namespace {

template <int MODEL> struct ConsTraits;
template <> struct ConsTraits<CONS_F> { static constexpr int S = 7, SLOTS = 3, FPP = 4; };
template <> struct ConsTraits<CONS_P> { static constexpr int S = 3, SLOTS = 4, FPP = 5; };

struct ConsArgs {
    const float *pts;
    int n, H;
    unsigned seed;
    double thr2, confidence;
    double K[4];
};

template <int MODEL>
__device__ __forceinline__ bool cons_inlier(const double *M, const double *K, const float *p, double thr2) {
    if (MODEL == CONS_F) return cons_inlier_fundamental(M, (double)p[0], (double)p[1], (double)p[2], (double)p[3], thr2);
    return cons_inlier_pnp(M, K, (double)p[0], (double)p[1], (double)p[2], (double)p[3], (double)p[4], thr2);
}

// every thread of a 256-thread workgroup calls this; the flagged values are appended to list in thread order.  s_wave: 4 ints of LDS
__device__ __forceinline__ void cons_append_ordered(bool flag, int value, int *list, int &base, int *s_wave) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) s_wave[w] = __popcll(b);
    __syncthreads();
    int off = base;
    for (int k = 0; k < 4; k++) if (k < w) off += s_wave[k];
    if (flag) list[off + __popcll(b & ((1ull << lane) - 1ull))] = value;
    base += (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
    __syncthreads();
}

// the sum over the workgroup's 256 threads of NV values each, by a fixed tree: the same bits on every call
template <int NV>
__device__ __forceinline__ void cons_block_sum(double *v, double *s_red /* 256 x NV */) {
    const int t = threadIdx.x;
    for (int k = 0; k < NV; k++) s_red[k * 256 + t] = v[k];
    __syncthreads();
    for (int step = 128; step >= 1; step >>= 1) {
        if (t < step) for (int k = 0; k < NV; k++) s_red[k * 256 + t] += s_red[k * 256 + t + step];
        __syncthreads();
    }
    for (int k = 0; k < NV; k++) v[k] = s_red[k * 256];
    __syncthreads();
}

template <int MODEL>
__global__ void __launch_bounds__(256) k_cons_prep(ConsArgs A, int *usable, int *nusable, double *norm) {
    constexpr int FPP = ConsTraits<MODEL>::FPP;
    __shared__ int s_wave[4];
    __shared__ double s_red[256 * 4];
    const int t = threadIdx.x;
    int base = 0;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int tile = 0; tile < A.n; tile += 256) {
        const int i = tile + t;
        bool ok = i < A.n;
        if (ok) for (int k = 0; k < FPP; k++) ok = ok && isfinite(A.pts[(size_t)i * FPP + k]);
        if (MODEL == CONS_F && ok) for (int k = 0; k < 4; k++) sum[k] += (double)A.pts[(size_t)i * 4 + k];
        cons_append_ordered(ok, i, usable, base, s_wave);
    }
    if (t == 0) nusable[0] = base;
    if (MODEL != CONS_F) return;
    cons_block_sum<4>(sum, s_red);
    double mean[4] = {0.0, 0.0, 0.0, 0.0};
    if (base > 0) for (int k = 0; k < 4; k++) mean[k] = sum[k] / (double)base;
    __syncthreads();                       // the usable list is read below by other threads than wrote it
    double dist[2] = {0.0, 0.0};
    for (int j = t; j < base; j += 256) {
        const float *p = A.pts + (size_t)usable[j] * 4;
        const double a = (double)p[0] - mean[0], b = (double)p[1] - mean[1], c = (double)p[2] - mean[2], d = (double)p[3] - mean[3];
        dist[0] += sqrt(a * a + b * b);
        dist[1] += sqrt(c * c + d * d);
    }
    cons_block_sum<2>(dist, s_red);
    if (t == 0) {
        // a view whose points coincide keeps scale 1: every sample of it is degenerate anyway
        const double s1 = dist[0] > 0.0 ? 1.4142135623730951 * (double)base / dist[0] : 1.0;
        const double s2 = dist[1] > 0.0 ? 1.4142135623730951 * (double)base / dist[1] : 1.0;
        norm[0] = mean[0]; norm[1] = mean[1]; norm[2] = isfinite(s1) ? s1 : 1.0;
        norm[3] = mean[2]; norm[4] = mean[3]; norm[5] = isfinite(s2) ? s2 : 1.0;
    }
}

template <int MODEL>
__global__ void __launch_bounds__(64) k_cons_hyp(ConsArgs A, const int *usable, const int *nusable, const double *norm, double *models, int *flags,
                                                 int *samples) {
    constexpr int S = ConsTraits<MODEL>::S, SLOTS = ConsTraits<MODEL>::SLOTS;
    __shared__ double s_W[MODEL == CONS_F ? 81 * 64 : 1];
    const int lane = threadIdx.x, h = blockIdx.x * 64 + lane;
    if (h >= A.H) return;
    double *out = models + (size_t)h * SLOTS * 12;
    int pos[S], idx[8];
    const bool sampled = cons_sample<S>(A.seed, (unsigned)h, nusable[0], pos);
    for (int k = 0; k < 8; k++) idx[k] = -1;
    if (sampled) for (int k = 0; k < S; k++) idx[k] = usable[pos[k]];
    for (int k = 0; k < 8; k++) samples[(size_t)h * 8 + k] = idx[k];
    int nm = 0;
    if (MODEL == CONS_F) {
        double N[6];
        for (int k = 0; k < 6; k++) N[k] = norm[k];
        double *W = s_W + lane;
        bool ok = sampled;
        if (ok) {
            for (int r = 0; r < 7; r++) {
                const float *p = A.pts + (size_t)idx[r] * 4;
                const double x1 = N[2] * ((double)p[0] - N[0]), y1 = N[2] * ((double)p[1] - N[1]);
                const double x2 = N[5] * ((double)p[2] - N[3]), y2 = N[5] * ((double)p[3] - N[4]);
                double *row = W + r * 9 * 64;
                row[0] = x2 * x1; row[64] = x2 * y1; row[128] = x2; row[192] = y2 * x1; row[256] = y2 * y1; row[320] = y2;
                row[384] = x1; row[448] = y1; row[512] = 1.0;
            }
            ok = cons_nullspace_7x9(W, 64);
        }
        if (ok) {
            double F1[9], F2[9], c[4], root[3];
            for (int k = 0; k < 9; k++) { F1[k] = W[(63 + k) * 64]; F2[k] = W[(72 + k) * 64]; }
            cons_det_cubic(F1, F2, c);
            cons_cubic(c, root);
            for (int m = 0; m < 3; m++) {
                if (!isfinite(root[m])) continue;
                double Fn[9], F[9];
                for (int k = 0; k < 9; k++) Fn[k] = root[m] * F1[k] + (1.0 - root[m]) * F2[k];
                if (!cons_denormalise(Fn, N, F)) continue;
                for (int k = 0; k < 9; k++) out[nm * 12 + k] = F[k];
                for (int k = 9; k < 12; k++) out[nm * 12 + k] = 0.0;
                nm++;
            }
        }
    } else {
        if (sampled) {
            double P[9], J[9];
            for (int r = 0; r < 3; r++) {
                const float *p = A.pts + (size_t)idx[r] * 5;
                for (int k = 0; k < 3; k++) P[3 * r + k] = (double)p[k];
                const double bx = ((double)p[3] - A.K[2]) / A.K[0], by = ((double)p[4] - A.K[3]) / A.K[1];
                const double nb = sqrt((bx * bx + by * by) + 1.0);
                J[3 * r] = bx / nb; J[3 * r + 1] = by / nb; J[3 * r + 2] = 1.0 / nb;
            }
            nm = cons_p3p(P, J, out);           // every accepted pose goes straight to its slot
        }
    }
    for (int m = 0; m < SLOTS; m++) {
        flags[(size_t)h * SLOTS + m] = m < nm ? 1 : 0;
        if (m >= nm) for (int k = 0; k < 12; k++) out[m * 12 + k] = 0.0;
    }
}

template <int MODEL>
__global__ void __launch_bounds__(256) k_cons_score(ConsArgs A, const double *models, int *flags) {
    constexpr int SLOTS = ConsTraits<MODEL>::SLOTS, FPP = ConsTraits<MODEL>::FPP;
    __shared__ float s_pts[CONS_CHUNK * FPP];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int M = A.H * SLOTS, m = blockIdx.x * 4 + w;
    const bool live = m < M && flags[m] != 0;                  // uniform in the wave
    double Mo[12];
    for (int k = 0; k < 12; k++) Mo[k] = live ? models[(size_t)m * 12 + k] : 0.0;
    int count = 0;
    for (int at = 0; at < A.n; at += CONS_CHUNK) {
        const int cn = A.n - at < CONS_CHUNK ? A.n - at : CONS_CHUNK;
        for (int e = threadIdx.x; e < cn * FPP; e += 256) s_pts[e] = A.pts[(size_t)at * FPP + e];
        __syncthreads();
        if (live)
            for (int b = 0; b < cn; b += 64) {
                const int i = b + lane;
                const bool in = i < cn && cons_inlier<MODEL>(Mo, A.K, s_pts + (i < cn ? i : 0) * FPP, A.thr2);
                count += __popcll(__ballot(in));
            }
        __syncthreads();
    }
    if (lane == 0 && m < M) flags[m] = live ? count : -1;
}

template <int MODEL>
__global__ void __launch_bounds__(256) k_cons_pick(ConsArgs A, const double *models, const int *counts, const int *samples, unsigned char *mask, int *list,
                                                   srl_consensus_result *res) {
    constexpr int S = ConsTraits<MODEL>::S, SLOTS = ConsTraits<MODEL>::SLOTS, FPP = ConsTraits<MODEL>::FPP;
    __shared__ int s_cnt[256], s_idx[256], s_valid[256], s_wave[4];
    const int t = threadIdx.x, M = A.H * SLOTS;
    int best = -1, bidx = 0x7fffffff, valid = 0;
    for (int m = t; m < M; m += 256) {                         // ascending: a later model must be strictly better
        const int c = counts[m];
        valid += c >= 0 ? 1 : 0;
        if (c > best) { best = c; bidx = m; }
    }
    s_cnt[t] = best; s_idx[t] = bidx; s_valid[t] = valid;
    __syncthreads();
    for (int step = 128; step >= 1; step >>= 1) {
        if (t < step) {
            const int c = s_cnt[t + step], i = s_idx[t + step];
            if (c > s_cnt[t] || (c == s_cnt[t] && i < s_idx[t])) { s_cnt[t] = c; s_idx[t] = i; }
            s_valid[t] += s_valid[t + step];
        }
        __syncthreads();
    }
    best = s_cnt[0]; bidx = s_idx[0]; valid = s_valid[0];
    const bool have = best >= 0;
    double Mo[12];
    for (int k = 0; k < 12; k++) Mo[k] = have ? models[(size_t)bidx * 12 + k] : 0.0;
    int base = 0;
    for (int tile = 0; tile < A.n; tile += 256) {
        const int i = tile + t;
        const bool in = have && i < A.n && cons_inlier<MODEL>(Mo, A.K, A.pts + (size_t)(i < A.n ? i : 0) * FPP, A.thr2);
        if (i < A.n) mask[i] = in ? 1 : 0;
        cons_append_ordered(in, i, list, base, s_wave);
    }
    if (t == 0) {
        for (int k = 0; k < 12; k++) res->model[k] = Mo[k];
        for (int k = 0; k < 8; k++) res->sample[k] = have ? samples[(size_t)(bidx / SLOTS) * 8 + k] : -1;
        res->hypothesis = have ? bidx / SLOTS : -1;
        res->slot = have ? bidx % SLOTS : -1;
        res->inliers = base;
        res->models_valid = valid;
        // 1 - (1 - w^S)^H >= confidence, by repeated multiplication
        const double wgt = A.n > 0 ? (double)base / (double)A.n : 0.0;
        double ws = 1.0, miss = 1.0;
        for (int k = 0; k < S; k++) ws *= wgt;
        for (int k = 0; k < A.H; k++) miss *= 1.0 - ws;
        res->confidence_reached = have && 1.0 - miss >= A.confidence ? 1 : 0;
        res->reserved = 0;
    }
}

// the pieces of the two blocks, sized for the limits (blocks not allocated yet: the pieces are null, and the sizes are all there is)
void cons_layout(SrlConsensus *c, size_t *d_bytes, size_t *h_bytes) {
    const size_t P = SRL_CONSENSUS_MAX_POINTS, H = SRL_CONSENSUS_MAX_HYPOTHESES, HM = H * CONS_MAX_SLOTS;
    SrlCarve v{c->d_block}, w{c->h_block};
    c->d_pts = v.take<float>(P * 5); c->d_usable = v.take<int>(P); c->d_norm = v.take<double>(8); c->d_nusable = v.take<int>(2);
    c->d_models = v.take<double>(HM * 12); c->d_flags = v.take<int>(HM); c->d_samples = v.take<int>(H * 8);
    c->d_mask = v.take<unsigned char>(P); c->d_list = v.take<int>(P); c->d_res = v.take<srl_consensus_result>(1);
    c->h_pts = w.take<float>(P * 5); c->h_mask = w.take<unsigned char>(P); c->h_list = w.take<int>(P); c->h_res = w.take<srl_consensus_result>(1);
    *d_bytes = v.at; *h_bytes = w.at;
}

int cons_workspace(srl_ctx *ctx) {
    if (ctx->consensus) return SRL_OK;
    SrlConsensus *c = new SrlConsensus();
    size_t d_bytes, h_bytes;
    cons_layout(c, &d_bytes, &h_bytes);
    hipError_t e = hipMalloc((void **)&c->d_block, d_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&c->h_block, h_bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        if (c->d_block) hipFree(c->d_block);
        delete c;
        HIPCHK(ctx, e);
    }
    cons_layout(c, &d_bytes, &h_bytes);
    ctx->consensus = c;
    return SRL_OK;
}

void cons_empty_result(srl_consensus_result *r) {
    std::memset(r, 0, sizeof *r);
    for (int k = 0; k < 8; k++) r->sample[k] = -1;
    r->hypothesis = -1; r->slot = -1;
}

bool cons_opts_ok(const srl_consensus_opts *o) {
    return std::isfinite(o->threshold) && o->threshold > 0.0 && o->confidence > 0.0 && o->confidence < 1.0 && o->hypotheses >= 1 &&
           o->hypotheses <= SRL_CONSENSUS_MAX_HYPOTHESES;
}

// the points are in c->h_pts; everything from the upload to the three downloads is enqueued without a wait in between
template <int MODEL>
int cons_run(srl_ctx *ctx, int n, const srl_consensus_opts *o, const double *K) {
    constexpr int SLOTS = ConsTraits<MODEL>::SLOTS, FPP = ConsTraits<MODEL>::FPP;
    SrlConsensus *c = ctx->consensus;
    hipStream_t st = ctx->stream;
    ConsArgs A;
    A.pts = c->d_pts; A.n = n; A.H = o->hypotheses; A.seed = o->seed; A.thr2 = o->threshold * o->threshold; A.confidence = o->confidence;
    for (int k = 0; k < 4; k++) A.K[k] = K ? K[k] : 0.0;
    c->last_model = -1;                    // a call that fails half way leaves nothing to read back
    HIPCHK(ctx, hipMemcpyAsync(c->d_pts, c->h_pts, (size_t)n * FPP * sizeof(float), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_cons_prep<MODEL>, dim3(1), dim3(256), 0, st, A, c->d_usable, c->d_nusable, c->d_norm);
    hipLaunchKernelGGL(k_cons_hyp<MODEL>, dim3((unsigned)((A.H + 63) / 64)), dim3(64), 0, st, A, (const int *)c->d_usable, (const int *)c->d_nusable,
                       (const double *)c->d_norm, c->d_models, c->d_flags, c->d_samples);
    hipLaunchKernelGGL(k_cons_score<MODEL>, dim3((unsigned)((A.H * SLOTS + 3) / 4)), dim3(256), 0, st, A, (const double *)c->d_models, c->d_flags);
    hipLaunchKernelGGL(k_cons_pick<MODEL>, dim3(1), dim3(256), 0, st, A, (const double *)c->d_models, (const int *)c->d_flags, (const int *)c->d_samples,
                       c->d_mask, c->d_list, c->d_res);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(c->h_mask, c->d_mask, (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(c->h_list, c->d_list, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(c->h_res, c->d_res, sizeof(srl_consensus_result), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    c->last_model = MODEL; c->last_H = A.H; c->last_n = n;
    return SRL_OK;
}

}  // namespace

extern "C" int srl_debug_consensus_download(srl_ctx *ctx, srl_debug_consensus_info *info, int32_t *usable, int64_t point_capacity, int32_t *samples,
                                            double *models, int32_t *counts, int64_t hypothesis_capacity) {
    if (!ctx || !info || !usable || !samples || !models || !counts) return SRL_ERR_BAD_ARG;
    SrlConsensus *c = ctx->consensus;
    if (!c || c->last_model < 0) return SRL_ERR_NO_MAP;
    if (point_capacity < (int64_t)c->last_n || hypothesis_capacity < (int64_t)c->last_H) return SRL_ERR_BAD_ARG;
    const int slots = c->last_model == CONS_F ? ConsTraits<CONS_F>::SLOTS : ConsTraits<CONS_P>::SLOTS;
    const size_t M = (size_t)c->last_H * slots;
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    int nusable = 0;
    HIPCHK(ctx, hipMemcpy(&nusable, c->d_nusable, sizeof(int), hipMemcpyDeviceToHost));
    if (nusable < 0 || nusable > c->last_n) { ctx->err = "consensus: the device holds a usable count outside 0 ... n"; return SRL_ERR_HIP; }
    std::memset(info, 0, sizeof *info);
    info->model = c->last_model; info->hypotheses = c->last_H; info->n = c->last_n; info->slots = slots; info->usable = nusable;
    // a PnP call computes no normalisation: its six values read 0, whatever a fundamental call before it left in the workspace
    if (c->last_model == CONS_F) HIPCHK(ctx, hipMemcpy(info->norm, c->d_norm, 6 * sizeof(double), hipMemcpyDeviceToHost));
    if (nusable > 0) HIPCHK(ctx, hipMemcpy(usable, c->d_usable, (size_t)nusable * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(samples, c->d_samples, (size_t)c->last_H * 8 * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(models, c->d_models, M * 12 * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(counts, c->d_flags, M * sizeof(int), hipMemcpyDeviceToHost));
    return SRL_OK;
}

extern "C" void srl_consensus_opts_default(srl_consensus_opts *o, int model) {
    if (!o) return;
    if (model == SRL_CONSENSUS_PNP) { o->threshold = 1.5; o->confidence = 0.99; o->hypotheses = 200; }
    else { o->threshold = 1.0; o->confidence = 0.997; o->hypotheses = 512; }
    o->seed = 0;
}

extern "C" void srl_consensus_release(srl_ctx *ctx) {
    if (!ctx || !ctx->consensus) return;
    if (ctx->consensus->d_block) hipFree(ctx->consensus->d_block);
    if (ctx->consensus->h_block) hipHostFree(ctx->consensus->h_block);
    delete ctx->consensus;
    ctx->consensus = nullptr;
}

extern "C" int srl_consensus_fundamental(srl_ctx *ctx, const float *last_xy, const float *cur_xy, int n, const srl_consensus_opts *opts, uint8_t *status,
                                         srl_consensus_result *result) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx) return SRL_ERR_BAD_ARG;
    srl_consensus_opts o;
    if (opts) o = *opts; else srl_consensus_opts_default(&o, SRL_CONSENSUS_FUNDAMENTAL);
    if (n < 0 || n > SRL_CONSENSUS_MAX_POINTS || (n > 0 && (!last_xy || !cur_xy || !status)) || !cons_opts_ok(&o)) return SRL_ERR_BAD_ARG;
    if (ctx->nranks > 1) { ctx->err = "consensus: one rank only, like the colour map"; return SRL_ERR_UNSUPPORTED; }
    if (n < 8) {                           // below the minimal sample plus one: nothing to agree on
        if (n > 0) std::memset(status, 0, (size_t)n);
        if (result) cons_empty_result(result);
        return SRL_OK;
    }
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    { const int rc = cons_workspace(ctx); if (rc) return rc; }
    SrlConsensus *c = ctx->consensus;
    for (int i = 0; i < n; i++) {
        c->h_pts[4 * i] = last_xy[2 * i]; c->h_pts[4 * i + 1] = last_xy[2 * i + 1];
        c->h_pts[4 * i + 2] = cur_xy[2 * i]; c->h_pts[4 * i + 3] = cur_xy[2 * i + 1];
    }
    { const int rc = cons_run<CONS_F>(ctx, n, &o, nullptr); if (rc) return rc; }
    std::memcpy(status, c->h_mask, (size_t)n);
    if (result) *result = *c->h_res;
    return SRL_OK;
}

extern "C" int srl_consensus_pnp(srl_ctx *ctx, const float *xyz, const float *uv, int n, const double *fx_fy_cx_cy, const srl_consensus_opts *opts,
                                 int32_t *inliers, int *n_inliers, srl_consensus_result *result) {
    if (result) std::memset(result, 0, sizeof *result);
    if (!ctx) return SRL_ERR_BAD_ARG;
    srl_consensus_opts o;
    if (opts) o = *opts; else srl_consensus_opts_default(&o, SRL_CONSENSUS_PNP);
    if (n < 0 || n > SRL_CONSENSUS_MAX_POINTS || !n_inliers || !fx_fy_cx_cy || (n > 0 && (!xyz || !uv || !inliers)) || !cons_opts_ok(&o)) return SRL_ERR_BAD_ARG;
    for (int k = 0; k < 4; k++) if (!std::isfinite(fx_fy_cx_cy[k])) return SRL_ERR_BAD_ARG;
    if (fx_fy_cx_cy[0] == 0.0 || fx_fy_cx_cy[1] == 0.0) return SRL_ERR_BAD_ARG;
    if (ctx->nranks > 1) { ctx->err = "consensus: one rank only, like the colour map"; return SRL_ERR_UNSUPPORTED; }
    if (n < 4) {
        *n_inliers = 0;
        if (result) cons_empty_result(result);
        return SRL_OK;
    }
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    { const int rc = cons_workspace(ctx); if (rc) return rc; }
    SrlConsensus *c = ctx->consensus;
    for (int i = 0; i < n; i++) {
        c->h_pts[5 * i] = xyz[3 * i]; c->h_pts[5 * i + 1] = xyz[3 * i + 1]; c->h_pts[5 * i + 2] = xyz[3 * i + 2];
        c->h_pts[5 * i + 3] = uv[2 * i]; c->h_pts[5 * i + 4] = uv[2 * i + 1];
    }
    { const int rc = cons_run<CONS_P>(ctx, n, &o, fx_fy_cx_cy); if (rc) return rc; }
    const int cnt = c->h_res->inliers;
    if (cnt < 0 || cnt > n) { ctx->err = "consensus: the device returned an inlier count outside 0 ... n"; return SRL_ERR_HIP; }
    std::memcpy(inliers, c->h_list, (size_t)cnt * sizeof(int));
    *n_inliers = cnt;
    if (result) *result = *c->h_res;
    return SRL_OK;
}

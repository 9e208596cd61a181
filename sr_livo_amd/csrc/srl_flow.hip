// srl_flow.hip -- the optical-flow step of the camera stage on the device for gfx950: LKOpticalFlowKernel::trackImage (src/lkpyramid.cpp:755-795)
// with opencvBuildOpticalFlowPyramid (:510-625), calcSharrDeriv (:57-154) and calculateLKOpticalFlow (:174-496) for one channel and
// err = nullptr.  The pyramid and the derivative are integer arithmetic; every float statement of the track is evaluated as written
// (-ffp-contract=off; `/` and sqrtf are correctly rounded, FP32 denormals are kept) and every float accumulation runs in the order of
// the reference's SSE loops, so the tracked positions are held to the bar of the rest of this tree: bitwise.  The contract is written out
// in include/srlivo_hip.h.
//
//   k_flow_level0  one thread per PADDED pixel of level 0: the padded coordinate is reflected (BORDER_REFLECT_101) into the image and copied.
//   k_flow_down    one thread per PADDED pixel of level k: reflected into the level's interior, where cv::pyrDown's value is evaluated from
//                  level k - 1 (separable [1 4 6 4 1] = a 5 x 5 integer sum, (s + 128) >> 8, taps reflected).  No thread depends on another.
//   k_flow_scharr  one thread per padded pixel: (Ix, Iy) inside, (0, 0) in the border (BORDER_CONSTANT).  The reflected neighbours beyond
//                  the edge (:86-88, :117-125) ARE the padded image's border, so the nine bytes are read without a test.  Ranges: the
//                  smoothing row (s0 + s2) 3 + s1 10 is at most 16 x 255 = 4080, the difference row at most 255 in magnitude, so
//                  |Ix|, |Iy| <= 4080 and no int16 intermediate wraps: the reference's SIMD and scalar paths agree, and so does this int arithmetic.
//   k_flow_track   one wave per point, all levels L ... 0 in one launch.  The 441-entry windows of I (int16, scaled by 32) and of (Ix, Iy) and
//                  the 441 differences It of an iteration live in LDS (3.5 KB).  All 64 lanes do the integer bilinear interpolation; the
//                  float sums are strictly sequential chains, one per lane: 15 lanes for the A-matrix (three sums x (four SSE lanes + the
//                  scalar tail)), 10 lanes for the b-vector (two SSE registers x four lanes + two tails).  Every lane carries the scalar
//                  state (the same IEEE operations on the same values), so control flow is uniform.  No floating-point atomics.
//
// Bounds of the window reads (I, dI and J alike): the admission tests allow -21 <= ix < cols and -21 <= iy < rows; the window reads
// columns ix ... ix + 21 and rows iy ... iy + 21 of the level, i.e. padded columns ix + 21 ... ix + 42 in [0, cols + 41] and padded rows in
// [0, rows + 41]: exactly the first and last column and row of the (rows + 42) x (cols + 42) buffers.  A corner that is not an int32 is
// treated as outside (the reference's cvFloor yields INT_MIN there, which its tests reject too).
//
// Two entries, one body (flow_track): srl_flow_track_image uploads the caller's gray image, srl_flow_track_prepared takes the equalised
// gray image srl_image_prepare left on the device (srl_image_prep.hip); level 0 is copied from either and nothing after that differs.
#include "srl_ctx.h"
#include "srl_image_prep.h"
#include "../../include/srlivo_hip_debug.h"

#include <cmath>
#include <cstring>

#define FLOW_WIN 21
#define FLOW_AREA 441
#define FLOW_MAX_LEVELS 4

struct SrlFlowLevel { int rows, cols; size_t img_at, der_at; };        // offsets into a set: bytes of the images, int16 PAIRS of the derivatives

struct SrlFlow {
    srl_flow_opts opts;
    int max_level = 0;                 // as reduced by the size rule at the first image; persists (trackImage assigns it back)
    int rows = 0, cols = 0;            // of the tracker's first image (0: none yet)
    bool have_prev = false;
    int nlev = 0;
    SrlFlowLevel lev[FLOW_MAX_LEVELS];
    size_t img_bytes = 0, der_pairs = 0;
    struct Mem {                       // what the tracker's storage owns: freed by flow_free, and a fresh one ({}) is a tracker without storage
        char *d_sets = nullptr;                            // one block, laid out by flow_layout_sets
        unsigned char *d_img[2] = {nullptr, nullptr};      // [prev], [cur]: swapped by pointer
        short *d_der[2] = {nullptr, nullptr};
        SrlImagePair gray;                                 // the upload of srl_flow_track_image: comes with the first uploaded image
        char *d_pts = nullptr;                             // one growable block, laid out by flow_layout_pts
        float *d_prev = nullptr, *d_next = nullptr;
        unsigned char *d_status = nullptr;
        int pts_cap = 0;
    } mem;
};

namespace {

// cv::borderInterpolate(p, n, BORDER_REFLECT_101); |p| exceeds n by at most 21 + 2, so the loop ends after a few turns
__device__ __forceinline__ int flow_reflect(int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

__global__ void __launch_bounds__(256) k_flow_level0(const unsigned char *gray, unsigned char *out, int rows, int cols) {
    const int pc = cols + 2 * FLOW_WIN, pr = rows + 2 * FLOW_WIN;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)pc * pr) return;
    const int py = (int)(i / pc), px = (int)(i - (long long)py * pc);
    out[i] = gray[(size_t)flow_reflect(py - FLOW_WIN, rows) * cols + flow_reflect(px - FLOW_WIN, cols)];
}

// src: padded level k - 1 (srows x scols inside); out: padded level k (rows x cols inside)
__global__ void __launch_bounds__(256) k_flow_down(const unsigned char *src, int srows, int scols, unsigned char *out, int rows, int cols) {
    const int pc = cols + 2 * FLOW_WIN, pr = rows + 2 * FLOW_WIN, spc = scols + 2 * FLOW_WIN;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)pc * pr) return;
    const int py = (int)(i / pc), px = (int)(i - (long long)py * pc);
    const int y = flow_reflect(py - FLOW_WIN, rows), x = flow_reflect(px - FLOW_WIN, cols);
    int cx[5];
#pragma unroll
    for (int k = 0; k < 5; k++) cx[k] = flow_reflect(2 * x + k - 2, scols) + FLOW_WIN;
    const int K[5] = {1, 4, 6, 4, 1};
    int s = 0;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const unsigned char *r = src + (size_t)(flow_reflect(2 * y + k - 2, srows) + FLOW_WIN) * spc;
        s += K[k] * ((int)r[cx[0]] + 4 * (int)r[cx[1]] + 6 * (int)r[cx[2]] + 4 * (int)r[cx[3]] + (int)r[cx[4]]);
    }
    out[i] = (unsigned char)((s + 128) >> 8);
}

__global__ void __launch_bounds__(256) k_flow_scharr(const unsigned char *img, short2 *der, int rows, int cols) {
    const int pc = cols + 2 * FLOW_WIN, pr = rows + 2 * FLOW_WIN;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)pc * pr) return;
    const int py = (int)(i / pc), px = (int)(i - (long long)py * pc);
    short2 v = make_short2(0, 0);
    if (py >= FLOW_WIN && py < FLOW_WIN + rows && px >= FLOW_WIN && px < FLOW_WIN + cols) {
        const unsigned char *r0 = img + (size_t)(py - 1) * pc + px, *r1 = r0 + pc, *r2 = r1 + pc;      // the border is 21 wide: px - 1 >= 20
        int t0[3], t1[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int a = r0[k - 1], b = r1[k - 1], c = r2[k - 1];
            t0[k] = (a + c) * 3 + b * 10;
            t1[k] = c - a;
        }
        v.x = (short)(t0[2] - t0[0]);
        v.y = (short)((t1[2] + t1[0]) * 3 + t1[1] * 10);
    }
    der[i] = v;
}

struct FlowLevelArgs { const unsigned char *I; const short *dI; const unsigned char *J; int rows, cols; };
struct FlowTrackArgs {
    FlowLevelArgs lv[FLOW_MAX_LEVELS];
    int L, n, max_count;
    double epsilon;
    float min_eig;
};

// cvFloor; false where the value is no int32 (NaN, infinities, beyond +-2^31)
__device__ __forceinline__ bool flow_floor(float v, int *out) {
    const float f = floorf(v);
    if (!(f >= -2147483648.f && f < 2147483648.f)) return false;
    *out = (int)f;
    return true;
}

struct FlowWeights { int w00, w01, w10, w11; };
// cvRound of the three products (round to nearest even), the fourth weight by difference (:234-237)
__device__ __forceinline__ FlowWeights flow_weights(float a, float b) {
    FlowWeights w;
    w.w00 = __float2int_rn((1.f - a) * (1.f - b) * (float)(1 << 14));
    w.w01 = __float2int_rn(a * (1.f - b) * (float)(1 << 14));
    w.w10 = __float2int_rn((1.f - a) * b * (float)(1 << 14));
    w.w11 = (1 << 14) - w.w00 - w.w01 - w.w10;
    return w;
}
#define FLOW_DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))

__global__ void __launch_bounds__(64) k_flow_track(const float2 *prev, float2 *next, unsigned char *status, FlowTrackArgs A) {
    __shared__ short s_I[FLOW_AREA], s_dx[FLOW_AREA], s_dy[FLOW_AREA], s_It[FLOW_AREA];
    __shared__ float s_sum[16];
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= A.n) return;
    const float2 pt = prev[p];
    {   // contract departure: a coordinate that is not finite, or whose window corner at level 0 is no int32
        int t;
        if (!(isfinite(pt.x) && isfinite(pt.y)) || !flow_floor(pt.x - 10.f, &t) || !flow_floor(pt.y - 10.f, &t)) {
            if (lane == 0) { next[p] = pt; status[p] = 0; }
            return;
        }
    }
    float nx = 0.f, ny = 0.f;              // nextPts[ptidx]
    unsigned char st = 1;
    const float FLT_SCALE = 1.f / (1 << 20);
    for (int level = A.L; level >= 0; level--) {
        const FlowLevelArgs &V = A.lv[level];
        const int stride = V.cols + 2 * FLOW_WIN;
        const float sc = (float)(1. / (1 << level));
        float ppx = pt.x * sc, ppy = pt.y * sc;
        if (level == A.L) { nx = ppx; ny = ppy; }
        else { nx = nx * 2.f; ny = ny * 2.f; }
        ppx -= 10.f; ppy -= 10.f;
        int ix = 0, iy = 0;
        if (!flow_floor(ppx, &ix) || !flow_floor(ppy, &iy) || ix < -FLOW_WIN || ix >= V.cols || iy < -FLOW_WIN || iy >= V.rows) {
            if (level == 0) st = 0;
            continue;
        }
        {
            const FlowWeights w = flow_weights(ppx - (float)ix, ppy - (float)iy);
            for (int e = lane; e < FLOW_AREA; e += 64) {
                const int y = e / FLOW_WIN, x = e - y * FLOW_WIN;
                const size_t at = (size_t)(iy + FLOW_WIN + y) * stride + (size_t)(ix + FLOW_WIN + x);
                const unsigned char *s = V.I + at;
                const short *d = V.dI + at * 2;
                s_I[e] = (short)FLOW_DESCALE((int)s[0] * w.w00 + (int)s[1] * w.w01 + (int)s[stride] * w.w10 + (int)s[stride + 1] * w.w11, 9);
                s_dx[e] = (short)FLOW_DESCALE((int)d[0] * w.w00 + (int)d[2] * w.w01 + (int)d[2 * stride] * w.w10 + (int)d[2 * stride + 2] * w.w11, 14);
                s_dy[e] = (short)FLOW_DESCALE((int)d[1] * w.w00 + (int)d[3] * w.w01 + (int)d[2 * stride + 1] * w.w10 + (int)d[2 * stride + 3] * w.w11, 14);
            }
        }
        __syncthreads();
        // A-matrix (:265-330): lane = 5 m + c; m = A11, A12, A22; c < 4: SSE lane c over x = 4 g + c, y ascending then g; c = 4: x = 20
        if (lane < 15) {
            const int m = lane / 5, c = lane - m * 5;
            const short *pa = m == 2 ? s_dy : s_dx, *pb = m == 0 ? s_dx : s_dy;
            float acc = 0.f;
            if (c < 4) {
                for (int y = 0; y < FLOW_WIN; y++)
                    for (int g = 0; g < 5; g++) { const int e = y * FLOW_WIN + 4 * g + c; acc += (float)((int)pa[e] * (int)pb[e]); }
            } else {
                for (int y = 0; y < FLOW_WIN; y++) { const int e = y * FLOW_WIN + 20; acc += (float)((int)pa[e] * (int)pb[e]); }
            }
            s_sum[lane] = acc;
        }
        __syncthreads();
        const float A11 = (s_sum[4] + (((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3])) * FLT_SCALE;
        const float A12 = (s_sum[9] + (((s_sum[5] + s_sum[6]) + s_sum[7]) + s_sum[8])) * FLT_SCALE;
        const float A22 = (s_sum[14] + (((s_sum[10] + s_sum[11]) + s_sum[12]) + s_sum[13])) * FLT_SCALE;
        __syncthreads();                   // s_sum is written again below
        float D = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * FLOW_WIN * FLOW_WIN);
        if (minEig < A.min_eig || D < 1.1920929e-07f) {
            if (level == 0) st = 0;
            continue;
        }
        D = 1.f / D;
        float tx = nx - 10.f, ty = ny - 10.f;      // nextPt -= halfWin
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < A.max_count; j++) {
            int jx = 0, jy = 0;
            if (!flow_floor(tx, &jx) || !flow_floor(ty, &jy) || jx < -FLOW_WIN || jx >= V.cols || jy < -FLOW_WIN || jy >= V.rows) {
                if (level == 0) st = 0;
                break;
            }
            const FlowWeights w = flow_weights(tx - (float)jx, ty - (float)jy);
            for (int e = lane; e < FLOW_AREA; e += 64) {
                const int y = e / FLOW_WIN, x = e - y * FLOW_WIN;
                const unsigned char *s = V.J + (size_t)(jy + FLOW_WIN + y) * stride + (size_t)(jx + FLOW_WIN + x);
                s_It[e] = (short)(FLOW_DESCALE((int)s[0] * w.w00 + (int)s[1] * w.w01 + (int)s[stride] * w.w10 + (int)s[stride + 1] * w.w11, 9) - (int)s_I[e]);
            }
            __syncthreads();
            // b-vector (:382-432): lanes 0..7 = SSE lanes of qb0 (i = 0, 1) and qb1 (i = 2, 3), component lane & 1; lanes 8, 9 = the scalar tails
            if (lane < 10) {
                const short *pd = (lane & 1) ? s_dy : s_dx;
                float acc = 0.f;
                if (lane < 8) {
                    const int i = lane >> 1;
                    for (int y = 0; y < FLOW_WIN; y++)
                        for (int g = 0; g < 2; g++) {
                            const int e = y * FLOW_WIN + 8 * g + i;
                            acc += (float)((int)s_It[e] * (int)pd[e] + (int)s_It[e + 4] * (int)pd[e + 4]);
                        }
                } else {
                    for (int y = 0; y < FLOW_WIN; y++)
                        for (int x = 16; x < FLOW_WIN; x++) { const int e = y * FLOW_WIN + x; acc += (float)((int)s_It[e] * (int)pd[e]); }
                }
                s_sum[lane] = acc;
            }
            __syncthreads();
            const float b1 = (s_sum[8] + ((s_sum[0] + s_sum[4]) + (s_sum[2] + s_sum[6]))) * FLT_SCALE;
            const float b2 = (s_sum[9] + ((s_sum[1] + s_sum[5]) + (s_sum[3] + s_sum[7]))) * FLT_SCALE;
            __syncthreads();
            const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
            tx += dx; ty += dy;
            nx = tx + 10.f; ny = ty + 10.f;
            if ((double)dx * (double)dx + (double)dy * (double)dy <= A.epsilon) break;
            if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {
                nx -= dx * 0.5f; ny -= dy * 0.5f;
                break;
            }
            pdx = dx; pdy = dy;
        }
    }
    if (lane == 0) { next[p] = make_float2(nx, ny); status[p] = st; }
}

// the two image sets and the two derivative sets of a plan out of d_sets (null: only measured); returns the block's size
size_t flow_layout_sets(SrlFlow *f) {
    SrlCarve c{f->mem.d_sets};
    for (int k = 0; k < 2; k++) { f->mem.d_img[k] = c.take<unsigned char>(f->img_bytes); f->mem.d_der[k] = c.take<short>(f->der_pairs * 2); }
    return c.at;
}
// ... and cap points out of d_pts
size_t flow_layout_pts(SrlFlow::Mem *m, size_t cap) {
    SrlCarve c{m->d_pts};
    m->d_prev = c.take<float>(cap * 2); m->d_next = c.take<float>(cap * 2); m->d_status = c.take<unsigned char>(cap);
    return c.at;
}

void flow_free(SrlFlow *f) {
    if (f->mem.d_sets) hipFree(f->mem.d_sets);
    if (f->mem.d_pts) hipFree(f->mem.d_pts);
    f->mem.gray.release();
    f->mem = {};
}

// opencvBuildOpticalFlowPyramid's level rule (:609-619): building stops after the level whose successor would be no larger than the window
int flow_plan(SrlFlow *f, int rows, int cols) {
    int r = rows, c = cols, L = f->max_level;
    size_t img = 0, der = 0;
    f->nlev = 0;
    for (int level = 0; level <= f->max_level; level++) {
        const size_t padded = (size_t)(r + 2 * FLOW_WIN) * (size_t)(c + 2 * FLOW_WIN);
        f->lev[level] = {r, c, img, der};
        img += (padded + 255) / 256 * 256;
        der += (padded + 255) / 256 * 256;
        f->nlev = level + 1;
        r = (r + 1) / 2; c = (c + 1) / 2;
        if (c <= FLOW_WIN || r <= FLOW_WIN) { L = level; break; }
    }
    f->img_bytes = img; f->der_pairs = der;
    return L;
}

// the refusal every entry point behind srl_flow_create makes
int srl_flow_need(srl_ctx *ctx) {
    if (!ctx->flow) { ctx->err = "no flow tracker (srl_flow_create)"; return SRL_ERR_NO_MAP; }
    return SRL_OK;
}

}  // namespace

extern "C" void srl_flow_opts_default(srl_flow_opts *o) {
    if (!o) return;
    o->win = 21; o->max_level = 3; o->max_count = 10; o->epsilon = 0.05; o->min_eig_threshold = 1e-4;
}

extern "C" int srl_flow_create(srl_ctx *ctx, const srl_flow_opts *opts) {
    if (!ctx || !opts) return SRL_ERR_BAD_ARG;
    if (opts->win != FLOW_WIN) { ctx->err = "flow: the window is 21 x 21 (the order of the float sums is that of a 21-wide row)"; return SRL_ERR_UNSUPPORTED; }
    if (opts->max_level < 0 || opts->max_level >= FLOW_MAX_LEVELS || opts->max_count < 0 || opts->max_count > 100 || !(opts->epsilon >= 0.0) ||
        !(opts->epsilon <= 10.0) || !std::isfinite(opts->min_eig_threshold)) {
        ctx->err = "flow options: max_level 0 ... 3, max_count 0 ... 100, epsilon 0 ... 10, a finite min_eig_threshold";
        return SRL_ERR_BAD_ARG;
    }
    if (ctx->flow) { ctx->err = "a flow tracker exists: its options hold for its life (srl_flow_destroy first)"; return SRL_ERR_BAD_ARG; }
    SrlFlow *f = new SrlFlow();
    f->opts = *opts;
    f->max_level = opts->max_level;
    ctx->flow = f;                        // storage comes with the first image
    return SRL_OK;
}

extern "C" int srl_flow_destroy(srl_ctx *ctx) {
    if (!ctx) return SRL_ERR_BAD_ARG;
    SrlFlow *f = ctx->flow;
    if (!f) return SRL_OK;
    SRL_DISARM(ctx);
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    flow_free(f);
    delete f;
    ctx->flow = nullptr;
    return SRL_OK;
}

// Everything of a track call behind its refusals.  The image is either the caller's (gray: staged and uploaded) or one a kernel of this
// context's stream has left on the device (d_prepared: rows x cols bytes, packed) -- from there on the two entries are one.
static int flow_track(srl_ctx *ctx, SrlFlow *f, const uint8_t *gray, const unsigned char *d_prepared, int rows, int cols, int64_t row_stride_bytes,
                      const float *prev_xy, int n, float *next_xy, uint8_t *status, int *n_tracked) {
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SrlFlow::Mem &m = f->mem;
    // the upload's blocks come with the first uploaded image, which need not be the tracker's first; a failure leaves the tracker as it was
    if (gray) { const int rc = m.gray.reserve(ctx, (size_t)rows * (size_t)cols, (size_t)rows * (size_t)cols); if (rc) return rc; }
    if (!f->rows) {
        const int L = flow_plan(f, rows, cols);
        const size_t bytes = flow_layout_sets(f);
        hipError_t e = hipMalloc((void **)&m.d_sets, bytes);
        // a set that has not seen an image reads as zeros (srl_flow_download_level)
        if (e == hipSuccess) e = hipMemsetAsync(m.d_sets, 0, bytes, st);
        if (e != hipSuccess) { flow_free(f); f->max_level = f->opts.max_level; HIPCHK(ctx, e); }
        flow_layout_sets(f);
        f->max_level = L; f->rows = rows; f->cols = cols;
    }
    if (n > m.pts_cap) {
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (m.d_pts) { hipFree(m.d_pts); m.d_pts = nullptr; m.pts_cap = 0; }
        const int cap = n < 512 ? 512 : n + n / 2;
        HIPCHK(ctx, hipMalloc((void **)&m.d_pts, flow_layout_pts(&m, (size_t)cap)));
        flow_layout_pts(&m, (size_t)cap);
        m.pts_cap = cap;
    }
    // the current image's pyramid and derivatives into set 1 (every call ends synchronised, so the staging block is free)
    const unsigned char *d_level0 = d_prepared;
    if (gray) {
        { const int rc = m.gray.upload(ctx, gray, rows, (size_t)cols, row_stride_bytes); if (rc) return rc; }
        d_level0 = m.gray.d;
    }
    for (int level = 0; level <= f->max_level; level++) {
        const SrlFlowLevel &V = f->lev[level];
        const size_t padded = (size_t)(V.rows + 2 * FLOW_WIN) * (size_t)(V.cols + 2 * FLOW_WIN);
        const unsigned nb = (unsigned)((padded + 255) / 256);
        if (level == 0) hipLaunchKernelGGL(k_flow_level0, dim3(nb), dim3(256), 0, st, d_level0, m.d_img[1] + V.img_at, V.rows, V.cols);
        else hipLaunchKernelGGL(k_flow_down, dim3(nb), dim3(256), 0, st, m.d_img[1] + f->lev[level - 1].img_at, f->lev[level - 1].rows, f->lev[level - 1].cols,
                                m.d_img[1] + V.img_at, V.rows, V.cols);
        hipLaunchKernelGGL(k_flow_scharr, dim3(nb), dim3(256), 0, st, m.d_img[1] + V.img_at, reinterpret_cast<short2 *>(m.d_der[1] + V.der_at * 2), V.rows, V.cols);
    }
    HIPCHK(ctx, hipGetLastError());
    const bool first = !f->have_prev;
    const size_t at_next = 0, at_status = (size_t)n * 2 * sizeof(float), at_prev = (at_status + (size_t)n + 63) / 64 * 64;
    if (!first && n > 0) {
        { const int rc = ensure_host_scratch(ctx, at_prev + (size_t)n * 2 * sizeof(float)); if (rc) return rc; }
        std::memcpy(ctx->h_scratch + at_prev, prev_xy, (size_t)n * 2 * sizeof(float));
        HIPCHK(ctx, hipMemcpyAsync(m.d_prev, ctx->h_scratch + at_prev, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice, st));
        FlowTrackArgs A;
        for (int level = 0; level < FLOW_MAX_LEVELS; level++) {
            const SrlFlowLevel &V = f->lev[level <= f->max_level ? level : 0];
            A.lv[level] = {m.d_img[0] + V.img_at, m.d_der[0] + V.der_at * 2, m.d_img[1] + V.img_at, V.rows, V.cols};
        }
        A.L = f->max_level; A.n = n; A.max_count = f->opts.max_count; A.epsilon = f->opts.epsilon; A.min_eig = (float)f->opts.min_eig_threshold;
        hipLaunchKernelGGL(k_flow_track, dim3((unsigned)n), dim3(64), 0, st, reinterpret_cast<const float2 *>(m.d_prev), reinterpret_cast<float2 *>(m.d_next),
                           m.d_status, A);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch + at_next, m.d_next, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch + at_status, m.d_status, (size_t)n, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    // swapImageBuffer (:744-753): the image just given is the previous one of the next call
    std::swap(m.d_img[0], m.d_img[1]);
    std::swap(m.d_der[0], m.d_der[1]);
    f->have_prev = true;
    if (first) {                          // :762-773: curr_tracked_pts = last_tracked_pts, status untouched, 0 returned
        if (n > 0) std::memcpy(next_xy, prev_xy, (size_t)n * 2 * sizeof(float));
        return SRL_OK;
    }
    if (n > 0) {
        std::memcpy(next_xy, ctx->h_scratch + at_next, (size_t)n * 2 * sizeof(float));
        std::memcpy(status, ctx->h_scratch + at_status, (size_t)n);
        int cnt = 0;
        for (int i = 0; i < n; i++) cnt += status[i];
        if (n_tracked) *n_tracked = cnt;
    }
    return SRL_OK;
}

extern "C" int srl_flow_track_image(srl_ctx *ctx, const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, const float *prev_xy, int n,
                                    float *next_xy, uint8_t *status, int *n_tracked) {
    if (n_tracked) *n_tracked = 0;
    if (!ctx || !gray || rows < 2 || cols < 2 || rows > SRL_FLOW_MAX_EXTENT || cols > SRL_FLOW_MAX_EXTENT || row_stride_bytes < (int64_t)cols || n < 0 ||
        n > SRL_FLOW_MAX_POINTS || (n > 0 && (!prev_xy || !next_xy || !status)))
        return SRL_ERR_BAD_ARG;
    { const int rc = srl_flow_need(ctx); if (rc) return rc; }
    SrlFlow *f = ctx->flow;
    if (f->rows && (rows != f->rows || cols != f->cols)) { ctx->err = "flow: the image size differs from the tracker's first image"; return SRL_ERR_BAD_ARG; }
    return flow_track(ctx, f, gray, nullptr, rows, cols, row_stride_bytes, prev_xy, n, next_xy, status, n_tracked);
}

extern "C" int srl_flow_track_prepared(srl_ctx *ctx, const float *prev_xy, int n, float *next_xy, uint8_t *status, int *n_tracked) {
    if (n_tracked) *n_tracked = 0;
    if (!ctx || n < 0 || n > SRL_FLOW_MAX_POINTS || (n > 0 && (!prev_xy || !next_xy || !status))) return SRL_ERR_BAD_ARG;
    { const int rc = srl_flow_need(ctx); if (rc) return rc; }
    SrlFlow *f = ctx->flow;
    { const int rc = srl_prep_need(ctx, true); if (rc) return rc; }
    const SrlImagePrep *p = ctx->prep;
    if (f->rows && (p->rows != f->rows || p->cols != f->cols)) { ctx->err = "flow: the image size differs from the tracker's first image"; return SRL_ERR_BAD_ARG; }
    return flow_track(ctx, f, nullptr, p->d_gray_eq, p->rows, p->cols, p->cols, prev_xy, n, next_xy, status, n_tracked);
}

extern "C" int srl_flow_levels(srl_ctx *ctx, int *L) {
    if (L) *L = 0;
    if (!ctx || !L) return SRL_ERR_BAD_ARG;
    { const int rc = srl_flow_need(ctx); if (rc) return rc; }
    *L = ctx->flow->max_level;
    return SRL_OK;
}

extern "C" int srl_flow_download_level(srl_ctx *ctx, int which, int level, uint8_t *image_padded, int16_t *deriv_padded, int *rows, int *cols) {
    if (rows) *rows = 0;
    if (cols) *cols = 0;
    if (!ctx || (which != SRL_FLOW_PREV && which != SRL_FLOW_CUR) || level < 0) return SRL_ERR_BAD_ARG;
    { const int rc = srl_flow_need(ctx); if (rc) return rc; }
    SrlFlow *f = ctx->flow;
    if (!f->rows) { ctx->err = "flow: no image yet"; return SRL_ERR_NO_SWEEP; }
    if (level > f->max_level) return SRL_ERR_BAD_ARG;
    const SrlFlowLevel &V = f->lev[level];
    if (rows) *rows = V.rows;
    if (cols) *cols = V.cols;
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t padded = (size_t)(V.rows + 2 * FLOW_WIN) * (size_t)(V.cols + 2 * FLOW_WIN);
    if (image_padded) HIPCHK(ctx, hipMemcpy(image_padded, f->mem.d_img[which] + V.img_at, padded, hipMemcpyDeviceToHost));
    if (deriv_padded) HIPCHK(ctx, hipMemcpy(deriv_padded, f->mem.d_der[which] + V.der_at * 2, padded * 2 * sizeof(short), hipMemcpyDeviceToHost));
    return SRL_OK;
}

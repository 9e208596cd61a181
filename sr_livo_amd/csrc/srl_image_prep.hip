// srl_image_prep.hip -- the top of imageProcessing::process (src/imageProcessing.cpp:113-125, :166-200) on the device for gfx950: one raw
// BGR frame in, the equalised gray image (the optical flow's) and the equalised BGR image (the colour map's) out, with no stage on the
// host.  The operations are THIS library's, specified in include/srlivo_hip.h; they follow OpenCV's fixed-point conventions but claim no
// equality with its bytes.  All arithmetic is integer except CLAHE's look-up scale and its bilinear blend, which are plain IEEE FP32
// (-ffp-contract=off, no atomics on floats): the same input gives the same bytes, and they equal a NumPy restatement bitwise.
//
//   k_resize_bgr  only behind srl_image_prepare_resized, and only for a frame of another size than the preparer's: four destination
//                 pixels per lane as below, each from its two source columns and two source rows through the tables of
//                 srl_image_resize_build_tables (device memory, rebuilt when the source size changes) -- or, at exactly half the size,
//                 the 2 x 2 box mean.  Integer only.  It writes where an upload of the preparer's size lands, so the three kernels below
//                 read the resized frame where they read the uploaded one.
//   k_prep_pixel  four consecutive pixels (of the image taken as one flat array) per lane, so that every store is an aligned dword
//                 whatever the width: reads map1 / map2 (16 + 8 bytes per lane) and up to four BGR neighbours per pixel, writes undist
//                 (12 bytes), gray, Y (4 each) and CrCb (8).  The planes are allocated for a multiple of four pixels: the last lane's
//                 surplus pixels repeat the last pixel's coordinates and land in that slack.
//   k_prep_tiles  one wave per (plane, tile), four per workgroup: a 256-bin histogram in LDS (integer atomics; the extension is read by
//                 reflect-101), then lane l holds bins 4 l ... 4 l + 3 in registers: clip, closed-form redistribution, wave scan, and
//                 the 256-byte look-up table as one dword per lane.  No per-lane array is indexed at run time; LDS = the four histograms.
//                 (Sized for the reference's rule, T = cols / 20: thousands of small tiles.  A small explicit T on a large image leaves
//                 few waves with long loops -- correct, not fast.)
//   k_prep_apply  four pixels per lane again: four LUT bytes per pixel and plane (the tables stay in L2), the FP32 blend, YCrCb -> BGR,
//                 writes gray_eq (4 bytes) and bgr_eq (12).
//
// Bounds: a source neighbour is read only inside 0 <= y < rows, 0 <= x < cols (anything else contributes 0).  A tile reads extended
// coordinates below cols + T and rows + T, reflected to >= cols - 1 - T and rows - 1 - T: create refuses rows <= T and cols <= T.  LUT
// indices are clamped to 0 ... T - 1 by the specification itself.  The resize reads source columns ofs and min(ofs + 1, src_cols - 1) with
// ofs clamped to 0 ... src_cols - 1 (the builder's own range), rows alike; at half the size columns 2 x, 2 x + 1 <= 2 cols - 1.
#include "srl_image_prep.h"
#include "srl_color_map.h"
#include "../../include/srlivo_hip_debug.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

struct PrepPlan { int T, tw, th, ext_rows, ext_cols, limit[2]; };

// every rule on the options (srl_image_prep_build_map and srl_image_prep_create share it)
bool prep_plan(const srl_image_prep_opts *o, PrepPlan *p) {
    if (o->rows < 16 || o->cols < 16 || o->rows > SRL_FLOW_MAX_EXTENT || o->cols > SRL_FLOW_MAX_EXTENT) return false;
    if ((int64_t)o->rows * o->cols > SRL_COLOR_IMAGE_MAX_PIXELS) return false;
    bool finite = std::isfinite(o->fx) && std::isfinite(o->fy) && std::isfinite(o->cx) && std::isfinite(o->cy);
    for (int k = 0; k < 5; k++) finite = finite && std::isfinite(o->dist[k]);
    if (!finite || o->fx == 0.0 || o->fy == 0.0) return false;
    if (!(std::isfinite(o->clip_gray) && o->clip_gray > 0.0 && std::isfinite(o->clip_color) && o->clip_color > 0.0)) return false;
    const int lesser = o->rows < o->cols ? o->rows : o->cols;
    if (o->tiles != 0 && (o->tiles < 2 || o->tiles > lesser / 2)) return false;
    int T = o->tiles;
    if (T == 0) { T = (int)(o->cols * 32.0 / 640); if (T < 4) T = 4; }      // :169
    if (o->rows <= T || o->cols <= T) return false;                          // the reflection would leave the image
    p->T = T;
    p->ext_rows = o->rows; p->ext_cols = o->cols;
    if (o->cols % T != 0 || o->rows % T != 0) { p->ext_cols += T - o->cols % T; p->ext_rows += T - o->rows % T; }
    p->tw = p->ext_cols / T; p->th = p->ext_rows / T;
    const double area = (double)p->tw * (double)p->th;
    const double clip[2] = {o->clip_gray, o->clip_color};
    for (int k = 0; k < 2; k++) {
        const double l = clip[k] * area / 256;
        p->limit[k] = l >= 2147483647.0 ? 2147483647 : (int)l;
        if (p->limit[k] < 1) p->limit[k] = 1;
    }
    return true;
}

#define PREP_DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))
__device__ __forceinline__ int prep_sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// sat8(DESCALE(x, 14)) with the clamp made BEFORE the shift (the same value: the shift is monotonic).  Written as sat8(x >> 14) twice and
// packed into neighbouring bytes, the pair is selected as gfx950's v_ashr_pk_u8_i32, which writes only the low half of its destination
// while the compiler takes the upper half for zero: the bits left there ended up in the next pixel's bytes.
__device__ __forceinline__ int prep_sat8_descale14(int x) {
    x += 1 << 13;
    x = x < 0 ? 0 : (x > (256 << 14) - 1 ? (256 << 14) - 1 : x);
    return x >> 14;
}

struct PrepResizeArgs { PrepDims D; int src_rows, src_cols; };               // D: the destination, the preparer's size

// HALF: src = 2 x dst in both directions, the 2 x 2 box mean; the tables are not read
template <bool HALF>
__global__ void __launch_bounds__(256) k_resize_bgr(const unsigned char *__restrict__ src, const int *__restrict__ ofs_x, const unsigned *__restrict__ coef_x,
                                                     const int *__restrict__ ofs_y, const unsigned *__restrict__ coef_y, unsigned *__restrict__ dst,
                                                     PrepResizeArgs A, int ngroups) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= ngroups) return;
    int x, y;
    prep_first(A.D, g, &x, &y);
    const size_t down = (size_t)A.src_cols * 3;
    unsigned ub[12];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int x0, x1, y0, y1, a0 = 0, a1 = 0, b0 = 0, b1 = 0;
        if (HALF) {
            x0 = 2 * x; x1 = x0 + 1; y0 = 2 * y; y1 = y0 + 1;
        } else {
            const unsigned cx = coef_x[x], cy = coef_y[y];                      // (coef[2 d], coef[2 d + 1]) as one dword
            a0 = (int)(cx & 0xFFFFu); a1 = (int)(cx >> 16); b0 = (int)(cy & 0xFFFFu); b1 = (int)(cy >> 16);
            x0 = ofs_x[x]; y0 = ofs_y[y];
            x0 = x0 < 0 ? 0 : (x0 > A.src_cols - 1 ? A.src_cols - 1 : x0);      // never taken (the builder's range); keeps the read inside
            y0 = y0 < 0 ? 0 : (y0 > A.src_rows - 1 ? A.src_rows - 1 : y0);
            x1 = x0 + 1 < A.src_cols ? x0 + 1 : A.src_cols - 1;
            y1 = y0 + 1 < A.src_rows ? y0 + 1 : A.src_rows - 1;
        }
        const unsigned char *r0 = src + (size_t)y0 * down, *r1 = src + (size_t)y1 * down;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const int s00 = r0[3 * x0 + ch], s01 = r0[3 * x1 + ch], s10 = r1[3 * x0 + ch], s11 = r1[3 * x1 + ch];
            int v;
            if (HALF) {
                v = (s00 + s01 + s10 + s11 + 2) >> 2;
            } else {
                const int h0 = s00 * a0 + s01 * a1, h1 = s10 * a0 + s11 * a1;
                v = ((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2;
                v = (v > 1023 ? 1023 : v) >> 2;                                 // min(255, v >> 2), the clamp first as in prep_sat8_descale14
            }
            ub[3 * k + ch] = (unsigned)v;
        }
        prep_step(A.D, &x, &y);
    }
    dst[3 * (size_t)g] = ub[0] | ub[1] << 8 | ub[2] << 16 | ub[3] << 24;
    dst[3 * (size_t)g + 1] = ub[4] | ub[5] << 8 | ub[6] << 16 | ub[7] << 24;
    dst[3 * (size_t)g + 2] = ub[8] | ub[9] << 8 | ub[10] << 16 | ub[11] << 24;
}

__global__ void __launch_bounds__(256) k_prep_pixel(const unsigned char *__restrict__ raw, const uint4 *__restrict__ map1, const uint2 *__restrict__ map2,
                                                    unsigned *__restrict__ undist, unsigned *__restrict__ gray, unsigned *__restrict__ yy,
                                                    uint2 *__restrict__ crcb, PrepDims D, int ngroups) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= ngroups) return;
    const uint4 m1v = map1[g];
    const uint2 m2v = map2[g];
    const unsigned m1[4] = {m1v.x, m1v.y, m1v.z, m1v.w};
    const unsigned m2[4] = {m2v.x & 0xFFFFu, m2v.x >> 16, m2v.y & 0xFFFFu, m2v.y >> 16};
    unsigned ub[12], gw = 0, yw = 0, cw[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int sx = (short)(m1[k] & 0xFFFFu), sy = (short)(m1[k] >> 16);
        const int ax = (int)(m2[k] & 31u), ay = (int)(m2[k] >> 5) & 31;
        const int w00 = (32 - ax) * (32 - ay) * 32, w01 = ax * (32 - ay) * 32, w10 = (32 - ax) * ay * 32, w11 = ax * ay * 32;
        const bool x0 = sx >= 0 && sx < D.cols, x1 = sx + 1 >= 0 && sx + 1 < D.cols, y0 = sy >= 0 && sy < D.rows, y1 = sy + 1 >= 0 && sy + 1 < D.rows;
        const unsigned char *p = raw + ((long long)sy * D.cols + sx) * 3;      // dereferenced only where the tests allow
        const long long down = (long long)D.cols * 3;
        int c[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const int p00 = (y0 && x0) ? p[ch] : 0, p01 = (y0 && x1) ? p[3 + ch] : 0, p10 = (y1 && x0) ? p[down + ch] : 0, p11 = (y1 && x1) ? p[down + 3 + ch] : 0;
            c[ch] = (w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 16384) >> 15;
            ub[3 * k + ch] = (unsigned)c[ch];
        }
        const int gv = (9798 * c[0] + 19235 * c[1] + 3735 * c[2] + 16384) >> 15;
        const int Y = PREP_DESCALE(1868 * c[0] + 9617 * c[1] + 4899 * c[2], 14);
        const int Cr = prep_sat8_descale14((c[2] - Y) * 11682 + (128 << 14));
        const int Cb = prep_sat8_descale14((c[0] - Y) * 9241 + (128 << 14));
        gw |= (unsigned)gv << (8 * k);
        yw |= (unsigned)Y << (8 * k);
        cw[k >> 1] |= ((unsigned)Cr | ((unsigned)Cb << 8)) << (16 * (k & 1));
    }
    undist[3 * (size_t)g] = ub[0] | ub[1] << 8 | ub[2] << 16 | ub[3] << 24;
    undist[3 * (size_t)g + 1] = ub[4] | ub[5] << 8 | ub[6] << 16 | ub[7] << 24;
    undist[3 * (size_t)g + 2] = ub[8] | ub[9] << 8 | ub[10] << 16 | ub[11] << 24;
    gray[g] = gw;
    yy[g] = yw;
    crcb[g] = make_uint2(cw[0], cw[1]);
}

struct PrepTileArgs { int rows, cols, T, tw, th, limit[2]; float scale; };      // scale = 255.0f / (float)(tw * th)

__global__ void __launch_bounds__(256) k_prep_tiles(const unsigned char *__restrict__ gray, const unsigned char *__restrict__ yy, unsigned *__restrict__ lut,
                                                    PrepTileArgs A) {
    __shared__ __attribute__((aligned(16))) unsigned s_hist[4][256];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tiles = A.T * A.T, tp = blockIdx.x * 4 + w;
    const bool valid = tp < 2 * tiles;
    const int plane = tp >= tiles ? 1 : 0, tile = tp - plane * tiles;
    const int ty = tile / A.T, tx = tile - ty * A.T;
    unsigned *h = s_hist[w];
    reinterpret_cast<uint4 *>(h)[lane] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    if (valid) {
        const unsigned char *src = plane ? yy : gray;
        const int area = A.tw * A.th;
        for (int e = lane; e < area; e += 64) {
            const int ly = e / A.tw, lx = e - ly * A.tw;
            int X = tx * A.tw + lx, Y = ty * A.th + ly;
            if (X >= A.cols) X = 2 * (A.cols - 1) - X;      // reflect-101 of the extension
            if (Y >= A.rows) Y = 2 * (A.rows - 1) - Y;
            X = X < 0 ? 0 : X; Y = Y < 0 ? 0 : Y;           // never taken (rows, cols > T); keeps the read inside whatever the arguments
            atomicAdd(&h[src[(size_t)Y * A.cols + X]], 1u);
        }
    }
    __syncthreads();
    const uint4 hv = reinterpret_cast<const uint4 *>(h)[lane];
    unsigned b0 = hv.x, b1 = hv.y, b2 = hv.z, b3 = hv.w;
    const unsigned limit = (unsigned)A.limit[plane];
    unsigned ex = (b0 > limit ? b0 - limit : 0u) + (b1 > limit ? b1 - limit : 0u) + (b2 > limit ? b2 - limit : 0u) + (b3 > limit ? b3 - limit : 0u);
    b0 = b0 > limit ? limit : b0; b1 = b1 > limit ? limit : b1; b2 = b2 > limit ? limit : b2; b3 = b3 > limit ? limit : b3;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) ex += __shfl_xor(ex, d);
    const unsigned batch = ex >> 8, res = ex & 255u, step = res ? 256u / res : 1u;      // res <= 255: 256 / res >= 1
    const unsigned i0 = 4u * (unsigned)lane;
    b0 += batch + ((res && (i0 + 0) % step == 0 && (i0 + 0) / step < res) ? 1u : 0u);
    b1 += batch + ((res && (i0 + 1) % step == 0 && (i0 + 1) / step < res) ? 1u : 0u);
    b2 += batch + ((res && (i0 + 2) % step == 0 && (i0 + 2) / step < res) ? 1u : 0u);
    b3 += batch + ((res && (i0 + 3) % step == 0 && (i0 + 3) / step < res) ? 1u : 0u);
    b1 += b0; b2 += b1; b3 += b2;                          // inclusive within the lane
    unsigned s = b3;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(s, d);
        if (lane >= d) s += t;
    }
    const unsigned before = s - b3;
    const int l0 = prep_sat8(__float2int_rn((float)(before + b0) * A.scale)), l1 = prep_sat8(__float2int_rn((float)(before + b1) * A.scale));
    const int l2 = prep_sat8(__float2int_rn((float)(before + b2) * A.scale)), l3 = prep_sat8(__float2int_rn((float)(before + b3) * A.scale));
    if (valid) lut[(size_t)tp * 64 + lane] = (unsigned)l0 | (unsigned)l1 << 8 | (unsigned)l2 << 16 | (unsigned)l3 << 24;
}

struct PrepApplyArgs { PrepDims D; int T; float inv_tw, inv_th; };              // 1.0f / (float)tw, 1.0f / (float)th

struct PrepBlend { int t1, t2; float a, a1; };
__device__ __forceinline__ PrepBlend prep_blend(int x, float inv, int T) {
    PrepBlend b;
    const float tf = (float)x * inv - 0.5f;
    const float fl = floorf(tf);
    b.t1 = (int)fl;
    b.a = tf - fl;
    b.a1 = 1.0f - b.a;
    b.t2 = b.t1 + 1;
    if (b.t1 < 0) b.t1 = 0;
    if (b.t2 > T - 1) b.t2 = T - 1;
    if (b.t1 > T - 1) b.t1 = T - 1;                        // never taken: x inv - 0.5 < T - 0.5 up to rounding; keeps the read inside
    return b;
}
__device__ __forceinline__ int prep_lookup(const unsigned char *lut, int T, const PrepBlend &bx, const PrepBlend &by, int v) {
    const float l11 = (float)lut[((size_t)(by.t1 * T + bx.t1) << 8) + v], l12 = (float)lut[((size_t)(by.t1 * T + bx.t2) << 8) + v];
    const float l21 = (float)lut[((size_t)(by.t2 * T + bx.t1) << 8) + v], l22 = (float)lut[((size_t)(by.t2 * T + bx.t2) << 8) + v];
    return prep_sat8(__float2int_rn((l11 * bx.a1 + l12 * bx.a) * by.a1 + (l21 * bx.a1 + l22 * bx.a) * by.a));
}

__global__ void __launch_bounds__(256) k_prep_apply(const unsigned *__restrict__ gray, const unsigned *__restrict__ yy, const uint2 *__restrict__ crcb,
                                                    const unsigned char *__restrict__ lut, unsigned *__restrict__ gray_eq, unsigned *__restrict__ bgr_eq,
                                                    PrepApplyArgs A, int ngroups) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= ngroups) return;
    const unsigned gw = gray[g], yw = yy[g];
    const uint2 cv = crcb[g];
    const unsigned cw[2] = {cv.x, cv.y};
    const unsigned char *lut_y = lut + ((size_t)A.T * A.T << 8);
    int x, y;
    prep_first(A.D, g, &x, &y);
    unsigned ub[12], ow = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const PrepBlend bx = prep_blend(x, A.inv_tw, A.T), by = prep_blend(y, A.inv_th, A.T);
        ow |= (unsigned)prep_lookup(lut, A.T, bx, by, (int)((gw >> (8 * k)) & 255u)) << (8 * k);
        const int Y = prep_lookup(lut_y, A.T, bx, by, (int)((yw >> (8 * k)) & 255u));
        const unsigned cc = cw[k >> 1] >> (16 * (k & 1));
        const int Cr = (int)(cc & 255u), Cb = (int)((cc >> 8) & 255u);
        ub[3 * k] = (unsigned)prep_sat8(Y + PREP_DESCALE((Cb - 128) * 29049, 14));
        ub[3 * k + 1] = (unsigned)prep_sat8(Y + PREP_DESCALE((Cb - 128) * (-5636) + (Cr - 128) * (-11698), 14));
        ub[3 * k + 2] = (unsigned)prep_sat8(Y + PREP_DESCALE((Cr - 128) * 22987, 14));
        prep_step(A.D, &x, &y);
    }
    gray_eq[g] = ow;
    bgr_eq[3 * (size_t)g] = ub[0] | ub[1] << 8 | ub[2] << 16 | ub[3] << 24;
    bgr_eq[3 * (size_t)g + 1] = ub[4] | ub[5] << 8 | ub[6] << 16 | ub[7] << 24;
    bgr_eq[3 * (size_t)g + 2] = ub[8] | ub[9] << 8 | ub[10] << 16 | ub[11] << 24;
}

// the maps, the five intermediate planes, the LUT, the two results and the resize's tables out of d_block (null: only measured); returns the block's size
size_t prep_layout(SrlImagePrep *p) {
    const size_t npix4 = ((size_t)p->rows * (size_t)p->cols + 3) / 4 * 4;
    SrlCarve c{p->d_block};
    p->d_map1 = c.take<short>(npix4 * 2); p->d_map2 = c.take<unsigned short>(npix4);
    p->d_undist = c.take<unsigned char>(npix4 * 3); p->d_gray = c.take<unsigned char>(npix4); p->d_y = c.take<unsigned char>(npix4);
    p->d_crcb = c.take<unsigned char>(npix4 * 2); p->d_lut = c.take<unsigned char>((size_t)2 * p->T * p->T * 256);
    p->d_gray_eq = c.take<unsigned char>(npix4); p->d_bgr_eq = c.take<unsigned char>(npix4 * 3);
    p->d_ofs_x = c.take<int>((size_t)p->cols); p->d_coef_x = c.take<unsigned>((size_t)p->cols);
    p->d_ofs_y = c.take<int>((size_t)p->rows); p->d_coef_y = c.take<unsigned>((size_t)p->rows);
    return c.at;
}

void prep_free(SrlImagePrep *p) {
    p->raw.release();
    p->src.release();
    if (p->d_block) hipFree(p->d_block);
}

void prep_info(const SrlImagePrep *p, int installed, srl_image_prep_info *info) {
    if (!info) return;
    info->tiles = p->T; info->tile_w = p->tw; info->tile_h = p->th; info->ext_rows = p->ext_rows; info->ext_cols = p->ext_cols;
    info->limit_gray = p->limit[0]; info->limit_color = p->limit[1]; info->installed_color = installed;
}

}  // namespace

extern "C" void srl_image_prep_opts_default(srl_image_prep_opts *o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->clip_gray = 3.0; o->clip_color = 1.0;               // :124, :195
}

extern "C" int srl_image_prep_build_map(const srl_image_prep_opts *o, int16_t *map1, uint16_t *map2) {
    PrepPlan plan;
    if (!o || !map1 || !map2 || !prep_plan(o, &plan)) return SRL_ERR_BAD_ARG;
    const double fx = o->fx, fy = o->fy, cx = o->cx, cy = o->cy, k1 = o->dist[0], k2 = o->dist[1], p1 = o->dist[2], p2 = o->dist[3], k3 = o->dist[4];
    for (int i = 0; i < o->rows; i++) {
        const double y = (i - cy) / fy;
        for (int j = 0; j < o->cols; j++) {
            const double x = (j - cx) / fx;
            const double r2 = x * x + y * y;
            const double kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2;
            const double xd = x * kr + (p1 * (2 * x * y) + p2 * (r2 + 2 * x * x));
            const double yd = y * kr + (p1 * (r2 + 2 * y * y) + p2 * (2 * x * y));
            const double u = fx * xd + cx, v = fy * yd + cy;
            const size_t at = (size_t)i * o->cols + j;
            const double u32 = u * 32, v32 = v * 32;
            // (NaN fails both comparisons' complement: !(a < b) is true for it)
            if (!(std::fabs(u32) < 2147483647.0) || !(std::fabs(v32) < 2147483647.0)) {
                map1[2 * at] = -32768; map1[2 * at + 1] = -32768; map2[at] = 0;
                continue;
            }
            const int32_t iu = (int32_t)std::nearbyint(u32), iv = (int32_t)std::nearbyint(v32);      // round to nearest even (the default mode)
            const int32_t sx = iu >> 5, sy = iv >> 5;
            map1[2 * at] = (int16_t)(sx < -32768 ? -32768 : (sx > 32767 ? 32767 : sx));
            map1[2 * at + 1] = (int16_t)(sy < -32768 ? -32768 : (sy > 32767 ? 32767 : sy));
            map2[at] = (uint16_t)((iv & 31) * 32 + (iu & 31));
        }
    }
    return SRL_OK;
}

extern "C" int srl_image_prep_create(srl_ctx *ctx, const srl_image_prep_opts *o) {
    PrepPlan plan;
    if (!ctx || !o) return SRL_ERR_BAD_ARG;
    if (!prep_plan(o, &plan)) {
        ctx->err = "image preparer options: rows, cols 16 ... 16384 and more than the tiles per side, finite intrinsics with fx, fy != 0, finite positive clips, "
                   "tiles 0 or 2 ... min(rows, cols) / 2";
        return SRL_ERR_BAD_ARG;
    }
    if (ctx->prep) { ctx->err = "an image preparer exists: its options hold for its life (srl_image_prep_destroy first)"; return SRL_ERR_BAD_ARG; }
    { const int rc = srl_prep_one_rank(ctx); if (rc) return rc; }
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)o->rows * (size_t)o->cols, npix4 = (npix + 3) / 4 * 4;
    std::vector<int16_t> m1(npix4 * 2, (int16_t)-32768);
    std::vector<uint16_t> m2(npix4, (uint16_t)0);
    { const int rc = srl_image_prep_build_map(o, m1.data(), m2.data()); if (rc) return rc; }
    SrlImagePrep *p = new SrlImagePrep();
    p->opts = *o; p->rows = o->rows; p->cols = o->cols;
    p->T = plan.T; p->tw = plan.tw; p->th = plan.th; p->ext_rows = plan.ext_rows; p->ext_cols = plan.ext_cols;
    p->limit[0] = plan.limit[0]; p->limit[1] = plan.limit[1];
    // (the upload's device side has the planes' slack of up to three pixels)
    { const int rc = p->raw.reserve(ctx, npix * 3, npix4 * 3); if (rc) { prep_free(p); delete p; return rc; } }
    hipError_t e = hipMalloc((void **)&p->d_block, prep_layout(p));
    // the maps once per preparer (a pageable source: the copies are made before the calls return)
    if (e == hipSuccess) { prep_layout(p); e = hipMemcpy(p->d_map1, m1.data(), npix4 * 2 * sizeof(short), hipMemcpyHostToDevice); }
    if (e == hipSuccess) e = hipMemcpy(p->d_map2, m2.data(), npix4 * sizeof(unsigned short), hipMemcpyHostToDevice);
    if (e != hipSuccess) { prep_free(p); delete p; HIPCHK(ctx, e); }
    ctx->prep = p;
    return SRL_OK;
}

extern "C" int srl_image_prep_destroy(srl_ctx *ctx) {
    if (!ctx) return SRL_ERR_BAD_ARG;
    SrlImagePrep *p = ctx->prep;
    if (!p) return SRL_OK;
    SRL_DISARM(ctx);
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    prep_free(p);
    delete p;
    ctx->prep = nullptr;
    return SRL_OK;
}

namespace {

// the three kernels over `frame` (rows x cols x 3 of the preparer's size on the device: uploaded, resized into raw.d, or decoded), the
// hand-over to the colour map and the wait
int prep_chain(srl_ctx *ctx, SrlImagePrep *p, const unsigned char *frame, srl_image_prep_info *info) {
    hipStream_t st = ctx->stream;
    const int rows = p->rows, cols = p->cols;
    const size_t npix = (size_t)rows * (size_t)cols;
    const int ngroups = (int)((npix + 3) / 4);
    const unsigned nb = (unsigned)((ngroups + 255) / 256);
    const PrepDims D = {rows, cols, (int)npix};
    hipLaunchKernelGGL(k_prep_pixel, dim3(nb), dim3(256), 0, st, frame, reinterpret_cast<const uint4 *>(p->d_map1), reinterpret_cast<const uint2 *>(p->d_map2),
                       reinterpret_cast<unsigned *>(p->d_undist), reinterpret_cast<unsigned *>(p->d_gray), reinterpret_cast<unsigned *>(p->d_y),
                       reinterpret_cast<uint2 *>(p->d_crcb), D, ngroups);
    PrepTileArgs TA;
    TA.rows = rows; TA.cols = cols; TA.T = p->T; TA.tw = p->tw; TA.th = p->th; TA.limit[0] = p->limit[0]; TA.limit[1] = p->limit[1];
    TA.scale = 255.0f / (float)(p->tw * p->th);
    const unsigned tile_planes = 2u * (unsigned)p->T * (unsigned)p->T;
    hipLaunchKernelGGL(k_prep_tiles, dim3((tile_planes + 3) / 4), dim3(256), 0, st, p->d_gray, p->d_y, reinterpret_cast<unsigned *>(p->d_lut), TA);
    PrepApplyArgs AA;
    AA.D = D; AA.T = p->T; AA.inv_tw = 1.0f / (float)p->tw; AA.inv_th = 1.0f / (float)p->th;
    hipLaunchKernelGGL(k_prep_apply, dim3(nb), dim3(256), 0, st, reinterpret_cast<const unsigned *>(p->d_gray), reinterpret_cast<const unsigned *>(p->d_y),
                       reinterpret_cast<const uint2 *>(p->d_crcb), p->d_lut, reinterpret_cast<unsigned *>(p->d_gray_eq), reinterpret_cast<unsigned *>(p->d_bgr_eq), AA,
                       ngroups);
    HIPCHK(ctx, hipGetLastError());
    int installed = 0;
    if (ctx->color) {
        const int rc = srl_color_image_install(ctx, p->d_bgr_eq, rows, cols);
        if (rc) return rc;
        installed = 1;
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    p->have_image = true;
    p->d_frame = frame;
    prep_info(p, installed, info);
    return SRL_OK;
}

// the tables of a source size on the device: built at its first use, rebuilt when it changes
int prep_resize_tables(srl_ctx *ctx, SrlImagePrep *p, int src_rows, int src_cols) {
    if (p->tab_rows == src_rows && p->tab_cols == src_cols) return SRL_OK;
    const int len[2] = {p->cols, p->rows}, from[2] = {src_cols, src_rows};
    int *d_ofs[2] = {p->d_ofs_x, p->d_ofs_y};
    unsigned *d_coef[2] = {p->d_coef_x, p->d_coef_y};
    p->tab_rows = p->tab_cols = 0;
    for (int k = 0; k < 2; k++) {
        std::vector<int32_t> ofs((size_t)len[k]);
        std::vector<int16_t> coef((size_t)len[k] * 2);
        { const int rc = srl_image_resize_build_tables(from[k], len[k], ofs.data(), coef.data()); if (rc) return rc; }
        // (pageable sources: the copies are made before the calls return; the last call ended synchronised)
        HIPCHK(ctx, hipMemcpy(d_ofs[k], ofs.data(), ofs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(d_coef[k], coef.data(), coef.size() * sizeof(int16_t), hipMemcpyHostToDevice));
    }
    p->tab_rows = src_rows; p->tab_cols = src_cols;
    return SRL_OK;
}

}  // namespace

int srl_prep_run_device(srl_ctx *ctx, const unsigned char *d_bgr, int src_rows, int src_cols, srl_image_prep_info *info) {
    SrlImagePrep *p = ctx->prep;
    if (src_rows == p->rows && src_cols == p->cols) return prep_chain(ctx, p, d_bgr, info);      // the preparer's own size: no resize kernel
    const bool half = src_cols == 2 * p->cols && src_rows == 2 * p->rows;
    if (!half) { const int rc = prep_resize_tables(ctx, p, src_rows, src_cols); if (rc) return rc; }
    const size_t npix = (size_t)p->rows * (size_t)p->cols;
    const int ngroups = (int)((npix + 3) / 4);
    const unsigned nb = (unsigned)((ngroups + 255) / 256);
    PrepResizeArgs RA;
    RA.D = {p->rows, p->cols, (int)npix}; RA.src_rows = src_rows; RA.src_cols = src_cols;
    if (half)
        hipLaunchKernelGGL(k_resize_bgr<true>, dim3(nb), dim3(256), 0, ctx->stream, d_bgr, p->d_ofs_x, p->d_coef_x, p->d_ofs_y, p->d_coef_y,
                           reinterpret_cast<unsigned *>(p->raw.d), RA, ngroups);
    else
        hipLaunchKernelGGL(k_resize_bgr<false>, dim3(nb), dim3(256), 0, ctx->stream, d_bgr, p->d_ofs_x, p->d_coef_x, p->d_ofs_y, p->d_coef_y,
                           reinterpret_cast<unsigned *>(p->raw.d), RA, ngroups);
    return prep_chain(ctx, p, p->raw.d, info);
}

extern "C" int srl_image_prepare(srl_ctx *ctx, const uint8_t *raw_bgr, int rows, int cols, int64_t row_stride_bytes, srl_image_prep_info *info) {
    if (info) std::memset(info, 0, sizeof *info);
    if (!ctx || !raw_bgr) return SRL_ERR_BAD_ARG;
    { const int rc = srl_prep_need(ctx, false); if (rc) return rc; }
    SrlImagePrep *p = ctx->prep;
    if (rows != p->rows || cols != p->cols) { ctx->err = "image preparer: the image size differs from the preparer's"; return SRL_ERR_BAD_ARG; }
    if (row_stride_bytes < (int64_t)cols * 3) return SRL_ERR_BAD_ARG;
    { const int rc = srl_prep_one_rank(ctx); if (rc) return rc; }
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // every call ends synchronised, so the staging block is free
    { const int rc = p->raw.upload(ctx, raw_bgr, rows, (size_t)cols * 3, row_stride_bytes); if (rc) return rc; }
    return srl_prep_run_device(ctx, p->raw.d, rows, cols, info);
}

extern "C" int srl_image_resize_build_tables(int src_len, int dst_len, int32_t *ofs, int16_t *coef) {
    if (src_len < 1 || dst_len < 1 || !ofs || !coef) return SRL_ERR_BAD_ARG;
    const double scale = (double)src_len / dst_len;
    for (int d = 0; d < dst_len; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f = f - (float)s;
        if (s < 0) { s = 0; f = 0.0f; }
        if (s >= src_len - 1) { s = src_len - 1; f = 0.0f; }
        ofs[d] = s;
        coef[2 * d] = (int16_t)std::nearbyint((1.0f - f) * 2048.0f);          // round to nearest even (the default mode)
        coef[2 * d + 1] = (int16_t)std::nearbyint(f * 2048.0f);
    }
    return SRL_OK;
}

extern "C" int srl_image_prepare_resized(srl_ctx *ctx, const uint8_t *raw_bgr, int src_rows, int src_cols, int64_t row_stride_bytes, srl_image_prep_info *info) {
    if (info) std::memset(info, 0, sizeof *info);
    if (!ctx || !raw_bgr) return SRL_ERR_BAD_ARG;
    { const int rc = srl_prep_need(ctx, false); if (rc) return rc; }
    SrlImagePrep *p = ctx->prep;
    if (src_rows < 1 || src_cols < 1 || src_rows > SRL_FLOW_MAX_EXTENT || src_cols > SRL_FLOW_MAX_EXTENT || (int64_t)src_rows * src_cols > SRL_COLOR_IMAGE_MAX_PIXELS) {
        ctx->err = "image preparer: a source frame of 1 ... 16384 rows and columns and at most SRL_COLOR_IMAGE_MAX_PIXELS pixels";
        return SRL_ERR_BAD_ARG;
    }
    if (row_stride_bytes < (int64_t)src_cols * 3) return SRL_ERR_BAD_ARG;
    { const int rc = srl_prep_one_rank(ctx); if (rc) return rc; }
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (src_rows == p->rows && src_cols == p->cols) {          // the preparer's own size: srl_image_prepare, no resize kernel
        { const int rc = p->raw.upload(ctx, raw_bgr, src_rows, (size_t)src_cols * 3, row_stride_bytes); if (rc) return rc; }
        return srl_prep_run_device(ctx, p->raw.d, src_rows, src_cols, info);
    }
    const size_t src_bytes = (size_t)src_rows * (size_t)src_cols * 3;
    { const int rc = p->src.reserve(ctx, src_bytes, src_bytes); if (rc) return rc; }
    { const int rc = p->src.upload(ctx, raw_bgr, src_rows, (size_t)src_cols * 3, row_stride_bytes); if (rc) return rc; }
    return srl_prep_run_device(ctx, p->src.d, src_rows, src_cols, info);
}

extern "C" int srl_image_prep_download(srl_ctx *ctx, int which, uint8_t *out, int64_t row_stride_bytes) {
    if (!ctx || !out || (which != 0 && which != 1)) return SRL_ERR_BAD_ARG;
    { const int rc = srl_prep_need(ctx, true); if (rc) return rc; }
    SrlImagePrep *p = ctx->prep;
    const size_t row_bytes = (size_t)p->cols * (which ? 3 : 1);
    if (row_stride_bytes < (int64_t)row_bytes) return SRL_ERR_BAD_ARG;
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy2D(out, (size_t)row_stride_bytes, which ? p->d_bgr_eq : p->d_gray_eq, row_bytes, row_bytes, (size_t)p->rows, hipMemcpyDeviceToHost));
    return SRL_OK;
}

extern "C" int srl_image_prep_download_stage(srl_ctx *ctx, int stage, uint8_t *out, int64_t capacity) {
    if (!ctx || !out || stage < SRL_PREP_STAGE_UNDIST || stage > SRL_PREP_STAGE_LUT_Y) return SRL_ERR_BAD_ARG;
    { const int rc = srl_prep_need(ctx, true); if (rc) return rc; }
    SrlImagePrep *p = ctx->prep;
    const size_t npix = (size_t)p->rows * (size_t)p->cols, lut_bytes = (size_t)p->T * p->T * 256;
    const size_t need = stage == SRL_PREP_STAGE_GRAY ? npix : (stage >= SRL_PREP_STAGE_LUT_GRAY ? lut_bytes : npix * 3);
    if (capacity < (int64_t)need) return SRL_ERR_BAD_ARG;
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (stage == SRL_PREP_STAGE_YCRCB) {                   // the Y plane, then the (Cr, Cb) pairs
        HIPCHK(ctx, hipMemcpy(out, p->d_y, npix, hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(out + npix, p->d_crcb, npix * 2, hipMemcpyDeviceToHost));
        return SRL_OK;
    }
    const unsigned char *src = stage == SRL_PREP_STAGE_UNDIST ? p->d_undist : stage == SRL_PREP_STAGE_GRAY ? p->d_gray
                               : p->d_lut + (stage == SRL_PREP_STAGE_LUT_Y ? lut_bytes : 0);
    HIPCHK(ctx, hipMemcpy(out, src, need, hipMemcpyDeviceToHost));
    return SRL_OK;
}

extern "C" int srl_image_prep_download_resized(srl_ctx *ctx, uint8_t *out, int64_t capacity) {
    if (!ctx || !out) return SRL_ERR_BAD_ARG;
    { const int rc = srl_prep_need(ctx, true); if (rc) return rc; }
    SrlImagePrep *p = ctx->prep;
    const size_t need = (size_t)p->rows * (size_t)p->cols * 3;
    if (capacity < (int64_t)need) return SRL_ERR_BAD_ARG;
    if (!p->d_frame) { ctx->err = "image preparer: the decoded frame the last chain read has been replaced since"; return SRL_ERR_NO_SWEEP; }
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, p->d_frame, need, hipMemcpyDeviceToHost));
    return SRL_OK;
}

// srl_jpeg.hip -- a baseline JPEG frame from its quantised coefficients to packed BGR on the device for gfx950 (include/srlivo_hip.h: the
// specification; srl_jpeg_scan.cpp: the host's entropy decode that fills the staging block).  Integer arithmetic only, no atomics: the same
// stream gives the same bytes, and they are libjpeg's (JDCT_ISLOW, fancy upsampling, 16-bit colour tables).
//
//   k_jpeg_idct   eight lanes per 8 x 8 block, 32 blocks per workgroup.  Lane r loads coefficient row r (16 bytes) and its table row and
//                 dequantises; the block is turned through LDS (rows of 9 words: lane (block b, r) touches word 72 b + 9 r + k, and
//                 8 b + 9 r + k mod 64 is distinct over a wave for writes by row and reads by column alike); the lane runs COLUMN r
//                 (pass 1, DESCALE 11), the results are turned back, the lane runs ROW r (pass 2, DESCALE 18), applies the range
//                 limit and stores its eight samples as one 8-byte word into the component plane.  All components in one launch.
//                 WIDE = false: 32-bit registers.  Every intermediate of a 1-D pass is a linear form of its eight inputs; over all of
//                 them (every sub-expression as written below) the largest single |coefficient| is g = 27431 and, over the eight
//                 results, gout = 11363 (tests/test_jpeg_guard.py recomputes both from the checker's pass).  With L1 = the block's
//                 sum of |coef qt|: a pass-1 intermediate is at most g L1 + 2^10; |ws| <= gout (column's L1) / 2^11 + 1, so a row of
//                 ws sums to at most gout L1 / 2^11 + 8, and a pass-2 intermediate is at most g (gout L1 / 2^11 + 8) + 2^17.  For
//                 L1 <= SRL_JPEG_L1_INT32 = 14000 that is 2 131 108 307 < 2^31.  The host knows the frame's largest L1 from the entropy
//                 decode (srl_jpeg_entropy_decode_l1); a frame above the limit runs WIDE = true: 64-bit registers, libjpeg's JLONG, where
//                 |coef qt| <= 32767 x 255 keeps pass 1 below 2^41 and its results (an int in libjpeg) below 2^30.
//   k_jpeg_color  four destination pixels of the flat image per lane as in k_prep_pixel, every store an aligned dword: Y from its
//                 plane, Cb and Cr from theirs through the upsampling rule of the frame's sampling, then the colour conversion.
//
// Bounds: a block index is below total_blocks, and its 8 x 8 samples lie inside its component's padded plane, which the planes block
// holds whole.  A chroma sample is read at row near / far in 0 ... ch - 1 and column i - 1 ... i + 1 clamped by the rule's own edge cases
// to 0 ... cw - 1, real sizes that never exceed the padded ones.  The BGR frame has room for the pixel count rounded up to four.
#include "srl_image_prep.h"
#include "srl_jpeg_scan.h"
#include "../../include/srlivo_hip_debug.h"

#include <cstring>
#include <type_traits>

#define SRL_JPEG_L1_INT32 14000

struct SrlJpeg {
    unsigned char *h_stage = nullptr;      // page-locked: the tables (3 x 64 uint16), then the coefficients (64 int16 per block)
    unsigned char *d_coef = nullptr;       // the same bytes on the device
    unsigned char *d_planes = nullptr;     // the component planes, padded to whole MCUs, one after the other: 64 bytes per block
    unsigned char *d_bgr = nullptr;        // rows x cols x 3, packed, for the pixel count rounded up to a multiple of 4
    size_t stage_cap = 0, coef_cap = 0, planes_cap = 0, bgr_cap = 0;      // bytes
    srl_jpeg_info info = {};               // of the frame in d_bgr
    bool have_frame = false;
};

namespace {

constexpr size_t JPEG_QT_BYTES = 3 * 64 * sizeof(uint16_t);      // 384: the coefficients behind it stay 16-byte aligned

// one 1-D pass of jidctint.c on d[0] ... d[7], in place
template <class T>
__device__ __forceinline__ void jpeg_idct_pass(T (&d)[8], int shift) {
    T z1 = (d[2] + d[6]) * (T)4433;
    const T t2 = z1 + d[6] * (T)(-15137);
    const T t3 = z1 + d[2] * (T)6270;
    const T t0 = (d[0] + d[4]) * (T)8192;
    const T t1 = (d[0] - d[4]) * (T)8192;
    const T t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    T o0 = d[7], o1 = d[5], o2 = d[3], o3 = d[1];
    z1 = o0 + o3;
    T z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const T z5 = (z3 + z4) * (T)9633;
    o0 = o0 * (T)2446; o1 = o1 * (T)16819; o2 = o2 * (T)25172; o3 = o3 * (T)12299;
    z1 = z1 * (T)(-7373); z2 = z2 * (T)(-20995); z3 = z3 * (T)(-16069); z4 = z4 * (T)(-3196);
    z3 += z5; z4 += z5;
    o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
    const T half = (T)1 << (shift - 1);
    d[0] = (t10 + o3 + half) >> shift; d[7] = (t10 - o3 + half) >> shift;
    d[1] = (t11 + o2 + half) >> shift; d[6] = (t11 - o2 + half) >> shift;
    d[2] = (t12 + o1 + half) >> shift; d[5] = (t12 - o1 + half) >> shift;
    d[3] = (t13 + o0 + half) >> shift; d[4] = (t13 - o0 + half) >> shift;
}

// libjpeg's range-limit table behind IDCT results, through its index
__device__ __forceinline__ unsigned jpeg_range_limit(int idx) {
    idx &= 0x3FF;
    return (unsigned)(idx < 128 ? idx + 128 : (idx < 512 ? 255 : (idx < 896 ? 0 : idx - 896)));
}

struct JpegIdctArgs {
    long long base[3];      // first block of each component (absent ones: total)
    int wb[3];              // blocks per row of its padded plane
    long long total;
};

template <bool WIDE>
__global__ void __launch_bounds__(256) k_jpeg_idct(const uint4 *__restrict__ coef, const uint4 *__restrict__ qt, unsigned char *__restrict__ planes, JpegIdctArgs A) {
    typedef typename std::conditional<WIDE, long long, int>::type T;
    __shared__ T s[32][72];
    const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
    const long long blk = (long long)blockIdx.x * 32 + lb;
    const bool valid = blk < A.total;
    const int c = !valid ? 0 : (blk >= A.base[2] ? 2 : (blk >= A.base[1] ? 1 : 0));
    const uint4 cv = valid ? coef[blk * 8 + r] : make_uint4(0, 0, 0, 0);
    const uint4 qv = qt[c * 8 + r];
    const unsigned cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
    T d[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        d[2 * k] = (T)((int)(short)(cw[k] & 0xFFFFu) * (int)(qw[k] & 0xFFFFu));
        d[2 * k + 1] = (T)((int)(short)(cw[k] >> 16) * (int)(qw[k] >> 16));
    }
#pragma unroll
    for (int k = 0; k < 8; k++) s[lb][r * 9 + k] = d[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = s[lb][k * 9 + r];      // column r
    jpeg_idct_pass<T>(d, 11);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) s[lb][k * 9 + r] = d[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = s[lb][r * 9 + k];      // row r
    jpeg_idct_pass<T>(d, 18);
    if (!valid) return;
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        lo |= jpeg_range_limit((int)d[k]) << (8 * k);
        hi |= jpeg_range_limit((int)d[4 + k]) << (8 * k);
    }
    const long long local = blk - A.base[c];
    const long long by = local / A.wb[c], bx = local - by * A.wb[c];
    unsigned char *at = planes + A.base[c] * 64 + ((by * 8 + r) * A.wb[c] + bx) * 8;
    *reinterpret_cast<uint2 *>(at) = make_uint2(lo, hi);
}

enum { JPEG_GRAY = 0, JPEG_444 = 1, JPEG_H2V1 = 2, JPEG_H2V2 = 3 };
struct JpegColorArgs {
    PrepDims D;
    int mode;
    int y_stride, c_stride;      // bytes per row of the padded luma / chroma planes
    int cw, ch;                  // the chroma planes' real size
};

__device__ __forceinline__ int jpeg_sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// one chroma sample of pixel (x, y) by the frame's upsampling rule
__device__ __forceinline__ int jpeg_chroma(const unsigned char *__restrict__ C, const JpegColorArgs &A, int x, int y) {
    if (A.mode == JPEG_444) return C[(size_t)y * A.c_stride + x];
    const int i = x >> 1;
    if (A.mode == JPEG_H2V1) {
        const unsigned char *row = C + (size_t)y * A.c_stride;
        const int cur = row[i];
        if (x & 1) return i == A.cw - 1 ? cur : (3 * cur + row[i + 1] + 2) >> 2;
        return i == 0 ? cur : (3 * cur + row[i - 1] + 1) >> 2;
    }
    const int near = y >> 1;
    int far = (y & 1) ? near + 1 : near - 1;
    far = far < 0 ? 0 : (far > A.ch - 1 ? A.ch - 1 : far);
    const unsigned char *rn = C + (size_t)near * A.c_stride, *rf = C + (size_t)far * A.c_stride;
    const int cur = 3 * rn[i] + rf[i];
    if (x & 1) return i == A.cw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + (3 * rn[i + 1] + rf[i + 1]) + 7) >> 4;
    return i == 0 ? (4 * cur + 8) >> 4 : (3 * cur + (3 * rn[i - 1] + rf[i - 1]) + 8) >> 4;
}

__global__ void __launch_bounds__(256) k_jpeg_color(const unsigned char *__restrict__ Yp, const unsigned char *__restrict__ Cb, const unsigned char *__restrict__ Cr,
                                                    unsigned *__restrict__ bgr, JpegColorArgs A, int ngroups) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= ngroups) return;
    int x, y;
    prep_first(A.D, g, &x, &y);
    unsigned ub[12];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int Y = Yp[(size_t)y * A.y_stride + x];
        if (A.mode == JPEG_GRAY) {
            ub[3 * k] = ub[3 * k + 1] = ub[3 * k + 2] = (unsigned)Y;
        } else {
            const int cb = jpeg_chroma(Cb, A, x, y) - 128, cr = jpeg_chroma(Cr, A, x, y) - 128;
            ub[3 * k] = (unsigned)jpeg_sat8(Y + ((116130 * cb + 32768) >> 16));
            ub[3 * k + 1] = (unsigned)jpeg_sat8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
            ub[3 * k + 2] = (unsigned)jpeg_sat8(Y + ((91881 * cr + 32768) >> 16));
        }
        prep_step(A.D, &x, &y);
    }
    bgr[3 * (size_t)g] = ub[0] | ub[1] << 8 | ub[2] << 16 | ub[3] << 24;
    bgr[3 * (size_t)g + 1] = ub[4] | ub[5] << 8 | ub[6] << 16 | ub[7] << 24;
    bgr[3 * (size_t)g + 2] = ub[8] | ub[9] << 8 | ub[10] << 16 | ub[11] << 24;
}

// a block of the decoder grown by doubling; what it held is gone
int jpeg_grow(srl_ctx *ctx, unsigned char *&p, size_t &cap, size_t need, bool host) {
    if (need <= cap) return SRL_OK;
    const size_t want = need > 2 * cap ? need : 2 * cap;
    if (p) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, host ? hipHostFree(p) : hipFree(p));
        p = nullptr; cap = 0;
    }
    if (host) HIPCHK(ctx, hipHostMalloc((void **)&p, want, hipHostMallocDefault));
    else HIPCHK(ctx, hipMalloc((void **)&p, want));
    cap = want;
    return SRL_OK;
}

void jpeg_launch_idct(hipStream_t st, bool wide, const unsigned char *d_coef, unsigned char *d_planes, const JpegIdctArgs &A) {
    const unsigned nb = (unsigned)((A.total + 31) / 32);
    const uint4 *qt = reinterpret_cast<const uint4 *>(d_coef), *coef = reinterpret_cast<const uint4 *>(d_coef + JPEG_QT_BYTES);
    if (wide) hipLaunchKernelGGL(k_jpeg_idct<true>, dim3(nb), dim3(256), 0, st, coef, qt, d_planes, A);
    else hipLaunchKernelGGL(k_jpeg_idct<false>, dim3(nb), dim3(256), 0, st, coef, qt, d_planes, A);
}

// srl_jpeg_decode behind the argument checks: parse, entropy decode into staging, one upload, the two kernels, the wait
int jpeg_decode(srl_ctx *ctx, const uint8_t *bytes, int64_t n, srl_jpeg_info *info) {
    srl_jpeg_info I;
    {
        const int rc = srl_jpeg_parse(bytes, n, &I);
        if (rc) { ctx->err = rc == SRL_ERR_UNSUPPORTED ? "JPEG: outside what srl_jpeg_parse accepts (baseline, 8 bit, 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0, one scan)" : "JPEG: malformed header"; return rc; }
    }
    if (I.rows > SRL_FLOW_MAX_EXTENT || I.cols > SRL_FLOW_MAX_EXTENT || (int64_t)I.rows * I.cols > SRL_COLOR_IMAGE_MAX_PIXELS) {
        ctx->err = "JPEG: a frame of more than 16384 rows or columns or SRL_COLOR_IMAGE_MAX_PIXELS pixels";
        return SRL_ERR_UNSUPPORTED;
    }
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->jpeg) ctx->jpeg = new SrlJpeg();
    SrlJpeg *J = ctx->jpeg;
    const size_t coef_bytes = JPEG_QT_BYTES + (size_t)I.total_blocks * 128;
    // every call ends synchronised, so the staging block is free
    { const int rc = jpeg_grow(ctx, J->h_stage, J->stage_cap, coef_bytes, true); if (rc) return rc; }
    int64_t l1 = 0;
    std::memset(J->h_stage, 0, JPEG_QT_BYTES);
    {
        const int rc = srl_jpeg_entropy_decode_l1(bytes, n, &I, reinterpret_cast<int16_t *>(J->h_stage + JPEG_QT_BYTES), I.total_blocks,
                                                  reinterpret_cast<uint16_t(*)[64]>(J->h_stage), &l1);
        if (rc) { ctx->err = "JPEG: malformed scan"; return rc; }
    }
    // ---- the stream is good: from here on the previous frame is replaced
    const size_t npix = (size_t)I.rows * (size_t)I.cols, npix4 = (npix + 3) / 4 * 4;
    { const int rc = jpeg_grow(ctx, J->d_coef, J->coef_cap, coef_bytes, false); if (rc) return rc; }
    { const int rc = jpeg_grow(ctx, J->d_planes, J->planes_cap, (size_t)I.total_blocks * 64, false); if (rc) return rc; }
    J->have_frame = false;
    // the frame the preparer's last chain read, if it was this block's, is about to be overwritten or freed: srl_image_prep_download_resized
    // must not hand out another frame, nor read a freed block (srl_image_prepare_jpeg sets it again behind its chain)
    if (ctx->prep && J->d_bgr && ctx->prep->d_frame == J->d_bgr) ctx->prep->d_frame = nullptr;
    { const int rc = jpeg_grow(ctx, J->d_bgr, J->bgr_cap, npix4 * 3, false); if (rc) return rc; }
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(J->d_coef, J->h_stage, coef_bytes, hipMemcpyHostToDevice, st));
    JpegIdctArgs IA;
    IA.total = I.total_blocks;
    for (int c = 0; c < 3; c++) {
        IA.base[c] = c < I.components ? (c ? IA.base[c - 1] + I.blocks[c - 1] : 0) : I.total_blocks;
        IA.wb[c] = c < I.components ? I.mcus_per_row * I.h[c] : 1;
    }
    jpeg_launch_idct(st, l1 > SRL_JPEG_L1_INT32, J->d_coef, J->d_planes, IA);
    JpegColorArgs CA;
    CA.D = {I.rows, I.cols, (int)npix};
    CA.mode = I.components == 1 ? JPEG_GRAY : (I.h[0] == 1 ? JPEG_444 : (I.v[0] == 1 ? JPEG_H2V1 : JPEG_H2V2));
    CA.y_stride = IA.wb[0] * 8; CA.c_stride = IA.wb[1] * 8;
    CA.cw = CA.mode == JPEG_444 ? I.cols : (I.cols + 1) / 2;
    CA.ch = CA.mode == JPEG_H2V2 ? (I.rows + 1) / 2 : I.rows;
    const int ngroups = (int)(npix4 / 4);
    const unsigned char *Cb = J->d_planes + (I.components == 3 ? IA.base[1] * 64 : 0), *Cr = J->d_planes + (I.components == 3 ? IA.base[2] * 64 : 0);
    hipLaunchKernelGGL(k_jpeg_color, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, st, J->d_planes, Cb, Cr, reinterpret_cast<unsigned *>(J->d_bgr), CA, ngroups);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    J->info = I;
    J->have_frame = true;
    if (info) *info = I;
    return SRL_OK;
}

}  // namespace

extern "C" void srl_jpeg_release(srl_ctx *ctx) {
    SrlJpeg *J = ctx->jpeg;
    if (!J) return;
    if (J->h_stage) hipHostFree(J->h_stage);
    if (J->d_coef) hipFree(J->d_coef);
    if (J->d_planes) hipFree(J->d_planes);
    if (J->d_bgr) hipFree(J->d_bgr);
    delete J;
    ctx->jpeg = nullptr;
}

extern "C" int srl_jpeg_decode(srl_ctx *ctx, const uint8_t *bytes, int64_t n, srl_jpeg_info *info) {
    if (info) std::memset(info, 0, sizeof *info);
    if (!ctx || !bytes || n < 2) return SRL_ERR_BAD_ARG;
    { const int rc = srl_prep_one_rank(ctx); if (rc) return rc; }
    return jpeg_decode(ctx, bytes, n, info);
}

extern "C" int srl_jpeg_download(srl_ctx *ctx, uint8_t *out, int64_t row_stride_bytes) {
    if (!ctx || !out) return SRL_ERR_BAD_ARG;
    SrlJpeg *J = ctx->jpeg;
    if (!J || !J->have_frame) { ctx->err = "JPEG decoder: no frame yet (srl_jpeg_decode)"; return SRL_ERR_NO_SWEEP; }
    const size_t row_bytes = (size_t)J->info.cols * 3;
    if (row_stride_bytes < (int64_t)row_bytes) return SRL_ERR_BAD_ARG;
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy2D(out, (size_t)row_stride_bytes, J->d_bgr, row_bytes, row_bytes, (size_t)J->info.rows, hipMemcpyDeviceToHost));
    return SRL_OK;
}

extern "C" int srl_image_prepare_jpeg(srl_ctx *ctx, const uint8_t *bytes, int64_t n, srl_image_prep_info *info) {
    if (info) std::memset(info, 0, sizeof *info);
    if (!ctx || !bytes || n < 2) return SRL_ERR_BAD_ARG;
    { const int rc = srl_prep_need(ctx, false); if (rc) return rc; }
    { const int rc = srl_prep_one_rank(ctx); if (rc) return rc; }
    srl_jpeg_info I;
    { const int rc = jpeg_decode(ctx, bytes, n, &I); if (rc) return rc; }
    return srl_prep_run_device(ctx, ctx->jpeg->d_bgr, I.rows, I.cols, info);
}

extern "C" int srl_jpeg_idct_blocks(srl_ctx *ctx, const int16_t *coef, int64_t n_blocks, const uint16_t qt[64], uint8_t *out) {
    if (!ctx || !coef || !qt || !out || n_blocks < 1 || n_blocks > (1 << 20)) return SRL_ERR_BAD_ARG;
    { const int rc = srl_prep_one_rank(ctx); if (rc) return rc; }
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t coef_bytes = JPEG_QT_BYTES + (size_t)n_blocks * 128, plane_bytes = (size_t)n_blocks * 64;
    DevBuf in, planes;
    HIPCHK(ctx, in.alloc(ctx, coef_bytes));
    HIPCHK(ctx, planes.alloc(ctx, plane_bytes));
    // (pageable sources: the copies are made before the calls return)
    HIPCHK(ctx, hipMemsetAsync(in.p, 0, JPEG_QT_BYTES, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(in.p, qt, 64 * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(in.as<unsigned char>() + JPEG_QT_BYTES, coef, (size_t)n_blocks * 128, hipMemcpyHostToDevice));
    JpegIdctArgs IA;
    IA.total = n_blocks;
    IA.base[0] = 0; IA.base[1] = IA.base[2] = n_blocks;
    IA.wb[0] = IA.wb[1] = IA.wb[2] = 1;                      // one block per row: the plane IS the blocks, one after the other
    jpeg_launch_idct(ctx->stream, srl_jpeg_blocks_l1(coef, n_blocks, qt) > SRL_JPEG_L1_INT32, in.as<unsigned char>(), planes.as<unsigned char>(), IA);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(out, planes.p, plane_bytes, hipMemcpyDeviceToHost));
    return SRL_OK;
}

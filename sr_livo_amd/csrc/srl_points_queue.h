// srl_points_queue.h -- the device point queue as its two producers see it: srl_points.hip (Livox CustomMsg, the cut, the undistortion of
// the cut) and srl_pc2.hip (PointCloud2 of the spinning LiDARs).  One SoA block of five planes, head and size on the host, a small word
// block every call reports through.  Stated once so that both decodes append to the SAME FIFO.
#pragma once
#include "srl_ctx.h"

#include <limits>
#include <string>

enum { PL_X = 0, PL_Y, PL_Z, PL_REL, PL_TS, PL_COUNT };
// words of the small device block every call reports through (ints), and where its report record starts
enum { W_VALID = 0, W_LASTJ, W_APPENDED, W_CUT, W_N, W_NONMONO, W_FAIL, W_BAD, W_WORDS = 16 };
#define SRL_POINTS_WORD_BYTES 256
#define SRL_POINTS_QUEUE_MIN_CAP 4096

struct SrlPoints {
    double *q = nullptr;               // the queue: PL_COUNT planes, stride cap
    int cap = 0, head = 0, size = 0;
    double front_ts = std::numeric_limits<double>::quiet_NaN(), back_ts = std::numeric_limits<double>::quiet_NaN();
    double *c = nullptr;               // the resident cut: PL_COUNT planes, stride cut_cap
    int cut_cap = 0, cut_n = -1;       // -1: no cut yet
    double *t = nullptr;               // rewritten times of the undistorted sweep: timestamp | alpha_time, stride t_cap (relative_time: d_corr_rel)
    int t_cap = 0;
    int *d_words = nullptr;            // SRL_POINTS_WORD_BYTES: W_WORDS ints, then the report record
    char *h_words = nullptr;           // pinned copy
    long long fallbacks = 0;
};

namespace {

#if defined(__HIPCC__)
__device__ inline double d_nan() { return __longlong_as_double(0x7FF8000000000000LL); }
#endif

inline dim3 grid256(int n) { return dim3((unsigned)((n + 255) / 256)); }

inline int points_words(srl_ctx *ctx, SrlPoints &P) {
    if (!P.d_words) HIPCHK(ctx, hipMalloc((void **)&P.d_words, SRL_POINTS_WORD_BYTES));
    if (!P.h_words) HIPCHK(ctx, hipHostMalloc((void **)&P.h_words, SRL_POINTS_WORD_BYTES, hipHostMallocDefault));
    return SRL_OK;
}
// room for `add` more records behind the queue's back: a fresh block (doubled until it fits) with the live records at its front
inline int points_reserve(srl_ctx *ctx, SrlPoints &P, int add) {
    const long long need = (long long)P.size + add;
    if (P.q && (long long)P.head + need <= P.cap) return SRL_OK;
    long long cap = P.cap > 0 ? P.cap : SRL_POINTS_QUEUE_MIN_CAP;
    while (cap < need) cap *= 2;
    if (cap > (1ll << 28)) { ctx->err = "the point queue would exceed 2^28 records"; return SRL_ERR_UNSUPPORTED; }
    double *nq = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&nq, (size_t)cap * PL_COUNT * sizeof(double)));
    if (P.q) {
        hipError_t e = hipSuccess;
        for (int pl = 0; pl < PL_COUNT && P.size > 0 && e == hipSuccess; pl++)
            e = hipMemcpyAsync(nq + (size_t)pl * cap, P.q + (size_t)pl * P.cap + P.head, (size_t)P.size * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { (void)hipFree(nq); ctx->err = std::string("point queue growth: ") + hipGetErrorString(e); return SRL_ERR_HIP; }
        HIPCHK(ctx, hipFree(P.q));
    }
    P.q = nq; P.cap = (int)cap; P.head = 0;
    return SRL_OK;
}

}  // namespace

// srl_wg_totals.h -- internal: how a counting kernel of the colour map's consumers (srl_color_render.hip, srl_color_select.hip,
// srl_color_cloud.hip) turns per-thread counters into totals without a second launch and with ONE atomic per workgroup.  DESIGN.md
// section 3, "Totals of a counting kernel".  srl_color_vio.hip uses the host block and srl_wave_sum and keeps its own epilogue.
//
//   every workgroup   the counters are summed over each wave and left in LDS; thread 0 alone adds the waves, writes the workgroup's row
//                     (N agent-scope stores: they leave the L2 of this XCD, whose lines of the row array are shared with workgroups of
//                     other XCDs), fences, waits for its stores and takes a ticket
//   the last one      (the ticket says so) fences, and its first wave adds the columns of the gridDim.x rows up with agent-scope loads,
//                     writes the totals and sets the ticket back to zero for the next launch
// The row, the fence and the ticket lie in ONE thread's program order; the reader goes ticket, barrier, fence, agent-scope loads.  With
// every thread of a workgroup fencing instead, the tail was 351 of the 848 us of a 1.2 M-point cloud export.
//
// The block `tot` is the owner's: words [0, N) the totals of the last launch, word [N] the ticket, words behind it whatever the owner
// keeps there (they are never written here).  A launch that fails half-way leaves the ticket non-zero.
#pragma once
#include "srl_ctx.h"

struct SrlWgTotals {
    unsigned long long *d_tot = nullptr;      // the block: allocated and zeroed at first use
    unsigned long long *d_rows = nullptr;     // one row of 8-byte words per workgroup
    size_t rows = 0;                          // rows allocated
};

// the block exists and is zero at first use; the rows hold nblocks workgroups (grown by half and 64 behind a synchronisation)
inline int srl_wg_totals_reserve(srl_ctx *ctx, SrlWgTotals &t, size_t tot_words, size_t row_words, unsigned nblocks) {
    if (!t.d_tot) {
        HIPCHK(ctx, hipMalloc((void **)&t.d_tot, tot_words * sizeof(unsigned long long)));
        HIPCHK(ctx, hipMemsetAsync(t.d_tot, 0, tot_words * sizeof(unsigned long long), ctx->stream));
    }
    if (nblocks > t.rows) {
        if (t.d_rows) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(t.d_rows)); t.d_rows = nullptr; t.rows = 0; }
        const size_t rows = (size_t)nblocks + nblocks / 2 + 64;
        HIPCHK(ctx, hipMalloc((void **)&t.d_rows, rows * row_words * sizeof(unsigned long long)));
        t.rows = rows;
    }
    return SRL_OK;
}
inline void srl_wg_totals_free(SrlWgTotals &t) {
    if (t.d_tot) hipFree(t.d_tot);
    if (t.d_rows) hipFree(t.d_rows);
    t = SrlWgTotals();
}

#if defined(__HIPCC__)
// the sum of v over the wave, in every lane
template <class T>
__device__ __forceinline__ T srl_wave_sum(T v) {
    for (int dlt = 32; dlt >= 1; dlt >>= 1) v += __shfl_xor(v, dlt);
    return v;
}

// called once by every thread of a BLOCK-thread workgroup, as the kernel's last statement.  rows: gridDim.x rows of N words
template <int N, int BLOCK>
__device__ __forceinline__ void srl_wg_totals(const unsigned (&c)[N], unsigned long long *rows, unsigned long long *tot) {
    static_assert(BLOCK % 64 == 0, "whole waves");
    __shared__ unsigned s_part[BLOCK / 64][N];
    __shared__ int s_last;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const unsigned v = srl_wave_sum(c[k]);
        if (lane == 0) s_part[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) {
            unsigned r = 0;
            for (int w = 0; w < BLOCK / 64; w++) r += s_part[w][k];
            __hip_atomic_store(&rows[(size_t)blockIdx.x * N + k], (unsigned long long)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __threadfence();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = atomicAdd(&tot[N], 1ull) == (unsigned long long)gridDim.x - 1ull ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    if (wv != 0) return;
    unsigned long long sum[N];
#pragma unroll
    for (int k = 0; k < N; k++) sum[k] = 0;
    for (unsigned b = lane; b < gridDim.x; b += 64) {
#pragma unroll
        for (int k = 0; k < N; k++) sum[k] += __hip_atomic_load(&rows[(size_t)b * N + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int k = 0; k < N; k++) sum[k] = srl_wave_sum(sum[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) tot[k] = sum[k];
        tot[N] = 0ull;
    }
}
#endif

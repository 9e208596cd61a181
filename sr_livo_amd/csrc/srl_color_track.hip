// srl_color_track.hip -- the colour voxel map's consumer that keeps the camera tracker's point set on the device for gfx950:
// opticalFlowTracker::updateAndAppendTrackPoints (src/opticalFlowTracker.cpp:13-102).  The first loop (:22-61) re-projects every tracked
// point (project3dPointInThisImage, shared with the render: srl_color_project.h), ages or drops it and lets the kept ones inside the
// field of view occupy their coarse image cell; the second (:63-99) walks the candidates of refreshPointsForProjection in order and tops
// the set up to maximum_tracked_points through the same occupancy mask, with a `break` behind every candidate it looks at.
//
// The first loop is order free: what a point becomes depends on the point alone, and the set of occupied cells is a union.  The second
// is a function of ranks.  With T the kept points, a candidate is PROCESSED iff its pool position is known, not in T and not met
// earlier in the list; a processed candidate is a WINNER iff it projects inside the field of view, no point of T occupies its cell and
// no processed candidate with a smaller index and an inside projection has the same cell (whoever comes first inserts the cell, and the
// mask never forgets).  The size of the set is tested behind every processed candidate and changes only on an add: with s0 = |T| below
// the maximum the adds are the first (maximum - s0) winners; otherwise the test already holds behind the first processed candidate,
// which is added iff it is a winner.  Everything behind the break is `not reached` -- a winner there is `cut`.  DESIGN.md section 4.5.
//
//   k_track_file    one thread per tracked point and per candidate: the pool position is found or claimed in an epoch-tagged table that
//                   is never cleared (srl_frame_scratch.h), tracked points and candidates under keys of their own, and the smallest
//                   input index of the key lowered: the first occurrence, which is what detects duplicates and repeats
//   k_track_old     one thread per tracked point: projection, error, flag, outcome; a kept point inside the field of view claims its
//                   cell with the value 0, which beats every candidate.  Six counters leave through srl_wg_totals
//   k_track_cand    one thread per candidate: unknown / in T / repeated, else the projection and the cell, lowered to 1 + index; the
//                   smallest processed index (the break of a set that is already full) is lowered once per wave
//   srl_scan        over the tracked points: the kept ones in input order, flags updated
//   srl_scan        over the candidates: the rank among the winners decides added / cut / not reached and the record's place
//   k_track_count   the candidates' final outcomes through srl_wg_totals
// The companion words are {0xFFFFFFFF - call counter, value} and only ever lowered, as the selection's are: nothing is reset per call.
#include "srl_ctx.h"
#include "srl_color_map.h"
#include "srl_color_project.h"
#include "srl_frame_scratch.h"
#include "srl_hash.h"

#include <algorithm>
#include <cmath>
#include <cstring>

static_assert(sizeof(srl_color_track_point) == 16, "srl_color_track_point is 16 bytes on both sides of the C-ABI");
static_assert(sizeof(srl_color_track_opts) == 16, "srl_color_track_opts is 16 bytes on both sides of the C-ABI");
static_assert(sizeof(srl_color_track_totals) == 14 * 8, "srl_color_track_totals is fourteen int64");

namespace {

#define SRL_TRK_NONE 0xFFFFFFFFu
enum { TRK_OLD_N = SRL_TRACK_DUPLICATE + 1, TRK_CAND_N = SRL_TRACK_CAND_NOT_REACHED + 1 };
enum { TRK_CAND_INSIDE = 0xFF };           // k_track_cand's word for "processed, inside the field of view, cell filed": the scan decides
enum { CNT_KEPT, CNT_ADDED, CNT_FIRST };   // the call's three device words

struct TrackArgs {
    SrlCamArgs C;
    double mini_distance, max_err;
    long long base_u, base_v, span_v;      // cell = (u - base_u) * span_v + (v - base_v), as the selection forms it
};

// slot of `key` in an epoch table whose entries of this epoch are complete (filed by an earlier kernel), or SRL_TRK_NONE
__device__ __forceinline__ unsigned track_find(const unsigned long long *keyw, unsigned mask, unsigned epoch16, unsigned long long key, unsigned hash) {
    const unsigned long long want = ((unsigned long long)epoch16 << 48) | key;
    unsigned h = hash & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        const unsigned long long k = keyw[h];
        if (k == want) return h;
        if ((unsigned)(k >> 48) != epoch16) return SRL_TRK_NONE;
        h = (h + 1) & mask;
    }
    return SRL_TRK_NONE;
}
__device__ __forceinline__ unsigned long long track_pool_key(int pool, unsigned candidate) { return ((unsigned long long)(unsigned)pool << 1) | candidate; }
// u_i = std::round(u_d / mini_distance) * mini_distance into an int (:29-30, :79-80): the selection's statements
__device__ __forceinline__ unsigned long long track_cell(const TrackArgs &A, double u_d, double v_d) {
    const int u = (int)(round(u_d / A.mini_distance) * A.mini_distance), v = (int)(round(v_d / A.mini_distance) * A.mini_distance);
    return ((unsigned long long)((long long)u - A.base_u) * (unsigned long long)A.span_v + (unsigned long long)((long long)v - A.base_v)) & SRL_KEY48_MASK;
}
__device__ __forceinline__ void track_lower(unsigned long long *w, unsigned tag, unsigned value) {
    const unsigned long long want = ((unsigned long long)tag << 32) | (unsigned long long)value;
    if (*w > want) atomicMin(w, want);     // a plain read: an older value is a larger one, never a missed update
}

__global__ void __launch_bounds__(256) k_track_file(const srl_color_track_point *tracked, int n, const int *cand, int nc, long long P, unsigned long long *keyw,
                                                    unsigned long long *minw, unsigned mask, unsigned epoch16, unsigned tag, unsigned *slot_t, unsigned *slot_c,
                                                    unsigned *cnt) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j == 0) { cnt[CNT_KEPT] = 0u; cnt[CNT_ADDED] = 0u; cnt[CNT_FIRST] = SRL_TRK_NONE; }
    if (j >= (long long)n + nc) return;
    const bool is_cand = j >= n;
    const unsigned idx = (unsigned)(is_cand ? j - n : j);
    const int pool = is_cand ? cand[idx] : tracked[idx].pool;
    unsigned slot = SRL_TRK_NONE;
    if (pool >= 0 && (long long)pool < P) {
        const unsigned long long key = track_pool_key(pool, is_cand ? 1u : 0u);
        slot = srl_epoch_claim(keyw, mask, epoch16, key, srl_hash_key(key));
        track_lower(&minw[slot], tag, idx);
    }
    (is_cand ? slot_c : slot_t)[idx] = slot;
}

__global__ void __launch_bounds__(256) k_track_old(const srl_color_track_point *tracked, int n, const SrlColorPoint *pool, TrackArgs A, const unsigned *slot_t,
                                                   const unsigned long long *pool_minw, unsigned long long *cell_keyw, unsigned long long *cell_minw,
                                                   unsigned cell_mask, unsigned cell_epoch16, unsigned cell_tag, unsigned char *outcome_out,
                                                   unsigned long long *spart, unsigned long long *stot) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned c[TRK_OLD_N] = {0, 0, 0, 0, 0, 0};
    if (i < n) {
        const srl_color_track_point t = tracked[i];
        const unsigned slot = slot_t[i];
        int outcome;
        if (slot == SRL_TRK_NONE) {
            outcome = SRL_TRACK_UNKNOWN;
        } else if ((unsigned)pool_minw[slot] != (unsigned)i) {
            outcome = SRL_TRACK_DUPLICATE;
        } else {
            const SrlColorPoint pt = pool[t.pool];
            double u_d, v_d;
            const int proj = srl_color_project(A.C, (double)pt.x, (double)pt.y, (double)pt.z, &u_d, &v_d);      // getPosition(): position.cast<double>()
            if (proj == SRL_PROJ_BEHIND) {
                outcome = SRL_TRACK_BEHIND;                      // the reference leaves u_d, v_d unwritten here: a stated departure
            } else {
                const double du = u_d - (double)t.u, dv = v_d - (double)t.v;
                const double error = sqrt(du * du + dv * dv);   // Eigen::Vector2d(...).norm()
                if (error > A.max_err) {
                    // is_out_lier_count++; erased if (count > 1) || (error > max_err * 2)
                    outcome = (t.flagged >= 1 || error > A.max_err * 2) ? SRL_TRACK_DROPPED : SRL_TRACK_KEPT_FLAGGED;
                } else {
                    outcome = SRL_TRACK_KEPT;
                }
                if (outcome != SRL_TRACK_DROPPED && proj == SRL_PROJ_OK) {
                    const unsigned long long cell = track_cell(A, u_d, v_d);
                    const unsigned cs = srl_epoch_claim(cell_keyw, cell_mask, cell_epoch16, cell, srl_hash_key(cell));
                    track_lower(&cell_minw[cs], cell_tag, 0u);
                }
            }
        }
        outcome_out[i] = (unsigned char)outcome;
#pragma unroll
        for (int k = 0; k < TRK_OLD_N; k++) c[k] = outcome == k ? 1u : 0u;      // (an index that is no constant would put the array into scratch)
    }
    srl_wg_totals<TRK_OLD_N, 256>(c, spart, stot);
}

__global__ void __launch_bounds__(256) k_track_cand(const int *cand, int nc, const SrlColorPoint *pool, TrackArgs A, const unsigned *slot_c,
                                                    const unsigned long long *pool_keyw, const unsigned long long *pool_minw, unsigned pool_mask,
                                                    unsigned pool_epoch16, unsigned pool_tag, const unsigned char *tracked_outcome,
                                                    unsigned long long *cell_keyw, unsigned long long *cell_minw, unsigned cell_mask, unsigned cell_epoch16,
                                                    unsigned cell_tag, unsigned char *natural, unsigned *cell_slot, float *uv_out, unsigned *cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned first = SRL_TRK_NONE;
    if (i < nc) {
        const unsigned slot = slot_c[i];
        int state;
        if (slot == SRL_TRK_NONE) {
            state = SRL_TRACK_CAND_UNKNOWN;
        } else {
            const int p = cand[i];
            bool in_T = false;
            const unsigned long long tkey = track_pool_key(p, 0u);
            const unsigned ts = track_find(pool_keyw, pool_mask, pool_epoch16, tkey, srl_hash_key(tkey));
            if (ts != SRL_TRK_NONE) {
                const unsigned long long w = pool_minw[ts];
                if ((unsigned)(w >> 32) == pool_tag) {
                    const unsigned char o = tracked_outcome[(unsigned)w];      // of the first occurrence: the later ones are duplicates
                    in_T = o == SRL_TRACK_KEPT || o == SRL_TRACK_KEPT_FLAGGED;
                }
            }
            if (in_T || (unsigned)pool_minw[slot] != (unsigned)i) {
                state = SRL_TRACK_CAND_ALREADY_TRACKED;          // found in the map (:69-73), or a repeat: it behaves as its first occurrence did
            } else {
                first = (unsigned)i;
                const SrlColorPoint pt = pool[p];
                double u_d, v_d;
                if (srl_color_project(A.C, (double)pt.x, (double)pt.y, (double)pt.z, &u_d, &v_d) != SRL_PROJ_OK) {
                    state = SRL_TRACK_CAND_REFUSED;
                } else {
                    const unsigned long long cell = track_cell(A, u_d, v_d);
                    const unsigned cs = srl_epoch_claim(cell_keyw, cell_mask, cell_epoch16, cell, srl_hash_key(cell));
                    track_lower(&cell_minw[cs], cell_tag, 1u + (unsigned)i);
                    cell_slot[i] = cs;
                    uv_out[(size_t)i * 2] = (float)u_d; uv_out[(size_t)i * 2 + 1] = (float)v_d;      // cv::Point2f(u_d, v_d)
                    state = TRK_CAND_INSIDE;
                }
            }
        }
        natural[i] = (unsigned char)state;
    }
    for (int d = 32; d >= 1; d >>= 1) first = min(first, __shfl_xor(first, d));
    if ((threadIdx.x & 63) == 0 && first != SRL_TRK_NONE && cnt[CNT_FIRST] > first) atomicMin(&cnt[CNT_FIRST], first);
}

struct TrackKeptIn {
    const unsigned char *outcome;
    __device__ int operator()(int i) const { return outcome[i] <= SRL_TRACK_KEPT_FLAGGED ? 1 : 0; }
};
struct TrackKeptSink {
    const srl_color_track_point *tracked;
    const unsigned char *outcome;
    srl_color_track_point *out;
    unsigned *cnt;
    int n;
    __device__ void operator()(int i, int kept, int excl) const {
        if (kept) {
            srl_color_track_point t = tracked[i];
            t.flagged = outcome[i] == SRL_TRACK_KEPT_FLAGGED ? t.flagged + 1 : 0;
            out[excl] = t;
        }
        if (i == n - 1) cnt[CNT_KEPT] = (unsigned)(excl + kept);
    }
};
struct TrackWinnerIn {
    const unsigned char *natural;
    const unsigned *cell_slot;
    const unsigned long long *cell_minw;
    unsigned cell_tag;
    __device__ int operator()(int i) const {
        if (natural[i] != TRK_CAND_INSIDE) return 0;
        return cell_minw[cell_slot[i]] == (((unsigned long long)cell_tag << 32) | (unsigned long long)(1u + (unsigned)i)) ? 1 : 0;
    }
};
struct TrackAddSink {
    const int *cand;
    const unsigned char *natural;
    const float *uv;
    srl_color_track_point *out;
    unsigned char *final_outcome;
    unsigned *cnt;
    long long out_cap, maximum;
    int nc;
    __device__ void operator()(int i, int winner, int excl) const {
        const long long s0 = (long long)cnt[CNT_KEPT];
        const bool room = s0 < maximum;
        // behind the break: the budget's last winner lies in front of i, or (a full set) the first processed candidate does
        const bool behind = room ? (long long)excl >= maximum - s0 : (cnt[CNT_FIRST] != SRL_TRK_NONE && (unsigned)i > cnt[CNT_FIRST]);
        const unsigned char nat = natural[i];
        int o;
        if (behind) o = winner ? SRL_TRACK_CAND_CUT : SRL_TRACK_CAND_NOT_REACHED;
        else if (winner) o = SRL_TRACK_CAND_ADDED;
        else o = nat == TRK_CAND_INSIDE ? SRL_TRACK_CAND_OCCUPIED : (int)nat;
        if (o == SRL_TRACK_CAND_ADDED) {
            const long long pos = room ? s0 + excl : s0;
            if (pos < out_cap) {
                srl_color_track_point t;
                t.pool = cand[i]; t.u = uv[(size_t)i * 2]; t.v = uv[(size_t)i * 2 + 1]; t.flagged = 0;
                out[pos] = t;
            }
            if (!room) cnt[CNT_ADDED] = 1u;
        }
        if (room && i == nc - 1) cnt[CNT_ADDED] = (unsigned)min((long long)(excl + winner), maximum - s0);
        final_outcome[i] = (unsigned char)o;
    }
};

__global__ void __launch_bounds__(256) k_track_count(const unsigned char *final_outcome, int nc, unsigned long long *spart, unsigned long long *stot) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned c[TRK_CAND_N] = {0, 0, 0, 0, 0, 0, 0};
    if (i < nc) {
        const int o = final_outcome[i];
#pragma unroll
        for (int k = 0; k < TRK_CAND_N; k++) c[k] = o == k ? 1u : 0u;
    }
    srl_wg_totals<TRK_CAND_N, 256>(c, spart, stot);
}

unsigned track_pow2(unsigned long long v) { unsigned p = 1024; while (p < v && p < 0x80000000u) p <<= 1; return p; }

}  // namespace

void srl_color_track_free(SrlColorMap *cm) {
    srl_epoch_table_free(cm->trk_pool);
    srl_epoch_table_free(cm->trk_cells);
}

extern "C" void srl_color_track_opts_default(srl_color_track_opts *o) {
    if (!o) return;
    o->mini_distance = 10.0;               // the tracker's call: imageProcessing.cpp:161
    o->maximum_tracked_points = 300;       // opticalFlowTracker.cpp:10
    o->reserved = 0;
}

extern "C" int srl_color_map_track_update(srl_ctx *ctx, const srl_color_camera *cam, int image_rows, int image_cols, const srl_color_track_point *tracked, int n,
                                          const int32_t *candidates, int n_candidates, const srl_color_track_opts *opts, srl_color_track_point *out,
                                          int64_t capacity, uint8_t *tracked_outcome, uint8_t *candidate_outcome, srl_color_track_totals *totals) {
    if (totals) std::memset(totals, 0, sizeof *totals);
    if (!ctx || !cam || !opts || n < 0 || n_candidates < 0 || (n > 0 && !tracked) || (n_candidates > 0 && !candidates) || capacity < 0) return SRL_ERR_BAD_ARG;
    if (n > SRL_COLOR_TRACK_MAX_POINTS || n_candidates > SRL_COLOR_TRACK_MAX_CANDIDATES) {
        ctx->err = "track update: n <= SRL_COLOR_TRACK_MAX_POINTS, n_candidates <= SRL_COLOR_TRACK_MAX_CANDIDATES";
        return SRL_ERR_BAD_ARG;
    }
    if (!std::isfinite(opts->mini_distance) || !(opts->mini_distance > 0.0) || opts->mini_distance > 65536.0) {
        ctx->err = "track update: mini_distance finite in (0, 65536]";
        return SRL_ERR_BAD_ARG;
    }
    if (image_rows < 2 || image_cols < 2 || (int64_t)image_rows * image_cols > SRL_COLOR_IMAGE_MAX_PIXELS) { ctx->err = "track update: image size"; return SRL_ERR_BAD_ARG; }
    if (!srl_color_cam_finite(cam)) { ctx->err = "track update: camera must be finite"; return SRL_ERR_BAD_ARG; }
    if (!(cam->fov_margin >= -4.0 && cam->fov_margin < 0.5)) { ctx->err = "track update: fov_margin must lie in [-4, 0.5)"; return SRL_ERR_BAD_ARG; }
    TrackArgs A;
    if (!srl_color_cam_args(cam, image_rows, image_cols, &A.C)) { ctx->err = "track update: camera pose is not finite"; return SRL_ERR_BAD_ARG; }
    { const int rc = srl_color_need_map_one_rank(ctx); if (rc) return rc; }
    SrlColorMap *cm = ctx->color;
    SRL_DISARM(ctx);                      // a waiting launch holds a workgroup on every compute unit
    if (totals) { totals->tracked_in = n; totals->candidates = n_candidates; }
    if (n == 0 && n_candidates == 0) return SRL_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;

    // the cells: keys lie within mini_distance / 2 (and a rounding) of the accepted u, v -- the selection's bounds
    const double md = opts->mini_distance;
    const long long maximum = opts->maximum_tracked_points;
    A.mini_distance = md;
    A.max_err = 2.0 * image_cols / 320.0;                  // :18
    const long long top_u = (long long)std::ceil(A.C.u_hi + md / 2) + 2, top_v = (long long)std::ceil(A.C.v_hi + md / 2) + 2;
    A.base_u = (long long)std::floor(A.C.u_lo - md / 2) - 2; A.base_v = (long long)std::floor(A.C.v_lo - md / 2) - 2;
    const long long span_u = std::max<long long>(top_u - A.base_u + 1, 1);
    A.span_v = std::max<long long>(top_v - A.base_v + 1, 1);
    const double quot_u = std::max(std::floor((A.C.u_hi - A.C.u_lo) / md), 0.0) + 3.0, quot_v = std::max(std::floor((A.C.v_hi - A.C.v_lo) / md), 0.0) + 3.0;
    const double cells_d = std::min((double)span_u, quot_u) * std::min((double)A.span_v, quot_v);      // distinct keys the accepted points can form
    const long long items = (long long)n + n_candidates;
    const unsigned long long cells_hi = cells_d < (double)items ? (unsigned long long)cells_d : (unsigned long long)items;
    const unsigned cell_cap = track_pow2(2ull * cells_hi), pool_cap = track_pow2(2ull * (unsigned long long)items);
    const long long add_cap = std::min<long long>(n_candidates, std::max<long long>(maximum, 1));     // adds of one call
    const long long out_cap = n + add_cap;

    const unsigned blocks_all = (unsigned)((items + 255) / 256), blocks_old = (unsigned)((n + 255) / 256), blocks_cand = (unsigned)((n_candidates + 255) / 256);
    if (n) { const int rc = srl_wg_totals_reserve(ctx, cm->track_old_tot, TRK_OLD_N + 1, TRK_OLD_N, blocks_old); if (rc) return rc; }
    if (n_candidates) { const int rc = srl_wg_totals_reserve(ctx, cm->track_cand_tot, TRK_CAND_N + 1, TRK_CAND_N, blocks_cand); if (rc) return rc; }
    { const int rc = srl_epoch_table_begin(ctx, cm->trk_pool, pool_cap, true); if (rc) return rc; }
    { const int rc = srl_epoch_table_begin(ctx, cm->trk_cells, cell_cap, true); if (rc) return rc; }
    const unsigned pool_tag = 0xFFFFFFFFu - cm->trk_pool.counter32, cell_tag = 0xFFFFFFFFu - cm->trk_cells.counter32;

    // page-locked scratch: [0, 64) the first loop's totals, [64, 128) the second's, [128, 192) the three words, then the lists going up
    // and later the outcomes coming down; the records come down over all of it once the outcomes have left
    const size_t in_bytes = (size_t)n * sizeof(srl_color_track_point) + (size_t)n_candidates * 4;
    const size_t h_need = std::max<size_t>(192 + std::max<size_t>(in_bytes, (size_t)items), (size_t)out_cap * sizeof(srl_color_track_point));
    { const int rc = ensure_host_scratch(ctx, h_need); if (rc) return rc; }

    DevBuf b_in, b_slot_t, b_slot_c, b_tout, b_nat, b_cslot, b_uv, b_cout, b_out, b_cnt, b_sc;
    HIPCHK(ctx, b_in.alloc(ctx, in_bytes));
    HIPCHK(ctx, b_slot_t.alloc(ctx, (size_t)n * 4));
    HIPCHK(ctx, b_slot_c.alloc(ctx, (size_t)n_candidates * 4));
    HIPCHK(ctx, b_tout.alloc(ctx, (size_t)n));
    HIPCHK(ctx, b_nat.alloc(ctx, (size_t)n_candidates));
    HIPCHK(ctx, b_cslot.alloc(ctx, (size_t)n_candidates * 4));
    HIPCHK(ctx, b_uv.alloc(ctx, (size_t)n_candidates * 8));
    HIPCHK(ctx, b_cout.alloc(ctx, (size_t)n_candidates));
    HIPCHK(ctx, b_out.alloc(ctx, (size_t)out_cap * sizeof(srl_color_track_point)));
    HIPCHK(ctx, b_cnt.alloc(ctx, 64));
    HIPCHK(ctx, b_sc.alloc(ctx, srl_scan_scratch_ints(std::max(n, n_candidates)) * 4));
    if (n) std::memcpy(ctx->h_scratch + 192, tracked, (size_t)n * sizeof(srl_color_track_point));
    if (n_candidates) std::memcpy(ctx->h_scratch + 192 + (size_t)n * sizeof(srl_color_track_point), candidates, (size_t)n_candidates * 4);
    HIPCHK(ctx, hipMemcpyAsync(b_in.p, ctx->h_scratch + 192, in_bytes, hipMemcpyHostToDevice, st));
    const srl_color_track_point *d_tracked = b_in.as<srl_color_track_point>();
    const int *d_cand = reinterpret_cast<const int *>(b_in.as<unsigned char>() + (size_t)n * sizeof(srl_color_track_point));
    unsigned *cnt = b_cnt.as<unsigned>();

    hipLaunchKernelGGL(k_track_file, dim3(blocks_all), dim3(256), 0, st, d_tracked, n, d_cand, n_candidates, cm->num_points, cm->trk_pool.keyw, cm->trk_pool.minw,
                       pool_cap - 1, cm->trk_pool.epoch16, pool_tag, b_slot_t.as<unsigned>(), b_slot_c.as<unsigned>(), cnt);
    HIPCHK(ctx, hipGetLastError());
    if (n) {
        hipLaunchKernelGGL(k_track_old, dim3(blocks_old), dim3(256), 0, st, d_tracked, n, cm->d_pool, A, b_slot_t.as<unsigned>(), cm->trk_pool.minw,
                           cm->trk_cells.keyw, cm->trk_cells.minw, cell_cap - 1, cm->trk_cells.epoch16, cell_tag, b_tout.as<unsigned char>(),
                           cm->track_old_tot.d_rows, cm->track_old_tot.d_tot);
        HIPCHK(ctx, hipGetLastError());
        srl_scan(TrackKeptIn{b_tout.as<unsigned char>()}, TrackKeptSink{d_tracked, b_tout.as<unsigned char>(), b_out.as<srl_color_track_point>(), cnt, n}, n,
                 b_sc.as<int>(), st);
        HIPCHK(ctx, hipGetLastError());
    }
    if (n_candidates) {
        hipLaunchKernelGGL(k_track_cand, dim3(blocks_cand), dim3(256), 0, st, d_cand, n_candidates, cm->d_pool, A, b_slot_c.as<unsigned>(), cm->trk_pool.keyw,
                           cm->trk_pool.minw, pool_cap - 1, cm->trk_pool.epoch16, pool_tag, b_tout.as<unsigned char>(), cm->trk_cells.keyw, cm->trk_cells.minw,
                           cell_cap - 1, cm->trk_cells.epoch16, cell_tag, b_nat.as<unsigned char>(), b_cslot.as<unsigned>(), b_uv.as<float>(), cnt);
        HIPCHK(ctx, hipGetLastError());
        srl_scan(TrackWinnerIn{b_nat.as<unsigned char>(), b_cslot.as<unsigned>(), cm->trk_cells.minw, cell_tag},
                 TrackAddSink{d_cand, b_nat.as<unsigned char>(), b_uv.as<float>(), b_out.as<srl_color_track_point>(), b_cout.as<unsigned char>(), cnt, out_cap,
                              maximum, n_candidates},
                 n_candidates, b_sc.as<int>(), st);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_track_count, dim3(blocks_cand), dim3(256), 0, st, b_cout.as<unsigned char>(), n_candidates, cm->track_cand_tot.d_rows,
                           cm->track_cand_tot.d_tot);
        HIPCHK(ctx, hipGetLastError());
    }

    // one wait for the totals (and the outcome bytes, whose number is known), then one DMA of exactly kept + added records
    char *h = ctx->h_scratch;
    if (n) HIPCHK(ctx, hipMemcpyAsync(h, cm->track_old_tot.d_tot, TRK_OLD_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (n_candidates) HIPCHK(ctx, hipMemcpyAsync(h + 64, cm->track_cand_tot.d_tot, TRK_CAND_N * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(h + 128, cnt, 3 * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    if (n && tracked_outcome) HIPCHK(ctx, hipMemcpyAsync(h + 192, b_tout.p, (size_t)n, hipMemcpyDeviceToHost, st));
    if (n_candidates && candidate_outcome) HIPCHK(ctx, hipMemcpyAsync(h + 192 + n, b_cout.p, (size_t)n_candidates, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    unsigned long long t_old[TRK_OLD_N] = {0, 0, 0, 0, 0, 0}, t_cand[TRK_CAND_N] = {0, 0, 0, 0, 0, 0, 0};
    unsigned h_cnt[3];
    if (n) std::memcpy(t_old, h, sizeof t_old);
    if (n_candidates) std::memcpy(t_cand, h + 64, sizeof t_cand);
    std::memcpy(h_cnt, h + 128, sizeof h_cnt);
    const int64_t kept = (int64_t)(t_old[SRL_TRACK_KEPT] + t_old[SRL_TRACK_KEPT_FLAGGED]), added = (int64_t)t_cand[SRL_TRACK_CAND_ADDED];
    if (totals) {
        totals->kept = kept; totals->flagged = (int64_t)t_old[SRL_TRACK_KEPT_FLAGGED]; totals->dropped = (int64_t)t_old[SRL_TRACK_DROPPED];
        totals->behind = (int64_t)t_old[SRL_TRACK_BEHIND]; totals->unknown = (int64_t)t_old[SRL_TRACK_UNKNOWN];
        totals->duplicate = (int64_t)t_old[SRL_TRACK_DUPLICATE];
        totals->already_tracked = (int64_t)t_cand[SRL_TRACK_CAND_ALREADY_TRACKED]; totals->cand_unknown = (int64_t)t_cand[SRL_TRACK_CAND_UNKNOWN];
        totals->refused = (int64_t)t_cand[SRL_TRACK_CAND_REFUSED]; totals->occupied = (int64_t)t_cand[SRL_TRACK_CAND_OCCUPIED];
        totals->added = added; totals->cut = (int64_t)t_cand[SRL_TRACK_CAND_CUT];
    }
    if (kept != (int64_t)h_cnt[CNT_KEPT] || added != (int64_t)h_cnt[CNT_ADDED] || kept + added > out_cap) {
        ctx->err = "track update: the scans and the counters disagree (internal)";
        return SRL_ERR_HIP;
    }
    const int64_t records = kept + added;
    if (out && capacity < records) { ctx->err = "track update: capacity below kept + added (totals)"; return SRL_ERR_BAD_ARG; }
    if (n && tracked_outcome) std::memcpy(tracked_outcome, h + 192, (size_t)n);
    if (n_candidates && candidate_outcome) std::memcpy(candidate_outcome, h + 192 + n, (size_t)n_candidates);
    if (!out || records == 0) return SRL_OK;
    const size_t bytes = (size_t)records * sizeof(srl_color_track_point);
    HIPCHK(ctx, hipMemcpyAsync(h, b_out.p, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    std::memcpy(out, h, bytes);
    return SRL_OK;
}

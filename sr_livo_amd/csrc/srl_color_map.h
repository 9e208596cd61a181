// srl_color_map.h -- internal: the colour voxel map's device layout, shared by its construction (srl_color_kernels.hip) and its
// consumers, the rendering pass (srl_color_render.hip), the selection for projection (srl_color_select.hip), the camera ESIKF's
// measurement passes (srl_color_vio.hip), the cloud export (srl_color_cloud.hip) and the tracker's point set (srl_color_track.hip).  DESIGN.md section 3.
// The inline host helpers at its end call the HIP runtime (HIPCHK, DevBuf): the runtime's headers come in through srl_ctx.h.
#pragma once
#include "srl_ctx.h"
#include "srl_wg_totals.h"

#include <cstring>

struct SrlColorVoxel { unsigned long long key; double last_visited_time; unsigned count; unsigned pad; };
struct SrlColorPoint { float x, y, z; int voxel; int slot; int reg; };
struct SrlColorSlot { unsigned long long key; unsigned voxel; unsigned pad; };
struct SrlGridCell { unsigned long long key; unsigned born; unsigned owner; };     // born: number of the batch that created the cell
// what rgbPoint::updateRgb reads and writes (include/cloudMap.h:51-66), one record per pool point in an array PARALLEL to the pool;
// all-zero bytes = rgbPoint::reset() (cloudMap.cpp:11-19)
struct SrlColorState { double observe_distance; double last_observe_time; float cov_rgb[3]; short rgb[3]; short n_rgb; };
static_assert(sizeof(SrlColorState) == 40, "DESIGN.md section 3: 40 bytes of colour state per stored point (36 + padding)");

struct SrlColorMap {
    srl_color_opts opts;
    SrlColorVoxel *d_vox = nullptr;    unsigned vox_cap = 0;      // voxel records in creation order
    SrlColorSlot *d_vtab = nullptr;    unsigned vtab_cap = 0;     // voxel key -> voxel (power of two, >= 2 vox_cap)
    SrlColorPoint *d_pool = nullptr;   size_t pool_cap = 0;       // stored points, append-only, in insertion order
    int *d_reg = nullptr;              size_t reg_cap = 0;        // registered list: pool position per point_index
    SrlGridCell *d_grid = nullptr;     unsigned grid_cap = 0;     // grid set (power of two, >= 2 reg_cap)
    int num_voxels = 0;
    long long num_points = 0, num_registered = 0;
    unsigned batch_seq = 0;
    int vtab_rebuilds = 0, grid_rebuilds = 0;
    SrlEpochTable scratch;

    // rendering (srl_color_render.hip); nothing of it exists before the first srl_color_image_upload
    bool render_on = false;
    SrlColorState *d_state = nullptr;  size_t state_cap = 0;      // parallel to d_pool; entries >= num_points are zero
    unsigned *d_mark = nullptr;        unsigned mark_cap = 0;     // per voxel: (render epoch << 16) | occurrences in the list of that render
    unsigned render_epoch = 0;                                    // 1 ... 65535 (0: the value of a word nobody has marked)
    SrlImagePair img;                                             // rows x cols x 3 bytes, rows packed, and the upload's page-locked staging
    int img_rows = 0, img_cols = 0;                               // 0: no image uploaded
    hipEvent_t img_ev = nullptr;       bool img_pending = false;  // the DMA out of img.h
    SrlWgTotals render_tot;                                       // k_render_points: [0..5] totals of the last render, [6] the ticket, [7] unknown keys
                                                                  // and [8] overflowing marks (both since allocation: never reset)
    unsigned long long unknown_seen = 0, overflow_seen = 0;       // host copies of [7] and [8] as of the previous render

    // selection for projection (srl_color_select.hip); nothing of it exists before the first srl_color_map_select
    int *d_tail = nullptr;             unsigned tail_cap = 0;     // per voxel: pool position of its last point (slot == count - 1)
    long long tail_swept = 0;                                     // pool positions [0, tail_swept) have been swept into d_tail
    SrlEpochTable sel_cells;                                      // image cell -> slot; minw = {~call counter, float bits of the cell's smallest depth}
    unsigned long long *d_sel_last = nullptr;                     // per slot {~call counter, ~(last index whose depth lies below the float minimum)}
    unsigned long long *d_sel_first = nullptr;                    // per slot {~call counter, first index whose depth rounds to the float minimum}
    unsigned sel_words_cap = 0;
    SrlWgTotals select_tot;                                       // k_select_cells: [0..3] far, near, behind, outside of the last selection, [4] the ticket

    // camera ESIKF measurement passes (srl_color_vio.hip); nothing of it exists before the first srl_color_map_vio_rows
    SrlWgTotals vio_tot;                                          // k_vio_rows, rows of 88 words (78 sums as FP64 bits, 5 counts): [0..87] the row of the
                                                                  // last call, [88] the ticket

    // the tracker's point set (srl_color_track.hip); nothing of it exists before the first srl_color_map_track_update
    SrlEpochTable trk_pool;                                       // (pool position << 1 | candidate) -> slot; minw = {~call counter, smallest input index}
    SrlEpochTable trk_cells;                                      // image cell -> slot; minw = {~call counter, 0 for a kept point, else 1 + smallest candidate index}
    SrlWgTotals track_old_tot;                                    // k_track_old: [0..5] the first loop's outcomes of the last call, [6] the ticket
    SrlWgTotals track_cand_tot;                                   // k_track_count: [0..6] the second loop's outcomes of the last call, [7] the ticket

    // cloud export (srl_color_cloud.hip); nothing of it exists before the first srl_color_map_export_cloud
    SrlWgTotals cloud_tot;                                        // k_cloud_flags: [0..1] below the views, stale, [2] the ticket, [4] an int: published
};

// the refusals every entry point of the map's consumers makes: no map, more than one rank
inline int srl_color_need_map(srl_ctx *ctx) {
    if (!ctx->color) { ctx->err = "no colour map (srl_color_map_create)"; return SRL_ERR_NO_MAP; }
    return SRL_OK;
}
inline int srl_color_one_rank(srl_ctx *ctx) {
    if (ctx->nranks > 1) { ctx->err = "the colour map is neither replicated nor sharded: one rank only"; return SRL_ERR_UNSUPPORTED; }
    return SRL_OK;
}
inline int srl_color_need_map_one_rank(srl_ctx *ctx) {
    const int rc = srl_color_need_map(ctx);
    return rc ? rc : srl_color_one_rank(ctx);
}

// a caller's voxel list (n x 3 ints) into a block of the pool, through the page-locked scratch behind its first 128 bytes (where the
// call's totals land)
inline int srl_color_upload_list(srl_ctx *ctx, const int32_t *voxels_xyz, int n, DevBuf &b) {
    const size_t bytes = (size_t)n * 12;
    HIPCHK(ctx, b.alloc(ctx, bytes));
    { const int rc = ensure_host_scratch(ctx, bytes + 128); if (rc) return rc; }
    std::memcpy(ctx->h_scratch + 128, voxels_xyz, bytes);
    HIPCHK(ctx, hipMemcpyAsync(b.p, ctx->h_scratch + 128, bytes, hipMemcpyHostToDevice, ctx->stream));
    return SRL_OK;
}

#if defined(__HIPCC__)
#include "srl_hash.h"
// the voxel an entry (x, y, z) of a caller's list names, or -1 for a key the map does not hold (vmask = vtab_cap - 1)
__device__ __forceinline__ int srl_color_find_voxel(const SrlColorSlot *vtab, unsigned vmask, int x, int y, int z) {
    if (!(x >= -32768 && x <= 32767 && y >= -32768 && y <= 32767 && z >= -32768 && z <= 32767)) return -1;      // voxelId holds what a voxel's shorts held
    const unsigned long long key = srl_pack_key((short)x, (short)y, (short)z);
    unsigned h = srl_hash_key(key) & vmask;
    for (unsigned probe = 0; probe <= vmask; ++probe) {
        const unsigned long long k = vtab[h].key;
        if (k == key) return (int)vtab[h].voxel;
        if (k == SRL_EMPTY_KEY) return -1;
        h = (h + 1) & vmask;
    }
    return -1;
}
#endif

// the state array follows the pool (x1.5 by copy, zero-filled tail) once rendering is on; called behind every pool growth
int srl_color_state_reserve(srl_ctx *ctx, SrlColorMap *cm);
// frees what rendering allocated (srl_color_map_destroy)
void srl_color_render_free(SrlColorMap *cm);
// frees what the selection allocated (srl_color_map_destroy)
void srl_color_select_free(SrlColorMap *cm);
// frees what the tracker's update allocated (srl_color_map_destroy)
void srl_color_track_free(SrlColorMap *cm);

// srl_color_kernels.hip -- construction of the colour voxel map on the device for gfx950:
// lioOptimization::addPointToColorMap (src/lioOptimization.cpp:448-518) as called from addPointsToMap (:520-554) for every
// add_point_step-th frame point, with the grid hashmap_3d_points (include/utility.h:94-141), the ordered list rgb_points_vec
// (include/rgbMapTracker.h:40) and voxels_recent_visited_temp (include/lioOptimization.h:291).  voxelBlock: include/cloudMap.h:147-169.
//
// The reference inserts the points one by one.  Unlike addPointToMap there is no min-distance replay against residents: a point is
// stored iff its voxel is not full, so the whole rule is a function of ranks and needs no sequential thread per voxel:
//   1. k[j] = short(float(p) / size_voxel_map), g[j] = short(float(p) / min_distance_points) per axis (:453-459) for the participating
//      points j (batch index i = j * add_point_step, :538); the points of a voxel are brought together, in batch order, by the stable
//      radix sort over the slot the voxel claims in an epoch-tagged scratch table (srl_frame_scratch.h, as k_point_slots does)
//   2. scan over the head flags: segment starts; per segment the voxel is looked up and its count read; a segment without a voxel marks
//      its first point
//   3. scan over those marks in batch order: the exclusive prefix is the creation rank (the sequential loop creates voxels in the order
//      their first points arrive) -> voxel record V + rank, key CAS-inserted into the voxel table
//   4. per point: rank r in its segment; stored <=> r < cap - count_before (:470, IsFull), slot = count_before + r.  The segment's first
//      point applies the visited rule of :487-491 / :510-514 to the voxel's time and stamps it; every stored point CAS-inserts g into
//      the persistent grid set -- the thread whose compare-and-swap creates the cell tags it with this batch's number
//   5. per stored point whose cell carries this batch's number: atomicMin of the batch index into the cell's owner word
//   6. registered <=> the cell is of this batch and owner == own index (:476-483, :501-508: the EARLIEST stored point of a cell that
//      was absent; a point a full voxel refuses never claims its cell, a later stored one does)
//   7. three scans in batch order: stored -> position in the append-only point pool; registered -> point_index (and the pool records,
//      the report records and the outcome bytes are written in its pass); visited -> the list in order of first touch
// Every order comes from a batch index, nothing from arrival order: two runs give the same bits.
//
// Layout: bytes per voxel and per stored point do not depend on max_num_points_in_voxel -- the map holds ~1.1
// points per voxel at 0.1 m, a cap-sized slab per voxel as in the LiDAR map would be ~98 % padding.  Voxel record 24 B {key, time, count},
// point-pool record 24 B {xyz FP32, voxel, slot, registered index or -1}, registered list 4 B (pool position), and two open-addressing
// tables of 16-B slots kept at a load <= 0.5: voxel key -> voxel, grid key -> {batch tag, owner}.  Both tables grow by rebuild.
#include "srl_ctx.h"
#include "srl_color_map.h"
#include "srl_frame_scratch.h"
#include "srl_hash.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

static_assert(sizeof(SrlColorVoxel) == 24 && sizeof(SrlColorPoint) == 24 && sizeof(SrlColorSlot) == 16 && sizeof(SrlGridCell) == 16, "DESIGN.md section 3");
static_assert(sizeof(srl_color_stored) == 28, "srl_color_stored is 28 bytes on both sides of the C-ABI");

namespace {

#define SRL_COLOR_NO_OWNER 0x7FFFFFFFu

struct ColorArgs {          // what every kernel of one insertion shares
    int m, step;            // participating points; batch index of j = j * step
    const double *xyz;      // world points, AoS
    double size_voxel, size_grid;
};

// step 1
__global__ void k_color_keys(ColorArgs A, unsigned long long *keyw, unsigned mask, unsigned epoch16, unsigned *slot_out, unsigned long long *gkey, int *new_flag) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= A.m) return;
    const size_t i = (size_t)j * A.step;
    const float fx = (float)A.xyz[i * 3], fy = (float)A.xyz[i * 3 + 1], fz = (float)A.xyz[i * 3 + 2];
    const short kx = (short)(int)((double)fx / A.size_voxel), ky = (short)(int)((double)fy / A.size_voxel), kz = (short)(int)((double)fz / A.size_voxel);
    const short gx = (short)(int)((double)fx / A.size_grid), gy = (short)(int)((double)fy / A.size_grid), gz = (short)(int)((double)fz / A.size_grid);
    const unsigned long long key = srl_pack_key(kx, ky, kz);
    slot_out[j] = srl_epoch_claim(keyw, mask, epoch16, key, srl_hash_key(key));
    gkey[j] = srl_pack_key(gx, gy, gz);
    new_flag[j] = 0;                       // (the segment scan, behind the sort, sets the marks)
}

struct ColorHeadFlag {
    const unsigned *slots;
    __device__ int operator()(int i) const { return (i == 0 || slots[i] != slots[i - 1]) ? 1 : 0; }
};
// step 2
struct ColorSegSink {
    const unsigned *slots_sorted, *idx_sorted;
    const unsigned long long *keyw;
    const SrlColorSlot *vtab;
    unsigned vmask;
    const SrlColorVoxel *vox;
    int *seg_of_pos, *seg_start, *seg_voxel, *seg_count;
    unsigned long long *seg_key;
    unsigned char *seg_new;
    int *new_flag, *seg_of_first, *counters;
    int m;
    __device__ void operator()(int pos, int head, int excl) const {
        seg_of_pos[pos] = excl + head - 1;
        if (head) {
            const unsigned long long key = keyw[slots_sorted[pos]] & SRL_KEY48_MASK;
            seg_key[excl] = key;
            seg_start[excl] = pos;
            unsigned h = srl_hash_key(key) & vmask;
            int v = -1;
            for (unsigned probe = 0; probe <= vmask; ++probe) {
                const unsigned long long k = vtab[h].key;
                if (k == key) { v = (int)vtab[h].voxel; break; }
                if (k == SRL_EMPTY_KEY) break;
                h = (h + 1) & vmask;
            }
            seg_voxel[excl] = v;
            seg_count[excl] = v >= 0 ? (int)vox[v].count : 0;
            seg_new[excl] = v < 0 ? 1 : 0;
            if (v < 0) {
                const unsigned first = idx_sorted[pos];            // stable sort: the segment's first element is its earliest point
                new_flag[first] = 1;
                seg_of_first[first] = excl;
            }
        }
        if (pos == m - 1) counters[0] = excl + head;               // segments
    }
};
// step 3
struct ColorCreateSink {
    const int *seg_of_first;
    const unsigned long long *seg_key;
    int V;
    SrlColorVoxel *vox;
    SrlColorSlot *vtab;
    unsigned vmask;
    int *seg_voxel, *counters;
    int m;
    __device__ void operator()(int j, int is_first_of_new, int rank) const {
        if (is_first_of_new) {
            const int s = seg_of_first[j];
            const unsigned long long key = seg_key[s];
            const int v = V + rank;
            SrlColorVoxel rec; rec.key = key; rec.last_visited_time = 0.0; rec.count = 0; rec.pad = 0;      // voxelBlock(): cloudMap.h:153
            vox[v] = rec;
            unsigned h = srl_hash_key(key) & vmask;
            for (unsigned probe = 0; probe <= vmask; ++probe) {
                const unsigned long long prev = atomicCAS(&vtab[h].key, SRL_EMPTY_KEY, key);
                if (prev == SRL_EMPTY_KEY) { vtab[h].voxel = (unsigned)v; break; }
                h = (h + 1) & vmask;
            }
            seg_voxel[s] = v;
        }
        if (j == m - 1) counters[1] = rank + is_first_of_new;      // voxels created
    }
};

// steps 4 (one thread per sorted position)
__global__ void k_color_store(ColorArgs A, const unsigned *idx_sorted, const int *seg_of_pos, const int *seg_start, const int *seg_voxel, const int *seg_count,
                              const unsigned char *seg_new, const int *counters, int cap, double time_sweep_end, int time_differs, SrlColorVoxel *vox,
                              const unsigned long long *gkey, SrlGridCell *grid, unsigned gmask, unsigned seq, int *stored, int *visited, int *vox_of,
                              int *slot_of, unsigned char *created, unsigned *gslot) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= A.m) return;
    const int s = seg_of_pos[pos];
    const int r = pos - seg_start[s];
    const int v = seg_voxel[s];
    const int c0 = seg_count[s];
    const int j = (int)idx_sorted[pos];
    const bool st = r < cap - c0;                                  // IsFull() (:470); a new voxel takes its first point (:497-499)
    stored[j] = st ? 1 : 0;
    vox_of[j] = v;
    slot_of[j] = c0 + r;
    created[j] = (r == 0 && seg_new[s]) ? 1 : 0;
    int vis = 0;
    if (r == 0) {
        const int S = counters[0];
        const int len = (s + 1 < S ? seg_start[s + 1] : A.m) - seg_start[s];
        vox[v].count = (unsigned)(c0 + len < cap ? c0 + len : cap);
        // :487-491 / :510-514 -- only this thread touches the voxel's time in this batch (one segment per voxel)
        if (time_differs && fabs(vox[v].last_visited_time - time_sweep_end) > 1e-5) {
            vox[v].last_visited_time = time_sweep_end;
            vis = 1;
        }
    }
    visited[j] = vis;
    if (st) {
        const unsigned long long g = gkey[j];
        unsigned h = srl_hash_key(g) & gmask;
        for (unsigned probe = 0; probe <= gmask; ++probe) {
            const unsigned long long prev = atomicCAS(&grid[h].key, SRL_EMPTY_KEY, g);
            if (prev == SRL_EMPTY_KEY) { grid[h].born = seq; grid[h].owner = SRL_COLOR_NO_OWNER; break; }   // read by the NEXT kernel only
            if (prev == g) break;
            h = (h + 1) & gmask;
        }
        gslot[j] = h;
    }
}
// step 5
__global__ void k_color_owner(int m, const int *stored, const unsigned *gslot, SrlGridCell *grid, unsigned seq) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m || !stored[j]) return;
    SrlGridCell *c = &grid[gslot[j]];
    if (c->born == seq) atomicMin(&c->owner, (unsigned)j);
}
// step 6
__global__ void k_color_regflag(int m, const int *stored, const unsigned *gslot, const SrlGridCell *grid, unsigned seq, int *reg) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    int r = 0;
    if (stored[j]) { const SrlGridCell c = grid[gslot[j]]; r = (c.born == seq && c.owner == (unsigned)j) ? 1 : 0; }
    reg[j] = r;
}
// step 7
struct ColorStoredSink {
    int *pool_pos, *counters;
    int m;
    __device__ void operator()(int j, int st, int excl) const {
        pool_pos[j] = excl;
        if (j == m - 1) counters[2] = excl + st;                   // points stored
    }
};
struct ColorRegSink {
    ColorArgs A;
    const int *stored, *pool_pos, *vox_of, *slot_of;
    const unsigned char *created;
    const SrlColorVoxel *vox;
    SrlColorPoint *pool;           // the map's pool, already offset by the points stored before this batch
    int *reg_list;                 // ... the registered list, offset by the points registered before
    int P0, R0;
    unsigned char *outcome;        // n bytes (zeroed beforehand when the step skips points) or nullptr
    srl_color_stored *rec;         // m records or nullptr
    int *counters;
    __device__ void operator()(int j, int reg, int excl) const {
        const int st = stored[j];
        const size_t i = (size_t)j * A.step;
        if (st) {
            const float fx = (float)A.xyz[i * 3], fy = (float)A.xyz[i * 3 + 1], fz = (float)A.xyz[i * 3 + 2];
            const int p = pool_pos[j], v = vox_of[j], slot = slot_of[j];
            const int ridx = reg ? R0 + excl : -1;
            SrlColorPoint pt; pt.x = fx; pt.y = fy; pt.z = fz; pt.voxel = v; pt.slot = slot; pt.reg = ridx;
            pool[p] = pt;
            if (reg) reg_list[excl] = P0 + p;
            if (rec) {
                srl_color_stored o;
                o.x = fx; o.y = fy; o.z = fz;
                srl_unpack_key(vox[v].key, &o.kx, &o.ky, &o.kz);
                o.slot = (uint16_t)slot; o.batch_index = (int32_t)i; o.point_index = ridx;
                rec[p] = o;
            }
        }
        if (outcome) outcome[i] = (unsigned char)(st | (created[j] << 1) | (reg << 2));
        if (j == A.m - 1) counters[3] = excl + reg;                // points registered
    }
};
struct ColorVisitedSink {
    const int *vox_of;
    const SrlColorVoxel *vox;
    int *out;                      // 3 ints per listed voxel
    int *counters;
    int m;
    __device__ void operator()(int j, int vis, int excl) const {
        if (vis) {
            short x, y, z;
            srl_unpack_key(vox[vox_of[j]].key, &x, &y, &z);
            out[(size_t)excl * 3] = x; out[(size_t)excl * 3 + 1] = y; out[(size_t)excl * 3 + 2] = z;     // voxelId(int, int, int)
        }
        if (j == m - 1) counters[4] = excl + vis;                  // voxels listed
    }
};

// growth by rebuild
__global__ void k_color_vtab_rebuild(const SrlColorVoxel *vox, int V, SrlColorSlot *vtab, unsigned mask) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const unsigned long long key = vox[v].key;
    unsigned h = srl_hash_key(key) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        if (atomicCAS(&vtab[h].key, SRL_EMPTY_KEY, key) == SRL_EMPTY_KEY) { vtab[h].voxel = (unsigned)v; return; }
        h = (h + 1) & mask;
    }
}
__global__ void k_color_grid_rehash(const SrlGridCell *old_grid, unsigned old_cap, SrlGridCell *grid, unsigned mask) {
    const unsigned o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= old_cap) return;
    const unsigned long long key = old_grid[o].key;
    if (key == SRL_EMPTY_KEY) return;
    unsigned h = srl_hash_key(key) & mask;
    for (unsigned probe = 0; probe <= mask; ++probe) {
        if (atomicCAS(&grid[h].key, SRL_EMPTY_KEY, key) == SRL_EMPTY_KEY) { grid[h].born = 0u; grid[h].owner = SRL_COLOR_NO_OWNER; return; }   // batch numbers start at 1
        h = (h + 1) & mask;
    }
}
// srl_color_registered_download
__global__ void k_color_reg_gather(const int *reg_list, long long first, int count, const SrlColorPoint *pool, const SrlColorVoxel *vox, srl_color_stored *out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int p = reg_list[first + t];
    const SrlColorPoint pt = pool[p];
    srl_color_stored o;
    o.x = pt.x; o.y = pt.y; o.z = pt.z;
    srl_unpack_key(vox[pt.voxel].key, &o.kx, &o.ky, &o.kz);
    o.slot = (uint16_t)pt.slot; o.batch_index = p; o.point_index = pt.reg;
    out[t] = o;
}

unsigned color_pow2(unsigned v) { unsigned p = 1; while (p < v) p <<= 1; return p; }

// a larger array with the old contents in front (the stream is drained before the old block is freed)
template <class T>
int color_grow_array(srl_ctx *ctx, T *&p, size_t used, size_t new_cap) {
    T *np = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&np, new_cap * sizeof(T)));
    if (p && used > 0) HIPCHK(ctx, hipMemcpyAsync(np, p, used * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (p) HIPCHK(ctx, hipFree(p));
    p = np;
    return SRL_OK;
}

// room for `m` more voxels, stored points and registered points (the worst case of a batch: nothing is read back before its end)
int color_reserve(srl_ctx *ctx, SrlColorMap *cm, int m) {
    hipStream_t st = ctx->stream;
    const size_t need_vox = (size_t)cm->num_voxels + (size_t)m, need_pool = (size_t)cm->num_points + (size_t)m, need_reg = (size_t)cm->num_registered + (size_t)m;
    if (need_vox > 0x3FFFFFFFu || need_pool > 0x7FFFFFFFu) { ctx->err = "colour map too large: voxel and pool positions are 32-bit"; return SRL_ERR_UNSUPPORTED; }
    if (need_vox > cm->vox_cap) {
        const size_t cap = std::max<size_t>(need_vox + need_vox / 2, 4096);
        const int rc = color_grow_array(ctx, cm->d_vox, (size_t)cm->num_voxels, cap);
        if (rc) return rc;
        cm->vox_cap = (unsigned)cap;
    }
    if (2u * cm->vox_cap > cm->vtab_cap) {
        const unsigned cap = color_pow2(2u * cm->vox_cap);
        SrlColorSlot *nt = nullptr;
        HIPCHK(ctx, hipMalloc((void **)&nt, (size_t)cap * sizeof(SrlColorSlot)));
        HIPCHK(ctx, hipMemsetAsync(nt, 0xFF, (size_t)cap * sizeof(SrlColorSlot), st));          // every key = SRL_EMPTY_KEY
        if (cm->num_voxels > 0) {
            hipLaunchKernelGGL(k_color_vtab_rebuild, dim3((cm->num_voxels + 255) / 256), dim3(256), 0, st, cm->d_vox, cm->num_voxels, nt, cap - 1);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (cm->d_vtab) { HIPCHK(ctx, hipFree(cm->d_vtab)); ++cm->vtab_rebuilds; }
        cm->d_vtab = nt; cm->vtab_cap = cap;
    }
    if (need_pool > cm->pool_cap) {
        const size_t cap = std::max<size_t>(need_pool + need_pool / 2, 4096);
        const int rc = color_grow_array(ctx, cm->d_pool, (size_t)cm->num_points, cap);
        if (rc) return rc;
        cm->pool_cap = cap;
        { const int rs = srl_color_state_reserve(ctx, cm); if (rs) return rs; }      // the colour state lies parallel to the pool
    }
    if (need_reg > cm->reg_cap) {
        const size_t cap = std::max<size_t>(need_reg + need_reg / 2, 4096);
        const int rc = color_grow_array(ctx, cm->d_reg, (size_t)cm->num_registered, cap);
        if (rc) return rc;
        cm->reg_cap = cap;
    }
    if (2 * cm->reg_cap > cm->grid_cap) {
        const unsigned cap = color_pow2((unsigned)(2 * cm->reg_cap));
        SrlGridCell *ng = nullptr;
        HIPCHK(ctx, hipMalloc((void **)&ng, (size_t)cap * sizeof(SrlGridCell)));
        HIPCHK(ctx, hipMemsetAsync(ng, 0xFF, (size_t)cap * sizeof(SrlGridCell), st));
        if (cm->d_grid && cm->num_registered > 0) {
            hipLaunchKernelGGL(k_color_grid_rehash, dim3((cm->grid_cap + 255) / 256), dim3(256), 0, st, cm->d_grid, cm->grid_cap, ng, cap - 1);
            HIPCHK(ctx, hipGetLastError());
        }
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (cm->d_grid) { HIPCHK(ctx, hipFree(cm->d_grid)); ++cm->grid_rebuilds; }
        cm->d_grid = ng; cm->grid_cap = cap;
    }
    return SRL_OK;
}

}  // namespace

extern "C" void srl_color_opts_default(srl_color_opts *o) {
    if (!o) return;
    o->size_voxel_map = 0.1;              // config/r3live.yaml:71-75 (the class defaults of parameters.h:98-106 are 0.1 / 20 / 0.01 / 4)
    o->max_num_points_in_voxel = 50;
    o->min_distance_points = 0.01;
    o->add_point_step = 1;
}

extern "C" int srl_color_map_create(srl_ctx *ctx, const srl_color_opts *opts) {
    if (!ctx || !opts) return SRL_ERR_BAD_ARG;
    if (!std::isfinite(opts->size_voxel_map) || !(opts->size_voxel_map > 0.0) || !std::isfinite(opts->min_distance_points) || !(opts->min_distance_points > 0.0) ||
        opts->max_num_points_in_voxel < 1 || opts->max_num_points_in_voxel > 255 || opts->add_point_step < 1) {
        ctx->err = "colour map options: sizes finite and > 0, max_num_points_in_voxel 1 ... 255, add_point_step >= 1";
        return SRL_ERR_BAD_ARG;
    }
    if (ctx->color) { ctx->err = "a colour map exists: its options hold for its life (srl_color_map_destroy first)"; return SRL_ERR_BAD_ARG; }
    SrlColorMap *cm = new SrlColorMap();
    cm->opts = *opts;
    ctx->color = cm;                      // storage comes with the first insertion
    return SRL_OK;
}

extern "C" int srl_color_map_destroy(srl_ctx *ctx) {
    if (!ctx) return SRL_ERR_BAD_ARG;
    SrlColorMap *cm = ctx->color;
    if (!cm) return SRL_OK;
    SRL_DISARM(ctx);
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    if (cm->d_vox) hipFree(cm->d_vox);
    if (cm->d_vtab) hipFree(cm->d_vtab);
    if (cm->d_pool) hipFree(cm->d_pool);
    if (cm->d_reg) hipFree(cm->d_reg);
    if (cm->d_grid) hipFree(cm->d_grid);
    srl_color_render_free(cm);
    srl_color_select_free(cm);
    srl_color_track_free(cm);
    for (SrlWgTotals *t : {&cm->render_tot, &cm->select_tot, &cm->vio_tot, &cm->cloud_tot, &cm->track_old_tot, &cm->track_cand_tot}) srl_wg_totals_free(*t);
    srl_epoch_table_free(cm->scratch);
    delete cm;
    ctx->color = nullptr;
    return SRL_OK;
}

extern "C" int srl_color_map_size(srl_ctx *ctx, int64_t *num_points, int32_t *num_voxels, int64_t *num_registered, int64_t *num_grid_cells) {
    if (num_points) *num_points = 0;
    if (num_voxels) *num_voxels = 0;
    if (num_registered) *num_registered = 0;
    if (num_grid_cells) *num_grid_cells = 0;
    if (!ctx) return SRL_ERR_BAD_ARG;
    const SrlColorMap *cm = ctx->color;
    if (!cm) return SRL_ERR_NO_MAP;
    if (num_points) *num_points = cm->num_points;
    if (num_voxels) *num_voxels = cm->num_voxels;
    if (num_registered) *num_registered = cm->num_registered;
    if (num_grid_cells) *num_grid_cells = cm->num_registered;          // one cell per registered point (:481, :506)
    return SRL_OK;
}

extern "C" int srl_debug_color_map_rebuilds(srl_ctx *ctx, int32_t *voxel_table, int32_t *grid_table) {
    if (!ctx) return SRL_ERR_BAD_ARG;
    if (!ctx->color) return SRL_ERR_NO_MAP;
    if (voxel_table) *voxel_table = ctx->color->vtab_rebuilds;
    if (grid_table) *grid_table = ctx->color->grid_rebuilds;
    return SRL_OK;
}

extern "C" int srl_debug_color_epochs(srl_ctx *ctx, uint32_t out[9]) {
    if (!ctx || !out) return SRL_ERR_BAD_ARG;
    const SrlColorMap *cm = ctx->color;
    if (!cm) return SRL_ERR_NO_MAP;
    out[0] = cm->scratch.epoch16; out[1] = cm->sel_cells.epoch16; out[2] = cm->trk_pool.epoch16; out[3] = cm->trk_cells.epoch16;
    out[4] = cm->sel_cells.counter32; out[5] = cm->trk_pool.counter32; out[6] = cm->trk_cells.counter32; out[7] = cm->scratch.counter32;
    out[8] = cm->render_epoch;
    return SRL_OK;
}

extern "C" int srl_debug_set_color_epochs(srl_ctx *ctx, int calls_to_epoch_wrap, int calls_to_counter_wrap) {
    if (!ctx || calls_to_epoch_wrap < -1 || calls_to_epoch_wrap > 0xFFFF || calls_to_counter_wrap < -1) return SRL_ERR_BAD_ARG;
    SrlColorMap *cm = ctx->color;
    if (!cm) return SRL_ERR_NO_MAP;
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // entries written so far carry numbers <= the old ones: moving a number forward keeps all of them stale (epochs compare unequal, a
    // companion word {0xFFFFFFFF - counter, ...} of an earlier call is larger than any of a later one and loses atomicMin)
    const unsigned epoch = 0xFFFFu - (unsigned)calls_to_epoch_wrap, counter = 0xFFFFFFFEu - (unsigned)calls_to_counter_wrap;
    SrlEpochTable *const tables[4] = {&cm->scratch, &cm->sel_cells, &cm->trk_pool, &cm->trk_cells};
    for (const SrlEpochTable *t : tables)
        if ((calls_to_epoch_wrap >= 0 && t->epoch16 > epoch) || (calls_to_counter_wrap >= 0 && t->counter32 > counter)) return SRL_ERR_BAD_ARG;
    if (calls_to_epoch_wrap >= 0 && cm->render_epoch > epoch) return SRL_ERR_BAD_ARG;
    for (SrlEpochTable *t : tables) {
        if (calls_to_epoch_wrap >= 0) t->epoch16 = epoch;
        if (calls_to_counter_wrap >= 0) t->counter32 = counter;
    }
    if (calls_to_epoch_wrap >= 0) cm->render_epoch = epoch;
    return SRL_OK;
}

extern "C" int srl_color_map_insert(srl_ctx *ctx, const double *world_xyz, int n, double time_sweep_end, double time_last_process, uint8_t *outcome,
                                    srl_color_stored *stored, int stored_capacity, int32_t *visited_xyz, int visited_capacity, srl_color_totals *totals) {
    if (totals) std::memset(totals, 0, sizeof *totals);
    if (!ctx || n < 0) return SRL_ERR_BAD_ARG;
    { const int rc = srl_color_need_map_one_rank(ctx); if (rc) return rc; }
    SrlColorMap *cm = ctx->color;
    const bool from_frame = world_xyz == nullptr;
    if (from_frame) {
        if (ctx->frame_world_n < 0 || !ctx->d_frame_world) {
            if (!ctx->frame_world_seen) { ctx->err = "no points given and no frame committed"; return SRL_ERR_BAD_ARG; }
            ctx->err = "a newer frame has been uploaded since the last srl_frame_commit";
            return SRL_ERR_NO_SWEEP;
        }
        n = ctx->frame_world_n;
    }
    if (n > SRL_COLOR_MAP_INSERT_MAX_POINTS) { ctx->err = "more points than the frame pipeline accepts"; return SRL_ERR_BAD_ARG; }
    const int step = cm->opts.add_point_step;
    const int m = (int)(((long long)n + step - 1) / step);          // participating points (:538)
    if ((stored && stored_capacity < m) || (visited_xyz && visited_capacity < m)) { ctx->err = "capacity below the number of participating points"; return SRL_ERR_BAD_ARG; }
    if (n == 0) return SRL_OK;
    SRL_DISARM(ctx);                      // a waiting launch holds the compute units
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    { const int rc = color_reserve(ctx, cm, m); if (rc) return rc; }
    if (++cm->batch_seq == 0xFFFFFFFFu) { ctx->err = "colour map: batch numbers exhausted"; return SRL_ERR_UNSUPPORTED; }

    DevBuf b_xyz;
    const double *d_xyz = ctx->d_frame_world;
    if (!from_frame) {
        HIPCHK(ctx, b_xyz.alloc(ctx, (size_t)n * 3 * sizeof(double)));
        HIPCHK(ctx, hipMemcpyAsync(b_xyz.p, world_xyz, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        d_xyz = b_xyz.as<double>();
    }
    // one block for the per-point / per-segment work arrays (4-byte words unless noted)
    enum { W_SLOT_IN, W_SLOT_SORTED, W_IDX_SORTED, W_TMP_K, W_TMP_V, W_NEWFLAG, W_SEG_OF_FIRST, W_SEG_OF_POS, W_SEG_START, W_SEG_VOXEL, W_SEG_COUNT,
           W_STORED, W_VISITED, W_REG, W_VOX_OF, W_SLOT_OF, W_GSLOT, W_POOL_POS, W_WORDS };
    const size_t mm = ((size_t)m + 63) / 64 * 64;
    DevBuf b_w, b_k64, b_bytes, b_cnt, b_sc, b_outcome, b_rec, b_vis;
    HIPCHK(ctx, b_w.alloc(ctx, mm * 4 * W_WORDS));
    HIPCHK(ctx, b_k64.alloc(ctx, mm * 8 * 2));                      // grid keys | segment keys
    HIPCHK(ctx, b_bytes.alloc(ctx, mm * 2));                        // created | seg_new
    HIPCHK(ctx, b_cnt.alloc(ctx, 64));                              // [0] segments [1] created [2] stored [3] registered [4] visited
    HIPCHK(ctx, b_sc.alloc(ctx, (srl_radix_scratch_ints(m) + srl_scan_scratch_ints(m)) * 4));
    if (outcome) HIPCHK(ctx, b_outcome.alloc(ctx, (size_t)n));
    if (stored) HIPCHK(ctx, b_rec.alloc(ctx, (size_t)m * sizeof(srl_color_stored)));
    HIPCHK(ctx, b_vis.alloc(ctx, (size_t)m * 12));
    auto W = [&](int k) { return b_w.as<int>() + mm * (size_t)k; };
    auto WU = [&](int k) { return reinterpret_cast<unsigned *>(b_w.as<int>() + mm * (size_t)k); };
    unsigned long long *gkey = b_k64.as<unsigned long long>(), *seg_key = gkey + mm;
    unsigned char *created = b_bytes.as<unsigned char>(), *seg_new = created + mm;
    int *cnt = b_cnt.as<int>();
    int *sc_radix = b_sc.as<int>(), *sc_scan = sc_radix + srl_radix_scratch_ints(m);

    unsigned cap2 = 1024, bits = 10;
    while (cap2 < 2u * (unsigned)m) { cap2 <<= 1; ++bits; }
    { const int rc = srl_epoch_table_begin(ctx, cm->scratch, cap2, false); if (rc) return rc; }
    const ColorArgs A = {m, step, d_xyz, cm->opts.size_voxel_map, cm->opts.min_distance_points};
    const dim3 grid_m((m + 255) / 256), block(256);
    if (outcome && step > 1) HIPCHK(ctx, hipMemsetAsync(b_outcome.p, 0, (size_t)n, st));       // the points the step skips
    hipLaunchKernelGGL(k_color_keys, grid_m, block, 0, st, A, cm->scratch.keyw, cap2 - 1, cm->scratch.epoch16, WU(W_SLOT_IN), gkey, W(W_NEWFLAG));
    HIPCHK(ctx, hipGetLastError());
    srl_radix_sort_pairs(WU(W_SLOT_IN), nullptr, WU(W_SLOT_SORTED), WU(W_IDX_SORTED), WU(W_TMP_K), WU(W_TMP_V), m, bits, st, sc_radix);
    HIPCHK(ctx, hipGetLastError());
    srl_scan(ColorHeadFlag{WU(W_SLOT_SORTED)},
             ColorSegSink{WU(W_SLOT_SORTED), WU(W_IDX_SORTED), cm->scratch.keyw, cm->d_vtab, cm->vtab_cap - 1, cm->d_vox, W(W_SEG_OF_POS), W(W_SEG_START),
                          W(W_SEG_VOXEL), W(W_SEG_COUNT), seg_key, seg_new, W(W_NEWFLAG), W(W_SEG_OF_FIRST), cnt, m},
             m, sc_scan, st);
    HIPCHK(ctx, hipGetLastError());
    srl_scan(SrlIntArrayIn{W(W_NEWFLAG)},
             ColorCreateSink{W(W_SEG_OF_FIRST), seg_key, cm->num_voxels, cm->d_vox, cm->d_vtab, cm->vtab_cap - 1, W(W_SEG_VOXEL), cnt, m}, m, sc_scan, st);
    HIPCHK(ctx, hipGetLastError());
    const int time_differs = std::fabs(time_sweep_end - time_last_process) > 1e-5 ? 1 : 0;      // :487, :510 -- the same for every point of the batch
    hipLaunchKernelGGL(k_color_store, grid_m, block, 0, st, A, WU(W_IDX_SORTED), W(W_SEG_OF_POS), W(W_SEG_START), W(W_SEG_VOXEL), W(W_SEG_COUNT), seg_new, cnt,
                       (int)cm->opts.max_num_points_in_voxel, time_sweep_end, time_differs, cm->d_vox, gkey, cm->d_grid, cm->grid_cap - 1, cm->batch_seq,
                       W(W_STORED), W(W_VISITED), W(W_VOX_OF), W(W_SLOT_OF), created, WU(W_GSLOT));
    hipLaunchKernelGGL(k_color_owner, grid_m, block, 0, st, m, W(W_STORED), WU(W_GSLOT), cm->d_grid, cm->batch_seq);
    hipLaunchKernelGGL(k_color_regflag, grid_m, block, 0, st, m, W(W_STORED), WU(W_GSLOT), cm->d_grid, cm->batch_seq, W(W_REG));
    HIPCHK(ctx, hipGetLastError());
    srl_scan(SrlIntArrayIn{W(W_STORED)}, ColorStoredSink{W(W_POOL_POS), cnt, m}, m, sc_scan, st);
    HIPCHK(ctx, hipGetLastError());
    const int P0 = (int)cm->num_points, R0 = (int)cm->num_registered;
    srl_scan(SrlIntArrayIn{W(W_REG)},
             ColorRegSink{A, W(W_STORED), W(W_POOL_POS), W(W_VOX_OF), W(W_SLOT_OF), created, cm->d_vox, cm->d_pool + P0, cm->d_reg + R0, P0, R0,
                          outcome ? b_outcome.as<unsigned char>() : nullptr, stored ? b_rec.as<srl_color_stored>() : nullptr, cnt},
             m, sc_scan, st);
    HIPCHK(ctx, hipGetLastError());
    srl_scan(SrlIntArrayIn{W(W_VISITED)}, ColorVisitedSink{W(W_VOX_OF), cm->d_vox, b_vis.as<int>(), cnt, m}, m, sc_scan, st);
    HIPCHK(ctx, hipGetLastError());

    // the report leaves through the page-locked scratch (pageable destinations are staged by the runtime): the outcome bytes in front of the
    // counters, then -- the counts known -- one DMA per requested list of exactly its length
    const size_t off_outcome = 64, off_rec = off_outcome + (outcome ? ((size_t)n + 63) / 64 * 64 : 0);
    const size_t off_vis = off_rec + (stored ? ((size_t)m * sizeof(srl_color_stored) + 63) / 64 * 64 : 0);
    { const int rc = ensure_host_scratch(ctx, off_vis + (visited_xyz ? (size_t)m * 12 : 0)); if (rc) return rc; }
    if (outcome) HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch + off_outcome, b_outcome.p, (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch, cnt, 5 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    int h_cnt[5];
    std::memcpy(h_cnt, ctx->h_scratch, sizeof h_cnt);
    cm->num_voxels += h_cnt[1];
    cm->num_points += h_cnt[2];
    cm->num_registered += h_cnt[3];
    if (totals) { totals->created = h_cnt[1]; totals->stored = h_cnt[2]; totals->registered = h_cnt[3]; totals->visited = h_cnt[4]; }
    if (outcome) std::memcpy(outcome, ctx->h_scratch + off_outcome, (size_t)n);
    const bool want_rec = stored && h_cnt[2] > 0, want_vis = visited_xyz && h_cnt[4] > 0;
    if (want_rec) HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch + off_rec, b_rec.p, (size_t)h_cnt[2] * sizeof(srl_color_stored), hipMemcpyDeviceToHost, st));
    if (want_vis) HIPCHK(ctx, hipMemcpyAsync(ctx->h_scratch + off_vis, b_vis.p, (size_t)h_cnt[4] * 12, hipMemcpyDeviceToHost, st));
    if (want_rec || want_vis) HIPCHK(ctx, hipStreamSynchronize(st));
    if (want_rec) std::memcpy(stored, ctx->h_scratch + off_rec, (size_t)h_cnt[2] * sizeof(srl_color_stored));
    if (want_vis) std::memcpy(visited_xyz, ctx->h_scratch + off_vis, (size_t)h_cnt[4] * 12);
    return SRL_OK;
}

extern "C" int srl_color_map_download(srl_ctx *ctx, int16_t *keys_xyz, int32_t *counts, double *last_visited_time, int max_voxels, float *xyz,
                                      int32_t *point_index, int64_t max_points) {
    if (!ctx) return SRL_ERR_BAD_ARG;
    const SrlColorMap *cm = ctx->color;
    if (!cm) return SRL_ERR_NO_MAP;
    const int V = cm->num_voxels;
    const long long P = cm->num_points;
    if (((keys_xyz || counts || last_visited_time) && max_voxels < V) || ((xyz || point_index) && max_points < P)) return SRL_ERR_BAD_ARG;
    if (V == 0) return SRL_OK;
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<SrlColorVoxel> vox((size_t)V);
    std::vector<SrlColorPoint> pool((size_t)P);
    HIPCHK(ctx, hipMemcpyAsync(vox.data(), cm->d_vox, (size_t)V * sizeof(SrlColorVoxel), hipMemcpyDeviceToHost, ctx->stream));
    if (P > 0) HIPCHK(ctx, hipMemcpyAsync(pool.data(), cm->d_pool, (size_t)P * sizeof(SrlColorPoint), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<long long> first((size_t)V + 1, 0);
    for (int v = 0; v < V; v++) {
        short x, y, z;
        srl_unpack_key(vox[v].key, &x, &y, &z);
        if (keys_xyz) { keys_xyz[3 * (size_t)v] = x; keys_xyz[3 * (size_t)v + 1] = y; keys_xyz[3 * (size_t)v + 2] = z; }
        if (counts) counts[v] = (int32_t)vox[v].count;
        if (last_visited_time) last_visited_time[v] = vox[v].last_visited_time;
        first[(size_t)v + 1] = first[v] + vox[v].count;
    }
    if (first[V] != P) { ctx->err = "colour map: voxel counts and point pool disagree"; return SRL_ERR_HIP; }
    if (xyz || point_index)
        for (long long p = 0; p < P; p++) {
            const SrlColorPoint &pt = pool[(size_t)p];
            const size_t at = (size_t)(first[pt.voxel] + pt.slot);          // voxel after voxel, slot order
            if (xyz) { xyz[at * 3] = pt.x; xyz[at * 3 + 1] = pt.y; xyz[at * 3 + 2] = pt.z; }
            if (point_index) point_index[at] = pt.reg;
        }
    return SRL_OK;
}

extern "C" int srl_color_registered_download(srl_ctx *ctx, int64_t first, int count, srl_color_stored *out) {
    if (!ctx || first < 0 || count < 0 || (count > 0 && !out)) return SRL_ERR_BAD_ARG;
    const SrlColorMap *cm = ctx->color;
    if (!cm) return SRL_ERR_NO_MAP;
    if (first + count > cm->num_registered) return SRL_ERR_BAD_ARG;
    if (count == 0) return SRL_OK;
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    DevBuf b_out;
    HIPCHK(ctx, b_out.alloc(ctx, (size_t)count * sizeof(srl_color_stored)));
    hipLaunchKernelGGL(k_color_reg_gather, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, cm->d_reg, (long long)first, count, cm->d_pool, cm->d_vox,
                       b_out.as<srl_color_stored>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out, b_out.p, (size_t)count * sizeof(srl_color_stored), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SRL_OK;
}

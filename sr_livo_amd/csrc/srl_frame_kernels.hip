// srl_frame_kernels.hip -- frame-resident pipeline (SURVEY 8(f) rows 1+2): the reconstructed sweep stays in HBM
// from keypoint selection to map insertion.
//   srl_frame_upload            p_frame->point_frame raw points -> HBM (once per sweep)
//   srl_frame_select_keypoints  gridSampling / subSampleFrame (src/utility.cpp:167-201): the device transforms the
//                               frame with the prior pose and keys every point at the sampling voxel size (k_select_group);
//                               the grid-sampling chain below keeps the first point of every voxel and emits the voxels in
//                               std::tr1::unordered_map iteration order.  The selected raw points are gathered on the device
//                               straight into the resident sweep (no keypoint upload).
//   srl_frame_subsample         buildFrame's subSampleFrame (lioOptimization.cpp:838-846) on the undistorted sweep: the same chain
//   srl_frame_take_subsampled   behind k_sub_group (the first shuffle's visit order, keyed on the uncorrected points); then the
//                               second shuffle as a gather into the resident frame
//   the grid-sampling chain     (GridChain: one host sequence for both) group kernel: voxel -> slot of an epoch-tagged scratch table,
//                               atomicMin of the element index (no sort) -> k_select_mark -> scan over the marks (first-occurrence
//                               rank; {std::hash<voxel>, first element} by rank) -> the container's iteration order on the device:
//                               k_tr1_bucket, scan over the bucket counts, k_tr1_rank.  The host waits for one tagged word
//                               {tag, overflow, bad order, count}; it replays the order itself (host/tr1_order.h) for frames
//                               beyond SRL_SCAN_MAX points, an overfull bucket, or on request (frame_order_mode).
//   srl_frame_commit            the re-transform loop of optimize() (optimize.cpp:441-445) + addPointsToMap
//                               (lioOptimization.cpp:520-554) chained on the device.
#include "srl_ctx.h"
#include "srl_frame_scratch.h"
#include "srl_undistort.h"
#include "srl_hash.h"
#include "host/srl_la.h"
#include "host/tr1_order.h"


#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int srl_map_insert_impl(srl_ctx *ctx, const double *world_xyz, bool on_device, int n, double voxel_size,
                        double min_distance_points, int min_num_points, int *num_added, bool defer_counters,
                        const SrlFrameTransform *xf = nullptr, int (*after_first_kernel)(srl_ctx *, void *) = nullptr, void *user = nullptr,
                        const SrlInsertReport *report = nullptr);

namespace {

using Xf = SrlXf;

// the re-transform of optimize() (optimize.cpp:441-445) as a kernel of its own: point = transformPoint(raw)
__global__ void k_frame_world(const double *raw, int n, const Xf X, double *world) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double wx, wy, wz;
    srl_transform_point(X, raw[(size_t)i * 3], raw[(size_t)i * 3 + 1], raw[(size_t)i * 3 + 2], wx, wy, wz);
    world[(size_t)i * 3] = wx; world[(size_t)i * 3 + 1] = wy; world[(size_t)i * 3 + 2] = wz;
}

// what a group kernel of the grid-sampling chain is given: the scratch table's words and epoch, and the marks it clears
struct GroupArgs {
    unsigned long long *keyw, *minw;
    unsigned mask, epoch16, counter32;
    int *flag;
};
// element e lies in the voxel `key` (short(p / size) per axis, utility.cpp:171-173): claim the voxel's slot and keep its smallest element --
// {~frame counter, e}, only ever lowered: a word of an earlier chain loses against any of this one
__device__ __forceinline__ void group_min(const GroupArgs &G, double x, double y, double z, double size, unsigned e) {
    const unsigned long long key = srl_pack_key((short)(int)(x / size), (short)(int)(y / size), (short)(int)(z / size));
    const unsigned h = srl_epoch_claim(G.keyw, G.mask, G.epoch16, key, srl_hash_key(key));
    atomicMin(&G.minw[h], ((unsigned long long)(0xFFFFFFFFu - G.counter32) << 32) | e);
}

// gridSampling keeps the FIRST point of every sampling voxel (utility.cpp:175-183): group the points by voxel key in a scratch hash
// table (open addressing, keys claimed by compare-and-swap) and keep the smallest point index per key (atomicMin) -- no sort: the
// order of the voxels is decided behind this kernel (std::tr1::unordered_map iteration order), from the first indices.
__global__ void k_select_group(const double *raw, int n, const Xf X, double size, const GroupArgs G) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G.flag[i] = 0;                         // (k_select_mark, the next kernel, sets the marks: no fill in front of this one)
    double wx, wy, wz;
    srl_transform_point(X, raw[(size_t)i * 3], raw[(size_t)i * 3 + 1], raw[(size_t)i * 3 + 2], wx, wy, wz);
    group_min(G, wx, wy, wz, size, (unsigned)i);
}
// ... then the voxels in FIRST-OCCURRENCE order (the order subSampleFrame's loop creates them in, utility.cpp:175-183 -- what the
// host's replay of the container's iteration order starts from): every occupied slot marks the index of its first point, an
// exclusive scan over the marks ranks the voxels, and the keys are written out by rank.
__global__ void k_select_mark(const unsigned long long *keyw, const unsigned long long *minw, unsigned cap, unsigned epoch16, int *flag,
                              unsigned long long *key_at, int *bucket_count, unsigned n_buckets) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_buckets) bucket_count[i] = 0;            // (device ordering below: no fill in front of k_tr1_bucket)
    if (i >= cap) return;
    const unsigned long long k = keyw[i];
    if ((unsigned)(k >> 48) != epoch16) return;
    const unsigned f = (unsigned)minw[i];
    flag[f] = 1;
    key_at[f] = k & SRL_KEY48_MASK;
}
// std::hash<voxel> (cloudMap.h:173-184) of a packed voxel key, in the reference's size_t arithmetic: what the container's order depends on
__device__ __forceinline__ unsigned long long tr1_voxel_hash(unsigned long long key) {
    short x, y, z;
    srl_unpack_key(key, &x, &y, &z);
    return (unsigned long long)(long long)x * 73856093ull + (unsigned long long)(long long)y * 19349669ull + (unsigned long long)(long long)z * 83492791ull;
}
// per-element work of the scan over the marks: {std::hash<voxel>, the element the voxel carries} by first-occurrence rank.  The element is
// the index of the voxel's first point, or order[that index] (the sub-sample: the sweep index of the first VISITED point).
// Device ordering: both arrays stay on the device and CountFin leaves the count in sync[1].
// Host replay: the voxels leave the device HERE, stored straight into page-locked host memory, and EmitFin -- the "tile done" step of the same
// scan -- has the last block to finish publish {tag, bad order, count} in one 8-byte word the host waits on.  No rank array, no launch of its
// own, no copy command, no stream synchronisation (a D2H copy + hipStreamSynchronize cost ~25 us per frame).
struct RankSink {
    const unsigned long long *key_at;
    unsigned long long *hash;
    unsigned *first;
    const int *order;                         // may be null
    __device__ void operator()(int i, int is_first, int r) const {
        if (!is_first) return;
        hash[r] = tr1_voxel_hash(key_at[i]);
        first[r] = order ? (unsigned)order[i] : (unsigned)i;
    }
};
// the published count word: {tag (high half), overflow (an overfull bucket, k_tr1_bucket), bad order, count}.  Bad order: srl_frame_subsample's
// visit order was not a permutation (sync[4], set by k_sub_group; never by a selection)
#define SRL_CTRL_OVERFLOW (1u << 31)
#define SRL_CTRL_BAD_ORDER (1u << 30)
#define SRL_CTRL_COUNT_MASK 0x3FFFFFFFu
struct EmitFin {
    unsigned *sync;                           // [0] workgroups done (reset by the last one), [1] the count (written by the workgroup holding the last tile),
                                              // [4] a bad visit order (k_sub_group)
    unsigned long long *host_ctrl;
    unsigned tag;
    __device__ void operator()(int tile_end) const {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x != 0) return;
        if (blockIdx.x == gridDim.x - 1) __hip_atomic_store(sync + 1, (unsigned)tile_end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned prev = __hip_atomic_fetch_add(sync, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == gridDim.x - 1) {
            __hip_atomic_store(sync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned count = __hip_atomic_load(sync + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned bad = __hip_atomic_load(sync + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (k_sub_group, below)
            if (bad) __hip_atomic_store(sync + 4, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence_system();
            __hip_atomic_store(host_ctrl, ((unsigned long long)tag << 32) | (bad ? SRL_CTRL_BAD_ORDER : 0u) | count, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
};

// ---------------------------------------------------------------------------- keypoint ORDER on the device
// gridSampling emits the keypoints in the iteration order of a std::tr1::unordered_map (utility.cpp:167-201).  host/tr1_order.h replays
// the container's moves level by level (one counting sort per rehash: ~70 us of host time for the 14k voxels of a 24k-point frame, on the
// critical path between selection and the first pass).  host/tr1_relation.h states the same order as a relation between two voxels, which
// needs no sequential replay: a count per final bucket (k_tr1_bucket), ONE scan over the bucket counts, and per voxel a rank among the
// handful of voxels sharing its bucket (k_tr1_rank, which also gathers the keypoint's raw point into the resident sweep).  One thread
// per VOXEL, not per bucket: a lane that ranked all pairs of a 6-voxel bucket held the kernel for 40 us.  A bucket with more than
// SRL_TR1_BUCKET_SLOTS voxels (adversarial keys) sends the frame to the host replay.
struct CountFin {
    unsigned *sync;
    __device__ void operator()(int tile_end) const {
        if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) sync[1] = (unsigned)tile_end;
    }
};
// per voxel e (first-occurrence rank): bucket at the final level G, and a RECORD in that bucket's member list that carries what nearly
// every comparison of two voxels of one final bucket ends on -- {e, era(e), bucket at level G - 1} -- so that the ranking lane has
// everything after one load of its bucket (the kernels of this chain are a few dependent loads long and nothing else: every level of
// indirection is ~1 us of the frame)
#define SRL_TR1_REC(e, era, bprev) ((unsigned long long)(e) | ((unsigned long long)(era) << 20) | ((unsigned long long)(bprev) << 32))
#define SRL_TR1_REC_E(r) ((unsigned)(r) & 0xFFFFFu)
#define SRL_TR1_REC_ERA(r) (((unsigned)(r) >> 20) & 0x3Fu)
#define SRL_TR1_REC_BPREV(r) ((unsigned)((r) >> 32))
static_assert(SRL_SCAN_SMALL_MAX <= (1 << 20), "a record holds a 20-bit voxel rank");
__global__ void k_tr1_bucket(const SrlTr1Sched *S, unsigned *sync, const unsigned long long *hash, int *bucket_count, unsigned long long *members,
                             unsigned *bucket_of, unsigned long long *host_ctrl, unsigned tag) {
    __shared__ SrlTr1Sched sh;                                   // 50 words: level look-ups walk it per lane
    static_assert(sizeof(SrlTr1Sched) <= 256 * 4, "one word per thread");
    if (threadIdx.x < sizeof(SrlTr1Sched) / 4) reinterpret_cast<unsigned *>(&sh)[threadIdx.x] = reinterpret_cast<const unsigned *>(S)[threadIdx.x];
    __syncthreads();
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned total = sync[1];
    if (e < total) {
        const int G = srl_tr1_level(&sh, total);
        if (e == 0) sync[3] = (unsigned)G;
        const unsigned era = (unsigned)srl_tr1_level(&sh, e + 1);
        const unsigned long long h = hash[e];
        const unsigned b = (unsigned)(h % sh.nb[G]);
        const unsigned bprev = G > 0 ? (unsigned)(h % sh.nb[G - 1]) : 0u;
        bucket_of[e] = b;
        const int slot = atomicAdd(&bucket_count[b], 1);
        if (slot < SRL_TR1_BUCKET_SLOTS) members[(size_t)b * SRL_TR1_BUCKET_SLOTS + slot] = SRL_TR1_REC(e, era, bprev);
        else __hip_atomic_store(sync + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // more voxels than k_tr1_rank ranks in place
    }
    // The host needs two things from this chain -- the voxel count and whether a bucket overflowed -- and both are known HERE: the last
    // workgroup publishes {tag, overflow, count}; the scan over the bucket counts and k_tr1_rank run on behind the host's back.
    // (No fence: the overflow marks are agent-scope atomics, acknowledged before the barrier; the host reads nothing but the word itself,
    // so it is stored relaxed -- a system-scope RELEASE writes the whole L2 back: 9 us on this kernel.)
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (__hip_atomic_fetch_add(sync, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != gridDim.x - 1) return;
    __hip_atomic_store(sync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned over = __hip_atomic_load(sync + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(sync + 2, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned bad = __hip_atomic_load(sync + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (bad) __hip_atomic_store(sync + 4, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(host_ctrl, ((unsigned long long)tag << 32) | (over ? SRL_CTRL_OVERFLOW : 0u) | (bad ? SRL_CTRL_BAD_ORDER : 0u) | total,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// T_G(o, me) from the two records; falls back to the general relation below level G - 1 (two voxels sharing their bucket at two levels)
struct Tr1EraOfSched {
    const SrlTr1Sched *S;
    __device__ int operator()(unsigned e) const { return srl_tr1_level(S, e + 1); }
};
__device__ __forceinline__ bool tr1_rec_before(const SrlTr1Sched *S, const unsigned long long *hash, int G, unsigned long long ro, unsigned long long rme) {
    const unsigned o = SRL_TR1_REC_E(ro), me = SRL_TR1_REC_E(rme);
    if ((int)SRL_TR1_REC_ERA(ro) == G || (int)SRL_TR1_REC_ERA(rme) == G) return me < o;          // T_G(o, me): the larger insertion index first
    // both older: T_G(o, me) = T_{G-1}(me, o)
    const unsigned bm = SRL_TR1_REC_BPREV(rme), bo = SRL_TR1_REC_BPREV(ro);
    if (bm != bo) return bm < bo;
    return srl_tr1_before_t(G - 1, me, o, Tr1EraOfSched{S}, SrlTr1BucketOfHash{S, hash});      // rare (one pair in ~n_{G-1})
}
// one thread per voxel: position = start of its bucket (scan over the bucket counts) + voxels of the bucket that precede it; writes the
// ordered index list and (kGather: keypoint selection) gathers the keypoint's raw point into the resident sweep
template <bool kGather>
__global__ void k_tr1_rank(const SrlTr1Sched *S, unsigned *sync, const unsigned long long *hash, const unsigned *first, const unsigned long long *members,
                           const int *bucket_count, const int *bucket_start, const unsigned *bucket_of, const double *raw,
                           double *x, double *y, double *z, int *sel) {
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned total = sync[1];
    if (e < total) {
        const unsigned b = bucket_of[e];
        const unsigned fi = first[e];
        const int G = (int)sync[3];
        // second level of loads, all independent: the bucket's count, start, its first four records, the raw point
        const int c = bucket_count[b];
        const int start = bucket_start[b];
        const unsigned long long *m = members + (size_t)b * SRL_TR1_BUCKET_SLOTS;
        const ulonglong2 r01 = *reinterpret_cast<const ulonglong2 *>(m), r23 = *reinterpret_cast<const ulonglong2 *>(m + 2);
        double px = 0.0, py = 0.0, pz = 0.0;
        if (kGather) { px = raw[(size_t)fi * 3]; py = raw[(size_t)fi * 3 + 1]; pz = raw[(size_t)fi * 3 + 2]; }
        if (c <= SRL_TR1_BUCKET_SLOTS) {            // (an overfull bucket: k_tr1_bucket has told the host, which orders the frame itself)
            int rank = 0;
            if (c > 1) {
                // own record: rebuilt from the others' point of view is not possible without its era -> find it among the members
                unsigned long long rme = r01.x;
                if (SRL_TR1_REC_E(r01.y) == e && c > 1) rme = r01.y;
                if (SRL_TR1_REC_E(r23.x) == e && c > 2) rme = r23.x;
                if (SRL_TR1_REC_E(r23.y) == e && c > 3) rme = r23.y;
                for (int i = 4; i < c; ++i) { const unsigned long long r = m[i]; if (SRL_TR1_REC_E(r) == e) rme = r; }
                if (SRL_TR1_REC_E(r01.x) != e && tr1_rec_before(S, hash, G, r01.x, rme)) ++rank;
                if (c > 1 && SRL_TR1_REC_E(r01.y) != e && tr1_rec_before(S, hash, G, r01.y, rme)) ++rank;
                if (c > 2 && SRL_TR1_REC_E(r23.x) != e && tr1_rec_before(S, hash, G, r23.x, rme)) ++rank;
                if (c > 3 && SRL_TR1_REC_E(r23.y) != e && tr1_rec_before(S, hash, G, r23.y, rme)) ++rank;
                for (int i = 4; i < c; ++i) {
                    const unsigned long long r = m[i];
                    if (SRL_TR1_REC_E(r) != e && tr1_rec_before(S, hash, G, r, rme)) ++rank;
                }
            }
            const int k = start + rank;
            sel[k] = (int)fi;
            if (kGather) {
                x[k] = px;
                y[k] = py;
                z[k] = pz;
            }
        }
    }
}

__global__ void k_gather_soa(const double *raw, const int *sel, int m, double *x, double *y, double *z) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int i = sel[k];
    x[k] = raw[(size_t)i * 3];
    y[k] = raw[(size_t)i * 3 + 1];
    z[k] = raw[(size_t)i * 3 + 2];
}

void fill_xf(Xf &X, const double q[4], const double t[3], const double R_il[9], const double t_il[3]) {
    const srl::Mat3 R = srl::Quat(q[0], q[1], q[2], q[3]).toRotationMatrix();     // q as is (utility.cpp:317)
    std::memcpy(X.R, R.a, sizeof X.R);
    std::memcpy(X.t, t, sizeof X.t);
    std::memcpy(X.R_il, R_il, sizeof X.R_il);
    std::memcpy(X.t_il, t_il, sizeof X.t_il);
}

}  // namespace

int srl_ctx_ensure_work(srl_ctx *ctx, int n);   // srl_capi.cpp
bool srl_ctx_is_pinned(const void *p);          // srl_capi.cpp

namespace {

int ensure_frame(srl_ctx *ctx, int n) {
    if (n > ctx->frame_cap) {
        if (ctx->d_frame_raw) HIPCHK(ctx, hipFree(ctx->d_frame_raw));
        if (ctx->d_frame_world) HIPCHK(ctx, hipFree(ctx->d_frame_world));
        ctx->d_frame_raw = ctx->d_frame_world = nullptr;
        ctx->frame_cap = 0;
        const int cap = std::max(n, 4096);
        HIPCHK(ctx, hipMalloc((void **)&ctx->d_frame_raw, (size_t)cap * 3 * sizeof(double)));
        HIPCHK(ctx, hipMalloc((void **)&ctx->d_frame_world, (size_t)cap * 3 * sizeof(double)));
        ctx->frame_cap = cap;
    }
    return SRL_OK;
}

// ---------------------------------------------------------------------------- sweep reconstruction (row f4)
// Per-point stages of buildFrame (lioOptimization.cpp:833-850): distortFrameByConstant / distortFrameByImu
// (utility.cpp:203-306) then transformAllImuPoint (:320-332), one thread per point, FP64, the reference's
// operation order (built with -ffp-contract=off: every + - * / sqrt is a separate IEEE operation).
//   bit-exact against the reference:  transformAllImuPoint (given imu_point), slerp's linear branch (absD >= 1 - eps), so3ToQuat's
//     small-angle branch (theta < 1e-4), MC_NONE, and every point the interval walk leaves untouched -- no transcendental is evaluated.
//   bounded:  slerp's general branch (acos, sin) and so3ToQuat's general branch (sin, cos) call the device math library.  Per point
//     |error| <= 11 * 2^-52 * (|R_il raw + t_il| + |trans|) against an exact evaluation (tests/undistort_checker.py: 4 x the reference's
//     own worst error of 2.57 such units); measured on an MI355X the device's worst error is 2.57 too and its bits differ from the CPU's
//     at 6 of 12 923 points (slerp over 1.3 rad, 35 rad/s gyro) -- a property of two math libraries, not of this kernel.
// tests/test_gpu_undistort_edges.py holds both.
struct Q4d { double w, x, y, z; };

__device__ inline void d_quat_to_rot(const Q4d &q, double R[9]) {             // Eigen toRotationMatrix
    const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}
__device__ inline Q4d d_q_normalized(const Q4d &q) {
    const double z = ((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w;
    if (z > 0.0) { const double n = sqrt(z); return Q4d{q.w / n, q.x / n, q.y / n, q.z / n}; }
    return q;
}
__device__ inline Q4d d_q_mul(const Q4d &a, const Q4d &b) {
    return Q4d{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
               a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
__device__ inline Q4d d_so3_to_quat(double x, double y, double z) {            // numType::so3ToQuat, utility.h:299-324
    const double theta = sqrt((x * x + y * y) + z * z);
    if (theta < 0.0001) return d_q_normalized(Q4d{1.0, x / 2.0, y / 2.0, z / 2.0});
    const double ux = x / theta, uy = y / theta, uz = z / theta;
    const double s = sin(0.5 * theta);
    return d_q_normalized(Q4d{cos(0.5 * theta), ux * s, uy * s, uz * s});
}
__device__ inline Q4d d_q_slerp(const Q4d &a, double t, const Q4d &b) {       // Eigen QuaternionBase::slerp
    const double one = 1.0 - 2.220446049250313e-16;
    const double d = ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w;
    const double absD = fabs(d);
    double scale0, scale1;
    if (absD >= one) { scale0 = 1.0 - t; scale1 = t; }
    else {
        const double theta = acos(absD), sinTheta = sin(theta);
        scale0 = sin((1.0 - t) * theta) / sinTheta;
        scale1 = sin(t * theta) / sinTheta;
    }
    if (d < 0.0) scale1 = -scale1;
    return Q4d{scale0 * a.w + scale1 * b.w, scale0 * a.x + scale1 * b.x, scale0 * a.y + scale1 * b.y, scale0 * a.z + scale1 * b.z};
}
__device__ inline void d_mv(const double R[9], double x, double y, double z, double &ox, double &oy, double &oz) {
    ox = (R[0] * x + R[1] * y) + R[2] * z;
    oy = (R[3] * x + R[4] * y) + R[5] * z;
    oz = (R[6] * x + R[7] * y) + R[8] * z;
}

struct UndistortArgs {
    const double *raw, *rel, *states;      // n x 3, n, n_states x 17
    const int *seg;                        // IMU mode: interval per point, -1 = never reached
    double *imu, *raw_out;                 // n x 3 each; imu is in/out
    int n, mode;
    double tfb, tfe;
    double q0[4], q1[4], tr0[3], tr1[3];
    double R_il[9], t_il[3];
    double Rinv[9], tinv[3], RilT[9], RilT_til[3];
};

__global__ void k_undistort(const UndistortArgs A) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const double rx = A.raw[(size_t)i * 3], ry = A.raw[(size_t)i * 3 + 1], rz = A.raw[(size_t)i * 3 + 2];
    double lx, ly, lz;
    d_mv(A.R_il, rx, ry, rz, lx, ly, lz);
    lx += A.t_il[0]; ly += A.t_il[1]; lz += A.t_il[2];
    double px = A.imu[(size_t)i * 3], py = A.imu[(size_t)i * 3 + 1], pz = A.imu[(size_t)i * 3 + 2];
    if (A.mode == SRL_MC_CONSTANT_VELOCITY) {
        double time_point = A.tfb + A.rel[i] / 1000.0;
        if (fabs(time_point - A.tfb) < 1e-6) time_point = A.tfb + 1e-6;
        if (fabs(time_point - A.tfe) < 1e-6) time_point = A.tfe - 1e-6;
        double alpha = (time_point - A.tfb) / (A.tfe - A.tfb);
        if (alpha > 1) alpha = 1;
        if (alpha < 0) alpha = 0;
        const Q4d qa = d_q_slerp(Q4d{A.q0[0], A.q0[1], A.q0[2], A.q0[3]}, alpha, Q4d{A.q1[0], A.q1[1], A.q1[2], A.q1[3]});
        double R[9];
        d_quat_to_rot(qa, R);
        d_mv(R, lx, ly, lz, px, py, pz);
        px += (1.0 - alpha) * A.tr0[0] + alpha * A.tr1[0];
        py += (1.0 - alpha) * A.tr0[1] + alpha * A.tr1[1];
        pz += (1.0 - alpha) * A.tr0[2] + alpha * A.tr1[2];
    } else if (A.mode == SRL_MC_IMU) {
        const int k = A.seg[i];
        if (k >= 0) {
            const double *a = A.states + 17 * (size_t)k, *b = a + 17;
            const double tb = a[0], te = b[0];
            double time_point = A.tfb + A.rel[i] / 1000.0;
            if (fabs(time_point - tb) < 1e-6) time_point = tb + 1e-6;
            if (fabs(time_point - te) < 1e-6) time_point = te - 1e-6;
            const double dt = time_point - tb;
            const Q4d qp = d_q_normalized(d_q_mul(Q4d{a[10], a[11], a[12], a[13]}, d_so3_to_quat(b[4] * dt, b[5] * dt, b[6] * dt)));
            double R[9];
            d_quat_to_rot(qp, R);
            d_mv(R, lx, ly, lz, px, py, pz);
            px += (a[7] + a[14] * dt) + ((0.5 * b[1]) * dt) * dt;
            py += (a[8] + a[15] * dt) + ((0.5 * b[2]) * dt) * dt;
            pz += (a[9] + a[16] * dt) + ((0.5 * b[3]) * dt) * dt;
        }
    }
    A.imu[(size_t)i * 3] = px; A.imu[(size_t)i * 3 + 1] = py; A.imu[(size_t)i * 3 + 2] = pz;
    // transformAllImuPoint
    double ex, ey, ez, ox, oy, oz;
    d_mv(A.Rinv, px, py, pz, ex, ey, ez);
    ex += A.tinv[0]; ey += A.tinv[1]; ez += A.tinv[2];
    d_mv(A.RilT, ex, ey, ez, ox, oy, oz);
    A.raw_out[(size_t)i * 3] = ox - A.RilT_til[0];
    A.raw_out[(size_t)i * 3 + 1] = oy - A.RilT_til[1];
    A.raw_out[(size_t)i * 3 + 2] = oz - A.RilT_til[2];
}

__global__ void k_gather_aos(const double *src, const int *sel, int m, double *dst) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int i = sel[k];
    dst[(size_t)k * 3] = src[(size_t)i * 3];
    dst[(size_t)k * 3 + 1] = src[(size_t)i * 3 + 1];
    dst[(size_t)k * 3 + 2] = src[(size_t)i * 3 + 2];
}

// ---------------------------------------------------------------------------- buildFrame's sub-sample (lioOptimization.cpp:838-846)
// subSampleFrame (utility.cpp:167-186) over the sweep in the order of the first shuffle: keyed on point3D::point -- the UNCORRECTED sensor-frame
// point (cloudProcessing.cpp:143), d_corr_in -- at the sample size, no pose.  Thread j visits point order[j]; the voxel keeps the point of the
// smallest visit rank j ({~frame counter, j} in the same scratch words keypoint selection lowers); the voxel then carries order[min j] (RankSink).
// The same pass checks that order is a permutation of 0..n-1: an index out of range is not visited, an index seen twice (its tag word already
// holds this call's tag) is still grouped; either sets sync[4], which the publisher of the count word folds into SRL_CTRL_BAD_ORDER.
__global__ void k_sub_group(const int *order, int n, const double *pts, double size, const GroupArgs G, unsigned *seen, unsigned seen_tag, unsigned *bad) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    G.flag[j] = 0;
    const int i = order[j];
    if ((unsigned)i >= (unsigned)n) { __hip_atomic_store(bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
    if (atomicExch(&seen[i], seen_tag) == seen_tag) __hip_atomic_store(bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    group_min(G, pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2], size, (unsigned)j);
}
// the second shuffle and the take: frame point k = kept[perm[k]] (perm == NULL: k) -> the resident frame, and on request its sweep index and
// imu_point; a perm that is not a permutation of 0..m-1 sets *bad (page-locked host word, read behind the stream synchronisation)
__global__ void k_sub_take(const int *kept, const int *perm, int m, unsigned *seen, unsigned seen_tag, const double *raw, const double *imu,
                           double *frame_raw, int *index_out, double *imu_out, unsigned *bad) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int p = perm ? perm[k] : k;
    if ((unsigned)p >= (unsigned)m) { __hip_atomic_store(bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); return; }
    if (perm && atomicExch(&seen[p], seen_tag) == seen_tag) __hip_atomic_store(bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const int i = kept[p];
    frame_raw[(size_t)k * 3] = raw[(size_t)i * 3];
    frame_raw[(size_t)k * 3 + 1] = raw[(size_t)i * 3 + 1];
    frame_raw[(size_t)k * 3 + 2] = raw[(size_t)i * 3 + 2];
    if (index_out) index_out[k] = i;
    if (imu_out) {
        imu_out[(size_t)k * 3] = imu[(size_t)i * 3];
        imu_out[(size_t)k * 3 + 1] = imu[(size_t)i * 3 + 1];
        imu_out[(size_t)k * 3 + 2] = imu[(size_t)i * 3 + 2];
    }
}

// the keypoint ORDER on the device applies to n points (frame_order_mode 0, a bucket table that fits one scan launch): the container's growth
// schedule goes to the device once, *nb_max = bucket count of its level for n elements; 0 = the host replay orders
int tr1_device_order(srl_ctx *ctx, int n, unsigned *nb_max) {
    *nb_max = 0;
    if (ctx->frame_order_mode != 0 || n > SRL_SCAN_MAX) return SRL_OK;
    if (ctx->tr1_steps < 0) {
        SrlTr1Sched S;
        std::memset(&S, 0, sizeof S);
        const int steps = srl::Tr1Order::export_schedule(SRL_SCAN_MAX, S.first, S.nb, SRL_TR1_MAX_STEPS);
        if (steps >= 0) {
            S.steps = steps;
            HIPCHK(ctx, hipMalloc((void **)&ctx->d_tr1_sched, sizeof S));
            HIPCHK(ctx, hipMemcpy(ctx->d_tr1_sched, &S, sizeof S, hipMemcpyHostToDevice));
            std::memcpy(ctx->tr1_first, S.first, sizeof S.first);
            std::memcpy(ctx->tr1_nb, S.nb, sizeof S.nb);
            ctx->tr1_steps = steps;
        } else {
            ctx->tr1_steps = -2;                                      // a growth policy this table cannot hold: host replay from now on
        }
    }
    if (ctx->tr1_steps < 0) return SRL_OK;
    int g = 0;
    while (g < ctx->tr1_steps && ctx->tr1_first[g] <= (unsigned)n) ++g;
    const unsigned nb = ctx->tr1_nb[g];
    if (nb > 0 && nb <= (1u << 23)) *nb_max = nb;                   // (srl_scan takes any size; the member lists are 128 B per bucket)
    return SRL_OK;
}

// wait for the count word {tag, flags, count} of a frame chain (the stream is looked at every ~1M polls: a fault must not become a hang)
int wait_frame_word(srl_ctx *ctx, const unsigned long long *h_ctrl, unsigned tag, const char *what, unsigned long long *out) {
    unsigned long long ctrl = 0, spins = 0;
    while ((unsigned)((ctrl = __atomic_load_n(h_ctrl, __ATOMIC_ACQUIRE)) >> 32) != tag) {
        if ((++spins & 0xFFFFF) == 0) {
            const hipError_t qe = hipStreamQuery(ctx->stream);
            if (qe != hipSuccess && qe != hipErrorNotReady) { ctx->err = std::string(what) + ": " + hipGetErrorString(qe); return SRL_ERR_HIP; }
            if (qe == hipSuccess && (unsigned)(__atomic_load_n(h_ctrl, __ATOMIC_ACQUIRE) >> 32) != tag) {
                ctx->err = std::string(what) + " finished without publishing its voxel list";
                return SRL_ERR_HIP;
            }
        }
    }
    *out = ctrl;
    return SRL_OK;
}

// ---------------------------------------------------------------------------- the grid-sampling chain, host side
// ONE sequence for keypoint selection and the sweep sub-sample: enqueue (the caller's group kernel goes in as a callable), wait, order.
struct GridChain {
    // inputs
    const int *order = nullptr;                 // device: the element a voxel carries is order[its first index] instead of the index (RankSink)
    int *d_list = nullptr;                      // device ordering: where the ordered list goes (null: scratch of the chain's own)
    const double *gather_raw = nullptr;         // device ordering: k_tr1_rank also gathers point list[k] of gather_raw into gx / gy / gz[k]
    double *gx = nullptr, *gy = nullptr, *gz = nullptr;
    // grid_chain_enqueue
    unsigned nb_max = 0, tag = 0;
    bool dev_order = false;
    DevBuf b_flag, b_keyat, b_hash, b_first, b_bcnt, b_members, b_elem, b_bstart, b_list, b_sc;
    // the host exchange block: [0] count word | hashes (8 B) | elements (4 B) | ordered list (4 B)
    unsigned long long *h_ctrl = nullptr, *h_hash = nullptr;
    unsigned *h_first = nullptr;
    int *h_list = nullptr;
    // grid_chain_wait
    int m = 0;                                  // voxels
    bool overflow = false, bad_order = false;
    // grid_chain_order
    bool list_on_host = false;                  // the ordered list is h_list (host replay), else d_list
};

template <class Group>
int grid_chain_enqueue(srl_ctx *ctx, GridChain &C, int n, Group &&launch_group) {
    hipStream_t st = ctx->stream;
    // group by sampling voxel in a scratch table of >= 2 n slots (epoch-tagged: never cleared between frames, srl_frame_scratch.h)
    unsigned cap = 1024;
    while (cap < 2u * (unsigned)n) cap <<= 1;
    // the ORDER on the device (see "keypoint ORDER on the device" above) when the bucket table of n voxels fits the scans
    { const int rco = tr1_device_order(ctx, n, &C.nb_max); if (rco) return rco; }
    const unsigned nb_max = C.nb_max;
    const bool dev_order = C.dev_order = nb_max > 0;
    HIPCHK(ctx, C.b_flag.alloc(ctx, (size_t)n * 4)); HIPCHK(ctx, C.b_keyat.alloc(ctx, (size_t)n * 8));
    HIPCHK(ctx, C.b_sc.alloc(ctx, srl_scan_scratch_ints(std::max(n, (int)nb_max)) * 4));      // tile sums of the scans beyond one launch (srl_scan)
    if (dev_order) {
        HIPCHK(ctx, C.b_hash.alloc(ctx, (size_t)n * 8)); HIPCHK(ctx, C.b_first.alloc(ctx, (size_t)n * 4));
        HIPCHK(ctx, C.b_bcnt.alloc(ctx, (size_t)nb_max * 4)); HIPCHK(ctx, C.b_members.alloc(ctx, (size_t)nb_max * SRL_TR1_BUCKET_SLOTS * 8));
        HIPCHK(ctx, C.b_elem.alloc(ctx, (size_t)n * 4)); HIPCHK(ctx, C.b_bstart.alloc(ctx, (size_t)nb_max * 4));
        if (!C.d_list) { HIPCHK(ctx, C.b_list.alloc(ctx, (size_t)n * 4)); C.d_list = C.b_list.as<int>(); }
    }
    // one epoch of the selection's scratch table per chain: the sub-sample and the selection of a frame share it, the chain that follows opens
    // the next epoch and its {~counter, ...} words win every atomicMin against the ones left here
    int rct = srl_epoch_table_begin(ctx, ctx->sel_table, cap, true);
    if (rct) return rct;
    const SrlEpochTable &T = ctx->sel_table;
    int rcx = ensure_frame_exchange(ctx, 64 + (size_t)n * 16);
    if (rcx) return rcx;
    C.h_ctrl = reinterpret_cast<unsigned long long *>(ctx->h_frame_x);
    C.h_hash = reinterpret_cast<unsigned long long *>(ctx->h_frame_x + 64);
    C.h_first = reinterpret_cast<unsigned *>(ctx->h_frame_x + 64 + (size_t)n * 8);
    C.h_list = reinterpret_cast<int *>(ctx->h_frame_x + 64 + (size_t)n * 12);
    if (++ctx->frame_tag == 0) ++ctx->frame_tag;
    C.tag = ctx->frame_tag;
    __atomic_store_n(C.h_ctrl, 0ull, __ATOMIC_RELEASE);
    int *flag = C.b_flag.as<int>();
    unsigned long long *key_at = C.b_keyat.as<unsigned long long>();
    launch_group(GroupArgs{T.keyw, T.minw, cap - 1, T.epoch16, T.counter32, flag});
    const unsigned mark_threads = dev_order && nb_max > cap ? nb_max : cap;
    hipLaunchKernelGGL(k_select_mark, dim3((mark_threads + 255) / 256), dim3(256), 0, st, T.keyw, T.minw, cap, T.epoch16, flag, key_at,
                       dev_order ? C.b_bcnt.as<int>() : (int *)nullptr, dev_order ? nb_max : 0u);
    if (dev_order) {
        // ranks (first-occurrence order) -> bucket of every voxel at the table's final size, {tag, overflow, bad order, count} to the host ->
        // scan over the bucket counts -> per voxel: rank inside its bucket, ordered list, gather of the raw point on request
        unsigned long long *hash = C.b_hash.as<unsigned long long>(), *members = C.b_members.as<unsigned long long>();
        unsigned *first = C.b_first.as<unsigned>(), *elem = C.b_elem.as<unsigned>();
        int *bcnt = C.b_bcnt.as<int>(), *bstart = C.b_bstart.as<int>();
        srl_scan(SrlIntArrayIn{flag}, RankSink{key_at, hash, first, C.order}, n, C.b_sc.as<int>(), st, CountFin{ctx->d_frame_sync});
        hipLaunchKernelGGL(k_tr1_bucket, dim3((n + 255) / 256), dim3(256), 0, st, ctx->d_tr1_sched, ctx->d_frame_sync, hash, bcnt, members, elem, C.h_ctrl, C.tag);
        srl_scan(SrlIntArrayIn{bcnt}, SrlIntArraySink{bstart}, (int)nb_max, C.b_sc.as<int>(), st);
        auto rank = C.gather_raw ? k_tr1_rank<true> : k_tr1_rank<false>;
        hipLaunchKernelGGL(rank, dim3((n + 255) / 256), dim3(256), 0, st, ctx->d_tr1_sched, ctx->d_frame_sync, hash, first, members, bcnt, bstart, elem,
                           C.gather_raw, C.gx, C.gy, C.gz, C.d_list);
    } else {
        // ranks, hand-over to the host and the completion word in the scan's own pass
        srl_scan(SrlIntArrayIn{flag}, RankSink{key_at, C.h_hash, C.h_first, C.order}, n, C.b_sc.as<int>(), st, EmitFin{ctx->d_frame_sync, C.h_ctrl, C.tag});
    }
    HIPCHK(ctx, hipGetLastError());
    return SRL_OK;
}

// the count word: how many voxels, and what the device had to say about them
int grid_chain_wait(srl_ctx *ctx, GridChain &C, const char *what) {
    unsigned long long ctrl = 0;
    { const int rcw = wait_frame_word(ctx, C.h_ctrl, C.tag, what, &ctrl); if (rcw) return rcw; }
    C.m = (int)((unsigned)ctrl & SRL_CTRL_COUNT_MASK);
    C.overflow = C.dev_order && ((unsigned)ctrl & SRL_CTRL_OVERFLOW);
    C.bad_order = ((unsigned)ctrl & SRL_CTRL_BAD_ORDER) != 0;
    return SRL_OK;
}

// who orders (frame_order_used: 1 the device, 2 the host, 3 the host behind an overfull bucket), and the host's part of it: the voxels arrive in
// FIRST-OCCURRENCE order (= the order subSampleFrame's loop creates them in); the iteration order of its std::tr1::unordered_map comes from
// replaying the container's bucket moves on flat arrays (host/tr1_order.h) for the m distinct voxels (not the n points)
int grid_chain_order(srl_ctx *ctx, GridChain &C) {
    ctx->frame_order_used = C.dev_order ? (C.overflow ? 3 : 1) : 2;
    C.list_on_host = !C.dev_order || C.overflow;
    if (!C.list_on_host) return SRL_OK;
    if (C.overflow) {
        // a bucket with more voxels than the device ranks in place: fetch {hash, element} and order on the host like larger frames
        HIPCHK(ctx, hipMemcpyAsync(C.h_hash, C.b_hash.p, (size_t)C.m * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(C.h_first, C.b_first.p, (size_t)C.m * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    static_assert(sizeof(std::size_t) == sizeof(unsigned long long), "hashes are exchanged as 64-bit words");
    std::vector<int> perm((size_t)C.m);
    srl::Tr1Order::order(reinterpret_cast<const std::size_t *>(C.h_hash), C.m, perm.data());
    for (int r = 0; r < C.m; r++) C.h_list[r] = (int)C.h_first[(size_t)perm[(size_t)r]];
    return SRL_OK;
}

// a fresh tag for the permutation checks (d_sub_seen: sub_cap words, zeroed when allocated and when the tag wraps)
int sub_seen_begin(srl_ctx *ctx, unsigned *tag) {
    if (++ctx->sub_seen_tag == 0) {
        HIPCHK(ctx, hipMemsetAsync(ctx->d_sub_seen, 0, (size_t)ctx->sub_cap * 4, ctx->stream));
        ctx->sub_seen_tag = 1;
    }
    *tag = ctx->sub_seen_tag;
    return SRL_OK;
}

}  // namespace

int srl_corr_reserve(srl_ctx *ctx, int n) {
    if (n <= ctx->corr_cap) return SRL_OK;
    void *bufs[] = {ctx->d_corr_raw, ctx->d_corr_imu, ctx->d_corr_in, ctx->d_corr_rel, ctx->d_corr_seg};
    for (void *b : bufs) if (b) HIPCHK(ctx, hipFree(b));
    ctx->d_corr_raw = ctx->d_corr_imu = ctx->d_corr_in = ctx->d_corr_rel = nullptr; ctx->d_corr_seg = nullptr;
    ctx->corr_cap = 0;
    const int cap = std::max(n, 4096);
    HIPCHK(ctx, hipMalloc((void **)&ctx->d_corr_raw, (size_t)cap * 24));
    HIPCHK(ctx, hipMalloc((void **)&ctx->d_corr_imu, (size_t)cap * 24));
    HIPCHK(ctx, hipMalloc((void **)&ctx->d_corr_in, (size_t)cap * 24));
    HIPCHK(ctx, hipMalloc((void **)&ctx->d_corr_rel, (size_t)cap * 8));
    HIPCHK(ctx, hipMalloc((void **)&ctx->d_corr_seg, (size_t)cap * 4));
    ctx->corr_cap = cap;
    return SRL_OK;
}

int srl_undistort_launch(srl_ctx *ctx, int n, const double *d_states, const srl_imu_state *imu_states, int n_states, double time_frame_begin,
                         int motion_compensation, const double R_il[9], const double t_il[3]) {
    UndistortArgs A;
    A.raw = ctx->d_corr_in; A.rel = ctx->d_corr_rel; A.states = d_states; A.seg = ctx->d_corr_seg;
    A.imu = ctx->d_corr_imu; A.raw_out = ctx->d_corr_raw; A.n = n; A.mode = motion_compensation;
    A.tfb = time_frame_begin; A.tfe = imu_states[n_states - 1].timestamp;
    const srl_imu_state &s0 = imu_states[0], &s1 = imu_states[n_states - 1];
    for (int d = 0; d < 4; d++) { A.q0[d] = s0.quat[d]; A.q1[d] = s1.quat[d]; }
    for (int d = 0; d < 3; d++) { A.tr0[d] = s0.trans[d]; A.tr1[d] = s1.trans[d]; A.t_il[d] = t_il[d]; }
    std::memcpy(A.R_il, R_il, sizeof A.R_il);
    const srl::Mat3 Rinv = srl::Quat(s1.quat[0], s1.quat[1], s1.quat[2], s1.quat[3]).inverse().toRotationMatrix();
    srl::Mat3 Ril;
    std::memcpy(Ril.a, R_il, sizeof Ril.a);
    const srl::Mat3 RilT = Ril.transpose();
    const srl::Vec3 tinv = (-1.0 * Rinv) * srl::vec3(s1.trans[0], s1.trans[1], s1.trans[2]);
    const srl::Vec3 rt = RilT * srl::vec3(t_il[0], t_il[1], t_il[2]);
    std::memcpy(A.Rinv, Rinv.a, sizeof A.Rinv);
    std::memcpy(A.RilT, RilT.a, sizeof A.RilT);
    for (int d = 0; d < 3; d++) { A.tinv[d] = tinv[d]; A.RilT_til[d] = rt[d]; }
    hipLaunchKernelGGL(k_undistort, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, A);
    HIPCHK(ctx, hipGetLastError());
    return SRL_OK;
}

extern "C" {

int srl_frame_undistort(srl_ctx *ctx, const double *raw_xyz, const double *relative_time_ms, const double *imu_point_in, int n,
                        const srl_imu_state *imu_states, int n_states, double time_frame_begin, int motion_compensation,
                        const double R_il[9], const double t_il[3], double *imu_point_out, double *raw_out) {
    if (!ctx || n < 0 || (n > 0 && (!raw_xyz || !relative_time_ms)) || !imu_states || n_states < 1 || !R_il || !t_il)
        return SRL_ERR_BAD_ARG;
    SRL_DISARM(ctx);
    if (motion_compensation != SRL_MC_IMU && motion_compensation != SRL_MC_CONSTANT_VELOCITY && motion_compensation != SRL_MC_NONE)
        return SRL_ERR_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ctx->corr_n = -1;
    ctx->sub_n = -1;
    ctx->corr_from_cut = false;
    int rc = srl_corr_reserve(ctx, n);
    if (rc) return rc;
    if (n == 0) { ctx->corr_n = 0; return SRL_OK; }
    hipStream_t st = ctx->stream;
    DevBuf b_states;
    HIPCHK(ctx, b_states.alloc(ctx, (size_t)n_states * sizeof(srl_imu_state)));
    static_assert(sizeof(srl_imu_state) == 17 * sizeof(double), "srl_imu_state is 17 packed doubles");
    HIPCHK(ctx, hipMemcpyAsync(b_states.p, imu_states, (size_t)n_states * sizeof(srl_imu_state), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_corr_in, raw_xyz, (size_t)n * 24, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_corr_rel, relative_time_ms, (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (imu_point_in) HIPCHK(ctx, hipMemcpyAsync(ctx->d_corr_imu, imu_point_in, (size_t)n * 24, hipMemcpyHostToDevice, st));
    else HIPCHK(ctx, hipMemsetAsync(ctx->d_corr_imu, 0, (size_t)n * 24, st));

    std::vector<int> seg;
    if (motion_compensation == SRL_MC_IMU) {
        // Integer control flow on N timestamps (srl_undistort.h): replayed on the host; the per-point math runs on the device.
        seg.resize((size_t)n);
        srl_imu_interval_walk(relative_time_ms, n, imu_states, n_states, time_frame_begin, seg.data());
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_corr_seg, seg.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    }

    rc = srl_undistort_launch(ctx, n, b_states.as<double>(), imu_states, n_states, time_frame_begin, motion_compensation, R_il, t_il);
    if (rc) return rc;
    if (imu_point_out) HIPCHK(ctx, hipMemcpyAsync(imu_point_out, ctx->d_corr_imu, (size_t)n * 24, hipMemcpyDeviceToHost, st));
    if (raw_out) HIPCHK(ctx, hipMemcpyAsync(raw_out, ctx->d_corr_raw, (size_t)n * 24, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    ctx->corr_n = n;
    return SRL_OK;
}

int srl_frame_take(srl_ctx *ctx, const int32_t *index, int m) {
    if (!ctx || m < 0 || (m > 0 && !index)) return SRL_ERR_BAD_ARG;
    SRL_DISARM(ctx);
    if (ctx->corr_n < 0) { ctx->err = "no undistorted sweep (srl_frame_undistort first)"; return SRL_ERR_NO_SWEEP; }
    for (int k = 0; k < m; k++)
        if (index[k] < 0 || index[k] >= ctx->corr_n) { ctx->err = "frame index out of range"; return SRL_ERR_BAD_ARG; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = ensure_frame(ctx, m);
    if (rc) return rc;
    ctx->frame_n = m;
    ctx->frame_world_n = -1;
    if (m > 0) {
        DevBuf b_sel;
        HIPCHK(ctx, b_sel.alloc(ctx, (size_t)m * 4));
        HIPCHK(ctx, hipMemcpyAsync(b_sel.p, index, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_gather_aos, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_corr_raw, b_sel.as<int>(), m, ctx->d_frame_raw);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return SRL_OK;
}

int srl_frame_subsample(srl_ctx *ctx, const int32_t *visit_order, int n, double sample_size, int *num_kept) {
    if (num_kept) *num_kept = 0;
    if (!ctx || n < 0 || (n > 0 && !visit_order) || !(sample_size > 0.0) || !num_kept) return SRL_ERR_BAD_ARG;
    SRL_DISARM(ctx);
    if (ctx->nranks > 1) { ctx->err = "frame pipeline is single-rank (shard with srl_sweep_upload instead)"; return SRL_ERR_UNSUPPORTED; }
    if (ctx->corr_n < 0) { ctx->err = "no undistorted sweep (srl_frame_undistort first)"; return SRL_ERR_NO_SWEEP; }
    ctx->sub_n = -1;
    if (n != ctx->corr_n) { ctx->err = "visit order: n is not the size of the undistorted sweep"; return SRL_ERR_BAD_ARG; }
    if ((unsigned)n > SRL_CTRL_COUNT_MASK) { ctx->err = "sweep too large for one sub-sample"; return SRL_ERR_UNSUPPORTED; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    static const bool trace = std::getenv("SRL_FRAME_TIMING") != nullptr;      // stage times on stderr (tools/frame_build_probe.py)
    const auto tp0 = std::chrono::steady_clock::now();
    auto tp1 = tp0, tp2 = tp0, tp3 = tp0;
    ctx->frame_order_used = 0;
    if (n == 0) { ctx->sub_n = 0; return SRL_OK; }
    hipStream_t st = ctx->stream;
    if (n > ctx->sub_cap) {
        if (ctx->d_sub_kept || ctx->d_sub_seen) HIPCHK(ctx, hipStreamSynchronize(st));       // a take may still read the old blocks
        if (ctx->d_sub_kept) { HIPCHK(ctx, hipFree(ctx->d_sub_kept)); ctx->d_sub_kept = nullptr; }
        if (ctx->d_sub_seen) { HIPCHK(ctx, hipFree(ctx->d_sub_seen)); ctx->d_sub_seen = nullptr; }
        ctx->sub_cap = 0;
        const int cap = std::max(n, 4096);
        HIPCHK(ctx, hipMalloc((void **)&ctx->d_sub_kept, (size_t)cap * 4));
        HIPCHK(ctx, hipMalloc((void **)&ctx->d_sub_seen, (size_t)cap * 4));
        HIPCHK(ctx, hipMemsetAsync(ctx->d_sub_seen, 0, (size_t)cap * 4, st));
        ctx->sub_cap = cap;
        ctx->sub_seen_tag = 0;
    }
    unsigned seen_tag = 0;
    { const int rcs = sub_seen_begin(ctx, &seen_tag); if (rcs) return rcs; }
    DevBuf b_order;
    HIPCHK(ctx, b_order.alloc(ctx, (size_t)n * 4));
    HIPCHK(ctx, hipMemcpyAsync(b_order.p, visit_order, (size_t)n * 4, hipMemcpyHostToDevice, st));
    GridChain C;
    C.order = b_order.as<int>();
    C.d_list = ctx->d_sub_kept;
    const int rce = grid_chain_enqueue(ctx, C, n, [&](const GroupArgs &G) {
        hipLaunchKernelGGL(k_sub_group, dim3((n + 255) / 256), dim3(256), 0, st, C.order, n, ctx->d_corr_in, sample_size, G, ctx->d_sub_seen, seen_tag,
                           ctx->d_frame_sync + 4);
    });
    if (rce) return rce;
    tp1 = std::chrono::steady_clock::now();
    { const int rcw = grid_chain_wait(ctx, C, "frame sub-sample"); if (rcw) return rcw; }
    tp2 = std::chrono::steady_clock::now();
    if (C.bad_order) { ctx->err = "visit order is not a permutation of 0..n-1"; return SRL_ERR_BAD_ARG; }
    const int m = C.m;
    { const int rco = grid_chain_order(ctx, C); if (rco) return rco; }
    if (C.list_on_host) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_sub_kept, C.h_list, (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipStreamSynchronize(st));      // (the exchange block is the next chain's)
    }
    tp3 = std::chrono::steady_clock::now();
    ctx->sub_n = m;
    *num_kept = m;
    if (trace) {
        auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        std::fprintf(stderr, "[srl_frame_subsample] n %d -> %d (order %d): enqueue %.0f us, wait %.0f us, host order replay %.0f us\n", n, m,
                     ctx->frame_order_used, us(tp0, tp1), us(tp1, tp2), us(tp2, tp3));
    }
    return SRL_OK;
}

int srl_frame_take_subsampled(srl_ctx *ctx, const int32_t *perm, int m, int32_t *index_out, double *raw_out, double *imu_out) {
    if (!ctx || m < 0) return SRL_ERR_BAD_ARG;
    SRL_DISARM(ctx);
    if (ctx->corr_n < 0 || ctx->sub_n < 0) { ctx->err = "no sub-sample of an undistorted sweep (srl_frame_subsample first)"; return SRL_ERR_NO_SWEEP; }
    if (m != ctx->sub_n) { ctx->err = "m is not the voxel count of the sub-sample"; return SRL_ERR_BAD_ARG; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = ensure_frame(ctx, m);
    if (rc) return rc;
    ctx->frame_n = m;
    ctx->frame_world_n = -1;
    if (m == 0) return SRL_OK;
    hipStream_t st = ctx->stream;
    unsigned seen_tag = 0;
    { const int rcs = sub_seen_begin(ctx, &seen_tag); if (rcs) return rcs; }
    DevBuf b_perm, b_idx, b_imu;
    if (perm) {
        HIPCHK(ctx, b_perm.alloc(ctx, (size_t)m * 4));
        HIPCHK(ctx, hipMemcpyAsync(b_perm.p, perm, (size_t)m * 4, hipMemcpyHostToDevice, st));
    }
    if (index_out) HIPCHK(ctx, b_idx.alloc(ctx, (size_t)m * 4));
    if (imu_out) HIPCHK(ctx, b_imu.alloc(ctx, (size_t)m * 24));
    int rcx = ensure_frame_exchange(ctx, 64);
    if (rcx) return rcx;
    unsigned *h_bad = reinterpret_cast<unsigned *>(ctx->h_frame_x + 8);      // (word 0 is the count word of the chains)
    __atomic_store_n(h_bad, 0u, __ATOMIC_RELEASE);
    hipLaunchKernelGGL(k_sub_take, dim3((m + 255) / 256), dim3(256), 0, st, ctx->d_sub_kept, perm ? b_perm.as<int>() : (const int *)nullptr, m,
                       ctx->d_sub_seen, seen_tag, ctx->d_corr_raw, ctx->d_corr_imu, ctx->d_frame_raw, index_out ? b_idx.as<int>() : (int *)nullptr,
                       imu_out ? b_imu.as<double>() : (double *)nullptr, h_bad);
    HIPCHK(ctx, hipGetLastError());
    if (index_out) HIPCHK(ctx, hipMemcpyAsync(index_out, b_idx.p, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    if (raw_out) HIPCHK(ctx, hipMemcpyAsync(raw_out, ctx->d_frame_raw, (size_t)m * 24, hipMemcpyDeviceToHost, st));
    if (imu_out) HIPCHK(ctx, hipMemcpyAsync(imu_out, b_imu.p, (size_t)m * 24, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (__atomic_load_n(h_bad, __ATOMIC_ACQUIRE)) {
        ctx->frame_n = -1;                                   // (the resident frame was partly overwritten)
        ctx->err = "perm is not a permutation of 0..m-1";
        return SRL_ERR_BAD_ARG;
    }
    return SRL_OK;
}

int srl_frame_upload(srl_ctx *ctx, const double *raw_xyz, int n) {
    if (!ctx || n < 0 || (n > 0 && !raw_xyz)) return SRL_ERR_BAD_ARG;
    SRL_DISARM(ctx);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc0 = ensure_frame(ctx, n);
    if (rc0) return rc0;
    ctx->frame_n = n;
    ctx->frame_world_n = -1;
    srl_stage_begin(ctx);
    if (n > 0) {
        if (!srl_ctx_is_pinned(raw_xyz)) {
            // a pageable source is consumed here
            HIPCHK(ctx, hipMemcpyAsync(ctx->d_frame_raw, raw_xyz, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        } else {
            // a page-locked source (srl_pinned_alloc) is read by the DMA engine behind this call: the caller may refill it once a later call
            // on this context has returned results (like srl_sweep_upload; srl_sweep_wait waits explicitly).  The copy runs on the COPY
            // stream, behind the last kernel that read the previous frame's raw points and beside whatever the compute stream still has to
            // do for that frame (its deferred map insertion); the compute stream picks up behind the copy.
            int rcc = ensure_copy_stream(ctx);
            if (rcc) return rcc;
            if (ctx->ev_frame_read) HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_frame_read, 0));
            HIPCHK(ctx, hipMemcpyAsync(ctx->d_frame_raw, raw_xyz, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->copy_stream));
            if (!ctx->upload_ev) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->upload_ev, hipEventDisableTiming));
            HIPCHK(ctx, hipEventRecord(ctx->upload_ev, ctx->copy_stream));
            HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->upload_ev, 0));
            ctx->upload_pending = true;
        }
    }
    srl_stage_end(ctx, 0);
    return SRL_OK;
}

int srl_frame_size(srl_ctx *ctx, int *n) {
    if (!ctx || !n) return SRL_ERR_BAD_ARG;
    *n = ctx->frame_n < 0 ? 0 : ctx->frame_n;
    return ctx->frame_n < 0 ? SRL_ERR_NO_SWEEP : SRL_OK;
}

int srl_frame_select_keypoints(srl_ctx *ctx, const double q[4], const double t[3], const double R_il[9], const double t_il[3],
                               double sample_voxel_size, int32_t *keypoint_index, int *num_keypoints) {
    if (!ctx || !q || !t || !R_il || !t_il || !(sample_voxel_size > 0.0)) return SRL_ERR_BAD_ARG;
    SRL_DISARM(ctx);
    if (ctx->frame_n < 0 || !ctx->d_frame_raw) { ctx->err = "no frame uploaded"; return SRL_ERR_NO_SWEEP; }
    if (ctx->nranks > 1) { ctx->err = "frame pipeline is single-rank (shard with srl_sweep_upload instead)"; return SRL_ERR_UNSUPPORTED; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int n = ctx->frame_n;
    if (num_keypoints) *num_keypoints = 0;
    hipStream_t st = ctx->stream;
    static const bool trace = std::getenv("SRL_FRAME_TIMING") != nullptr;      // stage times on stderr (tools/pipeline_probe.py)
    const auto tp0 = std::chrono::steady_clock::now();
    auto tp1 = tp0, tp2 = tp0, tp3 = tp0;
    srl_stage_begin(ctx);
    ctx->frame_order_used = 0;
    int m = 0;
    if (n > 0) {
        // the selection becomes the resident sweep (SoA, gathered on the device): at most n keypoints
        int rc = ctx->cur.reserve_soa(ctx, n);
        if (rc) return rc;
        if ((rc = srl_ctx_ensure_work(ctx, n))) return rc;
        Xf X;
        fill_xf(X, q, t, R_il, t_il);
        // the keypoints' raw points become the resident sweep: gathered by the chain's last kernel, or behind the host's replay
        double *sx = ctx->cur.x(), *sy = ctx->cur.y(), *sz = ctx->cur.z();
        GridChain C;
        C.gather_raw = ctx->d_frame_raw; C.gx = sx; C.gy = sy; C.gz = sz;
        rc = grid_chain_enqueue(ctx, C, n, [&](const GroupArgs &G) {
            hipLaunchKernelGGL(k_select_group, dim3((n + 255) / 256), dim3(256), 0, st, ctx->d_frame_raw, n, X, sample_voxel_size, G);
        });
        if (rc) return rc;
        srl_stage_end(ctx, 1);
        tp1 = std::chrono::steady_clock::now();
        rc = grid_chain_wait(ctx, C, "keypoint selection");      // (bad_order: no selection sets it)
        if (rc) return rc;
        srl_stage_end(ctx, 2);
        tp2 = std::chrono::steady_clock::now();
        m = C.m;
        rc = grid_chain_order(ctx, C);
        if (rc) return rc;
        srl_stage_end(ctx, 3);
        if (C.list_on_host) {
            // the gather reads the ordered index list straight out of the exchange block (its own region: nothing is written there before
            // the next frame's list, and that is produced behind a wait on a later kernel of this stream)
            tp3 = std::chrono::steady_clock::now();
            if (m > 0) {
                hipLaunchKernelGGL(k_gather_soa, dim3((m + 255) / 256), dim3(256), 0, st, ctx->d_frame_raw, C.h_list, m, sx, sy, sz);
                HIPCHK(ctx, hipGetLastError());
            }
        } else {
            tp3 = tp2;
            if (keypoint_index && m > 0) {
                // the ordered index list is wanted on the host (tests, tools; the host mirror passes NULL): one copy behind the chain
                HIPCHK(ctx, hipMemcpyAsync(C.h_list, C.d_list, (size_t)m * 4, hipMemcpyDeviceToHost, st));
                HIPCHK(ctx, hipStreamSynchronize(st));
            }
        }
        if (keypoint_index) std::memcpy(keypoint_index, C.h_list, (size_t)m * 4);
    } else {
        srl_stage_end(ctx, 3);
    }
    if (num_keypoints) *num_keypoints = m;
    srl_sweep_becomes_current(ctx, m, 0, m, m, false);      // (gathered straight into the planes)
    if (n > 0) { const int rcm = srl_mark_frame_read(ctx); if (rcm) return rcm; }
    srl_stage_end(ctx, 4);
    if (trace) {
        const auto tp4 = std::chrono::steady_clock::now();
        auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        std::fprintf(stderr, "[srl_frame_select_keypoints] n %d -> %d (order %d): enqueue %.0f us, wait %.0f us, host order replay %.0f us, gather + rest %.0f us\n",
                     n, m, ctx->frame_order_used, us(tp0, tp1), us(tp1, tp2), us(tp2, tp3), us(tp3, tp4));
    }
    return SRL_OK;
}

}  // extern "C"

namespace {
int frame_commit_impl(srl_ctx *ctx, const double q[4], const double t[3], const double R_il[9], const double t_il[3], double voxel_size, int cap,
                      double min_distance_points, int min_num_points, double *world_out, int *num_added, const SrlInsertReport *report) {
    if (!ctx || !q || !t || !R_il || !t_il) return SRL_ERR_BAD_ARG;
    SRL_DISARM(ctx);
    if (cap != SRL_VOXEL_CAP) { ctx->err = "max_num_points_in_voxel must be 20"; return SRL_ERR_UNSUPPORTED; }
    if (ctx->frame_n < 0 || !ctx->d_frame_raw) { ctx->err = "no frame uploaded"; return SRL_ERR_NO_SWEEP; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int n = ctx->frame_n;
    if (num_added) *num_added = 0;
    if (n == 0) return SRL_OK;
    SrlFrameTransform xf;
    xf.raw = ctx->d_frame_raw; xf.world = ctx->d_frame_world;
    fill_xf(xf.X, q, t, R_il, t_il);
    struct Download { double *world_out; int n; } dl = {world_out, n};
    // what has to happen as soon as the world points exist: the frame's raw points are free for the next upload, point3D::point leaves on
    // the copy stream beside the insertion
    auto world_ready = [](srl_ctx *c, void *user) -> int {
        const Download *d = static_cast<const Download *>(user);
        { const int rcm = srl_mark_frame_read(c); if (rcm) return rcm; }       // (= the world points are ready)
        if (d->world_out) {
            int rcc = ensure_copy_stream(c);
            if (rcc) return rcc;
            HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_frame_read, 0));
            HIPCHK(c, hipMemcpyAsync(d->world_out, c->d_frame_world, (size_t)d->n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->copy_stream));
            if (!c->ev_world) HIPCHK(c, hipEventCreateWithFlags(&c->ev_world, hipEventDisableTiming));
            HIPCHK(c, hipEventRecord(c->ev_world, c->copy_stream));
        }
        return SRL_OK;
    };
    srl_stage_begin(ctx);
    // A frame-sized batch outside the stage-timing mode: the re-transform is the first thing the insertion's first kernel does (one launch
    // less on a chain whose cost is its launches); otherwise a kernel of its own, as stage 5 of srl_debug_frame_timing.
    const bool fused = n <= SRL_SCAN_MAX && !ctx->frame_timing;
    if (!fused) {
        hipLaunchKernelGGL(k_frame_world, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_frame_raw, n, xf.X, ctx->d_frame_world);
        HIPCHK(ctx, hipGetLastError());
        srl_stage_end(ctx, 5);
        const int rcw = world_ready(ctx, &dl);
        if (rcw) return rcw;
        srl_stage_end(ctx, 6);
    }
    // num_added == NULL: the insert is only enqueued (its counters are folded in later, srl_map_settle); the caller's world points are
    // waited for on their own event, which fires long before the insert behind them is done
    const int rci = srl_map_insert_impl(ctx, ctx->d_frame_world, true, n, voxel_size, min_distance_points, min_num_points, num_added,
                                        num_added == nullptr && !report, fused ? &xf : nullptr, fused ? +world_ready : nullptr, &dl, report);
    if (world_out && rci == SRL_OK) HIPCHK(ctx, hipEventSynchronize(ctx->ev_world));
    if (rci == SRL_OK) { ctx->frame_world_n = n; ctx->frame_world_seen = true; }     // d_frame_world = the frame as inserted (srl_map_probe_checksum, srl_color_map_insert)
    return rci;
}
}  // namespace

extern "C" {
int srl_frame_commit(srl_ctx *ctx, const double q[4], const double t[3], const double R_il[9], const double t_il[3],
                     double voxel_size, int cap, double min_distance_points, int min_num_points, double *world_out, int *num_added) {
    return frame_commit_impl(ctx, q, t, R_il, t_il, voxel_size, cap, min_distance_points, min_num_points, world_out, num_added, nullptr);
}
int srl_frame_commit_report(srl_ctx *ctx, const double q[4], const double t[3], const double R_il[9], const double t_il[3],
                            double voxel_size, int cap, double min_distance_points, int min_num_points, double *world_out, uint8_t *outcome,
                            srl_cloud_point *cloud, int *num_cloud, int *num_added) {
    if (num_cloud) *num_cloud = 0;
    if (num_added) *num_added = 0;
    if (!ctx || !q || !t || !R_il || !t_il) return SRL_ERR_BAD_ARG;
    const SrlInsertReport rep = {t[2], outcome, cloud, num_cloud};
    return frame_commit_impl(ctx, q, t, R_il, t_il, voxel_size, cap, min_distance_points, min_num_points, world_out, num_added, &rep);
}
}  // extern "C"

// srl_ctx.h -- internal: the context object behind the opaque srl_ctx handle of include/srlivo_hip.h
#pragma once
#include "../../include/srlivo_hip.h"
#include "srl_device.h"
#include "srl_carve.h"
#include "host/tr1_relation.h"

#include <hip/hip_runtime.h>
#include "srl_rccl.h"

#include <string>
#include <vector>

// scratch hash table of the per-frame kernels that is never cleared between frames (srl_frame_scratch.h)
struct SrlEpochTable {
    unsigned long long *keyw = nullptr;       // (epoch16 << 48) | key48
    unsigned long long *minw = nullptr;       // optional companion: {~frame counter, smallest index}
    unsigned cap = 0;                         // slots allocated (power of two)
    unsigned epoch16 = 0;
    unsigned counter32 = 0;
};

// The word behind a rank's inbox rows that any rank sets when it gives a session up (srl_peer_set_deadline_ms): a rank whose pass times
// out looks at its own inbox's word and ends the session at once instead of waiting for its own deadline.
#define SRL_PEER_POISON_WORD SRL_PEER_INBOX_GRANULES
// ... and the word behind it: an identity of the DEVICE the inbox lives on (hash of its PCI bus id, never 0), written at srl_peer_export.
// srl_peer_attach compares the peers' words with its own: ranks that share a device (a test arrangement -- production is one process per
// GPU) do not arm launches, whose waiting workgroups would hold the compute units the other rank's kernel needs.
#define SRL_PEER_DEVICE_WORD (SRL_PEER_INBOX_GRANULES + 1)
#define SRL_PEER_INBOX_ALLOC_GRANULES (SRL_PEER_INBOX_GRANULES + 8)

struct srl_ctx;

// One of the context's two sweep buffers (this rank's shard).  `cur` is the sweep the passes read; `next` is the one srl_sweep_prefetch
// fills on the copy stream while `cur` is solved, and srl_sweep_swap exchanges the two.  Both blocks are grow-only, max(n, 1024) points.
struct SrlSweepSlot {
    double *soa = nullptr;             // SoA x|y|z, stride soa_cap
    double *stage = nullptr;           // AoS staging: the DMA's target (no kernel runs on the copy stream); transposed into soa by the
                                       // first pass that touches the points (SrlAssocArgs::aos)
    int soa_cap = 0, stage_cap = 0;    // capacities (points)
    int n = 0, begin = 0, total = 0;   // shard size, its first point, points of the whole sweep (next: n < 0 = nothing prefetched)
    double *x() const { return soa; }
    double *y() const { return soa + soa_cap; }
    double *z() const { return soa + 2 * (size_t)soa_cap; }
    bool has_buffers() const { return soa != nullptr && soa_cap > 0 && stage != nullptr; }   // an armed launch can carry it as its alternate
    int reserve_soa(srl_ctx *ctx, int points) { return reserve(ctx, soa, soa_cap, points); }
    int reserve_stage(srl_ctx *ctx, int points) { return reserve(ctx, stage, stage_cap, points); }
private:
    static int reserve(srl_ctx *ctx, double *&block, int &cap, int points);
};

// The ARMED launch (srl_capi.cpp: arm_next / fire_or_cancel / srl_ctx_disarm): the kernel of the NEXT pass, enqueued while the current
// one runs and waiting, resident, for its pose.
struct SrlArmedLaunch {
    bool on = false;
    SrlAssocArgs sig;                           // its arguments with the pose zeroed (arm_signature): a pass must equal them to fire it
    int nb = 0, kpw = 0;
    int nblocks = 0;                            // its grid (a pass over fewer keypoints may fire it: the surplus workgroups find empty tiles)
    const double *raw = nullptr, *alt = nullptr;   // x planes of the sweep buffer it was armed on / of the context's other buffer
    const double *alt_aos = nullptr;            // the staging buffer it reads when it is fired for the other buffer
    int raw_cap = 0, alt_cap = 0;               // ... and their strides (capacity in points)
    int ring = -1;                              // light profiling: ring slot of its event pair (-1: none)
    long long at_ns = 0;                        // steady clock at arm time
    bool measured = false;                      // light profiling: is it one of the timed launches ...
    unsigned gen = 0;                           // ... and of which srl_timing_mark generation
    // Which of its two sweep buffers holds the sweep of the pass with arguments `a` (cur: the context's current slot)?  On the buffer it
    // was armed on it reads the SoA planes: they must be valid (no a.aos).  On the other one -- after srl_sweep_swap -- it reads the
    // staging buffer.
    enum Serves { none, own, alternate };
    Serves serves(const SrlSweepSlot &cur, const SrlAssocArgs &a) const {
        if (a.raw_x == raw && cur.soa_cap == raw_cap && a.aos == nullptr) return own;
        if (alt != nullptr && a.raw_x == alt && cur.soa_cap == alt_cap && a.aos != nullptr && a.aos == alt_aos) return alternate;
        return none;
    }
};

// Light profiling (srl_set_profiling(ctx, 2)): the event pairs of association launches, read lazily (srl_capi.cpp: launch_assoc / drain_ring)
struct SrlProfRing {
    static constexpr int SLOTS = 512;
    struct Entry {
        hipEvent_t ev[2] = {};                  // start, end
        int prev = -1;                          // slot whose END event is this launch's start (armed launches), -1 = own start event
        unsigned gen = 0;                       // srl_timing_mark generation it was enqueued in
        bool voided = false;                    // a cancelled armed launch (not counted)
        bool marker = false;                    // with a period: only serves as the NEXT launch's start (not timed itself)
    };
    Entry e[SLOTS];
    unsigned head = 0, tail = 0;                // [tail, head) recorded and not yet read
    int period = 1;                             // srl_set_profiling_period: every period-th association launch is timed
    unsigned long long count = 0;               // association launches seen (own and armed)
    long long last_count = -2;                  // `count` of the launch behind the newest entry
    // srl_timing_mark: "the sums start here" without a read-back -- launches enqueued before the mark carry an older generation and are
    // left out when their events are read (their passes' bytes likewise)
    unsigned gen = 0;
    Entry &at(unsigned i) { return e[i % SLOTS]; }
    unsigned pending() const { return head - tail; }
    void restart() { count = 0; last_count = -2; }
};

struct srl_ctx {
    srl_ctx() { next.n = -1; }
    int device = 0;
    bool counted = false;              // this context is in the per-device census (srl_capi.cpp: g_live_ctx)
    hipStream_t stream = nullptr;
    std::string err;

    // map
    SrlMapSlot *d_table = nullptr;
    unsigned table_cap = 0;            // slots (power of two)
    unsigned char *d_slabs = nullptr;
    unsigned slab_cap = 0;             // slabs allocated
    unsigned *d_nbrec = nullptr;       // neighbour records (srl_device.h): SRL_NBREC_WORDS words per slab, slab_cap of them, allocated and grown with the slabs
    int nbrec_mode = 1;                // srl_debug_set_neighbour_records: 1 = the r = 1 fast path reads them, 0 = it looks every voxel up in the table
    int num_voxels = 0;
    long long num_points = 0;

    // the current sweep, and the NEXT one (srl_sweep_prefetch / srl_sweep_swap): uploaded on its own stream while the current one is solved
    SrlSweepSlot cur, next;
    bool sweep_loaded = false;         // a sweep (possibly empty) has been uploaded / selected
    int soa_valid_n = 0;               // leading keypoints of the current sweep whose SoA planes are filled
    int search_select_mode = 0;        // srl_debug_set_search_select_mode: selection path of srl_search_neighbors (tests)
    int select_mode = 0;               // srl_debug_set_select_mode: selection path of srl_build_residuals (tests; 0 = automatic)
    int ablate = 0;                    // srl_debug_set_ablate (profiling tools only; never set by the product)
    void (*overlap_fn)(void *) = nullptr;   // srl_build_residuals_overlap: host work to run while the kernels are in flight
    void *overlap_user = nullptr;

    hipStream_t copy_stream = nullptr;
    hipStream_t prefix_stream = nullptr;  // the PREFIX of a prefix-first prefetch: a stream (and with it a DMA engine) of its own, beside the tail
    int num_cu = 256;                 // compute units of the device (launch-shape policy)
    // PREFIX-FIRST upload.  With a finite max_num_residuals a solve visits only the first few thousand keypoints of
    // a sweep (srl_build_residuals: the prefix pass), yet the whole sweep had to cross PCIe before its first pass could fire.  The prefetch
    // therefore goes out as TWO DMAs -- the prefix the running solve's passes visit (prefix_hint) and the rest -- each with its own event and
    // on a stream of its own (chained on one stream the two copies and their markers took ~63 us per 1.5 MB sweep: every hop between a DMA
    // engine and the stream's queue costs; side by side the prefix lands ~11 us after the call and the tail in the ~36 us one copy takes);
    // two event pairs alternating between consecutive prefetches.  srl_sweep_swap keeps a waiting launch once the PREFIX has landed; a
    // pass that needs more (the whole-shard repeat, other options, anything launched normally) first orders the stream behind the FULL event.
    // (The pairs alternate per PREFETCH, the buffers per SWAP -- a prefetch that replaces one never swapped fills the same buffer behind the
    // other pair -- so the pairs, their parity and what they cover belong to the context, not to a SrlSweepSlot.  "slot" below = pair.)
    hipEvent_t up_ev[2][2] = {};          // [slot][0 = prefix landed, 1 = everything landed]
    bool up_one_dma[2] = {true, true};    // the slot's upload went out as ONE DMA: only its full event was recorded
    int next_slot = 0;                    // slot of the prefetch in flight / last issued
    int next_prefix_n = 0;                // points of it covered by the prefix event (== next.n: one DMA)
    int prefix_hint = 0;                  // keypoints the passes of the running solve visit when that is a prefix of the shard (0: whole sweeps)
    // neighbourhood bounds (SrlAssocArgs::bound_in): 4 floats per keypoint, written by every pass; entries [0, bound_n) were written on the
    // CURRENT sweep and map with the options of bound_sig -- reset by whatever changes one of them
    float *d_bound = nullptr;
    int bound_n = 0;
    int bound_sig[4] = {0, 0, 0, 0};      // K, voxel neighbourhood, occupancy threshold, (float) voxel size bits
    int bound_mode = 1;                   // srl_debug_set_bound_culling: 0 = never use them, 1 = voxel cull and prefilter threshold, 2 = voxel cull only
    bool tail_pending = false;            // the CURRENT sweep's tail may still be in flight: stream not yet ordered behind up_ev[cur_slot][1]
    int cur_slot = 0, cur_prefix_n = 0;   // ... its slot, and how many of its points are known to have landed

    // frame-resident pipeline (srl_frame_*)
    double *d_frame_raw = nullptr;     // AoS n x 3
    double *d_frame_world = nullptr;   // AoS n x 3
    int frame_cap = 0;
    int frame_n = -1;
    int frame_world_n = -1;            // points of d_frame_world as the last srl_frame_commit left them (-1: none, or a newer frame uploaded since)
    bool frame_world_seen = false;     // a frame has been committed at some time (srl_color_map_insert tells "never" from "a newer frame since")
    struct SrlColorMap *color = nullptr;   // the colour voxel map (srl_color_kernels.hip); nullptr until srl_color_map_create
    struct SrlFlow *flow = nullptr;        // the optical-flow tracker (srl_flow.hip); nullptr until srl_flow_create
    struct SrlImagePrep *prep = nullptr;   // the image preparer (srl_image_prep.hip); nullptr until srl_image_prep_create
    struct SrlJpeg *jpeg = nullptr;        // the JPEG decoder (srl_jpeg.hip): made by the first srl_jpeg_decode, freed by srl_jpeg_release
    struct SrlConsensus *consensus = nullptr;   // workspace of srl_consensus_* (srl_consensus.hip): made by the first call, freed by srl_consensus_release
    // undistorted sweep (srl_frame_undistort): inputs, imu_point, corrected raw_point
    double *d_corr_in = nullptr, *d_corr_rel = nullptr, *d_corr_imu = nullptr, *d_corr_raw = nullptr;
    int *d_corr_seg = nullptr;
    int corr_cap = 0;
    int corr_n = -1;
    bool corr_from_cut = false;        // the undistorted sweep came from the device point queue (srl_frame_undistort_cut): its rewritten
                                       // times are resident too (srl_frame_point_times)
    struct SrlPoints *points = nullptr;   // the device point queue and its resident cut (srl_points.hip); nullptr until the first srl_livox_decode
    // buildFrame's sub-sample of the undistorted sweep (srl_frame_subsample): the kept sweep indices in container order, and the tag words
    // that check a permutation on the device (zeroed when allocated; a call tags with a value no earlier call of this block used)
    int *d_sub_kept = nullptr;
    unsigned *d_sub_seen = nullptr;
    int sub_cap = 0;
    int sub_n = -1;                    // voxels kept by the last sub-sample of the CURRENT undistorted sweep (-1: none)
    unsigned sub_seen_tag = 0;

    // srl_debug_frame_timing: per-stage wall time of the frame pipeline (the stream is synchronised at every stage boundary while on)
    bool frame_timing = false;
    double frame_stage_us[16] = {};
    long long frame_stage_last_ns = 0;

    // page-locked sources: event behind the last DMA that read a caller's buffer (srl_sweep_wait)
    hipEvent_t upload_ev = nullptr;
    bool upload_pending = false;

    // pinned staging chunks of a sweep upload from pageable memory (upload_aos): CPU copy of one chunk overlaps the DMA of the previous
    static constexpr int CHUNK_SLOTS = 4;
    static constexpr int CHUNK_BYTES = 256 * 1024;
    char *h_chunks = nullptr;
    hipEvent_t chunk_ev[CHUNK_SLOTS] = {};
    bool chunk_busy[CHUNK_SLOTS] = {};
    unsigned chunk_next = 0;

    // pinned host scratch (grow-only) for the small D2H / H2D hops of the frame pipeline: pageable copies are staged
    // synchronously by the runtime and cost more than the kernels around them
    char *h_scratch = nullptr;
    size_t h_scratch_bytes = 0;
    // frame pipeline <-> host exchange (page-locked, coherent, device-mapped): the selection kernels write the voxel list straight into
    // it and the gather reads the ordered index list out of it -- no copy commands, the host waits on a tagged word, not on the stream
    char *h_frame_x = nullptr;
    size_t h_frame_x_bytes = 0;
    unsigned *d_frame_sync = nullptr;            // [0]: blocks of the emitting kernel that are done (reset by the last one)
    unsigned frame_tag = 0;                      // tag of the last exchange (never 0)
    // keypoint order on the device (srl_frame_kernels.hip): the growth schedule of std::tr1::unordered_map, recorded from a real container
    SrlTr1Sched *d_tr1_sched = nullptr;
    int tr1_steps = -1;                          // steps of the uploaded schedule (-1: not uploaded)
    unsigned tr1_first[SRL_TR1_MAX_STEPS] = {0}, tr1_nb[SRL_TR1_MAX_STEPS + 1] = {0};
    int frame_order_mode = 0;                    // srl_debug_set_frame_order_mode: 0 = device order where it applies, 1 = the host replay (tests)
    int frame_order_used = 0;                    // what the last selection did: 1 = device order, 2 = host replay, 3 = device order overflowed -> host replay
    // addPointsToMap on the device: counters of the last insert, folded into num_voxels / num_points lazily (srl_map_settle)
    int *h_insert_cnt = nullptr;                 // pinned: [0] segments, [1] new voxels, [2] points added
    hipEvent_t ev_insert = nullptr, ev_world = nullptr;
    bool insert_pending = false;
    hipEvent_t ev_frame_read = nullptr;          // main stream: the last kernel reading d_frame_raw (the next upload, on the copy stream, waits for it)
    SrlEpochTable sel_table, ins_table;          // keypoint selection (with first-index words) / frame insertion

    // work buffers
    double *d_rec = nullptr;
    unsigned char *d_status = nullptr;
    double *d_partials = nullptr;
    SrlBlockInfo *d_binfo = nullptr;
    int work_cap = 0;                  // keypoints capacity of rec/status
    int block_cap = 0;
    SrlDevOut *d_out = nullptr;
    SrlDevOut *h_out = nullptr;        // pinned
    long long *d_count = nullptr;
    long long *h_count = nullptr;      // pinned
    unsigned long long *d_rec_granules = nullptr;   // fused ordered cut: 16 tagged granules per keypoint (the record), grown on demand
    size_t rec_granule_cap = 0;
    unsigned long long *d_granules = nullptr;   // published rows of the fused final reduction: 512 workgroups x 64 granules
    int force_kpw = 0, force_wpb = 0;  // srl_debug_set_launch_shape (0 = automatic)
    bool fuse_reduce = true;           // srl_debug_set_fused_reduce(0): always run the separate reduce kernel (A/B, tests)
    SrlMailbox *h_mail = nullptr;      // host-mapped fine-grained mailbox the reduce kernel publishes into
    unsigned long long seq = 0;

    // ARMED launches (srl_capi.cpp: arm_next / pose_box_write / srl_ctx_disarm): the kernel of the NEXT pass is enqueued while the
    // current one runs and waits, resident, for its pose
    int arm_mode = 1;                           // srl_set_armed_launch: 0 off, 1 on (armed where it is likely to fire: arm_wanted in srl_capi.cpp), 2 always
    int passes_in_solve = 0;                    // srl_build_residuals calls since the last srl_solve_end / sweep change
    int expected_passes = 0;                    // passes the previous solve took (0: unknown): no launch is armed behind the pass expected to be the
                                                // last one unless a prefetched sweep is waiting (the armed launch then becomes ITS first pass)
    int pose_box_kind = -1;                     // -1: not chosen yet (1 where possible); 0: pinned host memory, workgroup 0 relays into device memory; 1: fine-grained device memory the host writes through the PCIe BAR
    bool pose_box_dev_visible = false;
    unsigned long long *h_pose_box = nullptr;   // where the HOST writes the pose granules (kind 1: the CPU-visible device pointer)
    unsigned long long *pose_box_pinned = nullptr;   // kind 0 allocation (hipHostMalloc)
    unsigned long long *pose_box_dev = nullptr;      // kind 1 allocation (hipExtMallocWithFlags, fine-grained)
    unsigned long long *d_pose_relay = nullptr;
    SrlArmedLaunch armed;
    double arm_host_linger_us = 150.0;          // an armed launch older than this is cancelled, never fired (the kernel's own bound is longer)
    unsigned arm_linger_ticks = 30000u;         // 300 us of the 100 MHz clock: after that a waiting launch leaves by itself (a device-wide
                                                // synchronisation from outside this library waits that long at most)
    unsigned long long arm_stats[4] = {0, 0, 0, 0};   // armed, fired, cancelled, expired
    SrlProfRing prof;
    bool cur_measured = true;                   // light profiling: is the launch of the pass now running one of the timed ones ...
    unsigned cur_gen = 0;                       // ... and of which srl_timing_mark generation (an armed launch's: SrlArmedLaunch::measured, gen)
    long long *h_arm_stamps = nullptr;          // srl_debug_pass_stamps: 64 rows x 16 slots the armed kernels file (host-mapped)
    long long arm_host_stamps[64][4] = {};      // per pass (row seq & 63), steady-clock ns: call entry, pose written / launch returned, result seen, fired?

    // taps
    bool taps = false;
    int tap_cap = 0, tap_K = 0;
    int *d_tap_ids = nullptr;
    int *d_tap_ncand = nullptr;
    double *d_tap_normal = nullptr, *d_tap_a2d = nullptr, *d_tap_offset = nullptr;
    bool taps_valid = false;
    int last_K = 0;
    long long last_visited_local = -1;

    // comm
    int nranks = 1, rank = 0;
    ncclComm_t comm = nullptr;
    ncclComm_t parked_comm = nullptr;  // srl_comm_suspend: the communicator set aside while the context runs unsharded
    int parked_nranks = 0, parked_rank = 0;
    bool force_coll = false;           // env SRL_FORCE_COLLECTIVES=1: run the RCCL calls even with one rank (test hook)
    srl_allreduce_fn cb_ar = nullptr;
    srl_allgather_i64_fn cb_ag = nullptr;
    void *cb_user = nullptr;
    long long *d_gather = nullptr;     // nranks (capacity d_gather_cap: grow-only, see ensure_gather)
    size_t d_gather_cap = 0;
    // direct peer exchange (srl_peer_export / srl_peer_attach): the sharded sum without an RCCL call on the data path
    unsigned long long *d_inbox = nullptr;     // fine-grained device memory the peers store into (SRL_PEER_INBOX_GRANULES)
    SrlPeerTable *d_peer = nullptr;            // the table the kernels read (device copy)
    void *peer_mapped[SRL_MAX_PEERS] = {};     // HIP IPC mappings of the other ranks' inboxes (closed at detach)
    bool peer_on = false;
    int peer_seen = 0;                 // inboxes mapped at srl_peer_attach (srl_comm_info: equal to nranks when every rank's handle opened)
    bool peer_shares_device = false;   // a peer rank's inbox lives on THIS device (SRL_PEER_DEVICE_WORD): launches are not armed (arm_mode 1)
    bool comm_shares_device = false;   // ... the same for the RCCL transport (device identities all-gathered at srl_comm_init_rank)
    bool peer_failed = false;          // a row of this session never arrived: no further exchange until srl_peer_export + srl_peer_attach
    unsigned long long *peer_inbox[SRL_MAX_PEERS] = {};     // every rank's inbox as mapped into this process (host copy of SrlPeerTable::inbox)
    int peer_deadline_ms = 10000;      // srl_peer_set_deadline_ms: how long a pass keeps re-polling for a late rank's row before the session is given up
    unsigned long long peer_retries = 0;       // passes repeated because a row had not arrived within one kernel's bounded spin (srl_comm_info)
    unsigned long long peer_seq = 0;           // exchange counter: advances in lock-step on every rank
    SrlMailbox *d_mail = nullptr;              // device-side mailbox: where a FUSED pass leaves its rank's result for the RCCL all-reduce
    bool dbg_gather = false;           // srl_debug_set_gather_counts: d_gather is preloaded (no all-gather)

    // timing
    // scratch pool: device blocks handed out to the map-insert / frame pipeline calls and kept for the next call
    // (hipMalloc / hipFree per call cost more than the kernels they serve; hipFree also synchronises the device)
    struct PoolBlock { void *p; size_t bytes; };
    std::vector<PoolBlock> pool_free;

    int last_nblocks = 0;
    int profiling = 0;                 // 0 off, 1 full (4 events + sync per call), 2 light (assoc kernel only, read lazily: prof)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    srl_timing timing = {};
    int last_nb = 1;
};

#define HIPCHK(ctx, call)                                                                      \
    do {                                                                                       \
        hipError_t e__ = (call);                                                               \
        if (e__ != hipSuccess) {                                                               \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                   \
            return SRL_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)

// RCCL calls go through the run-time table: NCCLCHK(ctx, AllReduce(...)) = srl_rccl()->AllReduce(...)
#define NCCLCHK(ctx, call)                                                                     \
    do {                                                                                       \
        const SrlRccl *rc__ = srl_rccl();                                                      \
        if (!rc__) { (ctx)->err = srl_rccl_error(); return SRL_ERR_COMM; }                     \
        ncclResult_t r__ = rc__->call;                                                         \
        if (r__ != ncclSuccess) {                                                              \
            (ctx)->err = std::string(#call) + ": " + rc__->GetErrorString(r__);                \
            return SRL_ERR_COMM;                                                               \
        }                                                                                      \
    } while (0)

// cancel an armed launch, if any (every entry point that touches the stream or waits for it calls this first: an armed launch
// that nobody fires would hold the stream until its bound)
extern "C" int srl_ctx_disarm(srl_ctx *ctx);
#define SRL_DISARM(ctx) do { if ((ctx)->armed.on) { int rcd__ = srl_ctx_disarm(ctx); if (rcd__) return rcd__; } } while (0)
// frees the consensus workspace (srl_consensus.hip); srl_ctx_destroy calls it
extern "C" void srl_consensus_release(srl_ctx *ctx);
// frees the device point queue (srl_points.hip); srl_ctx_destroy calls it
extern "C" void srl_points_release(srl_ctx *ctx);
// frees the JPEG decoder (srl_jpeg.hip); srl_ctx_destroy calls it
extern "C" void srl_jpeg_release(srl_ctx *ctx);

// frame pipeline stage stamps (only while srl_debug_frame_timing is on): close stage `slot` here
#include <chrono>
inline void srl_stage_begin(srl_ctx *ctx) {
    if (!ctx->frame_timing) return;
    hipStreamSynchronize(ctx->stream);
    ctx->frame_stage_last_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
inline void srl_stage_end(srl_ctx *ctx, int slot) {
    if (!ctx->frame_timing) return;
    hipStreamSynchronize(ctx->stream);
    const long long now = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    ctx->frame_stage_us[slot] += (double)(now - ctx->frame_stage_last_ns) * 1e-3;
    ctx->frame_stage_last_ns = now;
}

// fold the counters of a deferred insert into the map's totals (every reader of num_voxels / num_points calls this first)
inline int srl_map_settle(srl_ctx *ctx) {
    if (!ctx->insert_pending) return SRL_OK;
    HIPCHK(ctx, hipEventSynchronize(ctx->ev_insert));
    ctx->num_voxels += ctx->h_insert_cnt[1];
    ctx->num_points += ctx->h_insert_cnt[2];
    ctx->insert_pending = false;
    return SRL_OK;
}

inline int ensure_copy_stream(srl_ctx *ctx) {
    if (!ctx->copy_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    return SRL_OK;
}
// the frame's raw points have just been read for the last time by what is enqueued so far
inline int srl_mark_frame_read(srl_ctx *ctx) {
    if (!ctx->ev_frame_read) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_frame_read, hipEventDisableTiming));
    HIPCHK(ctx, hipEventRecord(ctx->ev_frame_read, ctx->stream));
    return SRL_OK;
}

inline int ensure_frame_exchange(srl_ctx *ctx, size_t bytes) {
    if (!ctx->d_frame_sync) {
        HIPCHK(ctx, hipMalloc((void **)&ctx->d_frame_sync, 256));
        HIPCHK(ctx, hipMemsetAsync(ctx->d_frame_sync, 0, 256, ctx->stream));
    }
    if (bytes <= ctx->h_frame_x_bytes) return SRL_OK;
    if (ctx->h_frame_x) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // a gather may still be reading its index list out of the old block
        HIPCHK(ctx, hipHostFree(ctx->h_frame_x)); ctx->h_frame_x = nullptr; ctx->h_frame_x_bytes = 0;
    }
    const size_t cap = ((bytes + bytes / 2 + 4095) / 4096) * 4096;
    HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_frame_x, cap, hipHostMallocCoherent | hipHostMallocMapped));
    ctx->h_frame_x_bytes = cap;
    return SRL_OK;
}

inline int ensure_host_scratch(srl_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->h_scratch_bytes) return SRL_OK;
    if (ctx->h_scratch) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // a DMA out of the old block may still be queued (srl_frame_select_keypoints' index list)
        HIPCHK(ctx, hipHostFree(ctx->h_scratch)); ctx->h_scratch = nullptr; ctx->h_scratch_bytes = 0;
    }
    const size_t cap = ((bytes + bytes / 2 + 4095) / 4096) * 4096;
    HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_scratch, cap, hipHostMallocDefault));
    ctx->h_scratch_bytes = cap;
    return SRL_OK;
}

template <class T>
int ensure(srl_ctx *ctx, T *&p, size_t count) {
    if (p) { HIPCHK(ctx, hipFree(p)); p = nullptr; }
    if (count == 0) count = 1;
    HIPCHK(ctx, hipMalloc((void **)&p, count * sizeof(T)));
    return SRL_OK;
}
// ensure() frees first and allocates after: whoever grows blocks that share a capacity word sets the word to 0 before the first ensure
// and to the new value behind the last one -- a growth that fails half-way then leaves "nothing fits", never a null block that "fits".

inline int SrlSweepSlot::reserve(srl_ctx *ctx, double *&block, int &cap, int points) {
    if (points <= cap) return SRL_OK;
    const int grown = points > 1024 ? points : 1024;
    cap = 0;
    const int rc = ensure(ctx, block, (size_t)grown * 3);
    if (rc) return rc;
    cap = grown;
    return SRL_OK;
}

// A sweep is current from now on: its counts, the leading keypoints whose SoA planes are filled already (the others are transposed out of
// cur.stage by the first pass that reads them), and whether its tail may still be in flight (srl_sweep_swap only; cur_slot and
// cur_prefix_n say how far it has landed).  Everything a pass has learnt about the sweep before it is void: its taps, its neighbourhood
// bounds (a stale bound_n would cull against another sweep's distances: wrong neighbours, silently) and the solve's pass count.
// srl_sweep_upload, srl_sweep_swap and srl_frame_select_keypoints call it; the three reset the same words.
inline void srl_sweep_becomes_current(srl_ctx *ctx, int n, int begin, int total, int soa_valid_n, bool tail_pending) {
    ctx->cur.n = n; ctx->cur.begin = begin; ctx->cur.total = total;
    ctx->sweep_loaded = true;
    ctx->soa_valid_n = soa_valid_n;
    ctx->tail_pending = tail_pending;
    ctx->taps_valid = false;
    ctx->bound_n = 0;
    ctx->passes_in_solve = 0;
}

// The per-rank counts of the ordered cut.  Grow-only and never re-allocated for a size that fits: hipFree waits for the WHOLE
// device, and a second rank of the same process may already sit in a pass that waits for THIS rank's row (a second peer
// session on live contexts: its attach used to free + re-allocate here and stalled until the peer's bounded spin gave up).
inline int ensure_gather(srl_ctx *ctx, size_t nranks) {
    if (ctx->d_gather && nranks <= ctx->d_gather_cap) return SRL_OK;
    const size_t cap = nranks < 64 ? 64 : nranks;
    int rc = ensure(ctx, ctx->d_gather, cap);
    if (rc) { ctx->d_gather_cap = 0; return rc; }
    ctx->d_gather_cap = cap;
    return SRL_OK;
}

// RAII scratch block from the context's pool (best fit, grow-only; everything is released by srl_ctx_destroy)
struct DevBuf {
    srl_ctx *ctx = nullptr;
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p && ctx) ctx->pool_free.push_back({p, bytes}); else if (p) hipFree(p); }
    hipError_t alloc(srl_ctx *c, size_t want) {
        ctx = c;
        if (want < 256) want = 256;
        int best = -1;
        for (int i = 0; i < (int)c->pool_free.size(); i++)
            if (c->pool_free[i].bytes >= want && (best < 0 || c->pool_free[i].bytes < c->pool_free[best].bytes)) best = i;
        if (best >= 0 && c->pool_free[best].bytes <= 4 * want + (1u << 20)) {
            p = c->pool_free[best].p; bytes = c->pool_free[best].bytes;
            c->pool_free.erase(c->pool_free.begin() + best);
            return hipSuccess;
        }
        const size_t cap = ((want + want / 4 + 255) / 256) * 256;
        hipError_t e = hipMalloc(&p, cap);
        bytes = (e == hipSuccess) ? cap : 0;
        return e;
    }
    template <class T> T *as() { return reinterpret_cast<T *>(p); }
};

// An uploaded image's two blocks: page-locked staging (h) and its place on the device (d), both grow-only.  Whoever uploads waits until
// the staging block is free again before the next upload -- by ending its call synchronised, or behind an event of its own.
struct SrlImagePair {
    unsigned char *h = nullptr, *d = nullptr;
    size_t h_cap = 0, d_cap = 0;
    int reserve(srl_ctx *ctx, size_t host_bytes, size_t device_bytes) {
        if (host_bytes > h_cap) {
            if (h) { HIPCHK(ctx, hipHostFree(h)); h = nullptr; h_cap = 0; }
            HIPCHK(ctx, hipHostMalloc((void **)&h, host_bytes, hipHostMallocDefault));
            h_cap = host_bytes;
        }
        if (device_bytes > d_cap) {
            if (d) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); HIPCHK(ctx, hipFree(d)); d = nullptr; d_cap = 0; }
            HIPCHK(ctx, hipMalloc((void **)&d, device_bytes));
            d_cap = device_bytes;
        }
        return SRL_OK;
    }
    // the caller's rows packed into h, and the DMA from there enqueued on the context's stream
    int upload(srl_ctx *ctx, const uint8_t *src, int rows, size_t row_bytes, int64_t stride) {
        srl_pack_rows(h, src, (size_t)rows, row_bytes, (size_t)stride);
        HIPCHK(ctx, hipMemcpyAsync(d, h, (size_t)rows * row_bytes, hipMemcpyHostToDevice, ctx->stream));
        return SRL_OK;
    }
    void release() { if (h) hipHostFree(h); if (d) hipFree(d); *this = SrlImagePair(); }
};

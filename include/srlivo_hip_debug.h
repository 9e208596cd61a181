/*
 * srlivo_hip_debug.h -- debug, parity and tuning hooks of libsrlivo_hip.so (srl_debug_*).
 *
 * Kept apart from the product ABI (srlivo_hip.h): nothing on the product path -- the host mirror, integration/optimize_hip.cpp, a node
 * that links the library -- calls any of these.  They exist for tests/, tools/ and bench.py's A/B legs: switching parts of the kernel
 * off, forcing selection paths and launch shapes, reading time lines.  Same conventions as srlivo_hip.h.
 */
#ifndef SRLIVO_HIP_DEBUG_H
#define SRLIVO_HIP_DEBUG_H

#include "srlivo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Selection path of srl_build_residuals on this context (until round 4 a field of srl_icp_opts; that struct now holds the fields of the
 * reference's icpOptions only): 0 = automatic (the default); 1 streaming extraction, 2 general two-pass, 3 FP64-retained fast path,
 * 4 Jacobi eigen-solver in phase 2, 5 heap replay (the reference's literal priority_queue sequence) for every keypoint. */
int srl_debug_set_select_mode(srl_ctx *ctx, int select_mode);

/* Where srl_frame_select_keypoints orders the keypoints (the iteration order of gridSampling's std::tr1::unordered_map,
 * utility.cpp:167-201): 0 = on the device where it applies (the default: frames whose bucket table fits one scan launch), 1 = always the
 * host replay of csrc/host/tr1_order.h (what rounds 3-4 shipped; still the path of larger frames and of a bucket with more than 16 voxels).
 * srl_debug_frame_order_used: what the last selection did -- 1 device order, 2 host replay, 3 device order found an overfull bucket and
 * the host replay ran behind it.  Both orders are the same permutation (tests/test_gpu_frame_order.py). */
/* The frame path's own stable sort of (key, position) pairs over the low `bits` (1..18) key bits, n <= 131072 (two one-launch radix
 * passes, csrc/srl_frame_scratch.h; what srl_frame_commit's addPointsToMap groups a frame's points with) on caller data: keys_sorted and
 * positions_sorted (the position 0..n-1 each key came from) as a stable sort by (key & ((1 << bits) - 1)) would leave them. */
int srl_debug_radix_sort_pairs(srl_ctx *ctx, const uint32_t *keys, int n, int bits, uint32_t *keys_sorted, uint32_t *positions_sorted);

/* How often the colour map (srl_color_map_*) has rebuilt its voxel table / its grid set since it was created: both grow by rebuild
 * (tests make sure a long run crosses several). */
int srl_debug_color_map_rebuilds(srl_ctx *ctx, int32_t *voxel_table, int32_t *grid_table);

int srl_debug_set_frame_order_mode(srl_ctx *ctx, int mode);
int srl_debug_frame_order_used(srl_ctx *ctx, int *used);

/* test hook for the ON-DEVICE budget derivation of the sharded ordered cut (optimize.cpp:107 across ordered shards): the
 * context acts as rank `rank` of `nranks` whose on-stream all-gather of per-rank counts (accepted residuals; keypoints with a
 * plane when max_num_residuals <= 0) has already delivered `counts`; the all-reduce is the identity, so srl_build_residuals
 * returns THIS rank's contribution.  Lets one GPU exercise the reduce kernel's rank > 0 branches, which a 1-rank communicator
 * cannot reach; the same result must come out of the host-side srl_shard_budget path (srl_comm_set_host_callbacks).
 * counts = NULL switches the hook off.  Upload the sweep after switching (the shard range changes). */
int srl_debug_set_gather_counts(srl_ctx *ctx, int nranks, int rank, const int64_t *counts);

/* srl_debug_set_ablate: bit mask that switches parts of the association kernel off (profiling tools only; results are
 *   wrong while it is set).  Replaces the SRL_ABLATE environment variable of round 1 -- the library reads no environment
 *   variable on the per-iteration path.  The switches live in ONE extra instantiation of the kernel (r = 1 fast path, 16 x 16
 *   keypoints per workgroup); while the mask is non-zero every pass is launched in that shape, whatever the sweep size.  The
 *   production instantiations carry no trace of them.
 * srl_debug_set_search_select_mode: selection path used by srl_search_neighbors (0 default, 1 extraction, 5 heap replay).
 * srl_debug_heap_topk: the device kernels' restatement of libstdc++'s push_heap / pop_heap (csrc/srl_heap.h, the
 *   std::priority_queue of optimize.cpp:355-363,394-404,411-422) run on the host: offers distances[0..n) in order to a
 *   bounded max-heap of K, writes the read-out order (candidate indices, ascending distance) and returns its size.  No GPU.
 * srl_debug_device_sqrt: out[i] = the device's sqrt(in[i]) (the tie replay relies on it being correctly rounded). */
int srl_debug_set_ablate(srl_ctx *ctx, int bits);
/* 0: always run the separate ordered-cut / reduce kernel.  Default 1: on an unsharded context without taps the last workgroup
 * of the association kernel sums the published rows and writes the normal equations itself (one kernel per ESIKF iteration)
 * -- also WITH the ordered cut of a finite max_num_residuals when the pass runs in workgroups of <= 64 keypoints (the
 * prefix pass of the shipped 600).  A finisher that gives up waiting for a row (bounded spin) makes srl_build_residuals repeat
 * the pass once with the separate reduce kernel instead of failing. */
int srl_debug_set_fused_reduce(srl_ctx *ctx, int enable);
/* Neighbourhood bounds (default on): every pass leaves, per keypoint, its world position and the exact squared distance of its K-th
 * nearest neighbour; the next pass over the same sweep and map does not visit voxels that lie further from the keypoint than
 * sqrt(tau) + |movement| -- the same neighbours (searchNeighbors, optimize.cpp:365-426, keeps the K nearest whatever else it looked at),
 * fewer candidates evaluated.  Where a keypoint's bound holds, that squared radius is also an upper bound of the K-th smallest FP32
 * prefilter distance, so the prefilter takes its survivor threshold from it and searches for none.
 * mode 1 (default): both.  2: the voxel cull only, every threshold searched.  0: the bounds are not used at all.  (A/B in the tests:
 * every bit must agree between the three.)  Other values: SRL_ERR_BAD_ARG. */
int srl_debug_set_bound_culling(srl_ctx *ctx, int mode);
/* Neighbour records (default on): the map keeps, per voxel, what the 27 lookups around it return (slab and count of every neighbour
 * voxel, or "none"), brought up to date by whatever edits the map.  A pass of the r = 1 fast path looks only a keypoint's HOME voxel
 * up in the table and takes the 27 answers from that voxel's record; keypoints whose home voxel is not in the map, r = 2 and the general
 * path look every voxel up as before.  enable 0: no pass reads the records (every pair of the fast path takes the table lookups); the
 * map still maintains them, and the table request of such a pair is issued when the pair is consumed, not a pair ahead -- a switch for
 * equality tests, not a timing baseline.  Every bit of a pass must agree between 0 and 1.  Other values: SRL_ERR_BAD_ARG. */
int srl_debug_set_neighbour_records(srl_ctx *ctx, int enable);
/* srl_debug_neighbour_records_download: the records of the map's voxels, 32 words each, in slab order (the order of srl_map_download):
 * word (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1) = slab << 5 | count of the voxel at key + (dx, dy, dz) (16-bit wrap), 0xFFFFFFFF = none,
 * words 27 .. 31 zero.  max_voxels < the map's voxels: SRL_ERR_BAD_ARG. */
int srl_debug_neighbour_records_download(srl_ctx *ctx, uint32_t *words, int max_voxels);
/* The neighbourhood bounds the last pass left: *num_keypoints entries {x, y, z, tau} (0 after anything that voids them), the first
 * max_keypoints >= that many floats x 4 of `bounds` filled.  Cancels a waiting launch. */
int srl_debug_bounds_download(srl_ctx *ctx, float *bounds, int max_keypoints, int *num_keypoints);
/* Where the pose box of the armed launches lives.  kind 1: fine-grained DEVICE memory the host writes through the PCIe BAR (every
 * workgroup polls it locally; SRL_ERR_UNSUPPORTED when device memory is not CPU-visible on this system).  kind 0: page-locked host
 * memory -- workgroup 0 of the waiting kernel polls it across PCIe and republishes the pose into device memory for the other
 * workgroups (~0.7 us per pass slower).  kind -1 (the default): 1 where possible, else 0.
 * srl_debug_set_arm_linger: the age (us) beyond which a call cancels an armed launch instead of firing it (default 150), and the
 * kernel-side bound (us, default 300) after which a waiting launch leaves by itself -- tests drive both paths with it. */
int srl_debug_set_pose_box(srl_ctx *ctx, int kind);
int srl_debug_set_arm_linger(srl_ctx *ctx, double host_linger_us, double kernel_linger_us);
/* Time line of the armed passes (tools/arm_timeline.py): enable allocates a host-mapped stamp buffer the armed kernels file into
 * (kernels built with -DSRL_ARM_STAMPS only: the product build has no stamp sites and leaves the buffer at zero);
 * gpu_out[64 * 32] (optional): per pass (row = sequence number & 63) the 100 MHz device clock at {entry, pose received, tile start,
 * phase 0 / 1 / 2 done, row published, finisher done} of workgroup 0 (slots 0..7) and of the finishing workgroup (8..15), slots
 * 16..24 inside the finisher and phase 2 (-DSRL_STAMP_DETAIL);
 * host_out[64 * 4] (optional): steady-clock ns at {call entry, pose written or launch returned, result seen} and a fired flag. */
int srl_debug_pass_stamps(srl_ctx *ctx, int enable, long long *gpu_out, long long *host_out);
/* Stage times of the frame pipeline (bench.py's `pipeline` leg, tools/pipeline_probe.py).  While enabled the stream is synchronised at
 * every stage boundary and the wall time of each stage is ACCUMULATED in us; out16 (optional) receives the sums since the last call,
 * which also clears them: [0] srl_frame_upload; srl_frame_select_keypoints: [1] grouping kernels (transform, voxel key, first point per
 * voxel), [2] download of the voxel list, [3] host: std::tr1::unordered_map iteration order, [4] gather into the resident sweep;
 * srl_frame_commit: [5] re-transform, [6] download of point3D::point; the map insertion behind it (also srl_map_insert): [7] keys +
 * (key, index) sort, [8] segments, [9] lookup + creation of new voxels, [10] per-voxel replay + counters. */
int srl_debug_frame_timing(srl_ctx *ctx, int enable, double out16[16]);
/* The scratch hash tables of the frame pipeline are never cleared per frame: entries carry a 16-bit epoch (csrc/srl_frame_scratch.h) and
 * the tables are cleared when it wraps, every 65 535 frames (1.8 h of a 10 Hz sensor).  Test hook: set the epoch counters of both tables so
 * that the wrap happens `frames_to_wrap` frames from now. */
int srl_debug_set_frame_epoch(srl_ctx *ctx, int frames_to_wrap);
/* The 32-bit companions of the same tables wrap as well: the selection's table and the insertion's carry a call counter (1 ... 0xFFFFFFFE; the
 * selection's first-index words hold 0xFFFFFFFF - counter) and are cleared when it wraps, and the seen words of srl_frame_subsample carry a
 * tag (1 ... 0xFFFFFFFF) and are cleared when that wraps.  srl_debug_set_frame_counters moves all three forward so that each owner's next
 * `calls_to_wrap` calls use its last `calls_to_wrap` values and the call after them wraps (the selection's table is opened once by every
 * srl_frame_subsample AND once by every srl_frame_select_keypoints; the seen words take a tag in every srl_frame_subsample AND in every
 * srl_frame_take_subsampled of m > 0 points).  It synchronises the stream first and only moves forward
 * (SRL_ERR_BAD_ARG otherwise, and nothing is changed): what the tables hold stays stale.  srl_frame_subsample sets its tag back to 0 when its
 * buffers grow, so apply the hook after a sub-sample of the largest sweep of the run has allocated them.
 * srl_debug_frame_counters: out = {counter of the selection's table, counter of the insertion's table, tag of the seen words} as the last
 * calls left them. */
int srl_debug_set_frame_counters(srl_ctx *ctx, int calls_to_wrap);
int srl_debug_frame_counters(srl_ctx *ctx, uint32_t out[3]);
/* The colour map keeps five structures of the same kind: the insertion's scratch table (srl_color_map_insert), the
 * selection's image cells with their two companion arrays (srl_color_map_select), the tracker's pool-position and image-cell tables (one
 * srl_color_map_track_update opens both) and the render's mark words (srl_color_map_render).  Each table carries a 16-bit epoch
 * (1 ... 0xFFFF) and a 32-bit call counter (1 ... 0xFFFFFFFE; companion words hold 0xFFFFFFFF - counter), the mark words the 16-bit render
 * epoch; a structure is cleared when its number wraps to 1.
 * srl_debug_color_epochs: out = { [0] scratch epoch, [1] selection epoch, [2] tracker pool epoch, [3] tracker cell epoch,
 *                                 [4] selection counter, [5] tracker pool counter, [6] tracker cell counter, [7] scratch counter,
 *                                 [8] render epoch } as the last calls left them (0: never used).  SRL_ERR_NO_MAP without a colour map.
 * srl_debug_set_color_epochs: -1 leaves a family alone; a value k >= 0 moves every number of the family forward so that the next k calls of
 * each owner use the last k values and call k + 1 wraps -- calls_to_epoch_wrap (<= 0xFFFF): the four epochs and the render epoch,
 * calls_to_counter_wrap: the four counters.  It synchronises the stream first and only moves forward (entries written so far then stay
 * stale: a larger counter is a smaller companion tag, and the smaller tag wins atomicMin); if any number would move backward it returns
 * SRL_ERR_BAD_ARG and changes nothing. */
int srl_debug_color_epochs(srl_ctx *ctx, uint32_t out[9]);
int srl_debug_set_color_epochs(srl_ctx *ctx, int calls_to_epoch_wrap, int calls_to_counter_wrap);
/* tuning experiments: force the association kernel's launch shape -- keypoints per wave (16-wave workgroups: 2 / 3 / 4 / 6 / 8 /
 * 12 / 16; 4-wave workgroups: 4 / 8 / 16) and waves per workgroup (4 / 16); 0, 0 = automatic (by sweep size).  Results do not
 * depend on the shape beyond FP64 summation order. */
int srl_debug_set_launch_shape(srl_ctx *ctx, int keypoints_per_wave, int waves_per_workgroup);
int srl_debug_set_search_select_mode(srl_ctx *ctx, int select_mode);
int srl_debug_heap_topk(const double *distances, int n, int K, int32_t *out_index);
int srl_debug_device_sqrt(srl_ctx *ctx, const double *in, int n, double *out);
/* debug (srl_debug_set_ablate(ctx, 128)): {start, end, xcc id} stamps of every workgroup of the last association launch, in ticks of
 * the 100 MHz wall clock; out = max_blocks x 3 doubles.  Used by tools/block_times.py. */
int srl_debug_block_times(srl_ctx *ctx, double *out, int max_blocks, int *nblocks);
/* parity tests of the optical flow (srl_flow_track_image): the level count L as lowered by the size rule, and one padded level of
 * either pyramid set as it is AFTER the last call's swap -- SRL_FLOW_PREV: the image given last, SRL_FLOW_CUR: the one before it (zeros
 * until a second image has been given).  image_padded: (rows + 42) x (cols + 42) bytes, deriv_padded: as many int16 pairs (Ix, Iy);
 * either may be NULL.  *rows, *cols: the level's size.  level > L: SRL_ERR_BAD_ARG; no image yet: SRL_ERR_NO_SWEEP. */
enum { SRL_FLOW_PREV = 0, SRL_FLOW_CUR = 1 };
int srl_flow_levels(srl_ctx *ctx, int *L);
int srl_flow_download_level(srl_ctx *ctx, int which, int level, uint8_t *image_padded, int16_t *deriv_padded, int *rows, int *cols);
/* parity tests of the image preparation (srl_image_prepare): one intermediate stage of the last image.  UNDIST: rows x cols x 3 bytes;
 * GRAY: rows x cols; YCRCB: the Y plane (rows x cols) followed by the (Cr, Cb) pairs (rows x cols x 2), as the device holds them;
 * LUT_GRAY, LUT_Y: T x T x 256 bytes, [ty][tx][value].  capacity: bytes of out (SRL_ERR_BAD_ARG when the stage is larger, as for a NULL
 * argument or an unknown stage); no preparer: SRL_ERR_NO_MAP; no image yet: SRL_ERR_NO_SWEEP. */
enum { SRL_PREP_STAGE_UNDIST = 0, SRL_PREP_STAGE_GRAY = 1, SRL_PREP_STAGE_YCRCB = 2, SRL_PREP_STAGE_LUT_GRAY = 3, SRL_PREP_STAGE_LUT_Y = 4 };
int srl_image_prep_download_stage(srl_ctx *ctx, int stage, uint8_t *out, int64_t capacity);
/* parity tests of the resize (srl_image_prepare_resized): the frame the last image's remap read, rows x cols x 3 bytes of the preparer's
 * size -- the resized frame, or the uploaded one where no resize ran (behind srl_image_prepare_jpeg with a frame of the preparer's size:
 * the decoded frame where it lies; SRL_ERR_NO_SWEEP once a later srl_jpeg_decode has replaced it).  capacity, refusals: as above. */
int srl_image_prep_download_resized(srl_ctx *ctx, uint8_t *out, int64_t capacity);
/* known-answer tests of the JPEG decode's IDCT (srl_jpeg_decode, operation (i)) on blocks no encoder produces: n_blocks blocks of 64
 * quantised coefficients in natural order, one table in natural order, out: 64 samples per block, row-major.  The 32-bit form runs iff
 * the largest block sum of |coef qt| is at most 14000, the 64-bit form otherwise, as for a frame.  Synchronous; cancels an armed launch.
 * SRL_ERR_BAD_ARG: NULL arguments, n_blocks < 1 or > 2^20; more than one rank: SRL_ERR_UNSUPPORTED. */
int srl_jpeg_idct_blocks(srl_ctx *ctx, const int16_t *coef, int64_t n_blocks, const uint16_t qt[64], uint8_t *out);
/* tests of the consensus estimators (srl_consensus_fundamental, srl_consensus_pnp) on EVERY hypothesis: what this context's last call that
 * ran on the device (n >= 8 / n >= 4, not refused) left in the workspace.  Synchronous; cancels an armed launch.
 * info: model = SRL_CONSENSUS_FUNDAMENTAL / _PNP, hypotheses = H, n, slots = 3 / 4, usable = the number of usable points, norm = Hartley's
 *   normalisation mx1, my1, s1, mx2, my2, s2 of the two views (fundamental; six zeros after a PnP call);
 * usable[0 .. info->usable): the usable points, ascending (the rest of the array is left alone);
 * samples: H x 8, each hypothesis' sample indices padded with -1 (all -1: no sample);
 * models: H x slots x 12 doubles as srl_consensus_result.model holds the winner's, twelve zeros where a slot has no model;
 * counts: H x slots, each model's inlier count, -1 where a slot has no model.
 * point_capacity, hypothesis_capacity: the entries of usable, and the hypotheses samples, models and counts have room for.
 * SRL_ERR_BAD_ARG: a NULL argument, point_capacity < n or hypothesis_capacity < H; SRL_ERR_NO_MAP: no workspace yet, or no such call. */
typedef struct srl_debug_consensus_info { int32_t model, hypotheses, n, slots, usable, reserved; double norm[6]; } srl_debug_consensus_info;
int srl_debug_consensus_download(srl_ctx *ctx, srl_debug_consensus_info *info, int32_t *usable, int64_t point_capacity, int32_t *samples,
                                 double *models, int32_t *counts, int64_t hypothesis_capacity);

/* Read-backs of the device point queue (csrc/srl_points.hip), for tests and for a caller's own fallback.  Each array is optional; *n (may
 * be NULL) receives the record count, and nothing is copied when capacity < count (SRL_ERR_BAD_ARG, *n set: ask again).
 * srl_points_queue_download: the queue front to back -- raw_point (n x 3), relative_time (ms within its message), timestamp.
 * srl_points_cut_download: the resident cut of the last srl_points_cut, same records (relative_time is still the message's: the rewrite
 *   belongs to srl_frame_undistort_cut).  SRL_ERR_NO_SWEEP without a queue / a cut.
 * srl_debug_points_fallbacks: how often srl_frame_undistort_cut replayed the IMU interval walk on the host because the rewritten times of
 *   the cut or the state stamps were not non-decreasing. */
int srl_points_queue_download(srl_ctx *ctx, double *raw_xyz, double *relative_time, double *timestamp, int capacity, int *n);
int srl_points_cut_download(srl_ctx *ctx, double *raw_xyz, double *relative_time, double *timestamp, int capacity, int *n);
int srl_debug_points_fallbacks(srl_ctx *ctx, int64_t *count);
/* The undistorted sweep as srl_frame_undistort or srl_frame_undistort_cut left it in HBM, all n points (each array optional, capacity as
 * above): the uncorrected points (what srl_frame_subsample keys on), imu_point, the corrected raw_point, and the IMU interval of every
 * point (-1: the walk never reached it; meaningful after a call in SRL_MC_IMU mode only). */
int srl_debug_undistorted_download(srl_ctx *ctx, double *uncorrected_xyz, double *imu_point, double *corrected_xyz, int32_t *interval, int capacity,
                                   int *n);

#ifdef __cplusplus
}
#endif
#endif

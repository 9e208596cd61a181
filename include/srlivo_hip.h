/*
 * srlivo_hip.h -- C-ABI of libsrlivo_hip.so: the MI355X (gfx950) implementation of SR-LIVO's LIO
 * scan-matching hot path (reference: ZikangYuan/sr_livo, src/optimize.cpp).
 *
 * The reference has no FFI/plugin API for this path: it sits behind member functions of
 * `class lioOptimization` (include/lioOptimization.h:334-357).  Each entry point below names the
 * reference interface it replaces (paths relative to the reference root).  The C++ host mirror that
 * keeps the reference's class surfaces (lioOptimization / eskfEstimator / cloudMap types) lives in
 * sr_livo_amd/csrc/host/ and forwards to this ABI; INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions: plain pointers and sizes, caller-owned HOST buffers unless a parameter says
 * "device"; all floating point is FP64 except stored map positions (FP32, cloudMap.h:54) and voxel
 * keys (int16, cloudMap.h:124-145); matrices ROW-MAJOR; quaternions (w,x,y,z).  Every function
 * returns SRL_OK (0) or a negative srl_status; no exceptions cross the ABI.  There is NO CPU
 * fallback: without a HIP device srl_ctx_create fails with SRL_ERR_NO_DEVICE.
 */
#ifndef SRLIVO_HIP_H
#define SRLIVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRL_VOXEL_CAP 20        /* max_num_points_in_voxel of the LIO map (config/r3live.yaml:50, ntu.yaml:49) */
#define SRL_MAX_NEIGHBORS 32    /* upper bound supported for icpOptions::max_number_neighbors (shipped: 20) */

typedef enum srl_status {
    SRL_OK = 0,
    SRL_ERR_NO_DEVICE = -1,     /* no HIP device / HIP runtime failure at create */
    SRL_ERR_HIP = -2,           /* a HIP call failed (see srl_last_error) */
    SRL_ERR_BAD_ARG = -3,
    SRL_ERR_UNSUPPORTED = -4,   /* option outside the supported envelope (cap != 20, K > 32, nb_voxels < 1 or > 2) */
    SRL_ERR_NO_MAP = -5,
    SRL_ERR_NO_SWEEP = -6,
    SRL_ERR_COMM = -7,          /* RCCL failure */
    SRL_ERR_NAN_PLANARITY = -8, /* optimize.cpp:348-350: a2D is NaN -> the reference throws std::runtime_error("error") */
    SRL_ERR_NOT_ENOUGH_RESIDUALS = -9  /* optimize.cpp:110-123: summary.success = false */
} srl_status;

typedef struct srl_ctx srl_ctx;

/* the fields of icpOptions the path reads (include/parameters.h:8-56) -- those and nothing else */
typedef struct srl_icp_opts {
    int32_t threshold_voxel_occupancy;  /* parameters.h:13 */
    int32_t init_num_frames;            /* parameters.h:15 */
    double  size_voxel_map;             /* parameters.h:17 */
    int32_t num_iters_icp;              /* parameters.h:19 */
    int32_t min_number_neighbors;       /* parameters.h:21 */
    int32_t voxel_neighborhood;         /* parameters.h:23 */
    double  power_planarity;            /* parameters.h:25 */
    int32_t max_number_neighbors;       /* parameters.h:30 */
    double  max_dist_to_plane_icp;      /* parameters.h:32 */
    double  threshold_orientation_norm; /* parameters.h:34 */
    double  threshold_translation_norm; /* parameters.h:36 */
    int32_t max_num_residuals;          /* parameters.h:40 */
    double  weight_alpha;               /* parameters.h:46 */
    double  weight_neighborhood;        /* parameters.h:48 */
} srl_icp_opts;

/* per-iteration pose + frame constants read by buildPlaneResiduals (optimize.cpp:21-28,83) */
typedef struct srl_frame {
    double  q[4];        /* p_frame->p_state->rotation (w,x,y,z), NOT normalised by the caller */
    double  t[3];        /* p_frame->p_state->translation */
    double  t_last[3];   /* all_cloud_frame[id-1]->p_state->translation (optimize.cpp:25) */
    double  R_il[9];     /* R_imu_lidar (lioOptimization.h:227) */
    double  t_il[3];     /* t_imu_lidar (lioOptimization.h:228) */
    int32_t frame_id;    /* p_frame->frame_id (selects init mode, optimize.cpp:21-23) */
} srl_frame;

/* what one buildPlaneResiduals pass hands to updateIEKF (optimize.cpp:160-170,235,239) */
typedef struct srl_normal_eq {
    double  HtH[36];         /* H_x^T H_x, 6x6 row-major */
    double  Hth[6];          /* H_x^T h */
    double  loss_sum;        /* sum of distance^2 over accepted residuals (optimize.cpp:104) */
    int32_t num_residuals;   /* optimizeSummary.num_residuals_used */
    int32_t success;         /* optimizeSummary.success (optimize.cpp:110) */
    int64_t sum_candidates;  /* sum over keypoints of resident points visited (P_k), whole sweep */
    int64_t last_visited;    /* global index of the last keypoint the sequential loop would visit (cut-off) */
    int32_t nan_error;       /* 1 if a NaN planarity was met among visited keypoints */
    int32_t num_fallback;    /* keypoints that took the streaming-extraction selection path */
} srl_normal_eq;

/* ------------------------------------------------------------------ context */
int         srl_device_count(int *count);
int         srl_ctx_create(int device, srl_ctx **out);
int         srl_ctx_destroy(srl_ctx *ctx);
const char *srl_last_error(const srl_ctx *ctx);      /* text of the last failure on this context */
const char *srl_status_str(int status);
void        srl_icp_opts_default(srl_icp_opts *o);   /* effective values of config/r3live.yaml:57-69 */

/* ------------------------------------------------------------------ voxel map
 * replaces: voxelHashMap voxel_map (lioOptimization.h:274; cloudMap.h:171 tsl::robin_map<voxel, voxelBlock>).
 * srl_map_upload installs a map built elsewhere (voxels in creation order; point id = voxel*cap + slot). */
int srl_map_upload(srl_ctx *ctx, const int16_t *keys_xyz /* V x 3 */, const int32_t *counts /* V */,
                   const float *xyz /* V x cap x 3, AoS */, int num_voxels, int cap);
/* replaces lioOptimization::addPointsToMap / addPointToMap (lioOptimization.cpp:520-554, 400-446):
 * order-dependent insert of world points (AoS n x 3, FP64) into the device-resident map. */
int srl_map_insert(srl_ctx *ctx, const double *world_xyz, int n, double voxel_size, int cap,
                   double min_distance_points, int min_num_points, int *num_added);
/* The same insertion, reporting what it stored: what addPointToMap hands to addPointToPcl (lioOptimization.cpp:428-429, 1346-1355) and
 * addPointsToMap publishes as cloud_world (:552-553).  outcome[i] (n bytes, batch order): 0 = not stored (voxel full, closer than
 * min_distance_points to a resident, min_num_points not met, or no voxel and min_num_points > 0), 1 = appended to a voxel that existed
 * when the point's turn came (one created by an EARLIER point of the batch included), 2 = created its voxel.  cloud (capacity n): the
 * points with outcome 1 in ascending batch index -- voxel creators are stored but not published, as in the reference -- with x, y, z the
 * FP32 position the map holds and intensity = (float)(50.0 * ((double)z - ref_z)), ref_z = p_frame->p_state->translation.z().
 * count(outcome != 0) == *num_added.  outcome, cloud, num_cloud and num_added are each optional.  The map ends up exactly as after
 * srl_map_insert, every n srl_map_insert accepts is accepted (SRL_MAP_INSERT_REPORT_MAX_POINTS), and like it the call cancels an armed
 * launch, folds a deferred insert in first and voids the neighbourhood bounds.  Always synchronous: it waits for the device once (the
 * record count) and then moves num_cloud records in one DMA.  NULL ctx or NULL points with n > 0: SRL_ERR_BAD_ARG with both counts
 * written as 0, before any device is touched; cap != 20: SRL_ERR_UNSUPPORTED; n == 0: SRL_OK, counts 0.  With a communicator the call
 * acts on this rank's map as srl_map_insert does (the map is replicated: every rank inserts the same batch); tests/test_gpu_sharded_stream.py takes three ranks through insertions, a
 * prune and passes in between and holds outcome, cloud, counts, map and checksum bytewise equal on every rank and to an unsharded context. */
typedef struct srl_cloud_point { float x, y, z, intensity; } srl_cloud_point;   /* the payload of pcl::PointXYZI */
#define SRL_MAP_INSERT_REPORT_MAX_POINTS 2147483647      /* no limit of its own: INT_MAX, as srl_map_insert */
int srl_map_insert_report(srl_ctx *ctx, const double *world_xyz, int n, double voxel_size, int cap,
                          double min_distance_points, int min_num_points, double ref_z,
                          uint8_t *outcome /* n or NULL */, srl_cloud_point *cloud /* capacity n, or NULL */,
                          int *num_cloud /* or NULL */, int *num_added /* or NULL */);
/* replaces lioOptimization::mapSize (lioOptimization.cpp:574-581) */
int srl_map_size(srl_ctx *ctx, int64_t *num_points, int32_t *num_voxels);
/* copies the device map back in creation order (same layout as srl_map_upload) */
int srl_map_download(srl_ctx *ctx, int16_t *keys_xyz, int32_t *counts, float *xyz, int max_voxels);
/* replaces lioOptimization::removePointsFarFromLocation (lioOptimization.cpp:556-572): erases every voxel whose FIRST stored point
 * (slot 0, FP32) p0 satisfies ((dx*dx + dy*dy) + dz*dz) > distance*distance with d = (double)p0 - location, all FP64 (a negative distance
 * acts like its absolute value; +inf or a NaN distance / location erases nothing).  The survivors are RENUMBERED: slab index = rank
 * among the surviving voxels in creation order (point id = slab * 20 + slot, as on a map rebuilt from them), and voxels created later
 * go behind them; a key that was erased and is hit again by an insert becomes a new voxel at the end.  Cancels an armed launch, folds a
 * deferred insert in first, voids the neighbourhood bounds and the taps of the last pass, and waits for the device once (the counts).
 * No map, or an empty one: SRL_OK with nothing removed.  Both counts are optional. */
int srl_map_remove_far(srl_ctx *ctx, const double location[3], double distance, int32_t *num_voxels_removed, int64_t *num_points_removed);
/* A cheap fingerprint of the part of the map a set of points falls into -- what a caller that keeps a map of its OWN (the node's
 * tsl::robin_map, lioOptimization.h:274) compares frame by frame instead of walking both maps: for every point the voxel it belongs to
 * (key = short(float(p) / voxel_size), lioOptimization.cpp:403-405) contributes srl_probe_mix(key, points in the voxel, position of the
 * voxel's LAST stored point); a point without a voxel contributes 0; the checksum is the sum modulo 2^64 (points of one voxel count
 * once each: no deduplication on either side).  world_xyz = host points (n x 3), or NULL: the world points the last srl_frame_commit
 * left in HBM (n is then ignored; the empty sum when a newer frame has been uploaded since).  stride >= 1: only the points 0, stride,
 * 2 stride, ... take part (a sample keeps the caller's side of the comparison cheap).  Waits for a deferred insertion to finish. */
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint64_t srl_probe_mix(int16_t kx, int16_t ky, int16_t kz, int32_t count, float lx, float ly, float lz) {
    union { float f; uint32_t u; } a, b, c;
    a.f = lx; b.f = ly; c.f = lz;
    uint64_t h = (uint64_t)(uint16_t)kx | ((uint64_t)(uint16_t)ky << 16) | ((uint64_t)(uint16_t)kz << 32) | ((uint64_t)(uint32_t)count << 48);
    h = (h ^ (h >> 31)) * 0x9E3779B97F4A7C15ull;
    h ^= ((uint64_t)a.u << 32) | b.u;
    h = (h ^ (h >> 29)) * 0xBF58476D1CE4E5B9ull;
    h ^= c.u;
    h = (h ^ (h >> 32)) * 0x94D049BB133111EBull;
    return h ^ (h >> 30);
}
int srl_map_probe_checksum(srl_ctx *ctx, const double *world_xyz, int n, int stride, double voxel_size, uint64_t *checksum);

/* ------------------------------------------------------------------ colour voxel map (construction only)
 * replaces: the second half of lioOptimization::addPointsToMap (lioOptimization.cpp:520-554) -- addPointToColorMap (:448-518) into
 * color_voxel_map (lioOptimization.h), with rgb_points_vec (rgbMapTracker.h:40) deduplicated through the grid hashmap_3d_points
 * (utility.h:94-141) and the list voxels_recent_visited_temp (lioOptimization.h:291).  The consumers of those containers (imageProcessing,
 * rgbMapTracker, rendering, the publishers) stay with the caller; this is what they need to keep their own rgbPoint objects in step.
 * For batch point i = 0, 1, ... where i % add_point_step == 0 (:538), with p = (float)world_i per axis (cloudMap.cpp:7):
 *   k = short(p / size_voxel_map), g = short(p / min_distance_points), FP64 division of the FP32 value, 16-bit wrap included (:453-459);
 *   stored     <=> the voxel k is new (created, slot 0) or holds fewer than max_num_points_in_voxel points (:470-474, :495-499): no
 *                  distance test among residents, and min_num_points is the 0 of the reference's call (:539);
 *   registered <=> stored and g not yet in the grid (:461-462, :476-483, :501-508): point_index = size of the registered list, g enters
 *                  the grid.  A point a full voxel refuses neither registers nor claims g;
 *   visited    <=> |time_sweep_end - time_last_process| > 1e-5 and |voxel.last_visited_time - time_sweep_end| > 1e-5 (:487-491, :510-514;
 *                  a new voxel starts at 0.0): the voxel is stamped with time_sweep_end and listed once, in order of first touch,
 *                  whether or not the point was stored.
 * Every order comes from batch indices, none from arrival order: results are bitwise reproducible.  The LiDAR map, the neighbourhood
 * bounds and the taps are not touched.  Device bytes do not depend on max_num_points_in_voxel: 24 per voxel,
 * 24 per stored point, 4 per registered point, 16 per slot of the two open-addressing tables. */
typedef struct srl_color_opts {          /* mapOptions (parameters.h:98-106) */
    double  size_voxel_map;
    int32_t max_num_points_in_voxel;     /* 1 ... 255 */
    double  min_distance_points;         /* cell size of the de-duplication grid */
    int32_t add_point_step;              /* >= 1 */
} srl_color_opts;
/* one stored point: position as stored (FP32), its voxel and slot there, its index in the batch, its index in the registered list or -1 */
typedef struct srl_color_stored {
    float    x, y, z;
    int16_t  kx, ky, kz;
    uint16_t slot;
    int32_t  batch_index;
    int32_t  point_index;
} srl_color_stored;
typedef struct srl_color_totals { int32_t stored, created, registered, visited; } srl_color_totals;   /* of one insertion */
#define SRL_COLOR_MAP_INSERT_MAX_POINTS 1048576          /* the frame pipeline's limit */
void srl_color_opts_default(srl_color_opts *o);          /* effective values of config/r3live.yaml:71-75: 0.1 / 50 / 0.01 / 1 */
/* The options hold for the map's life.  SRL_ERR_BAD_ARG: NULL, a size that is not finite or <= 0, a cap outside 1 ... 255, a step < 1, or
 * a colour map that already exists (destroy it first).  srl_ctx_destroy destroys the map with the context. */
int srl_color_map_create(srl_ctx *ctx, const srl_color_opts *opts);
int srl_color_map_destroy(srl_ctx *ctx);
/* world_xyz: host points (n x 3, FP64), or NULL = the world points the last srl_frame_commit left in HBM (n is ignored; nothing crosses
 * PCIe on the way in; SRL_ERR_NO_SWEEP when a newer frame has been uploaded since, SRL_ERR_BAD_ARG when no frame was ever committed).
 * Outputs, each optional: outcome[n] (bit 0 stored, bit 1 created its voxel, bit 2 registered; 0 for a point the step skips or a full voxel
 * refuses), the stored records in batch order, the visited list (int32 x 3 per voxel, voxelId, cloudMap.h:88) in order, and the totals.
 * stored_capacity / visited_capacity (records / voxels; checked only where the pointer is given) must be at least the number of
 * participating points ceil(n / add_point_step), else SRL_ERR_BAD_ARG before anything is done.  Synchronous: one wait for the counts,
 * then one DMA per requested list.  n == 0: SRL_OK.  NULL ctx, n < 0 or n > SRL_COLOR_MAP_INSERT_MAX_POINTS: SRL_ERR_BAD_ARG; no colour
 * map: SRL_ERR_NO_MAP; more than one rank: SRL_ERR_UNSUPPORTED -- all before a device is touched.  Cancels an armed launch.
 * Contract: finite coordinates with |p / size| < 2^31. */
int srl_color_map_insert(srl_ctx *ctx, const double *world_xyz, int n, double time_sweep_end, double time_last_process,
                         uint8_t *outcome /* n or NULL */, srl_color_stored *stored /* or NULL */, int stored_capacity,
                         int32_t *visited_xyz /* or NULL */, int visited_capacity, srl_color_totals *totals /* or NULL */);
/* grid_cells == registered: a cell enters the grid with the point that registers (kept apart because the two containers are) */
int srl_color_map_size(srl_ctx *ctx, int64_t *num_points, int32_t *num_voxels, int64_t *num_registered, int64_t *num_grid_cells);
/* The map in creation order: per voxel its key, count and last_visited_time; the points voxel after voxel in slot order (xyz, and
 * point_index = index in the registered list or -1), counts[v] of them for voxel v.  Every output optional; max_voxels / max_points are
 * the capacities (SRL_ERR_BAD_ARG when the map is larger). */
int srl_color_map_download(srl_ctx *ctx, int16_t *keys_xyz, int32_t *counts, double *last_visited_time, int max_voxels,
                           float *xyz, int32_t *point_index, int64_t max_points);
/* rgb_points_vec[first .. first + count): one record per registered point (batch_index = its position in the device's point pool,
 * i.e. its rank among all stored points; point_index = its index in the list). */
int srl_color_registered_download(srl_ctx *ctx, int64_t first, int count, srl_color_stored *out);

/* ------------------------------------------------------------------ colour voxel map: rendering an image into it
 * replaces: rgbMapTracker::renderPointsInRecentVoxel / threadRenderPointsInVoxel (rgbMapTracker.cpp:176-237): for every point of every
 * listed voxel cloudFrame::project3dPointInThisImage (lioOptimization.cpp:142-199) with if2dPointsAvailable (:48-60), the sub-pixel colour
 * cloudFrame::getRgb(u, v, 0) = getSubPixel<cv::Vec3b> (:71-103) and rgbPoint::updateRgb(colour, distance, (15, 15, 15), obs_time)
 * (cloudMap.cpp:59-100).  The per-point colour state (rgb int16 x 3, cov_rgb FP32 x 3, observe_distance, last_observe_time, N_rgb int16:
 * cloudMap.h:51-66) lives in HBM beside the point pool, 40 bytes per stored point, allocated at the first srl_color_image_upload; zero
 * bytes are rgbPoint::reset().  selectPointsForProjection is srl_color_map_select below, the measurement loops of vioEsikf and of
 * vioPhotometric are srl_color_map_vio_rows, the optical flow is srl_flow_track_image, the inlier sets the reference takes from findFundamentalMat and
 * solvePnPRansac have a stand-in of this library's own (srl_consensus_*, not OpenCV's results), and so have the undistortion and the
 * equalisation of the image (srl_image_prepare: this library's specified operations, not OpenCV's bytes); the rest of the vision stage
 * (the publishers) stays with the caller; cv::resize at a ratio other than 1 is srl_image_prepare_resized.
 *
 * Per point, FP64 unless noted, no contraction, sums of three as (a0 + a1) + a2:
 *   p = (double) stored FP32 position; pc = R_cw p + t_cw with q_cw = q_world_camera.inverse(), R_cw = q_cw.toRotationMatrix(),
 *   t_cw = -R_cw t_world_camera (refreshPoseForProjection, :201-205: computed on the host); rejected if pc.z < 0.001;
 *   u = (pc.x fx / pc.z + cx) * 1.0, v = (pc.y fy / pc.z + cy) * 1.0; accepted iff u >= m cols + 1, ceil(u) < (1 - m) cols, v >= m rows + 1,
 *   ceil(v) < (1 - m) rows with m = fov_margin; d = |p - t_world_camera|;
 *   colour: r0 = floor(v), c0 = floor(u), fr = v - r0, fc = u - c0; per channel the SATURATING 8-bit sum, left to right, of
 *   sat8((1-fr)(1-fc) I[r0][c0]), sat8(fr (1-fc) I[r0+1][c0]), sat8((1-fr) fc I[r0][c0+1]), sat8(fr fc I[r0+1][c0+1]) where
 *   sat8(x) = round to nearest, ties to even, clamped to 0 ... 255 -- OpenCV's `double * Vec3b` and `Vec3b + Vec3b`:
 *   a sum of four individually rounded bytes, not a rounded bilinear value.  The one neighbour the field-of-view test lets lie past the row or the image (integral u = cols - 1 or v = rows - 1) has
 *   weight exactly 0 and contributes 0 whatever it holds: it is read from the last column / row instead;
 *   updateRgb, literally: nothing if observe_distance != 0 and d > 1.2 observe_distance; the first observation (N_rgb == 0) stores the
 *   colour, cov = 15, d, obs_time, N_rgb = 1; otherwise per channel cov = (float)(cov + 0.1 (obs_time - last_observe_time)), old = cov,
 *   cov = (float)sqrt(1 / (1 / (cov * cov [FP32]) + 1 / 225)), rgb = (short)(cov * cov [FP32] * (rgb / old^2 + colour / 225)) truncated
 *   toward zero, then observe_distance = min(observe_distance, d), last_observe_time = obs_time, N_rgb++.
 * N_rgb is an int16 as in the reference: a point observed more than 32 767 times is outside the contract.  Results are bitwise those of
 * the reference's loop and reproducible.  The LiDAR map, the neighbourhood bounds and the taps are not touched. */
typedef struct srl_color_camera {
    double q_world_camera[4];            /* w, x, y, z (state.h) */
    double t_world_camera[3];
    double fx, fy, cx, cy;
    double fov_margin;                   /* state.cpp:25: 0.005; the render needs > 0 (at 0 an integral u = cols - 1 reads past the row) */
} srl_color_camera;
/* of one render, counted per occurrence of a voxel in the list: points of listed voxels; of those rejected behind the camera, rejected
 * by the field of view, refused by updateRgb's distance gate, first observations, updates (the reference's render_point_count); and the
 * list entries whose voxel the map does not hold */
typedef struct srl_color_render_totals { int64_t listed, behind, outside, gated, first, updated, unknown; } srl_color_render_totals;
#define SRL_COLOR_IMAGE_MAX_PIXELS 67108864
/* rgb_image of the frame (cloudFrame::rgb_image: 8-bit, 3 channels, BGR as OpenCV holds it; getRgb returns channels 0, 1, 2 as they lie),
 * already undistorted and equalised (imageProcessing.cpp:113-125) by the caller -- srl_image_prepare does both on the device and
 * installs its result here without this call.  Copied through page-locked staging into a device buffer
 * that is reused while the size stays the same; the call returns when the staging copy is made, the DMA is ordered in front of the next
 * render.  The first upload allocates the colour state.  NULL, rows or cols < 2, rows * cols > SRL_COLOR_IMAGE_MAX_PIXELS or
 * row_stride_bytes < 3 cols: SRL_ERR_BAD_ARG; no colour map: SRL_ERR_NO_MAP; more than one rank: SRL_ERR_UNSUPPORTED -- all before a
 * device is touched.  Cancels an armed launch. */
int srl_color_image_upload(srl_ctx *ctx, const uint8_t *bgr, int rows, int cols, int64_t row_stride_bytes);
/* voxels_xyz: n_voxels x 3 int32, the caller's voxels_recent_visited (the visited output of srl_color_map_insert).  The list may name a
 * voxel several times (lioOptimization.cpp:523-550: the temp list accumulates while to_rendering is false); the reference renders such
 * a voxel once per occurrence with the same observation, and so does this call: updateRgb runs `multiplicity` times in a row per point
 * (at most 65 535 occurrences of one voxel: SRL_ERR_UNSUPPORTED beyond, nothing changed, *totals all zero as for every other
 * refusal; the call after a refusal is an ordinary one).  A key the map does not hold is counted in
 * totals->unknown and otherwise ignored (the reference's map[voxel] would create an empty block; lists come from the insertion, so this
 * does not arise).  The pass visits every stored point of the map once, whatever the list's length.  Synchronous: one wait for the totals.
 * Return codes, all before a device is touched: NULL ctx, cam or (n_voxels > 0) voxels_xyz, n_voxels < 0, a non-finite camera or obs_time,
 * fov_margin <= 0: SRL_ERR_BAD_ARG; no colour map: SRL_ERR_NO_MAP; no image uploaded: SRL_ERR_NO_SWEEP; more than one rank:
 * SRL_ERR_UNSUPPORTED; n_voxels == 0: SRL_OK with zero totals.  Cancels an armed launch. */
int srl_color_map_render(srl_ctx *ctx, const srl_color_camera *cam, const int32_t *voxels_xyz, int n_voxels, double obs_time,
                         srl_color_render_totals *totals /* or NULL */);
/* The colour state in the order srl_color_map_download writes xyz in (voxel after voxel, slot order): rgb int16 x 3 (getRgb(): channels as
 * the image held them), N_rgb, cov_rgb FP32 x 3, observe_distance, last_observe_time.  Every output optional; max_points is the capacity
 * (SRL_ERR_BAD_ARG when the map holds more).  A map never rendered gives zeros. */
int srl_color_map_download_rgb(srl_ctx *ctx, int16_t *rgb, int16_t *n_rgb, float *cov_rgb, double *observe_distance, double *last_observe_time,
                               int64_t max_points);
/* ... and of rgb_points_vec[first .. first + count): what the publishers read (getRgb(), N_rgb against pub_point_minimum_views:
 * lioOptimization.cpp:1228-1230, 1290-1292, 1414-1416).  One gather kernel and one DMA of exactly count records. */
int srl_color_registered_rgb(srl_ctx *ctx, int64_t first, int count, int16_t *rgb, int16_t *n_rgb, float *cov_rgb, double *observe_distance,
                             double *last_observe_time);

/* ------------------------------------------------------------------ colour voxel map: selecting points for projection
 * replaces: rgbMapTracker::selectPointsForProjection (rgbMapTracker.cpp:45-152), as refreshPointsForProjection (:26-43) and the tracker's
 * own call (imageProcessing.cpp:131) use it.  Candidates points_for_projection[i]: in LIST mode (use_all_points clear and n_voxels > 0)
 * the last point (points.back(): the highest slot) of every list entry whose voxel the map holds, once per occurrence, in list order --
 * an entry the map does not hold is counted in totals->unknown and takes no index (the reference's map[voxel] creates an empty block
 * there); otherwise ALL registered points, rgb_points_vec in order.  For i = 0, skip_step, 2 skip_step, ...:
 *   p = (double) stored FP32 position; depth = |p - t_world_camera| (the render's d); skipped if depth > maximum_depth, then if
 *   depth < minimum_depth (a depth equal to a limit stays); project3dPointInThisImage(p, u_f, v_f, nullptr, 1.0) exactly as the render
 *   carries it; the cell key is the pair of int u = (int)(round(u_f / minimum_dis) * minimum_dis), v likewise: FP64 quotient, rounding
 *   half away from zero, FP64 product, truncation toward zero (for a non-integral or sub-unit minimum_dis distinct quotients can share a
 *   key); the cell keeps (float) depth of its last setter, and candidate i takes the cell iff it is empty or (double) stored > depth_i.
 * The output is the final holder of every cell, ascending in i, with cv::Point2f(u_f, v_f) = two casts to float.  Because the stored
 * depth is rounded the holder is not simply the nearest candidate: with M the smallest (float) depth of the cell it is the LAST i with
 * depth_i < (double) M if there is one, otherwise the FIRST i with (float) depth_i == M.  The device evaluates this rule with integer
 * atomics per cell; results are bitwise those of the reference's sequential loop and reproducible.
 * No image is needed (image_rows / image_cols are the frame's size: the pass reads no pixel).  fov_margin may be <= 0 here -- the
 * tracker's own frame uses -0.4 (rgbMapTracker.cpp:157, :164): any finite margin with -4 <= margin < 0.5.
 * Synchronous: one wait for the totals, then one DMA of exactly totals->selected records.  out == NULL: the totals alone.
 * capacity < selected: SRL_ERR_BAD_ARG with the totals filled and nothing copied (the call changes nothing in the map: ask again).
 * Before a device is touched: NULL ctx, cam, opts or (n_voxels > 0) voxels_xyz, n_voxels < 0, capacity < 0, a bad option, rows or cols
 * < 2, rows * cols > SRL_COLOR_IMAGE_MAX_PIXELS, a non-finite camera, a margin outside [-4, 0.5): SRL_ERR_BAD_ARG; no colour map:
 * SRL_ERR_NO_MAP; more than one rank: SRL_ERR_UNSUPPORTED.  Cancels an armed launch.  Neither map, nor the colour state, the neighbourhood
 * bounds or the taps are touched. */
typedef struct srl_color_select_opts {
    double minimum_dis;          /* finite, 0 < minimum_dis <= 65536 */
    int32_t skip_step;           /* >= 1 */
    int32_t use_all_points;
    double minimum_depth, maximum_depth;     /* not NaN */
} srl_color_select_opts;
/* 10.0, 1, 0, 0.1, 200 (rgbMapTracker.cpp:9-10, :36) */
void srl_color_select_opts_default(srl_color_select_opts *o);
typedef struct srl_color_selected {
    int32_t index;               /* position in points_for_projection */
    int32_t pool;                /* pool position = batch_index of srl_color_registered_download */
    int32_t point_index;         /* registered index or -1 */
    float x, y, z;
    float u, v;
} srl_color_selected;
/* candidates: size of points_for_projection; visited: those with i % skip_step == 0; of those: beyond maximum_depth, nearer than
 * minimum_depth, behind the camera, outside the field of view; selected: cells = records; unknown: list entries the map does not hold */
typedef struct srl_color_select_totals {
    int64_t candidates, visited, far, near, behind, outside, selected, unknown;
} srl_color_select_totals;
int srl_color_map_select(srl_ctx *ctx, const srl_color_camera *cam, int image_rows, int image_cols, const int32_t *voxels_xyz, int n_voxels,
                         const srl_color_select_opts *opts, srl_color_selected *out /* or NULL */, int64_t capacity,
                         srl_color_select_totals *totals /* or NULL */);

/* ------------------------------------------------------------------ colour voxel map: the camera ESIKF's measurement passes
 * replaces: the per-point loops of imageProcessing::vioEsikf (imageProcessing.cpp:308-349, the reprojection update of time offset,
 * extrinsics and intrinsics: 11 columns) and imageProcessing::vioPhotometric (:463-518, the photometric update of the extrinsics: 6
 * columns), and the products H^T H, H^T r over them.  The 11- and 6-dimensional solves, the state update and the covariance stay on the
 * host (csrc/host/imageProcessing.cpp, srl_lio_vio_* of srlivo_host.h); with the caller stay PnP / RANSAC, undistortion and
 * equalisation (updateAndAppendTrackPoints is srl_color_map_track_update below).  The points are named by pool position (srl_color_selected.pool) and visited in the
 * caller's order -- the reference walks a
 * std::map keyed by pointer value, whose order is not reproducible.
 *
 * Per point, FP64, no contraction, sums of three as (a0 + a1) + a2: p = (double) stored FP32 position, pc = R_cw p + t_cw as the render
 * forms it; pixel = (fx pc.x / pc.z + cx, fy pc.y / pc.z + cy) + time_td * vel.  A pool position outside [0, num_points) is `unknown`,
 * pc.z < 0.001 (the projection's own threshold) is `behind`: both are left out and counted, where the reference divides unguarded.
 * huber(x) = 1 for x < 1, else (2 sqrt(x) - 1) / x (getHuberLoss(x, 1.0)); J_u_pc = [fx/z 0 -(fx x)/(z z); 0 fy/z -(fy y)/(z z)].
 * REPROJECTION: d = pixel - match, residual = |d|, h = huber(residual); r = d h; H column 0 = vel h; with estimate_extrinsic columns
 *   1-3 = (J_u_pc skew(pc)) h and 4-6 = ((-J_u_pc) R_imu_camera^T) h; with estimate_intrinsic columns 7-10 = [x/z 0 1 0; 0 y/z 0 1] h;
 *   acc_residual += residual.
 * PHOTOMETRIC: a point with N_rgb < 3 is `few_views` and left out (the reference's `continue`; tested in front of the projection, so a
 *   point that is both is few_views; a map never rendered has no state: every point is few_views).  The sample is
 *   cloudFrame::getRgb(u, v, 0, &dx, &dy) (lioOptimization.cpp:99-140) on the uploaded image: obs = getSubPixel<cv::Vec3b>(v, u), the
 *   render's four individually rounded, saturating-added bytes; dx = (float)(sum_{b=1..4} sample(v, u + b) - sum sample(v, u - b)) / 20
 *   with float sums of integers, dy likewise in v.  The reference reads these 17 samples with no bounds check; here a point is sampled
 *   only if floor(u) - 4 >= 0, floor(u) + 5 <= cols - 1 and the same in v against rows, otherwise (and for a non-finite pixel) it is
 *   `outside` and left out; nothing is clamped.  info_k = 1 / (double) cov_rgb[k]; res = obs - (double) rgb; h = huber(|res|);
 *   r = res h; acc_residual += ((r0 i0) r0 + (r1 i1) r1) + (r2 i2) r2; J_color_pc = [dx dy] J_u_pc; with estimate_extrinsic columns
 *   0-2 = (J_color_pc skew(pc)) h and 3-5 = ((-J_color_pc) R_imu_camera^T) h, zeros without.
 * rows (optional): 24 doubles per input position: reprojection 2 x (11 H, r), photometric 3 x (6 H, r, info); zeros for a point left
 * out.  outcome (optional): one byte per input position, srl_color_vio_outcome.  sums: over the used points in list order within a
 * wave's 64 points, then the four waves of a workgroup, then the workgroups in index order -- no floating-point atomics, so two calls
 * with the same inputs return the same bytes whether or not rows / outcome are requested: H^T H[a][b] = sum h_a h_b (photometric:
 * sum (h_a info) h_b, in the leading 6 x 6, rest 0), a point's rows added as (row0 + row1) + row2; H^T r likewise.
 * Synchronous: one kernel, one DMA per requested output.  n == 0: SRL_OK with zeroed sums.  Before a device is touched: NULL ctx, args,
 * sums or (n > 0) points, n < 0, n > SRL_COLOR_VIO_MAX_POINTS, a mode that is neither, a non-finite camera, time_td or R_imu_camera:
 * SRL_ERR_BAD_ARG; no colour map: SRL_ERR_NO_MAP; photometric mode without an uploaded image: SRL_ERR_NO_SWEEP; more than one rank:
 * SRL_ERR_UNSUPPORTED.  Cancels an armed launch.  Nothing in the map or its colour state is changed. */
#define SRL_COLOR_VIO_MAX_POINTS 65536
typedef enum { SRL_VIO_REPROJECTION = 0, SRL_VIO_PHOTOMETRIC = 1 } srl_color_vio_mode;
typedef enum { SRL_VIO_USED = 0, SRL_VIO_FEW_VIEWS = 1, SRL_VIO_BEHIND = 2, SRL_VIO_OUTSIDE = 3, SRL_VIO_UNKNOWN = 4 } srl_color_vio_outcome;
typedef struct srl_color_vio_point {   /* 40 B */
    int32_t pool, pad;                 /* pool position, as srl_color_selected.pool */
    double match_u, match_v;           /* it->second of map_rgb_points_in_last_image_pose (reprojection mode only) */
    double vel_u, vel_v;               /* rgbPoint::image_velocity */
} srl_color_vio_point;
typedef struct srl_color_vio_args {
    srl_color_camera cam;              /* q_world_camera, t_world_camera, fx fy cx cy; fov_margin ignored */
    double time_td, R_imu_camera[9];   /* row-major */
    int32_t mode;                      /* SRL_VIO_REPROJECTION (11 columns) | SRL_VIO_PHOTOMETRIC (6 columns) */
    int32_t estimate_extrinsic, estimate_intrinsic;
} srl_color_vio_args;
typedef struct srl_color_vio_sums {
    double HtH[121];                   /* row-major, full and symmetric; photometric: Ht Rinv H in the leading 6 x 6, rest 0 */
    double Htr[11];                    /* Ht r, photometric: Ht Rinv r */
    double acc_residual;               /* sum of the loop's acc_residual terms, before any division */
    int64_t used, few_views, behind, outside, unknown;
} srl_color_vio_sums;
int srl_color_map_vio_rows(srl_ctx *ctx, const srl_color_vio_args *args, const srl_color_vio_point *points, int n,
                           srl_color_vio_sums *sums, double *rows /* n x 24 or NULL */, uint8_t *outcome /* n or NULL */);

/* ------------------------------------------------------------------ colour voxel map: the camera tracker's point set
 * replaces: opticalFlowTracker::updateAndAppendTrackPoints (opticalFlowTracker.cpp:13-102) without its closing
 * updateLastTrackingVectorAndIds, which is the host mirror's (csrc/host/opticalFlowTracker.h).  tracked = the elements of
 * map_rgb_points_in_last_image_pose in the caller's order (the reference walks a std::map keyed by pointer value, whose order is not
 * reproducible; nothing below depends on it), candidates = points_rgb_vec_for_projection as pool positions in its order.
 * FP64, no contraction, sums of three as (a0 + a1) + a2; p = (double) stored FP32 position; the projection is the render's
 * project3dPointInThisImage(p, u_d, v_d, nullptr, 1.0); cam->fov_margin is the frame's own (state.cpp:25: 0.005).
 * FIRST LOOP (:22-61), per tracked point: max_err = 2.0 * image_cols / 320.0; error = sqrt(du du + dv dv), du = u_d - (double) u,
 *   dv = v_d - (double) v, (u_d, v_d) as written by a projection inside OR outside the field of view.  error > max_err: the flag is
 *   raised, and the point is DROPPED (its flag back to 0) if the flag was raised already (flagged >= 1) or error > max_err * 2, otherwise
 *   KEPT_FLAGGED (flag = flagged + 1).  error <= max_err (or not comparable): KEPT with flag 0.  A kept point whose projection is inside
 *   the field of view occupies the cell (int)(round(u_d / mini_distance) * mini_distance), v likewise -- the selection's statements.
 *   The depth the reference stores in the mask is never read and not computed.
 *   Two departures from the reference: a point BEHIND the camera (pc.z < 0.001) leaves u_d, v_d unwritten there, so its error is formed
 *   from the previous map element's pixel (for the first element from an uninitialised variable): here it is dropped with flag 0.  A
 *   pool position outside [0, num_points) is UNKNOWN, one that occurred earlier in `tracked` is DUPLICATE (a std::map cannot hold
 *   either): both are dropped.
 * SECOND LOOP (:63-99), as a rule: with T the kept points and s0 = |T|, candidate i is PROCESSED iff its pool position is known, not in
 *   T and did not occur earlier among the candidates (a later occurrence is found in the map or refused as the first was: it is counted
 *   ALREADY_TRACKED).  A processed candidate is a WINNER iff its projection is inside the field of view, no point of T occupies its cell
 *   and no processed candidate with a smaller index and an inside projection has the same cell.  size() >= maximum_tracked_points is
 *   tested behind every processed candidate and the size changes only on an add: if s0 < maximum_tracked_points the adds are the first
 *   maximum_tracked_points - s0 winners in index order; otherwise (maximum_tracked_points <= 0 included: the reference's member is
 *   unsigned, a negative value is taken as 0 is) the only add is the first
 *   processed candidate, and only if it is a winner.  The loop breaks behind the last add of a filled set, or behind that first
 *   processed candidate.  Behind the break a winner is CUT and every other candidate NOT_REACHED, whatever it would have been; in front
 *   of it a processed candidate that is no winner is REFUSED (behind the camera or outside the field of view) or OCCUPIED.  An added
 *   point enters with cv::Point2f(u_d, v_d) = two casts to float and flagged = 0 (the reference keeps is_out_lier_count in the rgbPoint:
 *   the host mirror overlays the flags of points that left the set flagged).
 * out: the kept points in input order, u, v untouched, flags updated, then the added points in candidate order.  The outcome arrays
 * hold one byte per input position.  totals: tracked_in = n = kept + dropped + behind + unknown + duplicate, kept = s0 with `flagged`
 * of them KEPT_FLAGGED; candidates = n_candidates = already_tracked + cand_unknown + refused + occupied + added + cut + the not reached.
 * Synchronous: one wait for the totals (and the requested outcome bytes), then one DMA of exactly kept + added records.  out == NULL:
 * no records.  capacity < kept + added: SRL_ERR_BAD_ARG with the totals filled and nothing copied (the call changes nothing in the map:
 * ask again).  n == 0 and n_candidates == 0 are legal; with both zero SRL_OK and zero totals.
 * Before a device is touched: NULL ctx, cam or opts, a NULL array with a positive count, a negative count or capacity, n >
 * SRL_COLOR_TRACK_MAX_POINTS, n_candidates > SRL_COLOR_TRACK_MAX_CANDIDATES, mini_distance not finite or outside (0, 65536], rows or
 * cols < 2, rows * cols > SRL_COLOR_IMAGE_MAX_PIXELS, a non-finite camera, a margin outside [-4, 0.5): SRL_ERR_BAD_ARG; no colour map:
 * SRL_ERR_NO_MAP; more than one rank: SRL_ERR_UNSUPPORTED.  Cancels an armed launch.  Neither map, nor the colour state, the
 * neighbourhood bounds, the taps or the selection's buffers are touched. */
#define SRL_COLOR_TRACK_MAX_POINTS     65536      /* tracked points in */
#define SRL_COLOR_TRACK_MAX_CANDIDATES 1048576
typedef enum { SRL_TRACK_KEPT = 0, SRL_TRACK_KEPT_FLAGGED = 1, SRL_TRACK_DROPPED = 2, SRL_TRACK_BEHIND = 3, SRL_TRACK_UNKNOWN = 4, SRL_TRACK_DUPLICATE = 5 } srl_color_track_outcome;
typedef enum { SRL_TRACK_CAND_ADDED = 0, SRL_TRACK_CAND_ALREADY_TRACKED = 1, SRL_TRACK_CAND_UNKNOWN = 2, SRL_TRACK_CAND_REFUSED = 3, SRL_TRACK_CAND_OCCUPIED = 4,
               SRL_TRACK_CAND_CUT = 5, SRL_TRACK_CAND_NOT_REACHED = 6 } srl_color_track_candidate_outcome;
typedef struct srl_color_track_point {   /* 16 B */
    int32_t pool;        /* pool position, as srl_color_selected.pool */
    float   u, v;        /* it->second of map_rgb_points_in_last_image_pose (cv::Point2f) */
    int32_t flagged;     /* rgbPoint::is_out_lier_count: only ever 0 or 1 between calls */
} srl_color_track_point;
typedef struct srl_color_track_opts { double mini_distance; int32_t maximum_tracked_points, reserved; } srl_color_track_opts;
typedef struct srl_color_track_totals {
    int64_t tracked_in, kept, flagged, dropped, behind, unknown, duplicate;          /* first loop */
    int64_t candidates, already_tracked, cand_unknown, refused, occupied, added, cut; /* second loop */
} srl_color_track_totals;
/* 10.0, 300 (imageProcessing.cpp:161, opticalFlowTracker.cpp:10) */
void srl_color_track_opts_default(srl_color_track_opts *o);
int srl_color_map_track_update(srl_ctx *ctx, const srl_color_camera *cam, int image_rows, int image_cols,
        const srl_color_track_point *tracked, int n, const int32_t *candidates /* pool positions, in order */, int n_candidates,
        const srl_color_track_opts *opts, srl_color_track_point *out /* capacity, or NULL */, int64_t capacity,
        uint8_t *tracked_outcome /* n or NULL */, uint8_t *candidate_outcome /* n_candidates or NULL */, srl_color_track_totals *totals /* or NULL */);

/* ------------------------------------------------------------------ optical flow of the camera stage
 * replaces: LKOpticalFlowKernel::trackImage (lkpyramid.cpp:755-795) as opticalFlowTracker::trackImage calls it (opticalFlowTracker.cpp:134):
 * the 8-bit pyramid of the gray image with 21-pixel BORDER_REFLECT_101 borders (opencvBuildOpticalFlowPyramid, :510-625: level k =
 * cv::pyrDown of level k - 1; building stops after the level whose successor would be 21 or fewer pixels wide or high, and the lowered
 * level count holds for the tracker's life), the Scharr derivative of every level (calcSharrDeriv, :57-154, int16 (Ix, Iy), zero border)
 * and the pyramidal Lucas-Kanade track of n points (calculateLKOpticalFlow, :174-496, one channel, err = nullptr, no initial flow)
 * from the PREVIOUS image and ITS derivatives to the image given.  The two pyramid sets are then swapped.  next_xy and status are
 * bitwise the reference's: its float statements in its order, its SSE accumulation order, nextPts written before the range tests,
 * status cleared at level 0 only.  With the caller stay reduce_vector and the bookkeeping of opticalFlowTracker (the
 * host mirror's); cv::findFundamentalMat and solvePnPRansac have srl_consensus_*, and CLAHE, cvtColor and the undistortion have
 * srl_image_prepare, as stand-ins of this library's own.  gray is the caller's equalised gray image, an upload of its own (it is no
 * function of the image of srl_color_image_upload); srl_flow_track_prepared tracks on srl_image_prepare's gray image without an upload.
 * The first image of a tracker is only stored: next_xy = prev_xy, status is not written, *n_tracked = 0.  Every later call writes
 * next_xy (n x 2 floats, x then y) and status (n bytes) for ALL points and *n_tracked = the number of status == 1.  n == 0 is accepted
 * (the pyramid is still built and swapped).
 * Two departures from the reference, both on input it leaves to cvtss2si's overflow value: a point with a coordinate that is not
 * finite, or whose window corner (coordinate - 10) does not fit int32, gets status 0 and next = prev; an image whose size differs
 * from the tracker's first image is SRL_ERR_BAD_ARG (the reference would re-allocate one pyramid set and then assert).
 * Synchronous.  Before a device is touched: NULL ctx or gray, rows or cols < 2 or > SRL_FLOW_MAX_EXTENT, row_stride_bytes < cols, n < 0,
 * n > SRL_FLOW_MAX_POINTS, n > 0 with a NULL array: SRL_ERR_BAD_ARG with *n_tracked = 0; no tracker: SRL_ERR_NO_MAP.  Cancels an armed
 * launch.  srl_flow_create: win other than 21: SRL_ERR_UNSUPPORTED (the order of the float sums is that of a 21-wide window row);
 * max_level outside 0 ... 3, max_count outside 0 ... 100, epsilon outside [0, 10] (the ranges LKOpticalFlowKernel::setTerminationCriteria
 * clamps to), a min_eig_threshold that is not finite, or a tracker that already exists: SRL_ERR_BAD_ARG. */
#define SRL_FLOW_MAX_POINTS 65536
#define SRL_FLOW_MAX_EXTENT 16384
typedef struct srl_flow_opts {
    int32_t win, max_level, max_count, reserved;      /* 21, 3, 10 (opticalFlowTracker.cpp:5-8) */
    double epsilon, min_eig_threshold;                /* 0.05 (compared with |delta|^2 as it is), 1e-4 */
} srl_flow_opts;
void srl_flow_opts_default(srl_flow_opts *opts);
int srl_flow_create(srl_ctx *ctx, const srl_flow_opts *opts);
int srl_flow_destroy(srl_ctx *ctx);
int srl_flow_track_image(srl_ctx *ctx, const uint8_t *gray, int rows, int cols, int64_t row_stride_bytes, const float *prev_xy, int n,
                         float *next_xy, uint8_t *status, int *n_tracked);

/* ------------------------------------------------------------------ consensus outlier rejection of the camera tracker
 * stands where the reference calls cv::findFundamentalMat(last, cur, FM_RANSAC, 1.0, 0.997, status) (opticalFlowTracker.cpp:144) and
 * cv::solvePnPRansac(points_3d, points_2d, intrinsic, ..., 200, 1.5, 0.99, status) (:295).  The reference reads ONLY the inlier mask /
 * inlier list of either call (mat_F, cv_so3 and cv_trans are never used), and OpenCV's own mask depends on its private random generator,
 * so every consumer already takes any valid consensus set.  These two calls are therefore NOT OpenCV's results and claim no parity
 * with them: they are a deterministic RANSAC of this library, a function of (inputs, options) alone -- the same bytes call after call.
 *
 * H = opts->hypotheses hypotheses, always all of them (the run time does not depend on the data).  Hypothesis h draws its minimal sample
 * from the USABLE points (every coordinate finite; in input order, m of them) with a counter-based generator, no state between calls:
 *   draw(seed, h, k, m) = ((mix(((uint64) seed << 32 | h) * 0x9E3779B97F4A7C15 + (k + 1) * 0xBF58476D1CE4E5B9) >> 32) * m) >> 32,
 *   mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31      (all modulo 2^64)
 * for k = 0, 1, ...: a draw that repeats an earlier position is rejected, and a hypothesis that has not collected its sample after 64
 * draws has none.  The minimal problem is solved in FP64:
 *   fundamental  the 7-point algorithm on Hartley-normalised points (per call: centroid and sqrt 2 / mean distance of the usable points
 *                of each view): the two null vectors F1, F2 of the 7 x 9 system, the real roots of det(a F1 + (1 - a) F2) = 0, each
 *                solution de-normalised and scaled to unit Frobenius norm -- up to 3 model slots per hypothesis;
 *   PnP          P3P (Grunert's quartic as in Haralick et al., IJCV 1994, each root refined on the three distance equations) on image
 *                points normalised by fx, fy, cx, cy; every solution with positive depth at the three sample points is kept as R, t
 *                (camera = R world + t) -- up to 4 slots; no fourth point disambiguates, every solution is scored.
 * A degenerate sample (repeated or collinear points, a vanishing leading coefficient) gives no model, never a NaN model.
 * Every model is scored on all n points, FP64, no contraction, in exactly this order (float inputs converted to double first):
 *   fundamental, F row-major, (x1, y1) of last_xy, (x2, y2) of cur_xy:
 *     a = (F0 x1 + F1 y1) + F2, b = (F3 x1 + F4 y1) + F5, c = (F6 x1 + F7 y1) + F8, d2 = (a x2 + b y2) + c, e2 = (d2 d2) / (a a + b b);
 *     a' = (F0 x2 + F3 y2) + F6, b' = (F1 x2 + F4 y2) + F7, c' = (F2 x2 + F5 y2) + F8, d1 = (a' x1 + b' y1) + c', e1 = (d1 d1) / (a' a' + b' b');
 *     inlier iff e1 <= threshold^2 and e2 <= threshold^2 (the larger of the two squared distances to the epipolar lines);
 *   PnP: xc = ((R0 X + R1 Y) + R2 Z) + t0, yc and zc likewise with rows 1 and 2; du = (fx (xc / zc) + cx) - u, dv = (fy (yc / zc) + cy) - v;
 *     inlier iff zc > 0 and du du + dv dv <= threshold^2.
 * A point with a non-finite coordinate is never an inlier.  The valid model with the most inliers wins, ties go to the lowest model
 * index = hypothesis * slots + slot (slots: 3, 4).  status = its n-byte mask; inliers = the ascending indices of its inliers.
 * result: model = F row-major in [0, 9) (the rest 0), or R row-major then t; sample = the 7 or 3 sample indices padded with -1;
 * hypothesis, slot = the winner's; inliers = its count; models_valid = valid models among all slots; confidence_reached = 1 iff
 * 1 - (1 - w^s)^H >= confidence with w = inliers / n, s = 7 or 3 (powers by repeated multiplication) -- the only role of OpenCV's
 * confidence argument.  Without any valid model (every sample degenerate), or with n < 8 (fundamental) / n < 4 (PnP): SRL_OK, an
 * all-zero mask, no inliers, models_valid = 0, model 0, sample, hypothesis and slot -1.
 * Before a device is touched, SRL_ERR_BAD_ARG with the result zeroed and the outputs untouched: a NULL ctx (first), n < 0,
 * n > SRL_CONSENSUS_MAX_POINTS, a NULL array with n > 0, NULL n_inliers or intrinsics, hypotheses outside 1 ... SRL_CONSENSUS_MAX_HYPOTHESES,
 * a threshold that is not finite and positive, a confidence outside (0, 1), intrinsics that are not finite, fx or fy equal to 0.
 * opts == NULL: the defaults; result may be NULL.  More than one rank: SRL_ERR_UNSUPPORTED.  Synchronous; cancels an armed launch.  The
 * workspace (about 2 MB of device memory) is allocated at a context's first call and freed with the context; it is shared by both models
 * and never cleared, and no call depends on what it held (srl_debug_consensus_download of srlivo_hip_debug.h reads the usable list, the
 * normalisation and every hypothesis' sample, models and counts of the last call back for the tests of all the above). */
#define SRL_CONSENSUS_FUNDAMENTAL 0
#define SRL_CONSENSUS_PNP 1
#define SRL_CONSENSUS_MAX_POINTS 4096
#define SRL_CONSENSUS_MAX_HYPOTHESES 4096
typedef struct srl_consensus_opts { double threshold; double confidence; int32_t hypotheses; uint32_t seed; } srl_consensus_opts;
typedef struct srl_consensus_result {
    double model[12];
    int32_t sample[8];
    int32_t hypothesis, slot, inliers, models_valid, confidence_reached, reserved;
} srl_consensus_result;
/* SRL_CONSENSUS_FUNDAMENTAL: 1.0, 0.997, 512, 0; SRL_CONSENSUS_PNP: 1.5, 0.99, 200, 0 (the reference's call-site arguments; 512 is ours) */
void srl_consensus_opts_default(srl_consensus_opts *o, int model);
int srl_consensus_fundamental(srl_ctx *ctx, const float *last_xy, const float *cur_xy, int n, const srl_consensus_opts *opts, uint8_t *status,
                              srl_consensus_result *result);
int srl_consensus_pnp(srl_ctx *ctx, const float *xyz, const float *uv, int n, const double *fx_fy_cx_cy, const srl_consensus_opts *opts,
                      int32_t *inliers, int *n_inliers, srl_consensus_result *result);

/* ------------------------------------------------------------------ image preparation of the camera stage
 * stands where imageProcessing::process (imageProcessing.cpp:113-125, :166-200) calls cv::remap with the maps of
 * initUndistortRectifyMap(..., CV_16SC2) (:103), cvtColor(COLOR_RGB2GRAY) + imageEqualize(gray, 3.0) and equalizeColorImageYcrcb: one raw
 * BGR frame in, the equalised gray image (srl_flow_track_prepared's) and the equalised BGR image (the colour map's, as by
 * srl_color_image_upload) out, nothing in between on the host.  As for the consensus estimators, these are operations OF THIS LIBRARY,
 * specified here and checked against an independent restatement; they claim NO equality with OpenCV's bytes.  Followed from OpenCV: the
 * CV_16SC2 map layout with 5 fractional bits, the 15-bit fixed-point bilinear weights, the 15-bit gray and 14-bit YCrCb coefficients,
 * CLAHE's clip / redistribute / bilinear-LUT structure and the reference's tile rule.  The one deliberate difference: the map is the
 * explicit formula below on (j - cx) / fx (OpenCV iterates an inverse camera matrix along the row); DESIGN.md section 4.5 lists the rest.
 * cv::resize (:113-118; image_resize_ratio is 1.0 in the reference, :11) is stage (r) below, run by srl_image_prepare_resized alone.
 * Notation: DESCALE(x, n) = (x + (1 << (n - 1))) >> n with an arithmetic shift; sat8 clamps to 0 ... 255; rne = round half to even.
 * (a) map, built once per preparer on the HOST in FP64, no contraction (srl_image_prep_build_map: pure, no device).  For destination
 *     pixel (column j, row i): x = (j - cx) / fx, y = (i - cy) / fy, r2 = x x + y y, kr = 1 + ((k3 r2 + k2) r2 + k1) r2,
 *     xd = x kr + (p1 (2 x y) + p2 (r2 + 2 x x)), yd = y kr + (p1 (r2 + 2 y y) + p2 (2 x y)), u = fx xd + cx, v = fy yd + cy,
 *     iu = rne(u 32), iv = rne(v 32) as int32; map1 = (iu >> 5, iv >> 5) as int16 x 2, each clamped to the int16 range;
 *     map2 = (iv & 31) 32 + (iu & 31) as uint16.  A u or v that is not finite, or |u 32| or |v 32| >= 2^31 - 1: map1 = (-32768, -32768),
 *     map2 = 0 (wholly outside the image).
 * (b) remap, 8 bit x 3 channels, constant border 0: (sx, sy) = map1, ax = map2 & 31, ay = map2 >> 5, w00 = (32 - ax)(32 - ay) 32,
 *     w01 = ax (32 - ay) 32, w10 = (32 - ax) ay 32, w11 = ax ay 32 (sum 32768); per channel
 *     out = (w00 p(sy, sx) + w01 p(sy, sx + 1) + w10 p(sy + 1, sx) + w11 p(sy + 1, sx + 1) + 16384) >> 15, a neighbour outside = 0.
 * (c) gray = (9798 c0 + 19235 c1 + 3735 c2 + 16384) >> 15: the reference calls COLOR_RGB2GRAY on a BGR-held image, so channel 0 gets
 *     the red weight.
 * (d) BGR -> YCrCb, channels b, g, r as they lie: Y = DESCALE(1868 b + 9617 g + 4899 r, 14),
 *     Cr = sat8(DESCALE((r - Y) 11682 + (128 << 14), 14)), Cb = sat8(DESCALE((b - Y) 9241 + (128 << 14), 14)).
 * (e) YCrCb -> BGR: b = sat8(Y + DESCALE((Cb - 128) 29049, 14)), g = sat8(Y + DESCALE((Cb - 128)(-5636) + (Cr - 128)(-11698), 14)),
 *     r = sat8(Y + DESCALE((Cr - 128) 22987, 14)).
 * (f) CLAHE(plane, clip), clip = 3.0 for gray, 1.0 for Y (:124, :195).  T x T tiles, T = max((int)(cols 32.0 / 640), 4) (:169; both
 *     counts from cols) unless opts->tiles gives T.  If cols % T != 0 or rows % T != 0 the plane is extended on the right by T - cols % T
 *     and at the bottom by T - rows % T (a dimension that divided grows by a whole T) with reflect-101 (index 2 (n - 1) - k); otherwise
 *     not at all.  Tile tw x th = extended / T, area = tw th.  Per tile: the 256-bin histogram;
 *     limit = max((int)min(clip area / 256, 2147483647.0), 1) in FP64 (the min first: a large clip saturates at INT32_MAX, the cast is
 *     never out of range); every bin above limit is cut to it, the cuts summed into excess; batch = excess / 256, res = excess - 256 batch; every bin
 *     + batch; if res > 0, step = max(256 / res, 1) and bin i gets + 1 iff i % step == 0 and i / step < res;
 *     lut[i] = sat8(rne((float)cumsum_i (255.0f / (float)area))), quotient and product FP32.  Per pixel (x, y) of the plane, all FP32:
 *     txf = (float)x (1.0f / (float)tw) - 0.5f, tx1 = floor(txf), xa = txf - (float)tx1, xa1 = 1.0f - xa, tx2 = tx1 + 1, then tx1 clamped
 *     up to 0 and tx2 down to T - 1; the same in y;
 *     out = sat8(rne((lut[ty1][tx1][v] xa1 + lut[ty1][tx2][v] xa) ya1 + (lut[ty2][tx1][v] xa1 + lut[ty2][tx2][v] xa) ya)).
 * (r) resize of an 8 bit x 3 channel frame of src_rows x src_cols to the preparer's rows x cols, in front of (b).  Again this library's
 *     operation: it follows OpenCV's conventions for INTER_LINEAR (11-bit coefficients, the two-pass fixed-point rule) and claims no
 *     equality with its bytes.  Tables, built on the HOST, no contraction (srl_image_resize_build_tables: pure, no device), once for
 *     the columns (src_cols -> cols) and once for the rows (src_rows -> rows).  For each destination index d:
 *     scale = (double)src_len / dst_len; f = (float)((d + 0.5) scale - 0.5); s = floor(f); f = f - (float)s, a float subtraction;
 *     if s < 0 then s = 0 and f = 0; if s >= src_len - 1 then s = src_len - 1 and f = 0; ofs[d] = s;
 *     coef[2 d] = rne((1.0f - f) 2048.0f), coef[2 d + 1] = rne(f 2048.0f) as int16.
 *     Pixel rule, per channel, with s1 = min(s + 1, src_len - 1) in either direction, column coefficients a0, a1 and row coefficients
 *     b0, b1: h = S[row][ofs_x] a0 + S[row][s1_x] a1 in int32 for the two rows ofs_y (h0) and s1_y (h1);
 *     out = min(255, ((((b0 (h0 >> 4)) >> 16) + ((b1 (h1 >> 4)) >> 16) + 2) >> 2)).  Every operand is non-negative; the largest
 *     intermediate, 2048 x 32640, fits int32.
 *     Exact half (OpenCV's INTER_AREA substitution): when src_cols == 2 cols and src_rows == 2 rows the result is the 2 x 2 box mean
 *     instead, (s00 + s01 + s10 + s11 + 2) >> 2.
 * The chain: undist = remap(raw); gray_eq = CLAHE(gray(undist), 3.0); bgr_eq = YCrCb->BGR(CLAHE(Y, 1.0), Cr, Cb) of undist.  Integer
 * arithmetic and uncontracted IEEE FP32: the same input gives the same bytes, call after call.
 *
 * srl_image_prepare copies the raw image through page-locked staging (one upload), runs the chain on the device and keeps both results;
 * when the context has a colour map, bgr_eq is left as the map's image exactly as if handed to srl_color_image_upload (the colour state
 * is allocated on the first image) and info->installed_color = 1.  Synchronous.  srl_image_prep_download: which = 0 gray_eq (rows x cols),
 * 1 bgr_eq (rows x cols x 3).  srl_flow_track_prepared is srl_flow_track_image with the prepared gray_eq as its image and no host round
 * trip (first image of a tracker: next = prev, *n_tracked = 0, as there).
 * srl_image_prepare_resized is srl_image_prepare for a frame of any size: the frame is uploaded once at its own size, resized on the
 * device by (r) into the place of the preparer's upload, and the chain runs on that.  With src_rows == rows and src_cols == cols no
 * resize runs and every stage is bytewise srl_image_prepare's.  The tables live on the device, built at the first use of a source size
 * and rebuilt when it changes; the source's staging and device block come with the first resized frame and only grow.  Refused with
 * SRL_ERR_BAD_ARG: a NULL image, src_rows or src_cols < 1 or > SRL_FLOW_MAX_EXTENT, src_rows * src_cols > SRL_COLOR_IMAGE_MAX_PIXELS,
 * row_stride_bytes < 3 src_cols; everything else as srl_image_prepare, the prepared images staying as they were.
 * srl_image_resize_build_tables refuses src_len < 1, dst_len < 1 and NULL arrays (SRL_ERR_BAD_ARG, the arrays left alone).
 * Before a device is touched -- SRL_ERR_BAD_ARG: NULL arguments (info may be NULL); rows or cols outside 16 ... SRL_FLOW_MAX_EXTENT;
 * rows * cols > SRL_COLOR_IMAGE_MAX_PIXELS; rows <= T or cols <= T (the reflection would leave the image); tiles given and below 2 or
 * above min(rows, cols) / 2; intrinsics or coefficients that are not finite, fx or fy equal to 0, a clip that is not finite and positive;
 * row_stride_bytes below a row; an image whose size differs from the preparer's (or, for srl_flow_track_prepared, from the tracker's
 * first image); a second create; n as for srl_flow_track_image.  SRL_ERR_NO_MAP: no preparer, or srl_flow_track_prepared without a
 * tracker.  SRL_ERR_NO_SWEEP: a download or srl_flow_track_prepared before the first image.  SRL_ERR_UNSUPPORTED: more than one rank.
 * A refused srl_image_prepare zeroes *info and leaves the previous results in place.  Every call cancels an armed launch;
 * srl_ctx_destroy frees the preparer.  Device memory: 16 bytes per pixel and 512 T T bytes of look-up tables (2 MB at T = 64); the resize adds 8 bytes per row and per column of tables and 3 bytes per source pixel. */
typedef struct srl_image_prep_opts {
    int32_t rows, cols;
    double fx, fy, cx, cy;
    double dist[5];                 /* k1 k2 p1 p2 k3 */
    double clip_gray, clip_color;   /* 3.0, 1.0 */
    int32_t tiles, reserved;        /* 0 = the reference's rule */
} srl_image_prep_opts;
typedef struct srl_image_prep_info { int32_t tiles, tile_w, tile_h, ext_rows, ext_cols, limit_gray, limit_color, installed_color; } srl_image_prep_info;
void srl_image_prep_opts_default(srl_image_prep_opts *o);      /* clips 3.0 / 1.0, everything else 0 */
int srl_image_prep_build_map(const srl_image_prep_opts *o, int16_t *map1 /* rows x cols x 2 */, uint16_t *map2 /* rows x cols */);   /* host only */
int srl_image_prep_create(srl_ctx *ctx, const srl_image_prep_opts *o);
int srl_image_prep_destroy(srl_ctx *ctx);
int srl_image_prepare(srl_ctx *ctx, const uint8_t *raw_bgr, int rows, int cols, int64_t row_stride_bytes, srl_image_prep_info *info /* or NULL */);
int srl_image_resize_build_tables(int src_len, int dst_len, int32_t *ofs /* dst_len */, int16_t *coef /* dst_len x 2 */);   /* host only */
int srl_image_prepare_resized(srl_ctx *ctx, const uint8_t *raw_bgr, int src_rows, int src_cols, int64_t row_stride_bytes, srl_image_prep_info *info /* or NULL */);
int srl_image_prep_download(srl_ctx *ctx, int which /* 0 gray_eq, 1 bgr_eq */, uint8_t *out, int64_t row_stride_bytes);
int srl_flow_track_prepared(srl_ctx *ctx, const float *prev_xy, int n, float *next_xy, uint8_t *status, int *n_tracked);

/* ------------------------------------------------------------------ compressed camera frames: baseline JPEG into the image preparer
 * replaces: lioOptimization::compressedImageHandler (lioOptimization.cpp:640-664), whose cv_bridge::toCvCopy(msg, BGR8) decodes a
 * sensor_msgs/CompressedImage on the host.  The decode is split where the format splits: the entropy-coded scan is ONE sequential bit
 * stream and is decoded on the host (srl_jpeg_parse, srl_jpeg_entropy_decode: plain C++, no device, no allocation); everything behind
 * it is independent per block and per pixel and runs on the device.  The operations are libjpeg's default decode path -- JDCT_ISLOW,
 * "fancy" triangle upsampling, the 16-bit fixed-point colour tables -- which is integer arithmetic from the coefficient to the byte and
 * is restated here in full; tests/jpeg_checker.py restates it independently and is compared bytewise with libjpeg-turbo's decode.
 * Accepted: SOF0 with 8-bit samples and 8-bit quantisation tables; one component, or three with luma sampling 1x1, 2x1 or 2x2 and
 * chroma 1x1 (4:4:4, 4:2:2, 4:2:0); one scan that holds every component in the frame's order; any restart interval; APPn, COM and other
 * segments with a length are skipped.  SRL_ERR_UNSUPPORTED: every other frame type (extended, progressive, lossless, arithmetic), another
 * sample precision, 16-bit tables, two or four components, any other sampling (4:4:0, 4:1:1), a scan that holds fewer components than the
 * frame, zero rows (DNL).  SRL_ERR_BAD_ARG, everything malformed: NULL arguments; no SOI; a segment length beyond the buffer; a marker
 * that carries no segment in front of the scan; a second SOF0 or SOS before SOF0; zero columns or components; sampling factors outside
 * 1 ... 4; table selectors above 3; Huffman counts that form no prefix code; a table the scan names but no segment defined; Ss, Se, Ah, Al
 * other than 0, 63, 0; in the scan: a code that is in no table, a DC category above 15, a DC value leaving int16_t, a run past coefficient
 * 63 (a ZRL that reaches it included), a restart marker that is missing, wrong, or preceded by a whole unread byte, data ending before
 * the last MCU (after the last byte nothing is invented); capacity_blocks below info->total_blocks; an *info that is not this stream's.
 * srl_jpeg_info: the sampling factors of one component read 1 x 1 (its scan is not interleaved); MCUs are 8 h[0] x 8 v[0] pixels;
 * blocks[c] = mcus_per_row h[c] mcus_per_col v[c] blocks of 64 coefficients, the component plane padded to whole MCUs; scan_offset is
 * the first entropy-coded byte.  A refused srl_jpeg_parse leaves *info untouched.
 * srl_jpeg_entropy_decode writes the QUANTISED coefficients in natural (row-major) order, the zig-zag undone while storing: component
 * after component, within one the blocks in raster order of its padded plane (block (by, bx) at by mcus_per_row h[c] + bx).  DC
 * prediction per component, reset at every RSTn.  qt[c] is component c's quantisation table in natural order (rows of absent components
 * are left alone).  Refusals found before the scan's first bit leave coef and qt untouched; a refusal inside the scan leaves coef partly
 * decoded (it is decoded in place, in one pass) and qt untouched.  The decoder never reads at or beyond bytes + n.
 *
 * Device operations, integer arithmetic only, no atomics: the same bytes call after call.  >> is an arithmetic shift.
 * (i) IDCT per block (jidctint.c), d[r][c] = coef[r][c] qt[r][c], CONST_BITS 13, PASS1_BITS 2, DESCALE(x, n) = (x + (1 << (n - 1))) >> n.
 *     One 1-D pass on eight values d0 ... d7:
 *       z1 = (d2 + d6) 4433; t2 = z1 - d6 15137; t3 = z1 + d2 6270; t0 = (d0 + d4) << 13; t1 = (d0 - d4) << 13;
 *       t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2;
 *       z1 = d7 + d1; z2 = d5 + d3; z3 = d7 + d3; z4 = d5 + d1; z5 = (z3 + z4) 9633;
 *       o0 = d7 2446; o1 = d5 16819; o2 = d3 25172; o3 = d1 12299; z1 = -z1 7373; z2 = -z2 20995; z3 = -z3 16069 + z5; z4 = -z4 3196 + z5;
 *       o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
 *       out0, out7 = t10 +- o3; out1, out6 = t11 +- o2; out2, out5 = t12 +- o1; out3, out4 = t13 +- o0, each DESCALEd.
 *     Pass 1 runs on every COLUMN with DESCALE by 11, pass 2 on every ROW of pass 1's results with DESCALE by 18 (the order is part of
 *     the bytes: pass 1 rounds).  sample = limit(result & 0x3FF), libjpeg's range-limit table taken literally through its index:
 *     index < 128: index + 128; < 512: 255; < 896: 0; otherwise index - 896 -- a clamp of result + 128 to 0 ... 255 for every stream
 *     an encoder produces, and defined for every input.  The arithmetic is 64-bit (libjpeg's JLONG); 32-bit registers give the same
 *     values while no intermediate leaves int32_t, which the library proves per frame from the largest block sum of |d| and
 *     otherwise does not assume.  Sample (y, x) of a component plane comes from block (y / 8, x / 8).
 * (ii) upsampling of the chroma planes on their REAL size cw = ceil(cols / 2) (and ch = ceil(rows / 2) at 2x2), never the padded one.
 *     2x1 (h2v1 fancy), chroma row = image row: out[2 i] = (3 C[i] + C[i - 1] + 1) >> 2, out[2 i + 1] = (3 C[i] + C[i + 1] + 2) >> 2,
 *     except out[0] = C[0] and out[2 cw - 1] = C[cw - 1].
 *     2x2 (h2v2 fancy): image row y reads chroma rows near = y / 2 and far = near - 1 (y even) or near + 1 (y odd), far clamped to
 *     0 ... ch - 1; S[i] = 3 C[near][i] + C[far][i]; out[2 i] = (3 S[i] + S[i - 1] + 8) >> 4, out[2 i + 1] = (3 S[i] + S[i + 1] + 7) >> 4,
 *     except out[0] = (4 S[0] + 8) >> 4 and out[2 cw - 1] = (4 S[cw - 1] + 7) >> 4.  1x1: the sample itself.
 * (iii) YCbCr -> BGR with FIX(x) = (int)(x 65536 + 0.5): R = Y + ((91881 (Cr - 128) + 32768) >> 16), B = Y + ((116130 (Cb - 128) + 32768) >> 16),
 *     G = Y + ((-22554 (Cb - 128) - 46802 (Cr - 128) + 32768) >> 16), each clamped to 0 ... 255 and stored B, G, R.  One component:
 *     B = G = R = Y (what toCvCopy(..., BGR8) makes of a gray image).
 *
 * srl_jpeg_decode parses and entropy-decodes into page-locked staging, makes ONE upload (the tables and the coefficients) and runs the
 * kernels; the BGR frame, rows x cols x 3 packed, stays on the device.  Synchronous.  The decoder object belongs to the context: it comes
 * with the first call, grows by doubling and goes with srl_ctx_destroy.  srl_jpeg_download returns the frame of the last successful
 * decode (SRL_ERR_NO_SWEEP before it; SRL_ERR_BAD_ARG: NULL, a stride below 3 cols).
 * srl_image_prepare_jpeg is srl_jpeg_decode followed by the preparer's chain on the decoded frame where it lies, no host round trip:
 * srl_image_prepare's path when the frame has the preparer's size, srl_image_prepare_resized's otherwise.  Every stage and both results
 * are bytewise what those calls give for the raw frame srl_jpeg_download returns.
 * Refusals of all three, beside the stream's own above: NULL ctx or bytes, n < 2: SRL_ERR_BAD_ARG; rows or cols above
 * SRL_FLOW_MAX_EXTENT or rows * cols > SRL_COLOR_IMAGE_MAX_PIXELS: SRL_ERR_UNSUPPORTED; more than one rank: SRL_ERR_UNSUPPORTED;
 * srl_image_prepare_jpeg without a preparer: SRL_ERR_NO_MAP, before the stream is read.  A refused call zeroes *info
 * and leaves the previous decoded frame and the previous prepared images in place.  Every call cancels an armed launch. */
typedef struct srl_jpeg_info {
    int32_t rows, cols, components;             /* components: 1 or 3 */
    int32_t h[3], v[3];                         /* sampling factors; absent components 0 */
    int32_t mcus_per_row, mcus_per_col;
    int32_t restart_interval;                   /* MCUs between restart markers, 0: none */
    int32_t reserved[2];
    int64_t blocks[3], total_blocks;            /* 64-coefficient blocks per component (padded to whole MCUs) and their sum */
    int64_t scan_offset;
} srl_jpeg_info;
int srl_jpeg_parse(const uint8_t *bytes, int64_t n, srl_jpeg_info *info);   /* host only */
int srl_jpeg_entropy_decode(const uint8_t *bytes, int64_t n, const srl_jpeg_info *info, int16_t *coef /* capacity_blocks x 64 */, int64_t capacity_blocks,
                            uint16_t qt[3][64]);   /* host only */
int srl_jpeg_decode(srl_ctx *ctx, const uint8_t *bytes, int64_t n, srl_jpeg_info *info /* or NULL */);
int srl_jpeg_download(srl_ctx *ctx, uint8_t *out /* rows x cols x 3, B G R */, int64_t row_stride_bytes);
int srl_image_prepare_jpeg(srl_ctx *ctx, const uint8_t *bytes, int64_t n, srl_image_prep_info *info /* or NULL */);

/* ------------------------------------------------------------------ colour voxel map: the coloured cloud
 * replaces: the loops of lioOptimization::pubColorPoints (lioOptimization.cpp:1210-1241), threadPubColorPoints (:1243-1344) and
 * saveColorPoints (:1386-1426) over rgb_points_vec: a point is left out iff N_rgb < pub_point_minimum_views (:1221, :1281, :1404), every
 * other one becomes a pcl::PointXYZRGB.  ROS messages, topics, sleeping and the PCD file stay with the caller.
 * The call covers rgb_points_vec[first .. first + count); count < 0 = to the end of the list as it is at the call.  The range is walked
 * ascending, or descending when `reverse` is set (saveColorPoints walks down).  Record k is the k-th kept point of the walk:
 *   x, y, z = the stored FP32 position (getPosition() followed by the float assignment of :1225-1227 is the identity);
 *   r = (uint8_t) rgb[2], g = (uint8_t) rgb[1], b = (uint8_t) rgb[0] (:1228-1230), each defined here as the low 8 bits of the int16 --
 *   the reference's double -> uint8_t for 0 ... 255, where updateRgb keeps colours (a truncated weighted mean of bytes); a = 255;
 *   point_index[k], when requested, is the registered index of record k.
 * The record is meant as PCL's PointXYZRGB: the fields x y z rgb packed to 16 bytes, the rgb word holding b, g, r, a from the low byte,
 * a = 255 as PCL's constructor sets it.  PCL is not part of this tree and the stand-in pcl::PointXYZRGB of oracle/ref_shim is not PCL:
 * nothing here can confirm that layout, so check it against the PCL you link before you reinterpret the records.
 * `since` additionally leaves out a point iff last_observe_time < since (counted as stale, among the points that pass the N_rgb test);
 * -inf is the reference's loops, and the time is read only where since > -inf.
 * A map never rendered has no colour state and none is allocated by this call: every N_rgb is 0 and every colour 0, so that with
 * minimum_views <= 0 such a map exports every point black.
 * Synchronous: one wait for the totals, then one DMA of exactly totals->published records, and a second one of as many indices when
 * point_index is given.  out == NULL and point_index == NULL: the totals alone.  capacity (records, and indices) < published:
 * SRL_ERR_BAD_ARG with the totals filled and nothing copied.  The call changes nothing: ask again.  A cloud of up to 1 MiB (records
 * and indices) leaves through page-locked scratch inside the context; a larger one is copied straight into the caller's arrays.
 * Before a device is touched: NULL ctx or opts, first < 0, first + count beyond the list, capacity < 0, NaN since: SRL_ERR_BAD_ARG; no
 * colour map: SRL_ERR_NO_MAP; more than one rank: SRL_ERR_UNSUPPORTED; a range of more than 2^27 points (what one scan handles) is
 * REFUSED with SRL_ERR_UNSUPPORTED, not split: export it in pieces; an empty range: SRL_OK with zero totals.  Cancels an armed launch.
 * Neither map, nor the colour state, the neighbourhood bounds or the taps are touched; scratch comes from the context's pool. */
typedef struct srl_color_cloud_point { float x, y, z; uint8_t b, g, r, a; } srl_color_cloud_point;   /* 16 B */
typedef struct srl_color_cloud_opts {
    int32_t minimum_views;          /* pub_point_minimum_views: a point is left out iff N_rgb < minimum_views (so <= 0 keeps all) */
    int32_t reverse;                /* 0: ascending registered index; != 0: descending (saveColorPoints) */
    double  since;                  /* additionally left out iff last_observe_time < since; -inf = the reference's loops; NaN refused */
} srl_color_cloud_opts;
void srl_color_cloud_opts_default(srl_color_cloud_opts *o);   /* 1 (config/r3live.yaml:76; the class default, parameters.h:106, is 3), 0, -inf */
/* scanned = published + below_views + stale */
typedef struct srl_color_cloud_totals { int64_t scanned, published, below_views, stale; } srl_color_cloud_totals;
int srl_color_map_export_cloud(srl_ctx *ctx, int64_t first, int64_t count, const srl_color_cloud_opts *opts,
                               srl_color_cloud_point *out /* or NULL */, int32_t *point_index /* or NULL */, int64_t capacity,
                               srl_color_cloud_totals *totals /* or NULL */);

/* ------------------------------------------------------------------ sweep
 * replaces: the `keypoints` vector handed to updateIEKF (optimize.cpp:133; point3D::raw_point,
 * cloudMap.h:40).  AoS n x 3 FP64 in the lidar frame, in keypoint order.  Uploaded once per sweep.
 * With a communicator attached this rank keeps the contiguous range [rank*n/R, (rank+1)*n/R). */
int srl_sweep_upload(srl_ctx *ctx, const double *raw_xyz, int n);
/* Page-locked host memory for the sweep: srl_sweep_upload DMAs straight out of a buffer obtained here (or registered with
 * srl_host_register) -- one asynchronous copy on the context's stream, no staging, no synchronisation; such a buffer must stay
 * untouched until the next call that returns results.  From pageable memory the upload goes through a pinned ring inside
 * the context (CPU copy of a chunk overlapped with the DMA of the previous one) and the buffer is free on return. */
int srl_pinned_alloc(size_t bytes, void **out);
/* Blocks until the DMA of the last srl_sweep_upload / srl_sweep_prefetch that read a PAGE-LOCKED caller buffer has finished:
 * after it the buffer may be refilled.  (A result returned by srl_build_residuals implies the same for the
 * sweep it was computed on; a caller that refills its page-locked buffer earlier than that calls this first.  Uploads from
 * pageable memory never need it: the buffer is consumed on return.)  No-op when nothing is pending. */
int srl_sweep_wait(srl_ctx *ctx);
int srl_pinned_free(void *p);
int srl_host_register(void *p, size_t bytes);
int srl_host_unregister(void *p);
/* Thread placement helper for the node's estimation thread (the reference runs it as the ROS node's main thread,
 * src/lioOptimization.cpp:1587-1611): restricts the CALLING thread to the CPUs of the NUMA node the context's GPU hangs off
 * (/sys/bus/pci/devices/<gpu>/local_cpulist).  The solve is a latency-bound host loop -- one mailbox read and one doorbell
 * write per ESIKF iteration --, and from the other socket of a two-socket host every iteration costs ~3 us more.  Optional;
 * returns SRL_ERR_UNSUPPORTED when the topology cannot be read (nothing is changed then).  *numa_node (may be NULL) receives
 * the node. */
int srl_thread_pin_to_gpu_numa(srl_ctx *ctx, int *numa_node);
/* The NEXT sweep while the current one is being solved (a node receives sweep k + 1 during the solve of sweep k):
 * srl_sweep_prefetch uploads it on the context's copy stream into a second sweep buffer and returns at once; the current
 * sweep stays valid.  srl_sweep_swap makes the prefetched sweep current -- the compute stream waits for the upload's event,
 * the host does not; when the upload has already landed, a launch armed behind the previous sweep's last pass is kept and serves
 * as the new sweep's first pass (see ARMED LAUNCHES).  Same buffer rules as srl_sweep_upload (a page-locked source must stay untouched until the first
 * result computed on the swapped-in sweep has been returned). */
int srl_sweep_prefetch(srl_ctx *ctx, const double *raw_xyz, int n);
int srl_sweep_swap(srl_ctx *ctx);
int srl_sweep_shard(srl_ctx *ctx, int *begin, int *count, int *total);

/* ------------------------------------------------------------------ frame-resident pipeline (optional)
 * Keeps the whole reconstructed sweep in HBM from keypoint selection to map insertion.
 * srl_frame_upload            replaces handing p_frame->point_frame (raw points) to optimize() (optimize.cpp:428)
 * srl_frame_select_keypoints  replaces gridSampling / subSampleFrame (utility.cpp:167-201) applied to
 *                             point = R(q) (R_il raw + t_il) + t (utility.cpp:314-318): same keypoints in the same
 *                             (std::tr1::unordered_map iteration) order; they become the resident sweep.  The order is
 *                             computed on the device (csrc/host/tr1_relation.h; frames beyond 131 072 points or buckets, or
 *                             with more than 16 voxels in one bucket of the container, through the host replay of
 *                             csrc/host/tr1_order.h).  keypoint_index == NULL: only the count comes back (the call returns
 *                             while the last kernels of the selection still run; the passes queue behind them) -- the
 *                             index list costs a copy and a stream synchronisation, ask for it only if the caller needs it.
 * srl_frame_commit            replaces the re-transform loop (optimize.cpp:441-445) + addPointsToMap
 *                             (lioOptimization.cpp:520-554) with the final pose, without leaving the device.
 * A page-locked raw_xyz (srl_pinned_alloc) is copied by the DMA engine on the context's copy stream, beside whatever the compute stream
 * still does for the previous frame; the buffer may be refilled once a later call on the context has returned results (or after
 * srl_sweep_wait).  A pageable raw_xyz is consumed before the call returns. */
int srl_frame_upload(srl_ctx *ctx, const double *raw_xyz, int n);

/* Sweep reconstruction: the per-point stages of buildFrame (lioOptimization.cpp:833-850).
 * srl_imu_state mirrors imuState (cloudMap.h:110-122), quat as w x y z.
 * srl_frame_undistort replaces distortFrameByConstant / distortFrameByImu (utility.cpp:203-306) followed by
 *   transformAllImuPoint (utility.cpp:320-332) over ALL n points of the cut sweep: relative_time_ms is
 *   point3D::relative_time (makePointTimestamp, lioOptimization.cpp:786-819), motion_compensation the enum of
 *   include/utility.h:82-86 (SRL_MC_NONE = neither branch of lioOptimization.cpp:833-836 runs).  imu_point_in (or NULL
 *   = zeros) is what imu_point holds before: distortFrameByImu leaves points its interval walk does not reach untouched.
 *   Outputs (optional): point3D::imu_point and the corrected point3D::raw_point, n x 3 each.  The corrected sweep
 *   stays in HBM.
 * srl_frame_take makes the points index[0..m) of the corrected sweep the resident frame (what srl_frame_upload
 *   would upload) -- any index list; buildFrame's shuffle / subSampleFrame / shuffle is srl_frame_subsample +
 *   srl_frame_take_subsampled below (and srl_frame_take with the first shuffle's order when voxel_size <= 0). */
typedef struct srl_imu_state {
    double timestamp;
    double un_acc[3], un_gyr[3], trans[3];
    double quat[4];
    double vel[3];
} srl_imu_state;
enum { SRL_MC_IMU = 0, SRL_MC_CONSTANT_VELOCITY = 1, SRL_MC_NONE = 2 };
int srl_frame_undistort(srl_ctx *ctx, const double *raw_xyz, const double *relative_time_ms, const double *imu_point_in,
                        int n, const srl_imu_state *imu_states, int n_states, double time_frame_begin,
                        int motion_compensation, const double R_il[9], const double t_il[3], double *imu_point_out,
                        double *raw_out);
int srl_frame_take(srl_ctx *ctx, const int32_t *index, int m);
/* buildFrame's subSampleFrame (lioOptimization.cpp:838-846 -> utility.cpp:167-186) on the sweep srl_frame_undistort left in HBM, in place of
 * the host grouping and srl_frame_take's index list.  The two std::shuffle calls stay with the caller (its own engine and library).
 * srl_frame_subsample visits the points in visit_order (n = the undistorted count; a permutation of 0..n-1: the first shuffle), keys each
 *   by its UNCORRECTED point (raw_xyz as srl_frame_undistort received it: point3D::point, cloudProcessing.cpp:143) at sample_size
 *   (short(p / size) per axis), keeps the first visited point of every voxel and orders the voxels as std::tr1::unordered_map iterates
 *   them.  *num_kept = m, the voxel count.  The permutation is checked on the device (SRL_ERR_BAD_ARG if it is none); the order is computed
 *   there as in srl_frame_select_keypoints (srl_debug_frame_order_used reports the path).
 * srl_frame_take_subsampled makes frame point k = kept[perm[k]] the resident frame (perm: the second shuffle over 0..m-1 -- std::shuffle of
 *   the kept list equals this gather with perm = std::shuffle(0..m-1) on the same engine; NULL = container order), and downloads on request
 *   the sweep index (m), the corrected raw_point (m x 3) and imu_point (m x 3) of every frame point.  A perm that is not a permutation
 *   returns SRL_ERR_BAD_ARG and leaves no resident frame; the sub-sample stays and can be taken again.
 * Both return SRL_ERR_NO_SWEEP without an undistorted sweep (or, for the take, without a sub-sample of it), SRL_ERR_BAD_ARG for an n or m
 * that does not match, SRL_ERR_UNSUPPORTED with more than one rank.  srl_frame_undistort may then be called with both outputs NULL. */
int srl_frame_subsample(srl_ctx *ctx, const int32_t *visit_order, int n, double sample_size, int *num_kept);
int srl_frame_take_subsampled(srl_ctx *ctx, const int32_t *perm /* m or NULL */, int m, int32_t *index_out /* m or NULL */,
                              double *raw_out /* m x 3 or NULL */, double *imu_out /* m x 3 or NULL */);
int srl_frame_size(srl_ctx *ctx, int *n);      /* points of the resident frame (capacity needed for keypoint_index) */
int srl_frame_select_keypoints(srl_ctx *ctx, const double q[4], const double t[3], const double R_il[9],
                               const double t_il[3], double sample_voxel_size,
                               int32_t *keypoint_index /* capacity n, or NULL */, int *num_keypoints);
int srl_frame_commit(srl_ctx *ctx, const double q[4], const double t[3], const double R_il[9], const double t_il[3],
                     double voxel_size, int cap, double min_distance_points, int min_num_points,
                     double *world_out /* n x 3 or NULL */, int *num_added /* or NULL */);
/* srl_frame_commit + the report of srl_map_insert_report on the resident frame (ref_z = t[2]; the re-transform stays fused into the
 * insertion's first kernel).  Never deferred, whatever is NULL; world_out is bitwise what srl_frame_commit gives. */
int srl_frame_commit_report(srl_ctx *ctx, const double q[4], const double t[3], const double R_il[9], const double t_il[3],
                            double voxel_size, int cap, double min_distance_points, int min_num_points,
                            double *world_out /* n x 3 or NULL */, uint8_t *outcome /* n or NULL */,
                            srl_cloud_point *cloud /* capacity n, or NULL */, int *num_cloud /* or NULL */, int *num_added /* or NULL */);
/* num_added == NULL (addPointsToMap returns nothing either): the insertion is enqueued behind the re-transform and the call returns as
 * soon as world_out (if asked for) has arrived; the passes of the next sweep are ordered behind the insertion on the context's stream,
 * and the map's totals are brought up to date by the next call that reads them (srl_map_size, srl_map_download, the next insertion). */

/* ------------------------------------------------------------------ Livox messages -> device point queue -> sweeps cut at image times
 * (csrc/srl_points.hip).  Replaces cloudProcessing::livoxHandler (cloudProcessing.cpp:125-214), the point side of getMeasurements
 * (lioOptimization.cpp:672-680, :719-723, :759-763) and makePointTimestamp (:786-819).  The image and IMU queues and the policy of
 * getMeasurements stay with the caller, who is given the three numbers the policy reads of point_buffer (srl_points_info).
 *
 * srl_livox_decode: points = msg->points.data() (srl_livox_point is the in-memory layout of livox_ros_driver::CustomPoint), message index i
 *   from 1 (point 0 is never output).  Valid iff line < n_scans; |x|, |y|, |z| (float magnitude, compared as double) each not > 1e8;
 *   x > 0.7; not (x > 2.0 and (tag & 0x03 or tag & 0x0C)); and one of fabsf(x_i - x_{i-1}), fabsf(y_i - y_{i-1}), fabsf(z_i - z_{i-1}) > 1e-7
 *   (float subtraction against MESSAGE index i - 1, compared as double).  relative_time = double(offset_time) * time_unit_scale; timestamp =
 *   relative_time / 1000.0 + header_stamp.  The valid points are ordered by relative_time ascending, TIES BY MESSAGE INDEX (a stable sort:
 *   the reference's std::sort leaves ties in an order of its library's own; the two agree wherever no two valid points share an
 *   offset_time).  Sorted position j is picked iff (j + 1) % point_filter_num == 0; a picked point is appended to the queue iff
 *   (x x + y y) + z z > blind blind in FP64.  last_end_time = header_stamp + (relative_time of the last sorted valid point) / 1000.0; NaN
 *   when the message has no valid point (the reference reads .back() of an empty vector there).  first / last_timestamp: of the appended
 *   points, NaN when none.  The same message gives the same bytes, call after call.
 *   Synchronous; a page-locked `points` goes by DMA.  Before a device is touched: NULL ctx / opts, point_num < 0, NULL points with
 *   point_num > 0, point_filter_num < 1, n_scans < 0, time_unit_scale not > 0 (NaN included), NaN blind or header_stamp: SRL_ERR_BAD_ARG;
 *   point_num > 2^20: SRL_ERR_UNSUPPORTED; more than one rank: SRL_ERR_UNSUPPORTED.  report may be NULL.  Cancels an armed launch.
 * srl_time_unit_scale: cloudProcessing::setTimeUnit's float literal widened to double (unit 0 s: 1.e3f, 1 ms: 1.f, 2 us: 1.e-3f, 3 ns:
 *   1.e-6f, anything else: 1.f) -- 1.e-6f is not 1e-6.
 * The queue is a FIFO in HBM the context owns (grown by doubling; the order never changes).  srl_points_info: its size and the timestamps
 *   of its front and back (NaN when empty), from what the decode and cut reports already returned -- no device synchronisation.
 * srl_points_cut: while (front().timestamp < t) pop -- the longest PREFIX whose every timestamp is < t; it stops at the first element that
 *   fails even if later ones would pass.  An empty queue, or every element passing: everything is cut.  The cut points stay in HBM as THE
 *   RESIDENT CUT until the next cut.  report (may be NULL): the count and the new front timestamp (NaN: the queue is empty now).
 * srl_frame_undistort_cut: makePointTimestamp on the resident cut -- relative = timestamp - time_begin; alpha = relative / (time_end -
 *   time_begin); relative *= 1000.0; with point_time_enable every point is kept and alpha > 1.0 becomes 1.0 - 1e-5, otherwise points with
 *   timestamp > time_end or < time_begin are removed (stable, no clamp) -- then srl_frame_undistort's kernel with time_frame_begin =
 *   time_begin and imu_point_in = zeros.  *n = the points that remain.  The corrected sweep is where srl_frame_subsample, srl_frame_take and
 *   srl_frame_take_subsampled look for it.  SRL_MC_IMU: the interval of every point is found on the device (the smallest k with t <
 *   stamp[k + 1] + 1e-6, accepted iff t > stamp[k] - 1e-6; the first point without one and every point behind it get none) where the
 *   rewritten times and the state stamps are non-decreasing; otherwise the times are downloaded and the walk is replayed on the host as
 *   in srl_frame_undistort (srl_debug_points_fallbacks counts these) -- the result is the same.
 * srl_frame_point_times: timestamp, relative_time (ms) and alpha_time of the points index[0..m) of that sweep (each output optional).
 * SRL_ERR_NO_SWEEP: srl_points_info / _clear / _cut before the first srl_livox_decode; srl_frame_undistort_cut without a cut;
 *   srl_frame_point_times without a sweep undistorted from a cut. */
typedef struct srl_livox_point { uint32_t offset_time; float x, y, z; uint8_t reflectivity, tag, line, pad; } srl_livox_point;   /* 20 B */
typedef struct srl_livox_opts { int32_t n_scans, reserved0; double time_unit_scale; double blind; int32_t point_filter_num, reserved1; } srl_livox_opts;
typedef struct srl_livox_report { int32_t valid, picked, appended, reserved; double last_end_time, first_timestamp, last_timestamp; } srl_livox_report;
typedef struct srl_points_cut_report { int32_t count, reserved; double front_timestamp; } srl_points_cut_report;
double srl_time_unit_scale(int unit);
int srl_livox_decode(srl_ctx *ctx, const srl_livox_point *points, int point_num, double header_stamp, const srl_livox_opts *opts,
                     srl_livox_report *report);
int srl_points_info(srl_ctx *ctx, int *size, double *front_timestamp, double *back_timestamp);
int srl_points_clear(srl_ctx *ctx);
int srl_points_cut(srl_ctx *ctx, double t, srl_points_cut_report *report);
int srl_frame_undistort_cut(srl_ctx *ctx, double time_begin, double time_end, int point_time_enable, const srl_imu_state *imu_states,
                            int n_states, int motion_compensation, const double R_il[9], const double t_il[3], int *n);
int srl_frame_point_times(srl_ctx *ctx, const int32_t *index, int m, double *timestamp /* m or NULL */, double *relative_time /* m or NULL */,
                          double *alpha_time /* m or NULL */);

/* ------------------------------------------------------------------ PointCloud2 messages (Velodyne, Ouster, RoboSense) -> the same device
 * point queue (csrc/srl_pc2.hip, csrc/srl_pc2_layout.cpp).  Replaces cloudProcessing::process (cloudProcessing.cpp:100-123) with its three
 * handlers: velodyneHandler (:325-433), ousterHandler (:216-323), robosenseHandler (:435-542).  Everything behind the queue (srl_points_cut,
 * srl_frame_undistort_cut) is the Livox path's.
 *
 * srl_pc2_layout is what pcl::fromROSMsg reads of a sensor_msgs::PointCloud2: point i of n = width * height lies at (i / width) * row_step +
 *   (i % width) * point_step, its fields at the byte offsets given (no alignment needed: the kernels assemble unaligned fields from bytes).
 *   The datatypes are the reference's registered point structs (cloudProcessing.h:50-114), fixed by lidar_type: x, y, z float32 always;
 *   2 VELO: time float32, ring uint16.  3 OUST: t uint32, ring uint8.  4 ROBO: timestamp float64, ring uint16.  `data` goes up once, as it is.
 * srl_pc2_decode: last_end_time is the member the reference carries from message to message (-1 at construction): the caller passes what
 *   the previous report gave.  given_offset_time = (time field of the LAST point in message order) > 0, decided before any sort (a NaN
 *   there: 0).
 *   given_offset_time = 1: the points are ordered by the time field ascending, TIES BY MESSAGE INDEX (a stable sort; the reference's
 *     std::sort leaves ties in an order of its library's own -- every Ouster column shares one t).  relative_time of sorted position j:
 *     double(time) * time_unit_scale (VELO, OUST); (timestamp_j - timestamp_sorted[0]) * time_unit_scale (ROBO).  Position j is picked iff
 *     j % point_filter_num == 0; a picked point is appended iff (x x + y y) + z z > blind blind in FP64 and timestamp = relative_time / 1000.0 +
 *     header_stamp > last_end_time.  dt_last_point = the sorted last point's double(time) * time_unit_scale -- for ROBO its ABSOLUTE
 *     timestamp * time_unit_scale, not the difference (the reference's statement at :456, reproduced).
 *   given_offset_time = 0: yaw = atan2(double(y), double(x)) * 57.2957 per point, computed ON THE HOST with libm (srl_pc2_yaw_angles: the
 *     reference's bits are its libm's) and uploaded beside the message.  The first point of every ring in message order has relative_time =
 *     0.0 and timestamp = 0.0 (the reference never assigns it: such a point passes the last_end_time test only while that is negative); every
 *     other point has relative_time = (yaw_first - yaw) / omega if yaw <= yaw_first, else (yaw_first - yaw + 360.0) / omega, omega = 0.361 *
 *     scan_rate, timestamp = relative_time / 1000.0 + header_stamp.  Stable sort by relative_time; position j is picked iff j %
 *     point_filter_num == 0 and appended iff timestamp > last_end_time (NO blind test in this branch).  dt_last_point = the sorted last
 *     relative_time.
 *   report->last_end_time = header_stamp + dt_last_point / 1000.0.  points = n; picked = positions with j % point_filter_num == 0; first /
 *   last_timestamp: of the appended points, NaN when none.  The same call gives the same bytes, every time.
 *   n == 0: SRL_OK, nothing queued, report->last_end_time NaN (the reference returns before it assigns: the caller keeps its value).
 *   SRL_ERR_BAD_ARG with nothing queued: NULL ctx / layout / opts / data; is_bigendian != 0; a field that does not fit inside point_step;
 *   data_bytes short of the last point's end; lidar_type other than 2, 3, 4; point_filter_num < 1; time_unit_scale not positive and finite;
 *   NaN blind, header_stamp or last_end_time; yaw branch: scan_rate <= 0, n_scans < 1, a ring >= n_scans (the reference indexes out of
 *   bounds); a NaN sort key (given branch: any NaN time; yaw branch: a NaN relative_time) -- std::sort under < is undefined there.  The
 *   last two are found on the device; the queue's size lives on the host and is simply not advanced.  n > 2^20 or more than one rank:
 *   SRL_ERR_UNSUPPORTED.  Synchronous.  report may be NULL.  Cancels an armed launch.  The first call creates the queue, as the first
 *   srl_livox_decode does (srl_points_info and the others answer SRL_ERR_NO_SWEEP before either).
 * srl_pc2_yaw_angles: yaw[i] = atan2(double(y_i), double(x_i)) * 57.2957 for the n points of the layout; a pure host function (no HIP call,
 *   the coordinates are read with memcpy).  SRL_ERR_BAD_ARG as above for the layout, data_bytes and NULL pointers. */
typedef struct srl_pc2_layout {
    uint32_t width, height, point_step, row_step;
    int32_t  off_x, off_y, off_z, off_time, off_ring;   /* byte offsets inside one point */
    int32_t  is_bigendian;                               /* must be 0 */
} srl_pc2_layout;                                        /* 40 B */
typedef struct srl_pc2_opts {
    int32_t lidar_type;              /* cloudProcessing.h:25: 2 VELO, 3 OUST, 4 ROBO; 1 (LIVOX) and others refused */
    int32_t n_scans, scan_rate, point_filter_num;
    double  time_unit_scale, blind;
} srl_pc2_opts;                                          /* 32 B */
typedef struct srl_pc2_report {
    int32_t points, given_offset_time, picked, appended;
    double  last_end_time, first_timestamp, last_timestamp;
} srl_pc2_report;                                        /* 40 B */
int srl_pc2_decode(srl_ctx *ctx, const void *data, size_t data_bytes, const srl_pc2_layout *layout, double header_stamp,
                   double last_end_time, const srl_pc2_opts *opts, srl_pc2_report *report);
int srl_pc2_yaw_angles(const void *data, size_t data_bytes, const srl_pc2_layout *layout, double *yaw);

/* ------------------------------------------------------------------ hot path
 * replaces: lioOptimization::buildPlaneResiduals (optimize.cpp:18-131) incl. searchNeighbors
 * (:365-426), computeNeighborhoodDistribution (:316-353), and the H_x^T H_x / H_x^T h contraction
 * of updateIEKF (:235,:239).  One call per ESIKF iteration.  With a communicator the result is
 * all-reduced (RCCL) and identical on every rank.  Returns SRL_OK even when out->success == 0. */
int srl_build_residuals(srl_ctx *ctx, const srl_frame *frame, const srl_icp_opts *opts, srl_normal_eq *out);
/* The same call with a host callback that runs ONCE while the kernels are in flight (after the launches are enqueued,
 * before the result is awaited): updateIEKF's part of the 17-dim algebra that does not depend on H_x -- the prior error
 * state, the covariance projection and the first of the two 17x17 inverses, src/optimize.cpp:172-234 -- fits there, so
 * only the second inverse and the gain (src/optimize.cpp:235-244) remain behind the kernel.  fn may be NULL. */
typedef void (*srl_overlap_fn)(void *user);
int srl_build_residuals_overlap(srl_ctx *ctx, const srl_frame *frame, const srl_icp_opts *opts, srl_normal_eq *out,
                                srl_overlap_fn fn, void *user);
/* ARMED LAUNCHES.  The loop of updateIEKF (src/optimize.cpp:147-312) alternates kernel and host: buildPlaneResiduals' normal
 * equations (:153,:235,:239) -> 17-dim update (:172-261) -> next pose -> buildPlaneResiduals.  With armed launches on (the
 * default) an srl_build_residuals call on an unsharded context, besides running its own pass, enqueues the kernel of the NEXT
 * pass while the current one is in flight -- same map and options; the pose, which does not exist yet, arrives later through a
 * small host-written "pose box" the waiting workgroups poll, together with the keypoint count and which of the context's two
 * sweep buffers (srl_sweep_prefetch / srl_sweep_swap) the pass runs on.  The next call, if its arguments are those of the armed
 * launch (pose, sweep buffer and count may differ: that is the point), only writes the box: the launch call, the dispatch and the
 * ramp of the kernel are off the per-iteration critical path -- also across srl_sweep_swap, where the launch armed behind the last
 * pass of sweep k becomes the first pass of sweep k + 1 (src/lioOptimization.cpp:1003-1027: one optimize() per sweep).  Any other
 * call on the context, or a pass with other arguments, cancels the armed launch first (one 384-byte write; the waiting kernel
 * exits), so nothing observable changes: same kernels, same arithmetic, same results.
 * PROCESS-WIDE EFFECT: a waiting launch keeps one workgroup per compute unit resident.  Other work for the same GPU -- another
 * context or process, a foreign hipDeviceSynchronize / hipFree -- waits until the launch is fired, cancelled or leaves by itself
 * (300 us after it started waiting; a call arriving more than 150 us after arming cancels instead of firing).  Therefore a launch
 * is only armed where it is likely to fire: not behind the pass expected to be the last of a solve (the pass count of the
 * previous solve, told by srl_solve_end) unless a prefetched sweep is waiting, and not while a second context of this process
 * lives on the device.
 *   srl_set_armed_launch(ctx, 0 | 1 | 2)  off / on with the policy above (default) / armed behind every eligible pass
 *   srl_solve_end(ctx)                 the caller's ESIKF loop on the current sweep has ended (converged, iteration cap, failure):
 *                                      remembers how many passes it took and cancels an armed launch unless a prefetched sweep
 *                                      is waiting.  Optional (without it every eligible pass arms, as with mode 2).
 *   srl_disarm(ctx)                    cancel an armed launch now (optional: e.g. before the thread goes idle)
 *   srl_get_arm_stats                  counters {armed, fired, cancelled, expired} since context creation */
int srl_set_armed_launch(srl_ctx *ctx, int mode);
int srl_solve_end(srl_ctx *ctx);
int srl_disarm(srl_ctx *ctx);
int srl_get_arm_stats(srl_ctx *ctx, uint64_t out[4]);

/* enable/disable the per-keypoint parity taps written by srl_build_residuals (off by default) */
int srl_set_taps(srl_ctx *ctx, int enable);

/* parity taps for the LAST srl_build_residuals on this rank's shard (any pointer may be NULL).
 * status: 0 = < min_number_neighbors, 1 = plane built but distance gate rejected, 2 = accepted,
 * 3 = not visited by the sequential loop (after the max_num_residuals cut-off). */
int srl_fetch_neighbors(srl_ctx *ctx, int32_t *ids /* n x K, -1 padded */, uint8_t *status /* n */,
                        int32_t *num_candidates /* n */);
int srl_fetch_residuals(srl_ctx *ctx, double *normal /* n x 3 */, double *a2D, double *weight,
                        double *norm_offset, double *distance, double *jacobian /* n x 6 */);

/* replaces: lioOptimization::searchNeighbors for a batch of WORLD points (optimize.cpp:365-426) */
int srl_search_neighbors(srl_ctx *ctx, const double *world_xyz, int n, int nb_voxels_visited,
                         double size_voxel_map, int max_num_neighbors, int threshold_voxel_capacity,
                         int32_t *ids /* n x K */, float *nb_xyz /* n x K x 3, may be NULL */,
                         int32_t *num_found /* n */);

/* replaces: the re-transform loop at the end of optimize() (optimize.cpp:441-445 -> utility.cpp:314-318):
 * out = R(q) * (R_il * raw + t_il) + t for n points (AoS, host buffers). */
int srl_transform_points(srl_ctx *ctx, const double *raw_xyz, int n, const double q[4], const double t[3],
                         const double R_il[9], const double t_il[3], double *out_xyz);

/* ------------------------------------------------------------------ multi-GPU (RCCL over xGMI)
 * one context per process/GPU; the only exchange step is the all-reduce of the normal equations.
 *
 * SHARD LAYOUT.  A sweep is cut when it becomes current: srl_sweep_upload and srl_sweep_prefetch keep the range
 * srl_shard_range(n, nranks, rank) of the layout in force at that call.  Every call that changes (nranks, rank) -- srl_comm_init_rank,
 * srl_comm_destroy, srl_comm_suspend, srl_comm_set_host_callbacks, srl_peer_attach, srl_peer_detach, srl_debug_set_gather_counts --
 * leaves the current and the prefetched sweep cut under the OLD layout: upload the sweep again afterwards.  srl_build_residuals checks
 * it on the host (one comparison per pass): when the current sweep's range is not the one this rank owns under the present layout it
 * returns SRL_ERR_NO_SWEEP with a zeroed record and an srl_last_error that names both ranges, before anything is launched or exchanged;
 * a sweep prefetched under the old layout is refused the same way once srl_sweep_swap has made it current.  A change that leaves this
 * rank's range as it was (one rank before and after) needs no upload. */
#define SRL_COMM_ID_BYTES 128
int srl_comm_unique_id(void *id /* SRL_COMM_ID_BYTES */);
/* debug / test hook: take the nccl* entry points of this process from the given shared object instead of the process's RCCL.  Only
 * before the first communicator call (SRL_ERR_BAD_ARG afterwards: one instance per process).  tests/fake_rccl/libfake_rccl.so -- ranks
 * as processes meeting in shared memory, collectives stream-ordered through host callbacks -- lets the N > 1 sequencing of
 * srl_build_residuals (count all-gather -> reduce kernel -> all-reduce of 50 doubles -> publish, src/optimize.cpp:107,235,239 across
 * shards) run on a one-GPU box, where RCCL itself refuses two ranks per device. */
int srl_comm_set_library(const char *path);
int srl_comm_init_rank(srl_ctx *ctx, int nranks, int rank, const void *id);
int srl_comm_destroy(srl_ctx *ctx);
/* Which RCCL the communicator calls run on.  The library does not link librccl: it uses the RCCL instance the process has
 * already loaded (a PyTorch process: torch/lib/librccl.so) or, when there is none, dlopens librccl.so.1 -- one instance per
 * process, never two.  origin = path of that shared object, version = ncclGetVersion, preloaded = 1 when it was found in the
 * process.  SRL_ERR_COMM (origin = reason) when no RCCL is available; single-GPU use never needs one. */
int srl_comm_backend_info(char *origin, int origin_len, int *version, int *preloaded);
/* What the sharded path of this context runs on, for a run that has to explain itself (bench.py prints it for every --gpus N line):
 * transport 0 none (unsharded), 1 RCCL all-reduce, 2 direct peer exchange, 3 host callbacks; nranks / rank as attached; ranks_seen = the
 * communicator's own count (ncclCommCount) or the number of peer inboxes mapped -- equal to nranks when every rank really joined;
 * passes_armed = armed launches fired on this context so far (0 on a path that never arms).  Any pointer may be NULL. */
int srl_comm_info(srl_ctx *ctx, int *transport, int *nranks, int *rank, int *ranks_seen, int64_t *passes_armed);
/* suspend != 0: run unsharded (whole sweep, no collective) while keeping the communicator; 0: back to sharded mode.
 * Changes the shard layout: upload the sweep again after switching (SHARD LAYOUT above; a pass over the old range is refused). */
int srl_comm_suspend(srl_ctx *ctx, int suspend);
/* test hook: a host all-reduce callback (sum over ranks of `count` doubles, in place) used INSTEAD of
 * RCCL when set -- lets the sharded logic run over gloo/MPI or G logical shards on one device.  Sets the shard layout
 * (nranks, rank): upload the sweep afterwards (SHARD LAYOUT above). */
typedef int (*srl_allreduce_fn)(double *buf, int count, void *user);
typedef int (*srl_allgather_i64_fn)(const int64_t *mine, int64_t *all /* nranks */, void *user);
int srl_comm_set_host_callbacks(srl_ctx *ctx, int nranks, int rank, srl_allreduce_fn ar,
                                srl_allgather_i64_fn ag, void *user);

/* Direct peer exchange: the sum over the point-range shards (optimize.cpp:235,239 see the sum of all residuals) WITHOUT an
 * RCCL call on the data path -- the alternative of SURVEY.md 5 for one node.  Every rank owns an inbox in fine-grained device
 * memory; per pass each rank's finishing workgroup stores its 50-double row, as tagged 8-byte granules, into the inbox of every
 * rank over xGMI and adds the rows it received in rank order (the same bits on every rank).  A sharded pass then is still ONE
 * kernel; with the ordered cut (max_num_residuals can bind) the per-rank counts travel the same way, followed by the reduce
 * kernel and a one-wave exchange kernel.
 *   srl_peer_export : creates the inbox on first use and RESETS it (a new session: call it before every attachment, on every
 *                     rank, before the handles are exchanged -- never while peers are attached); ipc_handle
 *                     (SRL_PEER_HANDLE_BYTES, may be NULL) receives its HIP IPC handle for peers in OTHER processes,
 *                     *local_ptr (may be NULL) the device pointer for peers in the SAME process.
 *   srl_peer_attach : ipc_handles = nranks x SRL_PEER_HANDLE_BYTES gathered from all ranks (how they travel is the caller's
 *                     business: torch.distributed.all_gather_object, MPI, a file) and / or local_ptrs[nranks] for same-process
 *                     peers (NULL entries fall back to the handle).  Sets the shard layout like srl_comm_init_rank: upload the
 *                     sweep afterwards (SHARD LAYOUT above).  nranks <= 8.  Mutually exclusive with srl_comm_init_rank / host callbacks.
 *   srl_peer_detach : back to an unsharded context (unmaps the peers' inboxes).
 * All ranks must call srl_build_residuals the same number of times with the same options (as with any collective).
 *
 * A late rank is not a failure.  The kernel that waits for the rows gives up after a bounded spin (0.3-1 s: it must not hold the GPU for
 * ever), but what follows is decided on the HOST: srl_build_residuals repeats the pass with the same exchange tags -- this rank's rows are
 * in every inbox already, the repeat only polls again; nobody can run ahead, the next exchange needs a row of this rank -- until the
 * missing row is there (every rank then returns SRL_OK, the late one included) or until the wall-clock deadline of
 *   srl_peer_set_deadline_ms (default 10 000 ms, measured from the start of the pass; 0 = give up at the first time-out)
 * has passed.  Then the SESSION is given up for every rank: this rank sets the poison word of every inbox and returns SRL_ERR_COMM; a rank
 * whose own pass times out looks at its word first and returns SRL_ERR_COMM at once instead of waiting for its own deadline (a rank that
 * had already completed the exchange -- the rows were there -- fails at its next one).  After that every srl_build_residuals on the session
 * returns SRL_ERR_COMM until srl_peer_detach + srl_peer_export + srl_peer_attach on every rank start a new one.
 *   srl_peer_stats : passes repeated because a row had not arrived within one kernel's spin (since the attach), whether the session failed. */
#define SRL_PEER_HANDLE_BYTES 64
int srl_peer_export(srl_ctx *ctx, void *ipc_handle, void **local_ptr);
int srl_peer_attach(srl_ctx *ctx, int nranks, int rank, const void *ipc_handles, void *const *local_ptrs);
int srl_peer_set_deadline_ms(srl_ctx *ctx, int deadline_ms);
int srl_peer_stats(srl_ctx *ctx, int64_t *passes_repeated, int *session_failed);
int srl_peer_detach(srl_ctx *ctx);

/* pure helpers of the sharded path (also used internally): the contiguous point range of a rank
 * (SURVEY.md 8(e)), and the residual budget a rank may still spend given the accepted counts of all
 * shards (reproduces the sequential early exit, optimize.cpp:107, across ordered shards).
 * mode: 0 = spend up to *budget, 1 = visit only the first keypoint, 2 = visit nothing. */
void srl_shard_range(int n, int nranks, int rank, int *begin, int *count);
void srl_shard_budget(int max_num_residuals, const int64_t *accepted_per_rank, int nranks, int rank,
                      int64_t *budget, int *mode);

/* ------------------------------------------------------------------ measurement
 * HIP-event timings (ms) of the last srl_build_residuals on the context's own stream. */
typedef struct srl_timing {
    float   assoc_ms;          /* last call: association + plane fit + residual kernel */
    float   reduce_ms;         /* last call: ordered cut-off + final reduction kernel(s) */
    float   total_ms;          /* last call: first launch -> results on host */
    int32_t calls;             /* srl_build_residuals calls since profiling was switched on */
    int64_t algorithmic_bytes; /* last call: sum_k (24 + 12*(2r+1)^3 + 12*P_k) for this rank's shard */
    double  sum_assoc_ms;      /* accumulated over `calls` */
    double  sum_reduce_ms;
    double  sum_total_ms;
    int64_t sum_algorithmic_bytes;
    int64_t sum_keypoints;
    double  sum_host_launch_us; /* host wall: call entry -> both kernels enqueued */
    double  sum_host_wait_us;   /* host wall: enqueue done -> results on the host (copy + stream sync [+ all-reduce]) */
    double  sum_host_total_us;  /* host wall: whole srl_build_residuals call */
    int64_t sum_passes;         /* buildPlaneResiduals passes the timed launches ran (1 per launch) */
} srl_timing;
int srl_get_timing(srl_ctx *ctx, srl_timing *t);
/* (debug / parity / tuning hooks -- srl_debug_* -- are declared in srlivo_hip_debug.h: no product code path calls them) */
int srl_set_profiling(srl_ctx *ctx, int mode);     /* 0 off (default); 1 full: four events + a sync per call (kernel, reduce,
                                                      * device total, host splits); 2 light: one event pair around the association
                                                      * kernel, read back lazily (calls / sum_assoc_ms / sum_algorithmic_bytes only);
                                                      * 3 host stamps only, no events: sum_host_launch_us = the launch call,
                                                      * sum_host_wait_us = enqueued -> result (incl. the overlap callback),
                                                      * sum_host_total_us = the whole call, sum_assoc_ms / sum_reduce_ms = argument
                                                      * preparation / launch returned -> everything enqueued (tools/host_hop_probe.py).
                                                      * Switching on resets the sums. */
/* Mode 2 looks at every association launch by default (one event record behind each: ~2.5 us of the loop per launch).  With a period
 * P > 1 only every P-th launch is timed (the launch before it leaves its end event as the start): 2 records per P launches.  calls,
 * sum_assoc_ms, sum_algorithmic_bytes, sum_passes then cover the timed launches and their passes only.  1 <= P <= 64; pick an odd P where
 * the launches of a solve alternate (first / second iteration), so that both kinds are sampled. */
int srl_set_profiling_period(srl_ctx *ctx, int period);
/* "The sums of srl_get_timing start HERE" (mode 2) without a read-back: no event is waited for, an armed launch stays armed.  Launches
 * enqueued before the mark -- the one armed behind the last pass included -- are left out of calls / sum_assoc_ms when their events are
 * read later, and their passes out of the byte sums.  With a period P > 1 the launches timed behind the mark are the 4th, the (4 + P)-th,
 * ... (the first step behind a barrier -- an un-armed launch into an idle GPU -- is no steady-state sample).  (srl_get_timing itself waits for every outstanding event and cancels an armed
 * launch: called between warm-up and a timed region it idles the GPU for a few hundred microseconds.) */
int srl_timing_mark(srl_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif

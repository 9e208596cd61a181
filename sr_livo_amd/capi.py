"""ctypes bindings of libsrlivo_hip.so (include/srlivo_hip.h + include/srlivo_host.h).

Mirrors the C declarations one to one; numpy arrays are passed as plain pointers.  Nothing here
computes: if the shared library is missing, or no HIP device exists, the calls raise SrlError.
"""
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRL_LIB_PATH") or os.path.join(_HERE, "libsrlivo_hip.so")   # env override: A/B builds only
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

SRL_OK = 0
SRL_ERR_NO_DEVICE = -1
SRL_ERR_BAD_ARG = -3
SRL_ERR_UNSUPPORTED = -4
SRL_ERR_NO_MAP = -5
SRL_ERR_NO_SWEEP = -6
SRL_ERR_COMM = -7
SRL_ERR_NAN_PLANARITY = -8
SRL_ERR_NOT_ENOUGH_RESIDUALS = -9
SRL_COMM_ID_BYTES = 128


SRL_PEER_HANDLE_BYTES = 64


class SrlError(RuntimeError):
    def __init__(self, status, what, detail=""):
        self.status = status
        super().__init__(f"{what}: status {status} {detail}".strip())


class IcpOpts(C.Structure):
    _fields_ = [
        ("threshold_voxel_occupancy", C.c_int32), ("init_num_frames", C.c_int32),
        ("size_voxel_map", C.c_double), ("num_iters_icp", C.c_int32),
        ("min_number_neighbors", C.c_int32), ("voxel_neighborhood", C.c_int32),
        ("power_planarity", C.c_double), ("max_number_neighbors", C.c_int32),
        ("max_dist_to_plane_icp", C.c_double), ("threshold_orientation_norm", C.c_double),
        ("threshold_translation_norm", C.c_double), ("max_num_residuals", C.c_int32),
        ("weight_alpha", C.c_double), ("weight_neighborhood", C.c_double),
    ]
    # test hook, NOT part of the struct (srl_icp_opts = the reference's icpOptions fields only): default_opts(select_mode=...) keeps the
    # wish as a Python attribute and the wrappers hand it to srl_debug_set_select_mode before the call
    select_mode = 0


class Frame(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("t_last", C.c_double * 3),
                ("R_il", C.c_double * 9), ("t_il", C.c_double * 3), ("frame_id", C.c_int32)]


class CloudPoint(C.Structure):
    """srl_cloud_point: one record of cloud_world (the payload of pcl::PointXYZI)"""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("intensity", C.c_float)]


CLOUD_POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])      # cloud.view(CLOUD_POINT_DTYPE)


class ColorOpts(C.Structure):
    """srl_color_opts: mapOptions (parameters.h:98-106)"""
    _fields_ = [("size_voxel_map", C.c_double), ("max_num_points_in_voxel", C.c_int32), ("min_distance_points", C.c_double),
                ("add_point_step", C.c_int32)]


class ColorTotals(C.Structure):
    """srl_color_totals: what one srl_color_map_insert did"""
    _fields_ = [("stored", C.c_int32), ("created", C.c_int32), ("registered", C.c_int32), ("visited", C.c_int32)]


class ColorCamera(C.Structure):
    """srl_color_camera: the pose and intrinsics project3dPointInThisImage reads from the frame's state (q as w, x, y, z)"""
    _fields_ = [("q_world_camera", C.c_double * 4), ("t_world_camera", C.c_double * 3), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("fov_margin", C.c_double)]


class ColorRenderTotals(C.Structure):
    """srl_color_render_totals: what one srl_color_map_render did, per occurrence of a voxel in the list"""
    _fields_ = [("listed", C.c_int64), ("behind", C.c_int64), ("outside", C.c_int64), ("gated", C.c_int64), ("first", C.c_int64),
                ("updated", C.c_int64), ("unknown", C.c_int64)]

    def as_tuple(self):
        return tuple(int(getattr(self, f)) for f, _ in self._fields_)


class ColorSelectOpts(C.Structure):
    """srl_color_select_opts: the arguments of selectPointsForProjection and the tracker's two depth limits"""
    _fields_ = [("minimum_dis", C.c_double), ("skip_step", C.c_int32), ("use_all_points", C.c_int32), ("minimum_depth", C.c_double),
                ("maximum_depth", C.c_double)]


class ColorSelectTotals(C.Structure):
    """srl_color_select_totals: what one srl_color_map_select did"""
    _fields_ = [("candidates", C.c_int64), ("visited", C.c_int64), ("far", C.c_int64), ("near", C.c_int64), ("behind", C.c_int64),
                ("outside", C.c_int64), ("selected", C.c_int64), ("unknown", C.c_int64)]

    def as_tuple(self):
        return tuple(int(getattr(self, f)) for f, _ in self._fields_)


# srl_color_selected: records.view(COLOR_SELECTED_DTYPE)
COLOR_SELECTED_DTYPE = np.dtype([("index", "<i4"), ("pool", "<i4"), ("point_index", "<i4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"),
                                 ("u", "<f4"), ("v", "<f4")])


class ColorTrackOpts(C.Structure):
    """srl_color_track_opts: updateAndAppendTrackPoints' mini_distance and the tracker's maximum_tracked_points"""
    _fields_ = [("mini_distance", C.c_double), ("maximum_tracked_points", C.c_int32), ("reserved", C.c_int32)]


class ColorTrackTotals(C.Structure):
    """srl_color_track_totals: what the two loops of one srl_color_map_track_update did"""
    _fields_ = [(f, C.c_int64) for f in ("tracked_in", "kept", "flagged", "dropped", "behind", "unknown", "duplicate", "candidates",
                                         "already_tracked", "cand_unknown", "refused", "occupied", "added", "cut")]

    def as_tuple(self):
        return tuple(int(getattr(self, f)) for f, _ in self._fields_)


SRL_COLOR_TRACK_MAX_POINTS, SRL_COLOR_TRACK_MAX_CANDIDATES = 65536, 1048576
# srl_color_track_point: records.view(COLOR_TRACK_POINT_DTYPE)
COLOR_TRACK_POINT_DTYPE = np.dtype([("pool", "<i4"), ("u", "<f4"), ("v", "<f4"), ("flagged", "<i4")])
# srl_color_track_outcome, srl_color_track_candidate_outcome
(SRL_TRACK_KEPT, SRL_TRACK_KEPT_FLAGGED, SRL_TRACK_DROPPED, SRL_TRACK_BEHIND, SRL_TRACK_UNKNOWN, SRL_TRACK_DUPLICATE) = range(6)
(SRL_TRACK_CAND_ADDED, SRL_TRACK_CAND_ALREADY_TRACKED, SRL_TRACK_CAND_UNKNOWN, SRL_TRACK_CAND_REFUSED, SRL_TRACK_CAND_OCCUPIED,
 SRL_TRACK_CAND_CUT, SRL_TRACK_CAND_NOT_REACHED) = range(7)


class ColorVioArgs(C.Structure):
    """srl_color_vio_args: the camera state one iteration of vioEsikf / vioPhotometric reads (R_imu_camera row-major)"""
    _fields_ = [("cam", ColorCamera), ("time_td", C.c_double), ("R_imu_camera", C.c_double * 9), ("mode", C.c_int32),
                ("estimate_extrinsic", C.c_int32), ("estimate_intrinsic", C.c_int32)]


class ColorVioSums(C.Structure):
    """srl_color_vio_sums: H^T H (11 x 11 row-major), H^T r, the acc_residual sum and the outcome counts of one srl_color_map_vio_rows"""
    _fields_ = [("HtH", C.c_double * 121), ("Htr", C.c_double * 11), ("acc_residual", C.c_double), ("used", C.c_int64),
                ("few_views", C.c_int64), ("behind", C.c_int64), ("outside", C.c_int64), ("unknown", C.c_int64)]

    def counts(self):
        return (int(self.used), int(self.few_views), int(self.behind), int(self.outside), int(self.unknown))

    def as_arrays(self):
        """(HtH (11, 11), Htr (11,), acc_residual)"""
        return np.array(self.HtH[:]).reshape(11, 11), np.array(self.Htr[:]), float(self.acc_residual)


SRL_VIO_REPROJECTION, SRL_VIO_PHOTOMETRIC = 0, 1
SRL_COLOR_VIO_MAX_POINTS = 65536
# srl_color_vio_point: list.view(COLOR_VIO_POINT_DTYPE)
COLOR_VIO_POINT_DTYPE = np.dtype([("pool", "<i4"), ("pad", "<i4"), ("match_u", "<f8"), ("match_v", "<f8"), ("vel_u", "<f8"), ("vel_v", "<f8")])


class FlowOpts(C.Structure):
    """srl_flow_opts: the tracker's options (opticalFlowTracker.cpp:5-8); they hold for its life"""
    _fields_ = [("win", C.c_int32), ("max_level", C.c_int32), ("max_count", C.c_int32), ("reserved", C.c_int32),
                ("epsilon", C.c_double), ("min_eig_threshold", C.c_double)]


SRL_FLOW_MAX_POINTS = 65536
SRL_FLOW_MAX_EXTENT = 16384
SRL_FLOW_PREV, SRL_FLOW_CUR = 0, 1
FLOW_BORDER = 21


class ImagePrepOpts(C.Structure):
    """srl_image_prep_opts: image size, intrinsics, distortion (k1 k2 p1 p2 k3), CLAHE clips, tiles per side (0 = the reference's rule)"""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("dist", C.c_double * 5), ("clip_gray", C.c_double), ("clip_color", C.c_double), ("tiles", C.c_int32), ("reserved", C.c_int32)]


class ImagePrepInfo(C.Structure):
    """srl_image_prep_info: the tiling of the preparer and whether the last image became the colour map's"""
    _fields_ = [("tiles", C.c_int32), ("tile_w", C.c_int32), ("tile_h", C.c_int32), ("ext_rows", C.c_int32), ("ext_cols", C.c_int32),
                ("limit_gray", C.c_int32), ("limit_color", C.c_int32), ("installed_color", C.c_int32)]

    def as_tuple(self):
        return tuple(getattr(self, f) for f, _ in self._fields_)


class JpegInfo(C.Structure):
    """srl_jpeg_info: what srl_jpeg_parse reads from a baseline JPEG stream's header"""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("components", C.c_int32), ("h", C.c_int32 * 3), ("v", C.c_int32 * 3),
                ("mcus_per_row", C.c_int32), ("mcus_per_col", C.c_int32), ("restart_interval", C.c_int32), ("reserved", C.c_int32 * 2),
                ("blocks", C.c_int64 * 3), ("total_blocks", C.c_int64), ("scan_offset", C.c_int64)]


SRL_PREP_GRAY_EQ, SRL_PREP_BGR_EQ = 0, 1
SRL_PREP_STAGE_UNDIST, SRL_PREP_STAGE_GRAY, SRL_PREP_STAGE_YCRCB, SRL_PREP_STAGE_LUT_GRAY, SRL_PREP_STAGE_LUT_Y = 0, 1, 2, 3, 4


class ConsensusOpts(C.Structure):
    """srl_consensus_opts: inlier threshold (pixels), confidence, the fixed number of hypotheses, the generator's seed"""
    _fields_ = [("threshold", C.c_double), ("confidence", C.c_double), ("hypotheses", C.c_int32), ("seed", C.c_uint32)]


class ConsensusResult(C.Structure):
    """srl_consensus_result: the winning model (F row-major in [0, 9), or R row-major then t), its sample, where it came from, its count"""
    _fields_ = [("model", C.c_double * 12), ("sample", C.c_int32 * 8), ("hypothesis", C.c_int32), ("slot", C.c_int32), ("inliers", C.c_int32),
                ("models_valid", C.c_int32), ("confidence_reached", C.c_int32), ("reserved", C.c_int32)]

    def model_array(self):
        return np.array(self.model[:], dtype=np.float64)

    def sample_array(self):
        return np.array(self.sample[:], dtype=np.int32)


class DebugConsensusInfo(C.Structure):
    """srl_debug_consensus_info (include/srlivo_hip_debug.h): the shape of the last consensus call and its normalisation"""
    _fields_ = [("model", C.c_int32), ("hypotheses", C.c_int32), ("n", C.c_int32), ("slots", C.c_int32), ("usable", C.c_int32),
                ("reserved", C.c_int32), ("norm", C.c_double * 6)]


SRL_CONSENSUS_FUNDAMENTAL, SRL_CONSENSUS_PNP = 0, 1
SRL_CONSENSUS_MAX_POINTS = 4096
SRL_CONSENSUS_MAX_HYPOTHESES = 4096


class ColorCloudOpts(C.Structure):
    """srl_color_cloud_opts: pub_point_minimum_views, the direction of the walk and the optional observation-time cut"""
    _fields_ = [("minimum_views", C.c_int32), ("reverse", C.c_int32), ("since", C.c_double)]


class ColorCloudTotals(C.Structure):
    """srl_color_cloud_totals: what one srl_color_map_export_cloud did (scanned = published + below_views + stale)"""
    _fields_ = [("scanned", C.c_int64), ("published", C.c_int64), ("below_views", C.c_int64), ("stale", C.c_int64)]

    def as_tuple(self):
        return tuple(int(getattr(self, f)) for f, _ in self._fields_)


# srl_color_cloud_point: records.view(COLOR_CLOUD_DTYPE) -- x y z and the rgb word (b, g, r, a from the low byte)
COLOR_CLOUD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1")])

# srl_color_stored: records.view(COLOR_STORED_DTYPE)
COLOR_STORED_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("kx", "<i2"), ("ky", "<i2"), ("kz", "<i2"), ("slot", "<u2"),
                               ("batch_index", "<i4"), ("point_index", "<i4")])


class NormalEq(C.Structure):
    _fields_ = [("HtH", C.c_double * 36), ("Hth", C.c_double * 6), ("loss_sum", C.c_double),
                ("num_residuals", C.c_int32), ("success", C.c_int32), ("sum_candidates", C.c_int64),
                ("last_visited", C.c_int64), ("nan_error", C.c_int32), ("num_fallback", C.c_int32)]



class Timing(C.Structure):
    _fields_ = [("assoc_ms", C.c_float), ("reduce_ms", C.c_float), ("total_ms", C.c_float), ("calls", C.c_int32),
                ("algorithmic_bytes", C.c_int64), ("sum_assoc_ms", C.c_double), ("sum_reduce_ms", C.c_double),
                ("sum_total_ms", C.c_double), ("sum_algorithmic_bytes", C.c_int64), ("sum_keypoints", C.c_int64),
                ("sum_host_launch_us", C.c_double), ("sum_host_wait_us", C.c_double), ("sum_host_total_us", C.c_double),
                ("sum_passes", C.c_int64)]


class ImuState(C.Structure):
    _fields_ = [("timestamp", C.c_double), ("un_acc", C.c_double * 3), ("un_gyr", C.c_double * 3), ("trans", C.c_double * 3),
                ("quat", C.c_double * 4), ("vel", C.c_double * 3)]


class OdometryOpts(C.Structure):
    _fields_ = [("init_voxel_size", C.c_double), ("init_sample_voxel_size", C.c_double), ("init_num_frames", C.c_int),
                ("num_for_initialization", C.c_int), ("voxel_size", C.c_double), ("sample_voxel_size", C.c_double),
                ("max_num_points_in_voxel", C.c_int), ("min_distance_points", C.c_double), ("motion_compensation", C.c_int),
                ("initialization", C.c_int), ("point_time_enable", C.c_int), ("acc_cov", C.c_double), ("gyr_cov", C.c_double),
                ("b_acc_cov", C.c_double), ("b_gyr_cov", C.c_double), ("icp", IcpOpts)]


class ReplayResult(C.Structure):
    _fields_ = [("processed", C.c_int), ("initialized", C.c_int), ("index_frame", C.c_int), ("success", C.c_int),
                ("num_residuals_used", C.c_int), ("iterations", C.c_int), ("frame_points", C.c_int), ("keypoints", C.c_int),
                ("points_added", C.c_int), ("state", C.c_double * 16)]


MC_IMU, MC_CONSTANT_VELOCITY, MC_NONE = 0, 1, 2


class LivoxOpts(C.Structure):
    """srl_livox_opts: cloudProcessing's N_SCANS, time_unit_scale, blind, point_filter_num"""
    _fields_ = [("n_scans", C.c_int32), ("reserved0", C.c_int32), ("time_unit_scale", C.c_double), ("blind", C.c_double),
                ("point_filter_num", C.c_int32), ("reserved1", C.c_int32)]


class LivoxReport(C.Structure):
    _fields_ = [("valid", C.c_int32), ("picked", C.c_int32), ("appended", C.c_int32), ("reserved", C.c_int32), ("last_end_time", C.c_double),
                ("first_timestamp", C.c_double), ("last_timestamp", C.c_double)]


class PointsCutReport(C.Structure):
    _fields_ = [("count", C.c_int32), ("reserved", C.c_int32), ("front_timestamp", C.c_double)]


class Pc2Layout(C.Structure):
    """srl_pc2_layout: what pcl::fromROSMsg reads of a sensor_msgs::PointCloud2"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("point_step", C.c_uint32), ("row_step", C.c_uint32), ("off_x", C.c_int32),
                ("off_y", C.c_int32), ("off_z", C.c_int32), ("off_time", C.c_int32), ("off_ring", C.c_int32), ("is_bigendian", C.c_int32)]


class Pc2Opts(C.Structure):
    """srl_pc2_opts: cloudProcessing's lidar_type, N_SCANS, SCAN_RATE, point_filter_num, time_unit_scale, blind"""
    _fields_ = [("lidar_type", C.c_int32), ("n_scans", C.c_int32), ("scan_rate", C.c_int32), ("point_filter_num", C.c_int32),
                ("time_unit_scale", C.c_double), ("blind", C.c_double)]


class Pc2Report(C.Structure):
    _fields_ = [("points", C.c_int32), ("given_offset_time", C.c_int32), ("picked", C.c_int32), ("appended", C.c_int32),
                ("last_end_time", C.c_double), ("first_timestamp", C.c_double), ("last_timestamp", C.c_double)]


# cloudProcessing.h:25, and the fields srl_pc2_decode reads per type (the reference's registered point structs, :50-114)
LIDAR_LIVOX, LIDAR_VELO, LIDAR_OUST, LIDAR_ROBO = 1, 2, 3, 4
PC2_POINT_DTYPES = {
    LIDAR_VELO: np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("time", "<f4"), ("ring", "<u2")]),
    LIDAR_OUST: np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("time", "<u4"), ("ring", "u1")]),
    LIDAR_ROBO: np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("time", "<f8"), ("ring", "<u2")]),
}
# where the drivers put them: velodyne_pointcloud's PointXYZIRT (22 B, time unaligned), ouster_ros (48 B), rslidar_sdk's XYZIRT (26 B, the
# double at 18)
PC2_DRIVER_LAYOUTS = {
    LIDAR_VELO: (22, dict(x=0, y=4, z=8, ring=16, time=18)),
    LIDAR_OUST: (48, dict(x=0, y=4, z=8, time=20, ring=26)),
    LIDAR_ROBO: (26, dict(x=0, y=4, z=8, ring=16, time=18)),
}

# srl_livox_point = livox_ros_driver::CustomPoint in memory (20 B)
LIVOX_POINT_DTYPE = np.dtype([("offset_time", "<u4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("reflectivity", "u1"), ("tag", "u1"),
                              ("line", "u1"), ("pad", "u1")])
TIME_UNIT_SEC, TIME_UNIT_MS, TIME_UNIT_US, TIME_UNIT_NS = 0, 1, 2, 3

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_int, C.c_void_p)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p)
PROVIDER_FN = C.CFUNCTYPE(C.c_int, C.POINTER(Frame), C.POINTER(IcpOpts), C.POINTER(NormalEq), C.c_void_p)

# srl_oft_*_provider (srlivo_host.h)
OFT_FLOW_PROVIDER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
OFT_FUNDAMENTAL_PROVIDER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)
OFT_PNP_PROVIDER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p)
OFT_UPDATE_PROVIDER_FN = C.CFUNCTYPE(C.c_int, C.POINTER(ColorCamera), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(ColorTrackOpts),
                                     C.c_void_p, C.c_int64, C.POINTER(ColorTrackTotals), C.c_void_p)
VIO_ROWS_PROVIDER_FN = C.CFUNCTYPE(C.c_int, C.POINTER(ColorVioArgs), C.c_void_p, C.c_int, C.POINTER(ColorVioSums), C.c_void_p)


class ImageProcessOpts(C.Structure):
    """srl_image_process_opts: what imageProcessing::process reads beside the options of srl_lio_vio_set_options"""
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("image_resize_ratio", C.c_double), ("dist", C.c_double * 5),
                ("track_windows_size", C.c_double), ("maximum_tracked_points", C.c_int32), ("reserved", C.c_int32),
                ("tracker_minimum_depth", C.c_double), ("tracker_maximum_depth", C.c_double)]


class ImageProcessResult(C.Structure):
    """srl_image_process_result: what one srl_lio_image_process did"""
    _fields_ = [(f, C.c_int32) for f in ("first_data", "prepared_rows", "prepared_cols", "tracked_after_flow", "tracked_after_pnp", "pnp_accepted",
                                         "esikf_accepted", "esikf_iterations", "esikf_used", "photometric_accepted", "photometric_iterations",
                                         "photometric_used", "refreshed_candidates", "reserved")] + \
               [("image_scale_factor", C.c_double), ("render", ColorRenderTotals), ("track", ColorTrackTotals)]


IMAGE_PREP_CREATE_STEP_FN = C.CFUNCTYPE(C.c_int, C.POINTER(ImagePrepOpts), C.c_void_p)
IMAGE_PREPARE_STEP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p)
IMAGE_CONSENSUS_SETUP_STEP_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_void_p)
IMAGE_SELECT_STEP_FN = C.CFUNCTYPE(C.c_int, C.POINTER(ColorCamera), C.c_int, C.c_int, C.POINTER(ColorSelectOpts), C.c_int, C.c_void_p, C.c_int,
                                   C.POINTER(C.c_int), C.c_void_p)
IMAGE_RENDER_STEP_FN = C.CFUNCTYPE(C.c_int, C.POINTER(ColorCamera), C.c_double, C.POINTER(ColorRenderTotals), C.c_void_p)
IMAGE_JPEG_STEP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p)      # srl_image_jpeg_step: bytes, n, user


class ImageProcessSteps(C.Structure):
    """srl_image_process_steps: the steps of imageProcessing::process that leave the mirror; a NULL member keeps the device call"""
    _fields_ = [("user", C.c_void_p), ("prep_create", IMAGE_PREP_CREATE_STEP_FN), ("prepare", IMAGE_PREPARE_STEP_FN),
                ("consensus_setup", IMAGE_CONSENSUS_SETUP_STEP_FN), ("select", IMAGE_SELECT_STEP_FN), ("flow", OFT_FLOW_PROVIDER_FN),
                ("fundamental", OFT_FUNDAMENTAL_PROVIDER_FN), ("pnp", OFT_PNP_PROVIDER_FN), ("rows", VIO_ROWS_PROVIDER_FN),
                ("render", IMAGE_RENDER_STEP_FN), ("track_update", OFT_UPDATE_PROVIDER_FN)]
CAMERA_STATE_DOUBLES = 31      # time_td, R_imu_camera (9), t_imu_camera (3), fx fy cx cy, q_world_camera (4), t_world_camera (3), rotation (4), translation (3)

_lib = None


def load_library():
    """Load libsrlivo_hip.so; raises SrlError (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SrlError(-1, "libsrlivo_hip.so not built",
                       f"(expected {LIB_PATH}; run `python -c 'import __graft_entry__ as g; g.build()'`)")
    lib = C.CDLL(LIB_PATH)
    p = C.c_void_p
    dp = C.POINTER(C.c_double)
    sig = {
        "srl_device_count": ([C.POINTER(C.c_int)], C.c_int),
        "srl_ctx_create": ([C.c_int, C.POINTER(p)], C.c_int),
        "srl_ctx_destroy": ([p], C.c_int),
        "srl_last_error": ([p], C.c_char_p),
        "srl_status_str": ([C.c_int], C.c_char_p),
        "srl_icp_opts_default": ([C.POINTER(IcpOpts)], None),
        "srl_map_upload": ([p, p, p, p, C.c_int, C.c_int], C.c_int),
        "srl_map_insert": ([p, p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_map_insert_report": ([p, p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_double, p, p, C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)], C.c_int),
        "srl_map_size": ([p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)], C.c_int),
        "srl_map_download": ([p, p, p, p, C.c_int], C.c_int),
        "srl_map_remove_far": ([p, dp, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int64)], C.c_int),
        "srl_map_probe_checksum": ([p, p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_uint64)], C.c_int),
        "srl_color_opts_default": ([C.POINTER(ColorOpts)], None),
        "srl_color_map_create": ([p, C.POINTER(ColorOpts)], C.c_int),
        "srl_color_map_destroy": ([p], C.c_int),
        "srl_color_map_insert": ([p, p, C.c_int, C.c_double, C.c_double, p, p, C.c_int, p, C.c_int, C.POINTER(ColorTotals)], C.c_int),
        "srl_color_map_size": ([p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)], C.c_int),
        "srl_color_map_download": ([p, p, p, p, C.c_int, p, p, C.c_int64], C.c_int),
        "srl_color_registered_download": ([p, C.c_int64, C.c_int, p], C.c_int),
        "srl_debug_color_map_rebuilds": ([p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)], C.c_int),
        "srl_debug_color_epochs": ([p, C.POINTER(C.c_uint32)], C.c_int),
        "srl_debug_set_color_epochs": ([p, C.c_int, C.c_int], C.c_int),
        "srl_color_image_upload": ([p, p, C.c_int, C.c_int, C.c_int64], C.c_int),
        "srl_color_select_opts_default": ([C.POINTER(ColorSelectOpts)], None),
        "srl_color_map_select": ([p, C.POINTER(ColorCamera), C.c_int, C.c_int, p, C.c_int, C.POINTER(ColorSelectOpts), p, C.c_int64,
                                  C.POINTER(ColorSelectTotals)], C.c_int),
        "srl_color_map_render": ([p, C.POINTER(ColorCamera), p, C.c_int, C.c_double, C.POINTER(ColorRenderTotals)], C.c_int),
        "srl_color_track_opts_default": ([C.POINTER(ColorTrackOpts)], None),
        "srl_color_map_track_update": ([p, C.POINTER(ColorCamera), C.c_int, C.c_int, p, C.c_int, p, C.c_int, C.POINTER(ColorTrackOpts), p, C.c_int64,
                                        p, p, C.POINTER(ColorTrackTotals)], C.c_int),
        "srl_color_map_vio_rows": ([p, C.POINTER(ColorVioArgs), p, C.c_int, C.POINTER(ColorVioSums), p, p], C.c_int),
        "srl_flow_opts_default": ([C.POINTER(FlowOpts)], None),
        "srl_flow_create": ([p, C.POINTER(FlowOpts)], C.c_int),
        "srl_flow_destroy": ([p], C.c_int),
        "srl_flow_track_image": ([p, p, C.c_int, C.c_int, C.c_int64, p, C.c_int, p, p, C.POINTER(C.c_int)], C.c_int),
        "srl_flow_levels": ([p, C.POINTER(C.c_int)], C.c_int),
        "srl_flow_download_level": ([p, C.c_int, C.c_int, p, p, C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
        "srl_image_prep_opts_default": ([C.POINTER(ImagePrepOpts)], None),
        "srl_image_prep_build_map": ([C.POINTER(ImagePrepOpts), p, p], C.c_int),
        "srl_image_prep_create": ([p, C.POINTER(ImagePrepOpts)], C.c_int),
        "srl_image_prep_destroy": ([p], C.c_int),
        "srl_image_prepare": ([p, p, C.c_int, C.c_int, C.c_int64, C.POINTER(ImagePrepInfo)], C.c_int),
        "srl_image_resize_build_tables": ([C.c_int, C.c_int, p, p], C.c_int),
        "srl_image_prepare_resized": ([p, p, C.c_int, C.c_int, C.c_int64, C.POINTER(ImagePrepInfo)], C.c_int),
        "srl_image_prep_download_resized": ([p, p, C.c_int64], C.c_int),
        "srl_image_prep_download": ([p, C.c_int, p, C.c_int64], C.c_int),
        "srl_image_prep_download_stage": ([p, C.c_int, p, C.c_int64], C.c_int),
        "srl_jpeg_parse": ([p, C.c_int64, C.POINTER(JpegInfo)], C.c_int),
        "srl_jpeg_entropy_decode": ([p, C.c_int64, C.POINTER(JpegInfo), p, C.c_int64, p], C.c_int),
        "srl_jpeg_decode": ([p, p, C.c_int64, C.POINTER(JpegInfo)], C.c_int),
        "srl_jpeg_download": ([p, p, C.c_int64], C.c_int),
        "srl_image_prepare_jpeg": ([p, p, C.c_int64, C.POINTER(ImagePrepInfo)], C.c_int),
        "srl_jpeg_idct_blocks": ([p, p, C.c_int64, p, p], C.c_int),
        "srl_flow_track_prepared": ([p, p, C.c_int, p, p, C.POINTER(C.c_int)], C.c_int),
        "srl_oft_use_prepared_image": ([p, C.c_int], C.c_int),
        "srl_consensus_opts_default": ([C.POINTER(ConsensusOpts), C.c_int], None),
        "srl_consensus_fundamental": ([p, p, p, C.c_int, C.POINTER(ConsensusOpts), p, C.POINTER(ConsensusResult)], C.c_int),
        "srl_consensus_pnp": ([p, p, p, C.c_int, dp, C.POINTER(ConsensusOpts), p, C.POINTER(C.c_int), C.POINTER(ConsensusResult)], C.c_int),
        "srl_oft_use_device_consensus": ([p, dp, C.POINTER(ConsensusOpts), C.POINTER(ConsensusOpts)], C.c_int),
        "srl_oft_last_consensus": ([p, C.c_int, C.POINTER(ConsensusResult)], C.c_int),
        "srl_debug_consensus_download": ([p, C.POINTER(DebugConsensusInfo), p, C.c_int64, p, p, p, C.c_int64], C.c_int),
        "srl_oft_create": ([p, C.POINTER(p)], C.c_int),
        "srl_oft_destroy": ([p], C.c_int),
        "srl_oft_set_maximum_tracked_points": ([p, C.c_int], C.c_int),
        "srl_oft_set_flow_provider": ([p, OFT_FLOW_PROVIDER_FN, p], C.c_int),
        "srl_oft_set_fundamental_provider": ([p, OFT_FUNDAMENTAL_PROVIDER_FN, p], C.c_int),
        "srl_oft_set_pnp_provider": ([p, OFT_PNP_PROVIDER_FN, p], C.c_int),
        "srl_oft_set_update_provider": ([p, OFT_UPDATE_PROVIDER_FN, p], C.c_int),
        "srl_oft_set_track_points": ([p, p, C.c_int], C.c_int),
        "srl_oft_init": ([p, p, C.c_int, p, C.c_int, C.c_int, C.c_int64, C.c_double], C.c_int),
        "srl_oft_track_image": ([p, p, C.c_int, C.c_int, C.c_int64, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_oft_remove_outlier_using_ransac_pnp": ([p, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_oft_update_and_append_track_points": ([p, C.POINTER(ColorCamera), C.c_int, C.c_int, p, C.c_int, C.c_double, C.POINTER(ColorTrackTotals)], C.c_int),
        "srl_oft_sizes": ([p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
        "srl_oft_times": ([p, C.POINTER(C.c_double), C.POINTER(C.c_double)], C.c_int),
        "srl_oft_pose_map": ([p, C.c_int, p, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_oft_tracked_for_vio": ([p, p, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_lk_create": ([p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, C.POINTER(p)], C.c_int),
        "srl_lk_destroy": ([p], C.c_int),
        "srl_lk_get": ([p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)], C.c_int),
        "srl_lk_track_image": ([p, p, C.c_int, C.c_int, C.c_int64, p, C.c_int, p, p, C.POINTER(C.c_int)], C.c_int),
        "srl_color_cloud_opts_default": ([C.POINTER(ColorCloudOpts)], None),
        "srl_color_map_export_cloud": ([p, C.c_int64, C.c_int64, C.POINTER(ColorCloudOpts), p, p, C.c_int64, C.POINTER(ColorCloudTotals)], C.c_int),
        "srl_color_map_download_rgb": ([p, p, p, p, p, p, C.c_int64], C.c_int),
        "srl_color_registered_rgb": ([p, C.c_int64, C.c_int, p, p, p, p, p], C.c_int),
        "srl_sweep_upload": ([p, p, C.c_int], C.c_int),
        "srl_sweep_shard": ([p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
        "srl_sweep_prefetch": ([p, p, C.c_int], C.c_int),
        "srl_sweep_swap": ([p], C.c_int),
        "srl_sweep_wait": ([p], C.c_int),
        "srl_thread_pin_to_gpu_numa": ([p, C.POINTER(C.c_int)], C.c_int),
        "srl_pinned_alloc": ([C.c_size_t, C.POINTER(p)], C.c_int),
        "srl_pinned_free": ([p], C.c_int),
        "srl_host_register": ([p, C.c_size_t], C.c_int),
        "srl_host_unregister": ([p], C.c_int),
        "srl_comm_backend_info": ([C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
        "srl_build_residuals": ([p, C.POINTER(Frame), C.POINTER(IcpOpts), C.POINTER(NormalEq)], C.c_int),
        "srl_build_residuals_overlap": ([p, C.POINTER(Frame), C.POINTER(IcpOpts), C.POINTER(NormalEq), p, p], C.c_int),
        "srl_set_taps": ([p, C.c_int], C.c_int),
        "srl_fetch_neighbors": ([p, p, p, p], C.c_int),
        "srl_fetch_residuals": ([p, p, p, p, p, p, p], C.c_int),
        "srl_search_neighbors": ([p, p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, p, p, p], C.c_int),
        "srl_transform_points": ([p, p, C.c_int, dp, dp, dp, dp, p], C.c_int),
        "srl_frame_upload": ([p, p, C.c_int], C.c_int),
        "srl_frame_undistort": ([p, p, p, p, C.c_int, p, C.c_int, C.c_double, C.c_int, dp, dp, p, p], C.c_int),
        "srl_frame_take": ([p, p, C.c_int], C.c_int),
        "srl_frame_subsample": ([p, p, C.c_int, C.c_double, C.POINTER(C.c_int)], C.c_int),
        "srl_frame_take_subsampled": ([p, p, C.c_int, p, p, p], C.c_int),
        "srl_frame_size": ([p, C.POINTER(C.c_int)], C.c_int),
        "srl_frame_select_keypoints": ([p, dp, dp, dp, dp, C.c_double, p, C.POINTER(C.c_int)], C.c_int),
        "srl_frame_commit_report": ([p, dp, dp, dp, dp, C.c_double, C.c_int, C.c_double, C.c_int, p, p, p, C.POINTER(C.c_int),
                                     C.POINTER(C.c_int)], C.c_int),
        "srl_frame_commit": ([p, dp, dp, dp, dp, C.c_double, C.c_int, C.c_double, C.c_int, p, C.POINTER(C.c_int)], C.c_int),
        "srl_comm_unique_id": ([p], C.c_int),
        "srl_comm_init_rank": ([p, C.c_int, C.c_int, p], C.c_int),
        "srl_comm_destroy": ([p], C.c_int),
        "srl_comm_set_library": ([C.c_char_p], C.c_int),
        "srl_comm_suspend": ([p, C.c_int], C.c_int),
        "srl_comm_info": ([p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64)], C.c_int),
        "srl_comm_set_host_callbacks": ([p, C.c_int, C.c_int, ALLREDUCE_FN, ALLGATHER_FN, p], C.c_int),
        "srl_debug_set_gather_counts": ([p, C.c_int, C.c_int, C.POINTER(C.c_int64)], C.c_int),
        "srl_peer_export": ([p, p, C.POINTER(p)], C.c_int),
        "srl_peer_attach": ([p, C.c_int, C.c_int, p, C.POINTER(p)], C.c_int),
        "srl_peer_set_deadline_ms": ([p, C.c_int], C.c_int),
        "srl_peer_stats": ([p, C.POINTER(C.c_int64), C.POINTER(C.c_int)], C.c_int),
        "srl_peer_detach": ([p], C.c_int),
        "srl_shard_range": ([C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)], None),
        "srl_shard_budget": ([C.c_int, C.POINTER(C.c_int64), C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)], None),
        "srl_get_timing": ([p, C.POINTER(Timing)], C.c_int),
        "srl_debug_block_times": ([p, p, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_debug_set_ablate": ([p, C.c_int], C.c_int),
        "srl_debug_set_fused_reduce": ([p, C.c_int], C.c_int),
        "srl_debug_set_bound_culling": ([p, C.c_int], C.c_int),
        "srl_debug_set_neighbour_records": ([p, C.c_int], C.c_int),
        "srl_debug_neighbour_records_download": ([p, p, C.c_int], C.c_int),
        "srl_debug_bounds_download": ([p, p, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_debug_set_pose_box": ([p, C.c_int], C.c_int),
        "srl_debug_set_arm_linger": ([p, C.c_double, C.c_double], C.c_int),
        "srl_debug_pass_stamps": ([p, C.c_int, p, p], C.c_int),
        "srl_debug_frame_timing": ([p, C.c_int, p], C.c_int),
        "srl_debug_set_frame_epoch": ([p, C.c_int], C.c_int),
        "srl_debug_set_frame_counters": ([p, C.c_int], C.c_int),
        "srl_debug_frame_counters": ([p, C.POINTER(C.c_uint32)], C.c_int),
        "srl_set_armed_launch": ([p, C.c_int], C.c_int),
        "srl_disarm": ([p], C.c_int),
        "srl_solve_end": ([p], C.c_int),
        "srl_get_arm_stats": ([p, C.POINTER(C.c_uint64)], C.c_int),
        "srl_debug_set_launch_shape": ([p, C.c_int, C.c_int], C.c_int),
        "srl_debug_set_search_select_mode": ([p, C.c_int], C.c_int),
        "srl_debug_set_select_mode": ([p, C.c_int], C.c_int),
        "srl_debug_set_frame_order_mode": ([p, C.c_int], C.c_int),
        "srl_debug_radix_sort_pairs": ([p, p, C.c_int, C.c_int, p, p], C.c_int),
        "srl_debug_frame_order_used": ([p, C.POINTER(C.c_int)], C.c_int),
        "srl_debug_heap_topk": ([p, C.c_int, C.c_int, p], C.c_int),
        "srl_debug_device_sqrt": ([p, p, C.c_int, p], C.c_int),
        "srl_set_profiling": ([p, C.c_int], C.c_int),
        "srl_set_profiling_period": ([p, C.c_int], C.c_int),
        "srl_timing_mark": ([p], C.c_int),
        # host mirror handles
        "srl_lio_create": ([C.c_int, C.POINTER(p)], C.c_int),
        "srl_lio_destroy": ([p], C.c_int),
        "srl_lio_ctx": ([p], p),
        "srl_lio_last_error": ([p], C.c_char_p),
        "srl_lio_set_extrinsics": ([p, dp, dp], C.c_int),
        "srl_lio_set_laser_point_cov": ([p, C.c_double], C.c_int),
        "srl_lio_last_solve_launches": ([p, C.POINTER(C.c_int)], C.c_int),
        "srl_lio_eskf_get_state": ([p, dp], C.c_int),
        "srl_lio_eskf_set_state": ([p, dp], C.c_int),
        "srl_lio_eskf_get_cov": ([p, dp], C.c_int),
        "srl_lio_eskf_set_cov": ([p, dp], C.c_int),
        "srl_lio_eskf_set_noise": ([p, C.c_double, C.c_double, C.c_double, C.c_double], C.c_int),
        "srl_lio_eskf_init_imu": ([p, dp, dp], C.c_int),
        "srl_lio_eskf_scale_init_cov": ([p], C.c_int),
        "srl_lio_eskf_predict": ([p, C.c_double, dp, dp], C.c_int),
        "srl_lio_eskf_observe": ([p, dp], C.c_int),
        "srl_lio_add_points_to_map": ([p, p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int], C.c_int),
        "srl_lio_map_size": ([p, C.POINTER(C.c_int64)], C.c_int),
        "srl_lio_remove_points_far_from_location": ([p, dp, C.c_double], C.c_int),
        "srl_lio_set_collect_points_world": ([p, C.c_int], C.c_int),
        "srl_lio_points_world": ([p, p, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_lio_set_device_subsample": ([p, C.c_int], C.c_int),
        "srl_lio_set_color_map_options": ([p, C.POINTER(ColorOpts)], C.c_int),
        "srl_lio_set_color_times": ([p, C.c_double, C.c_double, C.c_int], C.c_int),
        "srl_lio_add_points_to_map_at": ([p, p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int], C.c_int),
        "srl_lio_color_cloud": ([p, C.c_int, C.c_int, p, p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(ColorCloudTotals)], C.c_int),
        "srl_lio_color_cloud_view": ([p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                      C.POINTER(ColorCloudTotals)], C.c_int),
        "srl_lio_color_topic_sizes": ([p, C.c_int64, p, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_lio_color_topic_state": ([p, C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
        "srl_lio_select_points_for_projection": ([p, C.POINTER(ColorCamera), C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, p, C.c_int,
                                                  C.POINTER(C.c_int), C.POINTER(ColorSelectTotals)], C.c_int),
        "srl_lio_color_visited": ([p, C.c_int, p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
        "srl_lio_color_stored": ([p, p, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_lio_render_points_in_recent_voxel": ([p, C.POINTER(ColorCamera), C.c_double, C.POINTER(ColorRenderTotals)], C.c_int),
        "srl_lio_probe_checksum_of_committed_frame": ([p, C.c_int, C.c_double, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)], C.c_int),
        "srl_lio_resident_sweep": ([p, p, C.c_int], C.c_int),
        "srl_lio_prefetch_sweep": ([p, p, C.c_int], C.c_int),
        "srl_lio_swap_sweep": ([p], C.c_int),
        "srl_lio_prefetch_sweep_during_solve": ([p, p, C.c_int], C.c_int),
        "srl_lio_update_iekf": ([p, C.POINTER(IcpOpts), p, C.c_int, dp, dp, C.c_int, p, C.c_int,
                                 C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
        "srl_lio_stream_step": ([p, C.POINTER(IcpOpts), dp, dp, C.c_int, dp, dp, C.c_int, p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
        "srl_lio_update_iekf_provided": ([p, C.POINTER(IcpOpts), PROVIDER_FN, p, C.c_int, dp, dp, C.c_int, p, C.c_int,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
        "srl_lio_optimize": ([p, C.POINTER(IcpOpts), C.c_double, p, p, C.c_int, dp, dp, C.c_int, p,
                              C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
        "srl_lio_eskf_try_init": ([p, dp, dp, dp, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_lio_eskf_get_init_stats": ([p, dp], C.c_int),
        "srl_lio_set_initial_flag": ([p, C.c_int], C.c_int),
        "srl_lio_state_initialization": ([p, C.c_int, C.c_int, dp, dp, dp], C.c_int),
        "srl_lio_set_odometry_options": ([p, C.POINTER(OdometryOpts)], C.c_int),
        "srl_lio_run_measurement": ([p, C.c_double, p, p, p, C.c_int, p, p, C.c_int, C.c_double, C.c_double,
                                     C.POINTER(ReplayResult)], C.c_int),
        "srl_lio_run_measurement_image": ([p, C.c_double, p, p, p, C.c_int, p, p, C.c_int, C.c_double, C.c_double, p, C.c_int, C.c_int, C.c_int64,
                                           C.POINTER(ReplayResult), C.POINTER(ImageProcessResult)], C.c_int),
        "srl_lio_set_g_norm": ([p, C.c_double], C.c_int),
        "srl_lio_last_frame": ([p, C.c_int, p, p, p, C.POINTER(C.c_int)], C.c_int),
        "srl_lio_optimize_resident": ([p, C.POINTER(IcpOpts), C.c_double, p, C.c_int, dp, dp, C.c_int, p,
                                       C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
        "srl_lio_commit_frame": ([p, dp, C.c_double, C.c_int, C.c_double, C.c_int, p, C.POINTER(C.c_int)], C.c_int),
        "srl_lio_search_neighbors": ([p, dp, C.c_int, C.c_double, C.c_int, C.c_int, p, p, C.POINTER(C.c_int)], C.c_int),
        "srl_lio_neighborhood": ([p, p, C.c_int, dp, dp, dp, dp], C.c_int),
        "srl_lio_build_plane_residuals": ([p, C.POINTER(IcpOpts), p, C.c_int, dp, dp, C.c_int, p, C.c_int,
                                           C.POINTER(C.c_int), dp, C.POINTER(C.c_int), p], C.c_int),
        "srl_lio_vio_set_options": ([p, C.c_int, C.c_int, C.c_int, p, p, p], C.c_int),
        "srl_lio_vio_set_camera_state": ([p, p], C.c_int),
        "srl_lio_vio_get_camera_state": ([p, p], C.c_int),
        "srl_lio_vio_set_initial_cov": ([p], C.c_int),
        "srl_lio_vio_set_cov": ([p, p], C.c_int),
        "srl_lio_vio_get_cov": ([p, p], C.c_int),
        "srl_lio_vio_set_rows_provider": ([p, VIO_ROWS_PROVIDER_FN, p], C.c_int),
        "srl_lio_vio_esikf": ([p, p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), p, C.c_int], C.c_int),
        "srl_lio_vio_photometric": ([p, p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), p, C.c_int], C.c_int),
        "srl_image_process_opts_default": ([C.POINTER(ImageProcessOpts)], None),
        "srl_lio_image_set_options": ([p, C.POINTER(ImageProcessOpts)], C.c_int),
        "srl_lio_image_set_steps": ([p, C.POINTER(ImageProcessSteps)], C.c_int),
        "srl_lio_image_process": ([p, p, C.c_int, C.c_int, C.c_int64, C.c_double, C.c_int, C.POINTER(ImageProcessResult)], C.c_int),
        "srl_lio_image_set_jpeg_step": ([p, IMAGE_JPEG_STEP_FN, p], C.c_int),
        "srl_lio_image_process_jpeg": ([p, p, C.c_int64, C.c_double, C.c_int, C.POINTER(ImageProcessResult)], C.c_int),
        "srl_lio_run_measurement_image_jpeg": ([p, C.c_double, p, p, p, C.c_int, p, p, C.c_int, C.c_double, C.c_double, p, C.c_int64,
                                                C.POINTER(ReplayResult), C.POINTER(ImageProcessResult)], C.c_int),
        "srl_lio_image_oft": ([p], C.c_void_p),
        "srl_lio_image_candidates": ([p, p, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_lio_image_time_last_process": ([p, C.POINTER(C.c_double)], C.c_int),
        "srl_time_unit_scale": ([C.c_int], C.c_double),
        "srl_livox_decode": ([p, p, C.c_int, C.c_double, C.POINTER(LivoxOpts), C.POINTER(LivoxReport)], C.c_int),
        "srl_points_info": ([p, C.POINTER(C.c_int), dp, dp], C.c_int),
        "srl_points_clear": ([p], C.c_int),
        "srl_points_cut": ([p, C.c_double, C.POINTER(PointsCutReport)], C.c_int),
        "srl_points_queue_download": ([p, p, p, p, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_points_cut_download": ([p, p, p, p, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_debug_points_fallbacks": ([p, C.POINTER(C.c_int64)], C.c_int),
        "srl_debug_undistorted_download": ([p, p, p, p, p, C.c_int, C.POINTER(C.c_int)], C.c_int),
        "srl_frame_undistort_cut": ([p, C.c_double, C.c_double, C.c_int, p, C.c_int, C.c_int, dp, dp, C.POINTER(C.c_int)], C.c_int),
        "srl_frame_point_times": ([p, p, C.c_int, p, p, p], C.c_int),
        "srl_lio_set_lidar_options": ([p, C.POINTER(LivoxOpts)], C.c_int),
        "srl_lio_feed_livox": ([p, p, C.c_int, C.c_double, C.POINTER(LivoxReport)], C.c_int),
        "srl_lio_points_info": ([p, C.POINTER(C.c_int), dp, dp, dp, dp], C.c_int),
        "srl_pc2_decode": ([p, p, C.c_size_t, C.POINTER(Pc2Layout), C.c_double, C.c_double, C.POINTER(Pc2Opts), C.POINTER(Pc2Report)], C.c_int),
        "srl_pc2_yaw_angles": ([p, C.c_size_t, C.POINTER(Pc2Layout), dp], C.c_int),
        "srl_lio_set_pc2_options": ([p, C.POINTER(Pc2Opts)], C.c_int),
        "srl_lio_feed_pointcloud2": ([p, p, C.c_size_t, C.POINTER(Pc2Layout), C.c_double, C.POINTER(Pc2Report)], C.c_int),
        "srl_lio_run_measurement_queued": ([p, C.c_double, p, p, p, C.c_int, C.c_double, C.c_double, C.c_double, C.POINTER(ReplayResult)], C.c_int),
        "srl_grid_sampling": ([p, C.c_int, C.c_double, p, C.POINTER(C.c_int)], C.c_int),
        "srl_debug_tr1_order": ([p, C.c_int, p], C.c_int),
        "srl_debug_tr1_order_by_relation": ([p, C.c_int, p], C.c_int),
    }
    for name, (argtypes, restype) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = lib
    return lib


def declared_symbols():
    """Every function name declared in include/srlivo_hip.h and include/srlivo_host.h."""
    names = []
    for hdr in ("srlivo_hip.h", "srlivo_hip_debug.h", "srlivo_host.h"):
        text = open(os.path.join(INCLUDE_DIR, hdr)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names += re.findall(r"\b(srl_[a-z0-9_]+)\s*\(", text)
    skip = {"srl_allreduce_fn", "srl_allgather_i64_fn", "srl_normal_eq_provider", "srl_probe_mix"}      # (types, and the inline helper of the header)
    return sorted(set(n for n in names if n not in skip))


def library_symbols():
    lib = load_library()
    return [n for n in declared_symbols() if hasattr(lib, n)]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def default_opts(**kw):
    o = IcpOpts()
    load_library().srl_icp_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def time_unit_scale(unit):
    """srl_time_unit_scale: cloudProcessing::setTimeUnit's float literal widened to double (1.e-6f is not 1e-6)"""
    return float(load_library().srl_time_unit_scale(int(unit)))


def livox_opts(n_scans=6, time_unit=TIME_UNIT_NS, blind=0.01, point_filter_num=1, time_unit_scale_value=None):
    """srl_livox_opts; the scale comes from srl_time_unit_scale(time_unit) unless given"""
    o = LivoxOpts()
    o.n_scans = int(n_scans)
    o.time_unit_scale = float(time_unit_scale(time_unit) if time_unit_scale_value is None else time_unit_scale_value)
    o.blind = float(blind)
    o.point_filter_num = int(point_filter_num)
    return o


def _livox_points(points):
    a = np.ascontiguousarray(points)
    if a.dtype != LIVOX_POINT_DTYPE:
        raise TypeError("Livox points must have LIVOX_POINT_DTYPE (the 20-byte CustomPoint record)")
    return a


def _livox_report_dict(r):
    return dict(valid=r.valid, picked=r.picked, appended=r.appended, last_end_time=r.last_end_time, first_timestamp=r.first_timestamp,
                last_timestamp=r.last_timestamp)


def pc2_opts(lidar_type, n_scans=16, scan_rate=10, point_filter_num=1, time_unit=TIME_UNIT_US, blind=0.01, time_unit_scale_value=None):
    """srl_pc2_opts; the scale comes from srl_time_unit_scale(time_unit) unless given"""
    o = Pc2Opts()
    o.lidar_type, o.n_scans, o.scan_rate, o.point_filter_num = int(lidar_type), int(n_scans), int(scan_rate), int(point_filter_num)
    o.time_unit_scale = float(time_unit_scale(time_unit) if time_unit_scale_value is None else time_unit_scale_value)
    o.blind = float(blind)
    return o


def pc2_message(points, lidar_type, point_step=None, offsets=None, height=1, row_pad=0, fill=0xA5):
    """A PointCloud2 `data` buffer for tests: points = PC2_POINT_DTYPES[lidar_type] records (x, y, z, time, ring), written field by field at
    `offsets` (dict x y z time ring -> byte offset inside a point; default: the driver's) into points of point_step bytes, height rows of
    len(points) / height points, each row followed by row_pad bytes.  Every byte that is no field is `fill`.  No field needs alignment.
    -> (uint8 array, Pc2Layout)"""
    a = np.ascontiguousarray(points, dtype=PC2_POINT_DTYPES[int(lidar_type)])
    step0, off0 = PC2_DRIVER_LAYOUTS[int(lidar_type)]
    point_step = int(step0 if point_step is None else point_step)
    off = dict(off0 if offsets is None else offsets)
    n, height = len(a), int(height)
    if height < 1 or n % height:
        raise ValueError("len(points) must be a multiple of height")
    width = n // height
    row_step = width * point_step + int(row_pad)
    buf = np.full((height, row_step), fill, dtype=np.uint8)
    body = buf[:, :width * point_step].reshape(height, width, point_step)
    for name in ("x", "y", "z", "time", "ring"):
        col = np.ascontiguousarray(a[name]).view(np.uint8).reshape(height, width, a.dtype[name].itemsize)
        if off[name] < 0 or off[name] + col.shape[2] > point_step:
            raise ValueError(f"field {name} does not fit inside point_step")
        body[:, :, off[name]:off[name] + col.shape[2]] = col
    lay = Pc2Layout(width=width, height=height, point_step=point_step, row_step=row_step, off_x=off["x"], off_y=off["y"], off_z=off["z"],
                    off_time=off["time"], off_ring=off["ring"], is_bigendian=0)
    return buf.reshape(-1), lay


def pc2_yaw_angles(data, layout):
    """srl_pc2_yaw_angles: atan2(double(y), double(x)) * 57.2957 per point, on the host (libm)"""
    d = np.ascontiguousarray(data, dtype=np.uint8)
    yaw = np.empty(int(layout.width) * int(layout.height))
    rc = load_library().srl_pc2_yaw_angles(_ptr(d), d.nbytes, C.byref(layout), _dptr(yaw))
    if rc != SRL_OK:
        raise SrlError(rc, "srl_pc2_yaw_angles")
    return yaw


def _pc2_report_dict(r):
    return dict(points=r.points, given_offset_time=r.given_offset_time, picked=r.picked, appended=r.appended, last_end_time=r.last_end_time,
                first_timestamp=r.first_timestamp, last_timestamp=r.last_timestamp)


def default_color_opts(**kw):
    o = ColorOpts()
    load_library().srl_color_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_color_select_opts(**kw):
    o = ColorSelectOpts()
    load_library().srl_color_select_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_color_track_opts(**kw):
    o = ColorTrackOpts()
    load_library().srl_color_track_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_flow_opts(**kw):
    o = FlowOpts()
    load_library().srl_flow_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _jpeg_bytes(jpeg):
    return np.frombuffer(jpeg, dtype=np.uint8) if isinstance(jpeg, (bytes, bytearray, memoryview)) else np.ascontiguousarray(jpeg, dtype=np.uint8).reshape(-1)


def jpeg_parse(jpeg):
    """srl_jpeg_parse (host only): the JpegInfo of a baseline JPEG stream; raises SrlError where it refuses"""
    d = _jpeg_bytes(jpeg)
    info = JpegInfo()
    rc = load_library().srl_jpeg_parse(_ptr(d), d.size, C.byref(info))
    if rc:
        raise SrlError(rc, "srl_jpeg_parse", "")
    return info


def jpeg_entropy_decode(jpeg, info=None):
    """srl_jpeg_entropy_decode (host only): (coef (total_blocks, 64) int16 natural order, qt (components, 64) uint16 natural order)"""
    d = _jpeg_bytes(jpeg)
    info = info if info is not None else jpeg_parse(d)
    coef = np.zeros((info.total_blocks, 64), dtype=np.int16)
    qt = np.zeros((3, 64), dtype=np.uint16)
    rc = load_library().srl_jpeg_entropy_decode(_ptr(d), d.size, C.byref(info), _ptr(coef), len(coef), _ptr(qt))
    if rc:
        raise SrlError(rc, "srl_jpeg_entropy_decode", "")
    return coef, qt[:info.components]


def default_image_prep_opts(**kw):
    """srl_image_prep_opts_default with the keywords applied (dist: a sequence of five)"""
    o = ImagePrepOpts()
    load_library().srl_image_prep_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, (C.c_double * 5)(*v) if k == "dist" else v)
    return o


def image_prep_build_map(opts):
    """srl_image_prep_build_map (host only): (map1 (rows, cols, 2) int16, map2 (rows, cols) uint16); raises SrlError where it refuses"""
    n = max(int(opts.rows), 0) * max(int(opts.cols), 0)
    map1 = np.zeros((max(n, 1), 2), dtype=np.int16)
    map2 = np.zeros(max(n, 1), dtype=np.uint16)
    rc = load_library().srl_image_prep_build_map(C.byref(opts), _ptr(map1), _ptr(map2))
    if rc != SRL_OK:
        raise SrlError(rc, "srl_image_prep_build_map", "")
    return map1[:n].reshape(opts.rows, opts.cols, 2), map2[:n].reshape(opts.rows, opts.cols)


def image_resize_build_tables(src_len, dst_len):
    """srl_image_resize_build_tables (host only): (ofs (dst_len,) int32, coef (dst_len, 2) int16); raises SrlError where it refuses"""
    n = max(int(dst_len), 1)
    ofs = np.zeros(n, dtype=np.int32)
    coef = np.zeros((n, 2), dtype=np.int16)
    rc = load_library().srl_image_resize_build_tables(int(src_len), int(dst_len), _ptr(ofs), _ptr(coef))
    if rc != SRL_OK:
        raise SrlError(rc, "srl_image_resize_build_tables", "")
    return ofs, coef


def default_consensus_opts(model, **kw):
    o = ConsensusOpts()
    load_library().srl_consensus_opts_default(C.byref(o), int(model))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _consensus_opts(model, opts, kw):
    """opts (None = the model's defaults) with the keywords applied to a copy"""
    if opts is None:
        return default_consensus_opts(model, **kw)
    o = ConsensusOpts(opts.threshold, opts.confidence, opts.hypotheses, opts.seed)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_color_cloud_opts(**kw):
    o = ColorCloudOpts()
    load_library().srl_color_cloud_opts_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def heap_topk(distances, K):
    """The device kernels' libstdc++-heap restatement (csrc/srl_heap.h) run on the host: read-out order of candidate indices."""
    d = np.ascontiguousarray(distances, dtype=np.float64)
    out = np.empty(K, dtype=np.int32)
    n = load_library().srl_debug_heap_topk(_ptr(d), len(d), int(K), _ptr(out))
    if n < 0:
        raise SrlError(n, "srl_debug_heap_topk")
    return out[:n].copy()


class PinnedArray:
    """A float64 numpy array in page-locked host memory (srl_pinned_alloc): srl_sweep_upload DMAs straight out of it."""

    def __init__(self, shape):
        self.lib = load_library()
        n = int(np.prod(shape))
        self.ptr = C.c_void_p()
        rc = self.lib.srl_pinned_alloc(max(n, 1) * 8, C.byref(self.ptr))
        if rc:
            raise SrlError(rc, "srl_pinned_alloc")
        buf = (C.c_double * max(n, 1)).from_address(self.ptr.value)
        self.array = np.frombuffer(buf, dtype=np.float64, count=n).reshape(shape)

    def close(self):
        if self.ptr:
            self.array = None
            self.lib.srl_pinned_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

def comm_set_library(path):
    """debug / test hook (srl_comm_set_library): resolve the nccl* entry points from `path`; only before the first communicator call"""
    rc = load_library().srl_comm_set_library(os.fsencode(path))
    if rc:
        raise SrlError(rc, "srl_comm_set_library", "a communicator call has already resolved this process's RCCL")


def comm_backend_info():
    """(path of the RCCL shared object in use, ncclGetVersion, found-already-loaded-in-the-process) or raises."""
    buf = C.create_string_buffer(512)
    ver, pre = C.c_int(), C.c_int()
    rc = load_library().srl_comm_backend_info(buf, 512, C.byref(ver), C.byref(pre))
    if rc:
        raise SrlError(rc, "srl_comm_backend_info", buf.value.decode())
    return buf.value.decode(), ver.value, bool(pre.value)


def shard_range(n, nranks, rank):
    b, c = C.c_int(), C.c_int()
    load_library().srl_shard_range(n, nranks, rank, C.byref(b), C.byref(c))
    return b.value, c.value


def shard_budget(max_num_residuals, accepted_per_rank, rank):
    arr = np.ascontiguousarray(accepted_per_rank, dtype=np.int64)
    b, m = C.c_int64(), C.c_int()
    load_library().srl_shard_budget(int(max_num_residuals), arr.ctypes.data_as(C.POINTER(C.c_int64)), len(arr), rank,
                                    C.byref(b), C.byref(m))
    return b.value, m.value


def grid_sampling(world_xyz, size_voxel):
    w = _f64(world_xyz, (-1, 3))
    idx = np.empty(len(w), dtype=np.int32)
    n = C.c_int()
    rc = load_library().srl_grid_sampling(_ptr(w), len(w), float(size_voxel), _ptr(idx), C.byref(n))
    if rc:
        raise SrlError(rc, "srl_grid_sampling")
    return idx[: n.value].copy()


def tr1_order(keys_xyz, by_relation=False):
    """Iteration order of std::tr1::unordered_map<voxel, ...> after inserting the distinct int16 keys in order: the flat replay of
    host/tr1_order.h, or (by_relation) the pairwise relation of host/tr1_relation.h the device ordering evaluates."""
    k = np.ascontiguousarray(keys_xyz, dtype=np.int16).reshape(-1, 3)
    out = np.empty(len(k), dtype=np.int32)
    name = "srl_debug_tr1_order_by_relation" if by_relation else "srl_debug_tr1_order"
    rc = getattr(load_library(), name)(_ptr(k), len(k), _ptr(out))
    if rc:
        raise SrlError(rc, name)
    return out


def make_frame(q, t, t_last, R_il=None, t_il=None, frame_id=100):
    f = Frame()
    f.q[:] = list(np.asarray(q, dtype=np.float64))
    f.t[:] = list(np.asarray(t, dtype=np.float64))
    f.t_last[:] = list(np.asarray(t_last, dtype=np.float64))
    f.R_il[:] = list(np.eye(3).ravel() if R_il is None else np.asarray(R_il, dtype=np.float64).ravel())
    f.t_il[:] = list(np.zeros(3) if t_il is None else np.asarray(t_il, dtype=np.float64))
    f.frame_id = int(frame_id)
    return f


class Context:
    """Kernel-level C-ABI (srl_ctx)."""

    def __init__(self, device=0, handle=None):
        self.lib = load_library()
        self._own = handle is None
        if handle is None:
            h = C.c_void_p()
            rc = self.lib.srl_ctx_create(device, C.byref(h))
            if rc:
                raise SrlError(rc, "srl_ctx_create", self.lib.srl_status_str(rc).decode())
            handle = h
        self.h = handle
        self._cb = None
        if os.environ.get("SRL_ABLATE"):      # profiling tools only (tools/*.py, tools/*.sh): the library itself reads no env
            self.lib.srl_debug_set_ablate(self.h, int(os.environ["SRL_ABLATE"]))

    def close(self):
        if self.h and self._own:
            self.lib.srl_ctx_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what, ok=()):
        if rc and rc not in ok:
            raise SrlError(rc, what, (self.lib.srl_last_error(self.h) or b"").decode())
        return rc

    def jpeg_decode(self, jpeg):
        """srl_jpeg_decode: a baseline JPEG stream (bytes or uint8 array) to a BGR frame that stays on the device.  Returns JpegInfo."""
        d = _jpeg_bytes(jpeg)
        info = JpegInfo()
        self._chk(self.lib.srl_jpeg_decode(self.h, _ptr(d), d.size, C.byref(info)), "srl_jpeg_decode")
        return info

    def jpeg_download(self, rows, cols):
        """srl_jpeg_download: the last decoded frame, (rows, cols, 3) uint8 B G R (rows, cols: JpegInfo's)"""
        out = np.zeros((rows, cols, 3), dtype=np.uint8)
        self._chk(self.lib.srl_jpeg_download(self.h, _ptr(out), out.strides[0]), "srl_jpeg_download")
        return out

    def jpeg_idct_blocks(self, coef, qt):
        """srl_jpeg_idct_blocks (debug): coef (n, 64) int16 and qt (64,) uint16, both natural order -> (n, 64) uint8"""
        c = np.ascontiguousarray(coef, dtype=np.int16).reshape(-1, 64)
        q = np.ascontiguousarray(qt, dtype=np.uint16).reshape(64)
        out = np.zeros((len(c), 64), dtype=np.uint8)
        self._chk(self.lib.srl_jpeg_idct_blocks(self.h, _ptr(c), len(c), _ptr(q), _ptr(out)), "srl_jpeg_idct_blocks")
        return out

    def map_upload(self, keys, counts, xyz, cap=20):
        keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(len(counts), cap, 3)
        self._chk(self.lib.srl_map_upload(self.h, _ptr(keys), _ptr(counts), _ptr(xyz), len(counts), cap), "srl_map_upload")

    def map_insert(self, world_xyz, voxel_size=1.0, cap=20, min_dist=0.15, min_num_points=0):
        w = _f64(world_xyz, (-1, 3))
        added = C.c_int()
        self._chk(self.lib.srl_map_insert(self.h, _ptr(w), len(w), voxel_size, cap, min_dist, min_num_points, C.byref(added)), "srl_map_insert")
        return added.value

    def map_insert_report(self, world_xyz, voxel_size=1.0, cap=20, min_dist=0.15, min_num_points=0, ref_z=0.0):
        """srl_map_insert_report: map_insert that also says what it stored.  Returns (outcome, cloud, num_added): outcome uint8 per point
        (0 not stored, 1 appended to an existing voxel, 2 created its voxel), cloud (m, 4) float32 rows x, y, z, intensity of the
        appended points in batch order (cloud_world; intensity = 50 (z - ref_z))."""
        w = _f64(world_xyz, (-1, 3))
        n = len(w)
        outcome = np.zeros(n, dtype=np.uint8)
        cloud = np.zeros((n, 4), dtype=np.float32)
        m, added = C.c_int(), C.c_int()
        self._chk(self.lib.srl_map_insert_report(self.h, _ptr(w), n, voxel_size, cap, min_dist, min_num_points, float(ref_z), _ptr(outcome), _ptr(cloud),
                                                 C.byref(m), C.byref(added)), "srl_map_insert_report")
        return outcome, cloud[: m.value].copy(), added.value

    def map_size(self):
        npnt, nv = C.c_int64(), C.c_int32()
        self._chk(self.lib.srl_map_size(self.h, C.byref(npnt), C.byref(nv)), "srl_map_size")
        return npnt.value, nv.value

    def map_probe_checksum(self, world_xyz=None, stride=1, voxel_size=1.0):
        """srl_map_probe_checksum: world_xyz None = the world points of the last committed frame"""
        out = C.c_uint64()
        if world_xyz is None:
            rc = self.lib.srl_map_probe_checksum(self.h, None, 0, int(stride), float(voxel_size), C.byref(out))
        else:
            w = _f64(world_xyz, (-1, 3))
            rc = self.lib.srl_map_probe_checksum(self.h, _ptr(w), len(w), int(stride), float(voxel_size), C.byref(out))
        self._chk(rc, "srl_map_probe_checksum")
        return out.value

    def map_download(self, cap=20):
        _, nv = self.map_size()
        keys = np.zeros((nv, 3), dtype=np.int16)
        counts = np.zeros(nv, dtype=np.int32)
        xyz = np.zeros((nv, cap, 3), dtype=np.float32)
        self._chk(self.lib.srl_map_download(self.h, _ptr(keys), _ptr(counts), _ptr(xyz), nv), "srl_map_download")
        return keys, counts, xyz

    def map_remove_far(self, location, distance):
        """srl_map_remove_far (removePointsFarFromLocation): erase the voxels whose first point lies farther than `distance` from
        `location`; the survivors keep their creation order.  Returns (voxels_removed, points_removed)."""
        nv, npnt = C.c_int32(), C.c_int64()
        loc = _f64(location).ravel()
        self._chk(self.lib.srl_map_remove_far(self.h, _dptr(loc), float(distance), C.byref(nv), C.byref(npnt)), "srl_map_remove_far")
        return nv.value, npnt.value

    def color_map_create(self, opts=None):
        """srl_color_map_create: the colour voxel map (addPointToColorMap); opts = ColorOpts, None = the yaml values 0.1 / 50 / 0.01 / 1"""
        o = default_color_opts() if opts is None else opts
        self._chk(self.lib.srl_color_map_create(self.h, C.byref(o)), "srl_color_map_create")

    def color_map_destroy(self):
        self._chk(self.lib.srl_color_map_destroy(self.h), "srl_color_map_destroy")

    def color_map_insert(self, world_xyz=None, time_sweep_end=0.0, time_last_process=0.0, n_frame=None, want_outcome=True, want_stored=True,
                         want_visited=True):
        """srl_color_map_insert.  world_xyz None = the world points of the last committed frame (n_frame: their number, for the output
        capacities; default srl_frame_size).  Returns (outcome uint8[n] or None, stored records (COLOR_STORED_DTYPE) or None,
        visited (m, 3) int32 or None, ColorTotals)."""
        if world_xyz is None:
            w, n = None, (self.frame_size() if n_frame is None else int(n_frame))
        else:
            w = _f64(world_xyz, (-1, 3))
            n = len(w)
        outcome = np.zeros(n, dtype=np.uint8) if want_outcome else None
        stored = np.zeros(n, dtype=COLOR_STORED_DTYPE) if want_stored else None
        visited = np.zeros((n, 3), dtype=np.int32) if want_visited else None
        tot = ColorTotals()
        self._chk(self.lib.srl_color_map_insert(self.h, _ptr(w), n, float(time_sweep_end), float(time_last_process), _ptr(outcome), _ptr(stored), n,
                                                _ptr(visited), n, C.byref(tot)), "srl_color_map_insert")
        return (outcome, None if stored is None else stored[: tot.stored].copy(), None if visited is None else visited[: tot.visited].copy(), tot)

    def color_map_size(self):
        """(points, voxels, registered, grid cells)"""
        a, b, c, d = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64()
        self._chk(self.lib.srl_color_map_size(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "srl_color_map_size")
        return a.value, b.value, c.value, d.value

    def color_map_download(self):
        """(keys (V, 3) int16, counts, last_visited_time, xyz (P, 3) float32 voxel after voxel in slot order, point_index (P))"""
        npnt, nv, _, _ = self.color_map_size()
        keys = np.zeros((nv, 3), dtype=np.int16)
        counts = np.zeros(nv, dtype=np.int32)
        times = np.zeros(nv, dtype=np.float64)
        xyz = np.zeros((npnt, 3), dtype=np.float32)
        pidx = np.zeros(npnt, dtype=np.int32)
        self._chk(self.lib.srl_color_map_download(self.h, _ptr(keys), _ptr(counts), _ptr(times), nv, _ptr(xyz), _ptr(pidx), npnt), "srl_color_map_download")
        return keys, counts, times, xyz, pidx

    def color_registered_download(self, first=0, count=None):
        """the device's rgb_points_vec[first : first + count] as COLOR_STORED_DTYPE records"""
        if count is None:
            count = self.color_map_size()[2] - first
        out = np.zeros(count, dtype=COLOR_STORED_DTYPE)
        self._chk(self.lib.srl_color_registered_download(self.h, int(first), int(count), _ptr(out)), "srl_color_registered_download")
        return out

    def color_image_upload(self, bgr):
        """srl_color_image_upload: bgr (rows, cols, 3) uint8, the frame's rgb_image as OpenCV holds it (rows may be strided)"""
        img = np.asarray(bgr)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.strides[2] != 1 or img.strides[1] != 3:
            img = np.ascontiguousarray(bgr, dtype=np.uint8)
        self._keep_image = img
        self._chk(self.lib.srl_color_image_upload(self.h, _ptr(img), img.shape[0], img.shape[1], img.strides[0]), "srl_color_image_upload")

    def color_map_render(self, camera, voxels_xyz, obs_time):
        """srl_color_map_render: camera = ColorCamera, voxels_xyz (n, 3) int32 (repeats allowed).  Returns ColorRenderTotals."""
        v = np.ascontiguousarray(voxels_xyz, dtype=np.int32).reshape(-1, 3)
        tot = ColorRenderTotals()
        self._chk(self.lib.srl_color_map_render(self.h, C.byref(camera), _ptr(v) if len(v) else None, len(v), float(obs_time), C.byref(tot)),
                  "srl_color_map_render")
        return tot

    def color_map_select(self, camera, rows, cols, voxels_xyz=None, opts=None, totals_only=False):
        """srl_color_map_select: camera = ColorCamera, voxels_xyz (n, 3) int32 or None (all points), opts = ColorSelectOpts (None = 10.0, 1,
        list mode, 0.1, 200).  Returns (records (COLOR_SELECTED_DTYPE), ColorSelectTotals): the totals are asked for first, then the
        records at their exact number (the call changes nothing in the map)."""
        v = np.zeros((0, 3), np.int32) if voxels_xyz is None else np.ascontiguousarray(voxels_xyz, dtype=np.int32).reshape(-1, 3)
        o = default_color_select_opts() if opts is None else opts
        tot = ColorSelectTotals()
        lp = _ptr(v) if len(v) else None
        self._chk(self.lib.srl_color_map_select(self.h, C.byref(camera), int(rows), int(cols), lp, len(v), C.byref(o), None, 0, C.byref(tot)),
                  "srl_color_map_select")
        out = np.zeros(tot.selected, dtype=COLOR_SELECTED_DTYPE)
        if tot.selected and not totals_only:
            self._chk(self.lib.srl_color_map_select(self.h, C.byref(camera), int(rows), int(cols), lp, len(v), C.byref(o), _ptr(out), len(out),
                                                    C.byref(tot)), "srl_color_map_select")
        return out, tot

    def consensus_fundamental(self, last_xy, cur_xy, opts=None, **kw):
        """srl_consensus_fundamental: last_xy, cur_xy (n, 2) float32; opts = ConsensusOpts (None = 1.0, 0.997, 512, seed 0; keywords
        override fields).  Returns (mask (n,) uint8, ConsensusResult)."""
        a = np.ascontiguousarray(last_xy, dtype=np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(cur_xy, dtype=np.float32).reshape(-1, 2)
        if len(a) != len(b):
            raise ValueError("last_xy and cur_xy differ in length")
        o = _consensus_opts(SRL_CONSENSUS_FUNDAMENTAL, opts, kw)
        n = len(a)
        mask = np.zeros(n, dtype=np.uint8)
        res = ConsensusResult()
        self._chk(self.lib.srl_consensus_fundamental(self.h, _ptr(a) if n else None, _ptr(b) if n else None, n, C.byref(o), _ptr(mask) if n else None,
                                                     C.byref(res)), "srl_consensus_fundamental")
        return mask, res

    def consensus_pnp(self, xyz, uv, fx_fy_cx_cy, opts=None, **kw):
        """srl_consensus_pnp: xyz (n, 3), uv (n, 2) float32, the intrinsics fx, fy, cx, cy; opts = ConsensusOpts (None = 1.5, 0.99, 200,
        seed 0; keywords override fields).  Returns (ascending inlier indices int32, ConsensusResult)."""
        x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        u = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        if len(x) != len(u):
            raise ValueError("xyz and uv differ in length")
        K = _f64(fx_fy_cx_cy, (4,))
        o = _consensus_opts(SRL_CONSENSUS_PNP, opts, kw)
        n = len(x)
        idx = np.zeros(n, dtype=np.int32)
        cnt = C.c_int()
        res = ConsensusResult()
        self._chk(self.lib.srl_consensus_pnp(self.h, _ptr(x) if n else None, _ptr(u) if n else None, n, _dptr(K), C.byref(o), _ptr(idx) if n else None,
                                             C.byref(cnt), C.byref(res)), "srl_consensus_pnp")
        return idx[:cnt.value].copy(), res

    def debug_consensus_download(self):
        """srl_debug_consensus_download: the last consensus call's trace as a dict -- model, hypotheses, n, slots, usable (ascending int32),
        norm (6,) float64, samples (H, 8) int32, models (H, slots, 12) float64, counts (H, slots) int32 (-1: no model)"""
        info = DebugConsensusInfo()
        usable = np.zeros(SRL_CONSENSUS_MAX_POINTS, dtype=np.int32)
        H = SRL_CONSENSUS_MAX_HYPOTHESES
        samples = np.zeros((H, 8), dtype=np.int32)
        models = np.zeros(H * 4 * 12, dtype=np.float64)
        counts = np.zeros(H * 4, dtype=np.int32)
        self._chk(self.lib.srl_debug_consensus_download(self.h, C.byref(info), _ptr(usable), len(usable), _ptr(samples), _ptr(models), _ptr(counts), H),
                  "srl_debug_consensus_download")
        H, S = info.hypotheses, info.slots
        return dict(model=info.model, hypotheses=H, n=info.n, slots=S, usable=usable[:info.usable].copy(), norm=np.array(info.norm[:], dtype=np.float64),
                    samples=samples[:H].copy(), models=models[:H * S * 12].reshape(H, S, 12).copy(), counts=counts[:H * S].reshape(H, S).copy())

    def color_map_track_update(self, camera, rows, cols, tracked, candidates, opts=None, with_outcomes=True, totals_only=False):
        """srl_color_map_track_update: camera = ColorCamera, tracked = COLOR_TRACK_POINT_DTYPE records in the caller's order, candidates =
        pool positions (int32) in the order of points_rgb_vec_for_projection, opts = ColorTrackOpts (None = 10.0, 300).  Returns (records
        (COLOR_TRACK_POINT_DTYPE): the kept points, then the added ones; tracked outcome (n,) uint8 or None; candidate outcome
        (n_candidates,) uint8 or None; ColorTrackTotals).  One call: kept + added is at most n + min(n_candidates, max(maximum, 1))."""
        t = np.ascontiguousarray(tracked, dtype=COLOR_TRACK_POINT_DTYPE).reshape(-1)
        c = np.ascontiguousarray(candidates, dtype=np.int32).reshape(-1)
        o = default_color_track_opts() if opts is None else opts
        tot = ColorTrackTotals()
        out = None if totals_only else np.zeros(len(t) + min(len(c), max(int(o.maximum_tracked_points), 1)), dtype=COLOR_TRACK_POINT_DTYPE)
        t_out = np.zeros(len(t), dtype=np.uint8) if with_outcomes else None
        c_out = np.zeros(len(c), dtype=np.uint8) if with_outcomes else None
        self._chk(self.lib.srl_color_map_track_update(self.h, C.byref(camera), int(rows), int(cols), _ptr(t) if len(t) else None, len(t),
                                                      _ptr(c) if len(c) else None, len(c), C.byref(o), _ptr(out) if out is not None and len(out) else None,
                                                      0 if out is None else len(out), _ptr(t_out) if len(t) else None, _ptr(c_out) if len(c) else None,
                                                      C.byref(tot)), "srl_color_map_track_update")
        return (None if out is None else out[:tot.kept + tot.added].copy()), t_out, c_out, tot

    def color_map_vio_rows(self, args, points, with_rows=True, with_outcome=True):
        """srl_color_map_vio_rows: args = ColorVioArgs, points = COLOR_VIO_POINT_DTYPE records in the caller's order.  Returns
        (ColorVioSums, rows (n, 24) float64 or None, outcome (n,) uint8 or None)."""
        pts = np.ascontiguousarray(points, dtype=COLOR_VIO_POINT_DTYPE)
        n = len(pts)
        sums = ColorVioSums()
        rows = np.zeros((n, 24), dtype=np.float64) if with_rows else None
        outcome = np.zeros(n, dtype=np.uint8) if with_outcome else None
        self._chk(self.lib.srl_color_map_vio_rows(self.h, C.byref(args), _ptr(pts) if n else None, n, C.byref(sums), _ptr(rows) if n else None,
                                                  _ptr(outcome) if n else None), "srl_color_map_vio_rows")
        return sums, rows, outcome

    def color_map_export_cloud(self, first=0, count=-1, opts=None, with_index=True, totals_only=False):
        """srl_color_map_export_cloud over rgb_points_vec[first : first + count] (count < 0: to the end); opts = ColorCloudOpts (None =
        1 view, ascending, no time cut).  Returns (records (COLOR_CLOUD_DTYPE), point_index or None, ColorCloudTotals): the totals are
        asked for first, then the records at their exact number (the call changes nothing)."""
        o = default_color_cloud_opts() if opts is None else opts
        tot = ColorCloudTotals()
        self._chk(self.lib.srl_color_map_export_cloud(self.h, int(first), int(count), C.byref(o), None, None, 0, C.byref(tot)), "srl_color_map_export_cloud")
        out = np.zeros(tot.published, dtype=COLOR_CLOUD_DTYPE)
        idx = np.zeros(tot.published, dtype=np.int32) if with_index else None
        if tot.published and not totals_only:
            self._chk(self.lib.srl_color_map_export_cloud(self.h, int(first), int(count), C.byref(o), _ptr(out), _ptr(idx), len(out), C.byref(tot)),
                      "srl_color_map_export_cloud")
        return out, idx, tot

    @staticmethod
    def _color_state_arrays(n):
        return (np.zeros((n, 3), dtype=np.int16), np.zeros(n, dtype=np.int16), np.zeros((n, 3), dtype=np.float32), np.zeros(n, dtype=np.float64),
                np.zeros(n, dtype=np.float64))

    def color_map_download_rgb(self):
        """(rgb (P, 3) int16, N_rgb, cov_rgb (P, 3) float32, observe_distance, last_observe_time) in the order of color_map_download's xyz"""
        out = self._color_state_arrays(self.color_map_size()[0])
        self._chk(self.lib.srl_color_map_download_rgb(self.h, *[_ptr(a) for a in out], len(out[1])), "srl_color_map_download_rgb")
        return out

    def color_registered_rgb(self, first=0, count=None):
        """the same fields for the device's rgb_points_vec[first : first + count]"""
        if count is None:
            count = self.color_map_size()[2] - first
        out = self._color_state_arrays(int(count))
        self._chk(self.lib.srl_color_registered_rgb(self.h, int(first), int(count), *[_ptr(a) for a in out]), "srl_color_registered_rgb")
        return out

    def color_map_rebuilds(self):
        a, b = C.c_int32(), C.c_int32()
        self._chk(self.lib.srl_debug_color_map_rebuilds(self.h, C.byref(a), C.byref(b)), "srl_debug_color_map_rebuilds")
        return a.value, b.value

    COLOR_EPOCHS = ("scratch_epoch", "select_epoch", "track_pool_epoch", "track_cell_epoch", "select_counter", "track_pool_counter",
                    "track_cell_counter", "scratch_counter", "render_epoch")

    def color_epochs(self):
        """test hook: the numbers of the colour map's never-cleared structures as a dict (COLOR_EPOCHS; srl_debug_color_epochs)"""
        out = (C.c_uint32 * 9)()
        self._chk(self.lib.srl_debug_color_epochs(self.h, out), "srl_debug_color_epochs")
        return dict(zip(self.COLOR_EPOCHS, (int(v) for v in out)))

    def set_color_epochs(self, calls_to_epoch_wrap=-1, calls_to_counter_wrap=-1):
        """test hook: the next k calls of each owner use the family's last k values, call k + 1 wraps; -1 leaves a family alone
        (srl_debug_set_color_epochs)"""
        self._chk(self.lib.srl_debug_set_color_epochs(self.h, int(calls_to_epoch_wrap), int(calls_to_counter_wrap)), "srl_debug_set_color_epochs")

    def sweep_upload(self, raw_xyz):
        r = _f64(raw_xyz, (-1, 3))
        self._chk(self.lib.srl_sweep_upload(self.h, _ptr(r), len(r)), "srl_sweep_upload")

    def sweep_prefetch(self, raw_xyz):
        r = _f64(raw_xyz, (-1, 3))
        self._keep_prefetch = r                   # a page-locked source must outlive the copy
        self._chk(self.lib.srl_sweep_prefetch(self.h, _ptr(r), len(r)), "srl_sweep_prefetch")

    def sweep_wait(self):
        self._chk(self.lib.srl_sweep_wait(self.h), "srl_sweep_wait")

    def sweep_swap(self):
        self._chk(self.lib.srl_sweep_swap(self.h), "srl_sweep_swap")

    def sweep_shard(self):
        b, c, t = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.srl_sweep_shard(self.h, C.byref(b), C.byref(c), C.byref(t)), "srl_sweep_shard")
        return b.value, c.value, t.value

    def set_taps(self, on):
        self._chk(self.lib.srl_set_taps(self.h, int(on)), "srl_set_taps")

    def set_profiling(self, on):
        self._chk(self.lib.srl_set_profiling(self.h, int(on)), "srl_set_profiling")

    def timing_mark(self):
        """the light profiling's sums start here (no read-back, an armed launch stays armed): srl_timing_mark"""
        self._chk(self.lib.srl_timing_mark(self.h), "srl_timing_mark")

    def set_profiling_period(self, period):
        """light profiling (mode 2): time every period-th association launch only (2 event records per period launches)"""
        self._chk(self.lib.srl_set_profiling_period(self.h, int(period)), "srl_set_profiling_period")

    def timing(self):
        t = Timing()
        self._chk(self.lib.srl_get_timing(self.h, C.byref(t)), "srl_get_timing")
        return t

    def _select(self, opts):
        """test hook: the selection path wished for with default_opts(select_mode=...) (srl_debug_set_select_mode; sticky per context)"""
        mode = int(getattr(opts, "select_mode", 0) or 0)
        if mode != getattr(self, "_select_mode", 0):
            self._chk(self.lib.srl_debug_set_select_mode(self.h, mode), "srl_debug_set_select_mode")
            self._select_mode = mode

    def build_residuals(self, frame, opts, allow=(SRL_ERR_NAN_PLANARITY,)):
        self._select(opts)
        out = NormalEq()
        rc = self._chk(self.lib.srl_build_residuals(self.h, C.byref(frame), C.byref(opts), C.byref(out)), "srl_build_residuals", ok=allow)
        return out, rc

    def build_residuals_overlap(self, frame, opts, fn, allow=(SRL_ERR_NAN_PLANARITY,)):
        """srl_build_residuals with a host callback (a Python callable without arguments) run while the kernels are in flight."""
        self._select(opts)
        out = NormalEq()
        cb = C.CFUNCTYPE(None, C.c_void_p)(lambda _u: fn())
        rc = self._chk(self.lib.srl_build_residuals_overlap(self.h, C.byref(frame), C.byref(opts), C.byref(out), cb, None),
                       "srl_build_residuals_overlap", ok=allow)
        return out, rc

    def pin_thread_to_gpu_numa(self):
        """restrict the calling thread to the CPUs of the GPU's NUMA node; returns the node, or None when the topology is unreadable"""
        node = C.c_int(-1)
        rc = self.lib.srl_thread_pin_to_gpu_numa(self.h, C.byref(node))
        return node.value if rc == 0 else None

    def fetch_neighbors(self, K=20):
        _, n, _ = self.sweep_shard()
        ids = np.empty((n, K), dtype=np.int32)
        status = np.empty(n, dtype=np.uint8)
        ncand = np.empty(n, dtype=np.int32)
        self._chk(self.lib.srl_fetch_neighbors(self.h, _ptr(ids), _ptr(status), _ptr(ncand)), "srl_fetch_neighbors")
        return ids, status, ncand

    def fetch_residuals(self):
        _, n, _ = self.sweep_shard()
        normal = np.empty((n, 3)); a2d = np.empty(n); w = np.empty(n); off = np.empty(n); d = np.empty(n); J = np.empty((n, 6))
        self._chk(self.lib.srl_fetch_residuals(self.h, _ptr(normal), _ptr(a2d), _ptr(w), _ptr(off), _ptr(d), _ptr(J)), "srl_fetch_residuals")
        return dict(normal=normal, a2D=a2d, weight=w, norm_offset=off, distance=d, jacobian=J)

    def search_neighbors(self, world_xyz, nb=1, size=1.0, K=20, thr=1):
        q = _f64(world_xyz, (-1, 3))
        ids = np.empty((len(q), K), dtype=np.int32)
        xyz = np.empty((len(q), K, 3), dtype=np.float32)
        nf = np.empty(len(q), dtype=np.int32)
        self._chk(self.lib.srl_search_neighbors(self.h, _ptr(q), len(q), nb, size, K, thr, _ptr(ids), _ptr(xyz), _ptr(nf)), "srl_search_neighbors")
        return ids, xyz, nf

    def set_launch_shape(self, kpw, wpb):
        self._chk(self.lib.srl_debug_set_launch_shape(self.h, int(kpw), int(wpb)), "srl_debug_set_launch_shape")

    def set_fused_reduce(self, on):
        self._chk(self.lib.srl_debug_set_fused_reduce(self.h, 1 if on else 0), "srl_debug_set_fused_reduce")

    def set_bound_culling(self, mode):
        """test hook: 0 = every pass visits every found voxel (no use of the previous pass's neighbourhood bounds); 1 (default) = the
        bounds cull voxels and give the prefilter its threshold; 2 = they cull voxels only, the threshold is searched"""
        self._chk(self.lib.srl_debug_set_bound_culling(self.h, int(mode)), "srl_debug_set_bound_culling")

    def set_neighbour_records(self, on):
        """test hook: 1 (default) = the r = 1 fast path takes a keypoint's 27 voxel lookups from its home voxel's neighbour record;
        0 = it looks every voxel up in the table"""
        self._chk(self.lib.srl_debug_set_neighbour_records(self.h, 1 if on else 0), "srl_debug_set_neighbour_records")

    def neighbour_records_download(self):
        """the neighbour records of the map's voxels, (voxels, 32) uint32 in the slab order of map_download"""
        _, nv = self.map_size()
        words = np.zeros((nv, 32), dtype=np.uint32)
        self._chk(self.lib.srl_debug_neighbour_records_download(self.h, _ptr(words), nv), "srl_debug_neighbour_records_download")
        return words

    def bounds_download(self):
        """the neighbourhood bounds the last pass left: (keypoints, 4) float32 {x, y, z, tau}; empty after anything that voids them"""
        _, n, _ = self.sweep_shard()
        out = np.zeros((max(n, 1), 4), dtype=np.float32)
        got = C.c_int()
        self._chk(self.lib.srl_debug_bounds_download(self.h, _ptr(out), len(out), C.byref(got)), "srl_debug_bounds_download")
        return out[: got.value].copy()

    def set_search_select_mode(self, mode):
        self._chk(self.lib.srl_debug_set_search_select_mode(self.h, int(mode)), "srl_debug_set_search_select_mode")

    def set_armed_launch(self, on):
        """armed launches (the next pass's kernel enqueued while the current one runs): on by default"""
        mode = int(on) if on in (0, 1, 2) and not isinstance(on, bool) else (1 if on else 0)      # 2: armed behind every eligible pass (no policy)
        self._chk(self.lib.srl_set_armed_launch(self.h, mode), "srl_set_armed_launch")

    def solve_end(self):
        """the caller's ESIKF loop on the current sweep has ended (srl_solve_end)"""
        self._chk(self.lib.srl_solve_end(self.h), "srl_solve_end")

    def disarm(self):
        self._chk(self.lib.srl_disarm(self.h), "srl_disarm")

    def arm_stats(self):
        out = (C.c_uint64 * 4)()
        self._chk(self.lib.srl_get_arm_stats(self.h, out), "srl_get_arm_stats")
        return dict(zip(("armed", "fired", "cancelled", "expired"), (int(v) for v in out)))

    def set_pose_box(self, kind):
        """0: pinned host memory + device relay; 1: fine-grained device memory written through the BAR (raises if not CPU-visible)"""
        self._chk(self.lib.srl_debug_set_pose_box(self.h, int(kind)), "srl_debug_set_pose_box")

    FRAME_STAGES = ("upload", "select_group", "select_download", "select_host_order", "select_gather", "commit_transform", "commit_download",
                    "insert_sort", "insert_segments", "insert_lookup_create", "insert_replay")

    def set_frame_epoch(self, frames_to_wrap):
        """test hook: the epoch of the frame pipeline's scratch tables wraps `frames_to_wrap` frames from now (srl_debug_set_frame_epoch)"""
        self._chk(self.lib.srl_debug_set_frame_epoch(self.h, int(frames_to_wrap)), "srl_debug_set_frame_epoch")

    def set_frame_counters(self, calls_to_wrap):
        """test hook: the 32-bit counters of the frame pipeline's scratch tables and the tag of the sub-sample's seen words wrap
        `calls_to_wrap` calls of each owner from now; apply it after the sub-sample's buffers exist (srl_debug_set_frame_counters)"""
        self._chk(self.lib.srl_debug_set_frame_counters(self.h, int(calls_to_wrap)), "srl_debug_set_frame_counters")

    def frame_counters(self):
        """(counter of the selection's table, counter of the insertion's table, tag of the sub-sample's seen words)"""
        out = (C.c_uint32 * 3)()
        self._chk(self.lib.srl_debug_frame_counters(self.h, out), "srl_debug_frame_counters")
        return tuple(int(v) for v in out)

    def frame_timing(self, enable=True):
        """accumulated stage times (us) of the frame pipeline since the last call (which clears them); see srl_debug_frame_timing"""
        out = np.zeros(16)
        self._chk(self.lib.srl_debug_frame_timing(self.h, 1 if enable else 0, _ptr(out)), "srl_debug_frame_timing")
        return dict(zip(self.FRAME_STAGES, (float(v) for v in out)))

    def pass_stamps(self, enable=True, read=True):
        """(gpu[64, 16] device-clock ticks of 10 ns, host[64, 4] steady-clock ns) of the last 64 passes; see srl_debug_pass_stamps"""
        g = np.zeros((64, 32), dtype=np.int64); h = np.zeros((64, 4), dtype=np.int64)
        self._chk(self.lib.srl_debug_pass_stamps(self.h, 1 if enable else 0, _ptr(g) if read else None, _ptr(h) if read else None), "srl_debug_pass_stamps")
        return g, h

    def set_arm_linger(self, host_linger_us=150.0, kernel_linger_us=300.0):
        self._chk(self.lib.srl_debug_set_arm_linger(self.h, float(host_linger_us), float(kernel_linger_us)), "srl_debug_set_arm_linger")

    def device_sqrt(self, x):
        x = _f64(x).ravel()
        out = np.empty_like(x)
        self._chk(self.lib.srl_debug_device_sqrt(self.h, _ptr(x), len(x), _ptr(out)), "srl_debug_device_sqrt")
        return out

    def transform_points(self, raw_xyz, q, t, R_il=None, t_il=None):
        r = _f64(raw_xyz, (-1, 3))
        out = np.empty_like(r)
        R_il = _f64(np.eye(3) if R_il is None else R_il).ravel()
        t_il = _f64(np.zeros(3) if t_il is None else t_il)
        self._chk(self.lib.srl_transform_points(self.h, _ptr(r), len(r), _dptr(_f64(q)), _dptr(_f64(t)), _dptr(R_il), _dptr(t_il), _ptr(out)), "srl_transform_points")
        return out

    # --- frame-resident pipeline
    def frame_upload(self, raw_xyz):
        r = _f64(raw_xyz, (-1, 3))
        self._chk(self.lib.srl_frame_upload(self.h, _ptr(r), len(r)), "srl_frame_upload")

    def frame_undistort(self, raw_xyz, relative_time_ms, imu_states, time_frame_begin, mode, R_il=None, t_il=None, imu_point_in=None,
                        want_outputs=True):
        """imu_states: (S, 17) array = timestamp, un_acc, un_gyr, trans, quat wxyz, vel.  Returns (imu_point, raw_point); (None, None) with
        want_outputs=False (both outputs NULL: the corrected sweep only stays in HBM)"""
        r = _f64(raw_xyz, (-1, 3)); rel = _f64(relative_time_ms)
        st = _f64(imu_states, (-1, 17))
        R_il = _f64(np.eye(3) if R_il is None else R_il).ravel()
        t_il = _f64(np.zeros(3) if t_il is None else t_il)
        pin = None if imu_point_in is None else _f64(imu_point_in, (-1, 3))
        imu = np.empty_like(r) if want_outputs else None
        out = np.empty_like(r) if want_outputs else None
        self._chk(self.lib.srl_frame_undistort(self.h, _ptr(r), _ptr(rel), None if pin is None else _ptr(pin), len(r), _ptr(st), len(st),
                                               float(time_frame_begin), int(mode), _dptr(R_il), _dptr(t_il), _ptr(imu), _ptr(out)),
                  "srl_frame_undistort")
        return imu, out

    def frame_take(self, index):
        idx = np.ascontiguousarray(index, dtype=np.int32)
        self._chk(self.lib.srl_frame_take(self.h, _ptr(idx), len(idx)), "srl_frame_take")

    def frame_subsample(self, order, sample_size):
        """srl_frame_subsample: buildFrame's subSampleFrame on the undistorted sweep, visiting the points in `order` (the first shuffle);
        returns m, the number of voxels kept"""
        o = np.ascontiguousarray(order, dtype=np.int32)
        m = C.c_int()
        self._chk(self.lib.srl_frame_subsample(self.h, _ptr(o), len(o), float(sample_size), C.byref(m)), "srl_frame_subsample")
        self._kept = m.value
        return m.value

    def frame_take_subsampled(self, perm=None, m=None, want_index=True, want_raw=False, want_imu=False):
        """srl_frame_take_subsampled: frame point k = kept[perm[k]] (perm = the second shuffle over 0..m-1; None = container order, m = the
        last sub-sample's count unless given).  Returns dict(index, raw, imu), None for what was not asked for."""
        pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        if m is None:
            m = len(pm) if pm is not None else getattr(self, "_kept", 0)
        m = int(m)
        idx = np.empty(m, dtype=np.int32) if want_index else None
        raw = np.empty((m, 3)) if want_raw else None
        imu = np.empty((m, 3)) if want_imu else None
        self._chk(self.lib.srl_frame_take_subsampled(self.h, _ptr(pm), m, _ptr(idx),
                                                     _ptr(raw), _ptr(imu)),
                  "srl_frame_take_subsampled")
        return dict(index=idx, raw=raw, imu=imu)

    def frame_size(self):
        n = C.c_int()
        self._chk(self.lib.srl_frame_size(self.h, C.byref(n)), "srl_frame_size")
        return n.value

    # --- Livox messages -> device point queue -> sweeps cut at image times
    def livox_decode(self, points, header_stamp, opts, ok=()):
        """srl_livox_decode: points = LIVOX_POINT_DTYPE records of one message.  Returns the report as a dict (with rc)."""
        a = _livox_points(points)
        r = LivoxReport()
        rc = self._chk(self.lib.srl_livox_decode(self.h, _ptr(a), len(a), float(header_stamp), C.byref(opts), C.byref(r)), "srl_livox_decode", ok=ok)
        return dict(_livox_report_dict(r), rc=rc)

    def pc2_decode(self, data, layout, header_stamp, last_end_time, opts, ok=()):
        """srl_pc2_decode: data = the message's bytes (pc2_message), layout = Pc2Layout.  Returns the report as a dict (with rc)."""
        d = np.ascontiguousarray(data, dtype=np.uint8)
        r = Pc2Report()
        rc = self._chk(self.lib.srl_pc2_decode(self.h, _ptr(d), d.nbytes, C.byref(layout), float(header_stamp), float(last_end_time), C.byref(opts),
                                               C.byref(r)), "srl_pc2_decode", ok=ok)
        return dict(_pc2_report_dict(r), rc=rc)

    def points_info(self):
        """srl_points_info -> (size, front_timestamp, back_timestamp); no device synchronisation"""
        n, f, b = C.c_int(), C.c_double(), C.c_double()
        self._chk(self.lib.srl_points_info(self.h, C.byref(n), C.byref(f), C.byref(b)), "srl_points_info")
        return n.value, f.value, b.value

    def points_clear(self):
        self._chk(self.lib.srl_points_clear(self.h), "srl_points_clear")

    def points_cut(self, t):
        """srl_points_cut: while (front().timestamp < t) pop -> (count, new front timestamp); the cut stays resident"""
        r = PointsCutReport()
        self._chk(self.lib.srl_points_cut(self.h, float(t), C.byref(r)), "srl_points_cut")
        return r.count, r.front_timestamp

    def _points_download(self, fn, what):
        n = C.c_int()
        self._chk(fn(self.h, None, None, None, 0, C.byref(n)), what, ok=(SRL_ERR_BAD_ARG,) )
        m = n.value
        raw = np.empty((m, 3)); rel = np.empty(m); ts = np.empty(m)
        self._chk(fn(self.h, _ptr(raw), _ptr(rel), _ptr(ts), m, C.byref(n)), what)
        return dict(raw=raw, relative_time=rel, timestamp=ts)

    def points_queue_download(self):
        """the queue front to back: dict(raw (n, 3), relative_time, timestamp)"""
        return self._points_download(self.lib.srl_points_queue_download, "srl_points_queue_download")

    def points_cut_download(self):
        return self._points_download(self.lib.srl_points_cut_download, "srl_points_cut_download")

    def points_fallbacks(self):
        n = C.c_int64()
        self._chk(self.lib.srl_debug_points_fallbacks(self.h, C.byref(n)), "srl_debug_points_fallbacks")
        return n.value

    def frame_undistort_cut(self, time_begin, time_end, point_time_enable, imu_states, mode, R_il=None, t_il=None):
        """srl_frame_undistort_cut on the resident cut; returns n, the points the time rewrite kept"""
        st = _f64(imu_states, (-1, 17))
        R_il = _f64(np.eye(3) if R_il is None else R_il).ravel()
        t_il = _f64(np.zeros(3) if t_il is None else t_il)
        n = C.c_int()
        self._chk(self.lib.srl_frame_undistort_cut(self.h, float(time_begin), float(time_end), int(bool(point_time_enable)), _ptr(st), len(st), int(mode),
                                                   _dptr(R_il), _dptr(t_il), C.byref(n)), "srl_frame_undistort_cut")
        return n.value

    def undistorted_download(self):
        """srl_debug_undistorted_download: dict(uncorrected, imu, raw (n, 3) each, interval (n,)) of the undistorted sweep in HBM"""
        n = C.c_int()
        self._chk(self.lib.srl_debug_undistorted_download(self.h, None, None, None, None, 0, C.byref(n)), "srl_debug_undistorted_download",
                  ok=(SRL_ERR_BAD_ARG,))
        m = n.value
        unc = np.empty((m, 3)); imu = np.empty((m, 3)); raw = np.empty((m, 3)); seg = np.empty(m, dtype=np.int32)
        self._chk(self.lib.srl_debug_undistorted_download(self.h, _ptr(unc), _ptr(imu), _ptr(raw), _ptr(seg), m, C.byref(n)),
                  "srl_debug_undistorted_download")
        return dict(uncorrected=unc, imu=imu, raw=raw, interval=seg)

    def frame_point_times(self, index):
        """srl_frame_point_times -> (timestamp, relative_time ms, alpha_time) of the points index[] of the sweep undistorted from the cut"""
        idx = np.ascontiguousarray(index, dtype=np.int32)
        ts = np.empty(len(idx)); rel = np.empty(len(idx)); al = np.empty(len(idx))
        self._chk(self.lib.srl_frame_point_times(self.h, _ptr(idx), len(idx), _ptr(ts), _ptr(rel), _ptr(al)), "srl_frame_point_times")
        return ts, rel, al

    def radix_sort_pairs(self, keys, bits):
        """test hook: the frame path's stable (key, position) sort over the low `bits` bits -> (keys_sorted, positions_sorted)"""
        k = np.ascontiguousarray(keys, dtype=np.uint32)
        ks = np.empty_like(k); ps = np.empty_like(k)
        self._chk(self.lib.srl_debug_radix_sort_pairs(self.h, _ptr(k), len(k), int(bits), _ptr(ks), _ptr(ps)), "srl_debug_radix_sort_pairs")
        return ks, ps

    def set_frame_order_mode(self, mode):
        """test hook: 0 = keypoint order on the device where it applies (default), 1 = always the host replay (srl_debug_set_frame_order_mode)"""
        self._chk(self.lib.srl_debug_set_frame_order_mode(self.h, int(mode)), "srl_debug_set_frame_order_mode")

    def frame_order_used(self):
        """1 = the last selection ordered on the device, 2 = host replay, 3 = device order overflowed a bucket and the host replay ran"""
        u = C.c_int()
        self._chk(self.lib.srl_debug_frame_order_used(self.h, C.byref(u)), "srl_debug_frame_order_used")
        return u.value

    def frame_select_keypoints(self, q, t, sample_voxel_size, R_il=None, t_il=None, want_index=True):
        """want_index=False: keypoint_index = NULL (the selection stays on the device as the resident sweep; only the count comes back)"""
        R_il = _f64(np.eye(3) if R_il is None else R_il).ravel()
        t_il = _f64(np.zeros(3) if t_il is None else t_il)
        m = C.c_int()
        if not want_index:
            self._chk(self.lib.srl_frame_select_keypoints(self.h, _dptr(_f64(q)), _dptr(_f64(t)), _dptr(R_il), _dptr(t_il),
                                                          float(sample_voxel_size), None, C.byref(m)), "srl_frame_select_keypoints")
            return m.value
        idx = np.empty(max(self.frame_size(), 1), dtype=np.int32)
        self._chk(self.lib.srl_frame_select_keypoints(self.h, _dptr(_f64(q)), _dptr(_f64(t)), _dptr(R_il), _dptr(t_il),
                                                      float(sample_voxel_size), _ptr(idx), C.byref(m)), "srl_frame_select_keypoints")
        return idx[: m.value].copy()

    def frame_commit(self, q, t, voxel_size=1.0, cap=20, min_dist=0.15, min_num_points=0, R_il=None, t_il=None, want_world=True, want_added=True,
                     world_out=None):
        """want_added=False: num_added = NULL (the insertion is only enqueued, see include/srlivo_hip.h); world_out: a caller-owned
        (n, 3) float64 array to receive the world points (page-locked for the fastest path) instead of a fresh one"""
        R_il = _f64(np.eye(3) if R_il is None else R_il).ravel()
        t_il = _f64(np.zeros(3) if t_il is None else t_il)
        world = None
        if want_world:
            world = world_out if world_out is not None else np.empty((self.frame_size(), 3))
            assert world.dtype == np.float64 and world.flags.c_contiguous and world.shape == (self.frame_size(), 3)
        added = C.c_int()
        self._chk(self.lib.srl_frame_commit(self.h, _dptr(_f64(q)), _dptr(_f64(t)), _dptr(R_il), _dptr(t_il), float(voxel_size), cap,
                                            float(min_dist), min_num_points, _ptr(world) if want_world else None,
                                            C.byref(added) if want_added else None),
                  "srl_frame_commit")
        return world, (added.value if want_added else None)

    def frame_commit_report(self, q, t, voxel_size=1.0, cap=20, min_dist=0.15, min_num_points=0, R_il=None, t_il=None, want_world=False):
        """srl_frame_commit_report: frame_commit with the report of map_insert_report (ref_z = t[2]).  Returns (outcome, cloud, num_added),
        or (outcome, cloud, num_added, world) with want_world."""
        R_il = _f64(np.eye(3) if R_il is None else R_il).ravel()
        t_il = _f64(np.zeros(3) if t_il is None else t_il)
        n = self.frame_size()
        world = np.empty((n, 3)) if want_world else None
        outcome = np.zeros(n, dtype=np.uint8)
        cloud = np.zeros((n, 4), dtype=np.float32)
        m, added = C.c_int(), C.c_int()
        self._chk(self.lib.srl_frame_commit_report(self.h, _dptr(_f64(q)), _dptr(_f64(t)), _dptr(R_il), _dptr(t_il), float(voxel_size), cap,
                                                   float(min_dist), min_num_points, _ptr(world), _ptr(outcome), _ptr(cloud), C.byref(m),
                                                   C.byref(added)), "srl_frame_commit_report")
        out = (outcome, cloud[: m.value].copy(), added.value)
        return out + (world,) if want_world else out

    # --- multi-GPU
    @staticmethod
    def comm_unique_id():
        buf = (C.c_ubyte * SRL_COMM_ID_BYTES)()
        rc = load_library().srl_comm_unique_id(buf)
        if rc:
            raise SrlError(rc, "srl_comm_unique_id")
        return bytes(buf)

    def comm_init_rank(self, nranks, rank, uid):
        buf = (C.c_ubyte * SRL_COMM_ID_BYTES).from_buffer_copy(uid)
        self._chk(self.lib.srl_comm_init_rank(self.h, nranks, rank, buf), "srl_comm_init_rank")

    def comm_suspend(self, suspend=True):
        self._chk(self.lib.srl_comm_suspend(self.h, int(bool(suspend))), "srl_comm_suspend")

    def comm_destroy(self):
        self._chk(self.lib.srl_comm_destroy(self.h), "srl_comm_destroy")

    def set_gather_counts(self, nranks=1, rank=0, counts=None):
        """srl_debug_set_gather_counts (counts=None: off)"""
        if counts is None:
            self._chk(self.lib.srl_debug_set_gather_counts(self.h, 1, 0, None), "set_gather_counts")
            return
        c = (C.c_int64 * int(nranks))(*[int(x) for x in counts])
        self._chk(self.lib.srl_debug_set_gather_counts(self.h, int(nranks), int(rank), c), "set_gather_counts")

    def peer_export(self):
        """srl_peer_export -> (64-byte HIP IPC handle for peers in other processes, device pointer for peers in this process)"""
        h = (C.c_ubyte * SRL_PEER_HANDLE_BYTES)()
        ptr = C.c_void_p()
        self._chk(self.lib.srl_peer_export(self.h, h, C.byref(ptr)), "srl_peer_export")
        return bytes(h), int(ptr.value)

    def peer_attach(self, nranks, rank, handles=None, local_ptrs=None):
        """srl_peer_attach: handles = list of nranks 64-byte handles (or None), local_ptrs = list of nranks device pointers (0 / None
        entries fall back to the handle).  Upload the sweep afterwards."""
        hb = None
        if handles is not None:
            assert len(handles) == nranks and all(len(x) == SRL_PEER_HANDLE_BYTES for x in handles)
            hb = (C.c_ubyte * (SRL_PEER_HANDLE_BYTES * nranks)).from_buffer_copy(b"".join(handles))
        lp = None
        if local_ptrs is not None:
            lp = (C.c_void_p * nranks)(*[C.c_void_p(int(x) if x else None) for x in local_ptrs])
        self._chk(self.lib.srl_peer_attach(self.h, int(nranks), int(rank), hb, lp), "srl_peer_attach")

    def peer_set_deadline_ms(self, ms):
        """how long a pass keeps re-polling for a late rank's row before the session is given up on every rank (srl_peer_set_deadline_ms)"""
        self._chk(self.lib.srl_peer_set_deadline_ms(self.h, int(ms)), "srl_peer_set_deadline_ms")

    def peer_stats(self):
        """(passes repeated because a row had not arrived within one kernel's spin, session failed)"""
        rep, failed = C.c_int64(), C.c_int()
        self._chk(self.lib.srl_peer_stats(self.h, C.byref(rep), C.byref(failed)), "srl_peer_stats")
        return rep.value, bool(failed.value)

    def comm_info(self):
        """srl_comm_info: what the sharded path of this context runs on"""
        tr, nr, rk, seen, armed = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        self._chk(self.lib.srl_comm_info(self.h, C.byref(tr), C.byref(nr), C.byref(rk), C.byref(seen), C.byref(armed)), "srl_comm_info")
        return dict(transport_used=("none", "rccl", "peer", "host-callbacks")[tr.value], nranks=nr.value, rank=rk.value, ranks_seen=seen.value,
                    passes_armed=armed.value)

    def peer_detach(self):
        self._chk(self.lib.srl_peer_detach(self.h), "srl_peer_detach")

    def comm_set_host_callbacks(self, nranks, rank, allreduce, allgather):
        """allreduce(np.ndarray float64) -> in place sum; allgather(int) -> list of ints."""
        def _ar(buf, count, _user):
            a = np.ctypeslib.as_array(buf, shape=(count,))
            allreduce(a)
            return 0

        def _ag(mine, allp, _user):
            vals = allgather(int(mine[0]))
            for i, v in enumerate(vals):
                allp[i] = int(v)
            return 0
        self._cb = (ALLREDUCE_FN(_ar), ALLGATHER_FN(_ag))
        self._chk(self.lib.srl_comm_set_host_callbacks(self.h, nranks, rank, self._cb[0], self._cb[1], None), "srl_comm_set_host_callbacks")


class Flow:
    """The optical-flow tracker of a context (srl_flow_*): LKOpticalFlowKernel::trackImage on the device.  One per context."""

    def __init__(self, ctx, opts=None, **kw):
        self.ctx = ctx
        self.lib = ctx.lib
        o = opts if opts is not None else default_flow_opts(**kw)
        ctx._chk(self.lib.srl_flow_create(ctx.h, C.byref(o)), "srl_flow_create")
        self.open = True

    def close(self):
        if self.open and self.ctx.h:
            self.lib.srl_flow_destroy(self.ctx.h)
        self.open = False

    def track_image(self, gray, prev_xy):
        """srl_flow_track_image: gray (rows, cols) uint8 (rows may be strided), prev_xy (n, 2) float32.  Returns (next_xy (n, 2) float32,
        status (n,) uint8, n_tracked); on the tracker's first image next_xy = prev_xy, status is zeros and n_tracked 0."""
        g = np.asarray(gray)
        if g.dtype != np.uint8 or g.ndim != 2 or g.strides[1] != 1 or g.strides[0] < g.shape[1]:
            g = np.ascontiguousarray(g, dtype=np.uint8)
        pts = np.ascontiguousarray(prev_xy, dtype=np.float32).reshape(-1, 2)
        n = len(pts)
        nxt = np.zeros((n, 2), dtype=np.float32)
        status = np.zeros(n, dtype=np.uint8)
        nt = C.c_int()
        self.ctx._chk(self.lib.srl_flow_track_image(self.ctx.h, _ptr(g), g.shape[0], g.shape[1], g.strides[0], _ptr(pts) if n else None, n,
                                                    _ptr(nxt) if n else None, _ptr(status) if n else None, C.byref(nt)), "srl_flow_track_image")
        return nxt, status, nt.value

    def track_prepared(self, prev_xy):
        """srl_flow_track_prepared: track_image on the gray image the context's preparer holds"""
        pts = np.ascontiguousarray(prev_xy, dtype=np.float32).reshape(-1, 2)
        n = len(pts)
        nxt = np.zeros((n, 2), dtype=np.float32)
        status = np.zeros(n, dtype=np.uint8)
        nt = C.c_int()
        self.ctx._chk(self.lib.srl_flow_track_prepared(self.ctx.h, _ptr(pts) if n else None, n, _ptr(nxt) if n else None, _ptr(status) if n else None,
                                                       C.byref(nt)), "srl_flow_track_prepared")
        return nxt, status, nt.value

    def levels(self):
        L = C.c_int()
        self.ctx._chk(self.lib.srl_flow_levels(self.ctx.h, C.byref(L)), "srl_flow_levels")
        return L.value

    def download_level(self, which, level):
        """srl_flow_download_level: (padded image (rows + 42, cols + 42) uint8, padded derivative (rows + 42, cols + 42, 2) int16)"""
        r, c = C.c_int(), C.c_int()
        self.ctx._chk(self.lib.srl_flow_download_level(self.ctx.h, which, level, None, None, C.byref(r), C.byref(c)), "srl_flow_download_level")
        img = np.zeros((r.value + 2 * FLOW_BORDER, c.value + 2 * FLOW_BORDER), dtype=np.uint8)
        der = np.zeros((r.value + 2 * FLOW_BORDER, c.value + 2 * FLOW_BORDER, 2), dtype=np.int16)
        self.ctx._chk(self.lib.srl_flow_download_level(self.ctx.h, which, level, _ptr(img), _ptr(der), C.byref(r), C.byref(c)), "srl_flow_download_level")
        return img, der


class ImagePrep:
    """The image preparer of a context (srl_image_prep_*): undistortion, gray, CLAHE and YCrCb equalisation on the device.  One per context."""

    def __init__(self, ctx, opts=None, **kw):
        self.ctx = ctx
        self.lib = ctx.lib
        self.opts = opts if opts is not None else default_image_prep_opts(**kw)
        self.open = False
        ctx._chk(self.lib.srl_image_prep_create(ctx.h, C.byref(self.opts)), "srl_image_prep_create")
        self.open = True

    def close(self):
        if self.open and self.ctx.h:
            self.lib.srl_image_prep_destroy(self.ctx.h)
        self.open = False

    def prepare(self, raw_bgr):
        """srl_image_prepare: raw_bgr (rows, cols, 3) uint8 (rows may be strided).  Returns ImagePrepInfo."""
        b = np.asarray(raw_bgr)
        if b.dtype != np.uint8 or b.ndim != 3 or b.shape[2] != 3 or b.strides[2] != 1 or b.strides[1] != 3 or b.strides[0] < 3 * b.shape[1]:
            b = np.ascontiguousarray(b, dtype=np.uint8)
        info = ImagePrepInfo()
        self.ctx._chk(self.lib.srl_image_prepare(self.ctx.h, _ptr(b), b.shape[0], b.shape[1], b.strides[0], C.byref(info)), "srl_image_prepare")
        return info

    def prepare_resized(self, raw_bgr):
        """srl_image_prepare_resized: raw_bgr (src_rows, src_cols, 3) uint8 of any size (rows may be strided), resized on the device to the
        preparer's size before the chain.  Returns ImagePrepInfo."""
        b = np.asarray(raw_bgr)
        if b.dtype != np.uint8 or b.ndim != 3 or b.shape[2] != 3 or b.strides[2] != 1 or b.strides[1] != 3 or b.strides[0] < 3 * b.shape[1]:
            b = np.ascontiguousarray(b, dtype=np.uint8)
        info = ImagePrepInfo()
        self.ctx._chk(self.lib.srl_image_prepare_resized(self.ctx.h, _ptr(b), b.shape[0], b.shape[1], b.strides[0], C.byref(info)),
                      "srl_image_prepare_resized")
        return info

    def prepare_jpeg(self, jpeg):
        """srl_image_prepare_jpeg: a baseline JPEG stream (bytes or uint8 array) decoded on the device and prepared where it lies, resized
        when its size is not the preparer's.  Returns ImagePrepInfo."""
        d = _jpeg_bytes(jpeg)
        info = ImagePrepInfo()
        self.ctx._chk(self.lib.srl_image_prepare_jpeg(self.ctx.h, _ptr(d), d.size, C.byref(info)), "srl_image_prepare_jpeg")
        return info

    def download_resized(self):
        """srl_image_prep_download_resized: the frame the last image's remap read, (rows, cols, 3) uint8"""
        out = np.zeros((self.opts.rows, self.opts.cols, 3), dtype=np.uint8)
        self.ctx._chk(self.lib.srl_image_prep_download_resized(self.ctx.h, _ptr(out), out.size), "srl_image_prep_download_resized")
        return out

    def download(self, which):
        """srl_image_prep_download: SRL_PREP_GRAY_EQ -> (rows, cols) uint8, SRL_PREP_BGR_EQ -> (rows, cols, 3) uint8"""
        shape = (self.opts.rows, self.opts.cols, 3) if which == SRL_PREP_BGR_EQ else (self.opts.rows, self.opts.cols)
        out = np.zeros(shape, dtype=np.uint8)
        self.ctx._chk(self.lib.srl_image_prep_download(self.ctx.h, int(which), _ptr(out), out.strides[0]), "srl_image_prep_download")
        return out

    def download_stage(self, stage, tiles):
        """srl_image_prep_download_stage: the stage's bytes as one flat uint8 array (tiles: ImagePrepInfo.tiles, for the LUT stages)"""
        npix = self.opts.rows * self.opts.cols
        size = {SRL_PREP_STAGE_UNDIST: 3 * npix, SRL_PREP_STAGE_GRAY: npix, SRL_PREP_STAGE_YCRCB: 3 * npix}.get(stage, int(tiles) * int(tiles) * 256)
        out = np.zeros(size, dtype=np.uint8)
        self.ctx._chk(self.lib.srl_image_prep_download_stage(self.ctx.h, int(stage), _ptr(out), out.size), "srl_image_prep_download_stage")
        return out


class Oft:
    """The host mirror's opticalFlowTracker (srl_oft_*): the bookkeeping of the camera tracker's point set by pool position.  ctx may be
    None for a handle whose flow and update go through providers.  Providers are Python callables on numpy views of the C arrays:
      flow(gray_address, rows, cols, stride, prev_xy (n, 2) float32, next_xy (n, 2) float32, status (n,) uint8) -> status code
      fundamental(last_xy, cur_xy, status) -> status code          pnp(xyz (n, 3), uv (n, 2)) -> (status code, inlier indices)
      update(camera, rows, cols, tracked, candidates, opts, out, totals) -> status code (fills out and totals)"""

    def __init__(self, ctx=None):
        self.lib = load_library()
        self.ctx = ctx
        self.h = C.c_void_p()
        self._keep = {}
        rc = self.lib.srl_oft_create(ctx.h if ctx is not None else None, C.byref(self.h))
        if rc != SRL_OK:
            raise SrlError(rc, "srl_oft_create", "")

    def close(self):
        if self.h:
            self.lib.srl_oft_destroy(self.h)
        self.h = C.c_void_p()

    def _chk(self, rc, what):
        if rc != SRL_OK:
            raise SrlError(rc, what, (self.lib.srl_last_error(self.ctx.h) or b"").decode() if self.ctx is not None else "")

    @staticmethod
    def _view(address, count, dtype):
        dtype = np.dtype(dtype)
        if not count or not address:
            return np.zeros(0, dtype)
        return np.frombuffer((C.c_char * (count * dtype.itemsize)).from_address(address), dtype=dtype)

    def set_maximum_tracked_points(self, m):
        self._chk(self.lib.srl_oft_set_maximum_tracked_points(self.h, int(m)), "srl_oft_set_maximum_tracked_points")

    def set_flow_provider(self, fn):
        cb = None if fn is None else OFT_FLOW_PROVIDER_FN(
            lambda gray, rows, cols, stride, prev, n, nxt, status, user: int(fn(gray, rows, cols, stride, self._view(prev, 2 * n, "<f4").reshape(-1, 2),
                                                                                self._view(nxt, 2 * n, "<f4").reshape(-1, 2), self._view(status, n, np.uint8))))
        self._keep["flow"] = cb
        self._chk(self.lib.srl_oft_set_flow_provider(self.h, cb, None), "srl_oft_set_flow_provider")

    def set_fundamental_provider(self, fn):
        cb = None if fn is None else OFT_FUNDAMENTAL_PROVIDER_FN(
            lambda last, cur, n, status, user: int(fn(self._view(last, 2 * n, "<f4").reshape(-1, 2), self._view(cur, 2 * n, "<f4").reshape(-1, 2),
                                                      self._view(status, n, np.uint8))))
        self._keep["fundamental"] = cb
        self._chk(self.lib.srl_oft_set_fundamental_provider(self.h, cb, None), "srl_oft_set_fundamental_provider")

    def set_pnp_provider(self, fn):
        def shim(xyz, uv, n, inliers, n_inliers, user):
            rc, idx = fn(self._view(xyz, 3 * n, "<f4").reshape(-1, 3), self._view(uv, 2 * n, "<f4").reshape(-1, 2))
            idx = np.asarray(idx, dtype=np.int32).reshape(-1)[:n]
            self._view(inliers, n, "<i4")[:len(idx)] = idx
            n_inliers[0] = len(idx)
            return int(rc)
        cb = None if fn is None else OFT_PNP_PROVIDER_FN(shim)
        self._keep["pnp"] = cb
        self._chk(self.lib.srl_oft_set_pnp_provider(self.h, cb, None), "srl_oft_set_pnp_provider")

    def set_update_provider(self, fn):
        cb = None if fn is None else OFT_UPDATE_PROVIDER_FN(
            lambda cam, rows, cols, tracked, n, cand, nc, opts, out, cap, tot, user: int(fn(
                cam.contents, rows, cols, self._view(tracked, n, COLOR_TRACK_POINT_DTYPE), self._view(cand, nc, "<i4"), opts.contents,
                self._view(out, cap, COLOR_TRACK_POINT_DTYPE), tot.contents)))
        self._keep["update"] = cb
        self._chk(self.lib.srl_oft_set_update_provider(self.h, cb, None), "srl_oft_set_update_provider")

    def use_device_consensus(self, fx_fy_cx_cy, fundamental_opts=None, pnp_opts=None):
        """srl_oft_use_device_consensus: the context's own consensus estimators as the fundamental and the PnP provider (NOT OpenCV's
        results: see srlivo_hip.h).  Raises SrlError(SRL_ERR_NO_DEVICE) on a handle made without a context."""
        K = _f64(fx_fy_cx_cy, (4,))
        self._chk(self.lib.srl_oft_use_device_consensus(self.h, _dptr(K), C.byref(fundamental_opts) if fundamental_opts is not None else None,
                                                        C.byref(pnp_opts) if pnp_opts is not None else None), "srl_oft_use_device_consensus")
        # a refused call installs nothing, so the handle may still call through earlier Python providers: let go of them only now
        self._keep.pop("fundamental", None)
        self._keep.pop("pnp", None)

    def use_prepared_image(self, on=True):
        """srl_oft_use_prepared_image: init / track_image ignore their gray and track on the context's prepared image"""
        self._chk(self.lib.srl_oft_use_prepared_image(self.h, int(bool(on))), "srl_oft_use_prepared_image")

    def last_consensus(self, which):
        """srl_oft_last_consensus: the ConsensusResult of the handle's last device call, which = 0 fundamental, 1 PnP"""
        res = ConsensusResult()
        self._chk(self.lib.srl_oft_last_consensus(self.h, int(which), C.byref(res)), "srl_oft_last_consensus")
        return res

    @staticmethod
    def _gray(gray):
        if gray is None:
            return None, 0, 0, 0
        g = np.asarray(gray)
        if g.dtype != np.uint8 or g.ndim != 2 or g.strides[1] != 1 or g.strides[0] < g.shape[1]:
            g = np.ascontiguousarray(g, dtype=np.uint8)
        return g, g.shape[0], g.shape[1], g.strides[0]

    def set_track_points(self, records):
        r = np.ascontiguousarray(records, dtype=COLOR_SELECTED_DTYPE)
        self._chk(self.lib.srl_oft_set_track_points(self.h, _ptr(r) if len(r) else None, len(r)), "srl_oft_set_track_points")

    def init(self, records, gray, time_sweep_end):
        r = np.ascontiguousarray(records, dtype=COLOR_SELECTED_DTYPE)
        g, rows, cols, stride = self._gray(gray)
        self._chk(self.lib.srl_oft_init(self.h, _ptr(r) if len(r) else None, len(r), _ptr(g), rows, cols, stride, float(time_sweep_end)), "srl_oft_init")

    def track_image(self, gray, time_sweep_end, image_rows, image_cols):
        """trackImage; returns map_rgb_points_in_cur_image_pose.size()"""
        g, rows, cols, stride = self._gray(gray)
        n = C.c_int()
        self._chk(self.lib.srl_oft_track_image(self.h, _ptr(g), rows, cols, stride, float(time_sweep_end), int(image_rows), int(image_cols), C.byref(n)),
                  "srl_oft_track_image")
        return n.value

    def remove_outlier_using_ransac_pnp(self, if_remove_outlier=1):
        a = C.c_int()
        self._chk(self.lib.srl_oft_remove_outlier_using_ransac_pnp(self.h, int(if_remove_outlier), C.byref(a)), "srl_oft_remove_outlier_using_ransac_pnp")
        return bool(a.value)

    def update_and_append_track_points(self, camera, image_rows, image_cols, candidates, mini_distance=10.0):
        """candidates: COLOR_SELECTED_DTYPE records (points_rgb_vec_for_projection).  Returns ColorTrackTotals."""
        c = np.ascontiguousarray(candidates, dtype=COLOR_SELECTED_DTYPE)
        tot = ColorTrackTotals()
        self._chk(self.lib.srl_oft_update_and_append_track_points(self.h, C.byref(camera), int(image_rows), int(image_cols), _ptr(c) if len(c) else None, len(c),
                                                                  float(mini_distance), C.byref(tot)), "srl_oft_update_and_append_track_points")
        return tot

    def sizes(self):
        """(map_rgb_points_in_last_image_pose, map_rgb_points_in_cur_image_pose, last_tracked_points, flagged positions)"""
        v = [C.c_int() for _ in range(4)]
        self._chk(self.lib.srl_oft_sizes(self.h, *[C.byref(x) for x in v]), "srl_oft_sizes")
        return tuple(x.value for x in v)

    def times(self):
        a, b = C.c_double(), C.c_double()
        self._chk(self.lib.srl_oft_times(self.h, C.byref(a), C.byref(b)), "srl_oft_times")
        return a.value, b.value

    def pose_map(self, which=0):
        n = C.c_int()
        self._chk(self.lib.srl_oft_pose_map(self.h, which, None, 0, C.byref(n)), "srl_oft_pose_map")
        out = np.zeros(n.value, dtype=COLOR_TRACK_POINT_DTYPE)
        if n.value:
            self._chk(self.lib.srl_oft_pose_map(self.h, which, _ptr(out), len(out), C.byref(n)), "srl_oft_pose_map")
        return out

    def tracked_for_vio(self):
        n = C.c_int()
        self._chk(self.lib.srl_oft_tracked_for_vio(self.h, None, 0, C.byref(n)), "srl_oft_tracked_for_vio")
        out = np.zeros(n.value, dtype=COLOR_VIO_POINT_DTYPE)
        if n.value:
            self._chk(self.lib.srl_oft_tracked_for_vio(self.h, _ptr(out), len(out), C.byref(n)), "srl_oft_tracked_for_vio")
        return out


class Lio:
    """C++ host mirror (lioOptimization + eskfEstimator) through the srl_lio handles."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.srl_lio_create(device, C.byref(h))
        if rc:
            raise SrlError(rc, "srl_lio_create", self.lib.srl_status_str(rc).decode())
        self.h = h
        self._provider = None
        ctxp = self.lib.srl_lio_ctx(self.h)
        self.ctx = Context(handle=C.c_void_p(ctxp)) if ctxp else None

    def close(self):
        if self.h:
            self.lib.srl_lio_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what, ok=()):
        if rc and rc not in ok:
            raise SrlError(rc, what, (self.lib.srl_lio_last_error(self.h) or b"").decode())
        return rc

    def set_extrinsics(self, R_il, t_il):
        self._chk(self.lib.srl_lio_set_extrinsics(self.h, _dptr(_f64(R_il).ravel()), _dptr(_f64(t_il))), "set_extrinsics")

    def last_solve_launches(self):
        n = C.c_int()
        self._chk(self.lib.srl_lio_last_solve_launches(self.h, C.byref(n)), "last_solve_launches")
        return n.value

    def set_laser_point_cov(self, c):
        self._chk(self.lib.srl_lio_set_laser_point_cov(self.h, float(c)), "set_laser_point_cov")

    def eskf_get_state(self):
        s = np.empty(19)
        self._chk(self.lib.srl_lio_eskf_get_state(self.h, _dptr(s)), "eskf_get_state")
        return s

    def eskf_set_state(self, s):
        self._chk(self.lib.srl_lio_eskf_set_state(self.h, _dptr(_f64(s))), "eskf_set_state")

    def eskf_get_cov(self):
        P = np.empty(289)
        self._chk(self.lib.srl_lio_eskf_get_cov(self.h, _dptr(P)), "eskf_get_cov")
        return P.reshape(17, 17)

    def eskf_set_cov(self, P):
        self._chk(self.lib.srl_lio_eskf_set_cov(self.h, _dptr(_f64(P).ravel())), "eskf_set_cov")

    def eskf_set_noise(self, acc, gyr, bacc, bgyr):
        self._chk(self.lib.srl_lio_eskf_set_noise(self.h, acc, gyr, bacc, bgyr), "eskf_set_noise")

    def eskf_init_imu(self, acc0, gyr0):
        self._chk(self.lib.srl_lio_eskf_init_imu(self.h, _dptr(_f64(acc0)), _dptr(_f64(gyr0))), "eskf_init_imu")

    def eskf_try_init(self, t, gyr, acc):
        t = _f64(t); g = _f64(gyr, (-1, 3)); a = _f64(acc, (-1, 3))
        r = C.c_int()
        self._chk(self.lib.srl_lio_eskf_try_init(self.h, _dptr(t), _dptr(g), _dptr(a), len(t), C.byref(r)), "eskf_try_init")
        return r.value

    def eskf_init_stats(self):
        o = np.zeros(14)
        self._chk(self.lib.srl_lio_eskf_get_init_stats(self.h, _dptr(o)), "eskf_get_init_stats")
        return dict(mean_gyr=o[0:3].copy(), mean_acc=o[3:6].copy(), gyr_cov=o[6:9].copy(), acc_cov=o[9:12].copy(),
                    num_init_meas=int(o[12]), initial_flag=bool(o[13]))

    def set_g_norm(self, g_norm=9.81):
        """srl_lio_set_g_norm: the process-global G_norm (9.81 at start; a replay's first processed frame rewrites it)"""
        self._chk(self.lib.srl_lio_set_g_norm(self.h, float(g_norm)), "srl_lio_set_g_norm")

    def set_initial_flag(self, flag):
        self._chk(self.lib.srl_lio_set_initial_flag(self.h, int(bool(flag))), "set_initial_flag")

    def state_initialization(self, index_frame, initialization, prev2, prev1):
        out = np.zeros(7)
        self._chk(self.lib.srl_lio_state_initialization(self.h, int(index_frame), int(initialization), _dptr(_f64(prev2)),
                                                        _dptr(_f64(prev1)), _dptr(out)), "state_initialization")
        return out[0:4].copy(), out[4:7].copy()

    def eskf_scale_init_cov(self):
        self._chk(self.lib.srl_lio_eskf_scale_init_cov(self.h), "eskf_scale_init_cov")

    def eskf_predict(self, dt, acc1, gyr1):
        self._chk(self.lib.srl_lio_eskf_predict(self.h, float(dt), _dptr(_f64(acc1)), _dptr(_f64(gyr1))), "eskf_predict")

    def eskf_observe(self, dx):
        self._chk(self.lib.srl_lio_eskf_observe(self.h, _dptr(_f64(dx))), "eskf_observe")

    def add_points_to_map(self, world_xyz, voxel_size=1.0, cap=20, min_dist=0.15, min_num_points=0):
        w = _f64(world_xyz, (-1, 3))
        self._chk(self.lib.srl_lio_add_points_to_map(self.h, _ptr(w), len(w), voxel_size, cap, min_dist, min_num_points), "add_points_to_map")

    def map_size(self):
        n = C.c_int64()
        self._chk(self.lib.srl_lio_map_size(self.h, C.byref(n)), "map_size")
        return n.value

    def remove_points_far_from_location(self, location, distance):
        """lioOptimization::removePointsFarFromLocation on the device map (srl_map_remove_far)"""
        loc = _f64(location).ravel()
        self._chk(self.lib.srl_lio_remove_points_far_from_location(self.h, _dptr(loc), float(distance)), "remove_points_far_from_location")

    def set_collect_points_world(self, on):
        """collect lioOptimization::points_world (cloud_world) at every insertion of this object; off by default (the collecting
        insertions are synchronous, see srl_lio_set_collect_points_world)"""
        self._chk(self.lib.srl_lio_set_collect_points_world(self.h, 1 if on else 0), "srl_lio_set_collect_points_world")

    def points_world(self):
        """the cloud the last insertion left: (m, 4) float32 rows x, y, z, intensity (empty while the switch is off)"""
        m = C.c_int()
        self._chk(self.lib.srl_lio_points_world(self.h, None, 0, C.byref(m)), "srl_lio_points_world")
        cloud = np.zeros((m.value, 4), dtype=np.float32)
        if m.value:
            self._chk(self.lib.srl_lio_points_world(self.h, _ptr(cloud), m.value, C.byref(m)), "srl_lio_points_world")
        return cloud

    def set_color_map_options(self, opts=None):
        """opt in to the colour half of addPointsToMap (srl_lio_set_color_map_options); opts = ColorOpts, None = the yaml values"""
        self._chk(self.lib.srl_lio_set_color_map_options(self.h, None if opts is None else C.byref(opts)), "srl_lio_set_color_map_options")

    def set_color_times(self, time_last_process=-1e5, commit_time_sweep_end=0.0, to_rendering=False):
        self._chk(self.lib.srl_lio_set_color_times(self.h, float(time_last_process), float(commit_time_sweep_end), 1 if to_rendering else 0),
                  "srl_lio_set_color_times")

    def add_points_to_map_at(self, world_xyz, time_sweep_end, to_rendering=False, voxel_size=1.0, cap=20, min_dist=0.15, min_num_points=0):
        w = _f64(world_xyz, (-1, 3))
        self._chk(self.lib.srl_lio_add_points_to_map_at(self.h, _ptr(w), len(w), voxel_size, cap, min_dist, min_num_points, float(time_sweep_end),
                                                        1 if to_rendering else 0), "srl_lio_add_points_to_map_at")

    def color_visited(self, which=0):
        """(list (m, 3) int32, number_of_new_visited_voxel); which 0 = voxels_recent_visited_temp, 1 = voxels_recent_visited"""
        m, new = C.c_int(), C.c_int()
        self._chk(self.lib.srl_lio_color_visited(self.h, int(which), None, 0, C.byref(m), C.byref(new)), "srl_lio_color_visited")
        out = np.zeros((m.value, 3), dtype=np.int32)
        if m.value:
            self._chk(self.lib.srl_lio_color_visited(self.h, int(which), _ptr(out), m.value, C.byref(m), C.byref(new)), "srl_lio_color_visited")
        return out, new.value

    def color_stored(self):
        """the stored records of the last insertion (COLOR_STORED_DTYPE)"""
        m = C.c_int()
        self._chk(self.lib.srl_lio_color_stored(self.h, None, 0, C.byref(m)), "srl_lio_color_stored")
        out = np.zeros(m.value, dtype=COLOR_STORED_DTYPE)
        if m.value:
            self._chk(self.lib.srl_lio_color_stored(self.h, _ptr(out), m.value, C.byref(m)), "srl_lio_color_stored")
        return out

    # ---- the camera ESIKF (csrc/host/imageProcessing.cpp)
    def vio_set_options(self, num_iterations=2, estimate_intrinsic=True, estimate_extrinsic=True, camera_intrinsic=None, R_imu_camera=None,
                        t_imu_camera=None):
        arr = [None if a is None else _f64(a).reshape(-1) for a in (camera_intrinsic, R_imu_camera, t_imu_camera)]
        self._chk(self.lib.srl_lio_vio_set_options(self.h, int(num_iterations), int(bool(estimate_intrinsic)), int(bool(estimate_extrinsic)),
                                                   *[_ptr(a) for a in arr]), "srl_lio_vio_set_options")

    def vio_set_camera_state(self, state31):
        s = _f64(state31, (CAMERA_STATE_DOUBLES,))
        self._chk(self.lib.srl_lio_vio_set_camera_state(self.h, _ptr(s)), "srl_lio_vio_set_camera_state")

    def vio_get_camera_state(self):
        s = np.zeros(CAMERA_STATE_DOUBLES)
        self._chk(self.lib.srl_lio_vio_get_camera_state(self.h, _ptr(s)), "srl_lio_vio_get_camera_state")
        return s

    def vio_set_initial_cov(self):
        self._chk(self.lib.srl_lio_vio_set_initial_cov(self.h), "srl_lio_vio_set_initial_cov")

    def vio_set_cov(self, cov):
        c = _f64(cov, (11, 11))
        self._chk(self.lib.srl_lio_vio_set_cov(self.h, _ptr(c)), "srl_lio_vio_set_cov")

    def vio_get_cov(self):
        c = np.zeros((11, 11))
        self._chk(self.lib.srl_lio_vio_get_cov(self.h, _ptr(c)), "srl_lio_vio_get_cov")
        return c

    def vio_set_rows_provider(self, fn):
        """fn(args: ColorVioArgs, points: COLOR_VIO_POINT_DTYPE array, sums: ColorVioSums) -> status replaces the device's measurement
        pass; None puts it back"""
        if fn is None:
            self._vio_provider = None
            self._chk(self.lib.srl_lio_vio_set_rows_provider(self.h, VIO_ROWS_PROVIDER_FN(), None), "srl_lio_vio_set_rows_provider")
            return

        def thunk(args, points, n, sums, user):
            pts = np.frombuffer((C.c_char * (n * COLOR_VIO_POINT_DTYPE.itemsize)).from_address(points), dtype=COLOR_VIO_POINT_DTYPE) if n else \
                np.zeros(0, COLOR_VIO_POINT_DTYPE)
            return int(fn(args.contents, pts, sums.contents))
        self._vio_provider = VIO_ROWS_PROVIDER_FN(thunk)
        self._chk(self.lib.srl_lio_vio_set_rows_provider(self.h, self._vio_provider, None), "srl_lio_vio_set_rows_provider")

    def _vio_update(self, fn, name, tracked, number_of_new_visited_voxel, capacity):
        pts = np.ascontiguousarray(tracked, dtype=COLOR_VIO_POINT_DTYPE)
        ok, it, used = C.c_int(), C.c_int(), C.c_int()
        states = np.zeros((capacity, CAMERA_STATE_DOUBLES))
        self._chk(fn(self.h, _ptr(pts) if len(pts) else None, len(pts), int(number_of_new_visited_voxel), C.byref(ok), C.byref(it), C.byref(used),
                     _ptr(states), capacity), name)
        return bool(ok.value), states[:min(it.value, capacity)], used.value

    def vio_esikf(self, tracked, number_of_new_visited_voxel, capacity=16):
        """imageProcessing::vioEsikf on the handle's camera state.  Returns (accepted, the camera state behind every iteration, used)."""
        return self._vio_update(self.lib.srl_lio_vio_esikf, "srl_lio_vio_esikf", tracked, number_of_new_visited_voxel, capacity)

    def vio_photometric(self, tracked, number_of_new_visited_voxel, capacity=16):
        return self._vio_update(self.lib.srl_lio_vio_photometric, "srl_lio_vio_photometric", tracked, number_of_new_visited_voxel, capacity)

    def image_set_options(self, **kw):
        """srl_lio_image_set_options: image_width, image_height, image_resize_ratio, dist (five), track_windows_size,
        maximum_tracked_points, tracker_minimum_depth, tracker_maximum_depth over the reference's defaults"""
        o = ImageProcessOpts()
        self.lib.srl_image_process_opts_default(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, (C.c_double * 5)(*v) if k == "dist" else v)
        self._chk(self.lib.srl_lio_image_set_options(self.h, C.byref(o)), "srl_lio_image_set_options")
        return o

    def image_set_steps(self, steps=None):
        """srl_lio_image_set_steps: an ImageProcessSteps whose members are ctypes callbacks (kept alive here), or None for the device calls"""
        self._image_steps = steps
        self._chk(self.lib.srl_lio_image_set_steps(self.h, C.byref(steps) if steps is not None else None), "srl_lio_image_set_steps")

    def image_process(self, raw_bgr, time_sweep_end, frame_id, ok=()):
        """srl_lio_image_process: imageProcessing::process on the handle's camera state, raw_bgr (rows, cols, 3) uint8 (rows may be
        strided).  Returns ImageProcessResult; with a status listed in `ok`, (status, ImageProcessResult)."""
        b = np.asarray(raw_bgr)
        if b.dtype != np.uint8 or b.ndim != 3 or b.shape[2] != 3 or b.strides[2] != 1 or b.strides[1] != 3 or b.strides[0] < 3 * b.shape[1]:
            b = np.ascontiguousarray(b, dtype=np.uint8)
        res = ImageProcessResult()
        rc = self._chk(self.lib.srl_lio_image_process(self.h, _ptr(b), b.shape[0], b.shape[1], b.strides[0], float(time_sweep_end), int(frame_id),
                                                      C.byref(res)), "srl_lio_image_process", ok)
        return (rc, res) if ok else res

    def image_set_jpeg_step(self, fn=None):
        """srl_lio_image_set_jpeg_step: fn(bytes_address, n, user) -> status as an IMAGE_JPEG_STEP_FN or a Python callable (kept alive here);
        None puts srl_image_prepare_jpeg back"""
        if fn is not None and not isinstance(fn, IMAGE_JPEG_STEP_FN):
            fn = IMAGE_JPEG_STEP_FN(fn)
        self._jpeg_step = fn
        self._chk(self.lib.srl_lio_image_set_jpeg_step(self.h, fn if fn is not None else IMAGE_JPEG_STEP_FN(), None), "srl_lio_image_set_jpeg_step")

    def image_process_jpeg(self, jpeg, time_sweep_end, frame_id, ok=()):
        """srl_lio_image_process_jpeg: image_process on a baseline JPEG stream (bytes or uint8 array).  Returns as image_process does."""
        d = _jpeg_bytes(jpeg)
        res = ImageProcessResult()
        rc = self._chk(self.lib.srl_lio_image_process_jpeg(self.h, _ptr(d), d.size, float(time_sweep_end), int(frame_id), C.byref(res)),
                       "srl_lio_image_process_jpeg", ok)
        return (rc, res) if ok else res

    def image_oft(self):
        """srl_lio_image_oft: the handle's tracker as an Oft that does not own it (read-backs: sizes, times, pose_map, tracked_for_vio)"""
        o = Oft.__new__(Oft)
        o.lib, o.ctx, o._keep = self.lib, self.ctx, {}
        o.h = C.c_void_p(self.lib.srl_lio_image_oft(self.h))
        o.close = lambda: None
        return o

    def image_candidates(self):
        """srl_lio_image_candidates: points_rgb_vec_for_projection as the last refresh left it (COLOR_SELECTED_DTYPE)"""
        n = C.c_int()
        self._chk(self.lib.srl_lio_image_candidates(self.h, None, 0, C.byref(n)), "srl_lio_image_candidates")
        out = np.zeros(n.value, dtype=COLOR_SELECTED_DTYPE)
        if n.value:
            self._chk(self.lib.srl_lio_image_candidates(self.h, _ptr(out), len(out), C.byref(n)), "srl_lio_image_candidates")
        return out

    def image_time_last_process(self):
        t = C.c_double()
        self._chk(self.lib.srl_lio_image_time_last_process(self.h, C.byref(t)), "srl_lio_image_time_last_process")
        return t.value

    def render_points_in_recent_voxel(self, camera, obs_time):
        """rgbMapTracker::renderPointsInRecentVoxel on voxels_recent_visited (srl_lio_render_points_in_recent_voxel); camera = ColorCamera.
        Returns ColorRenderTotals."""
        tot = ColorRenderTotals()
        self._chk(self.lib.srl_lio_render_points_in_recent_voxel(self.h, C.byref(camera), float(obs_time), C.byref(tot)),
                  "srl_lio_render_points_in_recent_voxel")
        return tot

    def select_points_for_projection(self, camera, rows, cols, minimum_dis=10.0, skip_step=1, use_all_points=False, refresh=False):
        """rgbMapTracker::selectPointsForProjection on voxels_recent_visited (srl_lio_select_points_for_projection); refresh=True is
        refreshPointsForProjection.  Returns (records (COLOR_SELECTED_DTYPE), ColorSelectTotals)."""
        m, tot = C.c_int(), ColorSelectTotals()
        args = (C.byref(camera), int(rows), int(cols), float(minimum_dis), int(skip_step), 1 if use_all_points else 0, 1 if refresh else 0)
        # one call into a buffer sized by what earlier calls selected; only a call that selects more than that is asked again
        out = np.zeros(max(getattr(self, "_select_capacity", 0), 4096), dtype=COLOR_SELECTED_DTYPE)
        rc = self.lib.srl_lio_select_points_for_projection(self.h, *args, _ptr(out), len(out), C.byref(m), C.byref(tot))
        if rc == SRL_ERR_BAD_ARG and m.value > len(out):
            out = np.zeros(m.value, dtype=COLOR_SELECTED_DTYPE)
            rc = self.lib.srl_lio_select_points_for_projection(self.h, *args, _ptr(out), len(out), C.byref(m), C.byref(tot))
        self._chk(rc, "srl_lio_select_points_for_projection")
        self._select_capacity = max(getattr(self, "_select_capacity", 0), m.value + m.value // 2)
        return out[:m.value].copy(), tot

    def refresh_points_for_projection(self, camera, rows, cols):
        return self.select_points_for_projection(camera, rows, cols, refresh=True)

    def color_cloud(self, which=0, minimum_views=1, with_index=True):
        """the publishers' coloured cloud (srl_lio_color_cloud): which = 0 pubColorPoints / threadPubColorPoints (the whole registered
        list, ascending), 1 saveColorPoints (descending, index 0 never saved).  Returns (records (COLOR_CLOUD_DTYPE), point_index or
        None, ColorCloudTotals)."""
        m, tot = C.c_int64(), ColorCloudTotals()
        # one call into a buffer sized by what earlier calls published; only a call that publishes more than that is asked again
        cap = max(getattr(self, "_cloud_capacity", 0), 4096)
        out = np.zeros(cap, dtype=COLOR_CLOUD_DTYPE)
        idx = np.zeros(cap, dtype=np.int32) if with_index else None
        rc = self.lib.srl_lio_color_cloud(self.h, int(which), int(minimum_views), _ptr(out), _ptr(idx), cap, C.byref(m), C.byref(tot))
        if rc == SRL_ERR_BAD_ARG and m.value > cap:
            cap = m.value
            out = np.zeros(cap, dtype=COLOR_CLOUD_DTYPE)
            idx = np.zeros(cap, dtype=np.int32) if with_index else None
            rc = self.lib.srl_lio_color_cloud(self.h, int(which), int(minimum_views), _ptr(out), _ptr(idx), cap, C.byref(m), C.byref(tot))
        self._chk(rc, "srl_lio_color_cloud")
        self._cloud_capacity = max(getattr(self, "_cloud_capacity", 0), m.value + m.value // 2)
        return out[:m.value].copy(), (idx[:m.value].copy() if with_index else None), tot

    def color_cloud_view(self, which=0, minimum_views=1, with_index=True):
        """the same through the object's own buffers (srl_lio_color_cloud_view: the mirror's pubColorPoints / saveColorPoints); the arrays
        returned here are copies of the view"""
        pts, idx, m, tot = C.c_void_p(), C.c_void_p(), C.c_int64(), ColorCloudTotals()
        self._chk(self.lib.srl_lio_color_cloud_view(self.h, int(which), int(minimum_views), 1 if with_index else 0, C.byref(pts), C.byref(idx),
                                                    C.byref(m), C.byref(tot)), "srl_lio_color_cloud_view")
        n = m.value
        rec = np.frombuffer((C.c_char * (n * 16)).from_address(pts.value), dtype=COLOR_CLOUD_DTYPE).copy() if n else np.zeros(0, COLOR_CLOUD_DTYPE)
        index = None
        if with_index:
            index = np.frombuffer((C.c_char * (n * 4)).from_address(idx.value), dtype=np.int32).copy() if n else np.zeros(0, np.int32)
        return rec, index, tot

    def color_topic_sizes(self, published):
        """one round of threadPubColorPoints' topic schedule for `published` points (srl_lio_color_topic_sizes): the topic sizes in order;
        the object carries number_of_points_per_topic and sleep_time_after_pub to the next round"""
        m = C.c_int()
        self._chk(self.lib.srl_lio_color_topic_sizes(self.h, int(published), None, 0, C.byref(m)), "srl_lio_color_topic_sizes")
        sizes = np.zeros(m.value, dtype=np.int32)
        self._chk(self.lib.srl_lio_color_topic_sizes(self.h, int(published), _ptr(sizes), len(sizes), C.byref(m)), "srl_lio_color_topic_sizes")
        return sizes

    def color_topic_state(self):
        """(number_of_points_per_topic, sleep_time_after_pub) as the next round will use them"""
        a, b = C.c_int(), C.c_int()
        self._chk(self.lib.srl_lio_color_topic_state(self.h, C.byref(a), C.byref(b)), "srl_lio_color_topic_state")
        return a.value, b.value

    def set_device_subsample(self, on):
        """buildFrame's sub-sample on the device (True, the default) or on the host (srl_lio_set_device_subsample)"""
        self._chk(self.lib.srl_lio_set_device_subsample(self.h, 1 if on else 0), "srl_lio_set_device_subsample")

    def resident_sweep(self, raw_xyz):
        r = _f64(raw_xyz, (-1, 3))
        self._chk(self.lib.srl_lio_resident_sweep(self.h, _ptr(r), len(r)), "resident_sweep")
        return len(r)

    def prefetch_sweep(self, raw_xyz):
        r = _f64(raw_xyz, (-1, 3))
        self._keep_prefetch = r
        self._chk(self.lib.srl_lio_prefetch_sweep(self.h, _ptr(r), len(r)), "prefetch_sweep")

    def swap_sweep(self):
        self._chk(self.lib.srl_lio_swap_sweep(self.h), "swap_sweep")

    def prefetch_sweep_during_solve(self, raw_xyz):
        """the upload of the NEXT sweep, issued by the next update_iekf beside the kernel of its first pass (srl_lio_prefetch_sweep_during_solve)"""
        r = _f64(raw_xyz, (-1, 3))
        self._keep_prefetch = r
        self._chk(self.lib.srl_lio_prefetch_sweep_during_solve(self.h, _ptr(r), len(r)), "prefetch_sweep_during_solve")

    def update_iekf(self, opts, raw_xyz, state, t_last, frame_id=100, log_iters=0, n_resident=None,
                    allow=(SRL_ERR_NOT_ENOUGH_RESIDUALS,)):
        """raw_xyz=None uses the sweep pinned by resident_sweep (n_resident = its size)."""
        if self.ctx is not None:
            self.ctx._select(opts)
        st = _f64(state).copy()
        log = np.zeros((max(log_iters, 1), 61)) if log_iters else None
        iters, nres = C.c_int(), C.c_int()
        if raw_xyz is None:
            rp, n = None, int(n_resident)
        else:
            r = _f64(raw_xyz, (-1, 3))
            rp, n = _ptr(r), len(r)
        rc = self._chk(self.lib.srl_lio_update_iekf(self.h, C.byref(opts), rp, n, _dptr(st), _dptr(_f64(t_last)), int(frame_id),
                                                    _ptr(log) if log is not None else None, log_iters, C.byref(iters), C.byref(nres)),
                       "update_iekf", ok=allow)
        return dict(rc=rc, state=st, iters=iters.value, num_residuals=nres.value, log=None if log is None else log[: iters.value])

    def bound_solver(self, opts, eskf_state, eskf_cov, state, t_last, frame_id, n_resident):
        """A zero-allocation closure for repeated solves of the resident sweep from the same prior (bench / replay
        loops): every argument is converted once; each call = srl_lio_eskf_set_state + _set_cov + srl_lio_update_iekf.
        Returns (status, iterations, residuals); the solved state is left in `solver.state`."""
        if self.ctx is not None:
            self.ctx._select(opts)
        es = _f64(eskf_state).copy(); ec = _f64(eskf_cov).ravel().copy()
        st0 = _f64(state).copy(); st = st0.copy(); tl = _f64(t_last).copy()
        iters, nres = C.c_int(), C.c_int()
        lib, h = self.lib, self.h
        p_es, p_ec, p_st, p_tl = _dptr(es), _dptr(ec), _dptr(st), _dptr(tl)
        o = C.byref(opts); bi, bn = C.byref(iters), C.byref(nres)
        set_state, set_cov, upd = lib.srl_lio_eskf_set_state, lib.srl_lio_eskf_set_cov, lib.srl_lio_update_iekf
        fid, n = int(frame_id), int(n_resident)

        def solve():
            st[:] = st0
            rc = set_state(h, p_es) or set_cov(h, p_ec) or upd(h, o, None, n, p_st, p_tl, fid, None, 0, bi, bn)
            return rc, iters.value, nres.value
        solve.state = st
        solve._keep = (es, ec, st0, tl, opts)
        return solve

    def bound_stream_step(self, opts, eskf_state, eskf_cov, state, t_last, frame_id, n_resident, next_pinned):
        """The node's loop body over a stream of sweeps as ONE C call per step (srl_lio_stream_step): prior reset, the upload of the NEXT
        sweep (`next_pinned`: a page-locked (n, 3) array) registered with the solve, the solve of the resident sweep, the swap.  Every argument
        is converted once.  Returns (status, iterations, residuals); the solved state is left in `step.state`."""
        if self.ctx is not None:
            self.ctx._select(opts)
        es = _f64(eskf_state).copy(); ec = _f64(eskf_cov).ravel().copy()
        st0 = _f64(state).copy(); st = st0.copy(); tl = _f64(t_last).copy()
        iters, nres = C.c_int(), C.c_int()
        lib, h = self.lib, self.h
        p_es, p_ec, p_st, p_tl = _dptr(es), _dptr(ec), _dptr(st), _dptr(tl)
        o = C.byref(opts); bi, bn = C.byref(iters), C.byref(nres)
        fn = lib.srl_lio_stream_step
        fid, n = int(frame_id), int(n_resident)
        nx_ptr, nx_n = next_pinned.ctypes.data_as(C.c_void_p), int(len(next_pinned))
        copy_state = np.copyto

        def step():
            copy_state(st, st0)
            return fn(h, o, p_es, p_ec, n, p_st, p_tl, fid, nx_ptr, nx_n, bi, bn), iters.value, nres.value
        step.state = st
        step._keep = (es, ec, st0, tl, opts, next_pinned)
        return step

    def update_iekf_provided(self, opts, provider, n, state, t_last, frame_id=100, log_iters=0,
                             allow=(SRL_ERR_NOT_ENOUGH_RESIDUALS,)):
        """provider(frame: Frame, opts: IcpOpts, out: NormalEq) -> int status."""
        if self.ctx is not None:
            self.ctx._select(opts)
        def _p(fp, op, outp, _user):
            return int(provider(fp.contents, op.contents, outp.contents))
        self._provider = PROVIDER_FN(_p)
        st = _f64(state).copy()
        log = np.zeros((max(log_iters, 1), 61)) if log_iters else None
        iters, nres = C.c_int(), C.c_int()
        rc = self._chk(self.lib.srl_lio_update_iekf_provided(self.h, C.byref(opts), self._provider, None, int(n), _dptr(st),
                                                             _dptr(_f64(t_last)), int(frame_id), _ptr(log) if log is not None else None,
                                                             log_iters, C.byref(iters), C.byref(nres)), "update_iekf_provided", ok=allow)
        return dict(rc=rc, state=st, iters=iters.value, num_residuals=nres.value, log=None if log is None else log[: iters.value])

    def optimize(self, opts, sample_voxel_size, frame_raw, frame_world, state, t_last, frame_id=100,
                 allow=(SRL_ERR_NOT_ENOUGH_RESIDUALS,)):
        if self.ctx is not None:
            self.ctx._select(opts)
        raw = _f64(frame_raw, (-1, 3))
        world = _f64(frame_world, (-1, 3)).copy()
        st = _f64(state).copy()
        kidx = np.empty(len(raw), dtype=np.int32)
        nk, iters, nres = C.c_int(), C.c_int(), C.c_int()
        rc = self._chk(self.lib.srl_lio_optimize(self.h, C.byref(opts), float(sample_voxel_size), _ptr(raw), _ptr(world), len(raw), _dptr(st),
                                                 _dptr(_f64(t_last)), int(frame_id), _ptr(kidx), C.byref(nk), C.byref(iters), C.byref(nres)),
                       "optimize", ok=allow)
        return dict(rc=rc, state=st, world=world, keypoint_index=kidx[: nk.value].copy(), iters=iters.value, num_residuals=nres.value)

    def set_odometry_options(self, **kw):
        o = OdometryOpts()
        d = dict(init_voxel_size=0.2, init_sample_voxel_size=1.0, init_num_frames=20, num_for_initialization=10, voxel_size=0.5,
                 sample_voxel_size=1.5, max_num_points_in_voxel=20, min_distance_points=0.1, motion_compensation=MC_CONSTANT_VELOCITY,
                 initialization=0, point_time_enable=1, acc_cov=0.1, gyr_cov=0.1, b_acc_cov=0.0001, b_gyr_cov=0.0001)
        icp = kw.pop("icp", None) or default_opts()
        d.update(kw)
        for k, v in d.items():
            setattr(o, k, v)
        o.icp = icp
        self._chk(self.lib.srl_lio_set_odometry_options(self.h, C.byref(o)), "set_odometry_options")
        return o

    def run_measurement(self, time_frame, imu_t, imu_acc, imu_gyr, pts_raw, pts_timestamp, time_sweep_begin, time_sweep_offset,
                        allow=(SRL_ERR_NOT_ENOUGH_RESIDUALS,)):
        it = _f64(imu_t); ia = _f64(imu_acc, (-1, 3)); ig = _f64(imu_gyr, (-1, 3))
        pr = _f64(pts_raw, (-1, 3)); pt = _f64(pts_timestamp)
        out = ReplayResult()
        rc = self._chk(self.lib.srl_lio_run_measurement(self.h, float(time_frame), _ptr(it), _ptr(ia), _ptr(ig), len(it), _ptr(pr), _ptr(pt),
                                                        len(pr), float(time_sweep_begin), float(time_sweep_offset), C.byref(out)),
                       "run_measurement", ok=allow)
        return dict(rc=rc, processed=bool(out.processed), initialized=bool(out.initialized), index_frame=out.index_frame,
                    success=bool(out.success), num_residuals=out.num_residuals_used, iters=out.iterations, frame_points=out.frame_points,
                    keypoints=out.keypoints, points_added=out.points_added, state=np.array(out.state))

    def run_measurement_image(self, time_frame, imu_t, imu_acc, imu_gyr, pts_raw, pts_timestamp, time_sweep_begin, time_sweep_offset, raw_bgr,
                              allow=(SRL_ERR_NOT_ENOUGH_RESIDUALS,)):
        """srl_lio_run_measurement_image: run_measurement with the measurement's camera frame, raw_bgr (rows, cols, 3) uint8 or None (no
        image: exactly run_measurement).  Returns run_measurement's dict with the ImageProcessResult under "image"."""
        it = _f64(imu_t); ia = _f64(imu_acc, (-1, 3)); ig = _f64(imu_gyr, (-1, 3))
        pr = _f64(pts_raw, (-1, 3)); pt = _f64(pts_timestamp)
        b, rows, cols, stride = None, 0, 0, 0
        if raw_bgr is not None:
            b = np.asarray(raw_bgr)
            if b.dtype != np.uint8 or b.ndim != 3 or b.shape[2] != 3 or b.strides[2] != 1 or b.strides[1] != 3 or b.strides[0] < 3 * b.shape[1]:
                b = np.ascontiguousarray(b, dtype=np.uint8)
            rows, cols, stride = b.shape[0], b.shape[1], b.strides[0]
        out, img = ReplayResult(), ImageProcessResult()
        rc = self._chk(self.lib.srl_lio_run_measurement_image(self.h, float(time_frame), _ptr(it), _ptr(ia), _ptr(ig), len(it), _ptr(pr), _ptr(pt),
                                                              len(pr), float(time_sweep_begin), float(time_sweep_offset), _ptr(b), rows, cols, stride,
                                                              C.byref(out), C.byref(img)), "run_measurement_image", ok=allow)
        return dict(rc=rc, processed=bool(out.processed), initialized=bool(out.initialized), index_frame=out.index_frame,
                    success=bool(out.success), num_residuals=out.num_residuals_used, iters=out.iterations, frame_points=out.frame_points,
                    keypoints=out.keypoints, points_added=out.points_added, state=np.array(out.state), image=img)

    def run_measurement_image_jpeg(self, time_frame, imu_t, imu_acc, imu_gyr, pts_raw, pts_timestamp, time_sweep_begin, time_sweep_offset, jpeg,
                                   allow=(SRL_ERR_NOT_ENOUGH_RESIDUALS,)):
        """srl_lio_run_measurement_image_jpeg: run_measurement_image with the frame as a baseline JPEG stream (bytes or uint8 array), or None"""
        it = _f64(imu_t); ia = _f64(imu_acc, (-1, 3)); ig = _f64(imu_gyr, (-1, 3))
        pr = _f64(pts_raw, (-1, 3)); pt = _f64(pts_timestamp)
        d = None if jpeg is None else _jpeg_bytes(jpeg)
        out, img = ReplayResult(), ImageProcessResult()
        rc = self._chk(self.lib.srl_lio_run_measurement_image_jpeg(self.h, float(time_frame), _ptr(it), _ptr(ia), _ptr(ig), len(it), _ptr(pr), _ptr(pt),
                                                                   len(pr), float(time_sweep_begin), float(time_sweep_offset), _ptr(d),
                                                                   0 if d is None else d.size, C.byref(out), C.byref(img)),
                       "run_measurement_image_jpeg", ok=allow)
        return dict(rc=rc, processed=bool(out.processed), initialized=bool(out.initialized), index_frame=out.index_frame,
                    success=bool(out.success), num_residuals=out.num_residuals_used, iters=out.iterations, frame_points=out.frame_points,
                    keypoints=out.keypoints, points_added=out.points_added, state=np.array(out.state), image=img)

    def set_lidar_options(self, opts):
        """srl_lio_set_lidar_options: opts = livox_opts(...)"""
        self._chk(self.lib.srl_lio_set_lidar_options(self.h, C.byref(opts)), "set_lidar_options")

    def feed_livox(self, points, header_stamp):
        """srl_lio_feed_livox (lioOptimization::livoxHandler): one message into the handle's device point queue; returns the report dict"""
        a = _livox_points(points)
        r = LivoxReport()
        self._chk(self.lib.srl_lio_feed_livox(self.h, _ptr(a), len(a), float(header_stamp), C.byref(r)), "feed_livox")
        return _livox_report_dict(r)

    def set_pc2_options(self, opts):
        """srl_lio_set_pc2_options: opts = pc2_opts(...)"""
        self._chk(self.lib.srl_lio_set_pc2_options(self.h, C.byref(opts)), "set_pc2_options")

    def feed_pointcloud2(self, data, layout, header_stamp):
        """srl_lio_feed_pointcloud2 (lioOptimization::standardCloudHandler): one message into the handle's device point queue"""
        d = np.ascontiguousarray(data, dtype=np.uint8)
        r = Pc2Report()
        self._chk(self.lib.srl_lio_feed_pointcloud2(self.h, _ptr(d), d.nbytes, C.byref(layout), float(header_stamp), C.byref(r)), "feed_pointcloud2")
        return _pc2_report_dict(r)

    def points_info(self):
        """srl_lio_points_info -> dict(size, front_timestamp, back_timestamp, last_time_lidar, last_end_time)"""
        n = C.c_int()
        f, b, tl, te = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        self._chk(self.lib.srl_lio_points_info(self.h, C.byref(n), C.byref(f), C.byref(b), C.byref(tl), C.byref(te)), "points_info")
        return dict(size=n.value, front_timestamp=f.value, back_timestamp=b.value, last_time_lidar=tl.value, last_end_time=te.value)

    def run_measurement_queued(self, time_frame, imu_t, imu_acc, imu_gyr, time_cut, time_sweep_begin, time_sweep_offset,
                               allow=(SRL_ERR_NOT_ENOUGH_RESIDUALS,)):
        """srl_lio_run_measurement_queued: run_measurement with the sweep cut from the device point queue at time_cut"""
        it = _f64(imu_t); ia = _f64(imu_acc, (-1, 3)); ig = _f64(imu_gyr, (-1, 3))
        out = ReplayResult()
        rc = self._chk(self.lib.srl_lio_run_measurement_queued(self.h, float(time_frame), _ptr(it), _ptr(ia), _ptr(ig), len(it), float(time_cut),
                                                               float(time_sweep_begin), float(time_sweep_offset), C.byref(out)),
                       "run_measurement_queued", ok=allow)
        return dict(rc=rc, processed=bool(out.processed), initialized=bool(out.initialized), index_frame=out.index_frame,
                    success=bool(out.success), num_residuals=out.num_residuals_used, iters=out.iterations, frame_points=out.frame_points,
                    keypoints=out.keypoints, points_added=out.points_added, state=np.array(out.state))

    def last_frame(self):
        n = C.c_int()
        self._chk(self.lib.srl_lio_last_frame(self.h, 0, None, None, None, C.byref(n)), "last_frame")
        raw = np.empty((n.value, 3)); pt = np.empty((n.value, 3)); imu = np.empty((n.value, 3))
        self._chk(self.lib.srl_lio_last_frame(self.h, n.value, _ptr(raw), _ptr(pt), _ptr(imu), C.byref(n)), "last_frame")
        return dict(raw_point=raw, point=pt, imu_point=imu)

    def optimize_resident(self, opts, sample_voxel_size, frame_raw, state, t_last, frame_id=100,
                          allow=(SRL_ERR_NOT_ENOUGH_RESIDUALS,)):
        if self.ctx is not None:
            self.ctx._select(opts)
        raw = _f64(frame_raw, (-1, 3))
        st = _f64(state).copy()
        kidx = np.empty(max(len(raw), 1), dtype=np.int32)
        nk, iters, nres = C.c_int(), C.c_int(), C.c_int()
        rc = self._chk(self.lib.srl_lio_optimize_resident(self.h, C.byref(opts), float(sample_voxel_size), _ptr(raw), len(raw), _dptr(st),
                                                          _dptr(_f64(t_last)), int(frame_id), _ptr(kidx), C.byref(nk), C.byref(iters),
                                                          C.byref(nres)), "optimize_resident", ok=allow)
        return dict(rc=rc, state=st, keypoint_index=kidx[: nk.value].copy(), iters=iters.value, num_residuals=nres.value)

    def commit_frame(self, state, voxel_size=1.0, cap=20, min_dist=0.15, min_num_points=0, want_world=True, want_added=True):
        world = np.empty((self.ctx.frame_size(), 3)) if want_world else None
        added = C.c_int()
        self._chk(self.lib.srl_lio_commit_frame(self.h, _dptr(_f64(state)), float(voxel_size), cap, float(min_dist), min_num_points,
                                                _ptr(world) if want_world else None, C.byref(added) if want_added else None), "commit_frame")
        return world, (added.value if want_added else None)

    def search_neighbors(self, point, nb=1, size=1.0, K=20, thr=1):
        out = np.zeros((K, 3)); vox = np.zeros((K, 3), dtype=np.int16); nf = C.c_int()
        self._chk(self.lib.srl_lio_search_neighbors(self.h, _dptr(_f64(point)), nb, size, K, thr, _ptr(out), _ptr(vox), C.byref(nf)), "search_neighbors")
        return out[: nf.value], vox[: nf.value]

    def neighborhood(self, pts):
        P = _f64(pts, (-1, 3))
        c = np.empty(3); n = np.empty(3); cov = np.empty(9); a = C.c_double()
        self._chk(self.lib.srl_lio_neighborhood(self.h, _ptr(P), len(P), _dptr(c), _dptr(n), _dptr(cov), C.byref(a)), "neighborhood")
        return dict(center=c, normal=n, covariance=cov.reshape(3, 3), a2D=a.value)

    def build_plane_residuals(self, opts, raw_xyz, state, t_last, frame_id=100):
        if self.ctx is not None:
            self.ctx._select(opts)
        r = _f64(raw_xyz, (-1, 3))
        rows = np.zeros((len(r), 15)); world = np.zeros((len(r), 3))
        nout, succ = C.c_int(), C.c_int(); loss = C.c_double()
        self._chk(self.lib.srl_lio_build_plane_residuals(self.h, C.byref(opts), _ptr(r), len(r), _dptr(_f64(state)), _dptr(_f64(t_last)), int(frame_id),
                                                         _ptr(rows), len(r), C.byref(nout), C.byref(loss), C.byref(succ), _ptr(world)),
                  "build_plane_residuals")
        return dict(rows=rows[: nout.value], loss_sum=loss.value, success=bool(succ.value), keypoint_world=world)

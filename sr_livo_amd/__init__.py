"""sr_livo_amd -- MI355X (gfx950) implementation of SR-LIVO's LIO scan-matching hot path.

The product is the C-ABI shared library ``libsrlivo_hip.so`` (include/srlivo_hip.h) plus the C++ host
mirror of the reference classes (sr_livo_amd/csrc/host/).  This package is the thin ctypes layer the
parity tests and bench.py use to drive that library; it contains no arithmetic of the path and no
CPU fallback: every compute entry point fails loudly when the HIP extension or a GPU is missing.
"""
from .capi import (  # noqa: F401
    LIB_PATH, SrlError, IcpOpts, Frame, NormalEq, Timing, Context, Lio,
    load_library, library_symbols, declared_symbols, default_opts, shard_range, shard_budget,
    grid_sampling, heap_topk, PinnedArray, comm_backend_info, comm_set_library, tr1_order,
    ColorVioArgs, ColorVioSums, COLOR_VIO_POINT_DTYPE, SRL_VIO_REPROJECTION, SRL_VIO_PHOTOMETRIC,
    Flow, FlowOpts, default_flow_opts,
    ColorTrackOpts, ColorTrackTotals, COLOR_TRACK_POINT_DTYPE, default_color_track_opts, Oft,
    ConsensusOpts, ConsensusResult, default_consensus_opts, SRL_CONSENSUS_FUNDAMENTAL, SRL_CONSENSUS_PNP,
    SRL_CONSENSUS_MAX_POINTS, SRL_CONSENSUS_MAX_HYPOTHESES,
    ImagePrep, ImagePrepOpts, ImagePrepInfo, default_image_prep_opts, image_prep_build_map, image_resize_build_tables,
    ImageProcessOpts, ImageProcessResult, ImageProcessSteps,
    LivoxOpts, LivoxReport, PointsCutReport, LIVOX_POINT_DTYPE, livox_opts, time_unit_scale,
    TIME_UNIT_SEC, TIME_UNIT_MS, TIME_UNIT_US, TIME_UNIT_NS,
    Pc2Layout, Pc2Opts, Pc2Report, PC2_POINT_DTYPES, PC2_DRIVER_LAYOUTS, LIDAR_LIVOX, LIDAR_VELO, LIDAR_OUST, LIDAR_ROBO,
    pc2_opts, pc2_message, pc2_yaw_angles,
    JpegInfo, jpeg_parse, jpeg_entropy_decode,
)

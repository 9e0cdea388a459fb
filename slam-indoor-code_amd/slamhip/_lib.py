"""ctypes binding of libslamhip (include/slamhip.h).

The shared library is built in-tree (``make -C slam-indoor-code_amd``) and loaded
from this directory.  There is no CPU fallback: if the library or a GPU is
missing, the calls that need them raise.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libslamhip.so")

# include/slamhip.h enums
SLAM_OK = 0
SLAM_E_INVALID_ARG = -1
SLAM_E_BAD_MATCHER = -2
SLAM_E_HIP = -3
SLAM_E_CAPACITY = -4
SLAM_E_NO_DEVICE = -5
SLAM_E_UNSUPPORTED = -6
SLAM_E_SOLVER = -7

SIFT_BF, SIFT_FLANN, ORB_BF = 0, 1, 2
NORM_DEFAULT, NORM_L1, NORM_L2, NORM_HAMMING = 0, 2, 4, 6
TYPE_5_8, TYPE_7_12, TYPE_9_16 = 0, 1, 2
HARRIS_SCORE, FAST_SCORE = 0, 1          # cv::ORB::ScoreType (slam_orb_detect's score_type)
LOSS_NONE, LOSS_TRIVIAL, LOSS_HUBER, LOSS_CAUCHY, LOSS_ARCTAN, LOSS_TUKEY = range(6)
EMPTY_BATCH, FRAME_NOT_FOUND = -2, -1
OPT_SIFT_KERNEL = 1
OPT_SIFT_BAND_SPLIT = 2
OPT_PNP_SUMS = 3
OPT_FAST_REUSE = 4
OPT_JPEG_LANES = 5
OPT_JPEG_SYNC = 6       # chunk-parallel entropy decoding: 0 off, 1 segments of at least 16 KiB, 2 every segment of more than a chunk
OPT_JPEG_CHUNK = 7      # bytes per chunk: a power of two in 16 .. 1024, 0 = 256
JPEG_MJPEG = 1          # parse flag of the _ex calls: a Motion-JPEG frame (Annex K tables when DHT is missing; AVI1 fields refused)
PNP_SUMS_ORDERED, PNP_SUMS_PAIRWISE = 0, 1
BAND_SPLIT_OFF, BAND_SPLIT_AUTO, BAND_SPLIT_ALL, BAND_SPLIT_ALL4 = 0, 1, 2, 3
STAGE_DESC_START, STAGE_DESC_END = 0, 1     # slam_order_after_stage
KNN_MODE_L2, KNN_MODE_SQRT, KNN_MODE_L2_PACKED, KNN_MODE_HAMMING_PACKED, KNN_MODE_L1_PACKED = 0, 2, 3, 4, 5
(KNN_VARIANT_MFMA, KNN_VARIANT_MFMA_PK_QT2, KNN_VARIANT_MFMA_PK_QT1, KNN_VARIANT_PIPE_QT2, KNN_VARIANT_PIPE_QT1,
 KNN_VARIANT_L1) = range(1, 7)
KNN_VARIANT_XCD = 0x100
SD_FORM_DOG_PLANES, SD_FORM_XCD, SD_FORM_DESC_STAGED, SD_FORM_DESC_CPL2, SD_FORM_DESC_XCD = 1, 2, 4, 8, 16   # slam_last_sift_detect_forms
KLT_USE_INITIAL_FLOW, KLT_GET_MIN_EIGENVALS = 4, 8     # cv::OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_LK_GET_MIN_EIGENVALS
KLT_MAX_LEVELS = 9                                     # maxLevel 0..8
JPEG_GRAY, JPEG_444, JPEG_422, JPEG_420 = 0, 0x11, 0x21, 0x22      # slam_jpeg_info's sampling
JPEG_EOF, JPEG_BAD_CODE, JPEG_RUN, JPEG_RESTART = 1, 2, 4, 8       # entropy fault bits of a decode's status
JPEG_ENC_OVERFLOW, JPEG_ENC_CATEGORY = 1, 2                        # status bits of an encode
SIM3_OK, SIM3_NO_MODEL, SIM3_TOO_FEW, SIM3_CHOLESKY = range(4)                      # slam_sim3_ransac's status
GBA_LOSS_SQUARE, GBA_LOSS_HUBER = 0, 1                             # slam_gba_params.loss
VOC_SIFT, VOC_ORB = 0, 1                                           # slam_voc_*'s descriptor kind
RENDER_POINT, RENDER_LINE, RENDER_FACE = 0, 1, 2                   # the kind in a rendered id (kind << 30 | index)
RENDER_AUTO, RENDER_THREAD, RENDER_WAVE, RENDER_WAVE_FULL_LIST = 0, 1, 2, 3   # slam_render_views_dev's raster_mode
SIFT_KERNEL_AUTO, SIFT_KERNEL_BAND,SIFT_KERNEL_TAB, SIFT_KERNEL_GENERAL, SIFT_KERNEL_COLS, SIFT_KERNEL_COLW = 0, 1, 2, 3, 4, 5

# byte-identical to cv::KeyPoint / cv::DMatch
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"),
                         ("distance", "<f4")])
assert KEYPOINT_DTYPE.itemsize == 28 and DMATCH_DTYPE.itemsize == 16


class BASummary(ctypes.Structure):
    _fields_ = [("initial_cost", ctypes.c_double), ("final_cost", ctypes.c_double),
                ("num_residuals", ctypes.c_int32), ("iterations", ctypes.c_int32),
                ("successful_steps", ctypes.c_int32), ("termination", ctypes.c_int32),
                ("usable", ctypes.c_int32), ("total_time_in_seconds", ctypes.c_double)]


class JpegInfo(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("channels", ctypes.c_int32),
                ("sampling", ctypes.c_int32), ("restart_interval", ctypes.c_int32), ("segments", ctypes.c_int32),
                ("orientation", ctypes.c_int32)]


class JpegSyncStats(ctypes.Structure):
    _fields_ = [("parallel_segments", ctypes.c_int32), ("fallback_segments", ctypes.c_int32),
                ("chunk_bytes", ctypes.c_int32), ("lanes", ctypes.c_int32), ("chunks", ctypes.c_int64),
                ("wg_rounds_max", ctypes.c_int32), ("launch_rounds_max", ctypes.c_int32),
                ("wg_rounds_total", ctypes.c_int64), ("launch_rounds_total", ctypes.c_int64),
                ("ms", ctypes.c_double * 5)]


class AviInfo(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("rate", ctypes.c_uint32),
                ("scale", ctypes.c_uint32), ("frames", ctypes.c_int64), ("handler", ctypes.c_uint32),
                ("compression", ctypes.c_uint32), ("stream", ctypes.c_int32)]


class GbaParams(ctypes.Structure):
    _fields_ = [("loss", ctypes.c_int32), ("loss_param", ctypes.c_double), ("zmin", ctypes.c_double),
                ("lambda0", ctypes.c_double), ("max_lm", ctypes.c_int32), ("max_pcg", ctypes.c_int32),
                ("pcg_tol", ctypes.c_double), ("cost_tol", ctypes.c_double)]


class GbaSummary(ctypes.Structure):
    _fields_ = [("cost0", ctypes.c_double), ("cost", ctypes.c_double), ("lm_steps", ctypes.c_int32),
                ("accepted", ctypes.c_int32), ("pcg_iters", ctypes.c_int32), ("kept_obs", ctypes.c_int32),
                ("behind_obs", ctypes.c_int32), ("points_held", ctypes.c_int32), ("cams_held", ctypes.c_int32)]


# exported symbols and their signatures: (restype, argtypes)
_P, _I, _SZ, _D, _U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_double, ctypes.c_uint64
_F = ctypes.c_float
SIGNATURES = {
    "slam_abi_version": (_I, []),
    "slam_device_count": (_I, []),
    "slam_create": (_P, [_I]),
    "slam_create_prio": (_P, [_I, _I]),
    "slam_destroy": (None, [_P]),
    "slam_last_error": (ctypes.c_char_p, [_P]),
    "slam_synchronize": (_I, [_P]),
    "slam_matcher_type": (_I, [_I, _I, _I]),
    "slam_fast": (_I, [_P, _P, _I, _I, _SZ, _I, _I, _I, _I, _P, _I, _P]),
    "slam_fast_dev": (_I, [_P, _P, _P, _I, _I, _SZ, _I, _I, _I, _I, _P, _I, _P]),
    "slam_describe": (_I, [_P, _P, _I, _I, _SZ, _I, _I, _P, _P, _P]),
    "slam_sift_detect": (_I, [_P, _P, _I, _I, _SZ, _I, _P, _I, _P, _P]),
    "slam_sift_detect_batch": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _P]),
    "slam_orb_detect": (_I, [_P, _P, _I, _I, _SZ, _I, _I, _F, _I, _I, _I, _P, _I, _P, _P]),
    "slam_orb_detect_batch": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _F, _I, _I, _I, _P, _I, _P, _P]),
    "slam_reconstruct": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "slam_estimate_transformation": (_I, [_P, _P, _P, _I, _P, _I, _D, _D, _D, _P, _P, _P, _P, _P]),
    "slam_solve_pnp_ransac": (_I, [_P, _P, _P, _I, _P, _I, ctypes.c_float, _D, _P, _P, _P, _P, _P]),
    "slam_rodrigues": (_I, [_P, _I, _P]),
    "slam_knn2": (_I, [_P, _P, _I, _P, _I, _I, _I, _P, _P]),
    "slam_match": (_I, [_P, _P, _I, _P, _I, _I, _I, _D, _P, _I, _P]),
    "slam_match_frame": (_I, [_P, _P, _I, _P, _I, _I, _SZ, _I, _I, _I, _D, _P, _P, _P, _I, _P]),
    "slam_select_good": (_I, [_P, _I, _I, _I, _I]),
    "slam_ba": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _D, _I, ctypes.POINTER(BASummary)]),
    "slam_batch_extract": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "slam_batch_match": (_I, [_P, _P, _P, _I, _I, _D, _P]),
    "slam_batch_extract_match": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _D, _P, _P]),
    "slam_batch_extract_match_ev": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _D, _P, _P, _P]),
    "slam_batch_extract_async": (_I, [_P, _P, _P, _I, _I, _I, _I, _I]),
    "slam_batch_match_async": (_I, [_P, _P, _I, _I, _D, _P]),
    "slam_batch_finish": (_I, [_P, _P, _P]),
    "slam_context_stream": (_P, [_P]),
    "slam_batch_desc_bytes": (_SZ, [_I, _I]),
    "slam_batch_counts": (_I, [_P, _P, _P, _I]),
    "slam_batch_export_desc": (_I, [_P, _P, _I, _P, _P]),
    "slam_batch_get_keypoints": (_I, [_P, _I, _P, _I, _P]),
    "slam_batch_get_descriptors": (_I, [_P, _I, _P, _I, _P]),
    "slam_batch_get_matches": (_I, [_P, _I, _P, _I, _P]),
    "slam_batch_get_result": (_I, [_P, _I, _P, _I, _P, _P, _I, _P]),
    "slam_batch_result_begin": (_I, [_P, _I]),
    "slam_batch_result_end": (_I, [_P, _P, _I, _P, _P, _I, _P]),
    "slam_batch_result_dev": (_I, [_P, _P, _I, _P, _I, _P, _I]),
    "slam_order_after": (_I, [_P, _P, _P]),
    "slam_order_after_stage": (_I, [_P, _P, _I]),
    "slam_set_option": (_I, [_P, _I, _I]),
    "slam_batch_fast_reused": (_I, [_P]),
    "slam_last_sift_kernel": (_I, [_P]),
    "slam_last_knn_launch": (_I, [_P, _P, _P, _P]),
    "slam_last_sift_detect_forms": (_I, [_P, _P, _P]),
    "slam_profile_enable": (_I, [_P, _I]),
    "slam_profile_read": (_I, [_P, _I, _P, _P]),
    "slam_synth_frames": (_I, [_I, _I, _I, _I, _U64, _P]),
    "slam_synth_sequence": (_I, [_I, _I, _I, _I, _U64, _I, _P]),
    "slam_batch_fast": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "slam_synth_sequence_dev": (_I, [_P, _P, _I, _I, _I, _I, _U64, _I, _P]),
    "slam_cluster_points": (_I, [_P, _P, _P, _I, _F, _F, _F, _P, _P]),
    "slam_cluster_points_dev": (_I, [_P, _P, _P, _P, _I, _F, _F, _F, _P]),
    "slam_cluster_last_stats": (_I, [_P, _P, _P]),
    "slam_fit_plane": (_I, [_P, _P, _I, _P, _P]),
    "slam_plane_moments": (_I, [_P, _P, _I, _P, _P, _P]),
    "slam_project_to_plane": (_I, [_P, _P, _I, _P, _P, _P]),
    "slam_delaunay_2d": (_I, [_P, _P, _I, _P, _I, _P]),
    "slam_delaunay_2d_dev": (_I, [_P, _P, _P, _I, _P, _I, _P]),
    "slam_delaunay_last_stats": (_I, [_P, _P, _P, _P]),
    "slam_delaunay_predicates": (_I, [_P, _P, _P, _I, _P, _P]),
    "slam_delaunay_2d_host": (_I, [_P, _I, _P, _I, _P]),
    "slam_mesh_filter": (_I, [_P, _I, _P, _I, _D, _P, _P]),
    "slam_undistort_batch": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _I, _P]),
    "slam_undistort": (_I, [_P, _P, _I, _I, _SZ, _I, _P, _P, _I, _P, _P, _SZ]),
    "slam_undistort_map": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P]),
    "slam_undistort_points": (_I, [_P, _P, _SZ, _I, _P, _P, _I, _P, _I, _D, _P, _P]),
    "slam_undistort_points_dev": (_I, [_P, _P, _P, _SZ, _I, _P, _P, _I, _P, _I, _D, _P, _P]),
    "slam_fisheye_undistort_batch": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _I, _P]),
    "slam_fisheye_undistort": (_I, [_P, _P, _I, _I, _SZ, _I, _P, _P, _I, _P, _P, _SZ]),
    "slam_fisheye_undistort_map": (_I, [_P, _I, _I, _P, _P, _I, _P, _P, _P]),
    "slam_fisheye_undistort_points": (_I, [_P, _P, _SZ, _I, _P, _P, _I, _P, _I, _D, _P, _P]),
    "slam_fisheye_undistort_points_dev": (_I, [_P, _P, _P, _SZ, _I, _P, _P, _I, _P, _I, _D, _P, _P]),
    "slam_chess_candidates": (_I, [_P, _P, _I, _I, _SZ, _I, _P, _I, _P, _P]),
    "slam_chess_candidates_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _P]),
    "slam_label_chessboard": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "slam_label_chessboard_grow": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "slam_find_chessboard": (_I, [_P, _P, _I, _I, _SZ, _I, _I, _I, _P, _P]),
    "slam_find_chessboard_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "slam_corner_subpix": (_I, [_P, _P, _I, _I, _SZ, _I, _P, _I, _I, _I, _I, _I, _I, _D]),
    "slam_corner_subpix_dev": (_I, [_P, _P, _P, _I, _I, _SZ, _I, _P, _I, _I, _I, _I, _I, _I, _D]),
    "slam_calibrate_camera": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "slam_fisheye_calibrate": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "slam_klt_pyramid": (_I, [_P, _P, _I, _I, _SZ, _I, _I, _I, _I, _P, _P, _P, _P, _SZ, _P]),
    "slam_klt_track": (_I, [_P, _P, _SZ, _P, _SZ, _I, _I, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _D, _I, _D]),
    "slam_klt_track_dev": (_I, [_P, _P, _P, _P, _I, _I, _SZ, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _D, _I, _D]),
    "slam_klt_track_batch_dev": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _D, _I,
                                      _D]),
    "slam_jpeg_last_error": (ctypes.c_char_p, []),
    "slam_jpeg_info": (_I, [_P, _SZ, _P]),
    "slam_jpeg_decode_host": (_I, [_P, _SZ, _P, _SZ, _I, _P]),
    "slam_jpeg_decode": (_I, [_P, _P, _SZ, _P, _SZ, _I, _P]),
    "slam_jpeg_decode_batch_dev": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P]),
    "slam_jpeg_last_orientations": (_I, [_P, _P, _I]),
    "slam_jpeg_last_timing": (_I, [_P, _P, _P]),
    "slam_jpeg_info_ex": (_I, [_P, _SZ, _P, _I]),
    "slam_jpeg_decode_host_ex": (_I, [_P, _SZ, _P, _SZ, _I, _I, _P]),
    "slam_jpeg_decode_batch_dev_ex": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _P, _I]),
    "slam_jpeg_std_table": (_I, [_I, _I, _P, _P, _P]),
    "slam_jpeg_last_sync": (_I, [_P, _P]),
    "slam_jpeg_decode_host_sync": (_I, [_P, _SZ, _P, _SZ, _I, _I, _I, _P, _P]),
    "slam_avi_last_error": (ctypes.c_char_p, []),
    "slam_avi_index": (_I, [_P, _SZ, _P, _P, _P, _SZ]),
    "slam_jpeg_encode_bound": (_SZ, [_I, _I, _I, _I]),
    "slam_jpeg_encode_host": (_I, [_P, _I, _I, _I, _SZ, _I, _I, _I, _P, _SZ, _P, _P]),
    "slam_jpeg_enc_last_error": (ctypes.c_char_p, []),
    "slam_jpeg_encode": (_I, [_P, _P, _I, _I, _I, _SZ, _I, _I, _I, _P, _SZ, _P, _P]),
    "slam_jpeg_encode_batch_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _SZ, _SZ, _I, _I, _I, _P, _SZ, _P, _P]),
    "slam_jpeg_enc_last_timing": (_I, [_P, _P, _P]),
    "slam_render_views_dev": (_I, [_P, _P, _P, _P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _I, _I, _I, _P, _P, _P, _I, _I]),
    "slam_render": (_I, [_P, _P, _P, _I, _P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P, _P, _P]),
    "slam_render_last_stats": (_I, [_P, _P, _P]),
    "slam_mvs_census_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "slam_mvs_depth_batch_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "slam_mvs_fuse_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _D, _I, _I, _I, _P, _P, _I,
                               _P]),
    "slam_mvs_depth": (_I, [_P, _P, _P, _I, _I, _I, _SZ, _I, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "slam_mvs_fuse": (_I, [_P, _P, _I, _I, _SZ, _I, _I, _P, _P, _P, _P, _P, _P, _P, _D, _I, _I, _I, _P, _P, _I, _P]),
    "slam_mvs_last_timing": (_I, [_P, _P]),
    "slam_mvs_depth_host": (_I, [_P, _P, _I, _I, _I, _SZ, _I, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "slam_mvs_cost_volume_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P]),
    "slam_mvs_sgm_aggregate_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "slam_mvs_depth_sgm_batch_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I,
                                          _P, _P, _P]),
    "slam_mvs_depth_sgm": (_I, [_P, _P, _P, _I, _I, _I, _SZ, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "slam_mvs_sgm_set_budget": (_I, [_P, _SZ]),
    "slam_mvs_sgm_last_timing": (_I, [_P, _P]),
    "slam_mvs_cost_volume_host": (_I, [_P, _P, _I, _I, _I, _SZ, _I, _P, _P, _P, _I, _I, _P, _P]),
    "slam_mvs_sgm_aggregate_host": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "slam_mvs_depth_sgm_host": (_I, [_P, _P, _I, _I, _I, _SZ, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "slam_tsdf_integrate_dev": (_I, [_P, _P, _P, _I, _I, _I, _P, _D, _D, _P, _I, _I, _I, _I, _P, _P, _P, _I]),
    "slam_tsdf_mesh_dev": (_I, [_P, _P, _P, _I, _I, _I, _P, _D, _I, _P, _P, _P, _I, _I, _P, _P]),
    "slam_tsdf_integrate": (_I, [_P, _P, _I, _I, _I, _P, _D, _D, _P, _I, _I, _I, _I, _P, _P, _P, _I]),
    "slam_tsdf_mesh": (_I, [_P, _P, _I, _I, _I, _P, _D, _I, _P, _P, _P, _I, _I, _P, _P]),
    "slam_tsdf_integrate_host": (_I, [_P, _I, _I, _I, _P, _D, _D, _P, _I, _I, _I, _I, _P, _P, _P, _I]),
    "slam_tsdf_mesh_host": (_I, [_P, _I, _I, _I, _P, _D, _I, _P, _P, _P, _I, _I, _P, _P]),
    "slam_tsdf_last_timing": (_I, [_P, _P]),
    "slam_tex_select_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "slam_tex_layout": (_I, [_I, _I, _I, _P, _P, _P, _I, _P, _P]),
    "slam_tex_fill_dev": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P]),
    "slam_tex_select": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "slam_tex_fill": (_I, [_P, _P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P]),
    "slam_tex_select_host": (_I, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "slam_tex_fill_host": (_I, [_P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P]),
    "slam_tex_last_timing": (_I, [_P, _P]),
    "slam_voc_assign_dev": (_I, [_P, _P, _P, _I, _P, _I, _I, _P, _P]),
    "slam_voc_train_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    "slam_bow_vectors_dev": (_I, [_P, _P, _P, _P, _I, _P, _I, _P, _P]),
    "slam_bow_score_dev": (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _I, _P]),
    "slam_bow_topk_dev": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "slam_voc_assign": (_I, [_P, _P, _I, _P, _I, _I, _P, _P]),
    "slam_voc_train": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "slam_bow_vectors": (_I, [_P, _P, _P, _I, _P, _I, _P, _P]),
    "slam_bow_query": (_I, [_P, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "slam_voc_assign_host": (_I, [_P, _I, _P, _I, _I, _P, _P]),
    "slam_voc_train_host": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "slam_bow_vectors_host": (_I, [_P, _P, _I, _P, _I, _P, _P]),
    "slam_bow_score_host": (_I, [_P, _P, _I, _P, _P, _I, _I, _P]),
    "slam_sim3_ransac_dev": (_I, [_P, _P, _P, _P, _P, _I, _P, _I, _D, _U64, _P, _P, _P, _P]),
    "slam_sim3_ransac": (_I, [_P, _P, _P, _P, _I, _P, _I, _D, _U64, _P, _P, _P, _P]),
    "slam_sim3_ransac_host": (_I, [_P, _P, _P, _I, _P, _I, _D, _U64, _P, _P, _P, _P]),
    "slam_pgo_sim3_dev": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _D, _D, _I, _I, _D, _D, _P, _P]),
    "slam_pgo_sim3": (_I, [_P, _P, _I, _P, _P, _P, _I, _D, _D, _I, _I, _D, _D, _P, _P]),
    "slam_pgo_sim3_host": (_I, [_P, _I, _P, _P, _P, _I, _D, _D, _I, _I, _D, _D, _P, _P]),
    "slam_sim3_apply_points_dev": (_I, [_P, _P, _P, _P, _I, _P, _P, _I, _P]),
    "slam_sim3_apply_points": (_I, [_P, _P, _P, _I, _P, _P, _I, _P]),
    "slam_sim3_apply_points_host": (_I, [_P, _P, _I, _P, _P, _I, _P]),
    "slam_gba_dev": (_I, [_P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _I, _P, _P]),
    "slam_gba": (_I, [_P, _P, _P, _I, _P, _I, _P, _P, _P, _I, _P, _P]),
    "slam_gba_host": (_I, [_P, _P, _I, _P, _I, _P, _P, _P, _I, _P, _P]),
}

_lib = None


def lib():
    """Load libslamhip.so (raises OSError when it has not been built)."""
    global _lib
    if _lib is None:
        # torch ships its own HIP runtime (torch/lib/libamdhip64.so, SONAME
        # libamdhip64.so.7).  Loading it first makes libslamhip bind to that same
        # runtime by SONAME; loading libslamhip first would put two HIP runtimes
        # in one process and torch would then see no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise OSError(f"libslamhip.so not built: {LIB_PATH} (run make -C slam-indoor-code_amd)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def ptr(a):
    """data pointer of a numpy array (None for None)."""
    if a is None:
        return None
    return ctypes.c_void_p(a.ctypes.data)


class SlamError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"slamhip error {code}: {msg}")
        self.code = code


def check(code, ctx=None):
    if code == SLAM_OK:
        return
    msg = ""
    if ctx is not None:
        m = lib().slam_last_error(ctx)
        msg = m.decode() if m else ""
    raise SlamError(code, msg)

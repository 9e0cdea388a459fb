"""slamhip: MI355X (gfx950) implementation of the FIT-2023-SLAM-indoor
extract -> match -> windowed-BA hot path, behind the reference's interface.

    import slamhip
    kps = slamhip.fastExtractor(frame, threshold=31)
    kps, desc = slamhip.extractDescriptor(frame, kps, slamhip.SIFT_FLANN)

The compute runs in libslamhip.so (hand-written HIP kernels); this package is
the host-side mirror of the reference's mainModule headers plus the
device-resident candidate scan (slamhip.batch).
"""
from ._lib import (DMATCH_DTYPE, EMPTY_BATCH, FRAME_NOT_FOUND, KEYPOINT_DTYPE, LOSS_ARCTAN, LOSS_CAUCHY,
                   LOSS_HUBER, LOSS_NONE, LOSS_TRIVIAL, LOSS_TUKEY, NORM_DEFAULT, NORM_HAMMING, NORM_L1, NORM_L2,
                   ORB_BF, SIFT_BF, SIFT_FLANN, HARRIS_SCORE, FAST_SCORE, KLT_GET_MIN_EIGENVALS, KLT_USE_INITIAL_FLOW, TYPE_5_8, TYPE_7_12, TYPE_9_16, SIGNATURES, SlamError, lib)
from .api import (Context, GlobalData, MatcherTypeError, TemporalImageData, ba_rmse, bundle_adjust_arrays,
                  bundleAdjustment, default_context, extractDescriptor, fastExtractor, getGoodMatches,
                  estimateTransformation, reconstruct, siftDetectAndCompute, siftDetectAndComputeBatch, SiftBatch, solvePnPRansac,
                  orbDetectAndCompute, orbDetectAndComputeBatch, OrbBatch,
                  getMatcherTypeIndex, knnMatch2, lastKnnLaunch, lastSiftDetectForms, loss_from_config, matchFeatures, matchFramesPairFeatures,
                  rodrigues_to_matrix, rodrigues_to_vector, selectGoodFrame, synth_frames,
                  SYNTH_DRIFT, SYNTH_STEADY, synth_frames_dev,
                  clusterizePoints, clusterLabels, getBestFittingPlaneByPoints, planeMoments, projectToPlane,
                  delaunay2d, delaunay2dHost, delaunayStats, delaunayPredicates, meshFilter,
                  load_calibration, undistort, undistortBatch, undistortMap, undistortPoints,
                  fisheyeUndistort, fisheyeUndistortBatch, fisheyeUndistortMap, fisheyeUndistortPoints,
                  fisheyeCalibrate,
                  chessCandidates, labelChessboard, findChessboardCorners, cornerSubPix, calibrateCamera,
                  buildOpticalFlowPyramid, calcOpticalFlowPyrLK, kltLevelSizes,
                  save_calibration, calibration_model,
                  imdecode, imread, imdecode_batch, jpegInfo, jpegLastTiming, applyOrientation,
                  jpegLastSync, imdecode_host_sync, imdecode_host, jpegStdTable, aviIndex,
                  imencode, imwrite, imencode_batch, jpegEncode, jpegEncodeBound, jpegEncLastTiming,
                  IMWRITE_JPEG_QUALITY, IMWRITE_JPEG_RST_INTERVAL, IMWRITE_JPEG_SAMPLING_FACTOR,
                  IMWRITE_JPEG_SAMPLING_FACTOR_420, IMWRITE_JPEG_SAMPLING_FACTOR_422, IMWRITE_JPEG_SAMPLING_FACTOR_444,
                  renderViews, renderCamera, renderStats,
                  censusTransform, planeSweepDepth, planeSweepDepthBatch, fuseDepthMaps,
                  planeSweepCostVolume, sgmAggregate, planeSweepDepthSgm, planeSweepDepthSgmBatch, sgmLastTiming,
                  tsdfIntegrate, tsdfMesh, tsdfLastTiming,
                  texSelect, texLayout, texFill, texLastTiming)
from .dense import DenseParams, SgmParams, densify, depth_maps, depth_planes, sweep_matrices
from . import surface
from .surface import SurfaceParams, TextureParams, projection_matrix, volume_bounds
from .place import Database, LoopParams, Vocabulary, detect_loops, verify_loop
from . import place
from . import loopclose
from .loopclose import (apply_points, close_loops, correct_map, loop_constraints, optimize_pose_graph,
                        sim3_from_pairs)
from . import globalba
from .globalba import global_bundle_adjust, merge_observations, refine_closed
from .video import VideoCapture, VideoWriter, write_mjpeg_avi
from .config import ConfigError, ConfigService, reference_example
from .calibration import CalibrationError, chessboard_photos_calibration

__all__ = [n for n in dir() if not n.startswith("_")]

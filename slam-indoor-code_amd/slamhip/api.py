"""Host-side mirror of the reference's hot-path interface, over libslamhip.

Names, argument meaning and error behaviour follow the reference's mainModule
headers so that a caller (or a parity test) reads like the reference:

  fastExtractor            src/mainModule/featureExtraction/fastExtractor.h:19-21
  extractDescriptor        src/mainModule/featureMatching/featureMatching.h:12-17
  matchFramesPairFeatures  featureMatching.h:47-53 (the 5-arg overload the batch uses)
  matchFeatures            featureMatchingCPU.cpp:17-43 (static in the reference)
  getGoodMatches           featureMatchingCommon.h:45-48
  getMatcherTypeIndex      featureMatchingCommon.h:19
  bundleAdjustment         src/mainModule/bundleAdjustment/bundleAdjustment.h:50-54

C++ passes containers by reference and mutates them; here the outputs are
returned (numpy arrays cannot shrink in place): ORB's border filter returns the
filtered keypoint array, exactly the vector the reference's caller ends up with.
Every computation runs in the HIP library on the GPU; there is no CPU path.
"""
import ctypes
import math
import os

import numpy as np

from . import _lib as L
from ._lib import DMATCH_DTYPE, KEYPOINT_DTYPE, check, lib, ptr


class MatcherTypeError(Exception):
    """getMatcherTypeIndex / extractDescriptor with an invalid type (the reference
    throws std::exception, featureMatchingCommon.cpp:20, featureMatchingCPU.cpp:37,63)."""


_default_ctx = None


class Context:
    """One HIP stream + device workspace (slam_ctx).  Not thread-safe: the
    reference's worker threads (batch.cpp:181-200) each need their own."""

    def __init__(self, device=0, priority=0):
        """priority > 0: the stream gets the device's highest priority
        (slam_create_prio)"""
        self.device = device
        self._det_out = None     # siftDetectAndCompute's reusable host output space (key, kps, desc)
        self.handle = lib().slam_create_prio(device, int(priority)) if priority else lib().slam_create(device)
        if not self.handle:
            raise L.SlamError(L.SLAM_E_NO_DEVICE, f"cannot open HIP device {device}")

    def set_option(self, option, value):
        """slam_set_option: per-context choices (all but L.OPT_PNP_SUMS never change results; e.g.
        L.OPT_SIFT_KERNEL -> L.SIFT_KERNEL_BAND / _TAB / _GENERAL / _AUTO)."""
        L.check(lib().slam_set_option(self.handle, int(option), int(value)), self.handle)
        self.__dict__.setdefault("_options", {})[int(option)] = int(value)

    def get_option(self, option):
        """the value last set through set_option (0, every option's default, when it never was)"""
        return self.__dict__.get("_options", {}).get(int(option), 0)

    def close(self):
        self._det_out = None
        if self.handle:
            lib().slam_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def _img(a):
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint8:
        raise TypeError("frames are 8-bit (CV_8UC1/3/4)")
    if a.ndim == 2:
        return a, a.shape[1], a.shape[0], 1
    if a.ndim == 3 and a.shape[2] in (3, 4):
        return a, a.shape[1], a.shape[0], a.shape[2]
    raise ValueError("frame must be HxW, HxWx3 (BGR) or HxWx4")


def _ctx(ctx):
    return (ctx or default_context()).handle


def fastExtractor(srcImage, threshold=10, suppression=True, type=L.TYPE_9_16, ctx=None):
    """FAST keypoints of a BGR (or gray) frame, raster order (fastExtractor.cpp:7-13)."""
    c = _ctx(ctx)
    img, w, h, ch = _img(srcImage)
    cap = max(4096, w * h // 16)
    while True:
        out = np.empty(cap, KEYPOINT_DTYPE)      # the library writes the first n (no zero fill: cap is ~w*h/16)
        n = ctypes.c_int(0)
        rc = lib().slam_fast(c, ptr(img), w, h, img.strides[0], ch, int(threshold), int(bool(suppression)),
                             int(type), ptr(out), cap, ctypes.byref(n))
        if rc == L.SLAM_E_CAPACITY:
            cap = n.value
            continue
        check(rc, c)
        return out[:n.value].copy()


def getMatcherTypeIndex(config):
    """featureMatchingCommon.cpp:13-21: SIFT_BF > SIFT_FLANN > ORB."""
    t = lib().slam_matcher_type(int(bool(config.getValue("useFM-SIFT-BF"))),
                                int(bool(config.getValue("useFM-SIFT-FLANN"))),
                                int(bool(config.getValue("useFM-ORB"))))
    if t < 0:
        raise MatcherTypeError("no feature matcher selected")
    return t


def _check_type(t):
    if t not in (L.SIFT_BF, L.SIFT_FLANN, L.ORB_BF):
        raise MatcherTypeError(f"invalid matcher type {t}")


def extractDescriptor(frame, features, extractorType, ctx=None):
    """SIFT (n x 128 float32, integer values) or ORB (n x 32 uint8) descriptors.
    Returns (features, desc); ORB returns the border-filtered keypoints."""
    _check_type(extractorType)
    c = _ctx(ctx)
    img, w, h, ch = _img(frame)
    kps = np.ascontiguousarray(np.asarray(features, KEYPOINT_DTYPE)).copy()
    n = ctypes.c_int(len(kps))
    if extractorType == L.ORB_BF:
        desc = np.empty((max(len(kps), 1), 32), np.uint8)      # the first n rows are written
    else:
        desc = np.empty((max(len(kps), 1), 128), np.float32)
    rc = lib().slam_describe(c, ptr(img), w, h, img.strides[0], ch, int(extractorType), ptr(kps), ctypes.byref(n),
                             ptr(desc))
    check(rc, c)
    return kps[:n.value].copy(), desc[:n.value].copy()


def siftDetectAndCompute(frame, ctx=None, with_descriptors=True):
    """cv::SIFT::create()->detectAndCompute(frame, noArray(), kps, desc): the full
    detector (DoG pyramid on the doubled image, extrema, orientation histogram)
    + 128-D descriptors (n x 128 float32, integer values).  Returns (kps, desc)."""
    cobj = ctx or default_context()
    c = cobj.handle
    img, w, h, ch = _img(frame)
    cap = max(4096, w * h // 16)
    while True:
        # output space kept on the context between its calls and freed by
        # Context.close() (the first n rows are copied out): a fresh
        # w * h / 16-row array per frame cost its page faults
        key = (cap, bool(with_descriptors))
        det = cobj._det_out
        if det is None or det[0] != key:
            det = (key, np.empty(cap, KEYPOINT_DTYPE), np.empty((cap, 128), np.float32) if with_descriptors else None)
            cobj._det_out = det
        _, kps, desc = det
        n = ctypes.c_int(0)
        rc = lib().slam_sift_detect(c, ptr(img), w, h, img.strides[0], ch, ptr(kps), cap, ctypes.byref(n),
                                    ptr(desc) if desc is not None else None)
        if rc == L.SLAM_E_CAPACITY and n.value > cap:
            cap = n.value
            continue
        check(rc, c)
        k = kps[:n.value].copy()
        return k, (desc[:n.value].copy() if desc is not None else None)


class SiftBatch:
    """siftDetectAndComputeBatch's result: keypoints (n, cap) and descriptors
    (n, cap, 128) float32 in device memory (torch tensors; frame f's first
    counts[f] rows are its keypoints / descriptors), counts (n,) on the host."""

    def __init__(self, kps_dev, desc_dev, counts):
        self.kps_dev, self.desc_dev, self.counts = kps_dev, desc_dev, counts

    def __len__(self):
        return len(self.counts)

    def host(self, f):
        """frame f's (keypoints, descriptors) as siftDetectAndCompute returns them"""
        n = int(self.counts[f])
        k = self.kps_dev[f, :n].cpu().numpy().reshape(-1).view(KEYPOINT_DTYPE).copy()
        d = self.desc_dev[f, :n].cpu().numpy().copy() if self.desc_dev is not None else None
        return k, d


def siftDetectAndComputeBatch(frames, ctx=None, with_descriptors=True, cap=None):
    """siftDetectAndCompute over a device-resident batch: frames is a CUDA uint8
    tensor (n, h, w, 3) or (n, h, w), already in HBM (slam_sift_detect_batch;
    every kernel launch covers the batch).  The keypoints and descriptors stay
    in device memory: returns a SiftBatch (SiftBatch.host(f) gives frame f's
    (kps, desc) as siftDetectAndCompute returns them)."""
    import torch
    c = _ctx(ctx)
    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() in (3, 4)):
        raise ValueError("frames: a CUDA uint8 tensor (n, h, w[, 3])")
    frames = frames.contiguous()
    n, h, w = frames.shape[:3]
    ch = frames.shape[3] if frames.dim() == 4 else 1
    torch.cuda.current_stream(frames.device).synchronize()   # the library's stream reads the frames next
    cap = cap or max(4096, w * h // 32)
    while True:
        kps = torch.empty((n, cap, KEYPOINT_DTYPE.itemsize), dtype=torch.uint8, device=frames.device)
        desc = torch.empty((n, cap, 128), dtype=torch.float32, device=frames.device) if with_descriptors else None
        cnt = np.zeros(n, np.int32)
        rc = lib().slam_sift_detect_batch(c, None, ctypes.c_void_p(frames.data_ptr()), n, w, h, ch,
                                          ctypes.c_void_p(kps.data_ptr()), cap, ptr(cnt),
                                          ctypes.c_void_p(desc.data_ptr()) if desc is not None else None)
        if rc == L.SLAM_E_CAPACITY and n and int(cnt.max()) > cap:
            cap = int(cnt.max())
            continue
        check(rc, c)
        return SiftBatch(kps, desc, cnt)


def orbDetectAndCompute(frame, nfeatures=500, scaleFactor=1.2, nlevels=8, fastThreshold=20,
                        scoreType=L.HARRIS_SCORE, ctx=None, with_descriptors=True, cap=None):
    """cv::ORB::create(nfeatures, scaleFactor, nlevels, 31, 0, 2, scoreType, 31,
    fastThreshold)->detectAndCompute(frame, noArray(), kps, desc): the full ORB
    detector (8-level pyramid, FAST + Harris ranking, intensity-centroid angle,
    steered rBRIEF).  Returns (kps, desc); desc is n x 32 uint8, usable with
    matchFeatures / slamhip.match(..., ORB_BF).  Keypoints come level by level,
    raster order inside a level (slam_orb_detect).  cap: the first output
    capacity tried (grown to the count found)."""
    c = _ctx(ctx)
    img, w, h, ch = _img(frame)
    cap = int(cap) if cap is not None else max(1024, 2 * int(nfeatures) + 256)
    while True:
        kps = np.empty(max(cap, 1), KEYPOINT_DTYPE)
        desc = np.empty((max(cap, 1), 32), np.uint8) if with_descriptors else None
        n = ctypes.c_int(0)
        rc = lib().slam_orb_detect(c, ptr(img), w, h, img.strides[0], ch, int(nfeatures), float(scaleFactor),
                                   int(nlevels), int(fastThreshold), int(scoreType), ptr(kps), cap, ctypes.byref(n),
                                   ptr(desc) if desc is not None else None)
        if rc == L.SLAM_E_CAPACITY and n.value > cap:
            cap = n.value
            continue
        check(rc, c)
        return kps[:n.value].copy(), (desc[:n.value].copy() if desc is not None else None)


class OrbBatch(SiftBatch):
    """orbDetectAndComputeBatch's result: SiftBatch with (n, cap, 32) uint8 descriptors"""


def orbDetectAndComputeBatch(frames, nfeatures=500, scaleFactor=1.2, nlevels=8, fastThreshold=20,
                             scoreType=L.HARRIS_SCORE, ctx=None, with_descriptors=True, cap=None):
    """orbDetectAndCompute over a device-resident batch: frames is a CUDA uint8
    tensor (n, h, w, 3 or 4) or (n, h, w) already in HBM (slam_orb_detect_batch;
    every kernel launch covers one pyramid level of the batch).  Keypoints and
    descriptors stay in device memory: returns an OrbBatch (OrbBatch.host(f)
    gives frame f's (kps, desc) as orbDetectAndCompute returns them)."""
    import torch
    c = _ctx(ctx)
    if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() in (3, 4)):
        raise ValueError("frames: a CUDA uint8 tensor (n, h, w[, 3 or 4])")
    frames = frames.contiguous()
    n, h, w = frames.shape[:3]
    ch = frames.shape[3] if frames.dim() == 4 else 1
    torch.cuda.current_stream(frames.device).synchronize()   # the library's stream reads the frames next
    cap = int(cap) if cap is not None else max(1024, 2 * int(nfeatures) + 256)
    while True:
        kps = torch.empty((n, cap, KEYPOINT_DTYPE.itemsize), dtype=torch.uint8, device=frames.device)
        desc = torch.empty((n, cap, 32), dtype=torch.uint8, device=frames.device) if with_descriptors else None
        cnt = np.zeros(n, np.int32)
        rc = lib().slam_orb_detect_batch(c, None, ctypes.c_void_p(frames.data_ptr()), n, w, h, ch, int(nfeatures),
                                         float(scaleFactor), int(nlevels), int(fastThreshold), int(scoreType),
                                         ctypes.c_void_p(kps.data_ptr()), cap, ptr(cnt),
                                         ctypes.c_void_p(desc.data_ptr()) if desc is not None else None)
        if rc == L.SLAM_E_CAPACITY and n and int(cnt.max()) > cap:
            cap = int(cnt.max())
            continue
        check(rc, c)
        return OrbBatch(kps, desc, cnt)


def reconstruct(calibration, rotation1, transition1, rotation2, transition2, points1, points2, ctx=None):
    """triangulate.cpp:74-100 reconstruct(): DLT triangulation of matched
    points (Point2f, n x 2) seen from two cameras [R | t] with intrinsics K.
    Returns spatialPoints as an n x 3 float64 array (Point3d)."""
    c = _ctx(ctx)
    K = np.ascontiguousarray(calibration, np.float64).reshape(3, 3)
    R1 = np.ascontiguousarray(rotation1, np.float64).reshape(3, 3)
    R2 = np.ascontiguousarray(rotation2, np.float64).reshape(3, 3)
    t1 = np.ascontiguousarray(transition1, np.float64).reshape(3)
    t2 = np.ascontiguousarray(transition2, np.float64).reshape(3)
    p1 = np.ascontiguousarray(points1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(points2, np.float32).reshape(-1, 2)
    if len(p1) != len(p2):
        raise ValueError("points1 and points2 differ in length")
    out = np.zeros((max(len(p1), 1), 3), np.float64)
    check(lib().slam_reconstruct(c, ptr(K), ptr(R1), ptr(t1), ptr(R2), ptr(t2), ptr(p1), ptr(p2), len(p1),
                                 ptr(out)), c)
    return out[:len(p1)].copy()


def estimateTransformation(points1, points2, calibrationMatrix, useRANSAC=True, RANSACProb=0.999,
                           RANSACThreshold=5.0, distanceThreshold=200.0, ctx=None):
    """cameraTranslation.cpp:32-69 estimateTransformation(): findEssentialMat
    (RANSAC) + recoverPose on matched points (n x 2).  The config keys
    RPUseRANSAC / RPRANSACProb / RPRANSACThreshold / RPDistanceThreshold are
    the keyword arguments.  Returns (ok, R 3x3, t 3, chiralityMask, ransacMask)."""
    c = _ctx(ctx)
    p1 = np.ascontiguousarray(points1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(points2, np.float32).reshape(-1, 2)
    if len(p1) != len(p2):
        raise ValueError("points1 and points2 differ in length")
    n = len(p1)
    K = np.ascontiguousarray(calibrationMatrix, np.float64).reshape(3, 3)
    R = np.zeros((3, 3))
    t = np.zeros(3)
    cm = np.zeros(max(n, 1), np.uint8)
    rm = np.zeros(max(n, 1), np.uint8)
    passed = ctypes.c_int(0)
    check(lib().slam_estimate_transformation(c, ptr(p1), ptr(p2), n, ptr(K), int(bool(useRANSAC)),
                                             float(RANSACProb), float(RANSACThreshold), float(distanceThreshold),
                                             ptr(R), ptr(t), ptr(cm), ptr(rm), ctypes.byref(passed)), c)
    return passed.value > 0, R, t, cm[:n].copy(), rm[:n].copy()


def solvePnPRansac(objectPoints, imagePoints, cameraMatrix, distCoeffs=None, iterationsCount=100,
                   reprojectionError=8.0, confidence=0.99, ctx=None):
    """mainCycle.cpp:155-161 solvePnPRansac(objectPoints, imagePoints,
    calibrationMatrix, distortionCoeffs, rvec, tvec) with OpenCV's defaults:
    EPnP RANSAC + SOLVEPNP_ITERATIVE refinement on the inliers.  Returns
    (retval, rvec (3, 1), tvec (3, 1), inliers (k, 1) int32 or None) as cv2
    does.  distCoeffs must be empty / zero (the reference never sets it)."""
    if distCoeffs is not None and np.any(np.asarray(distCoeffs, np.float64) != 0):
        raise ValueError("solvePnPRansac: only zero distortion is supported (the reference passes an empty Mat)")
    c = _ctx(ctx)
    op = np.ascontiguousarray(objectPoints, np.float32).reshape(-1, 3)
    ip = np.ascontiguousarray(imagePoints, np.float32).reshape(-1, 2)
    if len(op) != len(ip):
        raise ValueError("objectPoints and imagePoints differ in length")
    n = len(op)
    K = np.ascontiguousarray(cameraMatrix, np.float64).reshape(3, 3)
    rvec = np.zeros(3)
    tvec = np.zeros(3)
    mask = np.zeros(max(n, 1), np.uint8)
    ninl = ctypes.c_int(0)
    found = ctypes.c_int(0)
    check(lib().slam_solve_pnp_ransac(c, ptr(op), ptr(ip), n, ptr(K), int(iterationsCount), float(reprojectionError),
                                      float(confidence), ptr(rvec), ptr(tvec), ptr(mask), ctypes.byref(ninl),
                                      ctypes.byref(found)), c)
    inl = np.flatnonzero(mask[:n]).astype(np.int32).reshape(-1, 1) if found.value else None
    return bool(found.value), rvec.reshape(3, 1), tvec.reshape(3, 1), inl


def _desc_arg(desc, t):
    if t == L.ORB_BF:
        return np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    return np.ascontiguousarray(desc, np.float32).reshape(-1, 128)


def knnMatch2(queryDescriptors, trainDescriptors, matcherType, norm=L.NORM_DEFAULT, ctx=None):
    """DescriptorMatcher::knnMatch(query, train, k = 2): (idx nq x 2, dist nq x 2)."""
    _check_type(matcherType)
    c = _ctx(ctx)
    q, t = _desc_arg(queryDescriptors, matcherType), _desc_arg(trainDescriptors, matcherType)
    idx = np.zeros((len(q), 2), np.int32)
    dist = np.zeros((len(q), 2), np.float32)
    if len(q):
        check(lib().slam_knn2(c, ptr(q), len(q), ptr(t), len(t), int(matcherType), int(norm), ptr(idx), ptr(dist)), c)
    return idx, dist


def lastKnnLaunch(ctx=None):
    """(mode, tsplit, variant) of the context's last kNN launch (slam_last_knn_launch):
    L.KNN_MODE_*, the train-set split count, L.KNN_VARIANT_* (| L.KNN_VARIANT_XCD)."""
    c = _ctx(ctx)
    mode, tsplit, variant = ctypes.c_int(-1), ctypes.c_int(0), ctypes.c_int(0)
    check(lib().slam_last_knn_launch(c, ctypes.byref(mode), ctypes.byref(tsplit), ctypes.byref(variant)), c)
    return mode.value, tsplit.value, variant.value


def lastSiftDetectForms(ctx=None):
    """(forms, refine_blocks) of the context's last SIFT detector call
    (slam_last_sift_detect_forms): L.SD_FORM_* bits and sd_refine's grid size."""
    c = _ctx(ctx)
    forms, blocks = ctypes.c_int(-1), ctypes.c_int(0)
    check(lib().slam_last_sift_detect_forms(c, ctypes.byref(forms), ctypes.byref(blocks)), c)
    return forms.value, blocks.value


def getGoodMatches(idx, dist, knnMatcherDistance):
    """featureMatchingCommon.cpp:37-50 on knnMatch2 output (query order)."""
    ok = (idx[:, 0] >= 0) & (idx[:, 1] >= 0)
    ok &= dist[:, 0].astype(np.float64) < knnMatcherDistance * dist[:, 1].astype(np.float64)
    q = np.nonzero(ok)[0]
    out = np.zeros(len(q), DMATCH_DTYPE)
    out["queryIdx"] = q
    out["trainIdx"] = idx[q, 0]
    out["distance"] = dist[q, 0]
    return out


def matchFeatures(prevDesc, curDesc, extractorType, knnMatcherDistance, norm=L.NORM_DEFAULT, ctx=None):
    """knnMatch(prev = query, cur = train, 2) + getGoodMatches, fused on the GPU."""
    _check_type(extractorType)
    c = _ctx(ctx)
    q, t = _desc_arg(prevDesc, extractorType), _desc_arg(curDesc, extractorType)
    cap = max(len(q), 1)
    out = np.zeros(cap, DMATCH_DTYPE)
    n = ctypes.c_int(0)
    check(lib().slam_match(c, ptr(q), len(q), ptr(t), len(t), int(extractorType), int(norm),
                           float(knnMatcherDistance), ptr(out), cap, ctypes.byref(n)), c)
    return out[:n.value].copy()


def matchFramesPairFeatures(firstFrameDescriptor, secondFrame, secondFeatures, matcherType, knnMatcherDistance,
                            norm=L.NORM_DEFAULT, ctx=None):
    """featureMatchingCPU.cpp:83-95: describe the candidate, then match against the
    previous frame's descriptors.  Returns (secondFeatures, matches)."""
    _check_type(matcherType)
    kps, desc = extractDescriptor(secondFrame, secondFeatures, matcherType, ctx=ctx)
    if len(firstFrameDescriptor) == 0 or len(kps) == 0:
        return kps, np.zeros(0, DMATCH_DTYPE)
    return kps, matchFeatures(firstFrameDescriptor, desc, matcherType, knnMatcherDistance, norm=norm, ctx=ctx)


def selectGoodFrame(match_counts, requiredMatchedPointsCount, skipFramesFromBatchHead, useFirstFitInBatch):
    """batch.cpp:136-146 / :280-316 selection rule (index or FRAME_NOT_FOUND)."""
    a = np.ascontiguousarray(match_counts, np.int32)
    return lib().slam_select_good(ptr(a), len(a), int(requiredMatchedPointsCount), int(skipFramesFromBatchHead),
                                  int(bool(useFirstFitInBatch)))


# ---- bundle adjustment -------------------------------------------------------

def rodrigues_to_vector(R):
    """cv::Rodrigues(3x3 -> 3x1) (cvRodrigues2 restated, host code in
    libslamhip), as used by convertDataForBA (bundleAdjustment.cpp:167)."""
    src = np.ascontiguousarray(R, np.float64).reshape(9).copy()
    out = np.zeros(3)
    check(lib().slam_rodrigues(ptr(src), 9, ptr(out)))
    return out


def rodrigues_to_matrix(r):
    """cv::Rodrigues(3x1 -> 3x3) (cvRodrigues2 restated, host code in
    libslamhip), as used by convertDataFromBA (bundleAdjustment.cpp:195) and
    after solvePnPRansac (mainCycle.cpp:162)."""
    src = np.ascontiguousarray(r, np.float64).reshape(3).copy()
    out = np.zeros(9)
    check(lib().slam_rodrigues(ptr(src), 3, ptr(out)))
    return out.reshape(3, 3)


def loss_from_config(config):
    """getLossFunction (bundleAdjustment.cpp:131-151): priority
    Trivial > Huber > Cauchy > Arctan > Tukey > none."""
    g = config.getValue
    if g("BAUseTrivialLossFunction"):
        return L.LOSS_TRIVIAL, 0.0
    for flag, par, kind in (("BAUseHuberLossFunction", "BAHuberLossFunctionParameter", L.LOSS_HUBER),
                            ("BAUseCauchyLossFunction", "BACauchyLossFunctionParameter", L.LOSS_CAUCHY),
                            ("BAUseArctanLossFunction", "BAArctanLossFunctionParameter", L.LOSS_ARCTAN),
                            ("BAUseTukeyLossFunction", "BATukeyLossFunctionParameter", L.LOSS_TUKEY)):
        if g(flag):
            return kind, float(g(par))
    return L.LOSS_NONE, 0.0


def bundle_adjust_arrays(K4, ext6, pts3, obs_frame, obs_point, obs_xy, loss=L.LOSS_NONE, loss_param=0.0,
                         max_iters=50, ctx=None):
    """slam_ba on plain arrays; K4, ext6 (nf x 6), pts3 (np x 3) are updated IN PLACE."""
    c = _ctx(ctx)
    for a in (K4, ext6, pts3):
        if a.dtype != np.float64 or not a.flags.c_contiguous:
            raise TypeError("BA parameter arrays must be C-contiguous float64")
    of = np.ascontiguousarray(obs_frame, np.int32)
    op = np.ascontiguousarray(obs_point, np.int32)
    oxy = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2)
    s = L.BASummary()
    check(lib().slam_ba(c, ptr(K4), ext6.shape[0], ptr(ext6), pts3.shape[0], ptr(pts3), len(of), ptr(of), ptr(op),
                        ptr(oxy), int(loss), float(loss_param), int(max_iters), ctypes.byref(s)), c)
    return s


class TemporalImageData:
    """mainCycleStructures.h:38-45 (the fields BA reads and writes)."""

    def __init__(self, allExtractedFeatures, correspondSpatialPointIdx, rotation, motion):
        self.allExtractedFeatures = allExtractedFeatures
        self.correspondSpatialPointIdx = np.asarray(correspondSpatialPointIdx, np.int64)
        self.rotation = np.asarray(rotation, np.float64)
        self.motion = np.asarray(motion, np.float64).reshape(3, 1)


class GlobalData:
    """mainCycleStructures.h:49-54 (spatialPoints as an N x 3 float64 array)."""

    def __init__(self, spatialPoints):
        self.spatialPoints = np.ascontiguousarray(spatialPoints, np.float64)


def bundleAdjustment(calibrationMatrix, imagesDataForAdjustment, globalData, config, ctx=None):
    """bundleAdjustment.cpp:73-129: builds the observation list in the reference's
    AddResidualBlock order (frame, then keypoint), solves, writes K, R, t and the
    points back in place.  Returns the summary (RMSE as logged at :125-126)."""
    K = calibrationMatrix
    K4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float64)
    ext = np.zeros((len(imagesDataForAdjustment), 6), np.float64)
    of, op, oxy = [], [], []
    for i, im in enumerate(imagesDataForAdjustment):
        ext[i, :3] = rodrigues_to_vector(im.rotation)
        ext[i, 3:] = im.motion.reshape(3)
        kps = im.allExtractedFeatures
        for p, idx in enumerate(im.correspondSpatialPointIdx):
            if idx < 0:
                continue
            of.append(i)
            op.append(int(idx))
            oxy.append((float(kps[p]["x"]), float(kps[p]["y"])))
    loss, par = loss_from_config(config)
    pts = globalData.spatialPoints
    summary = bundle_adjust_arrays(K4, ext, pts, np.array(of, np.int32), np.array(op, np.int32),
                                   np.array(oxy, np.float64).reshape(-1, 2), loss, par, ctx=ctx)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = K4
    for i, im in enumerate(imagesDataForAdjustment):
        im.rotation[...] = rodrigues_to_matrix(ext[i, :3])
        im.motion[...] = ext[i, 3:].reshape(3, 1)
    return summary


def ba_rmse(summary):
    """the reference's logged 'RMSE' = sqrt(cost / num_residuals) (:125-126)."""
    if summary.num_residuals == 0:
        return 0.0
    return math.sqrt(summary.initial_cost / summary.num_residuals), math.sqrt(summary.final_cost / summary.num_residuals)


# ---- scene post-processing (src/vizualization) ---------------------------------------

def cluster_params(config_or_params):
    """(max, euclid weight, colour weight) as the reference reads them
    (geomAdditionalFunc.cpp:114-117, getValue<float>): from a config object with
    getValue, or a (max, euclid_weight, color_weight) triple.  Rounded to f32."""
    g = getattr(config_or_params, "getValue", None)
    if g is not None:
        t = (g("TriangleMaxDistance"), g("TriangleEuclidDistanceWeight"), g("TriangleColorDistance"))
    else:
        t = tuple(config_or_params)
        if len(t) != 3:
            raise ValueError("params are (max_distance, euclid_weight, color_weight)")
    return tuple(float(np.float32(v)) for v in t)


def _cloud(points, colors):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    if len(p) != len(c):
        raise ValueError("points and colors differ in length")
    return p, c


def components_from_labels(labels):
    """label classes as a list of int32 index arrays, ordered by label (= by
    smallest member), members ascending"""
    labels = np.asarray(labels, np.int32)
    if len(labels) == 0:
        return []
    order = np.argsort(labels, kind="stable").astype(np.int32)
    cuts = np.nonzero(np.diff(labels[order]))[0] + 1
    return np.split(order, cuts)


def clusterLabels(points, colors, config_or_params, ctx=None):
    """slam_cluster_points: labels[i] = the smallest index of point i's component"""
    c = _ctx(ctx)
    p, col = _cloud(points, colors)
    mx, dw, cw = cluster_params(config_or_params)
    labels = np.zeros(max(len(p), 1), np.int32)
    nc = ctypes.c_int(0)
    check(lib().slam_cluster_points(c, ptr(p), ptr(col), len(p), mx, dw, cw, ptr(labels), ctypes.byref(nc)), c)
    return labels[:len(p)].copy(), nc.value


def clusterizePoints(points, colors, config_or_params, ctx=None):
    """geomAdditionalFunc.cpp:105-163 clusterizePoints(): the connected
    components of the graph that joins points i and j iff
    distance(p_i, p_j) * TriangleEuclidDistanceWeight + norm(c_i, c_j) *
    TriangleColorDistance < TriangleMaxDistance (points n x 3, narrowed to
    Point3f; colors n x 3 uint8).  Returns comps: a list of int32 index arrays
    ordered by smallest member, which is the reference's order of discovery.
    Members ascend within each array; the reference lists them in DFS
    pre-order, so only the order inside a component differs."""
    labels, nc = clusterLabels(points, colors, config_or_params, ctx)
    comps = components_from_labels(labels)
    assert len(comps) == nc
    return comps


def planeMoments(points, ctx=None):
    """slam_plane_moments: (sum[3], mean[3], {xx, xy, xz, yy, yz, zz} about the
    f64 mean), the deterministic device sums behind getBestFittingPlaneByPoints"""
    c = _ctx(ctx)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    s, mean, mom = np.zeros(3), np.zeros(3), np.zeros(6)
    check(lib().slam_plane_moments(c, ptr(p), len(p), ptr(s), ptr(mean), ptr(mom)), c)
    return s, mean, mom


def getBestFittingPlaneByPoints(points, ctx=None):
    """bestFittingPlane.cpp:11-40: (centroid float32[3], normal float64[3]) of
    the least-squares plane through points (n x 3, Point3f).  The normal is the
    unit eigenvector of the smallest eigenvalue of the centred second-moment
    matrix, its largest-magnitude component positive (the reference's own
    normal is an at<double> read of a CV_32F matrix: DESIGN.md)."""
    c = _ctx(ctx)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    centroid, normal = np.zeros(3, np.float32), np.zeros(3, np.float64)
    check(lib().slam_fit_plane(c, ptr(p), len(p), ptr(centroid), ptr(normal)), c)
    return centroid, normal


def projectToPlane(points, centroid, normal, ctx=None):
    """projectPointOnPlane (geomAdditionalFunc.cpp:20-32) and makeMesh's
    flattening (bestFittingPlane.cpp:51-63) for every point, bit for bit:
    the n x 2 float32 (x, z) points the Delaunay step consumes."""
    c = _ctx(ctx)
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    cen = np.ascontiguousarray(centroid, np.float32).reshape(3)
    nrm = np.ascontiguousarray(normal, np.float64).reshape(3)
    out = np.zeros((max(len(p), 1), 2), np.float32)
    check(lib().slam_project_to_plane(c, ptr(p), len(p), ptr(cen), ptr(nrm), ptr(out)), c)
    return out[:len(p)].copy()


MESH_MAX_SIZE = 10000.0      # makeMesh's max_size (bestFittingPlane.cpp:89)


def delaunay2d(xy, ctx=None):
    """builtInTriangulation (bowyerWatson.cpp:86-105) with makeMesh's corner
    lookup (bestFittingPlane.cpp:67-95): the Delaunay triangulation of the n x 2
    float32 points as a (T, 3) int32 array of point indices, each row starting
    at its smallest index, counter-clockwise, rows sorted (slam_delaunay_2d has
    the contract).  A coordinate that is not finite or outside [-100000, 100000),
    where the reference's Subdiv2D throws, raises SlamError with
    SLAM_E_INVALID_ARG."""
    c = _ctx(ctx)
    p = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    cap = max(2 * len(p) - 5, 1)
    tris = np.zeros((cap, 3), np.int32)
    nt = ctypes.c_int(0)
    check(lib().slam_delaunay_2d(c, ptr(p), len(p), ptr(tris), cap, ctypes.byref(nt)), c)
    return tris[:nt.value].copy()


DELAUNAY_HOST_BELOW = 64     # SLAM_DELAUNAY_HOST_BELOW


def delaunay2dHost(xy):
    """slam_delaunay_2d_host: delaunay2d's contract evaluated on the host (the
    same exact predicates and tie rule; no context, no device).  For inputs of
    a few dozen points, where a launch costs more than the triangulation."""
    p = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    cap = max(2 * len(p) - 5, 1)
    tris = np.zeros((cap, 3), np.int32)
    nt = ctypes.c_int(0)
    rc = lib().slam_delaunay_2d_host(ptr(p), len(p), ptr(tris), cap, ctypes.byref(nt))
    if rc != L.SLAM_OK:
        raise L.SlamError(rc, "slam_delaunay_2d_host: a coordinate is not finite or outside [-100000, 100000)"
                          if rc == L.SLAM_E_INVALID_ARG else "slam_delaunay_2d_host")
    return tris[:nt.value].copy()


def delaunayStats(ctx=None):
    """slam_delaunay_last_stats: (predicates, exact-path predicates, tie passes)
    of the context's last Delaunay call"""
    c = _ctx(ctx)
    v = [ctypes.c_uint64(0) for _ in range(3)]
    check(lib().slam_delaunay_last_stats(c, *[ctypes.byref(x) for x in v]), c)
    return tuple(int(x.value) for x in v)


def delaunayPredicates(kinds, vals, ctx=None):
    """slam_delaunay_predicates: the star kernel's orient ('o'), incircle ('i')
    and closer ('c') evaluated on the device, one case per row of vals (n x 8
    float32; 'o' and 'c' read the first six).  kinds is a str or bytes of n
    letters.  Returns (filter_sign, sign), int8[n]: the f64 filter's answer
    alone (2 = undecided) and the exact sign."""
    c = _ctx(ctx)
    k = np.frombuffer(kinds.encode() if isinstance(kinds, str) else bytes(kinds), np.uint8).copy()
    v = np.ascontiguousarray(vals, np.float32).reshape(-1, 8)
    if len(k) != len(v):
        raise ValueError("delaunayPredicates: one kind per row of vals")
    n = len(k)
    fs, s = np.zeros(max(n, 1), np.int8), np.zeros(max(n, 1), np.int8)
    if n == 0:
        k, v = np.zeros(1, np.uint8), np.zeros((1, 8), np.float32)
    check(lib().slam_delaunay_predicates(c, ptr(k), ptr(v), n, ptr(fs), ptr(s)), c)
    return fs[:n].copy(), s[:n].copy()


def meshFilter(points, tris, max_size=MESH_MAX_SIZE):
    """makeMesh's filter (bestFittingPlane.cpp:96-114): the triangles (T, 3)
    none of whose 3-D edges between points (n x 3, Point3f) is longer than
    max_size, in order.  Host code; needs no device."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    out = np.zeros((max(len(t), 1), 3), np.int32)
    kept = ctypes.c_int(0)
    check(lib().slam_mesh_filter(ptr(p), len(p), ptr(t), len(t), float(max_size), ptr(out), ctypes.byref(kept)))
    return out[:kept.value].copy()


# ---- calibration file and undistortion (the batch.cpp:244 seam) ----------------

def calibration_model(path):
    """the lens model a calibration file names: the text of its string node
    <model> ("fisheye": DC holds k1 k2 k3 k4 of cv::fisheye), or None for a file
    without the node, which is the Brown-Conrady polynomial as the reference
    writes it (DC: k1 k2 p1 p2 k3)"""
    import xml.etree.ElementTree as ET
    node = ET.parse(path).getroot().find("model")
    if node is None:
        return None
    name = (node.text or "").strip().strip('"')
    if name != "fisheye":
        raise ValueError(f"{path}: unknown lens model {name!r}")
    return name


def load_calibration(path, key="K", model=None):
    """loadMatrixFromXML (IOmisc.cpp:80-88): the matrix `key` of an OpenCV XML
    storage as float64.  load_calibration(path) is the camera matrix K that
    defineCalibrationMatrix reads; "DC" the distortion coefficients that
    saveCalibParametersToXML writes beside it (IOmisc.cpp:68-76).  Reads
    opencv-matrix nodes of doubles: <dt> "d", or "<n>d" for n channels, which
    become n columns per element (R, 13x1 of "3d": 13 x 3).  A missing key raises
    KeyError.  model: the lens model the caller reads the coefficients for, None
    (the polynomial) or "fisheye"; "DC" of a file that names another model
    (calibration_model) raises ValueError, so that four fisheye coefficients are
    never taken for k1 k2 p1 p2 or the reverse."""
    import xml.etree.ElementTree as ET
    if key == "DC" and calibration_model(path) != model:
        raise ValueError(f"{path}: the coefficients are of lens model {calibration_model(path)!r}, not {model!r}")
    node = ET.parse(path).getroot().find(key)
    if node is None:
        raise KeyError(f"{path}: no matrix {key!r}")
    if node.get("type_id") != "opencv-matrix":
        raise ValueError(f"{path}: {key!r} is not an opencv-matrix")
    rows, cols = int(node.findtext("rows")), int(node.findtext("cols"))
    dt = node.findtext("dt").strip().strip('"')
    if not dt.endswith("d") or (dt[:-1] and not dt[:-1].isdigit()):
        raise ValueError(f"{path}: {key!r} has element type {dt!r}; only doubles are read")
    ch = int(dt[:-1]) if dt[:-1] else 1
    data = np.array([float(v) for v in node.findtext("data").split()], np.float64)
    if data.size != rows * cols * ch:
        raise ValueError(f"{path}: {key!r} holds {data.size} values, not {rows}x{cols}x{ch}")
    return data.reshape(rows, cols * ch)


def _camera(K, dist, newK):
    K = np.ascontiguousarray(K, np.float64).reshape(-1)
    if K.size != 9:
        raise ValueError("K is 3x3")
    d = np.ascontiguousarray(dist, np.float64).reshape(-1)
    n = None
    if newK is not None:
        n = np.ascontiguousarray(newK, np.float64).reshape(-1)
        if n.size != 9:
            raise ValueError("newK is 3x3")
    return K, d, n


def _entry(name, fisheye):
    """the C entry `slam_<name>` of the Brown-Conrady model, or its fisheye twin"""
    return getattr(lib(), ("slam_fisheye_" if fisheye else "slam_") + name)


def undistortMap(w, h, K, dist, newK=None, ctx=None):
    """the fixed-point map of cv::undistort(src, dst, K, dist, newK) for w x h
    frames (slam_undistort_map): xy (h, w, 2) int16 source x, y and frac (h, w)
    uint16, (fy << 5) | fx.  Built on the device, cached in the context."""
    return _undistortMap(False, w, h, K, dist, newK, ctx)


def _undistortMap(fisheye, w, h, K, dist, newK, ctx):
    """undistortMap, or its twin for the fisheye lens model"""
    c = _ctx(ctx)
    K, d, n = _camera(K, dist, newK)
    xy = np.empty((h, w, 2), np.int16)
    frac = np.empty((h, w), np.uint16)
    check(_entry("undistort_map", fisheye)(c, int(w), int(h), ptr(K), ptr(d), d.size, ptr(n), ptr(xy), ptr(frac)), c)
    return xy, frac


def undistort(frame, K, dist, newK=None, ctx=None):
    """cv::undistort(frame, out, K, dist, newK) of an 8-bit gray or BGR frame in
    host memory (slam_undistort); the seam the reference marks at batch.cpp:244.
    Rows may be strided (a column range of a wider image)."""
    return _undistort(False, frame, K, dist, newK, ctx)


def _undistort(fisheye, frame, K, dist, newK, ctx):
    """undistort, or its twin for the fisheye lens model"""
    c = _ctx(ctx)
    a = np.asarray(frame)
    if a.dtype != np.uint8:
        raise TypeError("frames are 8-bit (CV_8UC1/3)")
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError("frame must be HxW or HxWx3 (BGR)")
    ch = 1 if a.ndim == 2 else 3
    if a.strides[1:] != ((1,) if ch == 1 else (3, 1)) or a.strides[0] < a.shape[1] * ch:
        a = np.ascontiguousarray(a)
    K, d, n = _camera(K, dist, newK)
    out = np.empty(a.shape, np.uint8)
    h, w = a.shape[:2]
    check(_entry("undistort", fisheye)(c, ptr(a), w, h, a.strides[0], ch, ptr(K), ptr(d), d.size, ptr(n), ptr(out),
                                        out.strides[0]), c)
    return out


def undistortBatch(frames, K, dist, newK=None, ctx=None, out=None, stream=None):
    """cv::undistort of n frames resident in HBM in one launch
    (slam_undistort_batch): `frames` a contiguous torch uint8 tensor (n, h, w, 3)
    or (n, h, w); the result goes to `out` (same shape, no overlap) or a new
    tensor.  No host sync.  stream: a HIP stream handle the caller orders
    itself; by default the launch goes to the context's stream, after what
    torch's current stream holds so far (the frames' producer) and before what
    it is given later (the result's consumers), both by device-side waits."""
    return _undistortBatch(False, frames, K, dist, newK, ctx, out, stream)


def _undistortBatch(fisheye, frames, K, dist, newK, ctx, out, stream):
    """undistortBatch, or its twin for the fisheye lens model"""
    import torch
    ctx = ctx or default_context()
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3):
        raise ValueError("frames: uint8 (n, h, w) or (n, h, w, 3)")
    if not frames.is_contiguous():
        frames = frames.contiguous()
    if out is None:
        out = torch.empty_like(frames)
    if not out.is_contiguous() or out.shape != frames.shape or out.dtype != torch.uint8:
        raise ValueError("out: a contiguous uint8 tensor of the frames' shape")
    K, d, n = _camera(K, dist, newK)
    own = stream is None
    if own:
        # torch's current stream may be the legacy default stream, whose handle
        # (NULL) the C ABI reads as "the context's stream": run there, ordered
        # against the current stream on both sides
        cur = torch.cuda.current_stream(frames.device)
        ready = torch.cuda.Event()
        ready.record(cur)
        torch.cuda.ExternalStream(lib().slam_context_stream(ctx.handle), device=frames.device).wait_event(ready)
    nf, h, w = frames.shape[:3]
    check(_entry("undistort_batch", fisheye)(ctx.handle, None if own else stream, ctypes.c_void_p(frames.data_ptr()),
                                              ctypes.c_void_p(out.data_ptr()), int(nf), int(w), int(h),
                                              1 if frames.dim() == 3 else 3, ptr(K), ptr(d), d.size, ptr(n)), ctx.handle)
    if own:
        check(lib().slam_order_after(ctx.handle, ctypes.c_void_p(cur.cuda_stream), None), ctx.handle)
    return out


def undistortPoints(pts_or_keypoints, K, dist, P=None, criteria=(5, 0.0), ctx=None):
    """cv::undistortPoints(src, dst, K, dist, noArray(), P, criteria)
    (slam_undistort_points): the ideal position of distorted image points, for
    the keypoints that reach geometry when the frames stay raw (the
    batch.cpp:244 seam without the frame remap).  pts_or_keypoints: n x 2
    float32 points, or a keypoint record array, whose .pt is read in place.
    P: 3x3 applied to the normalised result (None: normalised coordinates).
    criteria = (max_iter, eps): max_iter in 1..1000; eps == 0 iterates max_iter
    times (OpenCV's default: 5), eps > 0 also stops below eps pixels of
    reprojection error.  Returns (xy float32 n x 2, err float32 n); err is the
    distance in pixels between each input point and the distortion model of its
    result.  A point beyond the fold of the lens model has no preimage: test
    err <= tol before using xy (a NaN fails the test)."""
    return _undistortPoints(False, pts_or_keypoints, K, dist, P, criteria, ctx)


def _undistortPoints(fisheye, pts_or_keypoints, K, dist, P, criteria, ctx):
    """undistortPoints, or its twin for the fisheye lens model"""
    c = _ctx(ctx)
    a = np.asarray(pts_or_keypoints)
    if a.dtype == KEYPOINT_DTYPE:
        a = np.ascontiguousarray(a).reshape(-1)
        stride = KEYPOINT_DTYPE.itemsize
    else:
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 2)
        stride = 8
    K, d, p = _camera(K, dist, P)
    max_iter, eps = criteria
    n = len(a)
    xy = np.empty((n, 2), np.float32)
    err = np.empty(n, np.float32)
    check(_entry("undistort_points", fisheye)(c, ptr(a), stride, n, ptr(K), ptr(d), d.size, ptr(p), int(max_iter),
                                               float(eps), ptr(xy), ptr(err)), c)
    return xy, err


# ---- the fisheye lens model (cv::fisheye) -------------------

def fisheyeUndistortMap(w, h, K, dist, newK=None, ctx=None):
    """undistortMap for the fisheye model (slam_fisheye_undistort_map): the map
    of cv::fisheye::initUndistortRectifyMap(K, dist, I, newK, (w, h), CV_16SC2),
    which cv::fisheye::undistortImage builds.  dist: exactly k1 k2 k3 k4; the last
    row of newK (K when None) is (0, 0, 1)."""
    return _undistortMap(True, w, h, K, dist, newK, ctx)


def fisheyeUndistort(frame, K, dist, newK=None, ctx=None):
    """cv::fisheye::undistortImage(frame, out, K, dist, newK) of a host frame
    (slam_fisheye_undistort); otherwise as undistort"""
    return _undistort(True, frame, K, dist, newK, ctx)


def fisheyeUndistortBatch(frames, K, dist, newK=None, ctx=None, out=None, stream=None):
    """cv::fisheye::undistortImage of n resident frames in one launch
    (slam_fisheye_undistort_batch); otherwise as undistortBatch"""
    return _undistortBatch(True, frames, K, dist, newK, ctx, out, stream)


def fisheyeUndistortPoints(pts_or_keypoints, K, dist, P=None, criteria=(10, 1e-8), ctx=None):
    """cv::fisheye::undistortPoints(src, dst, K, dist, noArray(), P, criteria)
    (slam_fisheye_undistort_points): (xy float32 n x 2, err float32 n).  A point
    that did not converge under an eps criterion, or whose angle changed sign, is
    (-1000000, -1000000) as OpenCV writes it, and its err is NaN; otherwise err
    is the pixel distance between the input and the forward model of the result.
    Arguments as undistortPoints."""
    return _undistortPoints(True, pts_or_keypoints, K, dist, P, criteria, ctx)


# ---- chessboard calibration (the reference's "calibrate" mode) -------------------

def _frame13(frame):
    a = np.asarray(frame)
    if a.dtype != np.uint8:
        raise TypeError("frames are 8-bit (CV_8UC1/3)")
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError("frame must be HxW or HxWx3 (BGR)")
    ch = 1 if a.ndim == 2 else 3
    if a.strides[1:] != ((1,) if ch == 1 else (3, 1)) or a.strides[0] < a.shape[1] * ch:
        a = np.ascontiguousarray(a)
    return a, a.shape[1], a.shape[0], ch


def _resident(frames):
    import torch
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3):
        raise ValueError("frames: uint8 (n, h, w) or (n, h, w, 3)")
    if not frames.is_contiguous():
        frames = frames.contiguous()
    torch.cuda.current_stream(frames.device).synchronize()    # the frames' producer
    return frames, int(frames.shape[0]), int(frames.shape[2]), int(frames.shape[1]), 1 if frames.dim() == 3 else 3


def chessCap(w, h):
    """the most candidates a w x h frame can have: ceil(W / 8) * ceil(H / 8) of its level"""
    s = max(1, -(-max(w, h) // 1024))
    return -(-(w // s) // 8) * -(-(h // s) // 8)


def chessCandidates(frame, ctx=None):
    """chessboard corner candidates (slam_chess_candidates): (cand, s) with cand
    (n, 3) int32 rows (x, y, R) in raster order, in the coordinates of the level
    image: the s x s area mean of the gray frame, s = max(1, ceil(max(w, h) / 1024)).
    R is 80 x the ChESS response; a candidate is the maximum of its 15 x 15 window.
    `frame`: a host array, or a resident torch batch (n, h, w[, 3]) -> a list of n
    arrays from one launch per kernel (slam_chess_candidates_dev)."""
    ctx = ctx or default_context()
    c = ctx.handle
    s = ctypes.c_int(0)
    if not isinstance(frame, np.ndarray) and hasattr(frame, "data_ptr"):
        fr, n, w, h, ch = _resident(frame)
        cap = chessCap(w, h)
        out = np.empty((n, cap, 3), np.int32)
        cnt = np.zeros(n, np.int32)
        check(lib().slam_chess_candidates_dev(c, None, ctypes.c_void_p(fr.data_ptr()), n, w, h, ch, ptr(out), cap,
                                              ptr(cnt), ctypes.byref(s)), c)
        return [out[f, :cnt[f]].copy() for f in range(n)], s.value
    a, w, h, ch = _frame13(frame)
    cap = chessCap(w, h)
    out = np.empty((cap, 3), np.int32)
    n = ctypes.c_int(0)
    check(lib().slam_chess_candidates(c, ptr(a), w, h, a.strides[0], ch, ptr(out), cap, ctypes.byref(n),
                                      ctypes.byref(s)), c)
    return out[:n.value].copy(), s.value


def _labeller(name):
    if name not in ("peel", "grow"):
        raise ValueError('labeller: "peel" or "grow"')
    return lib().slam_label_chessboard_grow if name == "grow" else lib().slam_label_chessboard


def labelChessboard(cand, scale, patternSize, labeller="peel"):
    """slam_label_chessboard (host only): the patternSize[0] * patternSize[1]
    strongest candidates as a complete board -> (found, corners (n, 2) float32 in
    full-resolution pixels, canonical order) or (False, None).  labeller="grow"
    (slam_label_chessboard_grow): a lattice grown among twice as many candidates,
    for boards a fisheye lens bends and scenes with clutter stronger than a corner."""
    label = _labeller(labeller)
    bw, bh = int(patternSize[0]), int(patternSize[1])
    cand = np.ascontiguousarray(cand, np.int32).reshape(-1, 3)
    corners = np.empty((bw * bh, 2), np.float32)
    found = ctypes.c_int(0)
    check(label(ptr(cand), len(cand), int(scale), bw, bh, ptr(corners), ctypes.byref(found)))
    return (True, corners) if found.value else (False, None)


def findChessboardCorners(frame, patternSize, ctx=None, labeller="peel"):
    """findChessboardCorners(gray, patternSize, corners) (cameraCalibration.cpp:168)
    by this library's own detector: (found, corners) with corners (w * h, 2) float32
    in pixels, row-major with rows of patternSize[0], right-handed in image
    coordinates, first corner nearest the image's origin; (False, None) when the
    strongest candidates are not a complete board.  A resident torch batch
    (n, h, w[, 3]) gives a list of n such pairs (slam_find_chessboard_dev).
    labeller="grow": the candidates of chessCandidates labelled by
    labelChessboard(..., labeller="grow")."""
    ctx = ctx or default_context()
    c = ctx.handle
    bw, bh = int(patternSize[0]), int(patternSize[1])
    if labeller != "peel":
        _labeller(labeller)
        cand, s = chessCandidates(frame, ctx=ctx)
        if isinstance(cand, list):
            return [labelChessboard(k, s, patternSize, labeller) for k in cand]
        return labelChessboard(cand, s, patternSize, labeller)
    if not isinstance(frame, np.ndarray) and hasattr(frame, "data_ptr"):
        fr, n, w, h, ch = _resident(frame)
        corners = np.empty((n, bw * bh, 2), np.float32)
        found = np.zeros(n, np.int32)
        check(lib().slam_find_chessboard_dev(c, None, ctypes.c_void_p(fr.data_ptr()), n, w, h, ch, bw, bh, ptr(corners),
                                             ptr(found)), c)
        return [(True, corners[f].copy()) if found[f] else (False, None) for f in range(n)]
    a, w, h, ch = _frame13(frame)
    corners = np.empty((bw * bh, 2), np.float32)
    found = ctypes.c_int(0)
    check(lib().slam_find_chessboard(c, ptr(a), w, h, a.strides[0], ch, bw, bh, ptr(corners), ctypes.byref(found)), c)
    return (True, corners) if found.value else (False, None)


def cornerSubPix(frame, corners, winSize=(11, 11), criteria=(30, 1e-4), zeroZone=(-1, -1), ctx=None):
    """cv::cornerSubPix(gray, corners, winSize, zeroZone, TermCriteria(COUNT + EPS,
    *criteria)) (cameraCalibration.cpp:169) on the device; returns the refined
    (n, 2) float32 corners.  `frame`: a host array or one resident torch frame
    (h, w[, 3]).  Only zeroZone (-1, -1); winSize at most (15, 15)."""
    ctx = ctx or default_context()
    c = ctx.handle
    out = np.array(corners, np.float32).reshape(-1, 2).copy()
    max_iter, eps = criteria
    tail = (len(out), int(winSize[0]), int(winSize[1]), int(zeroZone[0]), int(zeroZone[1]), int(max_iter), float(eps))
    if not isinstance(frame, np.ndarray) and hasattr(frame, "data_ptr"):
        fr, _, w, h, ch = _resident(frame[None])
        check(lib().slam_corner_subpix_dev(c, None, ctypes.c_void_p(fr.data_ptr()), w, h, w * ch, ch, ptr(out), *tail), c)
        return out
    a, w, h, ch = _frame13(frame)
    check(lib().slam_corner_subpix(c, ptr(a), w, h, a.strides[0], ch, ptr(out), *tail), c)
    return out


def _frame134(frame):
    a = np.asarray(frame)
    if a.dtype != np.uint8:
        raise TypeError("frames are 8-bit (CV_8UC1/3/4)")
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (3, 4)):
        raise ValueError("frame must be HxW, HxWx3 (BGR) or HxWx4")
    ch = 1 if a.ndim == 2 else a.shape[2]
    if a.strides[1:] != ((1,) if ch == 1 else (ch, 1)) or a.strides[0] < a.shape[1] * ch:
        a = np.ascontiguousarray(a)
    return a, a.shape[1], a.shape[0], ch


def kltLevelSizes(w, h, winSize, maxLevel):
    """the (w, h) of the levels cv::buildOpticalFlowPyramid builds: level 0, then
    halves ((w + 1) / 2, (h + 1) / 2) up to maxLevel while larger than the window"""
    out = [(int(w), int(h))]
    while len(out) <= maxLevel:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= winSize[0] or h <= winSize[1]:
            break
        out.append((w, h))
    return out


def buildOpticalFlowPyramid(img, winSize, maxLevel, withDerivatives=True, ctx=None):
    """cv::buildOpticalFlowPyramid(img, pyramid, winSize, maxLevel, withDerivatives)
    on the device (slam_klt_pyramid): (nlevels, levels, derivs) with levels a list
    of unpadded uint8 (h, w) gray levels (level 0 is the gray image; 3 / 4 channels
    go through BGR2GRAY) and derivs the int16 (h, w, 2) {Ix, Iy} planes of
    calcScharrDeriv per level (None without withDerivatives).  nlevels is the
    number of levels built: maxLevel + 1, or fewer when the next level would be no
    larger than the window."""
    ctx = ctx or default_context()
    c = ctx.handle
    a, w, h, ch = _frame134(img)
    sizes = kltLevelSizes(w, h, winSize, max(int(maxLevel), 0))
    px = sum(x * y for x, y in sizes)
    gray = np.empty(px, np.uint8)
    deriv = np.empty((px, 2), np.int16) if withDerivatives else None
    out_sizes = np.zeros((L.KLT_MAX_LEVELS, 2), np.int32)
    nl = ctypes.c_int(0)
    need = ctypes.c_size_t(0)
    check(lib().slam_klt_pyramid(c, ptr(a), w, h, a.strides[0], ch, int(winSize[0]), int(winSize[1]), int(maxLevel),
                                 ctypes.byref(nl), ptr(out_sizes), ptr(gray), ptr(deriv), px, ctypes.byref(need)), c)
    levels, derivs, off = [], [], 0
    for lw, lh in out_sizes[:nl.value]:
        levels.append(gray[off:off + lw * lh].reshape(lh, lw).copy())
        if withDerivatives:
            derivs.append(deriv[off:off + lw * lh].reshape(lh, lw, 2).copy())
        off += lw * lh
    return nl.value, levels, (derivs if withDerivatives else None)


def _klt_tail(winSize, maxLevel, criteria, flags, minEigThreshold):
    return (int(winSize[0]), int(winSize[1]), int(maxLevel), int(criteria[0]), float(criteria[1]), int(flags),
            float(minEigThreshold))


def calcOpticalFlowPyrLK(prev, next, prevPts, nextPts=None, winSize=(21, 21), maxLevel=3, criteria=(30, 0.01), flags=0,
                         minEigThreshold=1e-4, ctx=None):
    """cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err, winSize,
    maxLevel, TermCriteria(COUNT + EPS, *criteria), flags, minEigThreshold) on the
    device: (nextPts (n, 2) float32, status (n,) uint8, err (n,) float32).  prev /
    next: two host frames of one size (slam_klt_track) or two resident torch frames
    (h, w[, 3]) (slam_klt_track_dev).  flags: L.KLT_USE_INITIAL_FLOW (nextPts holds
    the initial positions) | L.KLT_GET_MIN_EIGENVALS.  winSize 3..31 per axis,
    maxLevel 0..8."""
    ctx = ctx or default_context()
    c = ctx.handle
    pts = np.ascontiguousarray(np.asarray(prevPts, np.float32).reshape(-1, 2))
    n = len(pts)
    if int(flags) & L.KLT_USE_INITIAL_FLOW:
        if nextPts is None or np.size(nextPts) != 2 * n:
            raise ValueError("USE_INITIAL_FLOW: one initial position per point")
        out = np.array(nextPts, np.float32).reshape(-1, 2).copy()
    else:
        out = np.zeros((n, 2), np.float32)
    status = np.ones(n, np.uint8)
    err = np.zeros(n, np.float32)
    tail = _klt_tail(winSize, maxLevel, criteria, flags, minEigThreshold)
    if not isinstance(prev, np.ndarray) and hasattr(prev, "data_ptr"):
        fr, _, w, h, ch = _resident(prev[None])
        nx, _, w2, h2, ch2 = _resident(next[None])
        if (w, h, ch) != (w2, h2, ch2):
            raise ValueError("frames of one size")
        check(lib().slam_klt_track_dev(c, None, ctypes.c_void_p(fr.data_ptr()), ctypes.c_void_p(nx.data_ptr()), w, h,
                                       w * ch, ch, ptr(pts), n, ptr(out), ptr(status), ptr(err), *tail), c)
        return out, status, err
    a, w, h, ch = _frame134(prev)
    b, w2, h2, ch2 = _frame134(next)
    if (w, h, ch) != (w2, h2, ch2):
        raise ValueError("frames of one size")
    check(lib().slam_klt_track(c, ptr(a), a.strides[0], ptr(b), b.strides[0], w, h, ch, ptr(pts), n, ptr(out),
                               ptr(status), ptr(err), *tail), c)
    return out, status, err


def calibrateCamera(objectPoints, imagePoints, imageSize):
    """calibrateCamera(objectPoints, imagePoints, imageSize, K, D, R, T) with default
    flags (cameraCalibration.cpp:196), on the host in f64: the optimum of the
    reprojection error over fx fy cx cy, k1 k2 p1 p2 k3 and a pose per view (not
    OpenCV's iterate after 30 steps).  objectPoints: (npts, 3) with z = 0, one
    board for all views; imagePoints: (nviews, npts, 2); imageSize (width, height)
    only places the initial principal point.  Returns (rms, K 3x3, D (5,), rvecs
    (nviews, 3), tvecs (nviews, 3))."""
    return _calibrateCamera(False, objectPoints, imagePoints, imageSize)


def _calibrateCamera(fisheye, objectPoints, imagePoints, imageSize):
    """calibrateCamera, or its twin for the fisheye lens model"""
    obj = np.ascontiguousarray(objectPoints, np.float32)
    if obj.ndim == 3:
        if any(not np.array_equal(o, obj[0]) for o in obj):
            raise ValueError("one board for all views")
        obj = np.ascontiguousarray(obj[0])
    img = np.ascontiguousarray(imagePoints, np.float32)
    if obj.ndim != 2 or obj.shape[1] != 3 or img.ndim != 3 or img.shape[1:] != (len(obj), 2):
        raise ValueError("objectPoints (npts, 3), imagePoints (nviews, npts, 2)")
    nv = len(img)
    K, D = np.zeros((3, 3)), np.zeros(4 if fisheye else 5)
    rv, tv = np.zeros((nv, 3)), np.zeros((nv, 3))
    rms = ctypes.c_double(0)
    it = ctypes.c_int(0)
    solve = lib().slam_fisheye_calibrate if fisheye else lib().slam_calibrate_camera
    check(solve(ptr(obj), ptr(img), nv, len(obj), int(imageSize[0]), int(imageSize[1]), ptr(K), ptr(D), ptr(rv), ptr(tv),
                ctypes.byref(rms), ctypes.byref(it)))
    return rms.value, K, D, rv, tv


def fisheyeCalibrate(objectPoints, imagePoints, imageSize):
    """cv::fisheye::calibrate(objectPoints, imagePoints, imageSize, K, D, R, T) with
    the skew fixed at 0 (slam_fisheye_calibrate), on the host in f64: the optimum
    over fx fy cx cy, k1 k2 k3 k4 and a pose per view.  Arguments and result as
    calibrateCamera, with D (4,)."""
    return _calibrateCamera(True, objectPoints, imagePoints, imageSize)


def save_calibration(path, K, D, R, T, model=None):
    """saveCalibParametersToXML (IOmisc.cpp:68-76): K 3x3 "d", DC 1x5 "d", R and T
    Nx1 "3d" in OpenCV's XML storage, doubles as %.16e: load_calibration reads each
    key back bit for bit.  model="fisheye": DC is k1 k2 k3 k4 of cv::fisheye and
    the file carries the string node <model>fisheye</model> that says so."""
    def node(name, rows, cols, dt, data):
        vals = " ".join("%.16e" % float(v) for v in np.asarray(data, np.float64).ravel())
        return (f'<{name} type_id="opencv-matrix">\n  <rows>{rows}</rows>\n  <cols>{cols}</cols>\n'
                f'  <dt>{dt}</dt>\n  <data>\n    {vals}</data></{name}>\n')
    K = np.asarray(K, np.float64).reshape(3, 3)
    D = np.asarray(D, np.float64).reshape(-1)
    R = np.asarray(R, np.float64).reshape(-1, 3)
    T = np.asarray(T, np.float64).reshape(-1, 3)
    if len(R) != len(T):
        raise ValueError("one rotation and one translation per view")
    if model not in (None, "fisheye") or (model == "fisheye" and D.size != 4):
        raise ValueError('model: None, or "fisheye" with four coefficients')
    name = "" if model is None else f"<model>{model}</model>\n"
    text = ('<?xml version="1.0"?>\n<opencv_storage>\n' + name + node("K", 3, 3, "d", K) + node("DC", 1, D.size, "d", D) +
            node("R", len(R), 1, '"3d"', R) + node("T", len(T), 1, '"3d"', T) + "</opencv_storage>\n")
    with open(path, "w") as f:
        f.write(text)


SYNTH_DRIFT, SYNTH_STEADY = 0, 1


def synth_frames(w, h, first, count, seed=1234, path=SYNTH_DRIFT):
    """Deterministic synthetic indoor sequence (count x h x w x 3 BGR uint8).
    path: SYNTH_DRIFT (the camera zooms in along the sequence, so the FAST count
    falls with the frame index; the fixtures' path) or SYNTH_STEADY (a bounded
    loop: every frame near frame 0's FAST count; the bench's configs[1] batches)."""
    out = np.zeros((count, h, w, 3), np.uint8)
    check(lib().slam_synth_sequence(w, h, first, count, ctypes.c_uint64(seed), int(path), ptr(out)))
    return out


def synth_frames_dev(w, h, first, count, seed=1234, path=SYNTH_DRIFT, ctx=None, out=None):
    """synth_frames rendered on the device (slam_synth_sequence_dev): a torch
    uint8 tensor (count, h, w, 3) in HBM, byte-identical to synth_frames."""
    import torch
    ctx = ctx or default_context()
    if out is None:
        out = torch.empty((count, h, w, 3), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    assert out.is_contiguous() and tuple(out.shape) == (count, h, w, 3) and out.dtype == torch.uint8
    torch.cuda.current_stream(out.device).synchronize()
    check(lib().slam_synth_sequence_dev(ctx.handle, None, w, h, first, count, ctypes.c_uint64(seed), int(path),
                                        ctypes.c_void_p(out.data_ptr()) if count else None), ctx.handle)
    return out


# ---- JPEG decoding: cv::imread / cv::imdecode on baseline JPEG (jpeg.hip, jpeg_parse.cpp) ----
def _jpeg_bytes(buf):
    if isinstance(buf, (bytes, bytearray, memoryview)):
        return np.frombuffer(buf, np.uint8)
    a = np.ascontiguousarray(buf)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise TypeError("a JPEG stream is bytes or a 1-D uint8 array")
    return a


def _jpeg_check(code, ctx=None):
    if code != L.SLAM_OK:
        msg = lib().slam_last_error(ctx.handle) if ctx is not None else lib().slam_jpeg_last_error()
        raise L.SlamError(code, msg.decode() if msg else "")


def jpegInfo(buf, flags=0):
    """slam_jpeg_info[_ex]: the stream's header as a dict (width, height, channels,
    sampling, restart_interval, segments, orientation); raises SlamError for a
    stream the decoder does not take.  flags: L.JPEG_MJPEG."""
    a = _jpeg_bytes(buf)
    info = L.JpegInfo()
    if flags:
        _jpeg_check(lib().slam_jpeg_info_ex(ptr(a), a.size, ctypes.byref(info), int(flags)))
    else:
        _jpeg_check(lib().slam_jpeg_info(ptr(a), a.size, ctypes.byref(info)))
    return {k: getattr(info, k) for k, _ in L.JpegInfo._fields_}


def applyOrientation(img, orientation):
    """cv::imread's ApplyExifOrientation on an (h, w[, c]) array, as a view: Exif
    2 mirrors, 3 turns by 180 degrees, 4 flips, 5 .. 8 transpose and then do as 1,
    2, 3, 4 do."""
    o = int(orientation)
    if o >= 5:
        img = img.swapaxes(0, 1)
    if o in (2, 6):
        return img[:, ::-1]
    if o in (3, 7):
        return img[::-1, ::-1]
    if o in (4, 8):
        return img[::-1]
    return img


def imdecode(buf, channels=3, apply_orientation=True, ctx=None, host=False, with_status=False):
    """cv::imdecode(buf, IMREAD_COLOR) (channels 3, BGR) or IMREAD_GRAYSCALE
    (channels 1) of a baseline JPEG stream, decoded on the device
    (slam_jpeg_decode); host=True runs the same arithmetic on the host
    (slam_jpeg_decode_host, the contract; needs no GPU).  Returns the (h, w,
    channels) uint8 array with the Exif orientation applied as cv::imread applies
    it; with_status: also the entropy fault bits (0 for a clean stream).  Raises
    SlamError for a stream that is invalid or outside the supported format."""
    a = _jpeg_bytes(buf)
    info = jpegInfo(a)
    out = np.empty((info["height"], info["width"], channels), np.uint8)
    st = ctypes.c_int(0)
    if host:
        _jpeg_check(lib().slam_jpeg_decode_host(ptr(a), a.size, ptr(out), out.strides[0], int(channels), ctypes.byref(st)))
    else:
        ctx = ctx or default_context()
        _jpeg_check(lib().slam_jpeg_decode(ctx.handle, ptr(a), a.size, ptr(out), out.strides[0], int(channels),
                                           ctypes.byref(st)), ctx)
    if apply_orientation:
        out = np.ascontiguousarray(applyOrientation(out, info["orientation"]))
    return (out, st.value) if with_status else out


def imread(path, channels=3, apply_orientation=True, ctx=None, host=False):
    """cv::imread(path) of a JPEG file: the BGR (or gray) frame, or None for what
    cv::imread returns empty (a file that cannot be read or is no valid JPEG).  A
    valid stream outside the decoder's format (progressive, ...) raises SlamError."""
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return None
    try:
        return imdecode(data, channels, apply_orientation, ctx=ctx, host=host)
    except L.SlamError as e:
        if e.code == L.SLAM_E_INVALID_ARG:
            return None
        raise


def imdecode_batch(bufs, ctx=None, out=None, size=None, parallel=False, flags=0):
    """slam_jpeg_decode_batch_dev[_ex]: n JPEG streams of one size decoded into a
    resident (n, h, w, 3) BGR torch tensor in one pass.  size: (w, h), by default
    that of the first stream.  parallel: SLAM_OPT_JPEG_SYNC is auto for this call
    (large segments without restart markers are decoded by a lane per chunk; the
    result is the same).  flags: L.JPEG_MJPEG for the frames of a Motion-JPEG
    video.  Returns (frames, status, orientations): status[i] is 0, the stream's
    entropy fault bits, or its negative SLAM_E_* (frame zeroed); the orientations
    are not applied."""
    import torch
    ctx = ctx or default_context()
    arrs = [_jpeg_bytes(b) for b in bufs]
    n = len(arrs)
    if n == 0:
        raise ValueError("empty batch")
    if size is None:
        first = jpegInfo(arrs[0], flags)
        size = (first["width"], first["height"])
    w, h = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    assert out.is_contiguous() and tuple(out.shape) == (n, h, w, 3) and out.dtype == torch.uint8
    ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
    lens = (ctypes.c_size_t * n)(*[a.size for a in arrs])
    status = np.zeros(n, np.int32)
    orient = np.ones(n, np.int32)
    torch.cuda.current_stream(out.device).synchronize()
    sync_was = ctx.get_option(L.OPT_JPEG_SYNC)
    if parallel and not sync_was:
        ctx.set_option(L.OPT_JPEG_SYNC, 1)
    try:
        if flags:
            check(lib().slam_jpeg_decode_batch_dev_ex(ctx.handle, None, ptrs, lens, n, w, h, ctypes.c_void_p(out.data_ptr()),
                                                      ptr(status), int(flags)), ctx.handle)
        else:
            check(lib().slam_jpeg_decode_batch_dev(ctx.handle, None, ptrs, lens, n, w, h, ctypes.c_void_p(out.data_ptr()),
                                                   ptr(status)), ctx.handle)
    finally:
        if parallel and not sync_was:
            ctx.set_option(L.OPT_JPEG_SYNC, 0)
    check(lib().slam_jpeg_last_orientations(ctx.handle, ptr(orient), n), ctx.handle)
    return out, status, orient


def _sync_stats(S):
    d = {k: getattr(S, k) for k, _ in L.JpegSyncStats._fields_ if k != "ms"}
    d["ms"] = dict(zip(("sync", "count", "scan", "write", "fallback"), list(S.ms)))
    return d


def jpegLastSync(ctx=None):
    """slam_jpeg_last_sync: what the chunk-parallel path did in the context's last
    batch decode, as a dict (parallel_segments, fallback_segments, chunk_bytes,
    lanes, chunks, wg_rounds_max / _total, launch_rounds_max / _total, ms per kernel)."""
    ctx = ctx or default_context()
    S = L.JpegSyncStats()
    check(lib().slam_jpeg_last_sync(ctx.handle, ctypes.byref(S)), ctx.handle)
    return _sync_stats(S)


def imdecode_host_sync(buf, chunk_bytes=0, flags=0, channels=3):
    """slam_jpeg_decode_host_sync: the host decoder with every segment of more than
    one chunk on the chunk-parallel path, in the kernels' round structure.  Returns
    (frame, status, stats); the orientation is not applied."""
    a = _jpeg_bytes(buf)
    info = jpegInfo(a, flags)
    out = np.empty((info["height"], info["width"], channels), np.uint8)
    st = ctypes.c_int(0)
    S = L.JpegSyncStats()
    _jpeg_check(lib().slam_jpeg_decode_host_sync(ptr(a), a.size, ptr(out), out.strides[0], int(channels), int(chunk_bytes),
                                                 int(flags), ctypes.byref(st), ctypes.byref(S)))
    return out, st.value, _sync_stats(S)


def imdecode_host(buf, flags=0, channels=3):
    """slam_jpeg_decode_host_ex: (frame, status) of the serial host decoder under the parse flags"""
    a = _jpeg_bytes(buf)
    info = jpegInfo(a, flags)
    out = np.empty((info["height"], info["width"], channels), np.uint8)
    st = ctypes.c_int(0)
    _jpeg_check(lib().slam_jpeg_decode_host_ex(ptr(a), a.size, ptr(out), out.strides[0], int(channels), int(flags),
                                               ctypes.byref(st)))
    return out, st.value


def jpegStdTable(klass, slot):
    """slam_jpeg_std_table: (counts[16], values) of the Annex K Huffman table of a class (0 DC, 1 AC) and slot (0, 1)"""
    counts = np.zeros(16, np.uint8)
    vals = np.zeros(256, np.uint8)
    n = ctypes.c_int(0)
    _jpeg_check(lib().slam_jpeg_std_table(int(klass), int(slot), ptr(counts), ptr(vals), ctypes.byref(n)))
    return counts, vals[:n.value].copy()


def aviIndex(buf):
    """slam_avi_index over bytes (or an mmap / uint8 array) of an AVI file: (info
    dict, offsets, sizes) of the frames of its Motion-JPEG video stream.  Raises
    SlamError for what the walker refuses."""
    a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    info = L.AviInfo()

    def call(off, siz, cap):
        code = lib().slam_avi_index(ptr(a) if a.size else None, a.size, ctypes.byref(info), off, siz, cap)
        if code != L.SLAM_OK:
            msg = lib().slam_avi_last_error()
            raise L.SlamError(code, msg.decode() if msg else "")
    call(None, None, 0)
    n = int(info.frames)
    offsets = np.zeros(n, np.uint64)
    sizes = np.zeros(n, np.uint64)
    if n:
        call(ptr(offsets), ptr(sizes), n)
    d = {k: getattr(info, k) for k, _ in L.AviInfo._fields_}
    d["fps"] = info.rate / info.scale if info.scale else 0.0
    return d, offsets, sizes


def jpegLastTiming(ctx=None):
    """slam_jpeg_last_timing: ({parse, upload, huff, idct, upcolor} ms, {compressed,
    tables, coefficients, frames} bytes) of the context's last imdecode_batch."""
    ctx = ctx or default_context()
    ms = np.zeros(5, np.float64)
    nb = np.zeros(4, np.uint64)
    check(lib().slam_jpeg_last_timing(ctx.handle, ptr(ms), ptr(nb)), ctx.handle)
    return (dict(zip(("parse_ms", "upload_ms", "huff_ms", "idct_ms", "upcolor_ms"), ms.tolist())),
            dict(zip(("compressed_bytes", "table_bytes", "coef_bytes", "frame_bytes"), [int(v) for v in nb])))


# ---- scene rendering (the cv::viz window of vizualizePointsAndCameras, headless) ----

def renderCamera(size=(1000, 1000)):
    """viz::Camera(Vec2d(1, 1), Size(w, h)) as (fx, fy, cx, cy, near, far): a field
    of view of 1 rad per axis, f = (size / 2) / tan(0.5), the principal point at
    the centre, and the clip range (0.01, 1000.01) viz::Camera starts with."""
    w, h = size
    return ((w / 2) / math.tan(0.5), (h / 2) / math.tan(0.5), w / 2, h / 2, 0.01, 1000.01)


def _views(views):
    """(n, 12) f64: R row major then t, from a list of (R, t) or an (n, 12) array"""
    if isinstance(views, np.ndarray) and views.ndim == 2 and views.shape[1] == 12:
        return np.ascontiguousarray(views, np.float64)
    out = np.zeros((len(views), 12), np.float64)
    for i, (R, t) in enumerate(views):
        out[i, :9] = np.asarray(R, np.float64).reshape(9)
        out[i, 9:] = np.asarray(t, np.float64).reshape(3)
    return out


def renderViews(points, colors, faces, lines, line_colors, views, camera=None, size=(1000, 1000), point_size=1,
                ids=False, depth=False, ctx=None, chunk_views=0, raster_mode=L.RENDER_AUTO):
    """The scene of vizualizePointsAndCameras seen from each of `views` (a list of
    camera-to-world poses (R, t), or an (n, 12) array): points (n, 3) float32 with
    colors (n, 3) uint8 BGR (WCloud), faces (m, 3) int32 into the points (WMesh,
    vertex colours), lines (k, 6) float32 segments with line_colors (k, 3) uint8
    (WTrajectory).  slam_render_views_dev has the contract; tests/render_ref.py is
    the definition.  camera: (fx, fy, cx, cy, near, far), default renderCamera(size);
    size: (w, h).  Returns the frames (n, h, w, 3) uint8 BGR, and with ids / depth a
    tuple that also holds the int32 id plane (kind << 30 | index, -1 for the
    background) and the float32 1/Z plane (0 for the background).  The primitives
    are numpy arrays (results are numpy arrays) or resident torch tensors (results
    are tensors on their device).  chunk_views lowers the number of views per
    pass and raster_mode picks the triangle path (L.RENDER_THREAD / _WAVE /
    _WAVE_FULL_LIST); neither changes a byte.  One view of numpy arrays with
    neither of them set goes through slam_render (host buffers); everything else
    through slam_render_views_dev."""
    ctx = ctx or default_context()
    c = ctx.handle
    w, h = int(size[0]), int(size[1])
    cam = np.ascontiguousarray(camera if camera is not None else renderCamera((w, h)), np.float64).reshape(6)
    vw = _views(views)
    nv = len(vw)
    resident = not isinstance(points, np.ndarray) and hasattr(points, "data_ptr")
    if not resident and nv == 1 and not chunk_views and raster_mode == L.RENDER_AUTO:     # slam_render takes neither
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        cols = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
        fcs = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        lns = np.ascontiguousarray(lines, np.float32).reshape(-1, 6)
        lcs = np.ascontiguousarray(line_colors, np.uint8).reshape(-1, 3)
        if len(pts) != len(cols) or len(lns) != len(lcs):
            raise ValueError("one colour per point and per line")
        out = np.empty((1, h, w, 3), np.uint8)
        o_ids = np.empty((1, h, w), np.int32) if ids else None
        o_depth = np.empty((1, h, w), np.float32) if depth else None
        check(lib().slam_render(c, ptr(pts), ptr(cols), len(pts), ptr(fcs), len(fcs), ptr(lns), ptr(lcs), len(lns), ptr(vw),
                                ptr(cam), w, h, int(point_size), ptr(out), ptr(o_ids), ptr(o_depth)), c)
        res = (out,) + ((o_ids,) if ids else ()) + ((o_depth,) if depth else ())
        return res[0] if len(res) == 1 else res
    import torch
    if resident:
        dev = points.device
    else:
        dev = torch.device("cuda", ctx.device)

    def put(a, dt, width):
        if not (not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")):
            a = torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1, width)).to(dev)
        if a.dtype != getattr(torch, np.dtype(dt).name) or a.dim() != 2 or a.shape[1] != width or a.device != dev:
            raise ValueError(f"expected a resident (n, {width}) {np.dtype(dt).name} tensor")
        return a.contiguous()

    pts, cols = put(points, np.float32, 3), put(colors, np.uint8, 3)
    fcs = put(faces, np.int32, 3)
    lns, lcs = put(lines, np.float32, 6), put(line_colors, np.uint8, 3)
    if len(pts) != len(cols) or len(lns) != len(lcs):
        raise ValueError("one colour per point and per line")
    out = torch.empty((nv, h, w, 3), dtype=torch.uint8, device=dev)
    o_ids = torch.empty((nv, h, w), dtype=torch.int32, device=dev) if ids else None
    o_depth = torch.empty((nv, h, w), dtype=torch.float32, device=dev) if depth else None
    torch.cuda.current_stream(dev).synchronize()    # the tensors' producer

    def dp(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

    check(lib().slam_render_views_dev(c, None, dp(pts), dp(cols), len(pts), dp(fcs), len(fcs), dp(lns), dp(lcs), len(lns),
                                      ptr(vw), nv, ptr(cam), w, h, int(point_size), dp(out), dp(o_ids), dp(o_depth),
                                      int(chunk_views), int(raster_mode)), c)
    res = [t for t in (out, o_ids, o_depth) if t is not None]
    if not resident:
        res = [t.cpu().numpy() for t in res]
    return res[0] if len(res) == 1 else tuple(res)


def renderStats(ctx=None):
    """slam_render_last_stats: ({primitives, skipped, clipped, rasterised, fragments},
    {clear, points_lines, faces, resolve} ms) of the context's last renderViews"""
    ctx = ctx or default_context()
    st = np.zeros(5, np.uint64)
    ms = np.zeros(4, np.float64)
    check(lib().slam_render_last_stats(ctx.handle, ptr(st), ptr(ms)), ctx.handle)
    return (dict(zip(("primitives", "skipped", "clipped", "rasterised", "fragments"), [int(v) for v in st])),
            dict(zip(("clear_ms", "points_lines_ms", "faces_ms", "resolve_ms"), ms.tolist())))


# ---- JPEG encoding: cv::imencode / cv::imwrite on baseline JPEG (jpeg_enc.hip, jpeg_enc_host.cpp) ----
# cv::ImwriteFlags and cv::ImwriteJPEGSamplingFactorParams, quoted from memory of OpenCV 4.8's
# imgcodecs.hpp (the headers are not part of this repository)
IMWRITE_JPEG_QUALITY = 1
IMWRITE_JPEG_RST_INTERVAL = 4
IMWRITE_JPEG_SAMPLING_FACTOR = 7
IMWRITE_JPEG_SAMPLING_FACTOR_420 = 0x221111
IMWRITE_JPEG_SAMPLING_FACTOR_422 = 0x211111
IMWRITE_JPEG_SAMPLING_FACTOR_444 = 0x111111
_JPEG_SAMPLING = {IMWRITE_JPEG_SAMPLING_FACTOR_420: L.JPEG_420, IMWRITE_JPEG_SAMPLING_FACTOR_422: L.JPEG_422,
                  IMWRITE_JPEG_SAMPLING_FACTOR_444: L.JPEG_444}
JPEG_ENC_HEADER_ROOM = 1024      # imencode_batch's first capacity: the pixels' bytes and this


def _jpeg_params(params):
    p = [int(v) for v in params]
    if len(p) & 1:
        raise ValueError("params: (flag, value) pairs")
    quality, restart, sampling = 95, 0, L.JPEG_420
    for k, v in zip(p[0::2], p[1::2]):
        if k == IMWRITE_JPEG_QUALITY:
            quality = min(max(v, 0), 100)
        elif k == IMWRITE_JPEG_RST_INTERVAL:
            restart = min(max(v, 0), 65535)
        elif k == IMWRITE_JPEG_SAMPLING_FACTOR:
            if v not in _JPEG_SAMPLING:
                raise L.SlamError(L.SLAM_E_UNSUPPORTED, f"sampling factor {v:#x}: 4:2:0, 4:2:2 and 4:4:4 are written")
            sampling = _JPEG_SAMPLING[v]
    return quality, sampling, restart


def _enc_image(img):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)) or a.size == 0:
        raise TypeError("an image to encode is a non-empty (h, w), (h, w, 1) or (h, w, 3) uint8 array")
    return np.ascontiguousarray(a)


def jpegEncodeBound(h, w, sampling=L.JPEG_420, restart_interval=0):
    """slam_jpeg_encode_bound: a capacity that no stream of this geometry exceeds"""
    return int(lib().slam_jpeg_encode_bound(int(h), int(w), int(sampling), int(restart_interval)))


def jpegEncode(img, quality=95, sampling=L.JPEG_420, restart_interval=0, ctx=None, host=False, cap=None):
    """slam_jpeg_encode (device) or slam_jpeg_encode_host of one (h, w[, 3]) uint8
    image (BGR or gray).  cap: the capacity offered (default: the bound).  Returns
    (bytes written, size needed, status bits)."""
    a = _enc_image(img)
    h, w = a.shape[:2]
    ch = 1 if a.ndim == 2 else a.shape[2]
    if cap is None:
        cap = jpegEncodeBound(h, w, sampling, restart_interval)
    out = np.empty(max(int(cap), 1), np.uint8)
    size = ctypes.c_size_t(0)
    st = ctypes.c_int(0)
    if host:
        code = lib().slam_jpeg_encode_host(ptr(a), h, w, ch, a.strides[0], int(quality), int(sampling), int(restart_interval),
                                           ptr(out), int(cap), ctypes.byref(size), ctypes.byref(st))
        if code != L.SLAM_OK:
            msg = lib().slam_jpeg_enc_last_error()
            raise L.SlamError(code, msg.decode() if msg else "")
    else:
        ctx = ctx or default_context()
        check(lib().slam_jpeg_encode(ctx.handle, ptr(a), h, w, ch, a.strides[0], int(quality), int(sampling),
                                     int(restart_interval), ptr(out), int(cap), ctypes.byref(size), ctypes.byref(st)),
              ctx.handle)
    return out[:min(size.value, int(cap))].tobytes(), size.value, st.value


def imencode(ext, img, params=(), ctx=None, host=False):
    """cv::imencode(ext, img, params) for ".jpg" / ".jpeg": (ok, bytes), encoded on
    the device (host=True: the same arithmetic on the host, no GPU needed).  img:
    (h, w, 3) BGR or (h, w) gray uint8.  params: IMWRITE_JPEG_QUALITY (default 95),
    IMWRITE_JPEG_RST_INTERVAL (MCUs, default 0) and IMWRITE_JPEG_SAMPLING_FACTOR
    (default 4:2:0, libjpeg's).  The flags' numeric values and the 4:2:0 default are
    quoted from memory of OpenCV 4.8 (imgcodecs.hpp, grfmt_jpeg.cpp), not read from
    its sources.  The bytes are libjpeg's with its defaults (tests/jpeg_enc_ref.py);
    another extension gives (False, b"")."""
    if str(ext).lower() not in (".jpg", ".jpeg"):
        return False, b""
    quality, sampling, restart = _jpeg_params(params)
    data, size, st = jpegEncode(img, quality, sampling, restart, ctx=ctx, host=host)
    return (st == 0 and size == len(data)), data


def imwrite(path, img, params=(), ctx=None, host=False):
    """cv::imwrite(path, img, params) for a .jpg / .jpeg name: imencode's bytes in a file; False when
    the extension is another or the file cannot be written."""
    ok, data = imencode(os.path.splitext(str(path))[1], img, params, ctx=ctx, host=host)
    if not ok:
        return False
    try:
        with open(path, "wb") as f:
            f.write(data)
    except OSError:
        return False
    return True


def imencode_batch(frames, quality=95, sampling=L.JPEG_420, restart_interval=0, ctx=None):
    """slam_jpeg_encode_batch_dev: n frames of one size, a resident (n, h, w, 3) /
    (n, h, w) uint8 torch tensor or a numpy array (uploaded), encoded in one set of
    launches.  Returns a list of n bytes objects.  The first call offers h w channels
    + JPEG_ENC_HEADER_ROOM bytes per image; images that overflow it are encoded once
    more with the largest size reported."""
    import torch
    ctx = ctx or default_context()
    dev = torch.device("cuda", ctx.device)
    if not isinstance(frames, torch.Tensor):
        frames = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or frames.numel() == 0 or \
            (frames.dim() == 4 and frames.shape[3] not in (1, 3)):
        raise TypeError("frames: a non-empty (n, h, w, 3) or (n, h, w) uint8 batch")
    frames = frames.contiguous()
    n, h, w = (int(v) for v in frames.shape[:3])
    ch = 1 if frames.dim() == 3 else int(frames.shape[3])

    def run(fr, cap):
        k = int(fr.shape[0])
        out = torch.empty((k, cap), dtype=torch.uint8, device=dev)
        sizes = torch.zeros(k, dtype=torch.int64, device=dev)
        status = torch.zeros(k, dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        check(lib().slam_jpeg_encode_batch_dev(ctx.handle, None, ctypes.c_void_p(fr.data_ptr()), k, h, w, ch, w * ch, h * w * ch,
                                               int(quality), int(sampling), int(restart_interval),
                                               ctypes.c_void_p(out.data_ptr()), cap, ctypes.c_void_p(sizes.data_ptr()),
                                               ctypes.c_void_p(status.data_ptr())), ctx.handle)
        sz = sizes.cpu().numpy()
        st = status.cpu().numpy()
        host = out[:, :int(min(sz.max(), cap))].cpu().numpy()
        return host, sz, st

    host, sz, st = run(frames, h * w * ch + JPEG_ENC_HEADER_ROOM)
    res = [None if st[i] & L.JPEG_ENC_OVERFLOW else host[i, :int(sz[i])].tobytes() for i in range(n)]
    again = [i for i in range(n) if res[i] is None]
    if again:
        host, sz2, st2 = run(frames[torch.tensor(again, device=dev)].contiguous(), int(sz[again].max()))
        for k, i in enumerate(again):
            if st2[k] & L.JPEG_ENC_OVERFLOW:
                raise L.SlamError(L.SLAM_E_CAPACITY, f"frame {i}: {int(sz2[k])} bytes after a retry sized by the first pass")
            res[i] = host[k, :int(sz2[k])].tobytes()
    return res


def jpegEncLastTiming(ctx=None):
    """slam_jpeg_enc_last_timing: ({dct, count, scan, readback, pack, ffcount, write} ms, {frame,
    coefficient, unstuffed, readback} bytes) of the context's last device encode."""
    ctx = ctx or default_context()
    ms = np.zeros(7, np.float64)
    nb = np.zeros(4, np.uint64)
    check(lib().slam_jpeg_enc_last_timing(ctx.handle, ptr(ms), ptr(nb)), ctx.handle)
    return (dict(zip(("dct_ms", "count_ms", "scan_ms", "readback_ms", "pack_ms", "ffcount_ms", "write_ms"), ms.tolist())),
            dict(zip(("frame_bytes", "coef_bytes", "unstuffed_bytes", "readback_bytes"), [int(v) for v in nb])))


# ---- dense points: plane-sweep stereo ------------------------

def _mvs_frames(frames):
    """host frames of one shape as contiguous arrays -> (list, w, h, channels)"""
    out = [np.ascontiguousarray(_frame13(f)[0]) for f in frames]
    a = out[0]
    if any(f.shape != a.shape for f in out):
        raise ValueError("frames of one shape")
    return out, a.shape[1], a.shape[0], 1 if a.ndim == 2 else 3


def _ptr_array(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def censusTransform(frame, ctx=None):
    """the 9 x 7 census of a frame (slam_mvs_census_dev): 62 bits in a uint64, bit
    b in the order dy = -3..3 outer, dx = -4..4 inner, centre skipped, set iff the
    clamped neighbour's gray is below the centre's.  `frame`: a host array -> (h,
    w) uint64, or a resident torch batch (n, h, w[, 3]) -> (n, h, w) uint64."""
    import torch
    c = _ctx(ctx)
    single = isinstance(frame, np.ndarray)
    if single:
        a = np.ascontiguousarray(_frame13(frame)[0])
        frame = torch.from_numpy(a[None]).cuda()
    fr, n, w, h, ch = _resident(frame)
    out = torch.empty((n, h, w), dtype=torch.int64, device=fr.device)
    check(lib().slam_mvs_census_dev(c, None, ctypes.c_void_p(fr.data_ptr()), n, w, h, ch, ctypes.c_void_p(out.data_ptr())), c)
    res = out.cpu().numpy().view(np.uint64)
    return res[0] if single else res


def _mvs_pose_args(M, v, planes, S):
    M = np.ascontiguousarray(M, np.float64).reshape(S, 9)
    v = np.ascontiguousarray(v, np.float64).reshape(S, 3)
    planes = np.ascontiguousarray(planes, np.float64).reshape(-1)
    return M, v, planes


def planeSweepDepth(ref, srcs, M, v, planes, radius=2, uniq=80, min_views=1, ctx=None, host=False):
    """Plane-sweep depth of one reference frame against S = len(srcs) sources (host
    arrays of one shape): slam_mvs_depth, or with host=True its twin
    slam_mvs_depth_host, which needs no device and gives the same bits.  M (S, 3, 3)
    and v (S, 3) as dense.sweep_matrices returns them, planes (D) inverse depths.
    Returns (plane int16, cost int32, inv_depth float32), each (h, w); inv_depth is
    0 where the winner was rejected."""
    fr, w, h, ch = _mvs_frames([ref] + list(srcs))
    S = len(fr) - 1
    M, v, planes = _mvs_pose_args(M, v, planes, S) if S > 0 else (np.zeros((0, 9)), np.zeros((0, 3)),
                                                                  np.ascontiguousarray(planes, np.float64).reshape(-1))
    plane = np.empty((h, w), np.int16)
    cost = np.empty((h, w), np.int32)
    inv = np.empty((h, w), np.float32)
    sp = _ptr_array(fr[1:]) if S > 0 else None
    tail = (S, w, h, w * ch, ch, ptr(M), ptr(v), ptr(planes), len(planes), int(radius), int(uniq), int(min_views),
            ptr(plane), ptr(cost), ptr(inv))
    if host:
        check(lib().slam_mvs_depth_host(ptr(fr[0]), sp, *tail))
    else:
        c = _ctx(ctx)
        check(lib().slam_mvs_depth(c, ptr(fr[0]), sp, *tail), c)
    return plane, cost, inv


def planeSweepDepthBatch(frames, ref_idx, src_idx, M, v, planes, radius=2, uniq=80, min_views=1, ctx=None):
    """slam_mvs_depth_batch_dev: depth maps of the references ref_idx among the
    resident frames (a torch batch (n, h, w[, 3])); src_idx[i] lists reference i's 1..4
    sources, M (nref, 4, 9) and v (nref, 4, 3) hold their matrices (unused rows
    ignored), planes (nref, D).  The census runs once per distinct frame.  Returns
    resident (plane int16, cost int32, inv_depth float32) tensors, each (nref, h, w)."""
    import torch
    c = _ctx(ctx)
    fr, n, w, h, ch = _resident(frames)
    nref = len(ref_idx)
    ref = np.ascontiguousarray(ref_idx, np.int32).reshape(nref)
    nsrc = np.array([len(s) for s in src_idx], np.int32)
    src = np.full((nref, 4), -1, np.int32)
    for i, s in enumerate(src_idx):
        if len(s) > 4:
            raise ValueError("at most 4 sources per reference")
        src[i, :len(s)] = s
    M = np.ascontiguousarray(M, np.float64).reshape(nref, 36)
    v = np.ascontiguousarray(v, np.float64).reshape(nref, 12)
    planes = np.ascontiguousarray(planes, np.float64).reshape(nref, -1)
    plane = torch.empty((nref, h, w), dtype=torch.int16, device=fr.device)
    cost = torch.empty((nref, h, w), dtype=torch.int32, device=fr.device)
    inv = torch.empty((nref, h, w), dtype=torch.float32, device=fr.device)
    check(lib().slam_mvs_depth_batch_dev(c, None, ctypes.c_void_p(fr.data_ptr()), n, w, h, ch, nref, ptr(ref), ptr(nsrc),
                                         ptr(src), ptr(M), ptr(v), ptr(planes), planes.shape[1], int(radius), int(uniq),
                                         int(min_views), ctypes.c_void_p(plane.data_ptr()),
                                         ctypes.c_void_p(cost.data_ptr()), ctypes.c_void_p(inv.data_ptr())), c)
    return plane, cost, inv


# ---- semi-global aggregation of the sweep's cost volume ---------

def _batch_args(ref_idx, src_idx, M, v, planes):
    nref = len(ref_idx)
    ref = np.ascontiguousarray(ref_idx, np.int32).reshape(nref)
    nsrc = np.array([len(s) for s in src_idx], np.int32)
    src = np.full((nref, 4), -1, np.int32)
    for i, s in enumerate(src_idx):
        if len(s) > 4:
            raise ValueError("at most 4 sources per reference")
        src[i, :len(s)] = s
    M = np.ascontiguousarray(M, np.float64).reshape(nref, 36)
    v = np.ascontiguousarray(v, np.float64).reshape(nref, 12)
    planes = np.ascontiguousarray(planes, np.float64).reshape(nref, -1)
    return nref, ref, nsrc, src, M, v, planes


def planeSweepCostVolume(frames, ref_idx, src_idx, M, v, planes, radius=2, ctx=None, host=False):
    """The cost volume the sweep never stores (slam_mvs_cost_volume_dev): (C uint16,
    nvalid uint8), each (nref, h, w, D) with the plane index innermost, of the
    references ref_idx among the frames; arguments as planeSweepDepthBatch.  frames:
    a resident torch batch -> resident tensors; with host=True a list of host arrays
    -> numpy arrays from the host twin, the same bits."""
    nref, ref, nsrc, src, M, v, planes = _batch_args(ref_idx, src_idx, M, v, planes)
    D = planes.shape[1]
    if host:
        fr, w, h, ch = _mvs_frames(list(frames))
        C = np.empty((nref, h, w, D), np.uint16)
        nv = np.empty((nref, h, w, D), np.uint8)
        for i in range(nref):
            S = int(nsrc[i])
            sp = _ptr_array([fr[j] for j in src[i, :S]]) if S > 0 else None
            check(lib().slam_mvs_cost_volume_host(ptr(fr[ref[i]]), sp, S, w, h, w * ch, ch, ptr(M[i]), ptr(v[i]),
                                                  ptr(planes[i]), D, int(radius), ptr(C[i]), ptr(nv[i])))
        return C, nv
    import torch
    c = _ctx(ctx)
    fr, n, w, h, ch = _resident(frames)
    C = torch.empty((nref, h, w, D), dtype=torch.uint16, device=fr.device)
    nv = torch.empty((nref, h, w, D), dtype=torch.uint8, device=fr.device)
    check(lib().slam_mvs_cost_volume_dev(c, None, ctypes.c_void_p(fr.data_ptr()), n, w, h, ch, nref, ptr(ref), ptr(nsrc),
                                         ptr(src), ptr(M), ptr(v), ptr(planes), D, int(radius),
                                         ctypes.c_void_p(C.data_ptr()), ctypes.c_void_p(nv.data_ptr())), c)
    return C, nv


def sgmAggregate(C, P1, P2, paths=8, ctx=None, host=False):
    """Semi-global aggregation of given volumes (slam_mvs_sgm_aggregate_dev): C (n, h,
    w, D) uint16 with every value <= 12544, the effective penalties 0 <= P1 <= P2 <=
    65535 - 12544, paths 4 or 8 -> S (n, h, w, D) int32, the sum of the path costs.  A
    resident torch tensor gives a resident tensor; a numpy array runs on the device
    too unless host=True (the host twin, the same bits)."""
    if isinstance(C, np.ndarray):
        a = np.ascontiguousarray(C, np.uint16)
        if a.ndim != 4:
            raise ValueError("C: (n, h, w, D) uint16")
        n, h, w, D = a.shape
        S = np.empty(a.shape, np.int32)
        if host:
            check(lib().slam_mvs_sgm_aggregate_host(ptr(a), n, w, h, D, int(P1), int(P2), int(paths), ptr(S)))
            return S
        import torch
        return sgmAggregate(torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16), P1, P2, paths, ctx=ctx).cpu().numpy()
    import torch
    if C.dtype != torch.uint16 or C.dim() != 4:
        raise ValueError("C: (n, h, w, D) uint16")
    c = _ctx(ctx)
    C = C.contiguous()
    torch.cuda.current_stream(C.device).synchronize()
    n, h, w, D = C.shape
    S = torch.empty((n, h, w, D), dtype=torch.int32, device=C.device)
    check(lib().slam_mvs_sgm_aggregate_dev(c, None, ctypes.c_void_p(C.data_ptr()), n, w, h, D, int(P1), int(P2), int(paths),
                                           ctypes.c_void_p(S.data_ptr())), c)
    return S


def planeSweepDepthSgm(ref, srcs, M, v, planes, radius=2, uniq=80, min_views=1, p1=10, p2=120, paths=8, ctx=None,
                       host=False):
    """planeSweepDepth with semi-global aggregation between the volume and the winner
    (slam_mvs_depth_sgm, host=True: slam_mvs_depth_sgm_host, the same bits).  p1 <= p2
    in 0..255 are the penalties per window pixel and source in Hamming bits for a
    change of one plane and of more; paths 4 or 8.  cost is S[best]."""
    fr, w, h, ch = _mvs_frames([ref] + list(srcs))
    S = len(fr) - 1
    M, v, planes = _mvs_pose_args(M, v, planes, S) if S > 0 else (np.zeros((0, 9)), np.zeros((0, 3)),
                                                                  np.ascontiguousarray(planes, np.float64).reshape(-1))
    plane = np.empty((h, w), np.int16)
    cost = np.empty((h, w), np.int32)
    inv = np.empty((h, w), np.float32)
    sp = _ptr_array(fr[1:]) if S > 0 else None
    tail = (S, w, h, w * ch, ch, ptr(M), ptr(v), ptr(planes), len(planes), int(radius), int(uniq), int(min_views),
            int(p1), int(p2), int(paths), ptr(plane), ptr(cost), ptr(inv))
    if host:
        check(lib().slam_mvs_depth_sgm_host(ptr(fr[0]), sp, *tail))
    else:
        c = _ctx(ctx)
        check(lib().slam_mvs_depth_sgm(c, ptr(fr[0]), sp, *tail), c)
    return plane, cost, inv


def planeSweepDepthSgmBatch(frames, ref_idx, src_idx, M, v, planes, radius=2, uniq=80, min_views=1, p1=10, p2=120, paths=8,
                            ctx=None, budget=None):
    """planeSweepDepthBatch with semi-global aggregation (slam_mvs_depth_sgm_batch_dev).
    The references are worked through in groups whose scratch stays under `budget`
    bytes (None: the library's 8 GiB); the results do not depend on it."""
    import torch
    c = _ctx(ctx)
    fr, n, w, h, ch = _resident(frames)
    nref, ref, nsrc, src, M, v, planes = _batch_args(ref_idx, src_idx, M, v, planes)
    plane = torch.empty((nref, h, w), dtype=torch.int16, device=fr.device)
    cost = torch.empty((nref, h, w), dtype=torch.int32, device=fr.device)
    inv = torch.empty((nref, h, w), dtype=torch.float32, device=fr.device)
    check(lib().slam_mvs_sgm_set_budget(c, int(budget or 0)), c)
    try:
        check(lib().slam_mvs_depth_sgm_batch_dev(c, None, ctypes.c_void_p(fr.data_ptr()), n, w, h, ch, nref, ptr(ref),
                                                 ptr(nsrc), ptr(src), ptr(M), ptr(v), ptr(planes), planes.shape[1],
                                                 int(radius), int(uniq), int(min_views), int(p1), int(p2), int(paths),
                                                 ctypes.c_void_p(plane.data_ptr()), ctypes.c_void_p(cost.data_ptr()),
                                                 ctypes.c_void_p(inv.data_ptr())), c)
    finally:
        lib().slam_mvs_sgm_set_budget(c, 0)
    return plane, cost, inv


def sgmLastTiming(ctx=None):
    """HIP-event times of the context's last aggregated sweep: dict(volume_ms, paths_ms, winner_ms)"""
    ms = np.zeros(3, np.float64)
    c = _ctx(ctx)
    check(lib().slam_mvs_sgm_last_timing(c, ptr(ms)), c)
    return dict(zip(("volume_ms", "paths_ms", "winner_ms"), ms.tolist()))


def fuseDepthMaps(frames, inv_depth, nbrs, M, v, B, c, eps=0.01, min_consistent=1, step=4, radius=2, frame_idx=None,
                  cap=None, ctx=None):
    """slam_mvs_fuse_dev / slam_mvs_fuse: the pairwise consistency filter over nmaps
    depth maps and the emission of the survivors, raster order, map after map.
    frames: a resident torch batch (map i belongs to frame frame_idx[i], default i)
    with inv_depth a resident (nmaps, h, w) float32 tensor, or a list of host frames
    with host maps.  nbrs[i]: the maps map i is checked against (at most 4), M
    (nmaps, 4, 9) / v (nmaps, 4, 3) the motions map i -> neighbour, B (nmaps, 9) and c
    (nmaps, 3) the back-projection (dense.backproject_matrices).  cap: the output
    capacity (default: every grid pixel); too small raises SlamError with code
    SLAM_E_CAPACITY and the needed count in its `needed`.  Returns (points (n, 3)
    float64, colors (n, 3) uint8)."""
    h_ctx = _ctx(ctx)
    nmaps = len(nbrs)
    nn = np.array([len(r) for r in nbrs], np.int32)
    nb = np.full((max(nmaps, 1), 4), -1, np.int32)
    for i, r in enumerate(nbrs):
        if len(r) > 4:
            raise ValueError("at most 4 neighbours per map")
        nb[i, :len(r)] = r
    M = np.ascontiguousarray(M, np.float64).reshape(nmaps, 36)
    v = np.ascontiguousarray(v, np.float64).reshape(nmaps, 12)
    B = np.ascontiguousarray(B, np.float64).reshape(nmaps, 9)
    cc = np.ascontiguousarray(c, np.float64).reshape(nmaps, 3)
    resident = not isinstance(frames, (list, tuple, np.ndarray)) and hasattr(frames, "data_ptr")
    if resident:
        fr, n, w, h, ch = _resident(frames)
    else:
        fl, w, h, ch = _mvs_frames(list(frames))
    if cap is None:
        cap = nmaps * (-(-h // step)) * (-(-w // step))
    pts = np.empty((max(cap, 1), 3), np.float64)
    cols = np.empty((max(cap, 1), 3), np.uint8)
    n_out = ctypes.c_int(0)
    if resident:
        import torch
        fi = np.ascontiguousarray(np.arange(nmaps) if frame_idx is None else frame_idx, np.int32).reshape(nmaps)
        inv = inv_depth if hasattr(inv_depth, "data_ptr") else torch.from_numpy(np.ascontiguousarray(inv_depth, np.float32)).to(fr.device)
        if inv.dtype != torch.float32 or tuple(inv.shape) != (nmaps, h, w):
            raise ValueError("inv_depth: float32 (nmaps, h, w)")
        inv = inv.contiguous()
        torch.cuda.current_stream(inv.device).synchronize()
        rc = lib().slam_mvs_fuse_dev(h_ctx, None, ctypes.c_void_p(fr.data_ptr()), n, w, h, ch, nmaps, ptr(fi),
                                     ctypes.c_void_p(inv.data_ptr()), ptr(nn), ptr(nb), ptr(M), ptr(v), ptr(B), ptr(cc),
                                     float(eps), int(min_consistent), int(step), int(radius), ptr(pts), ptr(cols), int(cap),
                                     ctypes.byref(n_out))
    else:
        if len(fl) != nmaps:
            raise ValueError("one host frame per map")
        inv = np.ascontiguousarray(inv_depth, np.float32).reshape(nmaps, h, w)
        rc = lib().slam_mvs_fuse(h_ctx, _ptr_array(fl), w, h, w * ch, ch, nmaps, ptr(inv), ptr(nn), ptr(nb), ptr(M), ptr(v),
                                 ptr(B), ptr(cc), float(eps), int(min_consistent), int(step), int(radius), ptr(pts),
                                 ptr(cols), int(cap), ctypes.byref(n_out))
    try:
        check(rc, h_ctx)
    except L.SlamError as e:
        e.needed = n_out.value          # SLAM_E_CAPACITY: the count that did not fit
        raise
    return pts[:n_out.value].copy(), cols[:n_out.value].copy()


# ---- surface from the depth maps: TSDF fusion and marching cubes ----

def _tsdf_volume(volume, host):
    """(pointer, nx, ny, nz, resident) of a volume: a resident int32 torch tensor or a host int32 array, (6, nz, ny, nx)"""
    resident = hasattr(volume, "data_ptr")
    if resident:
        import torch
        if host:
            raise ValueError("host=True takes a host volume")
        if volume.dtype != torch.int32 or volume.dim() != 4 or volume.shape[0] != 6 or not volume.is_contiguous():
            raise ValueError("volume: contiguous int32 (6, nz, ny, nx)")
        p = ctypes.c_void_p(volume.data_ptr())
    else:
        if not isinstance(volume, np.ndarray) or volume.dtype != np.int32 or volume.ndim != 4 or volume.shape[0] != 6 \
                or not volume.flags.c_contiguous:
            raise ValueError("volume: contiguous int32 (6, nz, ny, nx)")
        p = ptr(volume)
    return p, int(volume.shape[3]), int(volume.shape[2]), int(volume.shape[1]), resident


def tsdfIntegrate(volume, frames, inv_depth, P, origin, voxel, trunc, frame_idx=None, ctx=None, host=False):
    """slam_tsdf_integrate_dev / slam_tsdf_integrate / slam_tsdf_integrate_host: add the depth
    maps inv_depth (nmaps, h, w) float32 to `volume` (int32 (6, nz, ny, nx), updated in place
    and returned).  A resident volume takes a resident frame batch (n, h, w[, 3]) and resident
    maps; a host volume takes host frames (a list or an array) and host maps, on the device or,
    with host=True, through the host twin: the same bits without a device.  Map m belongs to
    frame frame_idx[m] (default m) and has the projection P[m] (3 x 4, surface.projection_matrix);
    origin (3), voxel and trunc describe the grid.  The caller keeps a volume below 2^20 maps
    in total (surface.fuse_maps counts)."""
    vp, nx, ny, nz, resident = _tsdf_volume(volume, host)
    P = np.ascontiguousarray(P, np.float64).reshape(-1, 12)
    nmaps = len(P)
    if nmaps > (1 << 20):
        raise ValueError("at most 2^20 maps per call")
    fi = None if frame_idx is None else np.ascontiguousarray(frame_idx, np.int32).reshape(nmaps)
    org = np.ascontiguousarray(origin, np.float64).reshape(3)
    if resident:
        import torch
        h_ctx = _ctx(ctx)
        fr, n, w, h, ch = _resident(frames)
        inv = inv_depth if hasattr(inv_depth, "data_ptr") else torch.from_numpy(np.ascontiguousarray(inv_depth, np.float32)).to(fr.device)
        if inv.dtype != torch.float32 or tuple(inv.shape) != (nmaps, h, w):
            raise ValueError("inv_depth: float32 (nmaps, h, w)")
        inv = inv.contiguous()
        torch.cuda.current_stream(inv.device).synchronize()
        check(lib().slam_tsdf_integrate_dev(h_ctx, None, vp, nx, ny, nz, ptr(org), float(voxel), float(trunc),
                                            ctypes.c_void_p(fr.data_ptr()), n, w, h, ch, ptr(fi),
                                            ctypes.c_void_p(inv.data_ptr()), ptr(P), nmaps), h_ctx)
        return volume
    fl, w, h, ch = _mvs_frames(list(frames))
    fr = np.ascontiguousarray(np.stack(fl))
    inv = np.ascontiguousarray(inv_depth, np.float32).reshape(nmaps, h, w)
    tail = (nx, ny, nz, ptr(org), float(voxel), float(trunc), ptr(fr), len(fl), w, h, ch, ptr(fi), ptr(inv), ptr(P), nmaps)
    if host:
        check(lib().slam_tsdf_integrate_host(vp, *tail))
    else:
        h_ctx = _ctx(ctx)
        check(lib().slam_tsdf_integrate(h_ctx, vp, *tail), h_ctx)
    return volume


TSDF_MESH_CAP = (1 << 16, 1 << 17)       # tsdfMesh's first try with cap=None: vertices, faces


def tsdfMesh(volume, origin, voxel, min_weight=2, cap=None, ctx=None, host=False):
    """slam_tsdf_mesh_dev / slam_tsdf_mesh / slam_tsdf_mesh_host: marching cubes on the node
    lattice of `volume` -> (vertices (n, 3) float64, colors (n, 3) uint8 blue-green-red, faces
    (m, 3) int32).  cap = (vertices, faces) are the output capacities; too small raises
    SlamError with code SLAM_E_CAPACITY and both needed counts in its `needed`.  With
    cap=None the call is repeated once with the needed counts."""
    vp, nx, ny, nz, resident = _tsdf_volume(volume, host)
    org = np.ascontiguousarray(origin, np.float64).reshape(3)
    h_ctx = None if host else _ctx(ctx)
    cv, cf = TSDF_MESH_CAP if cap is None else (int(cap[0]), int(cap[1]))
    for attempt in (0, 1):
        nv, nf = ctypes.c_int(0), ctypes.c_int(0)
        if resident:
            import torch
            dev = volume.device
            torch.cuda.current_stream(dev).synchronize()
            v = torch.empty((max(cv, 1), 3), dtype=torch.float64, device=dev)
            c = torch.empty((max(cv, 1), 3), dtype=torch.uint8, device=dev)
            f = torch.empty((max(cf, 1), 3), dtype=torch.int32, device=dev)
            rc = lib().slam_tsdf_mesh_dev(h_ctx, None, vp, nx, ny, nz, ptr(org), float(voxel), int(min_weight),
                                          ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(c.data_ptr()),
                                          ctypes.c_void_p(f.data_ptr()), cv, cf, ctypes.byref(nv), ctypes.byref(nf))
        else:
            v, c, f = np.empty((max(cv, 1), 3), np.float64), np.empty((max(cv, 1), 3), np.uint8), np.empty((max(cf, 1), 3), np.int32)
            tail = (nx, ny, nz, ptr(org), float(voxel), int(min_weight), ptr(v), ptr(c), ptr(f), cv, cf, ctypes.byref(nv),
                    ctypes.byref(nf))
            rc = lib().slam_tsdf_mesh_host(vp, *tail) if host else lib().slam_tsdf_mesh(h_ctx, vp, *tail)
        if rc == L.SLAM_E_CAPACITY and cap is None and attempt == 0:
            cv, cf = nv.value, nf.value
            continue
        try:
            check(rc, h_ctx)
        except L.SlamError as e:
            e.needed = (nv.value, nf.value)
            raise
        break
    if resident:
        return v[:nv.value].cpu().numpy(), c[:nv.value].cpu().numpy(), f[:nf.value].cpu().numpy()
    return v[:nv.value].copy(), c[:nv.value].copy(), f[:nf.value].copy()


def tsdfLastTiming(ctx=None):
    """slam_tsdf_last_timing: library HIP-event milliseconds of the last integrate call and the
    last extraction: dict(integrate, classify_count, scan, emit)"""
    ms = np.zeros(4, np.float64)
    c = _ctx(ctx)
    check(lib().slam_tsdf_last_timing(c, ptr(ms)), c)
    return dict(zip(("integrate", "classify_count", "scan", "emit"), [float(x) for x in ms]))


# ---- texture of the fused surface: a per-face atlas ----

def _is_resident(a):
    return not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def _dptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def texSelect(ids, view0, nf, state=None, ctx=None, host=False):
    """slam_tex_select_dev / slam_tex_select / slam_tex_select_host: fold the id images `ids`
    (nv, h, w) int32 (renderViews(..., ids=True) of the mesh from nv views) into the per-face
    state (best_count, best_view), two int32 arrays of nf, updated in place and returned.
    The views' global indices are view0 .. view0 + nv - 1; state=None starts from (0, -1).
    Resident ids take (and give) resident state tensors; host ids go through the device or,
    with host=True, through the host twin: the same bits without a device."""
    nf = int(nf)
    if _is_resident(ids):
        import torch
        if host:
            raise ValueError("host=True takes host ids")
        if ids.dtype != torch.int32 or ids.dim() != 3:
            raise ValueError("ids: int32 (nv, h, w)")
        ids = ids.contiguous()
        if state is None:
            state = (torch.zeros(nf, dtype=torch.int32, device=ids.device), torch.full((nf,), -1, dtype=torch.int32, device=ids.device))
        bc, bv = state
        if any(t.dtype != torch.int32 or tuple(t.shape) != (nf,) or not t.is_contiguous() or t.device != ids.device for t in (bc, bv)):
            raise ValueError("state: two contiguous int32 tensors of nf on the ids' device")
        torch.cuda.current_stream(ids.device).synchronize()
        h_ctx = _ctx(ctx)
        check(lib().slam_tex_select_dev(h_ctx, None, _dptr(ids), int(ids.shape[0]), int(ids.shape[1]), int(ids.shape[2]), int(view0),
                                        nf, _dptr(bc), _dptr(bv)), h_ctx)
        return bc, bv
    ids = np.ascontiguousarray(ids, np.int32)
    if ids.ndim != 3:
        raise ValueError("ids: int32 (nv, h, w)")
    if state is None:
        state = (np.zeros(nf, np.int32), np.full(nf, -1, np.int32))
    bc, bv = state
    if any(not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.shape != (nf,) or not a.flags.c_contiguous for a in (bc, bv)):
        raise ValueError("state: two contiguous int32 arrays of nf")
    tail = (ptr(ids) if ids.size else None, ids.shape[0], ids.shape[1], ids.shape[2], int(view0), nf, ptr(bc) if nf else None,
            ptr(bv) if nf else None)
    if host:
        check(lib().slam_tex_select_host(*tail))
    else:
        h_ctx = _ctx(ctx)
        check(lib().slam_tex_select(h_ctx, *tail), h_ctx)
    return bc, bv


def texLayout(nf, T, page):
    """slam_tex_layout: the atlas layout of nf faces with T texels per triangle leg on pages
    of at most `page` texels -> (page_w, page_h (list, one per page), uv (nf, 3, 2) float64,
    page (nf,) int32).  A corner at page texel (x, y) has uv (x / page_w, 1 - y / page_h)."""
    nf = int(nf)
    npages, pw = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().slam_tex_layout(nf, int(T), int(page), ctypes.byref(npages), ctypes.byref(pw), None, 0, None, None))
    ph = np.zeros(max(npages.value, 1), np.int32)
    uv = np.zeros((max(nf, 1), 3, 2), np.float64)
    fp = np.zeros(max(nf, 1), np.int32)
    check(lib().slam_tex_layout(nf, int(T), int(page), ctypes.byref(npages), ctypes.byref(pw), ptr(ph), npages.value,
                                ptr(uv) if nf else None, ptr(fp) if nf else None))
    return pw.value, [int(v) for v in ph[:npages.value]], uv[:nf], fp[:nf]


def _split_pages(atlas, page_w, page_h):
    out, o = [], 0
    for hgt in page_h:
        out.append(atlas[o:o + hgt * page_w * 3].reshape(hgt, page_w, 3))
        o += hgt * page_w * 3
    return out


def texFill(vertices, colors, faces, frames, P, best_count, best_view, min_pixels=4, T=12, page=4096, frame_idx=None, ctx=None,
            host=False):
    """slam_tex_fill_dev / slam_tex_fill / slam_tex_fill_host: the atlas pages (a list of
    (page_h, page_w, 3) uint8 arrays, blue-green-red) of the mesh vertices (nv, 3) float64,
    colors (nv, 3) uint8, faces (nf, 3) int32.  View m is frame frame_idx[m] (default m) with the
    projection P[m] (3 x 4, surface.projection_matrix); best_count / best_view are texSelect's
    state.  A resident frame batch (n, h, w[, 3]) takes the mesh and the state as host arrays or
    resident tensors; host frames (a list or an array) go through the device or, with host=True,
    through the host twin: the same bits without a device."""
    P = np.ascontiguousarray(P, np.float64).reshape(-1, 12)
    nviews = len(P)
    fi = None if frame_idx is None else np.ascontiguousarray(frame_idx, np.int32).reshape(nviews)
    nv, nf = int(vertices.shape[0]), int(faces.shape[0])
    pw, ph, _, _ = texLayout(nf, T, page)
    nbytes = sum(ph) * pw * 3
    scal = (int(min_pixels), int(T), int(page))
    if _is_resident(frames):
        import torch
        if host:
            raise ValueError("host=True takes host frames")
        fr, n, w, h, ch = _resident(frames)
        dev = fr.device

        def put(a, dt, shape):
            if not _is_resident(a):
                a = torch.from_numpy(np.ascontiguousarray(a, dt).reshape(shape)).to(dev)
            if a.dtype != getattr(torch, np.dtype(dt).name) or tuple(a.shape) != shape or a.device != dev:
                raise ValueError(f"expected {np.dtype(dt).name} {shape} on the frames' device")
            return a.contiguous()

        V, C, F = put(vertices, np.float64, (nv, 3)), put(colors, np.uint8, (nv, 3)), put(faces, np.int32, (nf, 3))
        bc, bv = put(best_count, np.int32, (nf,)), put(best_view, np.int32, (nf,))
        atlas = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        h_ctx = _ctx(ctx)
        check(lib().slam_tex_fill_dev(h_ctx, None, _dptr(V), _dptr(C), _dptr(F), nv, nf, _dptr(fr), n, h, w, ch, ptr(fi), ptr(P),
                                      nviews, _dptr(bc), _dptr(bv), *scal, _dptr(atlas) if nbytes else None), h_ctx)
        return _split_pages(atlas[:nbytes].cpu().numpy(), pw, ph)
    frames = list(frames)
    if frames:
        fl, w, h, ch = _mvs_frames(frames)
        fr = np.ascontiguousarray(np.stack(fl))
    else:
        fl, w, h, ch, fr = [], 1, 1, 1, None
    V = np.ascontiguousarray(vertices, np.float64).reshape(nv, 3)
    C = np.ascontiguousarray(colors, np.uint8).reshape(nv, 3)
    F = np.ascontiguousarray(faces, np.int32).reshape(nf, 3)
    bc = np.ascontiguousarray(best_count, np.int32).reshape(nf)
    bv = np.ascontiguousarray(best_view, np.int32).reshape(nf)
    atlas = np.zeros(max(nbytes, 1), np.uint8)

    def p0(a):
        return ptr(a) if a is not None and a.size else None

    tail = (p0(V), p0(C), p0(F), nv, nf, p0(fr), len(fl), h, w, ch, ptr(fi), p0(P), nviews, p0(bc), p0(bv), *scal,
            ptr(atlas) if nbytes else None)
    if host:
        check(lib().slam_tex_fill_host(*tail))
    else:
        h_ctx = _ctx(ctx)
        check(lib().slam_tex_fill(h_ctx, *tail), h_ctx)
    return _split_pages(atlas[:nbytes], pw, ph)


def texLastTiming(ctx=None):
    """slam_tex_last_timing: library HIP-event milliseconds of the last texSelect on the device
    (tex_count + tex_best) and of the last texFill: dict(select, fill)"""
    ms = np.zeros(2, np.float64)
    c = _ctx(ctx)
    check(lib().slam_tex_last_timing(c, ptr(ms)), c)
    return dict(zip(("select", "fill"), [float(x) for x in ms]))

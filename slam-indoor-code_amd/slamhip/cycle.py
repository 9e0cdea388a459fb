"""The reference's per-frame pipeline around the hot path: mainCycle and slamMain.

Restates, call for call, the host control flow that drives the extract ->
match -> pose -> triangulate -> BA path, so that a sequence run through this
module produces the reference's output files (points / colors / poses /
rotations .txt, rawOutput's 12-digit fixed format):

  slam_main                     src/main.cpp:71-107 (slamMain: restart loop, final outputs)
  main_cycle                    cycleProcessing/mainCycle.cpp:73-238
  processing_first_pair_frames  mainCycle.cpp:241-275
  define_first_pair_frames      mainCycle.cpp:278-306
  find_good_frame_from_batch    cycleProcessing/batch.cpp:59-99 (+ :101-160 scan, :228-267 fill)
  find_first_good_frame         mainCycleInternals.cpp:137-156
  compute_transformation_and_filter_points   mainCycleInternals.cpp:159-175
  define_features_correspond_spatial_indices mainCycleInternals.cpp:178-204
  get_old_spatial_points_and_new_frame_feature_coords  mainCycleInternals.cpp:207-219
  push_new_spatial_points       mainCycleInternals.cpp:222-246
  refine_transformation_for_global_coords    translation/cameraTranslation.cpp:71-77

Every numeric step goes through an `ops` object.  The default, GpuOps, is the
product path: the HIP kernels behind the C ABI (FAST, SIFT / ORB, kNN + ratio,
essential-matrix RANSAC + recoverPose, PnP RANSAC, DLT triangulation, BA),
with every BGR frame uploaded to HBM once and each candidate search run as one
device pass over the batch (GpuOps.search, the slam_batch_* calls).
The parity tests pass an object with the same methods backed by the CPU
oracle; this module never imports the oracle.

Reference semantics kept on purpose:
  * descriptors of the previous good frame are recomputed on every search and
    ORB's border filter mutates the keypoint lists in place (batch.cpp:113,178);
  * window entries pushed for BA are snapshots: keypoint and index lists are
    copied, R / t arrays are shared (cv::Mat shallow copies), so BA's in-place
    update reaches the deque (bundleAdjustment.cpp:178-201);
  * poses.txt / rotations.txt are written when a pose is estimated, before BA
    refines it (mainCycle.cpp:93-96, :172-177); BA mutates K in place.
"""
import ctypes
import os
import threading

import numpy as np

from . import _lib as L
from ._lib import DMATCH_DTYPE, KEYPOINT_DTYPE
from .api import (bundle_adjust_arrays, calcOpticalFlowPyrLK, estimateTransformation, extractDescriptor,
                  fastExtractor, getMatcherTypeIndex, loss_from_config, matchFramesPairFeatures, reconstruct,
                  rodrigues_to_matrix, rodrigues_to_vector, solvePnPRansac)

EMPTY_BATCH = L.EMPTY_BATCH          # batch.h:5
FRAME_NOT_FOUND = L.FRAME_NOT_FOUND  # batch.h:6
OPTIMAL_DEQUE_SIZE = 8               # main.cpp:15, mainCycle.cpp:20


class ResidentFrame(np.ndarray):
    """A frame in host memory (the reference's cv::Mat, read for point colours)
    that also lives in HBM: GpuOps.ingest uploads it once.  Frames are never
    written after decoding, so the pipeline passes them on as the reference
    passes cv::Mat (a shallow, shared copy), not as deep copies."""

    def __array_finalize__(self, obj):
        self._dev = getattr(obj, "_dev", None)
        self.fast_kps = getattr(obj, "fast_kps", None)
        self.seq = getattr(obj, "seq", None)      # (sequence tensor, index): DeviceMedia frames
        self.host_valid = getattr(obj, "host_valid", True)   # False: the pixels live in HBM only

    @property
    def dev(self):
        """the frame's HBM copy; for a DeviceMedia frame the view of its sequence,
        made on first use (a batch of consecutive frames is used as one range,
        device_frames, and never needs the per-frame views)"""
        d = self._dev
        if d is None and self.seq is not None:
            d = self._dev = self.seq[0][self.seq[1]]
        return d

    @dev.setter
    def dev(self, v):
        self._dev = v

    @property
    def resident(self):
        return self._dev is not None or self.seq is not None


def device_frames(frames):
    """the HBM copies of `frames` as one (n, h, w, 3) tensor: a view when they
    are consecutive frames of one DeviceMedia sequence (a batch whose filter
    skipped nothing), else a stacked copy.  Returns (tensor, stacked)."""
    import torch
    seqs = [getattr(f, "seq", None) for f in frames]
    if frames and all(q is not None and q[0] is seqs[0][0] for q in seqs):
        i0 = seqs[0][1]
        if all(q[1] == i0 + k for k, q in enumerate(seqs)):
            return seqs[0][0][i0:i0 + len(frames)], False
    return torch.stack([f.dev for f in frames]), True


class KltParams:
    """slam_main(tracker="klt"): the arguments of cv::calcOpticalFlowPyrLK every
    search tracks with (OpenCV's defaults)."""

    def __init__(self, win=(21, 21), max_level=3, criteria=(30, 0.01), min_eig=1e-4):
        self.win = (int(win[0]), int(win[1]))
        self.max_level = int(max_level)
        self.criteria = (int(criteria[0]), float(criteria[1]))
        self.min_eig = float(min_eig)


REPLENISH_DISTANCE = 7     # a FAST keypoint joins a tracked frame's features if farther than this from every survivor


def _xy(kps):
    return np.stack([kps["x"], kps["y"]], 1).astype(np.float32) if len(kps) else np.zeros((0, 2), np.float32)


def tracked_features(next_pts, status, err, fast_kps, shape):
    """tracker="klt": a winner's features and matches from its track (host only).
    Survivors are the points with status == 1 whose position lies in the frame
    (0 <= x <= w - 1, 0 <= y <= h - 1: the point colours are read there).  The
    features are the survivors in query order (pt = the tracked position; size,
    angle, octave and class_id as FAST writes them, response 0), followed by the
    frame's own FAST keypoints, in raster order, whose pixel is farther than
    REPLENISH_DISTANCE (Chebyshev) from every survivor's rounded position.  The
    matches are (queryIdx = index in the previous features, trainIdx = rank among
    the survivors, distance = err)."""
    h, w = int(shape[0]), int(shape[1])
    p = np.asarray(next_pts, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        ok = (np.asarray(status) == 1) & (p[:, 0] >= 0) & (p[:, 0] <= w - 1) & (p[:, 1] >= 0) & (p[:, 1] <= h - 1)
    q = np.nonzero(ok)[0]
    surv = np.zeros(len(q), KEYPOINT_DTYPE)
    surv["x"], surv["y"] = p[q, 0], p[q, 1]
    surv["size"], surv["angle"], surv["class_id"] = 7.0, -1.0, -1
    # pixels within the distance of a survivor: a 2-D difference array of the (clipped) squares
    d = REPLENISH_DISTANCE
    rx, ry = np.rint(p[q, 0]).astype(np.int64), np.rint(p[q, 1]).astype(np.int64)
    acc = np.zeros((h + 1, w + 1), np.int32)
    x0, x1 = np.clip(rx - d, 0, w), np.clip(rx + d + 1, 0, w)
    y0, y1 = np.clip(ry - d, 0, h), np.clip(ry + d + 1, 0, h)
    np.add.at(acc, (y0, x0), 1)
    np.add.at(acc, (y0, x1), -1)
    np.add.at(acc, (y1, x0), -1)
    np.add.at(acc, (y1, x1), 1)
    near = acc.cumsum(0).cumsum(1)[:h, :w] > 0
    fast_kps = np.asarray(fast_kps, KEYPOINT_DTYPE)
    fresh = fast_kps[~near[fast_kps["y"].astype(np.int64), fast_kps["x"].astype(np.int64)]] if len(fast_kps) else fast_kps
    matches = np.zeros(len(q), DMATCH_DTYPE)
    matches["queryIdx"], matches["trainIdx"], matches["distance"] = q, np.arange(len(q)), np.asarray(err, np.float32)[q]
    return np.concatenate([surv, fresh]), matches


class GpuOps:
    """The product path: every numeric step on the GPU through libslamhip, with
    the frames resident in HBM.

    ingest() uploads a frame once when it leaves MediaSources; FAST runs on that
    copy (slam_fast_dev), and each findGoodFrameFromBatch search is one
    slam_batch_extract_match over the batch's device frames (search()), matched
    against the previous good frame's descriptors, which stay in HBM from the
    search that selected it (the reference recomputes them per search,
    batch.cpp:113: the same values).  Only keypoints, match lists and counts
    cross PCIe.  The host-buffer entry points (describe / match_frame) remain
    for callers that hold plain arrays."""

    def __init__(self, ctx=None, early_exit=0):
        """early_exit: 0 = every search describes and matches its whole batch in
        one device pass (the reference's multi-thread scan, batch.cpp:162-226,
        computes every candidate speculatively too); C > 0 = first-fit searches
        run tail-first in chunks of C candidates and stop at the first chunk that
        holds a qualifying candidate (the single-thread scan's break,
        batch.cpp:120-146).  The same winner, features, matches and batch
        mutations either way (tests/test_gpu_parity.py)."""
        from .api import default_context
        self.ctx = ctx or default_context()
        self.early_exit = int(early_exit)
        self.last_processed = 0   # candidates described + matched by the last search
        self._db = None
        self._qdb = None
        self._q = None          # (source device frame, descriptors in HBM, count, matcher)
        self._ba_pool = self._ba_ctx = None   # ba_async: one host thread, one context
        self._post_pool = self._pctx = None   # post_worker: one host thread, one context

    # ---- residency ---------------------------------------------------------
    @staticmethod
    def _torch():
        import torch  # device memory + streams (plumbing only)
        return torch

    def _stream(self):
        return ctypes.c_void_p(self._torch().cuda.current_stream().cuda_stream)

    def ingest(self, frame):
        if isinstance(frame, ResidentFrame) and frame.dev is not None:
            return frame
        if frame.ndim != 3 or frame.shape[2] != 3:
            return frame                # the device batch path takes BGR frames; others use host buffers
        torch = self._torch()
        f = np.ascontiguousarray(frame, np.uint8)
        dev = torch.from_numpy(f).to(torch.device("cuda", self.ctx.device))
        torch.cuda.current_stream().synchronize()
        r = f.view(ResidentFrame)
        r.dev = dev
        return r

    def undistort(self, frame, K, dist, newK=None, lens_model=None):
        """cv::undistort of a frame at the batch.cpp:244 seam, on its resident
        copy (slam_undistort_batch): a ResidentFrame whose host pixels (the point
        colours are read from them) and HBM copy are the undistorted ones.
        Frames the device batch path does not take (not BGR) go through the
        host-buffer entry point.  lens_model="fisheye": cv::fisheye::undistortImage."""
        from . import api
        fisheye = _is_fisheye(lens_model)
        undistort = api.fisheyeUndistort if fisheye else api.undistort
        undistortBatch = api.fisheyeUndistortBatch if fisheye else api.undistortBatch
        frame = self.ingest(frame)
        dev = getattr(frame, "dev", None)
        if dev is None:
            return undistort(frame, K, dist, newK, ctx=self.ctx)
        out = undistortBatch(dev.unsqueeze(0), K, dist, newK, ctx=self.ctx)[0]
        r = out.cpu().numpy().view(ResidentFrame)     # the copy waits for the launch
        r.dev = out
        return r

    def undistort_points(self, kps, K, dist, P=None, criteria=(5, 0.0), lens_model=None):
        """cv::undistortPoints of a keypoint record array, its .pt read in place
        at the record stride (slam_undistort_points): (xy float32 n x 2, err
        float32 n).  Runs on the search context: call it from the thread that
        runs the searches.  lens_model="fisheye": cv::fisheye::undistortPoints."""
        from . import api
        points = api.fisheyeUndistortPoints if _is_fisheye(lens_model) else api.undistortPoints
        return points(np.ascontiguousarray(kps, KEYPOINT_DTYPE), K, dist, P, criteria, ctx=self.ctx)

    def _batches(self):
        if self._db is None:
            from .batch import DeviceBatch
            self._db, self._qdb = DeviceBatch(self.ctx), DeviceBatch(self.ctx)
        return self._db, self._qdb

    def prefetched(self, media, threshold, depth=3):
        """media whose next frames are uploaded and FAST-detected ahead of the
        pipeline on a worker thread (a context and stream of its own): the
        per-frame upload and fastExtractor leave the critical path.  Frames are
        still taken from `media` in order; each carries its FAST result."""
        return PrefetchedMedia(self, media, threshold, depth)

    # ---- fastExtractor -------------------------------------------------------
    def fast(self, frame, threshold):
        pre = getattr(frame, "fast_kps", None)
        if pre is not None and pre[0] == int(threshold):
            return pre[1].copy()                   # detected ahead (PrefetchedMedia)
        dev = getattr(frame, "dev", None)
        if dev is None:
            return fastExtractor(frame, threshold, True, ctx=self.ctx)
        return fast_dev(self.ctx, self._stream(), frame, threshold)

    # ---- findGoodFrameFromBatch (batch.cpp:59-160) on the device ---------------
    def _query(self, prev_frame, prev_holder, cond):
        """previous good frame's descriptors in HBM: kept from the search that
        selected it, else described once on the device"""
        dev = prev_frame.dev
        if self._q is not None and self._q[0] is dev and self._q[3] == cond.matcherType:
            return self._q[1], self._q[2]
        _, qdb = self._batches()
        raw = int(qdb.extract(dev.unsqueeze(0), cond.featureExtractingThreshold, cond.matcherType)[0])
        feats = qdb.keypoints(0).copy()
        # the holder keeps the frame's FAST set, or (ORB) its border-filtered part
        if len(prev_holder.allExtractedFeatures) not in (raw, len(feats)):
            raise RuntimeError("previous frame's keypoints differ from its FAST set")
        # ORB's in-place border filter (batch.cpp:113).  The holder is replaced only
        # when the contents differ: the post-search worker may be reading this
        # holder's array for its previous frame at the same time
        cur = np.asarray(prev_holder.allExtractedFeatures)
        if len(cur) != len(feats) or cur.dtype != feats.dtype or cur.tobytes() != feats.tobytes():
            prev_holder.allExtractedFeatures = feats
        q, nq = qdb.export_desc(0)
        self._q = (dev, q, nq, cond.matcherType)
        return q, nq

    def fast_batch(self, frames, threshold):
        """fillVideoFrameBatch's FAST over several resident frames in one device
        pass (slam_batch_fast): their keypoint counts, for the batch filter.
        The keypoints themselves are not copied out: a batch element's FAST set
        is recomputed (the same values) only where the pipeline reads it."""
        db, _ = self._batches()
        dev, stacked = device_frames(frames)
        if stacked:
            self._torch().cuda.current_stream().synchronize()
        # a view of the resident sequence is immutable, so the search's extraction
        # of the same view may take these results; a stacked copy is freed after
        # this call, and another stack may come back at its address
        return db.fast(dev, threshold, reuse=not stacked)

    def search(self, cond, batch, prev_frame, prev_holder):
        """the scan of batch.cpp:101-160 over the already filled batch: every
        candidate described and matched in one device pass (or, with
        early_exit, tail-first chunks until one holds the first fit), then the
        reference's selection (tail to skipFramesFromBatchHead, first fit) on the
        counts.  Returns (goodIndex, frame, features, matches) like the host
        scan, with the same batch mutations (scanned ORB candidates keep their
        border-filtered keypoints; the batch drops everything up to the winner)."""
        torch = self._torch()
        db, _ = self._batches()
        q, nq = self._query(prev_frame, prev_holder, cond)
        n, head = len(batch), cond.skipFramesFromBatchHead
        # first fit: the highest qualifying index wins, so once a tail chunk holds
        # one, no lower candidate can change the result (batch.cpp:140-141's break)
        chunk = self.early_exit if (self.early_exit > 0 and cond.useFirstFitInBatch and nq > 0) else 0
        counts = np.full(n, -1, np.int32)
        good, good_n = FRAME_NOT_FOUND, 0
        hi, lo, processed = n, 0, 0
        while True:
            lo = max(head, hi - chunk, 0) if chunk else 0
            if lo >= hi:
                break                       # nothing (left) at or above skipFramesFromBatchHead
            frames, stacked = device_frames([el.frame for el in batch[lo:hi]])
            if stacked:
                # the stack runs on torch's stream: complete before the batch kernels start
                torch.cuda.current_stream().synchronize()
            if nq > 0:
                _, mc = db.extract_match(frames, cond.featureExtractingThreshold, cond.matcherType, q, nq,
                                         cond.knnMatcherDistance)
            else:
                db.extract(frames, cond.featureExtractingThreshold, cond.matcherType)
                mc = np.zeros(hi - lo, np.int32)
            counts[lo:hi] = mc
            processed += hi - lo
            scanned = []
            for bi in range(hi - 1, max(head, lo) - 1, -1):
                scanned.append(bi)
                m = int(mc[bi - lo])
                if m >= cond.requiredMatchedPointsCount and m >= good_n:
                    good, good_n = bi, m
                    if cond.useFirstFitInBatch:
                        break
            for bi in scanned:
                batch[bi].estimated = True
                if cond.matcherType == L.ORB_BF:
                    batch[bi].features = db.keypoints(bi - lo).copy()
            if not chunk or good >= 0 or lo <= head:
                break
            hi = lo
        self.last_counts = counts        # per-candidate match counts (-1: not processed; bench checks)
        self.last_processed = processed
        if good < 0:
            return good, None, None, None
        el = batch[good]
        if nq > 0:
            k, m = db.result(good - lo, nq)                  # one sync for both
            el.features, el.matches = k.copy(), m.copy()
        else:
            el.features, el.matches = db.keypoints(good - lo).copy(), np.zeros(0, DMATCH_DTYPE)
        if len(el.features) > 0:
            qn, nqn = db.export_desc(good - lo)              # the next search's query, kept in HBM
            self._q = (el.frame.dev, qn, nqn, cond.matcherType)
        # the element leaves the batch here, so its fresh arrays are the returned copies
        out = (good, el.frame, el.features, el.matches)   # cv::Mat: shared
        del batch[:good + 1]
        return out

    # ---- tracker="klt": the candidate search without descriptors -----------------
    def track(self, prev_frame, prev_kps, frame, klt=None):
        """calcOpticalFlowPyrLK of the previous frame's keypoint positions into
        one frame: (next_pts, status, err); resident frames are tracked in HBM"""
        klt = klt or KltParams()
        a, b = getattr(prev_frame, "dev", None), getattr(frame, "dev", None)
        if a is None or b is None:
            a, b = _host_pixels(prev_frame), _host_pixels(frame)
        return calcOpticalFlowPyrLK(a, b, _xy(prev_kps), None, klt.win, klt.max_level, klt.criteria, 0, klt.min_eig,
                                    ctx=self.ctx)

    def track_search(self, cond, batch, prev_frame, prev_holder):
        """search() for tracker="klt": the previous good frame's feature positions
        tracked into every candidate in one device pass (slam_klt_track_batch_dev;
        with early_exit, tail-first chunks), a candidate's count being its number of
        status == 1 points; the reference's selection on those counts; then the
        winner's track read back and its features and matches made on the host
        (tracked_features).  Only counts cross PCIe for the other candidates."""
        torch = self._torch()
        db, _ = self._batches()
        klt = cond.tracker
        pts = _xy(prev_holder.allExtractedFeatures)
        n, head = len(batch), cond.skipFramesFromBatchHead
        chunk = self.early_exit if (self.early_exit > 0 and cond.useFirstFitInBatch and len(pts) > 0) else 0
        counts = np.full(n, -1, np.int32)
        good, good_n = FRAME_NOT_FOUND, 0
        hi, lo, processed = n, 0, 0
        prev = prev_frame.dev
        while True:
            lo = max(head, hi - chunk, 0) if chunk else 0
            if lo >= hi:
                break
            frames, stacked = device_frames([el.frame for el in batch[lo:hi]])
            if stacked:
                torch.cuda.current_stream().synchronize()
            mc = db.track(prev, frames, pts, None, klt.win, klt.max_level, klt.criteria, 0, klt.min_eig,
                          counts_only=True)[3]
            counts[lo:hi] = mc
            processed += hi - lo
            for bi in range(hi - 1, max(head, lo) - 1, -1):
                batch[bi].estimated = True
                m = int(mc[bi - lo])
                if m >= cond.requiredMatchedPointsCount and m >= good_n:
                    good, good_n = bi, m
                    if cond.useFirstFitInBatch:
                        break
            if not chunk or good >= 0 or lo <= head:
                break
            hi = lo
        self.last_counts = counts
        self.last_processed = processed
        if good < 0:
            return good, None, None, None
        el = batch[good]
        out, st, er, _ = db.track(prev, frames[good - lo:good - lo + 1], pts, None, klt.win, klt.max_level, klt.criteria,
                                  0, klt.min_eig)
        el.features, el.matches = tracked_features(out[0], st[0], er[0], el.features, el.frame.shape)
        res = (good, el.frame, el.features, el.matches)
        del batch[:good + 1]
        return res

    # ---- the other operations (host buffers: small per-frame arrays) -----------
    def describe(self, frame, kps, matcher):
        return extractDescriptor(_host_pixels(frame), kps, matcher, ctx=self.ctx)

    def match_frame(self, prev_desc, frame, kps, matcher, ratio):
        return matchFramesPairFeatures(prev_desc, _host_pixels(frame), kps, matcher, ratio, ctx=self.ctx)

    def estimate_transformation(self, p1, p2, K, use_ransac, prob, threshold, distance):
        ok, R, t, chir, _ = estimateTransformation(p1, p2, K, use_ransac, prob, threshold, distance, ctx=self.ctx)
        return ok, R, t, chir

    # the per-frame work after a search runs on one host thread with a context of
    # its own (main_cycle: the next search runs meanwhile on self.ctx); a
    # context is used by one thread at a time (include/slamhip.h)
    def _post_ctx(self):
        # a high-priority stream (SLAMHIP_POST_PRIO=0: normal): the pose work is
        # a chain of small launches each frame waits on, and the next search's
        # batch kernels run beside it on the main context
        if self._pctx is None:
            from .api import Context
            self._pctx = Context(self.ctx.device, priority=int(os.environ.get("SLAMHIP_POST_PRIO", "1")))
            sums = os.environ.get("SLAMHIP_PNP_SUMS")
            if sums is not None:
                self._pctx.set_option(L.OPT_PNP_SUMS, int(sums))
        return self._pctx

    def post_worker(self):
        if self._post_pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._post_ctx()
            self._post_pool = ThreadPoolExecutor(1, thread_name_prefix="slamhip-post")
        return self._post_pool

    def reconstruct(self, K, R1, t1, R2, t2, p1, p2):
        return reconstruct(K, R1, t1, R2, t2, p1, p2, ctx=self._post_ctx())

    def solve_pnp(self, obj, img, K):
        found, rvec, tvec, _ = solvePnPRansac(obj, img, K, None, ctx=self._post_ctx())
        return found, rvec.reshape(3), tvec.reshape(3)

    def rodrigues(self, rvec):
        return rodrigues_to_matrix(rvec)

    def ba(self, K4, ext, pts, obs_frame, obs_point, obs_xy, loss, loss_param):
        return bundle_adjust_arrays(K4, ext, pts, obs_frame, obs_point, obs_xy, loss, loss_param, ctx=self.ctx)

    def ba_async(self, K4, ext, pts, obs_frame, obs_point, obs_xy, loss, loss_param):
        """ba() started on a context of its own (its own HIP stream) from a host
        thread: the caller's next search runs on the GPU meanwhile (ctypes drops
        the GIL inside slam_ba).  Returns a future of the summary; K4 / ext /
        pts are written when it completes."""
        if self._ba_pool is None:
            from concurrent.futures import ThreadPoolExecutor
            from .api import Context
            self._ba_ctx = Context(self.ctx.device, priority=int(os.environ.get("SLAMHIP_POST_PRIO", "1")))
            self._ba_pool = ThreadPoolExecutor(1, thread_name_prefix="slamhip-ba")
        return self._ba_pool.submit(bundle_adjust_arrays, K4, ext, pts, obs_frame, obs_point, obs_xy, loss,
                                    loss_param, ctx=self._ba_ctx)

    def close(self):
        if self._post_pool is not None:
            self._post_pool.shutdown(wait=True)
            self._post_pool = None
        if self._pctx is not None:
            self._pctx.close()
            self._pctx = None
        if self._ba_pool is not None:
            self._ba_pool.shutdown(wait=True)
            self._ba_ctx.close()
            self._ba_pool = self._ba_ctx = None


def fast_dev(ctx, stream, frame, threshold):
    """fastExtractor on a ResidentFrame's HBM copy (slam_fast_dev on `stream`)"""
    dev = frame.dev
    h, w = frame.shape[:2]
    ch = 1 if frame.ndim == 2 else frame.shape[2]
    cap = max(4096, w * h // 16)
    while True:
        out = np.empty(cap, KEYPOINT_DTYPE)   # the first n are written
        n = ctypes.c_int(0)
        rc = L.lib().slam_fast_dev(ctx.handle, stream, ctypes.c_void_p(dev.data_ptr()), w, h,
                                   w * ch, ch, int(threshold), 1, L.TYPE_9_16, L.ptr(out), cap, ctypes.byref(n))
        if rc == L.SLAM_E_CAPACITY:
            cap = n.value
            continue
        L.check(rc, ctx.handle)
        return out[:n.value].copy()


class PrefetchedMedia:
    """MediaSources read `depth` frames ahead: each frame is uploaded to HBM and
    FAST-detected on a worker thread with its own context and stream (ctypes
    releases the GIL inside the library), so getNextFrame's frame arrives
    resident with its keypoints while the pipeline's previous operations run.
    Same frames, same order, same keypoints as ingest() + fast()."""

    def __init__(self, ops, media, threshold, depth=3):
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        from .api import Context
        self.ops, self.media, self.threshold = ops, media, int(threshold)
        self.ctx = Context(ops.ctx.device)
        self.pool = ThreadPoolExecutor(1, thread_name_prefix="slamhip-media")
        self.q = deque()
        self.done = False
        self._s = None
        for _ in range(max(1, depth)):
            self._submit()

    def _submit(self):
        if self.done:
            return
        f = self.media.next_frame()           # the source is read in order, on the caller's thread
        if f is None:
            self.done = True
            return
        self.q.append(self.pool.submit(self._work, f))

    def _work(self, frame):
        if frame.ndim != 3 or frame.shape[2] != 3:
            return frame                       # host-buffer frames: nothing ahead
        torch = GpuOps._torch()
        d = torch.device("cuda", self.ctx.device)
        if self._s is None:
            self._s = torch.cuda.Stream(d)
        f = np.ascontiguousarray(frame, np.uint8)
        with torch.cuda.stream(self._s):
            dev = torch.from_numpy(f).to(d, non_blocking=False)
            r = f.view(ResidentFrame)
            r.dev = dev
            kps = fast_dev(self.ctx, ctypes.c_void_p(self._s.cuda_stream), r, self.threshold)
        self._s.synchronize()
        dev.record_stream(torch.cuda.default_stream(d))   # used on the pipeline's stream from here on
        r.fast_kps = (self.threshold, kps)
        return r

    def next_frame(self):
        if not self.q:
            return None
        r = self.q.popleft().result()
        self._submit()
        return r

    def close(self):
        self.pool.shutdown(wait=True)
        self.ctx.close()


class Conditions:
    """DataProcessingConditions (mainCycleStructures.h:21-33), filled as
    defineProcessingEnvironment does (mainCycleInternals.cpp:80-104)."""

    def __init__(self, cfg):
        g = cfg.getValue
        self.featureExtractingThreshold = int(g("featureExtractingThreshold"))
        self.threadsCount = int(g("threadsCount"))
        self.frameBatchSize = int(g("framesBatchSize"))
        self.skipFramesFromBatchHead = int(g("skipFramesFromBatchHead"))
        self.useFirstFitInBatch = bool(g("useFirstFitInBatch"))
        self.requiredExtractedPointsCount = int(g("requiredExtractedPointsCount"))
        self.requiredMatchedPointsCount = int(g("requiredMatchedPointsCount"))
        self.matcherType = getMatcherTypeIndex(cfg)
        self.useBundleAdjustment = bool(g("useBundleAdjustment"))
        self.maxProcessedFramesVectorSz = int(g("BAMaxFramesCnt"))
        self.knnMatcherDistance = float(g("knnMatcherDistance"))
        self.rpUseRansac = bool(g("RPUseRANSAC"))
        self.rpProb = float(g("RPRANSACProb"))
        self.rpThreshold = float(g("RPRANSACThreshold"))
        self.rpDistance = float(g("RPDistanceThreshold"))
        self.loss, self.lossParam = loss_from_config(cfg)
        self.tracker = None       # slam_main(tracker="klt"): the KltParams of the search


class DeviceMedia:
    """MediaSources over a sequence already decoded into HBM: `dev` (n x h x w
    x 3 uint8 tensor) and its host copy `host` (the reference reads point
    colours from the cv::Mat).  getNextFrame hands out ResidentFrames whose
    device copy is a view of the sequence, so the consecutive frames of a batch
    are one contiguous range (device_frames: no stack per search), and take(n)
    gives fillVideoFrameBatch the next n frames for one FAST pass."""

    def __init__(self, host, dev):
        if host is not None and len(host) != len(dev):
            raise ValueError("host and device sequences differ in length")
        self.host, self.dev, self.i = host, dev, 0
        # host None: frames rendered / decoded into HBM only (colours gathered there)
        self._blank = np.broadcast_to(np.zeros(1, np.uint8), tuple(dev.shape[1:])) if host is None else None

    def next_frame(self):
        if self.i >= len(self.dev):
            return None
        if self.host is not None:
            r = self.host[self.i].view(ResidentFrame)
        else:
            r = self._blank.view(ResidentFrame)
            r.host_valid = False
        r.seq = (self.dev, self.i)              # r.dev: the view, made on first use
        self.i += 1
        return r

    def take(self, n):
        out = []
        while len(out) < n:
            f = self.next_frame()
            if f is None:
                break
            out.append(f)
        return out


class JpegMedia:
    """MediaSources over JPEG files (or streams in memory) decoded on the device:
    the reference's usePhotosCycle input (cv::imread of every path that
    photosPathPattern matches) without the host decoder.  take(n) decodes the next
    files, max(n, chunk) of them, in one slam_jpeg_decode_batch_dev call into one
    resident (k, h, w, 3) tensor and hands out ResidentFrames that are views of it,
    as DeviceMedia does: the frames of a batch are one contiguous range.  The host
    copy (the reference reads point colours from the cv::Mat) is fetched once per
    chunk.  All streams must have one size and one Exif orientation, which is
    applied as cv::imread applies it (torch view operations, then one packed copy);
    a stream the decoder refuses raises SlamError, entropy faults (status bits) are
    kept in `faults` and the frame is used as decoded."""

    def __init__(self, paths_or_buffers, ops, chunk=32, parallel=False):
        self._items = list(paths_or_buffers)
        self.ops, self.chunk = ops, max(1, int(chunk))
        self.parallel = bool(parallel)      # SLAM_OPT_JPEG_SYNC auto: a lane per chunk for photos without restart markers
        self._pos = 0            # the next item to decode
        self._seq = None         # DeviceMedia over the current chunk
        self._size = None
        self._orientation = None
        self.faults = {}         # item index -> status bits

    def _decode(self, n):
        from . import api
        items = self._items[self._pos:self._pos + n]
        bufs = []
        for it in items:
            if isinstance(it, (str, os.PathLike)):
                with open(it, "rb") as f:
                    it = f.read()
            bufs.append(it)
        dev, status, orient = api.imdecode_batch(bufs, ctx=self.ops.ctx, size=self._size, parallel=self.parallel)
        for k, st in enumerate(status):
            if st < 0:
                raise L.SlamError(int(st), f"JPEG stream {self._pos + k} cannot be decoded")
            if st:
                self.faults[self._pos + k] = int(st)
        if self._size is None:
            self._size = (dev.shape[2], dev.shape[1])
            self._orientation = int(orient[0])
        if any(int(o) != self._orientation for o in orient):
            raise ValueError("JpegMedia needs one Exif orientation per sequence")
        o = self._orientation
        if o != 1:
            if o >= 5:
                dev = dev.transpose(1, 2)
            if o in (2, 6):
                dev = dev.flip(2)
            elif o in (3, 7):
                dev = dev.flip(1, 2)
            elif o in (4, 8):
                dev = dev.flip(1)
            dev = dev.contiguous()
        self._pos += len(items)
        self._seq = DeviceMedia(dev.cpu().numpy(), dev)

    def take(self, n):
        if self._seq is None or self._seq.i >= len(self._seq.dev):
            left = len(self._items) - self._pos
            if left <= 0 or n <= 0:
                return []
            self._decode(min(left, max(n, self.chunk)))
        return self._seq.take(n)

    def next_frame(self):
        f = self.take(1)
        return f[0] if f else None


class VideoMedia:
    """MediaSources over a Motion-JPEG AVI file (the reference's videoSourcePath
    input, VideoCapture::read of every frame) decoded on the device: take(n)
    decodes the next max(n, chunk) frames in one VideoCapture.read_batch straight
    from the mapped file and hands out ResidentFrames that are views of one
    contiguous resident range, as JpegMedia does; the host copy is fetched once
    per chunk.  A frame the decoder refuses raises SlamError; entropy faults are
    kept in `faults` and the frame is used as decoded."""

    def __init__(self, path, ops, chunk=32):
        from . import video
        self.ops, self.chunk = ops, max(1, int(chunk))
        self.cap = video.VideoCapture(path, ctx=ops.ctx)
        if not self.cap.isOpened():
            raise self.cap.error if self.cap.error is not None else OSError(f"cannot open {path}")
        self._seq = None
        self.faults = {}

    def _decode(self, n):
        first = int(self.cap.get(1))
        dev, status = self.cap.read_batch(n)
        for k, st in enumerate(status):
            if st < 0:
                raise L.SlamError(int(st), f"video frame {first + k} cannot be decoded")
            if st:
                self.faults[first + k] = int(st)
        self._seq = DeviceMedia(dev.cpu().numpy(), dev)

    def take(self, n):
        if self._seq is None or self._seq.i >= len(self._seq.dev):
            left = int(self.cap.get(7)) - int(self.cap.get(1))
            if left <= 0 or n <= 0:
                return []
            self._decode(min(left, max(n, self.chunk)))
        return self._seq.take(n)

    def next_frame(self):
        f = self.take(1)
        return f[0] if f else None


def media_from_config(cfg, ops, chunk=32):
    """defineMediaSources: usePhotosCycle -> JpegMedia over the sorted paths that
    photosPathPattern matches (cv::glob sorts), else VideoMedia over videoSourcePath."""
    import glob
    if cfg.getValue("usePhotosCycle"):
        return JpegMedia(sorted(glob.glob(cfg.getValue("photosPathPattern"))), ops, chunk=chunk)
    return VideoMedia(cfg.getValue("videoSourcePath"), ops, chunk=chunk)


def _is_fisheye(lens_model):
    """lens_model: None (the Brown-Conrady polynomial of cv::undistort) or "fisheye" (cv::fisheye)"""
    if lens_model not in (None, "fisheye"):
        raise ValueError('lens_model: None or "fisheye"')
    return lens_model == "fisheye"


def _lens_kw(lens_model):
    """the keyword an ops method is given for a lens model: none for the default
    one, so ops written before the fisheye model keep working"""
    return {"lens_model": lens_model} if _is_fisheye(lens_model) else {}


class UndistortedMedia:
    """Any media with cv::undistort(frame, K, dist, newK) applied where the
    reference marks the seam (batch.cpp:244, between getNextFrame and
    fastExtractor): next_frame() is ops.undistort of the inner media's frame.
    Over a DeviceMedia the whole resident sequence is undistorted in one
    slam_undistort_batch and the frames handed out are views of the result, so a
    batch's frames stay one contiguous range and take(n) keeps working (the
    attribute exists only then: fillVideoFrameBatch tests for it).
    lens_model="fisheye": cv::fisheye::undistortImage(frame, K, dist, newK)."""

    def __init__(self, media, K, dist, ops, newK=None, lens_model=None):
        self.media, self.ops = media, ops
        self.lens = _lens_kw(lens_model)
        self.K = np.array(K, np.float64)     # a copy: BA refines the pipeline's K in place
        self.dist = np.array(dist, np.float64).reshape(-1)
        self.newK = None if newK is None else np.array(newK, np.float64)
        self._seq = None
        if isinstance(media, DeviceMedia):
            from . import api
            undistortBatch = api.fisheyeUndistortBatch if self.lens else api.undistortBatch
            rest = media.dev[media.i:]
            dev = undistortBatch(rest, self.K, self.dist, self.newK, ctx=ops.ctx)
            host = dev.cpu().numpy() if media.host is not None else None
            media.i = len(media.dev)         # the inner sequence is consumed
            self._seq = DeviceMedia(host, dev)
            self.take = self._seq.take

    def next_frame(self):
        if self._seq is not None:
            return self._seq.next_frame()
        f = self.media.next_frame()
        if f is None:
            return None
        return self.ops.undistort(f, self.K, self.dist, self.newK, **self.lens)


class MediaSources:
    """MediaSources + getNextFrame (mainCycleInternals.cpp:107-120) over an
    in-memory sequence, a list of image paths (decoded with PIL, as imread
    would give BGR) or .npy frames.  Motion-JPEG video: VideoMedia."""

    def __init__(self, frames=None, paths=None):
        self._frames = list(frames) if frames is not None else []
        self._paths = list(paths) if paths is not None else []

    def next_frame(self):
        if self._frames:
            return np.ascontiguousarray(self._frames.pop(0), np.uint8)
        while self._paths:
            p = self._paths.pop(0)
            if p.endswith(".npy"):
                return np.ascontiguousarray(np.load(p), np.uint8)
            from PIL import Image
            rgb = np.asarray(Image.open(p).convert("RGB"))
            return np.ascontiguousarray(rgb[:, :, ::-1])
        return None


class PointLens:
    """slam_main(undistort="points"): the lens model the keypoints that reach
    geometry are undistorted with (cv::undistortPoints through
    ops.undistort_points) instead of the frames.  lens(kps) is (xy float32
    n x 2 in the pixels of P, valid bool n); a keypoint whose residual exceeds
    max_residual pixels (or is NaN) has no undistorted position: it lies beyond
    the fold of the lens model, or the iteration did not reach it.
    lens_model="fisheye": cv::fisheye::undistortPoints, whose rejected points
    (a NaN residual) have no undistorted position either."""

    def __init__(self, ops, K, dist, P, criteria, max_residual, lens_model=None):
        self.ops = ops
        self.lens = _lens_kw(lens_model)
        self.K = np.array(K, np.float64)       # copies: BA refines the pipeline's K in place
        self.dist = np.array(dist, np.float64).reshape(-1)
        self.P = np.array(P, np.float64)
        self.criteria = (int(criteria[0]), float(criteria[1]))
        self.max_residual = float(max_residual)

    def __call__(self, kps):
        xy, err = self.ops.undistort_points(kps, self.K, self.dist, self.P, self.criteria, **self.lens)
        return xy, err <= np.float32(self.max_residual)


def drop_invalid_matches(prev, nxt, matches):
    """undistort="points": a match with an endpoint that has no undistorted
    position leaves the list before anything reads it"""
    if nxt.lens is None or len(matches) == 0:
        return matches
    keep = prev.valid[matches["queryIdx"]] & nxt.valid[matches["trainIdx"]]
    return matches if keep.all() else matches[keep]


class TemporalImageData:
    """mainCycleStructures.h:38-45.  With a lens (PointLens) the holder also
    carries its keypoints' undistorted coordinates and their validity mask,
    computed when the features are set and again whenever they are replaced."""

    def __init__(self, lens=None):
        self.lens = lens
        # (features, undistorted xy, valid) replaced as one object: the post-search
        # worker may read a holder while the search thread replaces its features
        self._f = (np.zeros(0, KEYPOINT_DTYPE), None, None)
        if lens is not None:
            self._f = (self._f[0], np.zeros((0, 2), np.float32), np.zeros(0, bool))
        self.allMatches = np.zeros(0, DMATCH_DTYPE)
        self.rotation = None
        self.motion = None
        self.correspondSpatialPointIdx = np.zeros(0, np.int64)

    @property
    def allExtractedFeatures(self):
        return self._f[0]

    @allExtractedFeatures.setter
    def allExtractedFeatures(self, v):
        if self.lens is None:
            self._f = (v, None, None)
        else:
            xy, valid = self.lens(v)
            self._f = (v, xy, valid)

    @property
    def undistorted(self):
        """the keypoints' undistorted coordinates (n x 2 float32), None without a lens"""
        return self._f[1]

    @property
    def valid(self):
        return self._f[2]

    def snapshot(self):
        """std::vector push_back copy: vectors deep, cv::Mat shallow."""
        s = TemporalImageData(self.lens)
        f, xy, valid = self._f
        s._f = (f.copy(), xy, valid)         # the undistorted arrays are never written: shared
        s.allMatches = self.allMatches.copy()
        s.rotation = self.rotation
        s.motion = self.motion
        s.correspondSpatialPointIdx = self.correspondSpatialPointIdx.copy()
        return s


class GlobalData:
    """mainCycleStructures.h:49-54 (points as an N x 3 float64 array, colors N x 3 uint8)."""

    def __init__(self):
        # std::vector storage: rows [0, n) of a buffer grown by doubling, so a
        # push_back of a frame's new points does not copy every earlier point
        self._pts, self._npts = np.zeros((0, 3), np.float64), 0      # Point3d rows
        self._cols, self._ncols = np.zeros((0, 3), np.uint8), 0      # Vec3b (b, g, r)
        self.spatialCameraPositions = []
        self.cameraRotations = []

    @property
    def spatialPoints(self):
        return self._pts[:self._npts]

    @spatialPoints.setter
    def spatialPoints(self, v):
        self._pts = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
        self._npts = len(self._pts)

    @property
    def spatialPointsColors(self):
        return self._cols[:self._ncols]

    @spatialPointsColors.setter
    def spatialPointsColors(self, v):
        self._cols = np.ascontiguousarray(v, np.uint8).reshape(-1, 3)
        self._ncols = len(self._cols)

    @staticmethod
    def _append(buf, n, rows):
        if n + len(rows) > len(buf):
            grown = np.empty((max(2 * len(buf), n + len(rows), 1024), 3), buf.dtype)
            grown[:n] = buf[:n]
            buf = grown
        buf[n:n + len(rows)] = rows
        return buf, n + len(rows)

    def push_points(self, pts, colors):
        self._pts, self._npts = self._append(self._pts, self._npts, np.asarray(pts, np.float64).reshape(-1, 3))
        self._cols, self._ncols = self._append(self._cols, self._ncols, np.asarray(colors, np.uint8).reshape(-1, 3))


class BatchElement:
    """mainCycleStructures.h:59-64.  `lazy` = (ops, threshold): the element's
    FAST set was counted in a batched intake pass (GpuOps.fast_batch) and is
    recomputed by ops.fast on first read -- the same keypoints."""

    def __init__(self, frame, features, lazy=None):
        self.frame = frame
        self._features = features
        self._lazy = lazy
        self.matches = np.zeros(0, DMATCH_DTYPE)
        self.estimated = False

    @property
    def features(self):
        if self._features is None and self._lazy is not None:
            ops, thr = self._lazy
            self._features = ops.fast(self.frame, thr)
        return self._features

    @features.setter
    def features(self, v):
        self._features = v


def raw_output(rows, f):
    """IOmisc.cpp:88-109 rawOutput: rows of doubles, std::fixed, 12 digits."""
    for r in np.atleast_2d(np.asarray(rows, np.float64)):
        f.write(" ".join("%.12f" % v for v in r) + "\n")


class Logs:
    """openLogsStreams (IOmisc.cpp:10-25): the four result files of outputDataDir."""

    def __init__(self, out_dir):
        self.poses = self.rotations = None
        self.out_dir = out_dir
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
            self.poses = open(os.path.join(out_dir, "poses.txt"), "w")
            self.rotations = open(os.path.join(out_dir, "rotations.txt"), "w")
        self.pose_list, self.rotation_list = [], []
        self.frames = None       # slam_main(dense=...): the good frame of every logged pose
        self.obs = None          # slam_main(loops=LoopParams(close=True)): per logged pose (xy f32 n x 2, point index i64 n)

    def pose(self, R, t, frame=None):
        if self.frames is not None:
            self.frames.append(frame)
        self.pose_list.append(np.asarray(t, np.float64).reshape(3).copy())
        self.rotation_list.append(np.asarray(R, np.float64).reshape(3, 3).copy())
        if self.poses:
            raw_output(np.asarray(t, np.float64).reshape(1, 3), self.poses)
            raw_output(np.asarray(R, np.float64).reshape(3, 3), self.rotations)

    def close(self, gd):
        if self.out_dir:
            self.poses.close()
            self.rotations.close()
            with open(os.path.join(self.out_dir, "points.txt"), "w") as f:
                if len(gd.spatialPoints):
                    raw_output(gd.spatialPoints, f)
            with open(os.path.join(self.out_dir, "colors.txt"), "w") as f:
                if len(gd.spatialPointsColors):
                    raw_output(gd.spatialPointsColors, f)


def _pts(kps, idx, xy=None):
    """the coordinates of keypoints idx; xy: their undistorted coordinates, read instead of the raw ones"""
    if xy is not None:
        return np.ascontiguousarray(xy[idx], np.float32).reshape(-1, 2)
    return np.stack([kps["x"][idx], kps["y"][idx]], 1).astype(np.float32) if len(idx) else np.zeros((0, 2), np.float32)


def _colors(frame, kps):
    # frame.at<Vec3b>(pt.y, pt.x): float -> int conversion (truncation) of the keypoint coordinates
    ys, xs = kps["y"].astype(np.int64), kps["x"].astype(np.int64)
    if not getattr(frame, "host_valid", True):
        # a DeviceMedia frame without a host copy: the same pixels gathered in HBM
        import torch
        d = frame.dev
        idx = torch.from_numpy(ys * frame.shape[1] + xs).to(d.device)
        return d.reshape(-1, 3).index_select(0, idx).cpu().numpy()
    return np.asarray(frame[ys, xs]).reshape(-1, 3)


def _assign_last(dst, idx, val):
    """dst[idx[i]] = val[i] for i in order (a repeated index keeps the last value):
    each index's last position by a max-scatter of the positions, O(n)"""
    n = len(idx)
    if n == 0:
        return
    pos = np.arange(n)
    w = np.full(len(dst), -1, np.int64)
    np.maximum.at(w, idx, pos)
    last = w[idx] == pos
    dst[idx[last]] = val[last]


# ---- batch.cpp ----------------------------------------------------------------

def fill_video_frame_batch(media, cond, batch, ops):
    """batch.cpp:228-267: FAST-filtered frames appended up to frameBatchSize."""
    skipped = 0
    fast_batch = getattr(ops, "fast_batch", None)
    if fast_batch is not None and getattr(media, "take", None) is not None:
        # frames already in HBM (DeviceMedia): the frames still missing are taken
        # in order and FAST-counted in one pass; the filter and the media
        # consumption are those of the frame-by-frame loop below
        while len(batch) < cond.frameBatchSize:
            frames = media.take(cond.frameBatchSize - len(batch))
            if not frames:
                break
            counts = fast_batch(frames, cond.featureExtractingThreshold)
            for f, c in zip(frames, counts):
                if c < cond.requiredExtractedPointsCount:
                    skipped += 1
                    continue
                batch.append(BatchElement(f, None, lazy=(ops, cond.featureExtractingThreshold)))
        return skipped
    ingest = getattr(ops, "ingest", None)
    while len(batch) < cond.frameBatchSize:
        frame = media.next_frame()
        if frame is None:
            break
        if ingest is not None:
            frame = ingest(frame)       # GpuOps: the frame's one upload to HBM
        feats = ops.fast(frame, cond.featureExtractingThreshold)
        if len(feats) < cond.requiredExtractedPointsCount:
            skipped += 1
            continue
        batch.append(BatchElement(frame, feats))
    return skipped


def _host_pixels(frame):
    """the frame's host pixels; a ResidentFrame whose pixels live in HBM only
    (DeviceMedia without a host copy) has none, and raises instead of handing on
    its placeholder zeros"""
    if not getattr(frame, "host_valid", True):
        raise ValueError("frame has no host pixels (DeviceMedia without a host copy): "
                         "this operation needs host pixels or ops with a device search")
    return np.asarray(frame)


def _resident(f):
    r = getattr(f, "resident", None)
    return r if r is not None else getattr(f, "dev", None) is not None


def find_good_frame_from_batch(media, cond, batch, prev_frame, prev_holder, ops):
    """batch.cpp:59-99 + the scan of :101-160.  prev_holder.allExtractedFeatures
    is mutated in place by the descriptor step (ORB border filter), as the
    reference's std::vector<KeyPoint>& is.  Returns (goodIndex, frame, features,
    matches)."""
    fill_video_frame_batch(media, cond, batch, ops)
    n = len(batch)
    if n == 0:
        return EMPTY_BATCH, None, None, None
    resident = _resident(prev_frame) and all(_resident(el.frame) for el in batch)
    if getattr(cond, "tracker", None) is not None:
        if getattr(ops, "track_search", None) is not None and resident:
            return ops.track_search(cond, batch, prev_frame, prev_holder)
        return _track_scan(cond, batch, prev_frame, prev_holder, ops)
    if getattr(ops, "search", None) is not None and resident:
        return ops.search(cond, batch, prev_frame, prev_holder)   # GpuOps: the scan in one device pass
    # the host scan reads host pixels: a frame that lives in HBM only (DeviceMedia
    # without its host copy) cannot take this path
    for f in [prev_frame] + [el.frame for el in batch]:
        _host_pixels(f)
    feats, prev_desc = ops.describe(prev_frame, prev_holder.allExtractedFeatures, cond.matcherType)
    prev_holder.allExtractedFeatures = feats
    good, good_n = FRAME_NOT_FOUND, 0
    for bi in range(n - 1, cond.skipFramesFromBatchHead - 1, -1):
        el = batch[bi]
        el.features, el.matches = ops.match_frame(prev_desc, el.frame, el.features, cond.matcherType,
                                                  cond.knnMatcherDistance)
        el.estimated = True
        m = len(el.matches)
        if m >= cond.requiredMatchedPointsCount and m >= good_n:
            good, good_n = bi, m
            if cond.useFirstFitInBatch:
                break
    if good < 0:
        return good, None, None, None
    el = batch[good]
    out = (good, el.frame, el.features.copy(), el.matches.copy())   # cv::Mat: shared
    del batch[:good + 1]
    return out


def _track_scan(cond, batch, prev_frame, prev_holder, ops):
    """tracker="klt" on the host scan: the loop of batch.cpp:101-160 with
    ops.track(prev_frame, prev_kps, frame, klt) in place of describe + match; a
    candidate's count is its number of status == 1 points"""
    for f in [prev_frame] + [el.frame for el in batch]:
        _host_pixels(f)
    prev_kps = prev_holder.allExtractedFeatures
    good, good_n, track = FRAME_NOT_FOUND, 0, None
    for bi in range(len(batch) - 1, cond.skipFramesFromBatchHead - 1, -1):
        el = batch[bi]
        res = ops.track(prev_frame, prev_kps, el.frame, cond.tracker)
        el.estimated = True
        m = int(np.asarray(res[1]).sum())
        if m >= cond.requiredMatchedPointsCount and m >= good_n:
            good, good_n, track = bi, m, res
            if cond.useFirstFitInBatch:
                break
    if good < 0:
        return good, None, None, None
    el = batch[good]
    el.features, el.matches = tracked_features(track[0], track[1], track[2], el.features, el.frame.shape)
    out = (good, el.frame, el.features, el.matches)
    del batch[:good + 1]
    return out


# ---- mainCycleInternals.cpp ----------------------------------------------------

def find_first_good_frame(media, cond, holder, ops):
    ingest = getattr(ops, "ingest", None)
    while True:
        frame = media.next_frame()
        if frame is None:
            return None
        if ingest is not None:
            frame = ingest(frame)
        holder.allExtractedFeatures = ops.fast(frame, cond.featureExtractingThreshold)
        if len(holder.allExtractedFeatures) >= cond.requiredExtractedPointsCount:
            return frame


def key_point_coords(f1, f2, matches, xy1=None, xy2=None):
    """getKeyPointCoordsFromFramePair: (queryIdx pts of frame 1, trainIdx pts of frame 2)."""
    return _pts(f1, matches["queryIdx"], xy1), _pts(f2, matches["trainIdx"], xy2)


def compute_transformation_and_filter_points(cond, K, d0, d1, ops):
    p1, p2 = key_point_coords(d0.allExtractedFeatures, d1.allExtractedFeatures, d1.allMatches, d0.undistorted,
                              d1.undistorted)
    ok, R, t, chir = ops.estimate_transformation(p1, p2, K, cond.rpUseRansac, cond.rpProb, cond.rpThreshold,
                                                 cond.rpDistance)
    if R is None:
        raise RuntimeError("findEssentialMat returned no model for the first pair")
    d1.rotation = np.array(R, np.float64).reshape(3, 3)
    d1.motion = np.array(t, np.float64).reshape(3, 1)
    keep = np.asarray(chir, np.uint8) > 0
    return p1[keep], p2[keep], keep


def refine_transformation_for_global_coords(R0, t0, d1):
    d1.motion = t0 + d1.rotation @ d1.motion
    d1.rotation = R0 @ d1.rotation


def define_features_correspond_spatial_indices(mask, second_frame, d0, d1):
    """returns the colors of the new points (mask order)"""
    d0.correspondSpatialPointIdx = np.full(len(d0.allExtractedFeatures), -1, np.int64)
    d1.correspondSpatialPointIdx = np.full(len(d1.allExtractedFeatures), -1, np.int64)
    m = d1.allMatches[np.asarray(mask, bool)]
    k = np.arange(len(m), dtype=np.int64)
    _assign_last(d0.correspondSpatialPointIdx, m["queryIdx"].astype(np.int64), k)
    _assign_last(d1.correspondSpatialPointIdx, m["trainIdx"].astype(np.int64), k)
    return _colors(second_frame, d1.allExtractedFeatures[m["trainIdx"]])


def old_spatial_points_and_new_coords(matches, prev_idx, points, new_kps, new_xy=None):
    sel = prev_idx[matches["queryIdx"]] if len(matches) else np.zeros(0, np.int64)
    keep = sel >= 0
    obj = points[sel[keep]].astype(np.float32) if keep.any() else np.zeros((0, 3), np.float32)
    img = _pts(new_kps, matches["trainIdx"][keep], new_xy) if keep.any() else np.zeros((0, 2), np.float32)
    return obj, img


def push_new_spatial_points(new_frame, new_points, gd, prev_idx, d1):
    """every match in order: a query without a point gets the match's new point
    (appended); the train keypoint takes the query's point index (queryIdx values
    are unique: one kNN match per query)."""
    d1.correspondSpatialPointIdx = np.full(len(d1.allExtractedFeatures), -1, np.int64)
    q = d1.allMatches["queryIdx"].astype(np.int64)
    t = d1.allMatches["trainIdx"].astype(np.int64)
    sid = prev_idx[q]
    new = sid < 0
    base = len(gd.spatialPoints)
    nid = base + np.arange(int(new.sum()), dtype=np.int64)
    gd.push_points(np.asarray(new_points, np.float64).reshape(-1, 3)[new],
                   _colors(new_frame, d1.allExtractedFeatures[t[new]]))
    prev_idx[q[new]] = nid
    val = sid.copy()
    val[new] = nid
    _assign_last(d1.correspondSpatialPointIdx, t, val)


class PendingBA:
    """One BA window whose solve may still be running (GpuOps.ba_async) while
    the next findGoodFrameFromBatch search runs: that search needs only the
    previous good frame (mainCycle.cpp:117-123), and the first consumer of BA's
    K / R / t / points is the PnP of the frame it returns (:155-161).  finish()
    writes the solution back in place (bundleAdjustment.cpp:153-201), moves the
    window to the global structure (mainCycle.cpp:203-210) and logs the summary,
    exactly as the synchronous sequence does."""

    def __init__(self, K, window, gd, result, K4, ext, pts, inputs, stats):
        self.K, self.window, self.gd, self.result = K, window, gd, result
        self.K4, self.ext, self.pts, self.inputs, self.stats = K4, ext, pts, inputs, stats

    def finish(self):
        summary = self.result.result() if hasattr(self.result, "result") else self.result
        K, K4, ext = self.K, self.K4, self.ext
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = K4
        for i, im in enumerate(self.window):
            im.rotation[...] = rodrigues_to_matrix(ext[i, :3])
            im.motion[...] = ext[i, 3:].reshape(3, 1)
        self.gd.spatialPoints = self.pts
        move_processed_data_to_global_struct(self.window, self.gd)
        if self.stats is not None:
            self.stats.setdefault("ba", []).append(summary)
            if self.stats.get("record_ba"):
                self.stats.setdefault("ba_io", []).append(
                    {"in": self.inputs, "out": (K4.copy(), ext.copy(), self.pts.copy())})
        return summary


def start_bundle_adjustment(K, window, gd, cond, ops, stats=None):
    """bundleAdjustment.cpp:73-129 over the processed-frames window: observations
    in AddResidualBlock order (frame, then keypoint), frame 0 held constant.
    Started on ops.ba_async when the ops have it (GpuOps), else solved here;
    PendingBA.finish() applies it.  stats["record_ba"]: keep each window's
    inputs and solution (stats["ba_io"]) for an oracle re-run on the same input."""
    K4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float64)
    ext = np.zeros((len(window), 6), np.float64)
    of, op, oxy = [], [], []
    for i, im in enumerate(window):
        ext[i, :3] = rodrigues_to_vector(im.rotation)
        ext[i, 3:] = im.motion.reshape(3)
        kps, uxy = im.allExtractedFeatures, im.undistorted
        p = np.nonzero(im.correspondSpatialPointIdx >= 0)[0]
        of.append(np.full(len(p), i, np.int32))
        op.append(im.correspondSpatialPointIdx[p].astype(np.int32))
        oxy.append((np.stack([kps["x"][p], kps["y"][p]], 1) if uxy is None else uxy[p]).astype(np.float64))
    pts = np.ascontiguousarray(gd.spatialPoints, np.float64).copy()
    of, op, oxy = np.concatenate(of), np.concatenate(op), np.concatenate(oxy).reshape(-1, 2)
    inputs = None
    if stats is not None and stats.get("record_ba"):
        inputs = dict(K4=K4.copy(), ext=ext.copy(), pts=pts.copy(), obs_frame=of, obs_point=op, obs_xy=oxy,
                      loss=cond.loss, loss_param=cond.lossParam)
    run = getattr(ops, "ba_async", None) or ops.ba
    result = run(K4, ext, pts, of, op, oxy, cond.loss, cond.lossParam)
    return PendingBA(K, list(window), gd, result, K4, ext, pts, inputs, stats)


def bundle_adjustment(K, window, gd, cond, ops, stats=None):
    """the synchronous form: solve, write back, move the window; returns the summary"""
    pending = start_bundle_adjustment(K, window, gd, cond, ops, stats)
    window.clear()
    return pending.finish()


def move_processed_data_to_global_struct(processed, gd):
    for fd in processed:
        gd.cameraRotations.append(fd.rotation.copy())
        gd.spatialCameraPositions.append(fd.motion.copy())
    processed.clear()


# ---- mainCycle.cpp -------------------------------------------------------------

def define_first_pair_frames(cond, media, batch, deque, ops, keep_first=False):
    first = find_first_good_frame(media, cond, deque[0], ops)
    if first is None:
        return EMPTY_BATCH, None
    while True:
        idx, frame, feats, matches = find_good_frame_from_batch(media, cond, batch, first, deque[0], ops)
        if idx == EMPTY_BATCH:
            return EMPTY_BATCH, None
        if idx >= 0:
            deque[1].allExtractedFeatures = feats
            deque[1].allMatches = drop_invalid_matches(deque[0], deque[1], matches)
            if keep_first:
                deque[0].first_frame = first     # the frame of the pair's first pose (slam_main(dense=...))
            return idx, frame
        first = batch[0].frame
        deque[0].allExtractedFeatures = batch[0].features.copy()
        del batch[0]


def processing_first_pair_frames(media, K, cond, batch, deque, gd, logs, ops):
    idx, second = define_first_pair_frames(cond, media, batch, deque, ops, keep_first=logs.frames is not None)
    if idx == EMPTY_BATCH:
        return EMPTY_BATCH, None
    p1, p2, mask = compute_transformation_and_filter_points(cond, K, deque[0], deque[1], ops)
    refine_transformation_for_global_coords(deque[0].rotation, deque[0].motion, deque[1])
    pts = ops.reconstruct(K, deque[0].rotation, deque[0].motion, deque[1].rotation, deque[1].motion, p1, p2)
    colors = define_features_correspond_spatial_indices(mask, second, deque[0], deque[1])
    gd.push_points(pts, colors)
    return idx, second


def main_cycle(media, K, cond, deque, gd, logs, ops, stats=None):
    batch = []
    processed = []
    idx, last_good = processing_first_pair_frames(media, K, cond, batch, deque, gd, logs, ops)
    if idx == EMPTY_BATCH:
        return EMPTY_BATCH
    processed.append(deque[0].snapshot())
    processed.append(deque[1].snapshot())
    logs.pose(deque[0].rotation, deque[0].motion, getattr(deque[0], "first_frame", None))
    logs.pose(deque[1].rotation, deque[1].motion, last_good)
    # loop closing: the frame data of every logged pose, read when their point indices are final (a frame's
    # after the next frame's push_new_spatial_points, which fills them in place; the last frame's at the end)
    logged = [deque[0], deque[1]] if logs.obs is not None else None

    last = 1
    bidx = FRAME_NOT_FOUND
    pending = None          # the last window's BA, solving while the next search runs
    # GpuOps: the work after a search (BA write-back, PnP, triangulation, point
    # bookkeeping, the next BA window's start) runs on a host thread with a
    # context of its own while the main thread runs the NEXT search, which needs
    # only the good frame and the batch (mainCycle.cpp:117-123).  The loop's
    # exits stay where the reference takes them: a search's outcome and the
    # "< 4 correspondences" test (:150-153, which reads correspondence indices
    # only) are decided on this thread before the next search starts, so no
    # search runs that the reference would not run.
    worker = getattr(ops, "post_worker", None)
    worker = worker() if worker is not None else None
    inflight = None

    def post_search(pending, prev, nxt, frame):
        """mainCycle.cpp:128-210 for one good frame; returns the BA window it
        started (or None)"""
        if pending is not None:
            pending.finish()            # K / R / t / points before PnP reads them
        obj, img = old_spatial_points_and_new_coords(nxt.allMatches, prev.correspondSpatialPointIdx,
                                                     gd.spatialPoints, nxt.allExtractedFeatures, nxt.undistorted)
        found, rvec, tvec = ops.solve_pnp(obj, img, K)
        nxt.motion = np.asarray(tvec, np.float64).reshape(3, 1).copy()
        nxt.rotation = ops.rodrigues(rvec)
        logs.pose(nxt.rotation, nxt.motion, frame)
        if logged is not None:
            logged.append(nxt)

        p1, p2 = key_point_coords(prev.allExtractedFeatures, nxt.allExtractedFeatures, nxt.allMatches,
                                  prev.undistorted, nxt.undistorted)
        new_points = ops.reconstruct(K, prev.rotation, prev.motion, nxt.rotation, nxt.motion, p1, p2)
        push_new_spatial_points(frame, new_points, gd, prev.correspondSpatialPointIdx, nxt)

        processed.append(nxt.snapshot())
        if len(processed) >= cond.maxProcessedFramesVectorSz:
            if cond.useBundleAdjustment:
                started = start_bundle_adjustment(K, processed, gd, cond, ops, stats)
                processed.clear()
                return started
            move_processed_data_to_global_struct(processed, gd)
        return None

    def too_few(prev, matches):
        # PnP's "< 4 correspondences" exit (mainCycle.cpp:150-153)
        return len(matches) == 0 or int((prev.correspondSpatialPointIdx[matches["queryIdx"]] >= 0).sum()) < 4

    # With the worker, each good frame's task is queued behind the previous
    # frame's post-search work on the one worker thread, which decides the
    # frame's "< 4" exit as soon as that work is done and goes straight on to
    # this frame's (no round trip through this thread); this thread waits only
    # for the decision before it starts the next search.
    wstate = {"pending": None}

    def checked_post(prev, nxt, frame, decided, verdict):
        try:
            if "error" in wstate:            # an earlier frame's work failed: stop with its error
                raise wstate["error"]
            verdict["stop"] = too_few(prev, nxt.allMatches)
        finally:
            decided.set()
        if not verdict["stop"]:
            p, wstate["pending"] = wstate["pending"], None
            try:
                wstate["pending"] = post_search(p, prev, nxt, frame)
            except BaseException as e:
                wstate["error"] = e
                raise

    try:
        while True:
            nxt, prev = deque[last + 1], deque[last]
            bidx, frame, feats, matches = find_good_frame_from_batch(media, cond, batch, last_good, prev, ops)
            if bidx == EMPTY_BATCH or bidx == FRAME_NOT_FOUND:
                break
            nxt.allExtractedFeatures = feats
            nxt.allMatches = matches = drop_invalid_matches(prev, nxt, matches)
            if worker is not None:
                decided, verdict = threading.Event(), {}
                fut = worker.submit(checked_post, prev, nxt, frame, decided, verdict)
                decided.wait()
                if verdict.get("stop", True):
                    fut.result()                 # (re-raises a failure of the decision itself)
                    break
                inflight = fut
            else:
                if too_few(prev, matches):
                    break
                pending = post_search(pending, prev, nxt, frame)

            last_good = frame
            if last == OPTIMAL_DEQUE_SIZE - 2:
                deque.pop(0)
                deque.append(TemporalImageData(deque[0].lens))
            else:
                last += 1
            if stats is not None:
                stats["frames"] = stats.get("frames", 0) + 1
    finally:
        if inflight is not None:
            inflight.result()                    # FIFO worker: every queued task is done after the last
        if worker is not None:
            pending = wstate["pending"]

    if pending is not None:             # a loop exit right after a window (PnP's < 4 points)
        pending.finish()
    if logged is not None:
        for d in logged:
            kps = d.allExtractedFeatures
            idx = getattr(d, "correspondSpatialPointIdx", None)
            if idx is None or len(idx) != len(kps):      # a frame whose points were never pushed
                idx = np.full(len(kps), -1, np.int64)
            logs.obs.append((np.stack([kps["x"], kps["y"]], 1).astype(np.float32).reshape(-1, 2),
                             np.asarray(idx, np.int64).copy()))
    if processed:
        if cond.useBundleAdjustment:
            bundle_adjustment(K, processed, gd, cond, ops, stats)
        else:
            move_processed_data_to_global_struct(processed, gd)
    if bidx == EMPTY_BATCH:
        return EMPTY_BATCH
    return last


def define_camera_position(old_deque, last_id, fd):
    """mainCycleInternals.cpp:123-134."""
    if last_id < 0 or not old_deque:
        fd.rotation = np.eye(3)
        fd.motion = np.zeros((3, 1))
    else:
        fd.rotation = old_deque[last_id].rotation.copy()
        fd.motion = old_deque[last_id].motion.copy()


def slam_main(media, K, cfg, ops=None, out_dir=None, stats=None, dist=None, newK=None, undistort="frames",
              criteria=(50, 0.01), max_residual=0.01, tracker=None, klt=None, lens_model=None, dense=None, loops=None, surface=None):
    """src/main.cpp:71-107 slamMain: mainCycle restarts from the last pose until
    the sequence ends, then points.txt / colors.txt.  K (3x3 float64) is
    updated in place by BA, as the reference's calibrationMatrix is.  dist: the
    calibration file's distortion coefficients (load_calibration(path, "DC"));
    when given and not all zero every frame is undistorted as it leaves the
    media (UndistortedMedia, the batch.cpp:244 seam; newK as cv::undistort's),
    otherwise nothing changes.

    undistort="points" takes the seam the cheap way: the frames stay raw (FAST,
    the descriptors, the candidate search and its match counts are those of a
    run without coefficients) and only the keypoints that reach geometry are
    undistorted, by cv::undistortPoints with K as it is at entry, P = newK (K
    when absent) and `criteria` = (max iterations, eps in pixels).  A keypoint
    whose residual exceeds max_residual pixels has no undistorted position; a
    winner's matches that touch one are dropped before anything reads them.  The
    essential matrix, PnP, triangulation and BA read the undistorted
    coordinates; the point colours are read from the raw frame at the raw
    coordinates, the same physical pixel.

    lens_model="fisheye" (opt-in; None is the polynomial model above) reads dist
    as the four coefficients k1 k2 k3 k4 of cv::fisheye: "frames" undistorts with
    cv::fisheye::undistortImage, "points" with cv::fisheye::undistortPoints, where
    eps of `criteria` bounds the last Newton step of the angle instead of a
    pixel error and a point OpenCV rejects has no undistorted position.

    tracker="klt" (opt-in; the reference's useFeatureTracker mode) searches
    without descriptors: the previous good frame's feature positions are tracked
    into every candidate by cv::calcOpticalFlowPyrLK with the arguments in `klt`
    (a KltParams; OpenCV's defaults when None), a candidate's count is its number
    of status == 1 points, and the reference's selection runs on those counts
    unchanged.  The winner's features are its surviving tracked positions
    followed by its own FAST keypoints away from them, its matches the tracks
    (tracked_features).  Everything downstream is untouched.  Not combined with
    dist.

    dense (opt-in; a dense.DenseParams, None changes and keeps nothing): the good
    frame of every logged pose is kept (logs.frames), and after the last cycle
    dense.densify runs plane-sweep stereo over them with the final rotations and
    positions (after BA) and the sparse cloud's depth range; the points go to
    gd.densePoints / gd.denseColors and, with out_dir, to dense_points.txt /
    dense_colors.txt in rawOutput's format.  The four result files are unchanged.
    A frame count that differs from the pose count raises.

    surface (opt-in, needs dense; a surface.SurfaceParams): the depth maps of the one
    sweep are also integrated into a TSDF volume around the sparse cloud and extracted
    by marching cubes (surface.fuse_maps); the mesh goes to gd.surfaceVertices /
    gd.surfaceColors / gd.surfaceFaces and, with out_dir, to surface.ply in
    scene.write_mesh's format.  Every other file is byte-identical with and without it.
    Without dense it raises ValueError.  With surface.texture (a surface.TextureParams)
    the mesh is also textured from the good frames (surface.texture, DESIGN.md section
    29): gd.surfaceTexture and, with out_dir, surface.obj, surface.mtl and
    surface_atlas_<p>.png (scene.write_textured_mesh); surface.ply and every other file
    stay byte-identical.

    loops (opt-in; a place.LoopParams, None keeps, computes and writes nothing): the
    good frames are kept as for dense (both may be set), and after the last cycle
    place.find_loops describes each of them (ops.fast + ops.describe with the run's
    matcher), trains a vocabulary on them or loads loops.vocabulary, builds the
    database, runs detect_loops and verifies every candidate (verify_loop), keeping
    those with at least loops.min_inliers.  The result goes to gd.loops as (i, j,
    score, n_matches, n_inliers, R, t) over the kept frames' indices and, with
    out_dir, to loops.txt: one row `i j score n_matches n_inliers R(9) t(3)` per loop
    in rawOutput's format.  The four result files are unchanged.
    loops.close (opt-in inside loops): the cycle keeps logs.obs[k] = (xy float32 n x 2, point
    index int64 n, -1 without a map point) for every logged good frame, the indices into
    the final gd.spatialPoints; after find_loops, loopclose.close_run matches every kept loop
    again, builds its Sim(3) constraint, optimises the pose graph and corrects the map.
    gd.closed holds the result (rotations, motions, points, colors, constraints, dropped,
    ...); with out_dir, poses_closed.txt, rotations_closed.txt, points_closed.txt and
    colors_closed.txt are written in rawOutput's format.  Nothing is appended to the four
    result files or to loops.txt; with no accepted loop the closed files repeat the open
    ones.  Together with tracker="klt" or undistort="points" it raises ValueError.
    loops.global_ba (opt-in, needs loops.close): globalba.refine_closed then re-fits the closed
    cameras and points to the run's observations with K constant.  gd.refined holds the result
    (rotations, motions, points, colors, summary) and gd.closed stays as it is; with out_dir,
    poses_refined.txt, rotations_refined.txt, points_refined.txt and colors_refined.txt are
    written.  With no accepted loop they repeat the closed files.  Without loops.close it
    raises ValueError.
    Returns (GlobalData, Logs)."""
    if undistort not in ("frames", "points"):
        raise ValueError('undistort: "frames" or "points"')
    if surface is not None and dense is None:
        raise ValueError("surface needs dense: the volume is fused from the sweep's depth maps")
    if tracker not in (None, "klt"):
        raise ValueError('tracker: None or "klt"')
    if tracker is not None and dist is not None:
        raise ValueError("tracker together with dist is not supported")
    close = loops is not None and getattr(loops, "close", False)
    if loops is not None and getattr(loops, "global_ba", False) and not close:
        raise ValueError("loops.global_ba needs loops.close")
    if close and (tracker is not None or undistort == "points"):
        raise ValueError('loops.close together with tracker="klt" or undistort="points" is not supported')
    if _is_fisheye(lens_model) and (dist is None or np.size(dist) != 4):
        raise ValueError('lens_model="fisheye" takes the four coefficients k1 k2 k3 k4 as dist')
    ops = ops or GpuOps()
    lens = None
    # all-zero coefficients are no lens at all in the polynomial model; in the fisheye model they are the equidistant lens
    if dist is not None and (_is_fisheye(lens_model) or np.any(np.asarray(dist, np.float64) != 0)):
        if undistort == "frames":
            media = UndistortedMedia(media, K, dist, ops, newK, lens_model)
        else:
            lens = PointLens(ops, K, dist, K if newK is None else newK, criteria, max_residual, lens_model)
    cond = Conditions(cfg)
    if tracker is not None:
        cond.tracker = klt or KltParams()
    logs = Logs(out_dir if out_dir is not None else None)
    if dense is not None or loops is not None:
        logs.frames = []
    if close:
        logs.obs = []
    gd = GlobalData()
    old, last_id = [], -1
    prefetch = getattr(ops, "prefetched", None)
    if getattr(media, "take", None) is not None:
        prefetch = None                 # DeviceMedia: the frames are resident already
    if prefetch is not None:
        media = prefetch(media, cond.featureExtractingThreshold)
    try:
        while True:
            deque = [TemporalImageData(lens) for _ in range(OPTIMAL_DEQUE_SIZE)]
            define_camera_position(old, last_id, deque[0])
            ngd = GlobalData()
            n_obs = len(logs.obs) if logs.obs is not None else 0
            last_id = main_cycle(media, K, cond, deque, ngd, logs, ops, stats)
            old = deque
            if logs.obs is not None:        # this cycle's indices refer to ngd: offset them by the earlier cycles' points
                base = len(gd.spatialPoints)
                for _, idx in logs.obs[n_obs:]:
                    idx[idx >= 0] += base
            gd.push_points(ngd.spatialPoints, ngd.spatialPointsColors)
            gd.cameraRotations += ngd.cameraRotations
            gd.spatialCameraPositions += ngd.spatialCameraPositions
            if last_id <= 0:
                break
    finally:
        if prefetch is not None:
            media.close()
    logs.close(gd)
    if dense is not None:
        from .dense import depth_maps, fuse_plan, stage_frames
        if len(logs.frames) != len(gd.cameraRotations) or len(logs.frames) != len(gd.spatialCameraPositions) \
                or any(f is None for f in logs.frames):
            raise RuntimeError(f"dense: {len(logs.frames)} good frames kept for {len(gd.cameraRotations)} final poses")
        # the sweep runs once: its maps feed the dense points and, with surface, the volume
        dctx = getattr(ops, "ctx", None)
        gd.densePoints, gd.denseColors = np.zeros((0, 3), np.float64), np.zeros((0, 3), np.uint8)
        staged = stage_frames(logs.frames, False) if len(logs.frames) >= 2 else None
        maps = None
        if staged is not None:
            maps = depth_maps(staged, K, gd.cameraRotations, gd.spatialCameraPositions, gd.spatialPoints, dense, ctx=dctx)
        if maps is not None:
            gd.densePoints, gd.denseColors = fuse_plan(staged, maps[0], maps[1], dense, ctx=dctx)
        if surface is not None:
            from . import surface as surface_mod
            if maps is None:
                res = surface_mod._empty()
            else:
                res = surface_mod.fuse_maps(staged, maps[0]["ref"], maps[1], K, gd.cameraRotations, gd.spatialCameraPositions,
                                            gd.spatialPoints, surface, ctx=dctx)
            gd.surfaceVertices, gd.surfaceColors, gd.surfaceFaces = res
            if logs.out_dir:
                from .scene import Mesh, write_mesh
                write_mesh(res[0], res[1], [Mesh(res[2], res[2])], os.path.join(logs.out_dir, "surface.ply"))
            if surface.texture is not None:
                # the good frames are still resident: every one of them is a view of the mesh
                gd.surfaceTexture = surface_mod.texture(res[0], res[1], res[2], staged if staged is not None else logs.frames, K,
                                                        gd.cameraRotations, gd.spatialCameraPositions, surface.texture, ctx=dctx)
                if logs.out_dir:
                    from .scene import write_textured_mesh
                    tx = gd.surfaceTexture
                    write_textured_mesh(os.path.join(logs.out_dir, "surface.obj"), res[0], res[2], tx.uv, tx.page, tx.atlas, ctx=dctx)
        if logs.out_dir:
            with open(os.path.join(logs.out_dir, "dense_points.txt"), "w") as f:
                if len(gd.densePoints):
                    raw_output(gd.densePoints, f)
            with open(os.path.join(logs.out_dir, "dense_colors.txt"), "w") as f:
                if len(gd.denseColors):
                    raw_output(gd.denseColors, f)
    if loops is not None:
        from .place import find_loops
        if any(f is None for f in logs.frames):
            raise RuntimeError("loops: a logged pose without its good frame")
        # operations without a device context (a CPU implementation of ops) get the host twins
        gd.loops = find_loops(logs.frames, K, cond, ops, loops, ctx=getattr(ops, "ctx", None), host=not hasattr(ops, "ctx"))
        if logs.out_dir:
            with open(os.path.join(logs.out_dir, "loops.txt"), "w") as f:
                for i, j, sc, n, inl, R, t in gd.loops:
                    raw_output(np.concatenate([[i, j, sc, n, inl], np.ravel(R), np.ravel(t)]), f)
        if close:
            from .loopclose import close_run
            if len(logs.obs) != len(logs.frames) or len(gd.cameraRotations) != len(logs.frames):
                raise RuntimeError(f"loops.close: {len(logs.obs)} observation sets and {len(gd.cameraRotations)} final poses "
                                   f"for {len(logs.frames)} good frames")
            gd.closed = close_run(gd, logs, K, cond, ops, loops, ctx=getattr(ops, "ctx", None), host=not hasattr(ops, "ctx"))
            if logs.out_dir:
                for name, rows in (("poses_closed.txt", gd.closed["motions"]), ("rotations_closed.txt", gd.closed["rotations"]),
                                   ("points_closed.txt", gd.closed["points"]), ("colors_closed.txt", gd.closed["colors"])):
                    with open(os.path.join(logs.out_dir, name), "w") as f:
                        for r in rows:
                            raw_output(r, f)
            if getattr(loops, "global_ba", False):
                from .globalba import refine_closed
                gd.refined = refine_closed(gd.closed, logs.obs, K, loops, ctx=getattr(ops, "ctx", None), host=not hasattr(ops, "ctx"))
                if logs.out_dir:
                    for name, rows in (("poses_refined.txt", gd.refined["motions"]), ("rotations_refined.txt", gd.refined["rotations"]),
                                       ("points_refined.txt", gd.refined["points"]), ("colors_refined.txt", gd.refined["colors"])):
                        with open(os.path.join(logs.out_dir, name), "w") as f:
                            for r in rows:
                                raw_output(r, f)
    return gd, logs

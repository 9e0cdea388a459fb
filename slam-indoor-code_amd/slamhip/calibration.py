"""The reference's "calibrate": true mode (mainCalibrationEntryPoint ->
chessboardPhotosCalibration, cameraCalibration.cpp:14-32, 142-203) on the device:
findChessboardCorners -> cornerSubPix over resident frames, calibrateCamera on the
host, saveCalibParametersToXML.

model="fisheye" (opt-in) calibrates cv::fisheye's lens model
instead: the growing labeller finds the bent boards, fisheyeCalibrate solves.

Out of scope: the video and webcam branches (no video decode), the preview window
and drawChessboardCorners (visualCalibration is ignored).
"""
import glob
import os
import sys

import numpy as np

from . import api
from .config import ConfigService

MINIMAL_FOUND_FRAMES_COUNT = 10      # cameraCalibration.h
SUBPIX_WIN = (11, 11)                # cameraCalibration.cpp:169-170
SUBPIX_CRITERIA = (30, 1e-4)
FISHEYE_SUBPIX_WIN = (5, 5)          # a fisheye photo's squares are a few pixels wide near the rim


class CalibrationError(RuntimeError):
    """the reference prints the message and exits (cameraCalibration.cpp:190-193)"""


def object_points(board_size, square_size):
    """getObjectPoints (cameraCalibration.cpp:71-79): row-major, z = 0"""
    bw, bh = board_size
    j, i = np.meshgrid(np.arange(bw), np.arange(bh))
    return np.stack([j.ravel() * float(square_size), i.ravel() * float(square_size), np.zeros(bw * bh)],
                    1).astype(np.float32)


def read_frame(path):
    """cv::imread's part in the calibration: a BGR (or gray) uint8 frame, or None
    for what imread would return empty.  .npy arrays are read as they are; other
    formats need PIL."""
    try:
        if str(path).lower().endswith(".npy"):
            a = np.load(path)
        else:
            from PIL import Image
            im = Image.open(path)
            a = np.asarray(im.convert("RGB"))[..., ::-1] if im.mode != "L" else np.asarray(im)
    except (OSError, EOFError, ValueError, ImportError):
        return None
    if a.dtype != np.uint8 or a.size == 0 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        return None
    return np.ascontiguousarray(a)


class DeviceOps:
    """detection on frames resident in HBM: one candidate launch per kernel for a
    batch of equally sized frames, cornerSubPix per found board on the same
    resident frame"""

    def __init__(self, ctx=None, labeller="peel", subpix_win=SUBPIX_WIN):
        self.ctx = ctx or api.default_context()
        self.labeller, self.subpix_win = labeller, tuple(subpix_win)

    def detect(self, frames, board_size):
        import torch
        dev = torch.device("cuda", self.ctx.device)
        out = [None] * len(frames)
        k = 0
        while k < len(frames):
            e = k + 1
            while e < len(frames) and frames[e].shape == frames[k].shape:
                e += 1
            batch = torch.from_numpy(np.stack(frames[k:e])).to(dev)
            found = api.findChessboardCorners(batch, board_size, ctx=self.ctx, labeller=self.labeller)
            for f, (ok, corners) in enumerate(found):
                if ok:
                    corners = api.cornerSubPix(batch[f], corners, self.subpix_win, SUBPIX_CRITERIA, ctx=self.ctx)
                out[k + f] = (ok, corners)
            k = e
        return out


def chessboard_photos_calibration(frames_or_paths, iters_count=10, square_size=23.0, board_size=(7, 7), ops=None,
                                  ctx=None, with_corners=False, decoder=None, model=None, subpix_win=None):
    """chessboardPhotosCalibration (cameraCalibration.cpp:142-203): frames (arrays or
    paths) are examined in order; empty frames and frames without a board are
    skipped; the search stops at iters_count boards; fewer than 10
    (MINIMAL_FOUND_FRAMES_COUNT) raise CalibrationError.  Returns (rms, K, D, R, T),
    with the refined corners (nviews, n, 2) appended when with_corners.
    ops: an object with detect(frames, board_size) -> [(found, refined corners)]
    (default: DeviceOps(ctx)).  decoder: None = read_frame (PIL on the host);
    "gpu" = paths ending in .jpg / .jpeg are decoded on the device (api.imread,
    byte-identical to cv::imread on baseline JPEG); other paths go to read_frame.
    model="fisheye": the boards are labelled by the growing labeller, refined in
    subpix_win (default (5, 5); (11, 11) for the default model) and the camera is
    that of api.fisheyeCalibrate, D = k1 k2 k3 k4, from Size(cols, rows)."""
    if decoder not in (None, "gpu"):
        raise ValueError("decoder is None or 'gpu'")
    if model not in (None, "fisheye"):
        raise ValueError('model is None or "fisheye"')
    fisheye = model == "fisheye"
    win = subpix_win or (FISHEYE_SUBPIX_WIN if fisheye else SUBPIX_WIN)
    ops = ops or DeviceOps(ctx, "grow" if fisheye else "peel", win)
    obj = object_points(board_size, square_size)
    image_points = []
    last = None
    items = list(frames_or_paths)
    pos = 0
    while pos < len(items) and len(image_points) < iters_count:
        # as many frames at a time as boards are still missing: none is examined after the last one needed
        frames = []
        while pos < len(items) and len(frames) < iters_count - len(image_points):
            item = items[pos]
            pos += 1
            if decoder == "gpu" and isinstance(item, (str, os.PathLike)) and str(item).lower().endswith((".jpg", ".jpeg")):
                frame = api.imread(item, ctx=ctx)
            else:
                frame = read_frame(item) if isinstance(item, (str, os.PathLike)) else item
            if frame is None or np.asarray(frame).size == 0:
                print("Empty frame", file=sys.stderr)
                continue
            frames.append(np.asarray(frame))
        for frame, (found, corners) in zip(frames, ops.detect(frames, board_size) if frames else []):
            last = frame
            if found:
                image_points.append(np.asarray(corners, np.float32))
            else:
                print("Cannot find chessboard corners")
            if len(image_points) >= iters_count:
                break
    if len(image_points) < MINIMAL_FOUND_FRAMES_COUNT:
        raise CalibrationError("Cannot detect chessboard on enough count of photos")
    # The reference passes Size(gray.rows, gray.cols) (cameraCalibration.cpp:197): width and
    # height swapped.  calibrateCamera uses the size only for the initial principal point,
    # so the quirk moves the start of the search, not the optimum; it is kept as it is.
    rows, cols = last.shape[:2]
    pts = np.stack(image_points)
    if fisheye:
        rms, K, D, R, T = api.fisheyeCalibrate(obj, pts, (cols, rows))
    else:
        rms, K, D, R, T = api.calibrateCamera(obj, pts, (rows, cols))
    return (rms, K, D, R, T, pts) if with_corners else (rms, K, D, R, T)


def main(config_path, ctx=None):
    """mainCalibrationEntryPoint (cameraCalibration.cpp:14-32): calibrate from the
    photos matching photosPathPattern and write calibrationPath.  Returns
    (rms, K, D, R, T)."""
    cfg = ConfigService()
    cfg.setConfigFile(config_path)
    if not cfg.getValue("usePhotosCycle"):
        raise NotImplementedError("calibration from a video needs video decode; set usePhotosCycle and photosPathPattern")
    files = sorted(glob.glob(cfg.getValue("photosPathPattern")))      # cv::glob sorts
    result = chessboard_photos_calibration(files, 10, ctx=ctx)
    save_calibration_path = cfg.getValue("calibrationPath")
    api.save_calibration(save_calibration_path, *result[1:])
    return result


if __name__ == "__main__":
    main(sys.argv[1])

"""Chessboard fixtures for the calibration stage: tests/golden/real_calib_boards.npz.

Provenance: the reference repository's own calibration photos,
docs/artifact/calibration/for_calib_1/*.JPG (3264 x 2448, an 8 x 8-square board:
7 x 7 inner corners, chessboardPhotosCalibration's default boardSize).  The
first ten in the order cv::glob hands them to the reference (1, 10, 11, 2 .. 8;
itersCount = 10 stops it there) are decoded with PIL convert("L"), cropped to a
multiple of 4 and area-downscaled by 4 with round half up, to 816 x 612 u8.
for_calib_2 (fisheye, beyond a 5-coefficient model) is not used.

To stay under the size limit of a committed file all ten are then cropped to one
common window that keeps every board corner (tests/calib_ref.py's detector on
the uncropped image) at least MARGIN pixels from its edge.  The file holds

  gray    10 x h x w u8   the windows
  window  x0 y0 w h       the window in the 816 x 612 image
  names   the photos' file names, in order
  full    w h             816 612

Only pixels go in: data the reference's program reads.  Run from the repository
root with the photo directory as the argument:
  python tests/golden/make_calib_fixtures.py <reference>/docs/artifact/calibration/for_calib_1
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
DOWN = 4
MARGIN = 40
BOARD = (7, 7)
LIMIT = 1 << 20


def load(path):
    from PIL import Image
    g = np.asarray(Image.open(path).convert("L"))
    h, w = g.shape[0] // DOWN * DOWN, g.shape[1] // DOWN * DOWN
    b = g[:h, :w].astype(np.uint32).reshape(h // DOWN, DOWN, w // DOWN, DOWN).sum(axis=(1, 3))
    return ((b + DOWN * DOWN // 2) // (DOWN * DOWN)).astype(np.uint8)


def main(src):
    import calib_ref as C
    names = sorted(f for f in os.listdir(src) if f.lower().endswith(".jpg"))[:10]
    imgs = [load(os.path.join(src, f)) for f in names]
    lo, hi = np.array([1 << 30, 1 << 30]), np.array([0, 0])
    for f, im in zip(names, imgs):
        found, c = C.find_chessboard(im, BOARD)
        if not found:
            raise SystemExit(f"{f}: no board")
        lo = np.minimum(lo, np.floor(c.min(0)).astype(int))
        hi = np.maximum(hi, np.ceil(c.max(0)).astype(int))
    H, W = imgs[0].shape
    x0, y0 = max(0, lo[0] - MARGIN), max(0, lo[1] - MARGIN)
    x1, y1 = min(W, hi[0] + MARGIN + 1), min(H, hi[1] + MARGIN + 1)
    gray = np.ascontiguousarray(np.stack(imgs)[:, y0:y1, x0:x1])
    out = os.path.join(HERE, "real_calib_boards.npz")
    np.savez_compressed(out, gray=gray, window=np.array([x0, y0, x1 - x0, y1 - y0], np.int32),
                        names=np.array(names), full=np.array([W, H], np.int32))
    size = os.path.getsize(out)
    print(out, gray.shape, size)
    if size > LIMIT:
        raise SystemExit("real_calib_boards.npz is above the size limit of a committed file")


if __name__ == "__main__":
    main(sys.argv[1])

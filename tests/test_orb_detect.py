"""CPU tests of the full ORB detector's definition (tests/orb_detect_ref.py) and of
the two ABI entry points' presence: the ref's self-checks, retainBest, the golden
fixture, the capability the detector adds over the upright level-0 descriptor
(matches that survive a 90 degree roll), and the exports."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import oracle_ffi as O
import orb_detect_ref as R
from slamhip import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "orb_detect_320x240.npz")
HEADER = os.path.join(ROOT, "include", "slamhip.h")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


# ---- level geometry: known answers worked out by hand ------------------------------

def test_level_sizes_kat():
    # 1.2f^l = 1, 1.2, 1.44, 1.728, 2.0736, 2.48832, 2.985984, 3.5831808 (to float precision):
    # 1920 / 1.44 = 1333.3 -> 1333; 1920 / 2.0736 = 925.9 -> 926; 1080 / 2.0736 = 520.8 -> 521;
    # 1920 / 2.48832 = 771.6 -> 772; 1080 / 2.985984 = 361.7 -> 362; 1920 / 3.5831808 = 535.8 -> 536
    assert R.level_sizes(1920, 1080, 1.2, 8) == [(1920, 1080), (1600, 900), (1333, 750), (1111, 625), (926, 521),
                                                 (772, 434), (643, 362), (536, 301)]
    # 161 / 1.2 = 134.2, 97 / 1.2 = 80.8; 161 / 1.44 = 111.8, 97 / 1.44 = 67.4; 161 / 1.728 = 93.2,
    # 97 / 1.728 = 56.1; 161 / 2.0736 = 77.6, 97 / 2.0736 = 46.8; 64.7, 39.0; 53.9, 32.5; 44.9, 27.1
    assert R.level_sizes(161, 97, 1.2, 8) == [(161, 97), (134, 81), (112, 67), (93, 56), (78, 47), (65, 39),
                                              (54, 32), (45, 27)]


def test_features_per_level_kat():
    # factor = 1 / 1.2 = 0.83333; 500 * (1 - factor) / (1 - factor^8) = 83.333 / 0.767432 = 108.59 -> 109;
    # then 90.49 -> 90, 75.41 -> 75, 62.84 -> 63, 52.37 -> 52, 43.64 -> 44, 36.37 -> 36;
    # the last level takes the rest: 500 - 469 = 31
    assert R.features_per_level(500, 1.2, 8) == [109, 90, 75, 63, 52, 44, 36, 31]
    assert R.features_per_level(500, 1.2, 1) == [500]
    # the rest is never negative: 0 features -> all zero
    assert R.features_per_level(0, 1.2, 4) == [0, 0, 0, 0]
    assert sum(R.features_per_level(40, 1.2, 8)) == 40


# ---- resize ---------------------------------------------------------------------------

def _resize_loop(img, dw, dh):
    """independent per-pixel restatement of the issue's INTER_LINEAR_EXACT passes"""
    sh, sw = img.shape

    def coef(src, dst, d):
        scale = 1.0 / (float(dst) / src)
        f = scale * (d + 0.5) - 0.5
        i = math.floor(f)
        if i < 0 or src == 1:
            return 0, 0, 256, 0
        if i >= src - 1:
            return src - 1, src - 1, 256, 0
        c1 = int(round((f - i) * 256))      # Python's round is half to even
        return i, i + 1, 256 - c1, c1

    out = np.zeros((dh, dw), np.uint8)
    for y in range(dh):
        ya, yb, cy0, cy1 = coef(sh, dh, y)
        for x in range(dw):
            xa, xb, cx0, cx1 = coef(sw, dw, x)
            h0 = int(img[ya, xa]) * cx0 + int(img[ya, xb]) * cx1
            h1 = int(img[yb, xa]) * cx0 + int(img[yb, xb]) * cx1
            out[y, x] = (h0 * cy0 + h1 * cy1 + 32768) >> 16
    return out


@pytest.mark.parametrize("src,dst", [((23, 17), (19, 14)), ((7, 5), (6, 4))])
def test_resize_matches_per_pixel_loop(src, dst):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (src[1], src[0]), dtype=np.uint8)
    assert np.array_equal(R.resize_linear_exact(img, dst[0], dst[1]), _resize_loop(img, dst[0], dst[1]))


def test_resize_identity_and_constant():
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (13, 21), dtype=np.uint8)
    assert np.array_equal(R.resize_linear_exact(img, 21, 13), img)
    for v in (0, 1, 77, 255):
        out = R.resize_linear_exact(np.full((30, 41), v, np.uint8), 34, 25)
        assert out.shape == (25, 34) and (out == v).all()


def test_pyramid_is_chained_level_to_level():
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (97, 161), dtype=np.uint8)
    lv = R.pyramid(img, 1.2, 4)
    assert [l.shape for l in lv] == [(97, 161), (81, 134), (67, 112), (56, 93)]
    assert np.array_equal(lv[2], R.resize_linear_exact(lv[1], 112, 67))
    assert not np.array_equal(lv[2], R.resize_linear_exact(lv[0], 112, 67))


# ---- umax, Harris, IC_Angle ----------------------------------------------------------------

def test_umax_table():
    assert R.derive_umax() == R.UMAX == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    # the disc is symmetric: row v is as wide as column v is tall
    um = R.UMAX
    for v in range(16):
        assert um[v] == max(u for u in range(16) if um[u] >= v)


def test_harris_flat_and_corner():
    flat = np.full((40, 40), 93, np.uint8)
    assert R.harris_responses(flat, [20], [20])[0] == 0
    corner = np.zeros((40, 40), np.uint8)
    corner[20:, 20:] = 200
    assert R.harris_responses(corner, [20], [20])[0] > 0
    # a straight edge is no corner
    edge = np.zeros((40, 40), np.uint8)
    edge[:, 20:] = 200
    assert R.harris_responses(edge, [20], [20])[0] <= 0


def test_harris_known_answer():
    # one bright pixel right of the centre row's start: worked by hand.  Image 0 except p(21, 20) = 8:
    # Ix is nonzero where the pixel is in the +-1 columns: at x = 20 (rows 19, 20, 21): +8, +16, +8;
    # at x = 22: -8, -16, -8; Iy at (x, y) = (20..22, 19): +8, +16, +8 and at y = 21: -8, -16, -8.
    # a = sum Ix^2 = 2 * (64 + 256 + 64) = 768 = b; c = sum Ix Iy = 64 - 64 - 64 + 64 = 0
    img = np.zeros((40, 40), np.uint8)
    img[20, 21] = 8
    s = np.float32(1) / np.float32(7140)
    want = (np.float32(768) * np.float32(768) - np.float32(0.04) * np.float32(1536) * np.float32(1536)) * (s * s * s * s)
    assert R.harris_responses(img, [21], [20])[0] == np.float32(want)


def test_ic_angle_rot90():
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (41, 41), dtype=np.uint8)
    img[:, 25:] //= 3                       # a clear centroid direction
    a0 = R.ic_angles(img, [20], [20])[0]
    a1 = R.ic_angles(np.ascontiguousarray(np.rot90(img)), [20], [20])[0]
    # np.rot90 turns the picture counter-clockwise: with y down the angle falls by 90
    d = (float(a0) - float(a1) - 90.0 + 180.0) % 360.0 - 180.0
    assert abs(d) <= 0.3, (a0, a1)
    # moments by hand on a one-pixel patch: a pixel at (u, v) = (3, -4) of value 10
    one = np.zeros((41, 41), np.uint8)
    one[16, 23] = 10
    m01, m10 = R.ic_moments(one, [20], [20])
    assert (m01[0], m10[0]) == (-40, 30)
    # outside the disc: (u, v) = (15, 4) is past umax[4] = 14
    out = np.zeros((41, 41), np.uint8)
    out[24, 35] = 10
    assert R.ic_moments(out, [20], [20]) == (0, 0)


# ---- retainBest ---------------------------------------------------------------------------------

def test_retain_best_ties_and_zero():
    r = np.array([5, 9, 7, 7, 3, 7, 1], np.float32)
    assert R.retain_best(r, 0).sum() == 0
    assert R.retain_best(r, 7).all() and R.retain_best(r, 20).all()
    assert R.retain_best(r, 1).tolist() == [False, True, False, False, False, False, False]
    # the cut falls inside the run of 7s: all three are kept (4 > n = 2)
    assert R.retain_best(r, 2).tolist() == [False, True, True, True, False, True, False]
    assert R.retain_best(r, 3).sum() == 4 and R.retain_best(r, 4).sum() == 4
    assert R.retain_best(r, 5).sum() == 5
    assert R.retain_best(np.array([-1.5, -0.5, -2.0], np.float32), 2).tolist() == [True, True, False]


def test_detect_level_clears_at_zero_and_skips_small():
    z = np.load(GOLDEN)["image"]
    assert len(R.detect_level(z, 0, 20, R.HARRIS_SCORE)[0]) == 0
    assert len(R.detect_level(z, 0, 20, R.FAST_SCORE)[0]) == 0
    assert len(R.detect_level(z[:62], 100, 20, R.FAST_SCORE)[0]) == 0
    assert len(R.detect_level(z[:63, :63], 100, 1, R.FAST_SCORE)[0]) <= 1     # only (31, 31) is inside the border


# ---- golden ---------------------------------------------------------------------------------------------

def test_golden_reproduced(golden):
    assert os.path.getsize(GOLDEN) < 200 * 1024
    k, d, counts = R.detect_and_compute(golden["image"], return_levels=True)
    assert counts == golden["level_counts"].tolist()
    assert k.tobytes() == golden["kps"].tobytes()
    assert np.array_equal(d, golden["desc"])
    # level ascending, raster inside a level
    key = [(int(o), float(y), float(x)) for o, y, x in zip(k["octave"], k["y"], k["x"])]
    assert key == sorted(key)
    assert (k["size"] == np.float32(31) * np.array([R.level_scale(1.2, int(o)) for o in k["octave"]])).all()


# ---- the capability: matches that survive a roll of the camera ----------------------------------------------

def _consistent(k0, d0, k1, d1, width, tol):
    """ratio-test matches (0.7, Hamming) whose train keypoint lies where np.rot90 puts the query keypoint"""
    if len(k0) == 0 or len(k1) < 2:
        return 0
    idx, dist = O.knn2(d0, d1, O.NORM_HAMMING)
    good = 0
    for m in O.ratio(idx, dist, 0.7):
        q, t = int(m["queryIdx"]), int(m["trainIdx"])
        ex, ey = float(k0["y"][q]), width - 1 - float(k0["x"][q])     # (x, y) -> (y, W - 1 - x)
        if max(abs(float(k1["x"][t]) - ex), abs(float(k1["y"][t]) - ey)) <= tol(k0[q]):
            good += 1
    return good


def test_full_orb_survives_rot90_where_upright_does_not(golden):
    img = golden["image"]
    assert img.shape[0] >= 240 and img.shape[1] >= 320
    rot = np.ascontiguousarray(np.rot90(img))
    k0, d0 = R.detect_and_compute(img)
    k1, d1 = R.detect_and_compute(rot)
    full = _consistent(k0, d0, k1, d1, img.shape[1], lambda k: 2.0 * float(R.level_scale(1.2, int(k["octave"]))))
    u0, e0 = O.orb(img, O.fast(img, 20, True))
    u1, e1 = O.orb(rot, O.fast(rot, 20, True))
    upright = _consistent(u0, e0, u1, e1, img.shape[1], lambda k: 2.0)
    print("rot90-consistent matches: full ORB", full, "of", len(k0), "; upright level-0 ORB", upright, "of", len(u0))
    assert full > upright
    assert full >= len(k0) // 2          # the oriented descriptor keeps most of them


# ---- ABI --------------------------------------------------------------------------------------------------------

def test_abi_exports_orb_detect():
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("slam_orb_detect", "slam_orb_detect_batch"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)

    def params(name):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, name
        return [" ".join(p.split()) for p in m.group(1).split(",")]

    one = params("slam_orb_detect")
    assert one == ["slam_ctx* ctx", "const uint8_t* img", "int w", "int h", "size_t step", "int channels",
                   "int nfeatures", "float scale_factor", "int nlevels", "int fast_threshold", "int score_type",
                   "slam_keypoint* kps", "int cap", "int* n_out", "uint8_t* desc"]
    many = params("slam_orb_detect_batch")
    assert many == ["slam_ctx* ctx", "void* stream", "const uint8_t* d_frames", "int nframes", "int w", "int h",
                    "int channels", "int nfeatures", "float scale_factor", "int nlevels", "int fast_threshold",
                    "int score_type", "slam_keypoint* d_kps", "int cap", "int32_t* n_out", "uint8_t* d_desc"]
    P, I, SZ, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
    assert L.SIGNATURES["slam_orb_detect"] == (I, [P, P, I, I, SZ, I, I, F, I, I, I, P, I, P, P])
    assert L.SIGNATURES["slam_orb_detect_batch"] == (I, [P, P, P, I, I, I, I, I, F, I, I, I, P, I, P, P])
    # argument errors are reported without a device: a null context first
    fn = L.lib().slam_orb_detect
    n = ctypes.c_int(-5)
    assert fn(None, None, 0, 0, 0, 1, 500, 1.2, 8, 20, 0, None, 0, ctypes.byref(n), None) == L.SLAM_E_INVALID_ARG
    import slamhip
    assert slamhip.HARRIS_SCORE == 0 and slamhip.FAST_SCORE == 1
    assert callable(slamhip.orbDetectAndCompute) and callable(slamhip.orbDetectAndComputeBatch)

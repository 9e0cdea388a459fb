"""CPU definition of the full ORB detector -- TEST INFRASTRUCTURE (the checker of
slam_orb_detect / slam_orb_detect_batch, csrc/orbdet.hip).  PARITY UNPINNED.

Restates OpenCV 4.8 features2d/src/orb.cpp ORB_Impl::detectAndCompute(img,
noArray(), kps, desc) for cv::ORB::create(nfeatures, scaleFactor, nlevels, 31, 0,
2, scoreType, 31, fastThreshold) from upstream knowledge: the image pyramid
(resize INTER_LINEAR_EXACT chained level to level), FAST-9/16 + runByImageBorder
+ retainBest per level, HarrisResponses, IC_Angle, GaussianBlur(7x7, 2) and the
256 steered bit_pattern_31_ tests.  No OpenCV is available where this project is
built, so fidelity to a real OpenCV build is NOT verified; the kernels are held
byte for byte to this restatement.

One stated deviation: the order inside a level.  OpenCV leaves whatever
std::nth_element produced; here a level's keypoints are in raster (y, x) order,
levels ascending.  Against OpenCV the contract is the set, against the kernels
the sequence.

FAST, the blur, the descriptor tests, fastAtan2 and BGR2GRAY are the existing
oracle's (orc_fast, orc_orb_blur, orc_orb_describe, orc_fast_atan2_deg,
orc_bgr2gray); everything else is numpy.
"""
import ctypes
import math

import numpy as np

import oracle_ffi as O

HARRIS_SCORE, FAST_SCORE = 0, 1
PATCH = 31
EDGE = 31
HALF_PATCH = 15
HARRIS_BLOCK = 7
HARRIS_K = np.float32(0.04)
UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]

_argtypes_set = False


def _oracle():
    global _argtypes_set
    lib = O.oracle()
    if not _argtypes_set:
        lib.orc_orb_blur.restype = None
        lib.orc_orb_blur.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.orc_orb_describe.restype = None
        lib.orc_orb_describe.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_void_p]
        _argtypes_set = True
    return lib


def cv_round(x):
    """cvRound: round half to even"""
    return int(np.rint(x))


def derive_umax(half=HALF_PATCH):
    """ORB_Impl's umax: cvRound(sqrt(r^2 - v^2)) up to vmax, then the symmetry fix-up"""
    umax = [0] * (half + 2)
    s = np.float32(half) * np.sqrt(np.float32(2.0)) / np.float32(2)
    vmax = int(math.floor(float(s + np.float32(1))))
    vmin = int(math.ceil(float(s)))
    for v in range(vmax + 1):
        umax[v] = cv_round(math.sqrt(float(half) * half - v * v))
    v0 = 0
    for v in range(half, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax[:half + 1]


def level_scale(scale_factor, level):
    """getScale: (float)pow(scaleFactor, (double)level), scaleFactor the double of the float parameter"""
    return np.float32(math.pow(float(np.float32(scale_factor)), float(level)))


def level_sizes(w, h, scale_factor, nlevels):
    out = []
    for l in range(nlevels):
        s = level_scale(scale_factor, l)
        out.append((cv_round(np.float32(w) / s), cv_round(np.float32(h) / s)))
    return out


def features_per_level(nfeatures, scale_factor, nlevels):
    sf = float(np.float32(scale_factor))
    factor = np.float32(1.0 / sf)
    nd = (np.float32(nfeatures) * (np.float32(1) - factor)
          / (np.float32(1) - np.float32(math.pow(float(factor), float(nlevels)))))
    out, total = [], 0
    for _ in range(nlevels - 1):
        n = cv_round(nd)
        out.append(n)
        total += n
        nd = np.float32(nd * factor)
    out.append(max(nfeatures - total, 0))
    return out


def resize_coeffs(src, dst):
    """per destination index: first source index and the weight (of 256) of the next one"""
    scale = 1.0 / (float(dst) / src)
    i0 = np.zeros(dst, np.int64)
    c1 = np.zeros(dst, np.int64)
    for d in range(dst):
        f = scale * (d + 0.5) - 0.5
        i = int(math.floor(f))
        if i < 0 or src == 1:
            i0[d], c1[d] = 0, 0
        elif i >= src - 1:
            i0[d], c1[d] = src - 1, 0
        else:
            i0[d], c1[d] = i, cv_round((f - i) * 256.0)
    return i0, c1


def resize_linear_exact(img, dw, dh):
    """resize(img, (dw, dh), INTER_LINEAR_EXACT) of a 1-channel 8-bit image"""
    sh, sw = img.shape
    xi, xc = resize_coeffs(sw, dw)
    yi, yc = resize_coeffs(sh, dh)
    s = img.astype(np.int64)
    xj = np.minimum(xi + 1, sw - 1)
    yj = np.minimum(yi + 1, sh - 1)
    hp = s[:, xi] * (256 - xc)[None, :] + s[:, xj] * xc[None, :]
    assert hp.max(initial=0) <= 65535
    v = hp[yi, :] * (256 - yc)[:, None] + hp[yj, :] * yc[:, None]
    return ((v + 32768) >> 16).astype(np.uint8)


def pyramid(gray, scale_factor, nlevels):
    h, w = gray.shape
    levels = [np.ascontiguousarray(gray)]
    for l, (lw, lh) in enumerate(level_sizes(w, h, scale_factor, nlevels)):
        if l == 0:
            assert (lw, lh) == (w, h)
            continue
        if lw < 1 or lh < 1:
            levels.append(np.zeros((max(lh, 0), max(lw, 0)), np.uint8))
            continue
        levels.append(np.ascontiguousarray(resize_linear_exact(levels[-1], lw, lh)))
    return levels


def retain_best(resp, n):
    """KeyPointsFilter::retainBest as a keep mask: n == 0 clears; more than n: everything >= the n-th largest"""
    resp = np.asarray(resp, np.float32)
    if n <= 0:
        return np.zeros(len(resp), bool)
    if len(resp) <= n:
        return np.ones(len(resp), bool)
    cut = np.sort(resp)[::-1][n - 1]
    return resp >= cut


def harris_responses(img, xs, ys):
    """HarrisResponses(blockSize 7, k 0.04) at integer points at least 4 px inside"""
    xs = np.asarray(xs, np.int64)
    ys = np.asarray(ys, np.int64)
    if len(xs) == 0:
        return np.zeros(0, np.float32)
    im = img.astype(np.int32)
    r = HARRIS_BLOCK // 2
    d = np.arange(-r, r + 1)
    yy = ys[:, None, None] + d[None, :, None]
    xx = xs[:, None, None] + d[None, None, :]

    def p(dy, dx):
        return im[yy + dy, xx + dx]

    ix = (p(0, 1) - p(0, -1)) * 2 + (p(-1, 1) - p(-1, -1)) + (p(1, 1) - p(1, -1))
    iy = (p(1, 0) - p(-1, 0)) * 2 + (p(1, -1) - p(-1, -1)) + (p(1, 1) - p(-1, 1))
    a = (ix * ix).sum((1, 2)).astype(np.int32)
    b = (iy * iy).sum((1, 2)).astype(np.int32)
    c = (ix * iy).sum((1, 2)).astype(np.int32)
    scale = np.float32(1) / (np.float32(4 * HARRIS_BLOCK) * np.float32(255))
    ssss = scale * scale * scale * scale
    fa, fb, fc = a.astype(np.float32), b.astype(np.float32), c.astype(np.float32)
    s = fa + fb
    return ((fa * fb - fc * fc - HARRIS_K * s * s) * ssss).astype(np.float32)


def ic_moments(img, xs, ys):
    """IC_Angle's integer moments (m01, m10) over the umax disc of half patch 15"""
    xs = np.asarray(xs, np.int64)
    ys = np.asarray(ys, np.int64)
    im = img.astype(np.int64)
    d = np.arange(-HALF_PATCH, HALF_PATCH + 1)
    um = np.array(UMAX)
    inside = np.abs(d)[None, :] <= um[np.abs(d)][:, None]      # [v][u]
    patch = im[ys[:, None, None] + d[None, :, None], xs[:, None, None] + d[None, None, :]] * inside[None]
    m10 = (patch * d[None, None, :]).sum((1, 2))
    m01 = (patch * d[None, :, None]).sum((1, 2))
    return m01.astype(np.int32), m10.astype(np.int32)


def ic_angles(img, xs, ys):
    lib = _oracle()
    m01, m10 = ic_moments(img, xs, ys)
    return np.array([lib.orc_fast_atan2_deg(float(np.float32(a)), float(np.float32(b))) for a, b in zip(m01, m10)],
                    np.float32)


def to_gray(img):
    img = np.ascontiguousarray(img)
    if img.ndim == 2:
        return img
    if img.shape[2] == 4:
        img = np.ascontiguousarray(img[:, :, :3])
    return O.gray(img)


def orb_blur(level):
    lib = _oracle()
    level = np.ascontiguousarray(level)
    out = np.zeros_like(level)
    lib.orc_orb_blur(O.vp(level), level.shape[1], level.shape[0], O.vp(out))
    return out


def orb_describe(blurred, kps):
    lib = _oracle()
    kps = np.ascontiguousarray(kps)
    desc = np.zeros((max(len(kps), 1), 32), np.uint8)
    if len(kps):
        lib.orc_orb_describe(O.vp(blurred), blurred.shape[1], blurred.shape[0], O.vp(kps), len(kps), O.vp(desc))
    return desc[:len(kps)]


def detect_level(level, n_level, fast_threshold, score_type):
    """one level's keypoints in level coordinates, raster order: (x, y, response) after both selections"""
    h, w = level.shape
    if w <= 2 * EDGE or h <= 2 * EDGE:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    k = O.fast(level, fast_threshold, True)
    x = k["x"].astype(np.int64)
    y = k["y"].astype(np.int64)
    resp = k["response"].astype(np.float32)
    inb = (x >= EDGE) & (x < w - EDGE) & (y >= EDGE) & (y < h - EDGE)
    x, y, resp = x[inb], y[inb], resp[inb]
    keep = retain_best(resp, 2 * n_level if score_type == HARRIS_SCORE else n_level)
    x, y, resp = x[keep], y[keep], resp[keep]
    if score_type == HARRIS_SCORE:
        resp = harris_responses(level, x, y)
        keep = retain_best(resp, n_level)
        x, y, resp = x[keep], y[keep], resp[keep]
    return x, y, resp


def detect_and_compute(img, nfeatures=500, scale_factor=1.2, nlevels=8, fast_threshold=20, score_type=HARRIS_SCORE,
                       return_levels=False):
    """(keypoints as O.KP, descriptors n x 32 u8); return_levels: also the per-level counts"""
    assert derive_umax() == UMAX
    gray = to_gray(img)
    levels = pyramid(gray, scale_factor, nlevels)
    per_level = features_per_level(nfeatures, scale_factor, nlevels)
    kps_all, desc_all, counts = [], [], []
    for l, level in enumerate(levels):
        x, y, resp = detect_level(level, per_level[l], fast_threshold, score_type)
        counts.append(len(x))
        if len(x) == 0:
            continue
        s = level_scale(scale_factor, l)
        k = np.zeros(len(x), O.KP)
        k["x"] = x.astype(np.float32) * s
        k["y"] = y.astype(np.float32) * s
        k["size"] = np.float32(PATCH) * s
        k["angle"] = ic_angles(level, x, y)
        k["response"] = resp
        k["octave"] = l
        k["class_id"] = -1
        inv = np.float32(1) / s
        assert np.array_equal(np.rint(k["x"] * inv).astype(np.int64), x)
        assert np.array_equal(np.rint(k["y"] * inv).astype(np.int64), y)
        lk = k.copy()
        lk["x"] = x
        lk["y"] = y
        kps_all.append(k)
        desc_all.append(orb_describe(orb_blur(level), lk))
    if kps_all:
        kps, desc = np.concatenate(kps_all), np.concatenate(desc_all)
    else:
        kps, desc = np.zeros(0, O.KP), np.zeros((0, 32), np.uint8)
    if return_levels:
        return kps, desc, counts
    return kps, desc

"""numpy restatement of cv::undistort(src, dst, K, D, newK) (OpenCV 4.8, scalar
path, uncontracted f64): the fixed-point map of initUndistortRectifyMap
(CV_16SC2 + CV_16UC1) built stripe by stripe as cv::undistort does, and
remap(INTER_LINEAR, BORDER_CONSTANT 0) on 8-bit frames.  The checker of
tests/test_undistort*.py; DESIGN.md has the contract.

Every f64 operation below is one numpy operation in the order the C++ source
evaluates it (left to right), so the values are those of a build without FMA
contraction.  The row walk `_x += ir0` is np.add.accumulate over
[start, step, step, ...]: a sequential sum, not start + j * step.

mode: "contract" (the default) or one of two deliberately wrong variants the
tests use to show that their inputs can tell the difference:
  "mul"      -- the row walk as start + j * step;
  "nostripe" -- one stripe for the whole image (s = h).
"""
import numpy as np

INT_MIN = -2 ** 31


def coefficients(dist):
    """k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]] padded with zeros to 12"""
    d = np.asarray(dist, np.float64).ravel()
    if d.size not in (4, 5, 8, 12):
        raise ValueError("4, 5, 8 or 12 distortion coefficients")
    out = np.zeros(12)
    out[:d.size] = d
    return out


def stripe_rows(w, h):
    return min(max(1, 4096 // max(w, 1)), h)


def invert3(a):
    """cv::invert's 3x3 closed form; a: 3x3 f64.  Returns the 9 entries."""
    a = np.asarray(a, np.float64)
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = [np.float64(v) for v in a.ravel()]
    d = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20)
    if d == 0:
        raise ValueError("singular new camera matrix")
    d = np.float64(1.0) / d
    return np.array([(a11 * a22 - a12 * a21) * d, (a02 * a21 - a01 * a22) * d, (a01 * a12 - a02 * a11) * d,
                     (a12 * a20 - a10 * a22) * d, (a00 * a22 - a02 * a20) * d, (a02 * a10 - a00 * a12) * d,
                     (a10 * a21 - a11 * a20) * d, (a01 * a20 - a00 * a21) * d, (a00 * a11 - a01 * a10) * d])


def cv_round(v):
    """cvRound on x86: nearest even; outside int, or NaN -> INT_MIN"""
    with np.errstate(invalid="ignore"):
        r = np.rint(v)
        ok = (r >= -2147483648.0) & (r <= 2147483647.0)
    return np.where(ok, np.where(ok, r, 0.0).astype(np.int64), INT_MIN).astype(np.int64)


def _walk(start, step, w, mode):
    if mode == "mul":
        return start + np.arange(w, dtype=np.float64) * step
    seq = np.full(w, step, np.float64)
    seq[0] = start
    return np.add.accumulate(seq)


def fixed_point(w, h, K, dist, newK=None, mode="contract"):
    """(iu, iv): cvRound(u * 32), cvRound(v * 32) per destination pixel, int64 h x w"""
    A = np.asarray(K, np.float64).reshape(3, 3)
    Ar = A if newK is None else np.asarray(newK, np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = coefficients(dist)
    fx, fy, u0, v0 = A[0, 0], A[1, 1], A[0, 2], A[1, 2]
    s = h if mode == "nostripe" else stripe_rows(w, h)
    iu = np.empty((h, w), np.int64)
    iv = np.empty((h, w), np.int64)
    one, two = np.float64(1.0), np.float64(2.0)
    with np.errstate(all="ignore"):
        for y0 in range(0, h, s):
            a = Ar.copy()
            a[1, 2] = Ar[1, 2] - y0
            ir = invert3(a)
            for i in range(min(s, h - y0)):
                fi = np.float64(i)
                _x = _walk(fi * ir[1] + ir[2], ir[0], w, mode)
                _y = _walk(fi * ir[4] + ir[5], ir[3], w, mode)
                _w = _walk(fi * ir[7] + ir[8], ir[6], w, mode)
                ww = one / _w
                x = _x * ww
                y = _y * ww
                x2 = x * x
                y2 = y * y
                r2 = x2 + y2
                _2xy = two * x * y
                kr = (one + ((k3 * r2 + k2) * r2 + k1) * r2) / (one + ((k6 * r2 + k5) * r2 + k4) * r2)
                xd = x * kr + p1 * _2xy + p2 * (r2 + two * x2) + s1 * r2 + s2 * r2 * r2
                yd = y * kr + p1 * (r2 + two * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2
                u = fx * xd + u0
                v = fy * yd + v0
                iu[y0 + i] = cv_round(u * 32.0)
                iv[y0 + i] = cv_round(v * 32.0)
    return iu, iv


def undistort_map(w, h, K, dist, newK=None, mode="contract"):
    """(xy int16 h x w x 2, frac uint16 h x w): m1 = ((short)(iu >> 5), (short)(iv >> 5))
    with the cast wrapping modulo 2^16, m2 = (iv & 31) * 32 + (iu & 31)"""
    iu, iv = fixed_point(w, h, K, dist, newK, mode)
    xy = np.stack([iu >> 5, iv >> 5], axis=-1).astype(np.uint16).view(np.int16)   # wraps
    frac = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return xy, frac


def weights():
    """the 1024 x 4 bilinear weight sets (w00, w01, w10, w11) indexed by m2"""
    m2 = np.arange(1024)
    a, b = m2 & 31, m2 >> 5
    return np.stack([(32 - b) * (32 - a) * 32, (32 - b) * a * 32, b * (32 - a) * 32, b * a * 32], axis=1)


def taps(xy, w, h):
    """validity of the four taps per map entry: (h, w, 4) bool in the order 00 01 10 11"""
    sx = xy[..., 0].astype(np.int64)
    sy = xy[..., 1].astype(np.int64)
    x0, x1 = (sx >= 0) & (sx < w), (sx + 1 >= 0) & (sx + 1 < w)
    y0, y1 = (sy >= 0) & (sy < h), (sy + 1 >= 0) & (sy + 1 < h)
    return np.stack([x0 & y0, x1 & y0, x0 & y1, x1 & y1], axis=-1)


def remap(src, xy, frac):
    """INTER_LINEAR, BORDER_CONSTANT 0 on an 8-bit h x w (gray) or h x w x c frame;
    the source has the map's size (cv::undistort)"""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    h, w = src.shape[:2]
    s = src.reshape(h, w, -1).astype(np.int64)
    sx = xy[..., 0].astype(np.int64)
    sy = xy[..., 1].astype(np.int64)
    wt = weights()[frac.astype(np.int64)]
    ok = taps(xy, w, h)
    acc = np.zeros((h, w, s.shape[2]), np.int64)
    for t, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy = np.clip(sy + dy, 0, h - 1)
        xx = np.clip(sx + dx, 0, w - 1)
        acc += s[yy, xx] * (wt[..., t] * ok[..., t])[..., None]
    out = ((acc + 16384) >> 15).astype(np.uint8)
    return out.reshape(src.shape)


def undistort(src, K, dist, newK=None, mode="contract"):
    src = np.asarray(src)
    h, w = src.shape[:2]
    xy, frac = undistort_map(w, h, K, dist, newK, mode)
    return remap(src, xy, frac)


def tie_family(w, h):
    """D = 0 and newK = K with cx, cy lowered by 1/64: every u * 32 sits on a
    half, so a last-bit difference in the row walk flips the rounding"""
    K = np.array([[517.3, 0, w / 2 + 0.37], [0, 519.1, h / 2 - 0.21], [0, 0, 1.0]])
    nk = K.copy()
    nk[0, 2] -= 1 / 64
    nk[1, 2] -= 1 / 64
    return K, nk

"""numpy restatement of cv::undistortPoints(src, dst, K, D, noArray(), P, criteria)
(OpenCV 4.8, cvUndistortPointsInternal, CV_32FC2 in and out, R absent, no tilt),
plus the per-point residual that slam_undistort_points adds.  The checker of
tests/test_undistort_points*.py; DESIGN.md section 13 has the contract.

Like tests/undistort_ref.py it is written from the OpenCV source and is not
pinned against a real OpenCV build: no OpenCV is available to the tests.

Every f64 operation below is one numpy operation in the order the C++ source
evaluates it (left to right), so the values are those of a build without FMA
contraction.  The points are independent, so the loop over j runs on the set of
points still iterating; each point sees exactly the scalar loop's operations.

Coefficients: k[0..11] = k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, zero-padded.
"""
import numpy as np

from undistort_ref import coefficients

EXIT_COUNT, EXIT_EPS, EXIT_ICDIST = 0, 1, 2
DBL_MAX = np.finfo(np.float64).max
MAX_ITER_LIMIT = 1000


def check_criteria(criteria):
    """(max_iter, eps): max_iter in 1..1000; eps = 0 is COUNT, eps > 0 COUNT|EPS.
    An EPS-only criterion (no count) is refused: OpenCV would loop forever on a
    point that never converges."""
    max_iter, eps = criteria
    if max_iter is None or int(max_iter) != max_iter or not 1 <= int(max_iter) <= MAX_ITER_LIMIT:
        raise ValueError("max_iter in 1..1000 (an EPS-only criterion is refused)")
    eps = float(eps)
    if not eps >= 0 or not np.isfinite(eps):
        raise ValueError("eps >= 0 and finite")
    return int(max_iter), eps


def _camera(K):
    A = np.asarray(K, np.float64).reshape(3, 3)
    return A[0, 0], A[1, 1], A[0, 2], A[1, 2]      # a skew entry is ignored, as OpenCV ignores it


def _reproject(x, y, k, fx, fy, cx, cy, u, v):
    """the EPS block: the forward model at (x, y), its pixel distance to (u, v)"""
    two, one = np.float64(2.0), np.float64(1.0)
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    a1 = two * x * y
    a2 = r2 + two * x * x
    a3 = r2 + two * y * y
    cdist = one + k[0] * r2 + k[1] * r4 + k[4] * r6
    icdist2 = one / (one + k[5] * r2 + k[6] * r4 + k[7] * r6)
    xd = x * cdist * icdist2 + k[2] * a1 + k[3] * a2 + k[8] * r2 + k[9] * r4
    yd = y * cdist * icdist2 + k[2] * a3 + k[3] * a1 + k[10] * r2 + k[11] * r4
    dx = xd * fx + cx - u
    dy = yd * fy + cy - v
    return np.sqrt(dx * dx + dy * dy)


def undistort_points(pts, K, dist, P=None, criteria=(5, 0.0), details=False):
    """pts: n x 2 float32 (u, v).  Returns (xy float32 n x 2, err float32 n), and
    with details=True also (exit int8 n, iterations int32 n): how each point
    left the loop and how many updates of (x, y) it made."""
    max_iter, eps = check_criteria(criteria)
    use_eps = eps > 0
    src = np.asarray(pts, np.float32).reshape(-1, 2)
    n = len(src)
    k = coefficients(dist)
    fx, fy, cx, cy = _camera(K)
    one, two = np.float64(1.0), np.float64(2.0)
    ifx = one / fx
    ify = one / fy
    RR = np.eye(3) if P is None else np.asarray(P, np.float64).reshape(3, 3)
    u = src[:, 0].astype(np.float64)
    v = src[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        x = (u - cx) * ifx
        y = (v - cy) * ify
        x0, y0 = x.copy(), y.copy()
        error = np.full(n, DBL_MAX)
        exit_ = np.full(n, EXIT_COUNT, np.int8)
        iters = np.full(n, max_iter, np.int32)
        act = np.arange(n)
        for j in range(max_iter):
            if use_eps:
                done = error[act] < eps
                exit_[act[done]] = EXIT_EPS
                iters[act[done]] = j
                act = act[~done]
            if len(act) == 0:
                break
            xa, ya, xa0, ya0 = x[act], y[act], x0[act], y0[act]
            r2 = xa * xa + ya * ya
            icdist = (one + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (one + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            neg = icdist < 0
            if neg.any():
                # the test of regression 14583: back to the start value, out of the loop
                out = act[neg]
                x[out] = (u[out] - cx) * ifx
                y[out] = (v[out] - cy) * ify
                exit_[out] = EXIT_ICDIST
                iters[out] = j
                keep = ~neg
                act, xa, ya, xa0, ya0, r2, icdist = act[keep], xa[keep], ya[keep], xa0[keep], ya0[keep], r2[keep], \
                    icdist[keep]
            deltaX = two * k[2] * xa * ya + k[3] * (r2 + two * xa * xa) + k[8] * r2 + k[9] * r2 * r2
            deltaY = k[2] * (r2 + two * ya * ya) + two * k[3] * xa * ya + k[10] * r2 + k[11] * r2 * r2
            xn = (xa0 - deltaX) * icdist
            yn = (ya0 - deltaY) * icdist
            x[act] = xn
            y[act] = yn
            if use_eps:
                error[act] = _reproject(xn, yn, k, fx, fy, cx, cy, u[act], v[act])
        err = _reproject(x, y, k, fx, fy, cx, cy, u, v).astype(np.float32)
        xx = RR[0, 0] * x + RR[0, 1] * y + RR[0, 2]
        yy = RR[1, 0] * x + RR[1, 1] * y + RR[1, 2]
        ww = one / (RR[2, 0] * x + RR[2, 1] * y + RR[2, 2])
        dst = np.stack([(xx * ww).astype(np.float32), (yy * ww).astype(np.float32)], axis=1)
    if details:
        return dst, err, exit_, iters
    return dst, err


def distort_points(xy, K, dist, newK=None, normalized=False):
    """the forward model point by point: ideal points (pixels of newK, K when
    absent, or normalised coordinates) to distorted pixels of K, f64 n x 2.
    initUndistortRectifyMap's polynomial without its row walk."""
    p = np.asarray(xy, np.float64).reshape(-1, 2)
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = coefficients(dist)
    fx, fy, cx, cy = _camera(K)
    one, two = np.float64(1.0), np.float64(2.0)
    with np.errstate(all="ignore"):
        if normalized:
            x, y = p[:, 0].copy(), p[:, 1].copy()
        else:
            nfx, nfy, ncx, ncy = _camera(K if newK is None else newK)
            x = (p[:, 0] - ncx) / nfx
            y = (p[:, 1] - ncy) / nfy
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = two * x * y
        kr = (one + ((k3 * r2 + k2) * r2 + k1) * r2) / (one + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * kr + p1 * _2xy + p2 * (r2 + two * x2) + s1 * r2 + s2 * r2 * r2
        yd = y * kr + p1 * (r2 + two * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2
        return np.stack([fx * xd + cx, fy * yd + cy], axis=1)

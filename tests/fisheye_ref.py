"""CPU definition of the fisheye lens model: the checker
of tests/test_fisheye*.py and of scripts/fisheye_bench.py.  numpy only; scipy is
imported by the solver part (fisheye_calibrate) alone.

Five parts, each the contract of one piece of the library:

  fe_atan / fe_tan                     csrc/fisheye_math.h
  distort / fisheye_map                slam_fisheye_undistort_map (csrc/fisheye.hip)
  undistort_points                     slam_fisheye_undistort_points (csrc/fisheye.hip)
  label_board_grow / find_chessboard   slam_label_chessboard_grow (csrc/calib_board.cpp)
  fisheye_calibrate                    slam_fisheye_calibrate (csrc/calib_solve.cpp)

The model restates cv::fisheye of OpenCV 4.8 (fisheye.cpp: projectPoints /
distortPoints, initUndistortRectifyMap with R = I, undistortPoints, calibrate)
from knowledge of the source; no OpenCV is available to pin it against.  Every
f64 operation is one numpy operation in the order written, i.e. the values of a
build without FMA contraction.  Stated deviations:
  * atan and tan are fe_atan and fe_tan below, not libm's: the device's and
    glibc's differ in the last place, so the contract is its own pair, a fixed
    sequence of f64 operations restated here operation for operation.
    Measured (tests/test_fisheye.py repeats both): over 2,000,001 arguments
    spread evenly over [0, pi/2] and the doubles adjacent to 0, pi/4 and pi/2,
    fe_atan is within 1 ulp of math.atan and fe_tan within 2 ulp of
    math.tan; of the 2 * 748 * 480 entries of the map of CAMERA (below), none
    differs from the map built with np.arctan.
  * the map's inverse of newK is the closed 3x3 form of csrc/undistort.hip, not
    the SVD inverse; a newK whose last row is not (0, 0, 1) is refused; the map
    is built in one piece (cv::fisheye has no stripes).
  * undistort_points takes theta_d > 1e-8 as the test for running Newton and
    scale = 1 below it, and counts an EPS criterion as in section 13: eps == 0
    is COUNT alone.  A second output holds the residual.
  * the skew is fixed at 0 everywhere, in the solver too (cv::fisheye::calibrate
    with flags = 0 estimates it).
The labeller is this project's own (as calib_ref.label_board is): every integer
and every f64 operation below is the contract.
"""
import math

import numpy as np

import calib_ref
from undistort_ref import cv_round, invert3

f64 = np.float64

# the camera fitted to tests/golden/fisheye (748 x 480): K and D of the issue's prototype
CAMERA_K = np.array([[208.08, 0, 384.53], [0, 208.11, 239.66], [0, 0, 1.0]])
CAMERA_D = np.array([-0.0360, 0.0053, -0.0084, 0.0018])

REJECTED = -1000000.0


# ---- fe_atan / fe_tan (csrc/fisheye_math.h) ---------------------------------------

AT_HI = (4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01,
         1.57079632679489655800e+00)
AT_LO = (2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17,
         6.12323399573676603587e-17)
AT = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01,
      -1.11111104054623557880e-01, 9.09088713343650656196e-02, -7.69187620504482999495e-02,
      6.66107313738753120669e-02, -5.83357013379057348645e-02, 4.97687799461593236017e-02,
      -3.65315727442169155270e-02, 1.62858201153657823623e-02)
TT = (3.33333333333334091986e-01, 1.33333333333201242699e-01, 5.39682539762260521377e-02,
      2.18694882948595424599e-02, 8.86323982359930005737e-03, 3.59207910759131235356e-03,
      1.45620945432529025516e-03, 5.88041240820264096874e-04, 2.46463134818469906812e-04,
      7.81794442939557092300e-05, 7.14072491382608190305e-05, -1.85586374855275456654e-05,
      2.59073051863633712884e-05)
PIO2_HI, PIO2_LO = AT_HI[3], AT_LO[3]
PIO4_HI, PIO4_LO = AT_HI[1], AT_LO[1]


def fe_atan(x):
    """x >= 0, elementwise; NaN propagates, inf gives pi/2"""
    x = np.asarray(x, f64)
    with np.errstate(all="ignore"):
        c0, c1, c2, c3 = x < 0.4375, x < 0.6875, x < 1.1875, x < 2.4375
        t = np.where(c0, x,
                     np.where(c1, (2.0 * x - 1.0) / (2.0 + x),
                              np.where(c2, (x - 1.0) / (x + 1.0),
                                       np.where(c3, (x - 1.5) / (1.0 + 1.5 * x), -1.0 / x))))
        k = np.where(c1, 0, np.where(c2, 1, np.where(c3, 2, 3)))
        hi = np.take(AT_HI, k)
        lo = np.take(AT_LO, k)
        z = t * t
        w = z * z
        s1 = z * (AT[0] + w * (AT[2] + w * (AT[4] + w * (AT[6] + w * (AT[8] + w * AT[10])))))
        s2 = w * (AT[1] + w * (AT[3] + w * (AT[5] + w * (AT[7] + w * AT[9]))))
        p = t * (s1 + s2)
        return np.where(c0, t - p, hi - ((p - lo) - t))


def _tan_poly(u):
    z = u * u
    w = z * z
    r = TT[1] + w * (TT[3] + w * (TT[5] + w * (TT[7] + w * (TT[9] + w * TT[11]))))
    v = z * (TT[2] + w * (TT[4] + w * (TT[6] + w * (TT[8] + w * (TT[10] + w * TT[12])))))
    s = z * u
    return u + (z * (s * (r + v)) + TT[0] * s)


def fe_tan(t):
    """t in [0, pi/2], elementwise; NaN propagates"""
    t = np.asarray(t, f64)
    with np.errstate(all="ignore"):
        big = t > PIO4_HI
        y = np.where(big, (PIO2_HI - t) + PIO2_LO, t)
        near = y >= 0.67434
        u = np.where(near, (PIO4_HI - y) + PIO4_LO, y)
        q = _tan_poly(u)
        ty = np.where(near, (1.0 - q) / (1.0 + q), q)
        return np.where(big, 1.0 / ty, ty)


# ---- the forward model and the map ------------------------------------------------

def coefficients(dist):
    d = np.asarray(dist, f64).ravel()
    if d.size != 4:
        raise ValueError("exactly 4 fisheye coefficients")
    return d


def _camera(K):
    A = np.asarray(K, f64).reshape(3, 3)
    return A[0, 0], A[1, 1], A[0, 2], A[1, 2]      # the skew is 0 by contract: the entry is ignored


def _theta_d(theta, k):
    t2 = theta * theta
    t4 = t2 * t2
    t6 = t4 * t2
    t8 = t4 * t4
    return theta * (1.0 + k[0] * t2 + k[1] * t4 + k[2] * t6 + k[3] * t8)


def distort(a, b, K, dist, atan=fe_atan):
    """the forward model at normalised (a, b) = (x / z, y / z): distorted pixels (u, v) in f64"""
    fx, fy, cx, cy = _camera(K)
    k = coefficients(dist)
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    with np.errstate(all="ignore"):
        r = np.sqrt(a * a + b * b)
        theta = atan(r)
        td = _theta_d(theta, k)
        scale = np.where(r == 0, 1.0, td / r)
        return fx * a * scale + cx, fy * b * scale + cy


def _walk(start, step, w):
    seq = np.full(w, step, f64)
    seq[0] = start
    return np.add.accumulate(seq)


def fixed_point(w, h, K, dist, newK=None, atan=fe_atan):
    """(iu, iv): cvRound(u * 32), cvRound(v * 32) per destination pixel, int64 h x w"""
    Ar = np.asarray(K if newK is None else newK, f64).reshape(3, 3)
    if Ar[2, 0] != 0 or Ar[2, 1] != 0 or Ar[2, 2] != 1:
        raise ValueError("the last row of the new camera matrix is (0, 0, 1)")
    ir = invert3(Ar)
    iu = np.empty((h, w), np.int64)
    iv = np.empty((h, w), np.int64)
    with np.errstate(all="ignore"):
        for i in range(h):
            fi = f64(i)
            _x = _walk(fi * ir[1] + ir[2], ir[0], w)
            _y = _walk(fi * ir[4] + ir[5], ir[3], w)
            _w = _walk(fi * ir[7] + ir[8], ir[6], w)
            u, v = distort(_x / _w, _y / _w, K, dist, atan)
            iu[i] = cv_round(u * 32.0)
            iv[i] = cv_round(v * 32.0)
    return iu, iv


def fisheye_map(w, h, K, dist, newK=None, atan=fe_atan):
    """(xy int16 h x w x 2, frac uint16 h x w): the layout of undistort_ref.undistort_map,
    so undistort_ref.remap consumes it unchanged"""
    iu, iv = fixed_point(w, h, K, dist, newK, atan)
    xy = np.stack([iu >> 5, iv >> 5], axis=-1).astype(np.uint16).view(np.int16)
    frac = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return xy, frac


# ---- undistortPoints ----------------------------------------------------------------

EXIT_CENTRE, EXIT_EPS, EXIT_COUNT, EXIT_NOT_CONVERGED, EXIT_FLIPPED = 0, 1, 2, 3, 4


def undistort_points(pts, K, dist, P=None, criteria=(10, 1e-8), details=False):
    """pts: n x 2 float32 (u, v).  Returns (xy float32 n x 2, err float32 n): a
    rejected point is (-1000000, -1000000) with err NaN.  details=True adds (exit
    int8 n, iterations int32 n)."""
    from undistort_points_ref import check_criteria
    max_iter, eps = check_criteria(criteria)
    use_eps = eps > 0
    src = np.asarray(pts, np.float32).reshape(-1, 2)
    n = len(src)
    k = coefficients(dist)
    fx, fy, cx, cy = _camera(K)
    RR = np.eye(3) if P is None else np.asarray(P, f64).reshape(3, 3)
    u = src[:, 0].astype(f64)
    v = src[:, 1].astype(f64)
    half_pi = f64(math.pi / 2)
    with np.errstate(all="ignore"):
        pwx = (u - cx) / fx
        pwy = (v - cy) / fy
        td = np.sqrt(pwx * pwx + pwy * pwy)
        td = np.minimum(np.maximum(-half_pi, td), half_pi)     # std::min(std::max(..)): a NaN becomes -pi/2
        td = np.where(np.isnan(pwx * pwx + pwy * pwy), -half_pi, td)
        run = td > 1e-8
        theta = td.copy()
        converged = ~run
        iters = np.zeros(n, np.int32)
        act = np.nonzero(run)[0]
        for j in range(max_iter):
            if len(act) == 0:
                break
            th = theta[act]
            t2 = th * th
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t6 * t2
            k0, k1, k2, k3 = k[0] * t2, k[1] * t4, k[2] * t6, k[3] * t8
            fix = (th * (1.0 + k0 + k1 + k2 + k3) - td[act]) / (1.0 + 3.0 * k0 + 5.0 * k1 + 7.0 * k2 + 9.0 * k3)
            theta[act] = th - fix
            iters[act] = j + 1
            if use_eps:
                done = np.abs(fix) < eps
                converged[act[done]] = True
                act = act[~done]
        scale = np.where(run, fe_tan(theta) / td, 1.0)
        flipped = ((td < 0) & (theta > 0)) | ((td > 0) & (theta < 0))
        ok = (converged | (not use_eps)) & ~flipped
        x = pwx * scale
        y = pwy * scale
        du, dv = distort(x, y, K, dist)
        dx = du - u
        dy = dv - v
        err = np.where(ok, np.sqrt(dx * dx + dy * dy), np.nan).astype(np.float32)
        xx = RR[0, 0] * x + RR[0, 1] * y + RR[0, 2]
        yy = RR[1, 0] * x + RR[1, 1] * y + RR[1, 2]
        ww = RR[2, 0] * x + RR[2, 1] * y + RR[2, 2]
        dst = np.stack([np.where(ok, xx / ww, REJECTED).astype(np.float32),
                        np.where(ok, yy / ww, REJECTED).astype(np.float32)], axis=1)
    if details:
        ex = np.where(~run, EXIT_CENTRE, np.where(converged, EXIT_EPS, EXIT_COUNT if not use_eps else EXIT_NOT_CONVERGED))
        ex = np.where(flipped, EXIT_FLIPPED, ex).astype(np.int8)
        return dst, err, ex, iters
    return dst, err


# ---- fisheye::calibrate (skew 0) ----------------------------------------------------

def project(obj, K4, D, rvec, tvec):
    """the forward model of board points under a pose, f64: (n, 2)"""
    Y = np.asarray(obj, f64) @ calib_ref.rodrigues(rvec).T + np.asarray(tvec, f64)
    K = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])
    u, v = distort(Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2], K, D)
    return np.stack([u, v], 1)


def initial_values(obj, img, size):
    """OpenCV's start: f = max(w, h) / pi, the principal point at the centre, D = 0,
    poses from the homographies board -> normalised coordinates of the points
    undistorted with D = 0 (theta = |pw|, held below 1.5): (8 intrinsics, rvecs, tvecs)"""
    obj = np.asarray(obj, f64)
    img = np.asarray(img, f64)
    f0 = max(size) / math.pi
    cx, cy = (size[0] - 1) / 2, (size[1] - 1) / 2
    rv, tv = [], []
    for view in img:
        pw = (view - [cx, cy]) / f0
        th = np.linalg.norm(pw, axis=1)
        sc = np.where(th > 1e-9, fe_tan(np.minimum(th, 1.5)) / np.maximum(th, 1e-9), 1.0)
        M = calib_ref._homography(obj[:, :2], pw * sc[:, None])
        if M[2, 2] < 0:
            M = -M
        lam = 1 / np.linalg.norm(M[:, 0])
        r1, r2, t = M[:, 0] * lam, M[:, 1] * lam, M[:, 2] * lam
        U, _, Vt = np.linalg.svd(np.stack([r1, r2, np.cross(r1, r2)], 1))
        rv.append(calib_ref.rodrigues_inv(U @ Vt))
        tv.append(t)
    return np.array([f0, f0, cx, cy, 0, 0, 0, 0.0]), np.array(rv), np.array(tv)


def residuals(p, obj, img):
    n = len(img)
    r = [project(obj, p[:4], p[4:8], p[8 + 6 * v:11 + 6 * v], p[11 + 6 * v:14 + 6 * v]) - img[v] for v in range(n)]
    return np.concatenate(r).ravel()


def cost(obj, img, K4, D, rvecs, tvecs):
    """sum of squared reprojection residuals in f64 (rms^2 * nviews * npts)"""
    p = np.concatenate([np.asarray(K4, f64).ravel(), np.asarray(D, f64).ravel()[:4]] +
                       [np.r_[np.ravel(r), np.ravel(t)] for r, t in zip(rvecs, tvecs)])
    r = residuals(p, np.asarray(obj, f64), np.asarray(img, f64))
    return float(r @ r)


def fisheye_calibrate(obj, img, size, tol=1e-15):
    """the optimum of fisheye::calibrate's model with the skew fixed at 0, by scipy's
    least_squares from initial_values: (rms, K 3x3, D 4, rvecs, tvecs, cost); rms as
    slam_calibrate_camera defines it"""
    from scipy.optimize import least_squares
    obj = np.asarray(obj, f64)
    img = np.asarray(img, f64)
    k0, rv, tv = initial_values(obj, img, size)
    p0 = np.concatenate([k0] + [np.r_[r, t] for r, t in zip(rv, tv)])
    sol = least_squares(residuals, p0, args=(obj, img), method="lm", x_scale="jac", xtol=tol, ftol=tol, gtol=tol,
                        max_nfev=20000)
    p = sol.x
    n = len(img)
    c = float(sol.fun @ sol.fun)
    K = np.array([[p[0], 0, p[2]], [0, p[1], p[3]], [0, 0, 1]])
    ext = p[8:].reshape(n, 6)
    return math.sqrt(c / (n * len(obj))), K, p[4:8].copy(), ext[:, :3].copy(), ext[:, 3:].copy(), c


# ---- the lattice-growing labeller -----------------------------------------------------

GROW_FACTOR = 2        # the 2 * bw * bh strongest candidates are the labeller's input
GROW_SEEDS = 8         # seeds are tried until a board is found and this seed index is reached


def _smooth(g, P):
    """the acceptance rule of a grown labelling (integer exact): _regular's midpoint
    rule, and along every row and column the deviations from the midpoint change
    slowly: a lens bends a row, it does not kink it.  dev_j = 2 P_j - P_(j-1) -
    P_(j+1) is twice the deviation at node j; for three inner nodes in a row
    16 |2 dev_j - dev_(j-1) - dev_(j+1)|^2 <= |P_(j+2) - P_(j-2)|^2."""
    Q = P[g]                                         # bh x bw x 2, int64
    for a in (Q, Q.transpose(1, 0, 2)):
        if a.shape[1] < 3:
            continue
        dev = 2 * a[:, 1:-1] - a[:, :-2] - a[:, 2:]
        span = a[:, 2:] - a[:, :-2]
        if np.any(16 * (dev ** 2).sum(2) > (span ** 2).sum(2)):
            return False
        if a.shape[1] >= 5:
            kink = 2 * dev[:, 1:-1] - dev[:, :-2] - dev[:, 2:]
            span4 = a[:, 4:] - a[:, :-4]
            if np.any(16 * (kink ** 2).sum(2) > (span4 ** 2).sum(2)):
                return False
    return True


def label_board_grow(cand, bw, bh):
    """bh x bw grid of indices into cand: the canonical labelling of a complete
    lattice among the 2 * bw * bh strongest candidates, or None.  Integer exact.

    For each seed in strength order: u is the step to its nearest neighbour, v the
    step to the nearest of its next three neighbours that is roughly perpendicular
    (|cos| < 0.5) and shorter than 2 |u|.  The lattice grows breadth-first; a new
    node is predicted at 2 P(i, j) - P(i - 1, j) when the node behind exists, else
    at P(i, j) + step, and takes the candidate nearest the prediction when that one
    is unused and within 0.3 of the local step; the local basis follows the accepted
    step.  Of the complete bw x bh windows (either orientation) of the grown set
    that pass _smooth, the one with the largest response sum is kept (ties: the
    first found).  Seeds are tried until a board is found and seed GROW_SEEDS is
    reached, and never more than bw * bh + GROW_SEEDS + 1 of them: at most bw * bh
    candidates are no corner of a complete board, so that many seeds hold at least
    GROW_SEEDS + 1 of its corners."""
    cand = np.asarray(cand, np.int64).reshape(-1, 3)
    n = bw * bh
    if bw < 2 or bh < 2 or len(cand) < n:
        return None
    sel = calib_ref.strongest(cand, min(len(cand), GROW_FACTOR * n))
    P = cand[sel, :2]
    m = len(P)
    if len(set(map(tuple, P.tolist()))) != m:
        return None
    D2 = ((P[:, None] - P[None]) ** 2).sum(2)
    lim = max(bw, bh)
    best = None
    for s in range(min(m, n + GROW_SEEDS + 1)):
        d = D2[s].copy()
        d[s] = np.iinfo(np.int64).max
        nb = np.lexsort((np.arange(m), d))[:4]
        u = P[nb[0]] - P[s]
        uu = int(u @ u)
        v = None
        for b in nb[1:]:
            w = P[b] - P[s]
            ww, uw = int(w @ w), int(u @ w)
            if 4 * uw * uw < uu * ww and ww < 4 * uu:
                v = w
                break
        if v is not None:
            lab = {(0, 0): s}
            used = {s}
            bas = {(0, 0): (u, v)}
            front = [(0, 0)]
            while front:
                nf = []
                for (i, j) in front:
                    bu, bv = bas[(i, j)]
                    cur = P[lab[(i, j)]]
                    for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                        q = (i + di, j + dj)
                        if q in lab or abs(q[0]) > lim or abs(q[1]) > lim:
                            continue
                        step = bu * di + bv * dj
                        back = (i - di, j - dj)
                        pred = 2 * cur - P[lab[back]] if back in lab else cur + step
                        e = ((P - pred) ** 2).sum(1)
                        k = int(np.lexsort((np.arange(m), e))[0])
                        if 100 * int(e[k]) > 9 * int(step @ step) or k in used:
                            continue
                        lab[q] = k
                        used.add(k)
                        ns = P[k] - cur
                        bas[q] = (ns * di, bv) if di else (bu, ns * dj)
                        nf.append(q)
                front = nf
            if len(lab) >= n:
                keys = np.array(list(lab.keys()))
                (i0, j0), (i1, j1) = keys.min(0), keys.max(0)
                for W, H in ((bw, bh), (bh, bw)):
                    for oi in range(i0, i1 - W + 2):
                        for oj in range(j0, j1 - H + 2):
                            if not all((oi + a, oj + b) in lab for a in range(W) for b in range(H)):
                                continue
                            g = np.array([[lab[(oi + a, oj + b)] for a in range(W)] for b in range(H)])
                            if (W, H) != (bw, bh):
                                g = g.T
                            if not _smooth(g, P):
                                continue
                            score = int(cand[sel[g.ravel()], 2].sum())
                            if best is None or score > best[0]:
                                best = (score, g)
                    if bw == bh:
                        break
        if best is not None and s >= GROW_SEEDS:
            break
    if best is None:
        return None
    pts = [(int(x), int(y)) for x, y in P]
    g = calib_ref.canonical(best[1], pts)
    a, b, c = pts[int(g[0, 0])], pts[int(g[0, 1])], pts[int(g[1, 0])]
    if calib_ref._cross(a, b, c) <= 0:
        return None
    return sel[g]


def find_chessboard(img, board):
    """calib_ref.find_chessboard with the growing labeller: (found, corners (bw * bh,
    2) f32 in full-resolution pixels, row-major)"""
    bw, bh = board
    cand, s = calib_ref.candidates(img)
    g = label_board_grow(cand, bw, bh)
    if g is None:
        return False, None
    xy = cand[g.ravel(), :2].astype(np.float32)
    return True, np.float32(s) * xy + np.float32((s - 1) / 2)

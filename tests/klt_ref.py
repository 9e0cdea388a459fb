"""numpy restatement of cv::buildOpticalFlowPyramid and cv::calcOpticalFlowPyrLK
(OpenCV 4.8, one 8-bit channel, images given as plain Mats).  The checker of
tests/test_klt*.py and the definition of slam_klt_pyramid / slam_klt_track*;
DESIGN.md section 15 has the contract and the deviations.

Like tests/calib_ref.py it is written from the OpenCV source and is not pinned
against a real OpenCV build: no OpenCV is available to the tests.

  gray              cvtColor BGR2GRAY (color.simd_helpers, the 14-bit integer form):
                    the library's gray_at
  pyr_down          pyramids.cpp pyrDown_<uchar>: separable 1 4 6 4 1, BORDER_REFLECT_101,
                    (sum + 128) >> 8, size ((w + 1) / 2, (h + 1) / 2)
  level_count       lkpyramid.cpp buildOpticalFlowPyramid: the early return when the
                    next level would be no larger than the window
  scharr            lkpyramid.cpp calcScharrDeriv (scalar path), int16 {Ix, Iy}
  track             lkpyramid.cpp calcOpticalFlowPyrLK + LKTrackerInvoker::operator()

Every f32 operation in `track` is one numpy float32 operation in the order the
C++ source evaluates it (a build without FMA contraction).  The points are
independent: the loops run on the set of points still active, and each point
sees exactly the scalar loop's operations.

The one deliberate deviation: the five window sums (Ix^2, Ix Iy, Iy^2, diff Ix,
diff Iy) are exact.  Every term is an integer below 2^26; OpenCV adds them into
f32 accumulators in an order that differs between its scalar, SSE and AVX
builds, so there is no single bit pattern to match.  Here they are summed in
int64 and converted to f32 once (round to nearest even) before the 2^-20 scale:
the value every OpenCV build approximates, independent of the order.

Reads outside a level: intensities reflect (101, as the border
buildOpticalFlowPyramid pads with), derivatives are 0 (copyMakeBorder
BORDER_CONSTANT on derivI).  Levels are stored unpadded; indices are reflected
with period 2 (n - 1), which is BORDER_REFLECT_101 for any distance.

status / err of a point no level wrote: status starts 1 and err starts 0 (OpenCV
leaves err unwritten there).
"""
import numpy as np

USE_INITIAL_FLOW = 4       # cv::OPTFLOW_USE_INITIAL_FLOW
GET_MIN_EIGENVALS = 8      # cv::OPTFLOW_LK_GET_MIN_EIGENVALS
W_BITS = 14
FLT_SCALE = np.float32(1.0 / (1 << 20))
FLT_EPSILON = np.float32(np.finfo(np.float32).eps)
MAX_LEVEL_LIMIT = 8
WIN_MIN, WIN_MAX = 3, 31

# the exits of LKTrackerInvoker a trace counts, per point (any level unless named)
EXITS = ("oob_prev_upper", "oob_prev_l0", "mineig", "oob_iter_upper", "oob_iter_l0", "eps", "oscillation", "cap",
         "oob_final")

f32 = np.float32


def check_params(win, max_level, criteria, flags):
    ww, wh = int(win[0]), int(win[1])
    if not (WIN_MIN <= ww <= WIN_MAX and WIN_MIN <= wh <= WIN_MAX):
        raise ValueError("window 3..31 per axis")
    if not 0 <= int(max_level) <= MAX_LEVEL_LIMIT:
        raise ValueError("maxLevel 0..8")
    max_count, eps = criteria
    if int(max_count) < 1 or not float(eps) >= 0:
        raise ValueError("maxCount >= 1, eps >= 0")
    if int(flags) & ~(USE_INITIAL_FLOW | GET_MIN_EIGENVALS):
        raise ValueError("flags: USE_INITIAL_FLOW | GET_MIN_EIGENVALS")
    # calcOpticalFlowPyrLK clamps the criteria: maxCount to 0..100, epsilon to 0..10, then squares it (f64)
    eps = min(max(float(eps), 0.0), 10.0)
    return ww, wh, int(max_level), min(int(max_count), 100), eps * eps


def gray(img):
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise TypeError("8-bit frames")
    if a.ndim == 2:
        return np.ascontiguousarray(a)
    b, g, r = (a[:, :, k].astype(np.uint32) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def reflect101(i, n):
    """BORDER_REFLECT_101 index of any integer i into 0..n-1 (borderInterpolate)"""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def pyr_down(g):
    h, w = g.shape
    dw, dh = (w + 1) // 2, (h + 1) // 2
    s = g.astype(np.int32)
    k = (1, 4, 6, 4, 1)
    xs = 2 * np.arange(dw)
    row = sum(k[t] * s[:, reflect101(xs + t - 2, w)] for t in range(5))
    ys = 2 * np.arange(dh)
    out = sum(k[t] * row[reflect101(ys + t - 2, h), :] for t in range(5))
    return ((out + 128) >> 8).astype(np.uint8)


def level_count(w, h, win, max_level):
    """levels built: level 0 always; level l + 1 only if larger than the window on both axes"""
    n = 1
    while n <= max_level:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win[0] or h <= win[1]:
            break
        n += 1
    return n


def scharr(g):
    h, w = g.shape
    s = g.astype(np.int32)
    r0, r2 = s[reflect101(np.arange(h) - 1, h)], s[reflect101(np.arange(h) + 1, h)]
    t0 = (r0 + r2) * 3 + s * 10
    t1 = r2 - r0
    xl, xr = reflect101(np.arange(w) - 1, w), reflect101(np.arange(w) + 1, w)
    out = np.empty((h, w, 2), np.int16)
    out[:, :, 0] = t0[:, xr] - t0[:, xl]
    out[:, :, 1] = (t1[:, xr] + t1[:, xl]) * 3 + t1 * 10
    return out


def build_pyramid(img, win=(21, 21), max_level=3, with_derivatives=True):
    """(gray levels, derivative planes or None): levels[0] is the gray image"""
    g = gray(img)
    n = level_count(g.shape[1], g.shape[0], win, max_level)
    levels = [g]
    for _ in range(1, n):
        levels.append(pyr_down(levels[-1]))
    return levels, ([scharr(l) for l in levels] if with_derivatives else None)


def _cv_round(v):
    return np.rint(v).astype(np.int64)       # cvRound: round half to even


def _weights(a, b):
    one, s = f32(1), f32(1 << W_BITS)
    iw00 = _cv_round((one - a) * (one - b) * s)
    iw01 = _cv_round(a * (one - b) * s)
    iw10 = _cv_round((one - a) * b * s)
    return iw00, iw01, iw10, (1 << W_BITS) - iw00 - iw01 - iw10


def _descale(v, n):
    return (v + (1 << (n - 1))) >> n


def _window(ix, iy, ww, wh):
    """pixel indices (n, wh, ww) of the windows with corners (ix, iy)"""
    xs = ix[:, None, None] + np.arange(ww)[None, None, :]
    ys = iy[:, None, None] + np.arange(wh)[None, :, None]
    return np.broadcast_arrays(ys, xs)


def _sample_gray(g, ys, xs, w4):
    """sum iw * src over the 2 x 2 neighbours, intensities reflected"""
    h, w = g.shape
    s = g.astype(np.int64)
    y0, y1, x0, x1 = reflect101(ys, h), reflect101(ys + 1, h), reflect101(xs, w), reflect101(xs + 1, w)
    iw00, iw01, iw10, iw11 = (v[:, None, None] for v in w4)
    return s[y0, x0] * iw00 + s[y0, x1] * iw01 + s[y1, x0] * iw10 + s[y1, x1] * iw11


def _sample_deriv(d, ys, xs, w4, k):
    """the same for derivative component k, 0 outside the level"""
    h, w = d.shape[:2]
    s = d[:, :, k].astype(np.int64)

    def at(y, x):
        ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        return np.where(ok, s[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0)
    iw00, iw01, iw10, iw11 = (v[:, None, None] for v in w4)
    return at(ys, xs) * iw00 + at(ys, xs + 1) * iw01 + at(ys + 1, xs) * iw10 + at(ys + 1, xs + 1) * iw11


def _corner(p, ww, wh, cols, rows):
    """(ix, iy, outside) of the window positions p (n x 2 f32): the integer corner
    floor(p) and the bounds test ix < -winW || ix >= cols || iy < -winH || iy >= rows,
    taken on the floored floats (the same test wherever the floor is an int; a
    position that is NaN, infinite or beyond the int range is outside)"""
    fx, fy = np.floor(p[:, 0]), np.floor(p[:, 1])
    with np.errstate(invalid="ignore"):
        inside = (fx >= -ww) & (fx < cols) & (fy >= -wh) & (fy < rows)
    return np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64), ~inside


def _isum(v):
    """exact window sum -> f32 once"""
    return v.reshape(len(v), -1).sum(1, dtype=np.int64).astype(np.float32)


def track(prev, nxt, prev_pts, next_pts=None, win=(21, 21), max_level=3, criteria=(30, 0.01), flags=0,
          min_eig_threshold=1e-4, trace=None):
    """calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err, win, maxLevel,
    TermCriteria(COUNT + EPS, *criteria), flags, minEigThreshold) -> (nextPts n x 2 f32,
    status n u8, err n f32).  trace: a dict that receives one bool array per EXITS name."""
    ww, wh, max_level, max_count, eps2 = check_params(win, max_level, criteria, flags)
    gp, gn = gray(prev), gray(nxt)
    if gp.shape != gn.shape:
        raise ValueError("frames of one size")
    prev_pts = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
    n = len(prev_pts)
    if flags & USE_INITIAL_FLOW:
        out = np.array(next_pts, np.float32).reshape(-1, 2).copy()
        if len(out) != n:
            raise ValueError("USE_INITIAL_FLOW: one initial position per point")
    else:
        out = np.zeros((n, 2), np.float32)
    status = np.ones(n, np.uint8)
    err = np.zeros(n, np.float32)
    tr = {k: np.zeros(n, bool) for k in EXITS}
    if trace is not None:
        trace.update(tr)
    if n == 0:
        return out, status, err
    lp, dp = build_pyramid(gp, (ww, wh), max_level, True)
    ln, _ = build_pyramid(gn, (ww, wh), max_level, False)
    top = len(lp) - 1
    half = np.array([(ww - 1) * f32(0.5), (wh - 1) * f32(0.5)], np.float32)
    min_eig_threshold = f32(min_eig_threshold)
    area2 = f32(2 * ww * wh)
    for level in range(top, -1, -1):
        I_img, D_img, J_img = lp[level], dp[level], ln[level]
        rows, cols = I_img.shape
        scale = f32(1.0 / (1 << level))
        pp = prev_pts * scale
        if level == top:
            out[:] = out * scale if flags & USE_INITIAL_FLOW else pp
        else:
            out[:] = out * f32(2)
        pp = pp - half
        ipx, ipy, oob = _corner(pp, ww, wh, cols, rows)
        tr["oob_prev_l0" if level == 0 else "oob_prev_upper"] |= oob
        if level == 0:
            status[oob] = 0
            err[oob] = 0
        act = np.nonzero(~oob)[0]
        if len(act) == 0:
            continue
        ix, iy = ipx[act], ipy[act]
        a, b = pp[act, 0] - ix.astype(np.float32), pp[act, 1] - iy.astype(np.float32)
        w4 = _weights(a, b)
        ys, xs = _window(ix, iy, ww, wh)
        Iw = _descale(_sample_gray(I_img, ys, xs, w4), W_BITS - 5)
        Ix = _descale(_sample_deriv(D_img, ys, xs, w4, 0), W_BITS)
        Iy = _descale(_sample_deriv(D_img, ys, xs, w4, 1), W_BITS)
        A11, A12, A22 = _isum(Ix * Ix) * FLT_SCALE, _isum(Ix * Iy) * FLT_SCALE, _isum(Iy * Iy) * FLT_SCALE
        D = A11 * A22 - A12 * A12
        min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + f32(4) * A12 * A12)) / area2
        if flags & GET_MIN_EIGENVALS:
            err[act] = min_eig
        bad = (min_eig < min_eig_threshold) | (D < FLT_EPSILON)
        tr["mineig"][act[bad]] = True
        if level == 0:
            status[act[bad]] = 0
        keep = ~bad
        act, Iw, Ix, Iy, A11, A12, A22 = act[keep], Iw[keep], Ix[keep], Iy[keep], A11[keep], A12[keep], A22[keep]
        if len(act) == 0:
            continue
        with np.errstate(over="ignore"):
            Dinv = f32(1) / D[keep]
        npt = out[act] - half                 # the running nextPt of the points in `act`
        pdx, pdy = np.zeros(len(act), np.float32), np.zeros(len(act), np.float32)
        live = np.ones(len(act), bool)
        for j in range(max_count):
            k = np.nonzero(live)[0]
            if len(k) == 0:
                break
            jx, jy, oob = _corner(npt[k], ww, wh, cols, rows)
            tr["oob_iter_l0" if level == 0 else "oob_iter_upper"][act[k[oob]]] = True
            if level == 0:
                status[act[k[oob]]] = 0
            live[k[oob]] = False
            k, jx, jy = k[~oob], jx[~oob], jy[~oob]
            if len(k) == 0:
                break
            a, b = npt[k, 0] - jx.astype(np.float32), npt[k, 1] - jy.astype(np.float32)
            ys, xs = _window(jx, jy, ww, wh)
            diff = _descale(_sample_gray(J_img, ys, xs, _weights(a, b)), W_BITS - 5) - Iw[k]
            b1, b2 = _isum(diff * Ix[k]) * FLT_SCALE, _isum(diff * Iy[k]) * FLT_SCALE
            with np.errstate(over="ignore", invalid="ignore"):
                dx = (A12[k] * b2 - A22[k] * b1) * Dinv[k]
                dy = (A12[k] * b1 - A11[k] * b2) * Dinv[k]
                npt[k, 0] = npt[k, 0] + dx
                npt[k, 1] = npt[k, 1] + dy
                out[act[k]] = npt[k] + half
                small = dx.astype(np.float64) * dx.astype(np.float64) + dy.astype(np.float64) * dy.astype(np.float64) <= eps2
                osc = ~small & (j > 0) & (np.abs(dx + pdx[k]).astype(np.float64) < 0.01) & \
                    (np.abs(dy + pdy[k]).astype(np.float64) < 0.01)
                tr["eps"][act[k[small]]] = True
                tr["oscillation"][act[k[osc]]] = True
                ko = k[osc]
                out[act[ko], 0] = out[act[ko], 0] - dx[osc] * f32(0.5)
                out[act[ko], 1] = out[act[ko], 1] - dy[osc] * f32(0.5)
            live[k[small | osc]] = False
            pdx[k], pdy[k] = dx, dy
        tr["cap"][act[live]] = True
        if level == 0 and not flags & GET_MIN_EIGENVALS:
            k = np.nonzero(status[act] != 0)[0]
            fin = out[act[k]] - half
            jx, jy, oob = _corner(fin, ww, wh, cols, rows)
            tr["oob_final"][act[k[oob]]] = True
            status[act[k[oob]]] = 0
            k, jx, jy, fin = k[~oob], jx[~oob], jy[~oob], fin[~oob]
            if len(k):
                a, b = fin[:, 0] - jx.astype(np.float32), fin[:, 1] - jy.astype(np.float32)
                ys, xs = _window(jx, jy, ww, wh)
                diff = _descale(_sample_gray(J_img, ys, xs, _weights(a, b)), W_BITS - 5) - Iw[k]
                err[act[k]] = _isum(np.abs(diff)) / f32(32 * ww * wh)
    return out, status, err


def parity_points(frame, fast_xy, win=(21, 21)):
    """the adversarial point set the GPU parity tests and the exit-coverage test
    share: the frame's FAST keypoints, the four corners, points within half a
    window of each border, points at (-1, y) and (w, y), .5 positions, the
    flattest spot of the frame, and points far enough outside that their window
    leaves the level (before the iterations)"""
    g = gray(frame).astype(np.float64)
    h, w = g.shape
    hw, hh = win[0] // 2, win[1] // 2
    pts = [np.asarray(fast_xy, np.float32).reshape(-1, 2)]
    pts.append([(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)])
    ys, xs = np.linspace(3, h - 4, 7), np.linspace(3, w - 4, 7)
    pts.append([(hw * 0.5, y) for y in ys] + [(w - 1 - hw * 0.5, y) for y in ys])
    pts.append([(x, hh * 0.5) for x in xs] + [(x, h - 1 - hh * 0.5) for x in xs])
    pts.append([(-1, y) for y in ys[::2]] + [(w, y) for y in ys[::2]])
    pts.append([(x + 0.5, y + 0.5) for x, y in zip(xs, ys)] + [(x + 0.5, y) for x, y in zip(xs, ys[::-1])])
    # flattest 9 x 9 neighbourhood (box variance from integral images), first in raster order
    k = 9
    c1 = np.pad(g, ((1, 0), (1, 0))).cumsum(0).cumsum(1)
    c2 = np.pad(g * g, ((1, 0), (1, 0))).cumsum(0).cumsum(1)
    box = lambda c: c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]
    var = box(c2) - box(c1) ** 2 / (k * k)
    fy, fx = np.unravel_index(np.argmin(var), var.shape)
    pts.append([(fx + k // 2, fy + k // 2)])
    # outside: the window misses the level at level 0, and at the upper levels too
    pts.append([(-2.0 * w, h / 2), (3.0 * w, h / 2), (w / 2, -2.0 * h), (w / 2, 3.0 * h), (-win[0] - 2, 5), (7, h + win[1] + 2)])
    return np.concatenate([np.asarray(p, np.float32).reshape(-1, 2) for p in pts])


def parity_initial_flow(prev_pts, w, h, seed=5):
    """initial positions for USE_INITIAL_FLOW: the points themselves, some moved by a
    few pixels, some placed on the frame's edges (their windows leave the level
    during the iterations or at the final error) and some far outside"""
    rng = np.random.default_rng(seed)
    out = np.array(prev_pts, np.float32).reshape(-1, 2).copy()
    n = len(out)
    k = rng.integers(0, 6, n)
    out[k == 1] += rng.uniform(-3, 3, (int((k == 1).sum()), 2)).astype(np.float32)
    m = k == 2
    out[m, 0] = np.where(rng.random(int(m.sum())) < 0.5, np.float32(-1.5), np.float32(w + 0.5))
    m = k == 3
    out[m, 1] = np.where(rng.random(int(m.sum())) < 0.5, np.float32(-1.5), np.float32(h + 0.5))
    m = k == 4
    out[m] = out[m] + np.float32(4 * max(w, h))
    return out


PARITY_WINDOWS = ((21, 21), (3, 3), (31, 31), (9, 15))
# (maxLevel, criteria, flags) run at every window of PARITY_WINDOWS
PARITY_VARIANTS = ((3, (30, 0.01), 0), (0, (30, 0.01), 0), (3, (1, 0.01), 0), (3, (30, 0.0), 0),
                   (3, (30, 0.01), USE_INITIAL_FLOW), (3, (30, 0.01), GET_MIN_EIGENVALS),
                   (3, (30, 0.01), USE_INITIAL_FLOW | GET_MIN_EIGENVALS))


def analytic_texture(w, h, dx=0.0, dy=0.0, seed=11, waves=24):
    """a smooth texture known in closed form, sampled with its content moved by
    (dx, dy): 24 plane waves of wavelengths 6..90 px (the long ones carry the coarse
    levels, the short ones the sub-pixel fit), rounded to 8 bits.  A point p of
    texture(w, h) is at p + (dx, dy) in texture(w, h, dx, dy), exactly."""
    rng = np.random.default_rng(seed)
    lam = np.exp(rng.uniform(np.log(6), np.log(90), waves))
    th, ph = rng.uniform(0, 2 * np.pi, waves), rng.uniform(0, 2 * np.pi, waves)
    amp = lam ** 0.5
    amp *= 100 / np.sqrt((amp ** 2).sum() / 2) / 2.2
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - dx, y - dy
    v = 128 + sum(a * np.sin(2 * np.pi * (np.cos(t) * x + np.sin(t) * y) / l + p) for a, l, t, p in zip(amp, lam, th, ph))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


TRUTH_SIZE = (192, 144)
TRUTH_SHIFTS = ((0.3, -0.7), (9.25, -6.5))     # the second needs the pyramid
# the reference's own largest displacement error (pixels, either axis) over the
# interior grid of truth_points(), measured on the CPU (tests/test_klt.py)
TRUTH_REF_MAX_ERR = {(0.3, -0.7): 0.0146, (9.25, -6.5): 0.0190}


def truth_points():
    w, h = TRUTH_SIZE
    ys, xs = np.mgrid[40:h - 40:8, 40:w - 40:8]
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32) + np.float32(0.25)

"""CPU definition of the chessboard calibration stage: the
checker of tests/test_calib*.py and of scripts/calib_bench.py.  numpy only;
scipy is imported by the solver part (calibrate) alone.

Four parts, each the contract of one piece of the library:

  gray / level / response / candidates   slam_chess_candidates (csrc/calib.hip)
  find_chessboard / label_board          slam_find_chessboard (csrc/calib_board.cpp)
  corner_subpix                          slam_corner_subpix (csrc/calib.hip)
  calibrate                              slam_calibrate_camera (csrc/calib_solve.cpp)

The detector is this project's own (OpenCV's findChessboardCorners is a chain
of heuristics that cannot be restated here); every integer below is therefore
the contract itself and the device must equal it bit for bit.

corner_subpix restates cv::cornerSubPix of OpenCV 4.8 (cornersubpix.cpp with
getRectSubPix_8u32f and getRectSubPix_Cn_ of samplers.cpp) from memory of the
source; no OpenCV is available to pin it against.  Known deviations:
  * the mask's exp: OpenCV calls expf(-x * x); here and in the library it is
    (float)exp((double)(-x * x)), computed on the host.  The two may differ by
    one f32 ulp; this form is the same in numpy, glibc and the library.
  * the zero zone is always (-1, -1) (the library refuses any other).
  * indices of the replicated-border sampler are clamped to the image.  This is
    what OpenCV reads whenever the corner under iteration is inside the image,
    which cornerSubPix guarantees after its first iteration; the library refuses
    start corners outside the image instead of reading as OpenCV would.
  * every f32 / f64 operation is one numpy operation in the source's order, i.e.
    the values of a build without FMA contraction; the five window sums are
    sequential (np.add.accumulate), never pairwise (np.sum).
"""
import math

import numpy as np

RING = ((0, -5), (2, -5), (3, -3), (5, -2), (5, 0), (5, 2), (3, 3), (2, 5),
        (0, 5), (-2, 5), (-3, 3), (-5, 2), (-5, 0), (-5, -2), (-3, -3), (-2, -5))
BORDER = 5          # the ring's radius: R = 0 closer to the level's edge
NMS_RADIUS = 7      # 15 x 15 window
MAX_WIN = 15        # corner_subpix: half window per axis


# ---- corner candidates ----------------------------------------------------------

def gray(img):
    """u8 gray of an HxW or HxWx3 (BGR) frame: cvtColor's fixed point, as FAST sees it"""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise TypeError("frames are 8-bit")
    if a.ndim == 2:
        return a
    b, g, r = (a[..., k].astype(np.uint32) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def scale_of(w, h):
    return max(1, -(-max(w, h) // 1024))


def level(g):
    """(level image, s): the s x s area mean, round half up, remainder dropped"""
    h, w = g.shape
    s = scale_of(w, h)
    W, H = w // s, h // s
    if s == 1:
        return g, 1
    blocks = g[:H * s, :W * s].astype(np.int64).reshape(H, s, W, s).sum(axis=(1, 3))
    return ((blocks + s * s // 2) // (s * s)).astype(np.uint8), s


def response(lv):
    """int32 map of 80 x the ChESS response; 0 in the 5-pixel border"""
    H, W = lv.shape
    R = np.zeros((H, W), np.int32)
    if W < 2 * BORDER + 1 or H < 2 * BORDER + 1:
        return R
    a = lv.astype(np.int32)
    ys, xs = slice(BORDER, H - BORDER), slice(BORDER, W - BORDER)

    def at(dx, dy):
        return a[BORDER + dy:H - BORDER + dy, BORDER + dx:W - BORDER + dx]
    I = [at(dx, dy) for dx, dy in RING]
    L = at(0, 0) + at(-1, 0) + at(1, 0) + at(0, -1) + at(0, 1)
    SR = sum(np.abs(I[n] + I[n + 8] - I[n + 4] - I[n + 12]) for n in range(4))
    DR = sum(np.abs(I[n] - I[n + 8]) for n in range(8))
    MR = np.abs(5 * sum(I) - 16 * L)
    R[ys, xs] = 80 * (SR - DR) - 16 * MR
    return R


def candidates_of_response(R):
    """(n, 3) int32 rows (x, y, R) in raster order: R > 0, strictly above every
    earlier cell (raster order) of its 15 x 15 window and at least every later
    one; cells outside the image count as 0"""
    H, W = R.shape
    r = NMS_RADIUS
    P = np.zeros((H + 2 * r, W + 2 * r), np.int32)
    P[r:r + H, r:r + W] = R
    # the window maximum, separably; then the tie rule on the few pixels that reach it
    M = P.copy()
    for d in range(1, r + 1):
        M[:, d:] = np.maximum(M[:, d:], P[:, :-d])
        M[:, :-d] = np.maximum(M[:, :-d], P[:, d:])
    Mx = M.copy()
    for d in range(1, r + 1):
        M[d:, :] = np.maximum(M[d:, :], Mx[:-d, :])
        M[:-d, :] = np.maximum(M[:-d, :], Mx[d:, :])
    ys, xs = np.nonzero((R > 0) & (R == M[r:r + H, r:r + W]))
    out = []
    for y, x in zip(ys.tolist(), xs.tolist()):
        v = P[y + r, x + r]
        win = P[y:y + 2 * r + 1, x:x + 2 * r + 1].ravel()
        earlier = win[:r * (2 * r + 1) + r]
        if not np.any(earlier >= v):
            out.append((x, y, int(v)))
    return np.array(out, np.int32).reshape(-1, 3)


def candidates(img):
    """(cand (n, 3) int32 in level coordinates, s) of a gray or BGR frame"""
    lv, s = level(gray(img))
    return candidates_of_response(response(lv)), s


# ---- board labelling --------------------------------------------------------------

def strongest(cand, n):
    """indices of the n strongest candidates, ties to the lower raster index"""
    order = np.lexsort((np.arange(len(cand)), -cand[:, 2].astype(np.int64)))
    return order[:n]


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _hull(pts):
    """convex hull (Andrew's monotone chain), collinear points dropped; indices"""
    idx = sorted(range(len(pts)), key=lambda i: (pts[i][0], pts[i][1]))
    def half(seq):
        h = []
        for i in seq:
            while len(h) >= 2 and _cross(pts[h[-2]], pts[h[-1]], pts[i]) <= 0:
                h.pop()
            h.append(i)
        return h
    lo, up = half(idx), half(idx[::-1])
    return lo[:-1] + up[:-1]


def _outer_quad(pts):
    """the four hull vertices that span the largest quadrilateral, in hull order"""
    hull = _hull(pts)
    n = len(hull)
    if n < 4:
        return None
    best, quad = -1, None
    for a in range(n):
        for b in range(a + 1, n):
            for c in range(b + 1, n):
                for d in range(c + 1, n):
                    q = [pts[hull[k]] for k in (a, b, c, d)]
                    area = abs(_cross(q[0], q[1], q[2]) + _cross(q[0], q[2], q[3]))
                    if area > best:
                        best, quad = area, [hull[k] for k in (a, b, c, d)]
    return quad


def _nearest_to_line(pts, p, q, n):
    """the n points nearest to the line p q, ordered from p to q"""
    d = (q[0] - p[0], q[1] - p[1])
    dist = [abs(_cross(p, q, z)) for z in pts]
    take = sorted(range(len(pts)), key=lambda i: (dist[i], i))[:n]
    return sorted(take, key=lambda i: ((pts[i][0] - p[0]) * d[0] + (pts[i][1] - p[1]) * d[1], i))


def _peel(pts, quad, bw, bh):
    """label by lines: the left and right columns, then each row between them"""
    A, B, C, D = quad
    left = _nearest_to_line(pts, pts[A], pts[D], bh)
    right = _nearest_to_line(pts, pts[B], pts[C], bh)
    if left[0] != A or left[-1] != D or right[0] != B or right[-1] != C:
        return None
    grid = []
    for k in range(bh):
        row = _nearest_to_line(pts, pts[left[k]], pts[right[k]], bw)
        if row[0] != left[k] or row[-1] != right[k]:
            return None
        grid.append(row)
    if sorted(i for row in grid for i in row) != list(range(bw * bh)):
        return None
    return grid


def _regular(grid, pts):
    """the acceptance rule of a labelling (part of the contract, integer exact):
    along every row and column each inner node lies within a quarter of the local
    spacing of the midpoint of its two neighbours"""
    g = np.array(grid)
    P = np.array([pts[int(i)] for i in g.ravel()], np.int64).reshape(g.shape + (2,))
    for a in (P, P.transpose(1, 0, 2)):
        if a.shape[1] < 3:
            continue
        dev = 2 * a[:, 1:-1] - a[:, :-2] - a[:, 2:]          # twice the deviation from the midpoint
        span = a[:, 2:] - a[:, :-2]                          # twice the spacing
        if np.any(16 * (dev ** 2).sum(2) > (span ** 2).sum(2)):
            return False
    return True


def canonical(grid, pts):
    """the canonical one of a labelling's symmetries: right-handed in image
    coordinates (y down), then the rotation whose first corner has the least
    x + y, ties to the least y.  grid: bh rows of bw indices."""
    g = np.array(grid)
    P = lambda i: pts[int(i)]
    if _cross(P(g[0, 0]), P(g[0, 1]), P(g[1, 0])) < 0:
        g = g[:, ::-1]
    rots = [g, g[::-1, ::-1]]
    if g.shape[0] == g.shape[1]:
        rots += [np.rot90(g, 1), np.rot90(g, 3)]
    key = lambda m: (P(m[0, 0])[0] + P(m[0, 0])[1], P(m[0, 0])[1])
    return min(rots, key=key)


def label_board(pts, bw, bh):
    """bh x bw index grid of the canonical labelling of bw * bh points, or None
    when they are not a complete lattice"""
    pts = [(int(x), int(y)) for x, y in pts]
    if len(pts) != bw * bh or bw < 2 or bh < 2 or len(set(pts)) != len(pts):
        return None
    quad = _outer_quad(pts)
    if quad is None:
        return None
    for shift in range(2):
        q = quad[shift:] + quad[:shift]
        grid = _peel(pts, q, bw, bh)
        if grid is not None and _regular(grid, pts):
            g = canonical(grid, pts)
            a, b, c = pts[int(g[0, 0])], pts[int(g[0, 1])], pts[int(g[1, 0])]
            if _cross(a, b, c) > 0:
                return g
    return None


def find_chessboard(img, board):
    """(found, corners (bw * bh, 2) f32 in full-resolution pixels, row-major)"""
    bw, bh = board
    cand, s = candidates(img)
    n = bw * bh
    if len(cand) < n:
        return False, None
    sel = cand[strongest(cand, n)]
    g = label_board(sel[:, :2], bw, bh)
    if g is None:
        return False, None
    xy = sel[g.ravel(), :2].astype(np.float32)
    return True, np.float32(s) * xy + np.float32((s - 1) / 2)


# ---- cornerSubPix -------------------------------------------------------------------

f32 = np.float32
f64 = np.float64


def subpix_mask(win):
    """(vx, vy) f32: exp(-x^2) per column / row, x = (float)(j - w) / w"""
    def axis(w):
        x = (np.arange(2 * w + 1) - w).astype(f32) / f32(w)
        return np.array([f32(math.exp(float(-v * v))) for v in x], f32)
    return axis(win[0]), axis(win[1])


def rect_subpix(g, ww, wh, cx, cy):
    """getRectSubPix(g, Size(ww, wh), (cx, cy)) u8 -> f32 (getRectSubPix_8u32f)"""
    H, W = g.shape
    cx = f32(cx) - f32((ww - 1) * 0.5)
    cy = f32(cy) - f32((wh - 1) * 0.5)
    ipx, ipy = int(math.floor(cx)), int(math.floor(cy))
    a = f32(cx - f32(ipx))
    b = f32(cy - f32(ipy))
    one = f32(1)
    if 0 <= ipx and ipx + ww < W and 0 <= ipy and ipy + wh < H:
        # the window and its right / lower neighbours are inside: the row recurrence
        a = max(a, f32(0.0001))
        a12 = a * (one - b)
        a22 = a * b
        b1 = one - b
        b2 = b
        s = (f64(1) - f64(a)) / f64(a)
        r0 = g[ipy:ipy + wh, ipx:ipx + ww + 1].astype(f32)
        r1 = g[ipy + 1:ipy + wh + 1, ipx:ipx + ww + 1].astype(f32)
        t = a12 * r0[:, 1:] + a22 * r1[:, 1:]                       # t_j, j = 0 .. ww - 1
        prev = np.empty_like(t)
        prev[:, 0] = (one - a) * (b1 * r0[:, 0] + b2 * r1[:, 0])
        prev[:, 1:] = (t[:, :-1].astype(f64) * s).astype(f32)
        return prev + t
    a11 = (one - a) * (one - b)
    a12 = a * (one - b)
    a21 = (one - a) * b
    a22 = a * b
    b1 = one - b
    b2 = b
    rx, rw = max(-ipx, 0), (ww if ipx < W - ww else W - ipx - 1)
    ya = np.clip(ipy + np.arange(wh), 0, H - 1)
    yb = np.clip(ipy + np.arange(wh) + 1, 0, H - 1)
    j = np.arange(ww)
    x0 = np.clip(ipx + j, 0, W - 1)
    x1 = np.clip(ipx + j + 1, 0, W - 1)
    xl = min(max(ipx + rx, 0), W - 1)
    xr = min(max(ipx + rw, 0), W - 1)
    A, B = g[ya].astype(f32), g[yb].astype(f32)
    mid = A[:, x0] * a11 + A[:, x1] * a12 + B[:, x0] * a21 + B[:, x1] * a22
    lft = A[:, [xl]] * b1 + B[:, [xl]] * b2
    rgt = A[:, [xr]] * b1 + B[:, [xr]] * b2
    return np.where(j < rx, lft, np.where(j >= rw, rgt, mid)).astype(f32)


def corner_subpix(img, corners, win=(11, 11), criteria=(30, 1e-4), info=None):
    """cv::cornerSubPix(gray, corners, win, Size(-1, -1), TermCriteria(COUNT + EPS,
    max_iter, eps)); returns the refined (n, 2) f32 corners.  info: a list that
    receives (exit, iterations, reverted) per corner, exit one of "det" (singular
    normal matrix), "outside" (the update left the image), "criteria"."""
    g = gray(img)
    H, W = g.shape
    w, h = win
    if not (1 <= w <= MAX_WIN and 1 <= h <= MAX_WIN):
        raise ValueError("win is 1..15 per axis")
    ww, wh = 2 * w + 1, 2 * h + 1
    max_iter = min(max(int(criteria[0]), 1), 100)
    eps = max(float(criteria[1]), 0.0)
    eps *= eps
    vx, vy = subpix_mask(win)
    mask = (vy[:, None] * vx[None, :]).astype(f32).astype(f64)
    px = np.broadcast_to((np.arange(ww) - w).astype(f64)[None, :], (wh, ww))
    py = np.broadcast_to((np.arange(wh) - h).astype(f64)[:, None], (wh, ww))
    seq = lambda v: np.add.accumulate(np.concatenate(([0.0], v.ravel())))[-1]
    out = np.array(corners, f32).reshape(-1, 2).copy()
    for k in range(len(out)):
        cT = out[k].copy()
        cI = cT.copy()
        it = 0
        why = "criteria"
        while True:
            sub = rect_subpix(g, ww + 2, wh + 2, cI[0], cI[1])
            tgx = (sub[1:-1, 2:] - sub[1:-1, :-2]).astype(f64)
            tgy = (sub[2:, 1:-1] - sub[:-2, 1:-1]).astype(f64)
            gxx = tgx * tgx * mask
            gxy = tgx * tgy * mask
            gyy = tgy * tgy * mask
            a, b, c = seq(gxx), seq(gxy), seq(gyy)
            bb1 = seq(gxx * px + gxy * py)
            bb2 = seq(gxy * px + gyy * py)
            det = a * c - b * b
            if abs(det) <= np.finfo(f64).eps * np.finfo(f64).eps:
                why = "det"
                break
            scale = f64(1) / det
            c2 = np.array([f32(f64(cI[0]) + c * scale * bb1 - b * scale * bb2),
                           f32(f64(cI[1]) - b * scale * bb1 + a * scale * bb2)], f32)
            dx, dy = c2[0] - cI[0], c2[1] - cI[1]
            err = f64(f32(dx * dx) + f32(dy * dy))
            cI = c2
            if cI[0] < 0 or cI[0] >= W or cI[1] < 0 or cI[1] >= H:
                why = "outside"
                break
            it += 1
            if not (it < max_iter and err > eps):
                break
        reverted = bool(abs(cI[0] - cT[0]) > w or abs(cI[1] - cT[1]) > h)
        if reverted:
            cI = cT
        if info is not None:
            info.append((why, it, reverted))
        out[k] = cI
    return out


# ---- calibrateCamera ------------------------------------------------------------------

def board_points(board, square):
    """getObjectPoints (cameraCalibration.cpp:71-79): (bw * bh, 3) f32, z = 0"""
    bw, bh = board
    j, i = np.meshgrid(np.arange(bw), np.arange(bh))
    return np.stack([j.ravel() * square, i.ravel() * square, np.zeros(bw * bh)], 1).astype(np.float32)


def rodrigues(r):
    r = np.asarray(r, f64)
    th = np.linalg.norm(r)
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * Kx


def rodrigues_inv(R):
    U, _, Vt = np.linalg.svd(R)
    R = U @ Vt
    th = math.acos(min(1.0, max(-1.0, (np.trace(R) - 1) / 2)))
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-12:
        return v / 2
    return v / (2 * math.sin(th)) * th


def project(obj, K4, D, rvec, tvec):
    """pinhole + k1 k2 p1 p2 k3 projection in f64: (n, 2)"""
    fx, fy, cx, cy = K4
    k1, k2, p1, p2, k3 = D
    Y = np.asarray(obj, f64) @ rodrigues(rvec).T + np.asarray(tvec, f64)
    x, y = Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2]
    r2 = x * x + y * y
    rad = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], 1)


def _homography(xy, uv):
    """normalised DLT"""
    def norm(p):
        m = p.mean(0)
        s = math.sqrt(2) / np.mean(np.linalg.norm(p - m, axis=1))
        return np.array([[s, 0, -s * m[0]], [0, s, -s * m[1]], [0, 0, 1]])
    Ta, Tb = norm(xy), norm(uv)
    a = np.c_[xy, np.ones(len(xy))] @ Ta.T
    b = np.c_[uv, np.ones(len(uv))] @ Tb.T
    rows = []
    for (x, y, _), (u, v, _) in zip(a, b):
        rows.append([x, y, 1, 0, 0, 0, -u * x, -u * y, -u])
        rows.append([0, 0, 0, x, y, 1, -v * x, -v * y, -v])
    h = np.linalg.svd(np.array(rows))[2][-1].reshape(3, 3)
    Hm = np.linalg.inv(Tb) @ h @ Ta
    return Hm / Hm[2, 2]


def initial_values(obj, img, size):
    """principal point at the centre, fx fy from the homographies' vanishing-point
    equations, poses from K^-1 H, distortion 0: (9 intrinsics, rvecs, tvecs)"""
    obj = np.asarray(obj, f64)
    img = np.asarray(img, f64)
    cx, cy = (size[0] - 1) / 2, (size[1] - 1) / 2
    Hs = [_homography(obj[:, :2], v) for v in img]
    A, bvec = [], []
    for Hm in Hs:
        G = Hm.copy()
        G[0] -= G[2] * cx
        G[1] -= G[2] * cy
        h, v = G[:, 0], G[:, 1]
        d1, d2 = (h + v) / 2, (h - v) / 2
        h, v, d1, d2 = (z / np.linalg.norm(z) for z in (h, v, d1, d2))
        A += [[h[0] * v[0], h[1] * v[1]], [d1[0] * d2[0], d1[1] * d2[1]]]
        bvec += [-h[2] * v[2], -d1[2] * d2[2]]
    f = np.linalg.lstsq(np.array(A), np.array(bvec), rcond=None)[0]
    fx, fy = math.sqrt(abs(1 / f[0])), math.sqrt(abs(1 / f[1]))
    Ki = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]))
    rv, tv = [], []
    for Hm in Hs:
        M = Ki @ Hm
        if M[2, 2] < 0:
            M = -M
        lam = 1 / np.linalg.norm(M[:, 0])
        r1, r2, t = M[:, 0] * lam, M[:, 1] * lam, M[:, 2] * lam
        U, _, Vt = np.linalg.svd(np.stack([r1, r2, np.cross(r1, r2)], 1))
        rv.append(rodrigues_inv(U @ Vt))
        tv.append(t)
    return np.array([fx, fy, cx, cy, 0, 0, 0, 0, 0.0]), np.array(rv), np.array(tv)


def residuals(p, obj, img):
    n = len(img)
    r = [project(obj, p[:4], p[4:9], p[9 + 6 * v:12 + 6 * v], p[12 + 6 * v:15 + 6 * v]) - img[v] for v in range(n)]
    return np.concatenate(r).ravel()


def cost(obj, img, K4, D, rvecs, tvecs):
    """sum of squared reprojection residuals in f64 (rms^2 * nviews * npts)"""
    p = np.concatenate([np.asarray(K4, f64).ravel(), np.asarray(D, f64).ravel()[:5]] +
                       [np.r_[np.ravel(r), np.ravel(t)] for r, t in zip(rvecs, tvecs)])
    r = residuals(p, np.asarray(obj, f64), np.asarray(img, f64))
    return float(r @ r)


def calibrate(obj, img, size, tol=1e-15, x_scale="jac", method="lm"):
    """the optimum of calibrateCamera's default model by scipy's least_squares
    from initial_values: (rms, K 3x3, D 5, rvecs, tvecs, cost)"""
    from scipy.optimize import least_squares
    obj = np.asarray(obj, f64)
    img = np.asarray(img, f64)
    k0, rv, tv = initial_values(obj, img, size)
    p0 = np.concatenate([k0] + [np.r_[r, t] for r, t in zip(rv, tv)])
    sol = least_squares(residuals, p0, args=(obj, img), method=method, x_scale=x_scale,
                        xtol=tol, ftol=tol, gtol=tol, max_nfev=20000)
    p = sol.x
    n = len(img)
    c = float(sol.fun @ sol.fun)
    K = np.array([[p[0], 0, p[2]], [0, p[1], p[3]], [0, 0, 1]])
    ext = p[9:].reshape(n, 6)
    return math.sqrt(c / (n * len(obj))), K, p[4:9].copy(), ext[:, :3].copy(), ext[:, 3:].copy(), c

"""The contract of global bundle adjustment (csrc/gba.hip, csrc/gba_host.cpp, csrc/gba_math.h) in numpy.

Arithmetic rule: only + - * / and sqrt in IEEE f64, one rounding per operation (nothing contracted), every sum
in the order written here.  numpy's elementwise f64 operations obey that; where this file works on all
observations at once, every element goes through exactly the scalar expression, and no reduction of numpy
(sum, dot, @) touches a value whose bits matter.

The problem: n cameras (qw, qx, qy, qz, tx, ty, tz), X_c = R(q) X + t, camera 0 fixed; m points; constant
K4 = (fx, fy, cx, cy); observations (camera, point, x, y) with residual pi(X_c) - xy.

plan (fixed at entry):
  * an observation with z_c <= zmin is excluded ("behind"); then every observation of a point with fewer than
    two remaining ones is excluded; such points keep their bits;
  * the kept observations are sorted stably by camera: camera k owns the positions cam_off[k] .. cam_off[k + 1];
    a point's list holds its positions in ascending order;
  * held cameras: camera 0 and every camera without a kept observation; their J_c is 0.

sums:
  * per point: serially down its list;
  * per camera (cam_sum): lane l of 64 adds the camera's positions l, l + 64, ... ascending, then the lanes fold
    +32 .. +1 (loop_ref.lane_tree_sum's order);
  * over cameras or camera unknowns (dots; the cost as the sum of the per-camera costs): the 1024-lane tree.

One LM step at damping lam: per point C = sum J_p^T J_p with its diagonal times (1 + lam), a 3 x 3 Cholesky and
C^-1 column by column (all zero when a pivot is not in (0, 1e300): the point is frozen for this step); per camera
the 54 sums of cam_terms, the Cholesky factor of the Schur diagonal block (identity where it fails) and the
reduced right-hand side; PCG on S p = lam D p + sum J_c^T (J_c p_k - J_p w_p), w_p = C_p^-1 sum J_p^T (J_c p_k),
with pgo's stopping rule; back-substitution dX = C^-1 (g_p - sum J_p^T (J_c dc_k)); the step; the trial cost (+inf
when a kept observation comes to z_c <= zmin).  Accepted (cost lower): lam / 10; rejected: the state is restored,
lam x 10.  Huber enters as plain reweighting: r and J times sqrt(rho').
"""
import functools

import numpy as np

from loop_ref import lane_tree_sum, same_bits, world_case      # noqa: F401  (re-exported for the tests)

LANES, PCG_LANES = 64, 1024
K4 = (300.0, 280.0, 320.0, 240.0)
DEFAULTS = dict(loss=0, loss_param=1.0, zmin=0.1, lambda0=1e-4, max_lm=10, max_pcg=200, pcg_tol=1e-10, cost_tol=1e-9)
SUMMARY = ("cost0", "cost", "lm_steps", "accepted", "pcg_iters", "kept_obs", "behind_obs", "points_held", "cams_held")


# ---- small algebra, elementwise over a leading axis -------------------------------------------------

def quat_matrix(q):
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]


def camera_point(cams, X):
    R = quat_matrix(cams)
    Y = [(R[3 * i] * X[:, 0] + R[3 * i + 1] * X[:, 1]) + R[3 * i + 2] * X[:, 2] for i in range(3)]
    return R, (Y[0] + cams[:, 4], Y[1] + cams[:, 5], Y[2] + cams[:, 6])


def cam_step(cams, d):
    """q <- normalise(q (x) (1, dr / 2)), t <- t + dt, row by row"""
    a = cams
    b1, b2, b3 = d[:, 0] / 2.0, d[:, 1] / 2.0, d[:, 2] / 2.0
    w = ((a[:, 0] * 1.0 - a[:, 1] * b1) - a[:, 2] * b2) - a[:, 3] * b3
    x = ((a[:, 0] * b1 + a[:, 1] * 1.0) + a[:, 2] * b3) - a[:, 3] * b2
    y = ((a[:, 0] * b2 - a[:, 1] * b3) + a[:, 2] * 1.0) + a[:, 3] * b1
    z = ((a[:, 0] * b3 + a[:, 1] * b2) - a[:, 2] * b1) + a[:, 3] * 1.0
    nrm = np.sqrt(((w * w + x * x) + y * y) + z * z)
    return np.stack([w / nrm, x / nrm, y / nrm, z / nrm, a[:, 4] + d[:, 3], a[:, 5] + d[:, 4], a[:, 6] + d[:, 5]], 1)


def chol(A):
    """(L, ok) of a batch of symmetric N x N blocks, straight through"""
    b, N = A.shape[0], A.shape[1]
    Lm = np.zeros((b, N, N))
    ok = np.ones(b, bool)
    with np.errstate(all="ignore"):
        for j in range(N):
            d = A[:, j, j].copy()
            for k in range(j):
                d = d - Lm[:, j, k] * Lm[:, j, k]
            ok &= (d > 0.0) & (d < 1e300)
            Lm[:, j, j] = np.sqrt(d)
            for i in range(j + 1, N):
                v = A[:, i, j].copy()
                for k in range(j):
                    v = v - Lm[:, i, k] * Lm[:, j, k]
                Lm[:, i, j] = v / Lm[:, j, j]
    return Lm, ok


def chol_solve(Lm, r):
    b, N = r.shape
    y, z = np.zeros((b, N)), np.zeros((b, N))
    with np.errstate(all="ignore"):
        for i in range(N):
            v = r[:, i].copy()
            for k in range(i):
                v = v - Lm[:, i, k] * y[:, k]
            y[:, i] = v / Lm[:, i, i]
        for i in range(N - 1, -1, -1):
            v = y[:, i].copy()
            for k in range(i + 1, N):
                v = v - Lm[:, k, i] * z[:, k]
            z[:, i] = v / Lm[:, i, i]
    return z


def mul3(A, v):
    return np.stack([(A[:, i, 0] * v[:, 0] + A[:, i, 1] * v[:, 1]) + A[:, i, 2] * v[:, 2] for i in range(3)], 1)


# ---- the plan ----------------------------------------------------------------------------------------

class Plan:
    def __init__(self, cams, points, obs_cam, obs_point, obs_xy, zmin):
        cams, points = np.asarray(cams, np.float64).reshape(-1, 7), np.asarray(points, np.float64).reshape(-1, 3)
        oc, op = np.asarray(obs_cam, np.int64).reshape(-1), np.asarray(obs_point, np.int64).reshape(-1)
        xy = np.asarray(obs_xy, np.float64).reshape(-1, 2)
        self.n, self.m = len(cams), len(points)
        if len(oc):
            _, (_, _, z) = camera_point(cams[oc], points[op])
            front = z > zmin
        else:
            front = np.zeros(0, bool)
        left = np.bincount(op[front], minlength=self.m)
        keep = front & (left[op] >= 2)
        idx = np.flatnonzero(keep)
        idx = idx[np.argsort(oc[idx], kind="stable")]
        self.behind = int((~front).sum())
        self.nk = len(idx)
        self.obs_cam, self.obs_pt, self.xy = oc[idx], op[idx], xy[idx]
        self.cam_off = np.concatenate([[0], np.cumsum(np.bincount(self.obs_cam, minlength=self.n))]).astype(np.int64)
        self.pt_off = np.concatenate([[0], np.cumsum(np.bincount(self.obs_pt, minlength=self.m))]).astype(np.int64)
        self.pt_obs = np.argsort(self.obs_pt, kind="stable")
        self.cam_cnt, self.pt_cnt = np.diff(self.cam_off), np.diff(self.pt_off)
        self.held = self.cam_cnt == 0
        if self.n:
            self.held[0] = True
        self.local = np.arange(self.nk) - self.cam_off[self.obs_cam]

    def counts(self):
        return dict(kept_obs=self.nk, behind_obs=self.behind, points_held=int((self.pt_cnt == 0).sum()),
                    cams_held=int(self.held.sum()))

    def point_sum(self, terms):
        """(m, ...) sums of the (nk, ...) terms, serially down every point's list"""
        out = np.zeros((self.m,) + terms.shape[1:])
        for d in range(int(self.pt_cnt.max()) if self.m else 0):
            has = self.pt_cnt > d
            out[has] = out[has] + terms[self.pt_obs[self.pt_off[:-1][has] + d]]
        return out

    def cam_sum(self, terms):
        """(n, S) sums of the (nk, S) terms in the 64-lane order"""
        S = terms.shape[1]
        rows = max(1, (int(self.cam_cnt.max()) + LANES - 1) // LANES)
        pad = np.zeros((self.n, rows * LANES, S))
        pad[self.obs_cam, self.local] = terms
        pad = pad.reshape(self.n, rows, LANES, S)
        part = np.zeros((self.n, LANES, S))
        for r in range(rows):
            part = part + pad[:, r]
        off = LANES // 2
        while off >= 1:
            part[:, :off] = part[:, :off] + part[:, off:2 * off]
            off //= 2
        return part[:, 0]


# ---- one linearisation ----------------------------------------------------------------------------------

def obs_lin(cams, X, K, xy, loss, a, zmin, held):
    """per observation: r (k, 2), rho (k), J_c (k, 2, 6), J_p (k, 2, 3); cams, X, xy, held row by row"""
    fx, fy, cx, cy = (float(v) for v in K)
    a = float(a)
    with np.errstate(all="ignore"):
        R, (xc, yc, zc) = camera_point(cams, X)
        u, v = xc / zc, yc / zc
        r0, r1 = (fx * u + cx) - xy[:, 0], (fy * v + cy) - xy[:, 1]
        s = r0 * r0 + r1 * r1
        rho, w = s.copy(), np.ones(len(s))
        if loss == 1:
            big = s > a * a
            rs = np.sqrt(s[big])
            rho[big] = (2.0 * a) * rs - a * a
            w[big] = np.sqrt(a / rs)
        rho[~(zc > zmin)] = np.inf
        a0, a1 = fx / zc, fy / zc
        b0, b1 = -(a0 * u), -(a1 * v)
        M = [None] * 9
        for i in range(3):
            M[3 * i + 0] = R[3 * i + 2] * X[:, 1] - R[3 * i + 1] * X[:, 2]
            M[3 * i + 1] = R[3 * i + 0] * X[:, 2] - R[3 * i + 2] * X[:, 0]
            M[3 * i + 2] = R[3 * i + 1] * X[:, 0] - R[3 * i + 0] * X[:, 1]
        k = len(s)
        Jc, Jp = np.zeros((k, 2, 6)), np.zeros((k, 2, 3))
        for j in range(3):
            Jc[:, 0, j] = w * (a0 * M[j] + b0 * M[6 + j])
            Jc[:, 1, j] = w * (a1 * M[3 + j] + b1 * M[6 + j])
            Jp[:, 0, j] = w * (a0 * R[j] + b0 * R[6 + j])
            Jp[:, 1, j] = w * (a1 * R[3 + j] + b1 * R[6 + j])
        Jc[:, 0, 3], Jc[:, 0, 5] = w * a0, w * b0
        Jc[:, 1, 4], Jc[:, 1, 5] = w * a1, w * b1
        Jc[held] = 0.0
        return np.stack([w * r0, w * r1], 1), rho, Jc, Jp


def linearize(P, K, cams, X, prm):
    r, rho, Jc, Jp = obs_lin(cams[P.obs_cam], X[P.obs_pt], K, P.xy, prm["loss"], prm["loss_param"], prm["zmin"],
                             P.held[P.obs_cam])
    with np.errstate(all="ignore"):
        cost = lane_tree_sum(P.cam_sum(rho[:, None])[:, 0], PCG_LANES)
    return (r, Jc, Jp), cost


def point_blocks(P, lin, lam):
    r, Jc, Jp = lin
    pairs = [(i, j) for i in range(3) for j in range(i, 3)]
    C = P.point_sum(np.stack([Jp[:, 0, i] * Jp[:, 0, j] + Jp[:, 1, i] * Jp[:, 1, j] for i, j in pairs], 1))
    sp = P.point_sum(np.stack([Jp[:, 0, i] * r[:, 0] + Jp[:, 1, i] * r[:, 1] for i in range(3)], 1))
    A = np.zeros((P.m, 3, 3))
    for t, (i, j) in enumerate(pairs):
        A[:, i, j] = A[:, j, i] = C[:, t] + lam * C[:, t] if i == j else C[:, t]
    Lm, ok = chol(A)
    Ci = np.zeros((P.m, 3, 3))
    for j in range(3):
        e = np.zeros((P.m, 3))
        e[:, j] = 1.0
        Ci[:, :, j] = chol_solve(Lm, e)
    Ci[~ok] = 0.0
    return Ci, -sp, ok


def cam_terms(Jc, Jp, r, Ci, gp):
    W = np.stack([np.stack([Jc[:, 0, i] * Jp[:, 0, j] + Jc[:, 1, i] * Jp[:, 1, j] for j in range(3)], 1) for i in range(6)], 1)
    T = np.stack([np.stack([(W[:, i, 0] * Ci[:, 0, j] + W[:, i, 1] * Ci[:, 1, j]) + W[:, i, 2] * Ci[:, 2, j] for j in range(3)], 1)
                  for i in range(6)], 1)
    y = mul3(Ci, gp)
    out = [Jc[:, 0, i] * Jc[:, 0, j] + Jc[:, 1, i] * Jc[:, 1, j] for i in range(6) for j in range(i, 6)]
    out += [Jc[:, 0, i] * r[:, 0] + Jc[:, 1, i] * r[:, 1] for i in range(6)]
    out += [(T[:, i, 0] * W[:, j, 0] + T[:, i, 1] * W[:, j, 1]) + T[:, i, 2] * W[:, j, 2] for i in range(6) for j in range(i, 6)]
    out += [(W[:, i, 0] * y[:, 0] + W[:, i, 1] * y[:, 1]) + W[:, i, 2] * y[:, 2] for i in range(6)]
    return np.stack(out, 1)


def cam_blocks(P, lin, Ci, gp, lam):
    r, Jc, Jp = lin
    s = P.cam_sum(cam_terms(Jc, Jp, r, Ci[P.obs_pt], gp[P.obs_pt]))
    A, dl = np.zeros((P.n, 6, 6)), np.zeros((P.n, 6))
    t = 0
    for i in range(6):
        for j in range(i, 6):
            bij = s[:, t] + lam * s[:, t] if i == j else s[:, t]
            A[:, i, j] = A[:, j, i] = bij - s[:, 27 + t]
            if i == j:
                dl[:, i] = lam * s[:, t]
            t += 1
    Lm, ok = chol(A)
    Lm[~ok] = np.eye(6)
    return dl, Lm, (-s[:, 21:27]) - s[:, 48:54]


def jc_p(Jc, p):
    u = []
    for a in range(2):
        s = Jc[:, a, 0] * p[:, 0]
        for c in range(1, 6):
            s = s + Jc[:, a, c] * p[:, c]
        u.append(s)
    return u


def point_gather(P, lin, vec, Ci, gp, mode):
    _, Jc, Jp = lin
    u = jc_p(Jc, vec[P.obs_cam])
    v = P.point_sum(np.stack([Jp[:, 0, i] * u[0] + Jp[:, 1, i] * u[1] for i in range(3)], 1))
    if mode == 1:
        v = gp - v
    return mul3(Ci, v)


def apply_S(P, lin, dl, Ci, gp, p):
    _, Jc, Jp = lin
    w = point_gather(P, lin, p, Ci, gp, 0)[P.obs_pt]
    u = jc_p(Jc, p[P.obs_cam])
    e = [u[a] - ((Jp[:, a, 0] * w[:, 0] + Jp[:, a, 1] * w[:, 1]) + Jp[:, a, 2] * w[:, 2]) for a in range(2)]
    return dl * p + P.cam_sum(np.stack([Jc[:, 0, i] * e[0] + Jc[:, 1, i] * e[1] for i in range(6)], 1))


def dot(a, b):
    return lane_tree_sum((a * b).reshape(-1), PCG_LANES)


def pcg(P, lin, dl, Lm, Ci, gp, b, max_pcg, pcg_tol):
    x = np.zeros_like(b)
    r = b.copy()
    z = chol_solve(Lm, r)
    p = z.copy()
    rz = dot(r, z)
    rz0 = rz
    it = 0
    done = not (rz0 > 0.0)
    while it < max_pcg and not done:
        Ap = apply_S(P, lin, dl, Ci, gp, p)
        pAp = dot(p, Ap)
        if not (pAp > 0.0):
            break
        alpha = rz / pAp
        x = x + alpha * p
        r = r - alpha * Ap
        z = chol_solve(Lm, r)
        rzn = dot(r, z)
        it += 1
        if rzn <= pcg_tol * rz0:
            done = True
        else:
            p = z + (rzn / rz) * p
        rz = rzn
    return x, it


def gba(K, cams, points, obs_cam, obs_point, obs_xy, trace=None, **kw):
    """(cams, points, summary dict); trace: a list that receives (lambda, trial cost, accepted, PCG iterations,
    frozen points) per LM step"""
    prm = dict(DEFAULTS, **kw)
    C = np.array(cams, np.float64).reshape(-1, 7)
    X = np.array(points, np.float64).reshape(-1, 3)
    P = Plan(C, X, obs_cam, obs_point, obs_xy, prm["zmin"])
    out = dict(cost0=0.0, cost=0.0, lm_steps=0, accepted=0, pcg_iters=0, **P.counts())
    if P.n <= 1 or P.nk == 0:
        return C, X, out
    lin, c = linearize(P, K, C, X, prm)
    c0, lam, lm, acc, total = c, float(prm["lambda0"]), 0, 0, 0
    free = ~P.held
    seen = P.pt_cnt > 0
    while lm < prm["max_lm"] and c > 0.0:
        Ci, gp, ok = point_blocks(P, lin, lam)
        dl, Lm, b = cam_blocks(P, lin, Ci, gp, lam)
        x, it = pcg(P, lin, dl, Lm, Ci, gp, b, prm["max_pcg"], prm["pcg_tol"])
        total += it
        dX = point_gather(P, lin, x, Ci, gp, 1)
        Ct, Xt = C.copy(), X.copy()
        with np.errstate(all="ignore"):
            Ct[free] = cam_step(C[free], x[free])
            Xt[seen] = X[seen] + dX[seen]
        lint, ct = linearize(P, K, Ct, Xt, prm)
        lm += 1
        good = bool(ct < c)
        if trace is not None:
            trace.append((lam, ct, good, it, int((~ok & seen).sum())))
        if good:
            rel = (c - ct) / c
            C, X, lin, c = Ct, Xt, lint, ct
            acc += 1
            lam = lam / 10.0
            if rel < prm["cost_tol"]:
                break
        else:
            lam = lam * 10.0
    out.update(cost0=c0, cost=c, lm_steps=lm, accepted=acc, pcg_iters=total)
    return C, X, out


def residuals(K, cams, points, obs_cam, obs_point, obs_xy):
    """plain residuals (k, 2) and depths of observations, for the tests' own measurements"""
    cams, points = np.asarray(cams, np.float64).reshape(-1, 7), np.asarray(points, np.float64).reshape(-1, 3)
    oc, op = np.asarray(obs_cam, np.int64), np.asarray(obs_point, np.int64)
    xy = np.asarray(obs_xy, np.float64).reshape(-1, 2)
    _, (xc, yc, zc) = camera_point(cams[oc], points[op])
    return np.stack([K[0] * (xc / zc) + K[2] - xy[:, 0], K[1] * (yc / zc) + K[3] - xy[:, 1]], 1), zc


# ---- cases ----------------------------------------------------------------------------------------------

def _quat(rng, angle):
    ax = rng.normal(size=3)
    ax = ax / np.linalg.norm(ax)
    ang = float(rng.uniform(-angle, angle))
    return np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax])


def synth(n, m, pairs, seed, noise=0.3, rot=0.01, trans=0.02, pts=0.03, outliers=0.0, shuffle=True):
    """n cameras looking down +z at m points 4 to 6 in front; pairs: (camera, point) rows.  Pixels are the f32
    projections of the true scene plus noise; the start is the true scene perturbed, camera 0 exact."""
    rng = np.random.default_rng(seed)
    gtX = np.stack([rng.uniform(-1.5, 1.5, m), rng.uniform(-1, 1, m), rng.uniform(4, 6, m)], 1)
    gtC = np.array([np.concatenate([_quat(rng, 0.15), rng.uniform(-0.5, 0.5, 3)]) for _ in range(n)]).reshape(-1, 7)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    if shuffle:
        pairs = pairs[rng.permutation(len(pairs))]
    res, _ = residuals(K4, gtC, gtX, pairs[:, 0], pairs[:, 1], np.zeros((len(pairs), 2)))
    xy = res + noise * rng.normal(size=res.shape)
    bad = rng.random(len(pairs)) < outliers
    xy[bad] += rng.uniform(-60, 60, (int(bad.sum()), 2))
    xy = xy.astype(np.float32).astype(np.float64)
    C = gtC.copy()
    for k in range(1, n):
        C[k:k + 1] = cam_step(C[k:k + 1], np.concatenate([rng.normal(size=3) * rot, rng.normal(size=3) * trans])[None])
    X = gtX + pts * rng.normal(size=gtX.shape)
    return dict(K=K4, cams=C, points=X, obs_cam=pairs[:, 0].astype(np.int32), obs_point=pairs[:, 1].astype(np.int32),
                obs_xy=xy, gt_cams=gtC, gt_points=gtX)


def _full(n, m):
    return [(k, p) for k in range(n) for p in range(m)]


@functools.lru_cache(maxsize=None)
def gba_cases():
    """name -> (problem dict, keyword arguments)"""
    cases = {}
    # cameras 1 .. 6 with 0, 1, 63, 64, 65 and 129 observations; camera 0 sees every point, so each has two
    tree = [(0, p) for p in range(129)] + [(6, p) for p in range(129)]
    for k, cnt in ((2, 1), (3, 63), (4, 64), (5, 65)):
        tree += [(k, p) for p in range(cnt)]
    cases["tree"] = (synth(7, 129, tree, 1), dict(max_lm=4))
    # points with two observations and points seen by every camera
    lists = _full(5, 3) + [(0, 3), (4, 3), (1, 4), (2, 4), (2, 5), (3, 5)] + [(k, p) for k in range(5) for p in range(6, 20) if (k + p) % 2]
    cases["lists"] = (synth(5, 20, lists, 2), dict(max_lm=4))
    # camera 2 sees point 1 twice (two pixels): both stay, as two residuals
    cases["repeat"] = (synth(4, 12, _full(4, 12) + [(2, 1), (2, 1)], 3), dict(max_lm=4))
    cases["two"] = (synth(2, 30, _full(2, 30), 4), dict(max_lm=4))
    cases["one"] = (synth(1, 10, _full(1, 10) + _full(1, 10), 5), {})
    cases["empty"] = (synth(3, 5, [], 5), {})
    # camera 3 looks the other way: its observations of points 0 and 1 are behind it.  Point 0 keeps two others;
    # point 1 had one other, which the second stage removes: point 1 is held and so is camera 3
    behind = synth(4, 10, [(k, p) for k in range(3) for p in range(2, 10)] + [(0, 0), (1, 0), (3, 0), (2, 1), (3, 1)], 6)
    behind["cams"][3, :4] = (0.0, 0.0, 1.0, 0.0)
    cases["behind"] = (behind, dict(max_lm=3))
    # cameras 1 and 2 share one pose and see point 0 at one pixel: two parallel rays, a rank-2 block
    for name, lam0 in (("parallel_l0", 0.0), ("parallel", 1e-4)):
        par = synth(4, 16, [(k, p) for k in range(4) for p in range(1, 16)] + [(1, 0), (2, 0)], 7)
        par["cams"][2] = par["cams"][1]
        sel = par["obs_point"] == 0
        par["obs_xy"][sel] = par["obs_xy"][sel][0]
        cases[name] = (par, dict(max_lm=3, lambda0=lam0))
    # more cameras than the 1024-lane tree has lanes, 3 observations each
    many = [(k, (k + d) % 1030) for k in range(1030) for d in range(3)]
    cases["many"] = (synth(1030, 1030, many, 8), dict(max_lm=2, max_pcg=24))
    out = synth(6, 60, _full(6, 60), 9, outliers=0.1)
    cases["huber"] = (out, dict(loss=1, loss_param=2.0, max_lm=5))
    cases["huber_off"] = (out, dict(max_lm=5))
    # no damping far from the minimum: the first step overshoots and is rejected
    cases["reject"] = (synth(5, 40, _full(5, 40), 10, rot=0.25, trans=0.6, pts=0.8), dict(lambda0=1e-9, max_lm=6))
    # the least depth a hair under the nearest kept observation: the first trial brings one to z_c <= zmin, costs +inf
    # and is rejected
    near = synth(4, 20, _full(4, 20), 22, rot=0.05, trans=0.2, pts=0.3)
    _, z = residuals(K4, near["cams"], near["points"], near["obs_cam"], near["obs_point"], near["obs_xy"])
    cases["zreject"] = (near, dict(zmin=float(z.min()) - 1e-3, max_lm=4))
    base = synth(8, 50, [(k, p) for k in range(8) for p in range(50) if (k * 7 + p) % 3], 11)
    cases["pcg0"] = (base, dict(max_pcg=0, max_lm=2))
    cases["pcg13"] = (base, dict(max_pcg=13, pcg_tol=0.0, max_lm=2))
    cases["pcg_loose"] = (base, dict(pcg_tol=1e-3, max_lm=2))
    cases["lm0"] = (base, dict(max_lm=0))
    return cases


GBA_NAMES = ("tree", "lists", "repeat", "two", "one", "empty", "behind", "parallel_l0", "parallel", "many", "huber",
             "huber_off", "reject", "zreject", "pcg0", "pcg13", "pcg_loose", "lm0")


@functools.lru_cache(maxsize=None)
def gba_expected(name):
    """(cams, points, summary, trace) of the reference on a named case"""
    W, kw = gba_cases()[name]
    trace = []
    C, X, s = gba(W["K"], W["cams"], W["points"], W["obs_cam"], W["obs_point"], W["obs_xy"], trace=trace, **kw)
    return C, X, s, trace

"""One Levenberg-Marquardt step of the windowed bundle adjustment, restated as
plainly as possible in extended precision -- TEST INFRASTRUCTURE.

oracle/ba.c follows Ceres closely (jets, Schur elimination, point-wise sums)
and csrc/ba.hip was written against it, so a formula error shared by both
would pass every oracle comparison.  This reference shares nothing with either:

  * residuals as plain formulas (angle-axis rotation with Ceres's
    th2 > DBL_EPSILON branch rule, + t, pinhole projection);
  * the Jacobian by complex-step differentiation (h = 1e-40: no subtraction,
    so no cancellation; the truncation error h^2 is far below the mantissa);
  * Ceres's Corrector (corrector.cc) with rho, rho', rho'' of each loss written
    from its formula (loss_function.h);
  * a DENSE Jacobian: no Schur complement, no per-point elimination;
  * numpy longdouble / clongdouble (64-bit mantissa on x86);
  * a hand-written Cholesky.

It imports neither the oracle nor the library.

Tangent layout (the oracle's): K4, then ext[1:] (frame 0 is constant), then
the points: N = 4 + 6 (nf - 1) + 3 np.
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
LOSS_NONE, LOSS_TRIVIAL, LOSS_HUBER, LOSS_CAUCHY, LOSS_ARCTAN, LOSS_TUKEY = range(6)
H_STEP = LD("1e-40")
EPS = LD(np.finfo(np.float64).eps)
DBL_MIN = LD(np.finfo(np.float64).tiny)


def residuals(K, e, X, xy):
    """K (n, 4), e (n, 6), X (n, 3), xy (n, 2), real or complex extended
    precision; returns the reprojection residuals (n, 2)"""
    aa, t = e[:, :3], e[:, 3:]
    th2 = (aa * aa).sum(1)
    big = th2.real > EPS
    th = np.sqrt(np.where(big, th2, 1))
    w = aa / th[:, None]
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    full = X * c + np.cross(w, X) * s + w * ((w * X).sum(1)[:, None] * (1 - c))
    small = X + np.cross(aa, X)
    P = np.where(big[:, None], full, small) + t
    u = K[:, 0] * (P[:, 0] / P[:, 2]) + K[:, 2] - xy[:, 0]
    v = K[:, 1] * (P[:, 1] / P[:, 2]) + K[:, 3] - xy[:, 1]
    return np.stack([u, v], 1)


def rho(loss, a, s):
    """rho(s), rho'(s), rho''(s) of Ceres's loss functions, s = |r|^2 (n,)"""
    a = LD(a)
    one = np.ones_like(s)
    if loss == LOSS_HUBER:
        out = s > a * a
        r = np.sqrt(np.where(out, s, 1))
        r1 = np.maximum(DBL_MIN, a / r)
        return (np.where(out, 2 * a * r - a * a, s), np.where(out, r1, one),
                np.where(out, -r1 / (2 * np.where(out, s, 1)), 0 * one))
    if loss == LOSS_CAUCHY:
        b = a * a
        q = 1 + s / b
        return b * np.log(q), np.maximum(DBL_MIN, 1 / q), -(1 / b) / (q * q)
    if loss == LOSS_ARCTAN:
        b = 1 / (a * a)
        q = 1 + s * s * b
        return a * np.arctan2(s, a), np.maximum(DBL_MIN, 1 / q), -2 * s * b / (q * q)
    if loss == LOSS_TUKEY:
        a2 = a * a
        inside = s <= a2
        v = np.where(inside, 1 - s / a2, 0)
        return a2 / 3 * (1 - v * v * v), v * v, np.where(inside, -2 / a2 * v, 0 * one)
    return s, one, 0 * one


def _gather(w, x):
    nf, npt = len(w["ext"]), len(w["pts"])
    nc = 4 + 6 * (nf - 1)
    of, op = np.asarray(w["obs_frame"]), np.asarray(w["obs_point"])
    E = np.concatenate([np.asarray(w["ext"][:1], LD).reshape(1, 6), x[4:nc].reshape(nf - 1, 6)])
    X = x[nc:].reshape(npt, 3)
    K = np.broadcast_to(x[:4], (len(of), 4))
    return K, E[of], X[op]


def pack(w):
    return np.concatenate([np.asarray(w["K4"], LD).ravel(), np.asarray(w["ext"][1:], LD).ravel(),
                           np.asarray(w["pts"], LD).ravel()])


def cost_at(w, loss, a, x):
    """0.5 sum rho(|r|^2) at tangent vector x"""
    xy = np.asarray(w["obs_xy"], LD).reshape(-1, 2)
    if len(xy) == 0:
        return LD(0)
    r = residuals(*_gather(w, x), xy)
    s = (r * r).sum(1)
    return 0.5 * (s if loss == LOSS_NONE else rho(loss, a, s)[0]).sum()


def cholesky_solve(A, b):
    """A y = b, A symmetric positive definite, in A's precision (left-looking
    LL', one column per pass); a non-positive pivot gives NaNs"""
    n = len(b)
    L = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for j in range(n):
            col = A[j:, j] - L[j:, :j] @ L[j, :j]
            L[j:, j] = col / np.sqrt(col[0])
        y = np.array(b)
        for j in range(n):
            y[j] = (y[j] - L[j, :j] @ y[:j]) / L[j, j]
        for j in range(n - 1, -1, -1):
            y[j] = (y[j] - L[j + 1:, j] @ y[j + 1:]) / L[j, j]
    return y


def dense_step(w, loss=LOSS_NONE, a=0.0, radius=1e4):
    """Ceres's first LM step on window w: returns (K4, ext, pts, cost) after
    the step as float64 arrays / float (the candidate point, whether or not LM
    would accept it), and the extended-precision tangent vector before and
    after under "x0" / "x1" of the returned dict `info`."""
    nf, npt = len(w["ext"]), len(w["pts"])
    nc = 4 + 6 * (nf - 1)
    N = nc + 3 * npt
    of, op = np.asarray(w["obs_frame"]), np.asarray(w["obs_point"])
    xy = np.asarray(w["obs_xy"], LD).reshape(-1, 2)
    no = len(of)
    x0 = pack(w)
    K, e, X = _gather(w, x0)
    with np.errstate(all="ignore"):
        r = residuals(K, e, X, xy)
        # complex step: d r / d p_i = Im r(p + i h e_i) / h
        loc = np.concatenate([K, e, X], 1).astype(CLD)
        J = np.empty((no, 2, 13), LD)
        for i in range(13):
            q = loc.copy()
            q[:, i] += 1j * H_STEP
            J[:, :, i] = residuals(q[:, :4], q[:, 4:10], q[:, 10:], xy.astype(CLD)).imag / H_STEP
        if loss != LOSS_NONE:
            s = (r * r).sum(1)
            _, r1, r2 = rho(loss, a, s)
            sr1 = np.sqrt(r1)
            plain = (s == 0) | (r2 <= 0)
            D = 1 + 2 * s * np.where(plain, 0, r2) / r1
            alpha = np.where(plain, 0, 1 - np.sqrt(D))
            asn = np.where(plain, 0, alpha / np.where(s == 0, 1, s))
            rtj = (J * r[:, :, None]).sum(1)                       # (no, 13)
            J = sr1[:, None, None] * (J - asn[:, None, None] * r[:, :, None] * rtj[:, None, :])
            r = r * (sr1 / (1 - alpha))[:, None]
        # the dense Jacobian: row 2 o + k, tangent columns (frame 0's extrinsics have none)
        Jd = np.zeros((2 * no, N), LD)
        rows = 2 * np.arange(no)
        for k in range(2):
            for i in range(13):
                if i < 4:
                    cols, m = np.full(no, i), np.ones(no, bool)
                elif i < 10:
                    cols, m = 4 + 6 * (of - 1) + (i - 4), of > 0
                else:
                    cols, m = nc + 3 * op + (i - 10), np.ones(no, bool)
                np.add.at(Jd, (rows[m] + k, cols[m]), J[m, k, i])
        scale = 1 / (1 + np.sqrt((Jd * Jd).sum(0)))
        Js = Jd * scale
        Hm = Js.T @ Js
        g = Js.T @ r.reshape(-1)
        A = Hm + np.diag(np.clip(np.diag(Hm), LD("1e-6"), LD("1e32")) / LD(radius))
        y = cholesky_solve(A, g)
        x1 = x0 - scale * y
        cost = cost_at(w, loss, a, x1)
    K4 = x1[:4].astype(np.float64)
    ext = np.array(w["ext"], np.float64)
    ext[1:] = x1[4:nc].reshape(nf - 1, 6).astype(np.float64)
    pts = x1[nc:].reshape(npt, 3).astype(np.float64)
    return K4, ext, pts, float(cost), {"x0": x0, "x1": x1, "scale": scale, "grad": Jd.T @ r.reshape(-1)}

"""The contract of loop closing (csrc/loop.hip, csrc/loop_host.cpp, csrc/loop_math.h) in numpy.

Arithmetic rule: only + - * / and sqrt in IEEE f64, one rounding per operation (nothing
contracted), every sum in the order written here.  Python floats and numpy's elementwise
f64 operations obey that, so the device, the host twin and this file agree bit for bit.
Where this file works on a whole array of pairs at once, every element goes through
exactly the scalar expression; no reduction of numpy (sum, dot, @) is used on values
whose bits matter.

A similarity is S = (sigma, qw, qx, qy, qz, tx, ty, tz), x' = sigma R(q) x + t, q a unit
quaternion.  compose(A, B) applies B first; inverse(S) undoes S.  A local step is
sigma <- sigma (1 + ds), q <- normalise(q (x) (1, dr / 2)), t <- t + dt.

sim3_ransac, per loop with pairs a_k, b_k (b ~ s R a + t), camera centres ci (of a), cj (of b):
  * samples: hypothesis h of loop l uses the three distinct indices sample(seed, l, h, n);
  * hypothesis: Gram-Schmidt frames Fa, Fb on the two triangles (frame()), R = Fb Fa^T,
    s = sqrt(spread(b) / spread(a)), q = normalise(shepperd(R)), t = mean(b) - s R(q) mean(a);
    a triangle with |u x v|^2 <= 1e-12 |u|^2 |v|^2 gives no hypothesis (0 inliers);
  * inlier: e2 = |b - (s R a + t)|^2 <= tau^2 |b - cj|^2 and e2 <= (tau^2 (s s)) |a - ci|^2;
  * winner: most inliers, ties to the lowest h; fewer than 3 inliers: NO_MODEL;
  * refit: REFIT_STEPS Gauss-Newton steps on r = b - (s R(q) a + t) over the winner's inliers.
    The 35 sums of a step (upper triangle of J^T J row by row, then J^T r): lane l = k mod 64
    adds its pairs in ascending k (a pair outside the mask adds +0.0), then the 64 lanes fold
    as a binary tree: for off in 32, 16, .. 1: lane[l] += lane[l + off] for l < off.  The 7 x 7
    system is solved by Cholesky (chol7_solve); a pivot that is not positive ends the refit
    with status CHOLESKY and the state reached so far.
"""
import math

import numpy as np

OK, NO_MODEL, TOO_FEW, CHOLESKY = 0, 1, 2, 3
REFIT_STEPS = 4
LANES = 64
DEGENERATE = 1e-12
M64 = (1 << 64) - 1
IDENTITY = (1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes()


# ---- the sample generator -------------------------------------------------------------------

def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def draw(seed, loop, hyp, k):
    ctr = ((loop << 40) ^ (hyp << 8) ^ k) & M64
    return _mix64(_mix64((seed + 0x9e3779b97f4a7c15) & M64) ^ ((ctr * 0x9e3779b97f4a7c15 + 0x632be59bd9b4e019) & M64))


def sample(seed, loop, hyp, n):
    i0 = draw(seed, loop, hyp, 0) % n
    i1 = draw(seed, loop, hyp, 1) % (n - 1)
    if i1 >= i0:
        i1 += 1
    i2 = draw(seed, loop, hyp, 2) % (n - 2)
    lo, hi = min(i0, i1), max(i0, i1)
    if i2 >= lo:
        i2 += 1
    if i2 >= hi:
        i2 += 1
    return i0, i1, i2


# ---- vectors, quaternions, similarities (scalars or arrays per component) -----------------------

def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross3(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def quat_mul(a, b):
    return (((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3],
            ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2],
            ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1],
            ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0])


def quat_normalise(q):
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return (q[0] / n, q[1] / n, q[2] / n, q[3] / n)


def quat_matrix(q):
    w, x, y, z = q
    return (1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y))


def matrix_quat(R):
    tr = (R[0] + R[4]) + R[8]
    if tr > 0.0:
        r = math.sqrt(1.0 + tr)
        f = 0.5 / r
        q = (0.5 * r, (R[7] - R[5]) * f, (R[2] - R[6]) * f, (R[3] - R[1]) * f)
    elif R[0] >= R[4] and R[0] >= R[8]:
        r = math.sqrt(((1.0 + R[0]) - R[4]) - R[8])
        f = 0.5 / r
        q = ((R[7] - R[5]) * f, 0.5 * r, (R[1] + R[3]) * f, (R[2] + R[6]) * f)
    elif R[4] >= R[8]:
        r = math.sqrt(((1.0 + R[4]) - R[0]) - R[8])
        f = 0.5 / r
        q = ((R[2] - R[6]) * f, (R[1] + R[3]) * f, 0.5 * r, (R[5] + R[7]) * f)
    else:
        r = math.sqrt(((1.0 + R[8]) - R[0]) - R[4])
        f = 0.5 / r
        q = ((R[3] - R[1]) * f, (R[2] + R[6]) * f, (R[5] + R[7]) * f, 0.5 * r)
    return quat_normalise(q)


def mat_vec(R, v):
    return ((R[0] * v[0] + R[1] * v[1]) + R[2] * v[2],
            (R[3] * v[0] + R[4] * v[1]) + R[5] * v[2],
            (R[6] * v[0] + R[7] * v[1]) + R[8] * v[2])


def mat_t_vec(R, v):
    return ((R[0] * v[0] + R[3] * v[1]) + R[6] * v[2],
            (R[1] * v[0] + R[4] * v[1]) + R[7] * v[2],
            (R[2] * v[0] + R[5] * v[1]) + R[8] * v[2])


def sim3_map(sigma, R, t, x):
    y = mat_vec(R, x)
    return (sigma * y[0] + t[0], sigma * y[1] + t[1], sigma * y[2] + t[2])


def apply(S, x):
    """sigma R(q) x + t (x: 3 scalars or 3 arrays)"""
    return sim3_map(S[0], quat_matrix(S[1:5]), S[5:8], x)


def compose(A, B):
    """the similarity x -> A(B(x))"""
    q = quat_mul(A[1:5], B[1:5])
    t = sim3_map(A[0], quat_matrix(A[1:5]), A[5:8], B[5:8])
    return (A[0] * B[0],) + tuple(q) + tuple(t)


def inverse(S):
    qc = (S[1], -S[2], -S[3], -S[4])
    y = mat_vec(quat_matrix(qc), S[5:8])
    return (1.0 / S[0],) + qc + (-(y[0] / S[0]), -(y[1] / S[0]), -(y[2] / S[0]))


def step(S, d):
    q = quat_normalise(quat_mul(S[1:5], (1.0, d[1] / 2.0, d[2] / 2.0, d[3] / 2.0)))
    return (S[0] * (1.0 + d[0]),) + q + (S[5] + d[4], S[6] + d[5], S[7] + d[6])


# ---- the hypothesis -----------------------------------------------------------------------------

def frame(p0, p1, p2):
    """F[r * 3 + k] = e_k[r], or None"""
    u = tuple(p1[k] - p0[k] for k in range(3))
    v = tuple(p2[k] - p0[k] for k in range(3))
    c = cross3(u, v)
    lu2, lv2, lc2 = dot3(u, u), dot3(v, v), dot3(c, c)
    if not (lc2 > (DEGENERATE * lu2) * lv2) or not (lc2 < 1e300):
        return None
    lu = math.sqrt(lu2)
    e1 = tuple(u[k] / lu for k in range(3))
    d = dot3(v, e1)
    w = tuple(v[k] - d * e1[k] for k in range(3))
    lw = math.sqrt(dot3(w, w))
    if not (lw > 0.0):
        return None
    e2 = tuple(w[k] / lw for k in range(3))
    e3 = cross3(e1, e2)
    return tuple(x for r in range(3) for x in (e1[r], e2[r], e3[r]))


def spread(p0, p1, p2):
    mean = tuple(((p0[k] + p1[k]) + p2[k]) / 3.0 for k in range(3))
    d = [tuple(p[k] - mean[k] for k in range(3)) for p in (p0, p1, p2)]
    return (dot3(d[0], d[0]) + dot3(d[1], d[1])) + dot3(d[2], d[2]), mean


def hypothesis(a0, a1, a2, b0, b1, b2):
    a0, a1, a2, b0, b1, b2 = [tuple(float(x) for x in p) for p in (a0, a1, a2, b0, b1, b2)]
    Fa, Fb = frame(a0, a1, a2), frame(b0, b1, b2)
    if Fa is None or Fb is None:
        return None
    R = tuple((Fb[r * 3] * Fa[c * 3] + Fb[r * 3 + 1] * Fa[c * 3 + 1]) + Fb[r * 3 + 2] * Fa[c * 3 + 2]
              for r in range(3) for c in range(3))
    sa, ma = spread(a0, a1, a2)
    sb, mb = spread(b0, b1, b2)
    if not (sa > 0.0):
        return None
    s = math.sqrt(sb / sa)
    if not (s > 0.0) or not (s < 1e300):
        return None
    q = matrix_quat(R)
    if q[0] != q[0]:
        return None
    y = mat_vec(quat_matrix(q), ma)
    return (s,) + q + (mb[0] - s * y[0], mb[1] - s * y[1], mb[2] - s * y[2])


# ---- scoring and the refit (arrays over the pairs) ----------------------------------------------

def _cols(p):
    p = np.asarray(p, np.float64).reshape(-1, 3)
    return (p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy())


def dist2(p, c):
    d = (p[0] - c[0], p[1] - c[1], p[2] - c[2])
    return dot3(d, d)


def inliers(S, a, b, da2, db2, tau2):
    """bool per pair; a, b: column triples"""
    p = sim3_map(S[0], quat_matrix(S[1:5]), S[5:8], a)
    e = (b[0] - p[0], b[1] - p[1], b[2] - p[2])
    e2 = dot3(e, e)
    return (e2 <= tau2 * db2) & (e2 <= (tau2 * (S[0] * S[0])) * da2)


def terms(S, a, b):
    """the 35 terms of every pair: list of 35 arrays"""
    s, R, t = S[0], quat_matrix(S[1:5]), S[5:8]
    y = mat_vec(R, a)
    one, zero = np.ones_like(a[0]), np.zeros_like(a[0])
    J, r = [], []
    for k in range(3):
        p = s * y[k]
        r.append(b[k] - (p + t[k]))
        J.append([p,
                  s * (R[k * 3 + 2] * a[1] - R[k * 3 + 1] * a[2]),
                  s * (R[k * 3 + 0] * a[2] - R[k * 3 + 2] * a[0]),
                  s * (R[k * 3 + 1] * a[0] - R[k * 3 + 0] * a[1]),
                  one if k == 0 else zero, one if k == 1 else zero, one if k == 2 else zero])
    out = []
    for i in range(7):
        for j in range(i, 7):
            out.append((J[0][i] * J[0][j] + J[1][i] * J[1][j]) + J[2][i] * J[2][j])
    for i in range(7):
        out.append((J[0][i] * r[0] + J[1][i] * r[1]) + J[2][i] * r[2])
    return out


def lane_tree_sum(v, lanes=LANES):
    """the stated order: `lanes` strided partial sums in ascending k, then the binary tree"""
    n = len(v)
    rows = (n + lanes - 1) // lanes
    pad = np.zeros(rows * lanes, np.float64)
    pad[:n] = v
    pad = pad.reshape(rows, lanes)
    part = np.zeros(lanes, np.float64)
    for r in range(rows):
        part = part + pad[r]
    off = lanes // 2
    while off >= 1:
        part[:off] = part[:off] + part[off:2 * off]
        off //= 2
    return float(part[0])


def chol7_solve(upper, g):
    A = [[0.0] * 7 for _ in range(7)]
    o = 0
    for i in range(7):
        for j in range(i, 7):
            A[i][j] = A[j][i] = upper[o]
            o += 1
    Lm = [[0.0] * 7 for _ in range(7)]
    for j in range(7):
        d = A[j][j]
        for k in range(j):
            d = d - Lm[j][k] * Lm[j][k]
        if not (d > 0.0) or not (d < 1e300):
            return None
        Lm[j][j] = math.sqrt(d)
        for i in range(j + 1, 7):
            v = A[i][j]
            for k in range(j):
                v = v - Lm[i][k] * Lm[j][k]
            Lm[i][j] = v / Lm[j][j]
    y = [0.0] * 7
    for i in range(7):
        v = g[i]
        for k in range(i):
            v = v - Lm[i][k] * y[k]
        y[i] = v / Lm[i][i]
    x = [0.0] * 7
    for i in range(6, -1, -1):
        v = y[i]
        for k in range(i + 1, 7):
            v = v - Lm[k][i] * x[k]
        x[i] = v / Lm[i][i]
    return x


def ransac_one(a, b, ci, cj, H, tau, seed, loop):
    """(S (8), mask uint8[n], count, status) of one loop"""
    a, b = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
    n = len(a)
    mask = np.zeros(n, np.uint8)
    if n < 3:
        return IDENTITY, mask, 0, TOO_FEW
    ac, bc = _cols(a), _cols(b)
    ci, cj = [float(x) for x in ci], [float(x) for x in cj]
    tau2 = float(tau) * float(tau)
    da2, db2 = dist2(ac, ci), dist2(bc, cj)
    best, best_S, best_in = 0, None, None
    for h in range(H):
        i0, i1, i2 = sample(seed, loop, h, n)
        S = hypothesis(a[i0], a[i1], a[i2], b[i0], b[i1], b[i2])
        if S is None:
            continue
        inl = inliers(S, ac, bc, da2, db2, tau2)
        cnt = int(inl.sum())
        if cnt > best:
            best, best_S, best_in = cnt, S, inl
    if best < 3:
        return IDENTITY, mask, 0, NO_MODEL
    mask = best_in.astype(np.uint8)
    S, status = best_S, OK
    for _ in range(REFIT_STEPS):
        tm = terms(S, ac, bc)
        sums = [lane_tree_sum(np.where(best_in, t, 0.0)) for t in tm]
        d = chol7_solve(sums[:28], sums[28:])
        if d is None:
            status = CHOLESKY
            break
        S = step(S, d)
    return S, mask, best, status


def sim3_ransac(a, b, offsets, centres, H, tau, seed):
    """(sim L x 8 f64, mask uint8[len(a)], count int32[L], status int32[L]); pairs outside
    [offsets[0], offsets[L]) keep mask 0"""
    a, b = np.asarray(a, np.float64).reshape(-1, 3), np.asarray(b, np.float64).reshape(-1, 3)
    centres = np.asarray(centres, np.float64).reshape(-1, 6)
    L = len(offsets) - 1
    sim = np.zeros((L, 8), np.float64)
    mask = np.zeros(len(a), np.uint8)
    count, status = np.zeros(L, np.int32), np.zeros(L, np.int32)
    for l in range(L):
        lo, hi = int(offsets[l]), int(offsets[l + 1])
        S, m, c, st = ransac_one(a[lo:hi], b[lo:hi], centres[l, :3], centres[l, 3:], H, tau, seed, l)
        sim[l], mask[lo:hi], count[l], status[l] = S, m, c, st
    return sim, mask, count, status


# ---- the map correction ---------------------------------------------------------------------------

def move_point(S, Sn, X):
    S, Sn = tuple(float(v) for v in S), tuple(float(v) for v in Sn)
    if all(S[k] == Sn[k] for k in range(8)):
        return tuple(X)
    Y = sim3_map(S[0], quat_matrix(S[1:5]), S[5:8], X)
    d = (Y[0] - Sn[5], Y[1] - Sn[6], Y[2] - Sn[7])
    z = mat_t_vec(quat_matrix(Sn[1:5]), d)
    return (z[0] / Sn[0], z[1] / Sn[0], z[2] / Sn[0])


def apply_points(points, anchor, nodes, nodes_new):
    """X' = S'^-1 (S (X)) with S, S' the anchor's node before and after; anchor -1 keeps X"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    out = points.copy()
    for i, an in enumerate(np.asarray(anchor)):
        if an >= 0:
            out[i] = move_point(nodes[an], nodes_new[an], tuple(float(v) for v in points[i]))
    return out


# ---- the pose graph over Sim(3) -------------------------------------------------------------------
#
# Nodes S_a (node 0 fixed), edges (i, j, Z, w) with the residual of E = Z^-1 o S_i o S_j^-1:
#   r = sqrt(w) (sigma_E - 1, 2 sign(qw_E) vec(q_E), t_E / ell),  q_E = (q_Zinv (x) q_i) (x) conj(q_j).
# Jacobians in the local steps (ds, dr, dt) of S_i and S_j are analytic (edge_terms); the fixed node's are 0.
# Orders: an edge's cost is r0 r0 + r1 r1 + ... in component order; sums over edges and dot products over the
# 7 n unknowns (index 7 a + row) are lane_tree_sum(., 1024); a node's block H_aa and gradient g_a = -J^T r add
# the contributions of its incident (edge, side) entries in ascending edge order, each contribution summed over
# the residual's components in order; A p = Hd_aa p_a + sum over the same entries of J_a^T (J_b p_b) with
# Hd = H + lambda diag(H).  The preconditioner is the Cholesky factor of every Hd_aa.
# PCG: x = 0, r = g, z = M^-1 r, p = z, rz0 = rz = r.z; stop at once unless rz0 > 0; per iteration
#   pAp = p.Ap (stop unless > 0), alpha = rz / pAp, x += alpha p, r -= alpha Ap, z = M^-1 r, rzn = r.z,
#   stop if rzn <= pcg_tol rz0, else beta = rzn / rz, p = z + beta p.
# LM: lambda = lambda0; while iterations < max_lm and cost > 0: solve, S_try = step(S, x) (node 0 kept),
#   cost_try < cost: accept, lambda /= 10, stop if (cost - cost_try) / cost < cost_tol; else lambda *= 10.

PGO_LANES = 1024


def _cols8(S):
    S = np.asarray(S, np.float64).reshape(-1, 8)
    return tuple(S[:, k].copy() for k in range(8))


def inverse_all(Z):
    return np.stack([np.asarray(v, np.float64) * np.ones(len(Z)) for v in inverse(_cols8(Z))], axis=1)


def edge_terms(Si, Sj, A, sw, ell, fix_i, fix_j):
    """r (E, 7), J (E, 2, 7, 7) of edges given as column tuples (8 arrays each)"""
    E = len(Si[0])
    zero = np.zeros(E)
    qjc = (Sj[1], -Sj[2], -Sj[3], -Sj[4])
    Ri, Rjc, Rz = quat_matrix(Si[1:5]), quat_matrix(qjc), quat_matrix(A[1:5])
    u = mat_vec(Rjc, Sj[5:8])
    v = mat_vec(Ri, u)
    sM = Si[0] / Sj[0]
    tM = tuple(Si[5 + k] - sM * v[k] for k in range(3))
    P = quat_mul(A[1:5], Si[1:5])
    qE = quat_mul(P, qjc)
    sE = A[0] * sM
    y = mat_vec(Rz, tM)
    tE = tuple(A[0] * y[k] + A[5 + k] for k in range(3))
    sgn = np.where(qE[0] >= 0.0, 1.0, -1.0)
    r = [sw * (sE - 1.0)] + [sw * ((2.0 * sgn) * qE[1 + k]) for k in range(3)] + [sw * (tE[k] / ell) for k in range(3)]
    Ji = [[zero] * 7 for _ in range(7)]
    Jj = [[zero] * 7 for _ in range(7)]
    c = (sw * A[0]) / ell
    j00 = sw * sE
    w0 = mat_vec(Rz, v)
    Ji[0][0], Jj[0][0] = j00, -j00
    for m in range(3):
        a = sM * (c * w0[m])
        Ji[4 + m][0], Jj[4 + m][0] = -a, a
    for k in range(3):
        ek = (0.0, 1.0 if k == 0 else 0.0, 1.0 if k == 1 else 0.0, 1.0 if k == 2 else 0.0)
        g = quat_mul(quat_mul(P, ek), qjc)
        cr = ((zero, -u[2], u[1]), (u[2], zero, -u[0]), (-u[1], u[0], zero))[k]
        w1 = mat_vec(Rz, mat_vec(Ri, cr))
        w3 = mat_vec(Rz, mat_vec(Ri, (Rjc[k], Rjc[3 + k], Rjc[6 + k])))
        for m in range(3):
            gq = sw * (sgn * g[1 + m])
            a = sM * (c * w1[m])
            Ji[1 + m][1 + k], Jj[1 + m][1 + k] = gq, -gq
            Ji[4 + m][1 + k], Jj[4 + m][1 + k] = -a, a
            Ji[4 + m][4 + k] = c * Rz[m * 3 + k]
            Jj[4 + m][4 + k] = -(sM * (c * w3[m]))
    J = np.zeros((E, 2, 7, 7))
    for a in range(7):
        for b in range(7):
            J[:, 0, a, b] = np.where(fix_i, 0.0, Ji[a][b])
            J[:, 1, a, b] = np.where(fix_j, 0.0, Jj[a][b])
    return np.stack(r, axis=1), J


class Graph:
    def __init__(self, n, edges, meas, weight, ell):
        self.n, self.ell = n, float(ell)
        self.edges = np.asarray(edges, np.int64).reshape(-1, 2)
        self.E = len(self.edges)
        self.zinv = _cols8(inverse_all(meas))
        self.sw = np.sqrt(np.asarray(weight, np.float64))
        lists = [[] for _ in range(n)]
        for e, (i, j) in enumerate(self.edges):
            lists[i].append(2 * e)
            lists[j].append(2 * e + 1)
        self.deg = max(len(x) for x in lists)
        self.ent = np.full((n, self.deg), -1, np.int64)
        for a, x in enumerate(lists):
            self.ent[a, :len(x)] = x

    def linearize(self, S):
        S = np.asarray(S, np.float64)
        i, j = self.edges[:, 0], self.edges[:, 1]
        r, J = edge_terms(_cols8(S[i]), _cols8(S[j]), self.zinv, self.sw, self.ell, i == 0, j == 0)
        c = r[:, 0] * r[:, 0]
        for k in range(1, 7):
            c = c + r[:, k] * r[:, k]
        return r, J, lane_tree_sum(c, PGO_LANES)

    def scatter(self, init, contrib, sign):
        """init[a] (+ or -) contrib[entry] over every node's entries in list order"""
        out = init
        flat = contrib.reshape((2 * self.E,) + contrib.shape[2:])
        for d in range(self.deg):
            has = self.ent[:, d] >= 0
            add = flat[self.ent[has, d]]
            out[has] = out[has] + add if sign > 0 else out[has] - add
        return out

    def assemble(self, r, J):
        B = J[:, :, 0, :, None] * J[:, :, 0, None, :]
        gb = J[:, :, 0, :] * r[:, None, 0, None]
        for k in range(1, 7):
            B = B + J[:, :, k, :, None] * J[:, :, k, None, :]
            gb = gb + J[:, :, k, :] * r[:, None, k, None]
        H = self.scatter(np.zeros((self.n, 7, 7)), B, +1)
        g = self.scatter(np.zeros((self.n, 7)), gb, -1)
        return H, g

    def damp(self, H, lam):
        n = self.n
        Hd = H.copy()
        for i in range(7):
            Hd[:, i, i] = H[:, i, i] + lam * H[:, i, i]
        Lm = np.zeros((n, 7, 7))
        ok = np.ones(n, bool)
        ok[0] = False
        with np.errstate(all="ignore"):
            for j in range(7):
                d = Hd[:, j, j].copy()
                for k in range(j):
                    d = d - Lm[:, j, k] * Lm[:, j, k]
                ok &= (d > 0.0) & (d < 1e300)
                Lm[:, j, j] = np.sqrt(d)
                for i in range(j + 1, 7):
                    v = Hd[:, i, j].copy()
                    for k in range(j):
                        v = v - Lm[:, i, k] * Lm[:, j, k]
                    Lm[:, i, j] = v / Lm[:, j, j]
        Hd[~ok] = np.eye(7)
        Lm[~ok] = np.eye(7)
        return Hd, Lm

    @staticmethod
    def block_solve(Lm, r):
        n = len(r)
        y, z = np.zeros((n, 7)), np.zeros((n, 7))
        for i in range(7):
            v = r[:, i].copy()
            for k in range(i):
                v = v - Lm[:, i, k] * y[:, k]
            y[:, i] = v / Lm[:, i, i]
        for i in range(6, -1, -1):
            v = y[:, i].copy()
            for k in range(i + 1, 7):
                v = v - Lm[:, k, i] * z[:, k]
            z[:, i] = v / Lm[:, i, i]
        return z

    def apply_A(self, J, Hd, p):
        pn = p[self.edges]                                  # (E, 2, 7)
        u = J[:, :, :, 0] * pn[:, :, None, 0]
        for c in range(1, 7):
            u = u + J[:, :, :, c] * pn[:, :, None, c]
        uo = u[:, ::-1, :]                                  # the other end's J p
        t = J[:, :, 0, :] * uo[:, :, 0, None]
        y = Hd[:, :, 0] * p[:, None, 0]
        for k in range(1, 7):
            t = t + J[:, :, k, :] * uo[:, :, k, None]
            y = y + Hd[:, :, k] * p[:, None, k]
        return self.scatter(y, t, +1)


def dot(a, b):
    return lane_tree_sum((a * b).reshape(-1), PGO_LANES)


def pcg(G, J, Hd, Lm, g, max_pcg, pcg_tol):
    x = np.zeros_like(g)
    r = g.copy()
    z = G.block_solve(Lm, r)
    p = z.copy()
    rz = dot(r, z)
    rz0 = rz
    it = 0
    done = not (rz0 > 0.0)
    while it < max_pcg and not done:
        Ap = G.apply_A(J, Hd, p)
        pAp = dot(p, Ap)
        if not (pAp > 0.0):
            break
        alpha = rz / pAp
        x = x + alpha * p
        r = r - alpha * Ap
        z = G.block_solve(Lm, r)
        rzn = dot(r, z)
        it += 1
        if rzn <= pcg_tol * rz0:
            done = True
        else:
            p = z + (rzn / rz) * p
        rz = rzn
    return x, it


def step_all(S, x):
    out = np.array(S, np.float64)
    for a in range(1, len(out)):
        out[a] = step(tuple(float(v) for v in S[a]), [float(v) for v in x[a]])
    return out


def pgo_sim3(nodes, edges, meas, weight, ell, lambda0=1e-4, max_lm=10, max_pcg=200, pcg_tol=1e-12, cost_tol=1e-9,
             trace=None):
    """(nodes, (cost0, cost), (lm iterations, accepted steps, pcg iterations)); trace: a list that
    receives (lambda, cost_try, accepted) per LM iteration"""
    S = np.array(nodes, np.float64).reshape(-1, 8)
    G = Graph(len(S), edges, meas, weight, ell)
    r, J, c = G.linearize(S)
    c0, lam, lm, acc, total = c, float(lambda0), 0, 0, 0
    while lm < max_lm and c > 0.0:
        H, g = G.assemble(r, J)
        Hd, Lm = G.damp(H, lam)
        x, it = pcg(G, J, Hd, Lm, g, max_pcg, pcg_tol)
        total += it
        St = step_all(S, x)
        rt, Jt, ct = G.linearize(St)
        lm += 1
        ok = ct < c
        if trace is not None:
            trace.append((lam, ct, ok))
        if ok:
            rel = (c - ct) / c
            S, r, J, c = St, rt, Jt, ct
            acc += 1
            lam = lam / 10.0
            if rel < cost_tol:
                break
        else:
            lam = lam * 10.0
    return S, (c0, c), (lm, acc, total)


def residual(Si, Sj, Z, w, ell):
    """the 7 residuals of one edge (scalars)"""
    one = lambda S: tuple(np.array([float(v)]) for v in S)
    r, _ = edge_terms(one(Si), one(Sj), one(inverse(tuple(float(v) for v in Z))), np.array([math.sqrt(w)]), ell,
                      np.array([False]), np.array([False]))
    return r[0]


def relative(Si, Sj):
    """the measurement that makes the edge (i, j) consistent: S_i o S_j^-1"""
    return compose(tuple(float(v) for v in Si), inverse(tuple(float(v) for v in Sj)))


def loop_measurement(Si, Sj, Sab):
    """the measurement of a loop edge (i, j) from the similarity b = Sab(a) between the two copies of
    the map (a in the copy node i lives in, b in node j's): the corrected S_i is S_i o Sab^-1, so
    Z = S_i o Sab^-1 o S_j^-1"""
    return compose(compose(tuple(float(v) for v in Si), inverse(tuple(float(v) for v in Sab))),
                   inverse(tuple(float(v) for v in Sj)))


# ---- the shared cases -----------------------------------------------------------------------------

def quat_of_axis_angle(axis, angle):
    """test data only (sin / cos never enter the library)"""
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    return quat_normalise((math.cos(angle / 2),) + tuple(math.sin(angle / 2) * ax))


def random_sim(rng, scale_range=(0.6, 1.6)):
    q = quat_of_axis_angle(rng.normal(size=3), rng.uniform(-2.5, 2.5))
    return (float(rng.uniform(*scale_range)),) + q + tuple(float(v) for v in rng.uniform(-2, 2, 3))


def pairs_case(seed, n, outlier_frac=0.0, noise=1e-3):
    """n pairs b = S a (+ noise), some replaced by outliers: (a, b, centres (6), S)"""
    rng = np.random.default_rng(seed)
    S = random_sim(rng)
    a = rng.uniform(-3, 3, (n, 3)) + np.array([0.0, 0.0, 8.0])
    b = np.stack(apply(S, _cols(a)), axis=1) + noise * rng.normal(size=(n, 3))
    bad = rng.permutation(n)[:int(round(outlier_frac * n))]
    b[bad] = rng.uniform(-20, 20, (len(bad), 3))
    ci = np.zeros(3)
    cj = np.array(apply(S, (0.0, 0.0, 0.0)))
    return a, b, np.concatenate([ci, cj]), S


PAIR_COUNTS = [3, 4, 63, 64, 65, 257]
HYP_COUNTS = [1, 64, 65]
TAU = 0.01
SEED = 0x5eed1234


def batch_case(counts, seed=7, outlier_frac=0.25):
    """several loops in one call: (a, b, offsets int32, centres L x 6)"""
    A, B, C, off = [], [], [], [0]
    for i, n in enumerate(counts):
        a, b, c, _ = pairs_case(seed * 100 + i, n, outlier_frac if n >= 8 else 0.0)
        A.append(a)
        B.append(b)
        C.append(c)
        off.append(off[-1] + n)
    return (np.concatenate(A).reshape(-1, 3), np.concatenate(B).reshape(-1, 3), np.array(off, np.int32),
            np.array(C).reshape(-1, 6))


def exact_case(n=12):
    """noise-free pairs of sigma = 2, a half turn about x (R = diag(1, -1, -1)) and an integer t on
    integer points: every product and sum of b = S a is exact"""
    rng = np.random.default_rng(5)
    S = (2.0, 0.0, 1.0, 0.0, 0.0, 3.0, -1.0, 4.0)
    a = rng.integers(-8, 9, (n, 3)).astype(np.float64) + np.array([0.0, 0.0, 20.0])
    b = np.stack(apply(S, _cols(a)), axis=1)
    return a, b, np.concatenate([np.zeros(3), np.array(apply(S, (0.0, 0.0, 0.0)))]), S


def collinear_case(n=9):
    """every a on one line: no sample gives a frame"""
    a = np.outer(np.arange(n, dtype=np.float64), [1.0, 2.0, -1.0]) + np.array([0.5, 0.0, 6.0])
    rng = np.random.default_rng(6)
    b = rng.uniform(-3, 3, (n, 3))
    return a, b, np.zeros(6)


def duplicate_case(n=40):
    """each of n / 2 pairs twice (a sample may pick a point and its copy: a degenerate triangle)"""
    a, b, c, S = pairs_case(77, n // 2)
    return np.concatenate([a, a]), np.concatenate([b, b]), c, S


def ransac_cases():
    """name -> (a, b, offsets, centres, H): the single-loop grid, the batches and the special cases"""
    out = {}
    for n in PAIR_COUNTS:
        for H in HYP_COUNTS:
            a, b, c, _ = pairs_case(n, n, 0.5 if n >= 63 else 0.0)
            out[f"n{n}_h{H}"] = (a, b, np.array([0, n], np.int32), c.reshape(1, 6), H)
    a, b, off, c = batch_case([65, 0, 257])
    out["batch3_empty"] = (a, b, off, c, 65)
    a, b, off, c = batch_case([4, 2, 64])
    out["batch3_two"] = (a, b, off, c, 64)
    # two hypotheses from different triangles that both hold all 4 pairs: the lower one wins, so H = 2 gives
    # what H = 1 gives
    a, b, c, _ = pairs_case(4, 4)
    out["tie_h1"] = (a, b, np.array([0, 4], np.int32), c.reshape(1, 6), 1)
    out["tie_h2"] = (a, b, np.array([0, 4], np.int32), c.reshape(1, 6), 2)
    a, b, c, _ = exact_case()
    out["exact"] = (a, b, np.array([0, len(a)], np.int32), c.reshape(1, 6), 16)
    a, b, c = collinear_case()
    out["collinear"] = (a, b, np.array([0, len(a)], np.int32), c.reshape(1, 6), 64)
    a, b, c, _ = duplicate_case()
    out["duplicates"] = (a, b, np.array([0, len(a)], np.int32), c.reshape(1, 6), 64)
    a = np.tile(np.array([[1.0, 2.0, 3.0]]), (6, 1))
    out["one_point"] = (a, a + 1.0, np.array([0, 6], np.int32), np.zeros((1, 6)), 8)
    return out


_REF_CACHE = {}


def ransac_expected(name):
    """the reference's outputs of a case, computed once per process"""
    if name not in _REF_CACHE:
        a, b, off, c, H = ransac_cases()[name]
        _REF_CACHE[name] = sim3_ransac(a, b, off, c, H, TAU, SEED)
    return _REF_CACHE[name]


RANSAC_NAMES = list(ransac_cases())

APPLY_COUNTS = [0, 1, 64, 65]


def apply_case(n, m=5, seed=3):
    """(points, anchor, nodes, nodes_new): anchors run over the first node, the last node and none"""
    rng = np.random.default_rng(seed + n)
    nodes = np.array([random_sim(rng, (1.0, 1.0)) for _ in range(m)])
    new = np.array([random_sim(rng, (0.7, 1.4)) for _ in range(m)])
    new[2] = nodes[2]                    # an unchanged node
    pts = rng.uniform(-5, 5, (n, 3))
    anchor = np.array([(0, m - 1, -1, 2, 1)[i % 5] for i in range(n)], np.int32)
    return pts, anchor, nodes, new


# ---- pose-graph cases -----------------------------------------------------------------------------

def centres_of(S):
    """camera centres -R^T t / sigma of nodes x_c = sigma R x_w + t"""
    return np.array([apply(inverse(tuple(float(v) for v in s)), (0.0, 0.0, 0.0)) for s in np.asarray(S).reshape(-1, 8)])


def ring_case(n, seed=1, drift=0.01, rot=0.002, trans=0.002, radius=5.0):
    """n cameras on a ring looking along the tangent; odometry with a scale drift of `drift` per step and
    small rotation / translation noise chained from node 0; one loop edge (n - 1, 0) with the true relative
    pose: (drifted nodes, edges, measurements, weights, ell, ground truth)"""
    rng = np.random.default_rng(seed)
    gt = []
    for k in range(n):
        ang = 2.0 * math.pi * k / n
        q = quat_of_axis_angle([0.0, 0.0, 1.0], ang)
        c = (radius * math.cos(ang), radius * math.sin(ang), 0.0)
        y = mat_vec(quat_matrix(q), c)
        gt.append((1.0,) + q + (-y[0], -y[1], -y[2]))
    est = [gt[0]]
    for k in range(1, n):
        noise = (1.0 + drift,) + quat_of_axis_angle(rng.normal(size=3), rot * rng.normal()) + tuple(trans * rng.normal(size=3))
        z = compose(relative(gt[k - 1], gt[k]), noise)
        Sk = compose(inverse(z), est[k - 1])
        est.append((Sk[0],) + quat_normalise(Sk[1:5]) + Sk[5:8])
    est = np.array(est)
    edges = [(k - 1, k) for k in range(1, n)] + [(n - 1, 0)]
    meas = [relative(est[k - 1], est[k]) for k in range(1, n)] + [relative(gt[n - 1], gt[0])]
    cen = centres_of(est)
    ell = float(np.mean(np.linalg.norm(cen[1:] - cen[:-1], axis=1)))
    return est, np.array(edges, np.int32), np.array(meas), np.ones(n), ell, np.array(gt)


def pgo_cases():
    """name -> (nodes, edges, meas, weight, ell, kwargs)"""
    out = {}
    # two nodes, one edge that the nodes satisfy exactly (identity rotations, integers): cost 0
    S = np.array([IDENTITY, (1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 2.0, 3.0)])
    out["two_consistent"] = (S, np.array([[0, 1]], np.int32), np.array([relative(S[0], S[1])]), np.ones(1), 1.0, {})
    est, e, m, w, ell, _ = ring_case(3, seed=3, drift=0.05, rot=0.02, trans=0.05)
    out["three"] = (est, e, m, w, ell, dict(max_lm=6, max_pcg=30))
    for n in (65, 257):
        est, e, m, w, ell, _ = ring_case(n, seed=n)
        out[f"ring{n}"] = (est, e, m, w * np.where(np.arange(len(e)) == len(e) - 1, 4.0, 1.0), ell, dict(max_lm=3, max_pcg=40))
    # a star: node 1 is the hub of 70 edges (more than one wave's worth of an incident list), either side
    rng = np.random.default_rng(70)
    S = np.array([IDENTITY] + [random_sim(rng, (0.8, 1.25)) for _ in range(70)])
    e = np.array([(1, a) if a % 2 else (a, 1) for a in [0] + list(range(2, 71))], np.int32)
    m = np.array([compose(relative(S[i], S[j]), (1.02,) + quat_of_axis_angle(rng.normal(size=3), 0.03) + tuple(0.03 * rng.normal(size=3)))
                  for i, j in e])
    out["star70"] = (S, e, m, rng.uniform(0.5, 2.0, len(e)), 1.0, dict(max_lm=4, max_pcg=60))
    # two loop edges between the same nodes that disagree a little
    est, e, m, w, ell, gt = ring_case(12, seed=12, drift=0.03)
    z2 = compose(m[-1], (1.01,) + quat_of_axis_angle([1.0, 0.0, 0.0], 0.01) + (0.01, -0.02, 0.0))
    out["double_loop"] = (est, np.concatenate([e, [[11, 0]]]).astype(np.int32), np.concatenate([m, [z2]]), np.append(w, 0.5), ell,
                          dict(max_lm=5, max_pcg=60))
    # a step that must be rejected: a badly wrong start and almost no damping, so the first Gauss-Newton
    # step overshoots, the cost rises, the nodes are restored and lambda grows
    est, e, m, w, ell, gt = ring_case(8, seed=8, drift=0.02)
    bad = est.copy()
    rng = np.random.default_rng(88)
    for a in range(1, 8):
        bad[a] = step(tuple(est[a]), [0.5 * rng.normal()] + list(1.2 * rng.normal(size=3)) + list(3.0 * rng.normal(size=3)))
        bad[a, 0] = abs(bad[a, 0]) + 0.2
    out["reject"] = (bad, e, m, w, ell, dict(lambda0=1e-9, max_lm=8, max_pcg=60))
    return out


_PGO_CACHE = {}


def pgo_expected(name):
    """(nodes, costs, iteration counts, trace) of the reference, computed once per process"""
    if name not in _PGO_CACHE:
        S, e, m, w, ell, kw = pgo_cases()[name]
        tr = []
        _PGO_CACHE[name] = pgo_sim3(S, e, m, w, ell, trace=tr, **kw) + (tr,)
    return _PGO_CACHE[name]


PGO_NAMES = list(pgo_cases())


# ---- a synthetic world for the end-to-end test ------------------------------------------------------

def world_case(n=40, seed=4, drift=0.01, per_wall=220, wrong=False):
    """Points on the walls of a box, n cameras on a ring looking outward.  The estimated poses carry the
    ring_case drift; a point is born in the map of the first camera of a visit (X_est = S_k^-1 (gt_k (X)), the
    pose being the rigid (R, t / sigma) that sees the same rays), so a point seen again after the gap at the
    ring's seam exists twice.  Returns a dict: rotations, motions, points, colors, obs (per camera: xy f32,
    point index), loops [(39, 0, xy_i, xy_j), (38, 0, ...)], gt_centres, dup (pairs of indices of one world
    point).  wrong: the loop (39, 0) alone, its matches paired at random."""
    rng = np.random.default_rng(seed)
    est, _, _, _, _, gt = ring_case(n, seed=seed, drift=drift, radius=2.0)
    # ring_case's cameras look along +z of a frame rotated about z: turn them to look outward (x_c z-axis radial)
    look = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]).T      # camera z = world x (radial at angle 0)
    walls = []
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            p = rng.uniform(-6, 6, (per_wall, 3))
            p[:, ax] = sgn * (6.0 if ax < 2 else 3.0)
            if ax == 2:
                p[:, :2] = rng.uniform(-6, 6, (per_wall, 2))
            else:
                p[:, 2] = rng.uniform(-3, 3, per_wall)
            walls.append(p)
    world = np.concatenate(walls)
    f, w, h = 300.0, 640, 480
    gtS, estS = [], []
    for k in range(n):
        for src, dst in ((gt, gtS), (est, estS)):
            Rk = look.T @ np.array(quat_matrix(tuple(src[k, 1:5]))).reshape(3, 3)
            tk = look.T @ src[k, 5:8]
            dst.append((src[k, 0], Rk, tk))
    seen = np.zeros((n, len(world)), bool)
    pix = np.zeros((n, len(world), 2), np.float32)
    for k in range(n):
        _, Rk, tk = gtS[k]
        xc = world @ Rk.T + tk
        z = np.where(xc[:, 2] > 0.5, xc[:, 2], 1.0)
        u, v = f * xc[:, 0] / z + w / 2, f * xc[:, 1] / z + h / 2
        seen[k] = (xc[:, 2] > 0.5) & (u >= 0) & (u < w) & (v >= 0) & (v < h)
        pix[k] = np.stack([u, v], 1).astype(np.float32)
    points, colors, dup = [], [], []
    obs_idx = np.full((n, len(world)), -1, np.int64)
    for p in np.flatnonzero(seen.any(0)):
        ks = np.flatnonzero(seen[:, p])
        visits, cur = [], [ks[0]]
        for k in ks[1:]:
            if k == cur[-1] + 1:
                cur.append(k)
            else:
                visits.append(cur)
                cur = [k]
        visits.append(cur)
        ids = []
        for vis in visits:
            s, Rk, tk = estS[vis[0]]
            _, Rg, tg = gtS[vis[0]]
            xc = Rg @ world[p] + tg
            points.append(Rk.T @ (xc - tk) / s)
            colors.append(rng.integers(0, 256, 3))
            ids.append(len(points) - 1)
            obs_idx[vis, p] = ids[-1]
        if len(ids) == 2:
            dup.append(ids)
    obs = [(pix[k, seen[k]], obs_idx[k, seen[k]]) for k in range(n)]
    loops = []
    for i, j in ((n - 1, 0), (n - 2, 0)):
        both = np.flatnonzero(seen[i] & seen[j])
        xi, xj = pix[i, both], pix[j, both]
        if wrong:
            xj = xj[rng.permutation(len(xj))]
        loops.append((i, j, xi, xj))
        if wrong:
            break
    return {"rotations": np.array([Rk for _, Rk, _ in estS]), "motions": np.array([tk / s for s, _, tk in estS]),
            "points": np.array(points), "colors": np.array(colors, np.uint8), "obs": obs, "loops": loops,
            "gt_centres": np.array([-Rk.T @ tk for _, Rk, tk in gtS]), "dup": np.array(dup, np.int64)}

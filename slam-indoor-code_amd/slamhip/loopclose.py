"""Loop closing: the Sim(3) constraint of each verified loop, pose-graph optimisation over
Sim(3) and the correction of the map (csrc/loop.hip; the contract is tests/loop_ref.py).

Only + - * / and sqrt in f64 in a stated order, so the device (ctx), the host twins
(host=True) and the reference agree bit for bit.  A similarity is 8 doubles
(sigma, qw, qx, qy, qz, tx, ty, tz): x' = sigma R(q) x + t.  Host arrays in give host
arrays out; torch device tensors (float64 points, int32 anchors) give device tensors.

    sim, mask, count, status = sim3_from_pairs(a, b, offsets, centres, hypotheses=256, tau=0.01)
    nodes, costs, iters = optimize_pose_graph(nodes, edges, meas, weight, ell)
    moved = apply_points(points, anchor, nodes, nodes_new)
    closed = close_loops(rotations, motions, points, colors, obs, loops)      # constraints -> graph -> map
    points, colors, dropped = correct_map(points, colors, obs, nodes, nodes_new, constraints)
    closed = close_run(gd, logs, K, cond, ops, LoopParams(close=True))        # what slam_main(loops=...) calls
"""
import ctypes

import numpy as np

from . import _lib as L
from ._lib import check, lib, ptr

OK, NO_MODEL, TOO_FEW, CHOLESKY = L.SIM3_OK, L.SIM3_NO_MODEL, L.SIM3_TOO_FEW, L.SIM3_CHOLESKY


def _is_dev(a):
    return not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def _dp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _handle(ctx):
    from .api import default_context
    return (ctx or default_context()).handle


def _sync():
    import torch
    torch.cuda.synchronize()      # the library runs on its own stream: torch's writes must have landed


def _f64(a, cols):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, cols))


def sim3_from_pairs(a, b, offsets, centres, hypotheses=256, tau=0.01, seed=0, ctx=None, host=False):
    """The similarity b ~ s R a + t of each of L loops by RANSAC (slam_sim3_ransac): loop l owns
    the pairs offsets[l] .. offsets[l + 1]; centres (L x 6) holds the centre of the camera that
    saw a, then of the one that saw b.  Returns (sim (L, 8) f64, mask uint8 per pair, count
    int32[L], status int32[L]: OK, NO_MODEL, TOO_FEW or CHOLESKY)."""
    off = np.ascontiguousarray(np.asarray(offsets, np.int32).reshape(-1))
    if len(off) < 1:
        raise ValueError("offsets holds L + 1 values")
    nl, H = len(off) - 1, int(hypotheses)
    cen = _f64(centres, 6)
    if len(cen) != nl:
        raise ValueError("centres is L x 6")
    if _is_dev(a) != _is_dev(b):
        raise TypeError("a and b: both host arrays or both device tensors")
    if _is_dev(a):
        import torch
        if a.dtype != torch.float64 or b.dtype != torch.float64 or a.shape != b.shape:
            raise TypeError("device pairs are float64 tensors of one shape")
        a, b = a.reshape(-1, 3).contiguous(), b.reshape(-1, 3).contiguous()
        n = a.shape[0]
        if nl and (off[0] < 0 or int(off.max()) > n):
            raise ValueError("offsets outside the pairs")
        sim = torch.empty((nl, 8), dtype=torch.float64, device=a.device)
        mask = torch.zeros(n, dtype=torch.uint8, device=a.device)
        count = torch.empty(nl, dtype=torch.int32, device=a.device)
        status = torch.empty(nl, dtype=torch.int32, device=a.device)
        _sync()
        h = _handle(ctx)
        check(lib().slam_sim3_ransac_dev(h, None, _dp(a), _dp(b), ptr(off), nl, ptr(cen), H, float(tau), int(seed),
                                         _dp(sim), _dp(mask), _dp(count), _dp(status)), h)
        return sim, mask, count, status
    a, b = _f64(a, 3), _f64(b, 3)
    if a.shape != b.shape:
        raise ValueError("a and b hold the same number of points")
    if nl and (off[0] < 0 or int(off.max()) > len(a)):
        raise ValueError("offsets outside the pairs")
    sim = np.zeros((nl, 8), np.float64)
    mask = np.zeros(len(a), np.uint8)
    count, status = np.zeros(nl, np.int32), np.zeros(nl, np.int32)
    if host:
        check(lib().slam_sim3_ransac_host(ptr(a), ptr(b), ptr(off), nl, ptr(cen), H, float(tau), int(seed), ptr(sim),
                                          ptr(mask), ptr(count), ptr(status)))
    else:
        h = _handle(ctx)
        check(lib().slam_sim3_ransac(h, ptr(a), ptr(b), ptr(off), nl, ptr(cen), H, float(tau), int(seed), ptr(sim),
                                     ptr(mask), ptr(count), ptr(status)), h)
    return sim, mask, count, status


def apply_points(points, anchor, nodes, nodes_new, ctx=None, host=False):
    """X' = S'^-1 (S (X)) for every map point with S = nodes[anchor], S' = nodes_new[anchor]
    (slam_sim3_apply_points); anchor -1 keeps the point, and so does an unchanged node."""
    nd, nn = _f64(nodes, 8), _f64(nodes_new, 8)
    if nd.shape != nn.shape:
        raise ValueError("nodes and nodes_new are m x 8")
    m = len(nd)
    if _is_dev(points):
        import torch
        if points.dtype != torch.float64 or not _is_dev(anchor) or anchor.dtype != torch.int32:
            raise TypeError("device points are float64 with int32 device anchors")
        p, an = points.reshape(-1, 3).contiguous(), anchor.reshape(-1).contiguous()
        if an.shape[0] != p.shape[0]:
            raise ValueError("one anchor per point")
        out = torch.empty_like(p)
        _sync()
        h = _handle(ctx)
        check(lib().slam_sim3_apply_points_dev(h, None, _dp(p), _dp(an), p.shape[0], ptr(nd), ptr(nn), m, _dp(out)), h)
        return out
    p = _f64(points, 3)
    an = np.ascontiguousarray(np.asarray(anchor, np.int32).reshape(-1))
    if len(an) != len(p):
        raise ValueError("one anchor per point")
    out = np.empty_like(p)
    if host:
        check(lib().slam_sim3_apply_points_host(ptr(p), ptr(an), len(p), ptr(nd), ptr(nn), m, ptr(out)))
    else:
        h = _handle(ctx)
        check(lib().slam_sim3_apply_points(h, ptr(p), ptr(an), len(p), ptr(nd), ptr(nn), m, ptr(out)), h)
    return out


def optimize_pose_graph(nodes, edges, meas, weight, ell, lambda0=1e-4, max_lm=10, max_pcg=200, pcg_tol=1e-12,
                        cost_tol=1e-9, ctx=None, host=False):
    """Pose-graph optimisation over Sim(3) (slam_pgo_sim3): nodes (n, 8), node 0 fixed; edge e joins
    edges[e] = (i, j) with the measurement meas[e] ~ S_i o S_j^-1 and weight[e]; ell scales the
    translation residual (the mean consecutive baseline).  Returns (nodes, (initial cost, final
    cost), (LM steps, accepted steps, PCG iterations)); device nodes in give device nodes out."""
    ed = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 2))
    ms = _f64(meas, 8)
    wt = np.ascontiguousarray(np.asarray(weight, np.float64).reshape(-1))
    if len(ms) != len(ed) or len(wt) != len(ed):
        raise ValueError("one measurement and one weight per edge")
    cost = np.zeros(2, np.float64)
    iters = np.zeros(3, np.int32)
    args = (ptr(ed), ptr(ms), ptr(wt), len(ed), float(ell), float(lambda0), int(max_lm), int(max_pcg), float(pcg_tol),
            float(cost_tol), ptr(cost), ptr(iters))
    if _is_dev(nodes):
        import torch
        if nodes.dtype != torch.float64:
            raise TypeError("device nodes are float64")
        out = nodes.reshape(-1, 8).contiguous().clone()
        _sync()
        h = _handle(ctx)
        check(lib().slam_pgo_sim3_dev(h, None, _dp(out), out.shape[0], *args), h)
    else:
        out = _f64(nodes, 8).copy()
        if host:
            check(lib().slam_pgo_sim3_host(ptr(out), len(out), *args))
        else:
            h = _handle(ctx)
            check(lib().slam_pgo_sim3(h, ptr(out), len(out), *args), h)
    return out, (float(cost[0]), float(cost[1])), tuple(int(v) for v in iters)


# ---- from the run's poses, points and observations to the closed map ----------------------------------
# Host bookkeeping in plain f64 (it prepares the same inputs for the device and the host=True path, so the
# two still agree by bits); the heavy steps are the three library calls above.

def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def quat_matrix(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def matrix_quat(R):
    """unit quaternion (w, x, y, z) of a rotation matrix (Shepperd's branches; sqrt and division only)"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        r = np.sqrt(1 + tr)
        q = [0.5 * r, (R[2, 1] - R[1, 2]) * 0.5 / r, (R[0, 2] - R[2, 0]) * 0.5 / r, (R[1, 0] - R[0, 1]) * 0.5 / r]
    elif R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        r = np.sqrt(1 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) * 0.5 / r, 0.5 * r, (R[0, 1] + R[1, 0]) * 0.5 / r, (R[0, 2] + R[2, 0]) * 0.5 / r]
    elif R[1, 1] >= R[2, 2]:
        r = np.sqrt(1 + R[1, 1] - R[0, 0] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) * 0.5 / r, (R[0, 1] + R[1, 0]) * 0.5 / r, 0.5 * r, (R[1, 2] + R[2, 1]) * 0.5 / r]
    else:
        r = np.sqrt(1 + R[2, 2] - R[0, 0] - R[1, 1])
        q = [(R[1, 0] - R[0, 1]) * 0.5 / r, (R[0, 2] + R[2, 0]) * 0.5 / r, (R[1, 2] + R[2, 1]) * 0.5 / r, 0.5 * r]
    q = np.array(q)
    return q / np.sqrt(q @ q)


def sim_compose(A, B):
    """x -> A(B(x))"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    q = _qmul(A[1:5], B[1:5])
    return np.concatenate([[A[0] * B[0]], q / np.sqrt(q @ q), A[0] * (quat_matrix(A[1:5]) @ B[5:8]) + A[5:8]])


def sim_inverse(S):
    S = np.asarray(S, np.float64)
    qc = S[1:5] * np.array([1.0, -1.0, -1.0, -1.0])
    return np.concatenate([[1.0 / S[0]], qc, -(quat_matrix(qc) @ S[5:8]) / S[0]])


def nodes_from_poses(rotations, motions):
    """(n, 8) similarities (1, q(R), t) of the poses x_c = R x_w + t"""
    return np.array([np.concatenate([[1.0], matrix_quat(R), np.asarray(t, np.float64).reshape(3)])
                     for R, t in zip(rotations, motions)]).reshape(-1, 8)


def _table(obs_k):
    oxy, oid = obs_k
    return {(float(x), float(y)): int(p) for (x, y), p in zip(np.asarray(oxy, np.float32).reshape(-1, 2), oid)}


def _lookup(obs_k, xy, table=None):
    """point index of each pixel position of xy in one frame's observations (-1: none), by exact position"""
    if table is None:
        table = _table(obs_k)
    return np.array([table.get((float(x), float(y)), -1) for x, y in np.asarray(xy, np.float32).reshape(-1, 2)], np.int64)


def loop_constraints(nodes, points, obs, loops, hypotheses=256, tau=0.01, min_pairs=30, seed=0, ctx=None, host=False):
    """The Sim(3) constraint of every loop (i, j, xy_i, xy_j): xy_i / xy_j are the matched keypoint
    positions in the later frame i and the earlier frame j.  A match counts when both ends carry a map
    point in obs; the pairs (a from frame i's copy of the map, b from frame j's) go to sim3_from_pairs
    in one batch.  Returns a list of dicts (i, j, ia, ib, sim, mask, count, status, accepted); accepted:
    status OK, at least min_pairs pairs and at least min_pairs inliers."""
    nodes = _f64(nodes, 8)
    points = _f64(points, 3)
    out, A, B, off, cen = [], [], [], [0], []
    tables = {}                 # one position table per frame, however many loops end in it
    for i, j, xy_i, xy_j in loops:
        for k in (i, j):
            if k not in tables:
                tables[k] = _table(obs[k])
        ia, ib = _lookup(obs[i], xy_i, tables[i]), _lookup(obs[j], xy_j, tables[j])
        keep = (ia >= 0) & (ib >= 0) & (ia != ib)
        ia, ib = ia[keep], ib[keep]
        out.append({"i": int(i), "j": int(j), "ia": ia, "ib": ib})
        A.append(points[ia])
        B.append(points[ib])
        off.append(off[-1] + len(ia))
        ci = sim_inverse(nodes[i])[5:8]
        cj = sim_inverse(nodes[j])[5:8]
        cen.append(np.concatenate([ci, cj]))
    if not out:
        return out
    sim, mask, count, status = sim3_from_pairs(np.concatenate(A).reshape(-1, 3), np.concatenate(B).reshape(-1, 3), off,
                                               np.array(cen).reshape(-1, 6), hypotheses, tau, seed, ctx=ctx, host=host)
    for l, c in enumerate(out):
        c.update(sim=sim[l].copy(), mask=mask[off[l]:off[l + 1]].astype(bool), count=int(count[l]), status=int(status[l]))
        c["accepted"] = c["status"] == OK and len(c["ia"]) >= min_pairs and c["count"] >= min_pairs
    return out


def anchors_of(obs, npoints):
    """the first logged keyframe that observes each point (-1: none)"""
    anchor = np.full(npoints, -1, np.int32)
    for k in range(len(obs)):
        idx = np.asarray(obs[k][1], np.int64)
        idx = idx[(idx >= 0) & (idx < npoints)]
        idx = idx[anchor[idx] < 0]
        anchor[idx] = k
    return anchor


def merged_roots(npoints, constraints):
    """The representative of every point under the merges that the accepted loops' inlier pairs name (union-find,
    the lowest index of a set is its root): root[i] == i for a point that stays."""
    parent = np.arange(npoints)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for c in constraints:
        if c["accepted"]:
            for a, b in zip(c["ia"][c["mask"]], c["ib"][c["mask"]]):
                ra, rb = find(int(a)), find(int(b))
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(npoints)], np.int64)


def correct_map(points, colors, obs, nodes, nodes_new, constraints, ctx=None, host=False):
    """Moves every point with its anchor node (apply_points) and merges the duplicates that the accepted
    loops' inlier pairs name: of each set the lowest index stays (with its colour), the others are dropped.
    Returns (points, colors, dropped indices)."""
    points = _f64(points, 3)
    moved = apply_points(points, anchors_of(obs, len(points)), nodes, nodes_new, ctx=ctx, host=host)
    keep = merged_roots(len(points), constraints) == np.arange(len(points))
    colors = np.asarray(colors)
    return moved[keep], colors[keep] if len(colors) == len(points) else colors, np.flatnonzero(~keep)


def close_loops(rotations, motions, points, colors, obs, loops, hypotheses=256, tau=0.01, min_pairs=30, loop_weight=1.0,
                lambda0=1e-4, max_lm=10, max_pcg=400, pcg_tol=1e-10, cost_tol=1e-6, seed=0, ctx=None, host=False):
    """Closes the loops of a finished run: constraints (loop_constraints), the pose graph over the n logged
    keyframes with the run's own relative poses and the accepted loops (optimize_pose_graph), the map
    correction (correct_map).  A corrected camera is the rigid pose that sees the same rays: R(q), t / sigma.
    Returns a dict: rotations (n, 3, 3), motions (n, 3), points, colors, constraints, dropped, nodes, costs,
    iters.  With no accepted loop everything comes back as it went in."""
    rot = np.asarray(rotations, np.float64).reshape(-1, 3, 3)
    mot = np.asarray(motions, np.float64).reshape(-1, 3)
    pts = _f64(points, 3)
    n = len(rot)
    nodes = nodes_from_poses(rot, mot)
    cons = loop_constraints(nodes, pts, obs, loops, hypotheses, tau, min_pairs, seed, ctx=ctx, host=host)
    acc = [c for c in cons if c["accepted"]]
    res = {"rotations": rot.copy(), "motions": mot.copy(), "points": pts.copy(), "colors": np.asarray(colors).copy(),
           "constraints": cons, "dropped": np.zeros(0, np.int64), "nodes": nodes, "costs": (0.0, 0.0), "iters": (0, 0, 0)}
    if not acc or n < 2:
        return res
    edges = [(k - 1, k) for k in range(1, n)] + [(c["i"], c["j"]) for c in acc]
    meas = [sim_compose(nodes[k - 1], sim_inverse(nodes[k])) for k in range(1, n)]
    meas += [sim_compose(sim_compose(nodes[c["i"]], sim_inverse(c["sim"])), sim_inverse(nodes[c["j"]])) for c in acc]
    weight = [1.0] * (n - 1) + [float(loop_weight)] * len(acc)
    cen = np.array([sim_inverse(s)[5:8] for s in nodes])
    ell = float(np.mean(np.linalg.norm(cen[1:] - cen[:-1], axis=1)))
    new, costs, iters = optimize_pose_graph(nodes, edges, meas, weight, ell, lambda0, max_lm, max_pcg, pcg_tol, cost_tol,
                                            ctx=ctx, host=host)
    p2, c2, dropped = correct_map(pts, colors, obs, nodes, new, cons, ctx=ctx, host=host)
    res.update(rotations=np.array([quat_matrix(s[1:5]) for s in new]), motions=np.array([s[5:8] / s[0] for s in new]),
               points=p2, colors=c2, dropped=dropped, nodes=new, costs=costs, iters=iters)
    return res


# ---- through slam_main ------------------------------------------------------------------------------

def loop_matches(frames, loops, cond, ops):
    """The matched keypoint positions of every kept loop (i, j, ...), found the way verify_loop found them:
    frame i's fresh keypoints described, then the ratio-test match against frame j (ops.match_frame).
    Returns [(i, j, xy_i, xy_j)] with float32 n x 2 positions."""
    feats, out = {}, []
    for lp in loops:
        i, j = int(lp[0]), int(lp[1])
        for k in (i, j):
            if k not in feats:
                kps = ops.fast(frames[k], cond.featureExtractingThreshold)
                feats[k] = ops.describe(frames[k], kps, cond.matcherType)
        (ki, di), (kj, dj) = feats[i], feats[j]
        if len(di) == 0 or len(dj) == 0:
            out.append((i, j, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)))
            continue
        kj2, m = ops.match_frame(di, frames[j], kj, cond.matcherType, cond.knnMatcherDistance)
        q, t = m["queryIdx"].astype(np.int64), m["trainIdx"].astype(np.int64)
        out.append((i, j, np.stack([ki["x"][q], ki["y"][q]], 1).astype(np.float32).reshape(-1, 2),
                    np.stack([kj2["x"][t], kj2["y"][t]], 1).astype(np.float32).reshape(-1, 2)))
    return out


def close_run(gd, logs, K, cond, ops, prm, ctx=None, host=False):
    """close_loops on a finished slam_main run: the final poses and points of gd, the observations and good
    frames of logs, the loops of gd.loops with their matches (loop_matches).  Returns close_loops' dict; with
    no accepted loop its rotations, motions, points and colors are the run's open ones."""
    matches = loop_matches(logs.frames, gd.loops, cond, ops)
    res = close_loops(gd.cameraRotations, [np.reshape(t, 3) for t in gd.spatialCameraPositions], gd.spatialPoints,
                      gd.spatialPointsColors, logs.obs, matches, hypotheses=prm.hypotheses, tau=prm.tau,
                      min_pairs=prm.min_pairs, loop_weight=prm.loop_weight, max_lm=prm.max_lm, max_pcg=prm.max_pcg,
                      ctx=ctx, host=host)
    if not any(c["accepted"] for c in res["constraints"]):
        res["rotations"] = np.array(logs.rotation_list, np.float64).reshape(-1, 3, 3)
        res["motions"] = np.array(logs.pose_list, np.float64).reshape(-1, 3)
    return res

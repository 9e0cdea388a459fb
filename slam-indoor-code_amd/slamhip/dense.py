"""Dense points for the meshing stage: plane-sweep stereo over the good frames
(DESIGN.md section 22).  The library never forms a pose: this module turns the
cycle's poses into the matrices the kernels take, picks the depth planes from the
sparse cloud, runs slam_mvs_depth_batch_dev and slam_mvs_fuse_dev, and returns the
points.  The reference has no such stage; it is opt-in everywhere.

Pose convention (the one cycle.py logs and reconstruct() takes): a camera is
[R | t], x_cam = R X + t, and a pixel is K x_cam / z.
"""
import numpy as np

MAX_SOURCES = 4
FILTER_BORDER = 4


def _inv_K(K):
    """the closed-form inverse of an upper-triangular camera matrix (last row 0 0 1)"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    fx, s, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    return np.array([[1.0 / fx, -s / (fx * fy), (s * cy - cx * fy) / (fx * fy)],
                     [0.0, 1.0 / fy, -cy / fy],
                     [0.0, 0.0, 1.0]])


def sweep_matrices(K, R_ref, t_ref, R_src, t_src):
    """(M, v) of the motion reference -> source: with R = R_src R_ref^T and t =
    t_src - R t_ref, M = K R K^-1 (3 x 3) and v = K t (3): a reference pixel p at
    inverse depth w lands at M p + w v in the source.  tests/mvs_ref.py uses this
    same function, so both sides hand the kernels the same bits."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    Rr, Rs = np.asarray(R_ref, np.float64).reshape(3, 3), np.asarray(R_src, np.float64).reshape(3, 3)
    tr, ts = np.asarray(t_ref, np.float64).reshape(3), np.asarray(t_src, np.float64).reshape(3)
    R = Rs @ Rr.T
    t = ts - R @ tr
    return (K @ R) @ _inv_K(K), K @ t


def backproject_matrices(K, R, t):
    """(B, c): the point of pixel p at inverse depth w is c + (B p) / w, B = R^T K^-1, c = -R^T t"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    return R.T @ _inv_K(K), -(R.T @ np.asarray(t, np.float64).reshape(3))


def depth_planes(K, R, t, sparse_points, shape, D):
    """D inverse depths for a frame, uniform from 1 / (1.5 hi) to 1.5 / lo, where lo
    and hi are the 5 % and 95 % order statistics (z[n // 20], z[n - 1 - n // 20]) of
    the depths of the sparse points in front of the camera that project inside the
    (h, w) image.  None when fewer than 8 such points exist: the frame is skipped."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    X = np.asarray(sparse_points, np.float64).reshape(-1, 3)
    h, w = shape[0], shape[1]
    cam = X @ np.asarray(R, np.float64).reshape(3, 3).T + np.asarray(t, np.float64).reshape(1, 3)
    z = cam[:, 2]
    front = z > 0
    cam, z = cam[front], z[front]
    p = cam @ K.T
    with np.errstate(all="ignore"):
        u, v = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    inside = (u >= -0.5) & (u < w - 0.5) & (v >= -0.5) & (v < h - 0.5)
    z = np.sort(z[inside])
    n = len(z)
    if n < 8:
        return None
    lo, hi = z[n // 20], z[n - 1 - n // 20]
    w0, w1 = 1.0 / (1.5 * hi), 1.5 / lo
    t = np.arange(D, dtype=np.float64) / (D - 1)
    return w0 * (1.0 - t) + w1 * t          # both ends exact


class SgmParams:
    """Semi-global aggregation of the sweep's cost volume: the
    penalties p1 <= p2 (0..255, Hamming bits per window pixel and source) for a change
    of one plane and of more between neighbouring pixels, and 4 or 8 paths.  The
    defaults are the customary census penalties of GPU SGM libraries; they are not
    tuned on this project's data."""

    def __init__(self, p1=10, p2=120, paths=8):
        if not 0 <= p1 <= p2 <= 255 or paths not in (4, 8):
            raise ValueError("SgmParams: 0 <= p1 <= p2 <= 255, paths 4 or 8")
        self.p1, self.p2, self.paths = int(p1), int(p2), int(paths)


class DenseParams:
    """slam_main(dense=...) / densify: D planes per reference, `sources` nearest good
    frames per reference, the aggregation radius, the uniqueness ratio in percent,
    the least number of sources that must see the winner, and the fuse step's eps,
    min_consistent and grid step.  sgm (an SgmParams; None = winner-take-all, every
    byte as without it) aggregates the cost volume semi-globally before the winner."""

    def __init__(self, D=64, sources=2, radius=2, uniq=80, min_views=1, eps=0.01, min_consistent=1, step=4, sgm=None):
        if sgm is not None and not isinstance(sgm, SgmParams):
            raise ValueError("DenseParams: sgm is an SgmParams or None")
        self.sgm = sgm
        if not 4 <= D <= 256 or not 1 <= sources <= MAX_SOURCES or not 0 <= radius <= 3 or not 1 <= uniq <= 100 \
                or not 1 <= min_views <= sources or not eps >= 0 or not 0 <= min_consistent <= MAX_SOURCES or step < 1:
            raise ValueError("DenseParams: D 4..256, sources 1..4, radius 0..3, uniq 1..100, min_views 1..sources, "
                             "eps >= 0, min_consistent 0..4, step >= 1")
        self.D, self.sources, self.radius, self.uniq, self.min_views = int(D), int(sources), int(radius), int(uniq), int(min_views)
        self.eps, self.min_consistent, self.step = float(eps), int(min_consistent), int(step)


def source_order(i, n, count):
    """the `count` nearest frames of frame i in sequence order: i - 1, i + 1, i - 2, i + 2, ..."""
    out = []
    k = 1
    while len(out) < count and (i - k >= 0 or i + k < n):
        for j in (i - k, i + k):
            if 0 <= j < n and len(out) < count:
                out.append(j)
        k += 1
    return out


def plan(shape, K, rotations, positions, sparse_points, params):
    """the references of a sequence and everything the two library calls take:
    dict(ref, src, M, v, planes, nbr, nbrM, nbrv, B, c) with one row per reference
    (a frame with depth planes and at least min_views sources)"""
    n = len(rotations)
    refs, srcs, planes = [], [], []
    for i in range(n):
        w = depth_planes(K, rotations[i], positions[i], sparse_points, shape, params.D)
        s = source_order(i, n, params.sources)
        if w is None or len(s) < params.min_views or not np.all(np.isfinite(w)):
            continue
        refs.append(i)
        srcs.append(s)
        planes.append(w)
    map_of = {f: m for m, f in enumerate(refs)}
    nr = len(refs)
    M, v = np.zeros((nr, 4, 9)), np.zeros((nr, 4, 3))
    nbr, nbrM, nbrv = [], np.zeros((nr, 4, 9)), np.zeros((nr, 4, 3))
    B, c = np.zeros((nr, 9)), np.zeros((nr, 3))
    for m, i in enumerate(refs):
        row = []
        for k, j in enumerate(srcs[m]):
            Mk, vk = sweep_matrices(K, rotations[i], positions[i], rotations[j], positions[j])
            M[m, k], v[m, k] = Mk.reshape(9), vk
            if j in map_of:
                nbrM[m, len(row)], nbrv[m, len(row)] = Mk.reshape(9), vk
                row.append(map_of[j])
        nbr.append(row)
        Bm, cm = backproject_matrices(K, rotations[i], positions[i])
        B[m], c[m] = Bm.reshape(9), cm
    return dict(ref=refs, src=srcs, M=M, v=v, planes=np.array(planes).reshape(nr, params.D), nbr=nbr, nbrM=nbrM,
                nbrv=nbrv, B=B, c=c)


def _host_pixels(f):
    if getattr(f, "host_valid", True) is False:
        return f.dev.cpu().numpy()
    return np.ascontiguousarray(np.asarray(f))


def fuse_host(frames, inv, nbrs, M, v, B, c, eps, min_consistent, step, radius):
    """slam_mvs_fuse_dev's rule in numpy, operation for operation (the host path of densify)"""
    pts, cols = [np.zeros((0, 3))], [np.zeros((0, 3), np.uint8)]
    for i in range(len(inv)):
        wi = np.asarray(inv[i], np.float32)
        H, W = wi.shape
        ys, xs = np.mgrid[0:H, 0:W]
        fx, fy, wd = xs.astype(np.float64), ys.astype(np.float64), wi.astype(np.float64)
        count = np.zeros((H, W), np.int32)
        with np.errstate(all="ignore"):
            for n, j in enumerate(nbrs[i]):
                Mn, vn = np.asarray(M[i][n], np.float64).reshape(9), np.asarray(v[i][n], np.float64).reshape(3)
                h0, h1, h2 = (((Mn[3 * k] * fx + Mn[3 * k + 1] * fy) + Mn[3 * k + 2]) + wd * vn[k] for k in range(3))
                u, vv = h0 / h2, h1 / h2
                ok = (h2 > 0) & (u >= -0.5) & (u < W - 0.5) & (vv >= -0.5) & (vv < H - 0.5)
                ix = np.where(ok, np.floor(np.where(ok, u, 0.0) + 0.5), 0).astype(np.int64)
                iy = np.where(ok, np.floor(np.where(ok, vv, 0.0) + 0.5), 0).astype(np.int64)
                wj = np.asarray(inv[j], np.float32)[iy, ix]
                count += ok & (wi > 0) & (wj > 0) & (np.abs(h2 * wj.astype(np.float64) / wd - 1.0) <= eps)
        bd = radius + FILTER_BORDER
        keep = (wi > 0) & (count >= min_consistent) & (xs % step == 0) & (ys % step == 0) & (xs >= bd) & (xs < W - bd) \
            & (ys >= bd) & (ys < H - bd)
        y, x = np.nonzero(keep)
        Bi, ci = np.asarray(B[i], np.float64).reshape(9), np.asarray(c[i], np.float64).reshape(3)
        s = 1.0 / wi[y, x].astype(np.float64)
        px, py = x.astype(np.float64), y.astype(np.float64)
        pts.append(np.stack([ci[k] + ((Bi[3 * k] * px + Bi[3 * k + 1] * py) + Bi[3 * k + 2]) * s for k in range(3)], 1).reshape(-1, 3))
        f = np.asarray(frames[i], np.uint8)
        cols.append((np.repeat(f[y, x][:, None], 3, 1) if f.ndim == 2 else f[y, x]).reshape(-1, 3))
    return np.concatenate(pts).astype(np.float64), np.concatenate(cols).astype(np.uint8)


def stage_frames(frames, host):
    """the frames as the two paths take them: host arrays (host=True) or one resident
    torch batch (n, h, w[, 3]); a batch or a list that is staged already passes through"""
    if host:
        return [_host_pixels(f) for f in frames]
    import torch
    if isinstance(frames, torch.Tensor):
        return frames
    if all(getattr(f, "resident", False) for f in frames):
        from .cycle import device_frames
        return device_frames(list(frames))[0]
    return torch.from_numpy(np.stack([_host_pixels(f) for f in frames])).cuda()


def depth_maps(frames, K, rotations, positions, sparse_points, params=None, ctx=None, host=False, chunk=8):
    """The plane-sweep depth map of every reference of a sequence: (plan, inv_depth),
    with plan as plan() returns it and inv_depth[m] the float32 (h, w) map of frame
    plan["ref"][m]: a list of host arrays with host=True (slam_mvs_depth_host), else one
    resident (nref, h, w) tensor.  With params.sgm the maps are the semi-globally
    aggregated ones (slam_mvs_depth_sgm_batch_dev / slam_mvs_depth_sgm_host).  None when there are fewer than two frames or no
    reference.  densify and surface.reconstruct both start here."""
    from . import api
    params = params or DenseParams()
    if len(frames) != len(rotations) or len(frames) != len(positions):
        raise ValueError("depth_maps: one rotation and one position per frame")
    if len(frames) < 2:
        return None
    shape = tuple(frames[0].shape)
    if any(tuple(f.shape) != shape for f in frames):
        raise ValueError("depth_maps: frames of one shape")
    P = plan(shape, K, rotations, positions, sparse_points, params)
    nr = len(P["ref"])
    if nr == 0:
        return None
    h, w = shape[0], shape[1]
    st = stage_frames(frames, host)
    sgm = params.sgm
    if host:
        inv = []
        for m, i in enumerate(P["ref"]):
            S = len(P["src"][m])
            args = (st[i], [st[j] for j in P["src"][m]], P["M"][m, :S], P["v"][m, :S], P["planes"][m], params.radius,
                    params.uniq, params.min_views)
            if sgm is None:
                inv.append(api.planeSweepDepth(*args, host=True)[2])
            else:
                inv.append(api.planeSweepDepthSgm(*args, sgm.p1, sgm.p2, sgm.paths, host=True)[2])
        return P, inv
    import torch
    inv = torch.empty((nr, h, w), dtype=torch.float32, device=st.device)
    for m0 in range(0, nr, chunk):
        m1 = min(nr, m0 + chunk)
        args = (st, P["ref"][m0:m1], P["src"][m0:m1], P["M"][m0:m1], P["v"][m0:m1], P["planes"][m0:m1], params.radius,
                params.uniq, params.min_views)
        if sgm is None:
            _, _, iv = api.planeSweepDepthBatch(*args, ctx=ctx)
        else:
            _, _, iv = api.planeSweepDepthSgmBatch(*args, sgm.p1, sgm.p2, sgm.paths, ctx=ctx)
        inv[m0:m1] = iv
    return P, inv


def fuse_plan(st, P, inv, params, ctx=None, host=False):
    """the points of depth_maps' result: the pairwise filter and the emission (densify's second half)"""
    from . import api
    if host:
        return fuse_host([st[i] for i in P["ref"]], inv, P["nbr"], P["nbrM"], P["nbrv"], P["B"], P["c"], params.eps,
                         params.min_consistent, params.step, params.radius)
    return api.fuseDepthMaps(st, inv, P["nbr"], P["nbrM"], P["nbrv"], P["B"], P["c"], params.eps, params.min_consistent,
                             params.step, params.radius, frame_idx=P["ref"], ctx=ctx)


def densify(frames, K, rotations, positions, sparse_points, params=None, ctx=None, host=False, chunk=8):
    """Dense points of a sequence of good frames: (points (n, 3) float64, colors
    (n, 3) uint8).  frames[i] (ResidentFrames or host arrays of one shape) has the
    pose rotations[i], positions[i]; sparse_points bound each frame's depth range
    (depth_planes).  Every frame with planes is a reference with the params.sources
    nearest frames in sequence order as sources; the maps are filtered against the
    neighbours that are references themselves and emitted reference after reference.
    host=True computes the depth maps with slam_mvs_depth_host and fuses in numpy:
    the same points bit for bit, without a device."""
    params = params or DenseParams()
    if len(frames) != len(rotations) or len(frames) != len(positions):
        raise ValueError("densify: one rotation and one position per frame")
    empty = np.zeros((0, 3), np.float64), np.zeros((0, 3), np.uint8)
    if len(frames) < 2:
        return empty
    shape = frames[0].shape
    if any(f.shape != shape for f in frames):
        raise ValueError("densify: frames of one shape")
    st = stage_frames(frames, host)
    got = depth_maps(st, K, rotations, positions, sparse_points, params, ctx=ctx, host=host, chunk=chunk)
    if got is None:
        return empty
    return fuse_plan(st, got[0], got[1], params, ctx=ctx, host=host)

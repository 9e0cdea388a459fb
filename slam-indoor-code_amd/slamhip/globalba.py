"""Global bundle adjustment after loop closing (csrc/gba.hip; the contract is tests/gba_ref.py).

Every logged keyframe and every map point are re-fitted to the pixels with the intrinsics held constant:
Levenberg-Marquardt whose steps solve the Schur complement onto the cameras by conjugate gradients without
forming it.  Only + - * / and sqrt in f64 in a stated order, so the device (ctx), the host twin (host=True)
and the reference agree bit for bit.  A camera is 7 doubles (qw, qx, qy, qz, tx, ty, tz), X_c = R(q) X + t.

    cams, points, summary = solve(K4, cams, points, obs_cam, obs_point, obs_xy)        # the library call
    rot, mot, points, summary = global_bundle_adjust(K, rotations, motions, points, obs)
    obs2 = merge_observations(obs, npoints, constraints, dropped)                      # onto the closed cloud
    refined = refine_closed(closed, obs, K, LoopParams(close=True, global_ba=True))    # what slam_main calls
"""
import ctypes

import numpy as np

from . import _lib as L
from ._lib import check, lib, ptr
from .loopclose import _dp, _f64, _handle, _is_dev, _sync, matrix_quat, merged_roots, quat_matrix

SQUARE, HUBER = L.GBA_LOSS_SQUARE, L.GBA_LOSS_HUBER
SUMMARY_FIELDS = tuple(name for name, _ in L.GbaSummary._fields_)


def _k4(K):
    K = np.asarray(K, np.float64)
    if K.shape == (3, 3):
        return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float64)
    if K.size != 4:
        raise ValueError("K is a 3 x 3 matrix or (fx, fy, cx, cy)")
    return np.ascontiguousarray(K.reshape(4))


def solve(K4, cams, points, obs_cam, obs_point, obs_xy, loss=SQUARE, loss_param=1.0, zmin=0.1, lambda0=1e-4, max_lm=10,
          max_pcg=200, pcg_tol=1e-10, cost_tol=1e-9, ctx=None, host=False, staged=True):
    """slam_gba on cameras (n, 7) and points (m, 3) with observations (camera, point, x, y) in host arrays.
    Returns (cams, points, summary dict).  Host arrays in give host arrays out (host=True: the twin; staged=False:
    through torch tensors and slam_gba_dev); float64 device tensors in give device tensors out."""
    K4 = _k4(K4)
    oc = np.ascontiguousarray(np.asarray(obs_cam, np.int32).reshape(-1))
    op = np.ascontiguousarray(np.asarray(obs_point, np.int32).reshape(-1))
    xy = _f64(obs_xy, 2)
    if len(op) != len(oc) or len(xy) != len(oc):
        raise ValueError("one camera, one point and one pixel per observation")
    prm = L.GbaParams(int(loss), float(loss_param), float(zmin), float(lambda0), int(max_lm), int(max_pcg), float(pcg_tol),
                      float(cost_tol))
    out = L.GbaSummary()
    tail = (ptr(oc), ptr(op), ptr(xy), len(oc), ctypes.byref(prm), ctypes.byref(out))
    if _is_dev(cams) != _is_dev(points):
        raise TypeError("cameras and points: both host arrays or both device tensors")
    if _is_dev(cams):
        import torch
        if cams.dtype != torch.float64 or points.dtype != torch.float64:
            raise TypeError("device cameras and points are float64")
        c, p = cams.reshape(-1, 7).contiguous().clone(), points.reshape(-1, 3).contiguous().clone()
        _sync()
        h = _handle(ctx)
        check(lib().slam_gba_dev(h, None, ptr(K4), _dp(c), c.shape[0], _dp(p), p.shape[0], *tail), h)
    else:
        c, p = _f64(cams, 7).copy(), _f64(points, 3).copy()
        if host:
            check(lib().slam_gba_host(ptr(K4), ptr(c), len(c), ptr(p), len(p), *tail))
        elif staged:
            h = _handle(ctx)
            check(lib().slam_gba(h, ptr(K4), ptr(c), len(c), ptr(p), len(p), *tail), h)
        else:
            import torch
            dc, dp = torch.from_numpy(c).cuda(), torch.from_numpy(p).cuda()
            _sync()
            h = _handle(ctx)
            check(lib().slam_gba_dev(h, None, ptr(K4), _dp(dc), len(c), _dp(dp), len(p), *tail), h)
            c, p = dc.cpu().numpy(), dp.cpu().numpy()
    return c, p, {k: getattr(out, k) for k in SUMMARY_FIELDS}


def flatten_observations(obs, npoints):
    """(camera int32, point int32, xy f64) of observations in logs.obs form: per camera (xy n x 2, point index);
    an index outside [0, npoints) is no observation"""
    oc, op, xy = [], [], []
    for k, (pix, idx) in enumerate(obs):
        idx = np.asarray(idx, np.int64).reshape(-1)
        pix = np.asarray(pix, np.float64).reshape(-1, 2)
        ok = (idx >= 0) & (idx < npoints)
        oc.append(np.full(int(ok.sum()), k, np.int32))
        op.append(idx[ok].astype(np.int32))
        xy.append(pix[ok])
    if not oc:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2))
    return np.concatenate(oc), np.concatenate(op), np.concatenate(xy).reshape(-1, 2)


def global_bundle_adjust(K, rotations, motions, points, obs, loss=SQUARE, loss_param=1.0, zmin=0.1, lambda0=1e-4, max_lm=10,
                         max_pcg=200, pcg_tol=1e-10, cost_tol=1e-9, ctx=None, host=False):
    """Refits the poses X_c = R X + t (rotations (n, 3, 3), motions (n, 3)) and the points (m, 3) to the
    observations obs (logs.obs form) with K constant; camera 0 stays.  Returns (rotations, motions, points,
    summary).  Device tensors for rotations, motions and points give device tensors back."""
    dev = _is_dev(points)
    if dev != _is_dev(rotations) or dev != _is_dev(motions):
        raise TypeError("rotations, motions and points: all host arrays or all device tensors")
    if dev:
        import torch
        device = points.device
        rot = rotations.detach().cpu().numpy()
        mot = motions.detach().cpu().numpy()
    else:
        rot, mot = rotations, motions
    rot = np.asarray(rot, np.float64).reshape(-1, 3, 3)
    mot = np.asarray(mot, np.float64).reshape(-1, 3)
    if len(rot) != len(mot):
        raise ValueError("one motion per rotation")
    cams = np.array([np.concatenate([matrix_quat(R), t]) for R, t in zip(rot, mot)]).reshape(-1, 7)
    npoints = int(points.reshape(-1, 3).shape[0]) if dev else len(_f64(points, 3))
    oc, op, xy = flatten_observations(obs, npoints)
    kw = dict(loss=loss, loss_param=loss_param, zmin=zmin, lambda0=lambda0, max_lm=max_lm, max_pcg=max_pcg, pcg_tol=pcg_tol,
              cost_tol=cost_tol, ctx=ctx)
    if dev:
        c, p, summary = solve(K, torch.from_numpy(cams).to(device), points, oc, op, xy, **kw)
        c = c.cpu().numpy()
    else:
        c, p, summary = solve(K, cams, points, oc, op, xy, host=host, **kw)
    # a camera the solve did not move comes back as it went in, not through the quaternion
    same = (c == cams).all(1)
    r2 = np.array([rot[k] if same[k] else quat_matrix(c[k, :4]) for k in range(len(c))]).reshape(-1, 3, 3)
    m2 = c[:, 4:7].copy()
    if dev:
        return torch.from_numpy(r2).to(device), torch.from_numpy(m2).to(device), p, summary
    return r2, m2, p, summary


def merge_observations(obs, npoints, constraints, dropped):
    """The observations of the open map (npoints points) re-indexed onto the closed cloud: an observation of a dropped
    duplicate goes to its kept representative, and every index is compacted the way correct_map compacts the points.
    Both of a camera's observations of one merged point stay, as two residuals."""
    root = merged_roots(npoints, constraints)
    keep = root == np.arange(npoints)
    if not np.array_equal(np.flatnonzero(~keep), np.asarray(dropped, np.int64).reshape(-1)):
        raise ValueError("dropped is not what the constraints merge")
    new = np.cumsum(keep) - 1
    out = []
    for pix, idx in obs:
        idx = np.asarray(idx, np.int64).reshape(-1)
        ok = (idx >= 0) & (idx < npoints)
        to = np.full(len(idx), -1, np.int64)
        to[ok] = new[root[idx[ok]]]
        out.append((pix, to))
    return out


def refine_closed(closed, obs, K, prm, ctx=None, host=False):
    """Global bundle adjustment of a closed map (close_loops' or close_run's dict) over the run's observations.
    Returns a dict: rotations, motions, points, colors, summary.  With no accepted loop the closed result comes
    back as it is (summary None)."""
    res = {k: np.array(closed[k]) for k in ("rotations", "motions", "points", "colors")}
    res["summary"] = None
    if not any(c["accepted"] for c in closed["constraints"]):
        return res
    npoints = len(closed["points"]) + len(closed["dropped"])
    obs2 = merge_observations(obs, npoints, closed["constraints"], closed["dropped"])
    rot, mot, pts, summary = global_bundle_adjust(K, closed["rotations"], closed["motions"], closed["points"], obs2,
                                                  loss=prm.gba_loss, loss_param=prm.gba_loss_param, zmin=prm.gba_zmin,
                                                  max_lm=prm.gba_max_lm, max_pcg=prm.gba_max_pcg, ctx=ctx, host=host)
    res.update(rotations=rot, motions=mot, points=pts, summary=summary)
    return res

"""One coloured surface from the depth maps: volumetric fusion into a truncated signed
distance field and marching cubes on its node lattice.  The
library never forms a pose or a projection: this module turns the cycle's poses into the
3 x 4 matrices slam_tsdf_integrate_dev takes, sizes the volume from the sparse cloud,
integrates the plane-sweep maps chunk by chunk and extracts the mesh.  The reference has
no such stage; it is opt-in everywhere.

Pose convention (dense.py's): a camera is [R | t], x_cam = R X + t, a pixel is K x_cam / z.
"""
import math

import numpy as np

MAX_MAPS = 1 << 20          # a volume's sums stay inside int32 up to this many maps


def projection_matrix(K, R, t):
    """P = K [R | t] (3 x 4 float64): [K R | K t], each a plain matrix product.
    tests/tsdf_ref.py uses this same function, so both sides hand the kernels the same bits."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    return np.concatenate([K @ R, (K @ t).reshape(3, 1)], axis=1)


class SurfaceParams:
    """slam_main(surface=...) / reconstruct: the node count of the volume's longest side,
    the truncation distance in voxels, the least number of maps that must have seen a
    node (the outlier filter), and the margin added to the sparse cloud's 5 % .. 95 % box
    on each side, as a fraction of its extent."""

    def __init__(self, max_dim=256, trunc_voxels=4.0, min_weight=2, pad=0.25):
        if not 2 <= int(max_dim) <= 2048 or not (trunc_voxels > 0 and math.isfinite(trunc_voxels)) or int(min_weight) < 1 \
                or not (pad >= 0 and math.isfinite(pad)):
            raise ValueError("SurfaceParams: max_dim 2..2048, trunc_voxels > 0, min_weight >= 1, pad >= 0")
        self.max_dim, self.trunc_voxels, self.min_weight, self.pad = int(max_dim), float(trunc_voxels), int(min_weight), float(pad)


def volume_bounds(sparse_points, params):
    """(origin (3,), voxel, (nx, ny, nz)) of the volume around the sparse cloud, or None
    with fewer than 8 points (or a cloud without extent).  Per axis lo = x[n // 20] and
    hi = x[n - 1 - n // 20] of the sorted coordinates, each side extended by pad * (hi - lo);
    voxel = the largest extent / (max_dim - 1); n_k = clamp(ceil(extent_k / voxel) + 1, 2, max_dim)."""
    X = np.asarray(sparse_points, np.float64).reshape(-1, 3)
    n = len(X)
    if n < 8 or not np.all(np.isfinite(X)):
        return None
    srt = np.sort(X, axis=0)
    lo, hi = srt[n // 20], srt[n - 1 - n // 20]
    ext = hi - lo
    lo, hi = lo - params.pad * ext, hi + params.pad * ext
    ext = hi - lo
    voxel = float(ext.max()) / (params.max_dim - 1)
    if not (voxel > 0 and math.isfinite(voxel)):
        return None
    dims = tuple(int(min(max(math.ceil(float(e) / voxel) + 1, 2), params.max_dim)) for e in ext)
    return lo.copy(), voxel, dims


def _empty():
    return np.zeros((0, 3), np.float64), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32)


def fuse_maps(frames, ref, inv_depth, K, rotations, positions, sparse_points, params, ctx=None, host=False, chunk=8):
    """the surface of depth maps already computed: inv_depth[m] belongs to frame ref[m]
    (dense.depth_maps' plan["ref"] and maps).  frames: a resident torch batch with a
    resident inv_depth, or (host=True) host arrays.  Returns (vertices, colors, faces)."""
    from . import api
    bounds = volume_bounds(sparse_points, params)
    if bounds is None or len(ref) == 0:
        return _empty()
    origin, voxel, (nx, ny, nz) = bounds
    if len(ref) > MAX_MAPS:
        raise ValueError("a volume takes at most 2^20 maps")
    trunc = params.trunc_voxels * voxel
    P = np.stack([projection_matrix(K, rotations[i], positions[i]) for i in ref])
    if host:
        vol = np.zeros((6, nz, ny, nx), np.int32)
    else:
        import torch
        vol = torch.zeros((6, nz, ny, nx), dtype=torch.int32, device=inv_depth.device)
    for m0 in range(0, len(ref), chunk):
        m1 = min(len(ref), m0 + chunk)
        api.tsdfIntegrate(vol, frames, inv_depth[m0:m1], P[m0:m1], origin, voxel, trunc, frame_idx=list(ref[m0:m1]), ctx=ctx,
                          host=host)
    return api.tsdfMesh(vol, origin, voxel, params.min_weight, ctx=ctx, host=host)


def reconstruct(frames, K, rotations, positions, sparse_points, dense_params=None, params=None, ctx=None, host=False, chunk=8):
    """The surface of a sequence of good frames: (vertices (n, 3) float64, colors (n, 3)
    uint8 blue-green-red, faces (m, 3) int32).  The plane-sweep maps of dense.depth_maps
    are integrated chunk by chunk into a volume sized by volume_bounds and extracted with
    params.min_weight.  host=True runs the host twins: the same bits, without a device."""
    from . import dense
    params = params or SurfaceParams()
    dense_params = dense_params or dense.DenseParams()
    if len(frames) < 2:
        return _empty()
    st = dense.stage_frames(frames, host)
    got = dense.depth_maps(st, K, rotations, positions, sparse_points, dense_params, ctx=ctx, host=host, chunk=chunk)
    if got is None:
        return _empty()
    plan, inv = got
    return fuse_maps(st, plan["ref"], inv, K, rotations, positions, sparse_points, params, ctx=ctx, host=host, chunk=chunk)

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

    def __init__(self, max_dim=256, trunc_voxels=4.0, min_weight=2, pad=0.25, texture=None):
        if not 2 <= int(max_dim) <= 2048 or not (trunc_voxels > 0 and math.isfinite(trunc_voxels)) or int(min_weight) < 1 \
                or not (pad >= 0 and math.isfinite(pad)):
            raise ValueError("SurfaceParams: max_dim 2..2048, trunc_voxels > 0, min_weight >= 1, pad >= 0")
        if texture is not None and not isinstance(texture, TextureParams):
            raise ValueError("SurfaceParams: texture is a TextureParams or None")
        self.max_dim, self.trunc_voxels, self.min_weight, self.pad = int(max_dim), float(trunc_voxels), int(min_weight), float(pad)
        self.texture = texture       # slam_main: also texture the mesh from the good frames (section 29)


class TextureParams:
    """texture(...) / SurfaceParams(texture=...): texels per triangle leg (1..64), the largest
    page side in texels (texel + 4 .. 8192), the least number of pixels a face must cover in
    its best view to be textured from it (fewer: the vertex colours), and the number of views
    (None: every posed frame; otherwise an evenly spaced subset)."""

    def __init__(self, texel=12, page=4096, min_pixels=4, max_views=None):
        if not 1 <= int(texel) <= 64 or not int(texel) + 4 <= int(page) <= 8192 or not 1 <= int(min_pixels) <= 1 << 30 \
                or (max_views is not None and int(max_views) < 1):
            raise ValueError("TextureParams: texel 1..64, page texel + 4..8192, min_pixels 1..2^30, max_views >= 1 or None")
        self.texel, self.page, self.min_pixels = int(texel), int(page), int(min_pixels)
        self.max_views = None if max_views is None else int(max_views)


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


# ---- texture of the surface: a per-face atlas from the good frames ----

def view_camera(K, R, t, vertices, size):
    """What the rasteriser takes to see the mesh as the camera [R | t] with the matrix K does:
    (pose, camera), pose = (R^T, -(R^T t)) (camera to world) and camera = (fx, fy, cx + 0.5,
    cy + 0.5, near, far); the + 0.5 because the rasteriser's pixel (i, j) covers [i, i + 1) while
    a frame's pixel centres sit at integer coordinates.  near and far come from the vertices'
    depths in this view, z = ((R20 X + R21 Y) + R22 Z) + t2 over the finite vertices with z > 0:
    far = 2 max z, near = max(min z / 2, far / 16384); without such a vertex (0.01, 1000.01).
    tests/tex_ref.py uses this same function, so both sides hand the rasteriser the same bits.
    A K with skew (K[0][1] != 0) raises ValueError: the rasteriser has none."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    if K[0, 1] != 0.0:
        raise ValueError("view_camera: K has skew, the rasteriser has none")
    V = np.asarray(vertices, np.float64).reshape(-1, 3)
    z = ((R[2, 0] * V[:, 0] + R[2, 1] * V[:, 1]) + R[2, 2] * V[:, 2]) + t[2]
    z = z[np.isfinite(z) & (z > 0)]
    if len(z):
        far = 2.0 * float(z.max())
        near = max(float(z.min()) / 2.0, far / 16384.0)
    else:
        near, far = 0.01, 1000.01
    if not (0 < near < far and math.isfinite(far)):
        near, far = 0.01, 1000.01
    return (R.T.copy(), -(R.T @ t)), (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]) + 0.5, float(K[1, 2]) + 0.5, near, far)


def texture_views(n, max_views=None):
    """the frames a texture takes its views from: all n, or the centres of max_views equal
    bins of 0 .. n - 1: (2 i n + n) // (2 max_views)"""
    if max_views is None or max_views >= n:
        return list(range(n))
    return [(2 * i * n + n) // (2 * max_views) for i in range(max_views)]


class Texture:
    """texture()'s result: uv (nf, 3, 2) float64, page (nf,) int32, atlas (a list of (H, W, 3)
    uint8 pages, blue-green-red), best_view / best_count (nf,) int32 (view indices into
    `views`, the frame index of every view), textured = the faces that take a frame's pixels"""

    def __init__(self, uv, page, atlas, best_view, best_count, views, min_pixels):
        self.uv, self.page, self.atlas, self.best_view, self.best_count, self.views = uv, page, atlas, best_view, best_count, views
        self.textured = (best_count >= min_pixels) & (best_view >= 0)


def texture(vertices, colors, faces, frames, K, rotations, positions, params=None, ctx=None, host=False, ids=None, chunk=8):
    """A per-face texture atlas of the mesh (tsdfMesh's vertices, colors, faces) from the posed
    frames: frame i has the camera [rotations[i] | positions[i]] (dense.py's convention).  Every
    view (texture_views) renders the mesh's face ids (view_camera, api.renderViews), chunk views
    at a time, never all resident at once; api.texSelect keeps the view that shows each face
    in the most pixels, api.texFill resamples that frame into the face's atlas cell.  A face
    partly hidden in its best view samples the occluder there (section 29).  Returns a Texture.
    The library has no host rasteriser: host=True runs the host twins and needs the id images
    passed in, `ids` = an (nviews, h, w) int32 array or a function (m0, m1) -> the ids of
    views m0 .. m1 - 1.  frames: a resident batch or a list, staged as dense.stage_frames does."""
    from . import api
    from .dense import stage_frames
    params = params or TextureParams()
    V = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    C = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    F = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nf = len(F)
    if host and ids is None:
        raise ValueError("texture(host=True) needs ids: the library has no host rasteriser")
    if nf == 0:
        _, _, uv, page = api.texLayout(0, params.texel, params.page)
        return Texture(uv, page, [], np.full(nf, -1, np.int32), np.zeros(nf, np.int32), [], params.min_pixels)
    if len(frames) == 0:
        raise ValueError("texture: no frames")
    st = stage_frames(frames, host)
    h, w = (int(st.shape[1]), int(st.shape[2])) if hasattr(st, "data_ptr") else st[0].shape[:2]
    views = texture_views(min(len(st), len(rotations)), params.max_views)
    P = np.stack([projection_matrix(K, rotations[i], positions[i]) for i in views]) if views else np.zeros((0, 3, 4))
    if host:
        state = (np.zeros(nf, np.int32), np.full(nf, -1, np.int32))
    else:
        import torch
        dev = st.device
        state = (torch.zeros(nf, dtype=torch.int32, device=dev), torch.full((nf,), -1, dtype=torch.int32, device=dev))
        pts = torch.from_numpy(V.astype(np.float32)).to(dev)
        cols, fcs = torch.from_numpy(C).to(dev), torch.from_numpy(F).to(dev)
        no_lines = (np.zeros((0, 6), np.float32), np.zeros((0, 3), np.uint8))
    for m0 in range(0, len(views) if nf else 0, chunk):
        m1 = min(len(views), m0 + chunk)
        if ids is not None:
            part = ids(m0, m1) if callable(ids) else ids[m0:m1]
            if not host and not hasattr(part, "data_ptr"):
                part = torch.from_numpy(np.ascontiguousarray(part, np.int32)).to(dev)
        else:
            part = []
            for m in range(m0, m1):
                pose, cam = view_camera(K, rotations[views[m]], positions[views[m]], V, (w, h))
                part.append(api.renderViews(pts, cols, fcs, *no_lines, [pose], camera=cam, size=(w, h), ids=True, ctx=ctx)[1])
            part = torch.cat(part)
        api.texSelect(part, m0, nf, state, ctx=ctx, host=host)
    bc, bv = state
    atlas = api.texFill(V, C, F, st, P, bc, bv, params.min_pixels, params.texel, params.page, frame_idx=views, ctx=ctx, host=host)
    if not host:
        bc, bv = bc.cpu().numpy(), bv.cpu().numpy()
    _, _, uv, page = api.texLayout(nf, params.texel, params.page)
    return Texture(uv, page, atlas, bv, bc, views, params.min_pixels)

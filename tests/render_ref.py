"""The definition of the scene renderer (slam-indoor-code_amd/csrc/render.hip,
render_setup.h): numpy and Python floats, no device.  The kernels must equal
`render` byte for byte: frames, ids and depth.

Python's float is an IEEE f64 and nothing here is fused, so every expression
below is the operation order of the contract; the C++ header restates it.

Camera    view = (R, t), camera to world; p_cam = R^T (p - t), sums left to
          right.  u = fx X / Z + cx, v = fy Y / Z + cy.  Looks along +z, x right,
          y down.  Pixel (i, j) covers [i, i + 1) x [j, j + 1), centre (i + 1/2, j + 1/2).
Clip      in camera space, before any rounding: near, far, left, right, top,
          bottom, the side planes widened by GUARD pixels; distance >= 0 is
          inside; a new vertex is I + t (O - I), t = dI / (dI - dO), always from
          the inside vertex I to the outside vertex O.  Colours are carried as
          f64 and rounded half up once, after the last plane.
Faces     indices sorted ascending first (the picture does not depend on how a
          face lists its vertices); clipped polygon v0 .. -> fan (v0, vi, vi+1);
          vertices snapped to 1/16 pixel by floor(16 u + 1/2); winding normalised
          by swapping vertices 1 and 2; int64 edge functions, top-left rule;
          colour = exact integer affine blend, round half up; depth = 1/Z, affine:
          ((w0 z0 + w1 z1) + w2 z2) / area2 in f64, rounded to f32.
Lines     clipped alike; endpoints snapped to floor(u), floor(v); walked from the
          endpoint lower in (y, x): step k of n = max(|dx|, |dy|) (x major when
          |dx| >= |dy|) moves the minor axis by (2 k dminor + n) // (2 n): the
          midpoint (Bresenham) line; depth ((n - k) z0 + k z1) / n, and the nearer
          endpoint's when n = 0.
Points    near <= Z <= far and 0 <= u < w, 0 <= v < h, else culled; a square of
          point_size pixels about (floor(u), floor(v)) at f32(1 / Z).
Key       ~bits(f32 depth) << 32 | kind << 30 | index, kind 0 point, 1 line,
          2 face; the smallest key wins the pixel.  Background: white, id -1, depth 0.
"""
import math

import numpy as np

GUARD = 32768.0
MAX_DIM = 8192
SNAP_LIMIT = (MAX_DIM + GUARD) * 16.0 + 16.0
PIXEL_LIMIT = MAX_DIM + GUARD + 1.0
POINT, LINE, FACE = 0, 1, 2
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def default_camera(size=(1000, 1000)):
    """viz::Camera(Vec2d(1, 1), Size(w, h)): a field of view of 1 rad per axis,
    the principal point at the centre, clip range (0.01, 1000.01)"""
    w, h = size
    return ((w / 2) / math.tan(0.5), (h / 2) / math.tan(0.5), w / 2, h / 2, 0.01, 1000.01)


class Camera:
    def __init__(self, cam, w, h):
        self.fx, self.fy, self.cx, self.cy, self.near, self.far = (float(v) for v in cam)
        self.w, self.h = int(w), int(h)
        self.kl = self.cx + GUARD
        self.kr = (float(w) + GUARD) - self.cx
        self.kt = self.cy + GUARD
        self.kb = (float(h) + GUARD) - self.cy

    def dist(self, k, p):
        x, y, z = p[0], p[1], p[2]
        if k == 0:
            return z - self.near
        if k == 1:
            return self.far - z
        if k == 2:
            return self.fx * x + self.kl * z
        if k == 3:
            return self.kr * z - self.fx * x
        if k == 4:
            return self.fy * y + self.kt * z
        return self.kb * z - self.fy * y


def view_of(R, t):
    """the 12 numbers of a view: R row major, then t"""
    return [float(v) for v in np.asarray(R, np.float64).reshape(9)] + [float(v) for v in np.asarray(t, np.float64).reshape(3)]


def to_camera(view, p):
    d0, d1, d2 = float(p[0]) - view[9], float(p[1]) - view[10], float(p[2]) - view[11]
    return [(view[0] * d0 + view[3] * d1) + view[6] * d2,
            (view[1] * d0 + view[4] * d1) + view[7] * d2,
            (view[2] * d0 + view[5] * d1) + view[8] * d2]


def clip_point(a, da, b, db):
    """from the inside vertex a to the outside vertex b; vertices are lists of position then attributes"""
    t = da / (da - db)
    return [x + t * (y - x) for x, y in zip(a, b)]


def clip_polygon(cam, poly):
    for k in range(6):
        d = [cam.dist(k, p) for p in poly]
        inside = [v >= 0.0 for v in d]
        if all(inside):
            continue
        if not any(inside):
            return []
        out = []
        n = len(poly)
        for i in range(n):
            j = i - 1 if i else n - 1
            if inside[i]:
                if not inside[j]:
                    out.append(clip_point(poly[i], d[i], poly[j], d[j]))
                out.append(poly[i])
            elif inside[j]:
                out.append(clip_point(poly[j], d[j], poly[i], d[i]))
        poly = out[:9]
        if len(poly) < 3:
            return []
    return poly


def round_color(v):
    r = math.floor(v + 0.5)
    return 0 if not r > 0 else min(int(r), 255)


def setup_triangle(cam, view, p, c):
    """p: three world points, c: three BGR colours.  The clipped polygon as a
    list of (x, y, 1/Z, (b, g, r)) with x, y in 1/16 pixel; [] when clipped
    away; None when a coordinate leaves the fixed-point range."""
    poly = clip_polygon(cam, [to_camera(view, p[i]) + [float(v) for v in c[i]] for i in range(3)])
    out = []
    for v in poly:
        u = (cam.fx * v[0]) / v[2] + cam.cx
        w = (cam.fy * v[1]) / v[2] + cam.cy
        if not (math.isfinite(u) and math.isfinite(w)):
            return None
        su, sv = math.floor(u * 16.0 + 0.5), math.floor(w * 16.0 + 0.5)
        if not (-SNAP_LIMIT <= su <= SNAP_LIMIT and -SNAP_LIMIT <= sv <= SNAP_LIMIT):
            return None
        out.append((int(su), int(sv), 1.0 / v[2], tuple(round_color(x) for x in v[3:6])))
    return out


def tri_prepare(cam, poly, piece):
    """fan piece `piece` as (x[3], y[3], iz[3], c[3], area2, (bx0, by0, bx1, by1)), or None when it covers nothing"""
    v = [poly[0], poly[piece + 1], poly[piece + 2]]
    a = (v[1][0] - v[0][0]) * (v[2][1] - v[0][1]) - (v[1][1] - v[0][1]) * (v[2][0] - v[0][0])
    if a == 0:
        return None
    if a < 0:
        a = -a
        v[1], v[2] = v[2], v[1]
    xs, ys = [q[0] for q in v], [q[1] for q in v]
    bx0, bx1 = max((min(xs) + 7) >> 4, 0), min((max(xs) - 8) >> 4, cam.w - 1)
    by0, by1 = max((min(ys) + 7) >> 4, 0), min((max(ys) - 8) >> 4, cam.h - 1)
    if bx0 > bx1 or by0 > by1:
        return None
    return xs, ys, [q[2] for q in v], [q[3] for q in v], a, (bx0, by0, bx1, by1)


def edge_bias(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return 0 if (dy < 0 or (dy == 0 and dx > 0)) else -1


def tri_fragments(tri):
    """(ys, xs, depth f32, colour u8 (n, 3)) of the covered pixels of a prepared triangle"""
    xs, ys, iz, col, area2, (bx0, by0, bx1, by1) = tri
    py, px = np.mgrid[by0:by1 + 1, bx0:bx1 + 1]
    sx, sy = px.astype(np.int64) * 16 + 8, py.astype(np.int64) * 16 + 8
    w = []
    cover = np.ones(px.shape, bool)
    for i in range(3):
        a, b = (i + 1) % 3, (i + 2) % 3
        e = (xs[b] - xs[a]) * (sy - ys[a]) - (ys[b] - ys[a]) * (sx - xs[a])
        cover &= (e + edge_bias(xs[a], ys[a], xs[b], ys[b])) >= 0
        w.append(e)
    depth = (((w[0].astype(np.float64) * iz[0] + w[1].astype(np.float64) * iz[1]) + w[2].astype(np.float64) * iz[2])
             / float(area2)).astype(np.float32)
    color = np.stack([(2 * (w[0] * col[0][k] + w[1] * col[1][k] + w[2] * col[2][k]) + area2) // (2 * area2)
                      for k in range(3)], -1).astype(np.uint8)
    return py[cover], px[cover], depth[cover], color[cover]


def tri_pixel(tri, px, py):
    """one pixel centre of a prepared triangle: None when not covered, else (f32 depth, (b, g, r))"""
    xs, ys, iz, col, area2, _ = tri
    sx, sy = px * 16 + 8, py * 16 + 8
    w = []
    for i in range(3):
        a, b = (i + 1) % 3, (i + 2) % 3
        e = (xs[b] - xs[a]) * (sy - ys[a]) - (ys[b] - ys[a]) * (sx - xs[a])
        if e + edge_bias(xs[a], ys[a], xs[b], ys[b]) < 0:
            return None
        w.append(e)
    depth = np.float32(((float(w[0]) * iz[0] + float(w[1]) * iz[1]) + float(w[2]) * iz[2]) / float(area2))
    return depth, tuple((2 * (w[0] * col[0][k] + w[1] * col[1][k] + w[2] * col[2][k]) + area2) // (2 * area2)
                        for k in range(3))


def project_pixel(cam, q):
    u = (cam.fx * q[0]) / q[2] + cam.cx
    v = (cam.fy * q[1]) / q[2] + cam.cy
    if not (math.isfinite(u) and math.isfinite(v)):
        return None
    u, v = math.floor(u), math.floor(v)
    if not (-PIXEL_LIMIT <= u <= PIXEL_LIMIT and -PIXEL_LIMIT <= v <= PIXEL_LIMIT):
        return None
    return int(u), int(v)


def setup_line(cam, view, a, b):
    """((x0, y0), (x1, y1), iz0, iz1) in pixels with (y0, x0) <= (y1, x1); [] when clipped away; None out of range"""
    p = [to_camera(view, a), to_camera(view, b)]
    for k in range(6):
        d = [cam.dist(k, p[0]), cam.dist(k, p[1])]
        inside = [d[0] >= 0.0, d[1] >= 0.0]
        if all(inside):
            continue
        if not any(inside):
            return []
        i = 0 if inside[0] else 1
        p[1 - i] = clip_point(p[i], d[i], p[1 - i], d[1 - i])
    e = [project_pixel(cam, p[0]), project_pixel(cam, p[1])]
    if e[0] is None or e[1] is None:
        return None
    s = 1 if (e[1][1], e[1][0]) < (e[0][1], e[0][0]) else 0
    return e[s], e[1 - s], 1.0 / p[s][2], 1.0 / p[1 - s][2]


def line_fragments(cam, line):
    """(ys, xs, depth f32) of the walk's pixels inside the viewport, and the number of steps tested"""
    (x0, y0), (x1, y1), iz0, iz1 = line
    dx, dy = x1 - x0, y1 - y0
    adx, sx = abs(dx), (-1 if dx < 0 else 1)
    xmajor = adx >= dy
    n, dminor = (adx, dy) if xmajor else (dy, adx)
    if xmajor:
        lo, hi = (-x0, cam.w - 1 - x0) if sx > 0 else (x0 - (cam.w - 1), x0)
    else:
        lo, hi = -y0, cam.h - 1 - y0
    k0, k1 = max(lo, 0), min(hi, n)
    if k0 > k1:
        return None
    k = np.arange(k0, k1 + 1, dtype=np.int64)
    m = (2 * k * dminor + n) // (2 * n) if n > 0 else np.zeros_like(k)
    if xmajor:
        x, y = x0 + sx * k, y0 + m
    else:
        x, y = x0 + sx * m, y0 + k
    if n > 0:
        depth = (((n - k).astype(np.float64) * iz0 + k.astype(np.float64) * iz1) / float(n)).astype(np.float32)
    else:
        depth = np.full(len(k), max(iz0, iz1), np.float64).astype(np.float32)
    ok = (x >= 0) & (x < cam.w) & (y >= 0) & (y < cam.h)
    return y[ok], x[ok], depth[ok], len(k)


def setup_point(cam, view, p):
    """(px, py, f32 depth) or None when culled"""
    q = to_camera(view, p)
    if not (q[2] >= cam.near and q[2] <= cam.far):
        return None
    u = (cam.fx * q[0]) / q[2] + cam.cx
    v = (cam.fy * q[1]) / q[2] + cam.cy
    if not (0.0 <= u < float(cam.w) and 0.0 <= v < float(cam.h)):
        return None
    return int(u), int(v), np.float32(1.0 / q[2])


def keys_of(depth, kind, index):
    bits = np.asarray(depth, np.float32).view(np.uint32)
    return ((~bits).astype(np.uint64) << np.uint64(32)) | np.uint64((kind << 30) | index)


class Stats:
    def __init__(self):
        self.prims = self.skipped = self.clipped = self.rasterised = self.fragments = 0

    def tuple(self):
        return (self.prims, self.skipped, self.clipped, self.rasterised, self.fragments)


def face_pieces(cam, view, pts, cols, face):
    """the prepared fan triangles of one face; None when it is skipped"""
    idx = sorted(int(i) for i in face)
    if idx[0] < 0 or idx[2] >= len(pts):
        return None
    p = [pts[i] for i in idx]
    if not all(np.isfinite(q).all() for q in p):
        return None
    poly = setup_triangle(cam, view, p, [cols[i] for i in idx])
    if poly is None:
        return None
    return [t for t in (tri_prepare(cam, poly, i) for i in range(max(len(poly) - 2, 0))) if t is not None]


def render_view(pts, cols, faces, lines, line_cols, view, cam, point_size=1, stats=None):
    """one view: (frame (h, w, 3) u8 BGR, ids (h, w) int32, depth (h, w) f32)"""
    st = stats if stats is not None else Stats()
    w, h = cam.w, cam.h
    keys = np.full((h, w), EMPTY, np.uint64)
    tri_frags = []
    st.prims += len(pts) + len(faces) + len(lines)

    def put(ys, xs, depth, kind, index):
        k = keys_of(depth, kind, index)
        np.minimum.at(keys, (ys, xs), k)
        return k

    r = (point_size - 1) // 2
    for i, p in enumerate(pts):
        if not np.isfinite(p).all():
            st.skipped += 1
            continue
        s = setup_point(cam, view, p)
        if s is None:
            st.clipped += 1
            continue
        px, py, d = s
        ys, xs = np.mgrid[max(py - r, 0):min(py + r, h - 1) + 1, max(px - r, 0):min(px + r, w - 1) + 1]
        put(ys.ravel(), xs.ravel(), np.full(ys.size, d, np.float32), POINT, i)
        st.rasterised += 1
        st.fragments += ys.size
    for i, l in enumerate(lines):
        if not np.isfinite(l).all():
            st.skipped += 1
            continue
        s = setup_line(cam, view, l[:3], l[3:])
        f = line_fragments(cam, s) if s else None
        if s is None:
            st.skipped += 1
        elif f is None:
            st.clipped += 1
        else:
            put(f[0], f[1], f[2], LINE, i)
            st.rasterised += 1
            st.fragments += f[3]
    for i, face in enumerate(faces):
        pieces = face_pieces(cam, view, pts, cols, face)
        if pieces is None:
            st.skipped += 1
            continue
        if not pieces:
            st.clipped += 1
            continue
        for t in pieces:
            ys, xs, d, c = tri_fragments(t)
            k = put(ys, xs, d, FACE, i)
            st.rasterised += 1
            st.fragments += (t[5][2] - t[5][0] + 1) * (t[5][3] - t[5][1] + 1)
            tri_frags.append((ys, xs, k, c))
    frame = np.full((h, w, 3), 255, np.uint8)
    ids = np.full((h, w), -1, np.int32)
    depth = np.zeros((h, w), np.float32)
    hit = keys != EMPTY
    lo = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    kind, index = lo >> np.uint32(30), (lo & np.uint32((1 << 30) - 1)).astype(np.int64)
    ids[hit] = lo[hit].astype(np.int32)
    depth[hit] = (~(keys >> np.uint64(32)).astype(np.uint32)).view(np.float32)[hit]
    m = hit & (kind == POINT)
    frame[m] = cols[index[m]]
    m = hit & (kind == LINE)
    frame[m] = line_cols[index[m]]
    for ys, xs, k, c in tri_frags:          # fan pieces of one face share a key and never a pixel
        win = keys[ys, xs] == k
        frame[ys[win], xs[win]] = c[win]
    return frame, ids, depth


def _arrays(points, colors, faces, lines, line_colors):
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    cols = np.asarray(colors, np.uint8).reshape(-1, 3)
    fcs = np.asarray(faces, np.int32).reshape(-1, 3)
    lns = np.asarray(lines, np.float32).reshape(-1, 6)
    lcs = np.asarray(line_colors, np.uint8).reshape(-1, 3)
    assert len(pts) == len(cols) and len(lns) == len(lcs)
    return pts, cols, fcs, lns, lcs


def render(points, colors, faces, lines, line_colors, views, camera=None, size=(1000, 1000), point_size=1, stats=None):
    """views: a list of (R, t).  Returns (frames (n, h, w, 3), ids (n, h, w), depth (n, h, w))."""
    pts, cols, fcs, lns, lcs = _arrays(points, colors, faces, lines, line_colors)
    w, h = size
    cam = Camera(camera if camera is not None else default_camera(size), w, h)
    out = [render_view(pts, cols, fcs, lns, lcs, view_of(R, t), cam, point_size, stats) for R, t in views]
    if not out:
        return np.zeros((0, h, w, 3), np.uint8), np.zeros((0, h, w), np.int32), np.zeros((0, h, w), np.float32)
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def coverage(points, faces, view, camera, size):
    """how many faces cover each pixel centre (no depth test): (h, w) int"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    cols = np.zeros((len(pts), 3), np.uint8)
    cam = Camera(camera, *size)
    count = np.zeros((size[1], size[0]), np.int64)
    for face in np.asarray(faces, np.int32).reshape(-1, 3):
        for t in face_pieces(cam, view_of(*view), pts, cols, face) or []:
            ys, xs, _, _ = tri_fragments(t)
            np.add.at(count, (ys, xs), 1)
    return count

"""numpy restatement of the reference's scene post-processing, the yardstick of
tests/test_scene.py and tests/test_scene_gpu.py (our own text, as oracle/
restates OpenCV):

  edge_matrix / clusterize   clusterizePoints + findComps + dfs
                             src/vizualization/delauney-triangulation/geomAdditionalFunc.cpp:16-18,105-163
  project_to_plane           projectPointOnPlane (:20-32) + makeMesh (bestFittingPlane.cpp:51-63)
  fit_plane                  the intent of getBestFittingPlaneByPoints (bestFittingPlane.cpp:11-40)

numpy evaluates every elementwise operation on its own (one IEEE rounding per
operation, no fused multiply-add), its f64 sqrt and divide are correctly
rounded, and a float32 array minus a float32 array stays float32: the same
arithmetic the reference's C++ performs.
"""
import numpy as np


def params32(max_distance, euclid_weight, color_weight):
    """the config values as the reference holds them: getValue<float> widened to double"""
    return tuple(np.float64(np.float32(v)) for v in (max_distance, euclid_weight, color_weight))


def pair_sums(points, colors, rows, euclid_weight, color_weight):
    """realDistance + colorDistance (f64) of the points `rows` against all points"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3).astype(np.int32)
    d = p[rows, None, :] - p[None, :, :]                   # Point3f operator-: f32
    assert d.dtype == np.float32
    d = d.astype(np.float64)
    s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]   # sqr(x) + sqr(y) + sqr(z)
    real = np.sqrt(s) * euclid_weight
    dc = c[rows, None, :] - c[None, :, :]
    ci = dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1] + dc[..., 2] * dc[..., 2]   # normDiffL2Sqr, exact
    col = np.sqrt(ci.astype(np.float64)) * color_weight
    return real + col


def edge_matrix(points, colors, max_distance, euclid_weight, color_weight, chunk=512):
    """graph != -1 of clusterizePoints as an n x n bool matrix.  The parameters
    pass through f32 first (params32)."""
    mx, dw, cw = params32(max_distance, euclid_weight, color_weight)
    n = len(np.asarray(points).reshape(-1, 3))
    adj = np.zeros((n, n), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, n, chunk):
            rows = np.arange(r0, min(n, r0 + chunk))
            adj[rows] = pair_sums(points, colors, rows, dw, cw) < mx
    return adj


def find_comps(adj):
    """findComps + dfs (:138-163), the recursion made iterative: the same
    visiting order, so each component lists its members in DFS pre-order and
    the components come in order of their smallest member."""
    n = len(adj)
    used = np.zeros(n, bool)
    comps = []
    for start in range(n):
        if used[start]:
            continue
        comp = [start]
        used[start] = True
        stack = [(start, iter(np.nonzero(adj[start])[0]))]
        while stack:
            node, it = stack[-1]
            for to in it:
                if not used[to]:
                    used[to] = True
                    comp.append(int(to))
                    stack.append((int(to), iter(np.nonzero(adj[to])[0])))
                    break
            else:
                stack.pop()
        comps.append(comp)
    return comps


def clusterize(points, colors, max_distance, euclid_weight, color_weight):
    """clusterizePoints: comps in the reference's order (members in DFS pre-order)"""
    return find_comps(edge_matrix(points, colors, max_distance, euclid_weight, color_weight))


def canonical(comps):
    """components as sorted member lists ordered by first member: what a
    clustering is compared by (only the order inside a component may differ)"""
    out = [sorted(int(i) for i in c) for c in comps]
    out.sort(key=lambda c: c[0])
    return out


def project_to_plane(points, centroid, normal):
    """projectPointOnPlane + makeMesh:56-63 per point -> n x 2 float32 (x, z)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(centroid, np.float32).reshape(3)
    nr = np.ascontiguousarray(normal, np.float64).reshape(3)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = p - c[None, :]                                    # float - float
        assert d.dtype == np.float32
        num = d[:, 0].astype(np.float64) * nr[0] + d[:, 1].astype(np.float64) * nr[1] + d[:, 2].astype(np.float64) * nr[2]
        den = nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]
        x = num / den
        q = np.stack([(p[:, k].astype(np.float64) - nr[k] * x).astype(np.float32) for k in range(3)], 1)
        q = q - c[None, :]                                    # Point3f - Point3f
        assert q.dtype == np.float32
        q = q.astype(np.float64)
        coef = np.sqrt(q[:, 1] * q[:, 1] / (q[:, 0] * q[:, 0] + q[:, 2] * q[:, 2]) + 1.0)
        return np.stack([(q[:, 0] * coef).astype(np.float32), (q[:, 2] * coef).astype(np.float32)], 1)


def plane_moments(points):
    """(mean f64[3], 3 x 3 second-moment matrix of the points about it)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    mean = p.mean(0)
    d = p - mean
    return mean, d.T @ d


def fit_plane(points):
    """(centroid float32[3], unit normal float64[3]): the eigenvector of the
    smallest eigenvalue, its largest-magnitude component positive"""
    mean, m = plane_moments(points)
    w, v = np.linalg.eigh(m)
    nrm = v[:, 0].copy()
    if nrm[np.argmax(np.abs(nrm))] < 0:
        nrm = -nrm
    return mean.astype(np.float32), nrm


def clustered_cloud(n, seed=7, blobs=40, sigma=0.08, box=5.0):
    """n points in `blobs` Gaussian blobs (sigma) with centres in a +-box cube,
    each blob with a palette colour of its own +-3, indices shuffled"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-box, box, (blobs, 3))
    palette = rng.integers(8, 248, (blobs, 3))
    which = rng.integers(0, blobs, n)
    pts = (centres[which] + rng.normal(0.0, sigma, (n, 3))).astype(np.float32)
    cols = (palette[which] + rng.integers(-3, 4, (n, 3))).astype(np.uint8)
    perm = rng.permutation(n)
    return pts[perm], cols[perm]

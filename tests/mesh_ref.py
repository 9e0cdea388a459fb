"""Exact restatement of the meshing contract (csrc/delaunay.hip),
the yardstick of tests/test_mesh.py and tests/test_mesh_gpu.py (our own text):

  orient2d / incircle / closer   exact signs with fractions.Fraction
  delaunay_ref                   the star walk with the cocircular tie rule, O(n^2)
  check_delaunay                 an O(T) verifier for any n
  mesh_filter                    makeMesh's edge-length filter (bestFittingPlane.cpp:96-111)
  parse_ply                      reads back what scene.write_mesh wrote

Every f32 coordinate is an exact rational with a power-of-two denominator.
delaunay_ref and check_delaunay scale all coordinates of one input by their
common denominator (found with Fraction) so that the predicates run on Python
integers: the same exact values, about ten times faster than Fraction objects.
"""
import math
from fractions import Fraction

import numpy as np

RANGE = 100000.0          # Subdiv2D(Rect(-100000, -100000, 200000, 200000)): x, y in [-RANGE, RANGE)


def _sign(v):
    return (v > 0) - (v < 0)


def orient2d(a, b, c):
    """exact sign of the turn a -> b -> c: +1 counter-clockwise (c strictly left of a -> b)"""
    return _sign((a[0] - c[0]) * (b[1] - c[1]) - (a[1] - c[1]) * (b[0] - c[0]))


def incircle(a, b, c, d):
    """exact sign: +1 iff d is strictly inside the circle through the counter-clockwise a, b, c"""
    adx, ady = a[0] - d[0], a[1] - d[1]
    bdx, bdy = b[0] - d[0], b[1] - d[1]
    cdx, cdy = c[0] - d[0], c[1] - d[1]
    return _sign((adx * adx + ady * ady) * (bdx * cdy - cdx * bdy)
                 + (bdx * bdx + bdy * bdy) * (cdx * ady - adx * cdy)
                 + (cdx * cdx + cdy * cdy) * (adx * bdy - bdx * ady))


def closer(a, p, q):
    """exact sign of |p - a|^2 - |q - a|^2: -1 iff p is strictly nearer to a than q"""
    px, py, qx, qy = p[0] - a[0], p[1] - a[1], q[0] - a[0], q[1] - a[1]
    return _sign(px * px + py * py - qx * qx - qy * qy)


def fractions_of(xy):
    """n x 2 float32 -> list of (Fraction, Fraction), the exact values"""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    return [(Fraction(float(x)), Fraction(float(y))) for x, y in xy]


def exact_ints(xy):
    """the points scaled by the common (power of two) denominator: exact integers"""
    fr = fractions_of(xy)
    den = 1
    for x, y in fr:
        den = max(den, x.denominator, y.denominator)      # powers of two: the largest is the lcm
    return [(int(x * den), int(y * den)) for x, y in fr]


def in_range(xy):
    """the component is meshed at all: every coordinate finite and in [-RANGE, RANGE)"""
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        return bool((np.isfinite(xy) & (xy >= -RANGE) & (xy < RANGE)).all())


def vertices(xy):
    """indices i with no j < i at the same coordinates (float ==, so -0.0 == 0.0)"""
    seen, out = set(), []
    for i, p in enumerate(exact_ints(xy)):
        if p not in seen:
            seen.add(p)
            out.append(i)
    return out


def _apex(P, V, a, b):
    """the contract's apex of the directed edge (a, b), or -1 on the hull"""
    pa, pb = P[a], P[b]
    cand = [p for p in V if orient2d(pa, pb, P[p]) > 0]
    if not cand:
        return -1
    c = cand[0]
    for p in cand[1:]:
        if incircle(pa, pb, P[c], P[p]) > 0:
            c = p
    T = [p for p in cand if p == c or incircle(pa, pb, P[c], P[p]) == 0]
    if len(T) == 1:
        return c
    m = min(T + [a, b])
    if m in T:
        return m
    if m == a:
        win = [t for t in T if all(u == t or orient2d(pb, P[t], P[u]) > 0 for u in T)]
    else:
        win = [t for t in T if all(u == t or orient2d(P[t], pa, P[u]) > 0 for u in T)]
    assert len(win) == 1
    return win[0]


def canonical(tris):
    """each triangle rotated to start at its smallest index, the list sorted"""
    out = []
    for t in tris:
        t = [int(v) for v in t]
        k = t.index(min(t))
        out.append((t[k], t[(k + 1) % 3], t[(k + 2) % 3]))
    out.sort()
    return np.array(out, np.int32).reshape(-1, 3)


def delaunay_ref(xy):
    """the contract: every vertex walks its own star from its nearest neighbour;
    triangle (a, b, c) is kept by its smallest index.  (T, 3) int32, canonical."""
    P = exact_ints(xy)
    V = vertices(xy)
    tris = []
    for a in V:
        b0 = -1
        for p in V:
            if p != a and (b0 < 0 or closer(P[a], P[p], P[b0]) < 0):
                b0 = p
        if b0 < 0:
            continue
        b, closed = b0, False
        for _ in range(len(V)):
            c = _apex(P, V, a, b)
            if c < 0:
                break
            if a < b and a < c:
                tris.append((a, b, c))
            if c == b0:
                closed = True
                break
            b = c
        else:
            raise AssertionError("the walk did not end")
        if closed:
            continue
        cc = b0
        for _ in range(len(V)):
            c = _apex(P, V, cc, a)
            if c < 0:
                break
            if a < c and a < cc:
                tris.append((a, c, cc))
            cc = c
        else:
            raise AssertionError("the walk did not end")
    return canonical(tris)


def check_delaunay(xy, tris):
    """raise AssertionError unless tris is the canonical list of a complete
    Delaunay triangulation of the vertices of xy.  O(T) exact predicates."""
    P = exact_ints(xy)
    V = vertices(xy)
    tris = np.asarray(tris)
    assert tris.ndim == 2 and tris.shape[1] == 3 and tris.dtype == np.int32
    T = [tuple(int(v) for v in t) for t in tris]
    hull_only = len(V) < 3 or all(orient2d(P[V[0]], P[V[1]], P[v]) == 0 for v in V[2:])
    if hull_only:
        assert len(T) == 0, "fewer than 3 vertices, or all collinear: no triangles"
        return
    assert len(T) > 0, "no triangles for vertices that span the plane"
    vset = set(V)
    assert T == sorted(T), "not in lexicographic order"
    edge = {}
    used = set()
    area2 = 0
    for t in T:
        i, j, k = t
        assert i < j and i < k and j != k, f"{t}: the smallest index does not lead"
        assert i in vset and j in vset and k in vset, f"{t}: names a point that is no vertex"
        o = (P[i][0] - P[k][0]) * (P[j][1] - P[k][1]) - (P[i][1] - P[k][1]) * (P[j][0] - P[k][0])
        assert o > 0, f"{t}: not strictly counter-clockwise"
        area2 += o
        for u, v, w in ((i, j, k), (j, k, i), (k, i, j)):
            assert (u, v) not in edge, f"directed edge {(u, v)} twice"
            edge[(u, v)] = w
        used.update(t)
    assert used == vset, f"vertices without a triangle: {sorted(vset - used)[:5]}"
    # boundary: directed edges whose reverse is absent; one cycle that never turns right
    nxt = {}
    for (u, v), w in edge.items():
        if (v, u) in edge:
            assert incircle(P[u], P[v], P[w], P[edge[(v, u)]]) <= 0, f"edge {(u, v)}: opposite vertex inside"
        else:
            assert u not in nxt, f"boundary vertex {u} has two outgoing edges"
            nxt[u] = v
    start = min(nxt)
    cycle, u = [start], nxt[start]
    while u != start:
        assert u in nxt and len(cycle) <= len(nxt), "boundary is not a cycle"
        cycle.append(u)
        u = nxt[u]
    assert len(cycle) == len(nxt), "boundary has more than one cycle"
    m = len(cycle)
    poly2 = 0
    for q in range(m):
        a, b, c = P[cycle[q]], P[cycle[(q + 1) % m]], P[cycle[(q + 2) % m]]
        assert orient2d(a, b, c) >= 0, "boundary turns right"
        poly2 += a[0] * b[1] - a[1] * b[0]
    assert poly2 == area2, "triangles do not tile the boundary polygon"


def mesh_filter(points, tris, max_size=10000.0):
    """makeMesh:96-111: drop a triangle when any 3-D edge is longer than max_size
    (distance(Point3f, Point3f): f32 differences, squares summed in f64, strict >)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    keep = np.ones(len(tris), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for u, v in ((0, 1), (1, 2), (2, 0)):
            d = p[tris[:, u]] - p[tris[:, v]]
            assert d.dtype == np.float32
            d = d.astype(np.float64)
            keep &= ~(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) > max_size)
    return tris[keep]


def parse_ply(path):
    """(points n x 3, colours n x 3 as red green blue, faces as rows '3 i j k') of an ASCII PLY"""
    with open(path) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    head = lines[:end]
    assert head[0] == "ply" and head[1] == "format ascii 1.0"
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[2])
    nf = int([h for h in head if h.startswith("element face")][0].split()[2])
    props = [h.split()[-1] for h in head if h.startswith("property") and "list" not in h]
    assert props == ["x", "y", "z", "red", "green", "blue"]
    body = [ln for ln in lines[end + 1:] if ln]
    assert len(body) == nv + nf
    verts = np.array([ln.split() for ln in body[:nv]], np.float64).reshape(-1, 6)
    faces = np.array([ln.split() for ln in body[nv:]], np.int64).reshape(-1, 4)
    return verts[:, :3], verts[:, 3:].astype(np.uint8), faces


# ---- fixtures shared by the CPU and the GPU tests ------------------------------------------

def uniform(n, seed=None):
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    return rng.uniform(-50, 50, (n, 2)).astype(np.float32)


def grid(w=6, h=5, seed=3):
    g = np.array([(x, y) for y in range(h) for x in range(w)], np.float32)
    return g[np.random.default_rng(seed).permutation(len(g))]


def circle12():
    """the 12 integer points on the circle of radius 5 about the origin, shuffled"""
    c = np.array([(x, y) for x in range(-5, 6) for y in range(-5, 6) if x * x + y * y == 25], np.float32)
    assert len(c) == 12
    return c[np.random.default_rng(5).permutation(12)]


def circle12_centre():
    return np.concatenate([circle12()[:7], np.zeros((1, 2), np.float32), circle12()[7:]])


def circle12_around(seed=11):
    """the circle scaled by 5 around 20 inner points"""
    inner = np.random.default_rng(seed).uniform(-8, 8, (20, 2)).astype(np.float32)
    pts = np.concatenate([circle12() * np.float32(5), inner])
    return pts[np.random.default_rng(seed + 1).permutation(len(pts))]


def circle_nudged(seed=13):
    """8 concentric copies of the circle plus 4 inner points (n = 100), every
    coordinate moved by one ulp up or down: nearly cocircular everywhere"""
    rng = np.random.default_rng(seed)
    rings = np.concatenate([circle12() * np.float32(s) for s in (1, 2, 3, 4, 5, 6, 7, 8)])
    pts = np.concatenate([rings, rng.uniform(-2, 2, (4, 2)).astype(np.float32)])
    up = rng.integers(0, 2, pts.shape).astype(bool)
    return np.where(up, np.nextafter(pts, np.float32(np.inf)), np.nextafter(pts, np.float32(-np.inf))).astype(np.float32)


def duplicates(seed=17):
    """40 points, 10 repeats of some of them, then (0, 0) and (-0, 0)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-10, 10, (40, 2)).astype(np.float32)
    rep = p[rng.integers(0, 40, 10)]
    return np.concatenate([p, rep, np.array([[0.0, 0.0], [-0.0, 0.0]], np.float32)])


def collinear(n=10):
    t = np.random.default_rng(19).permutation(n).astype(np.float32)
    return np.stack([t, np.float32(2) * t + np.float32(1)], 1)      # exact in f32


def collinear_plus_one():
    return np.concatenate([collinear(), np.array([[3.5, -4.0]], np.float32)])


# ---- adversarial sets: more tie members than lanes, tile-crossing duplicates, the ends of
# ---- the coordinate range, triangle counts at the sort's powers of two

def _shuffled(pts, seed):
    pts = np.ascontiguousarray(pts, np.float32)
    return pts[np.random.default_rng(seed).permutation(len(pts))]


def lattice_circle(R=1105, seed=7):
    """every integer point on the circle of radius R about the origin, shuffled.
    1105 = 5 * 13 * 17: 108 points (32045 = 5 * 13 * 17 * 29: 324), exact in f32:
    more cocircular vertices than a wave has lanes, one fan of len - 2 triangles"""
    c = set()
    for x in range(-R, R + 1):
        y = math.isqrt(R * R - x * x)
        if x * x + y * y == R * R:
            c.update([(x, y), (x, -y)])
    c = sorted(c)
    assert R < 2 ** 24
    return _shuffled(c, seed)


def lattice_circle_centre(R=1105, seed=7):
    """the origin inserted at index 50: every circle point has an edge to it"""
    c = lattice_circle(R, seed)
    return np.concatenate([c[:50], np.zeros((1, 2), np.float32), c[50:]])


def lattice_circle_around(R=1105, seed=7):
    """the circle around 40 inner points, uniform in +-500"""
    inner = np.random.default_rng(seed + 100).uniform(-500, 500, (40, 2)).astype(np.float32)
    return _shuffled(np.concatenate([lattice_circle(R, seed), inner]), seed + 200)


def grid272():
    """17 x 16: four-point ties everywhere, across the 256-point tile of the pre-pass"""
    return grid(17, 16)


def near_9e4():
    """300 points on the 2^-7 lattice next to 90000 (formed in f32): duplicates,
    collinear runs, cocircular quadruples, lifted terms near 1e20"""
    xy = uniform(300) * np.float32(0.002) + np.float32(90000)
    assert xy.dtype == np.float32
    return xy


def full_range():
    """200 points over nearly all of [-100000, 100000)"""
    xy = uniform(200, seed=5) * np.float32(1999.9)
    assert xy.dtype == np.float32
    return xy


def mixed_magnitudes(seed=29):
    """130 points: 60 of order 1e-30, 30 small integer multiples of the smallest
    f32 subnormal, 40 uniform in +-9e4, shuffled"""
    rng = np.random.default_rng(seed)
    tiny = (rng.uniform(-5, 5, (60, 2)) * 1e-30).astype(np.float32)
    sub = (rng.integers(-20, 20, (30, 2)).astype(np.int64).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    assert (sub.astype(np.float64) * 2.0 ** 149 == np.round(sub.astype(np.float64) * 2.0 ** 149)).all()
    big = rng.uniform(-9e4, 9e4, (40, 2)).astype(np.float32)
    return _shuffled(np.concatenate([tiny, sub, big]), seed + 1)


def dups650(seed=31):
    """400 points and 250 copies drawn from them, shuffled: three pre-pass tiles"""
    p = uniform(400)
    rng = np.random.default_rng(seed)
    return _shuffled(np.concatenate([p, p[rng.integers(0, 400, 250)]]), seed + 1)


def dups_tile_edges():
    """640 points with four copies, each with its first occurrence in an earlier
    256-point tile of the pre-pass: the last point of the tile before, the first
    point of the first tile, a third copy two tiles back, and mid-tile to the end"""
    xy = uniform(640).copy()
    xy[256] = xy[255]
    xy[511] = xy[0]
    xy[512] = xy[256]
    xy[639] = xy[300]
    return xy


def hull3(n):
    """n - 3 points inside a triangle and its corners: 2 n - 5 triangles (Euler)"""
    return np.concatenate([uniform(n - 3), np.array([[0, 300], [-300, -100], [300, -100]], np.float32)])


def hull4(n):
    """n - 4 points inside a square and its corners: 2 n - 6 triangles"""
    return np.concatenate([uniform(n - 4), np.array([[-300, -300], [300, -300], [300, 300], [-300, 300]], np.float32)])


# (name, maker, what the device counters must show: "ties" = ties > 0 and exact > 0, "exact", None)
ADVERSARIAL = [
    ("lattice_circle_s7", lambda: lattice_circle(seed=7), "ties"),
    ("lattice_circle_s8", lambda: lattice_circle(seed=8), "ties"),
    ("lattice_circle_centre_s7", lambda: lattice_circle_centre(seed=7), "ties"),
    ("lattice_circle_centre_s8", lambda: lattice_circle_centre(seed=8), "ties"),
    ("lattice_circle_around_s7", lambda: lattice_circle_around(seed=7), "ties"),
    ("lattice_circle_around_s8", lambda: lattice_circle_around(seed=8), "ties"),
    ("lattice_circle_32045", lambda: lattice_circle(32045, seed=9), "ties"),
    ("grid272", grid272, "ties"),
    ("near_9e4", near_9e4, "ties"),
    ("full_range", full_range, None),
    ("mixed_magnitudes", mixed_magnitudes, "exact"),
    ("dups650", dups650, None),
    ("dups_tile_edges", dups_tile_edges, None),
]
HULL_COUNTS = [(hull3, 130, 255), (hull3, 131, 257), (hull3, 259, 513), (hull4, 131, 256), (hull4, 259, 512)]

_REF_CACHE = {}


def cached_ref(name, make):
    """(xy, delaunay_ref(xy)) of a named fixture, computed once per process; treat both as read-only"""
    if name not in _REF_CACHE:
        xy = make()
        ref = delaunay_ref(xy)
        xy.setflags(write=False)
        ref.setflags(write=False)
        _REF_CACHE[name] = (xy, ref)
    return _REF_CACHE[name]

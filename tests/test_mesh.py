"""CPU tests of the meshing stage's yardstick (tests/mesh_ref.py) and of its host
code: the exact reference against scipy's qhull, the verifier against broken
triangulations, slam_mesh_filter, scene.write_mesh and scene.make_mesh's skip
rule.  The kernel itself is tested in tests/test_mesh_gpu.py."""
import numpy as np
import pytest

import mesh_ref as M
from slamhip import api, scene

F32 = np.float32


def scipy_delaunay(xy):
    """scipy.spatial.Delaunay's simplices, canonical"""
    spatial = pytest.importorskip("scipy.spatial")
    p = np.asarray(xy, np.float64)
    tris = []
    for a, b, c in spatial.Delaunay(p).simplices:
        ccw = M.orient2d(*M.fractions_of(np.asarray(xy)[[a, b, c]])) > 0
        tris.append((a, b, c) if ccw else (a, c, b))
    return M.canonical(tris)


def dedup(xy):
    """the vertices only, with the map back to the input's indices (qhull has
    no first-duplicate rule)"""
    v = np.array(M.vertices(xy))
    return np.asarray(xy)[v], v


@pytest.mark.parametrize("n", [3, 4, 5, 17, 64, 65, 150])
def test_ref_equals_scipy_on_uniform_points(n):
    xy = M.uniform(n)
    ref = M.delaunay_ref(xy)
    M.check_delaunay(xy, ref)
    assert np.array_equal(ref, scipy_delaunay(xy))


def test_ref_equals_scipy_on_duplicates_and_collinear_plus_one():
    xy = M.duplicates()
    v_xy, v = dedup(xy)
    assert len(v) < len(xy) - 10                      # the repeats and -0.0 are dropped
    ref = M.delaunay_ref(xy)
    M.check_delaunay(xy, ref)
    assert np.array_equal(ref, M.canonical(v[scipy_delaunay(v_xy)]))
    xy = M.collinear_plus_one()
    ref = M.delaunay_ref(xy)
    M.check_delaunay(xy, ref)
    assert len(ref) == 9 and np.array_equal(ref, scipy_delaunay(xy))
    assert len(M.delaunay_ref(M.collinear())) == 0
    M.check_delaunay(M.collinear(), np.zeros((0, 3), np.int32))


DEGENERATE = [M.grid, M.circle12, M.circle12_centre, M.circle12_around]


@pytest.mark.parametrize("make", DEGENERATE, ids=lambda f: f.__name__)
def test_verifier_accepts_the_reference_on_degenerate_sets(make):
    xy = make()
    ref = M.delaunay_ref(xy)
    M.check_delaunay(xy, ref)
    # the fan rule: a cocircular polygon's triangles all share its lowest-indexed vertex
    if make is M.circle12:
        assert len(ref) == 10 and (ref[:, 0] == 0).all()
    # and it does not depend on the order of the points beyond their indices: a
    # second build gives the same bytes
    assert ref.tobytes() == M.delaunay_ref(xy).tobytes()


def flip_one_interior_edge(xy, tris):
    """the same triangulation with the first flippable, strictly non-Delaunay-
    after-flip interior edge flipped, canonical again"""
    P = M.exact_ints(xy)
    T = [tuple(int(v) for v in t) for t in tris]
    edge = {}
    for t in T:
        for q in range(3):
            edge[(t[q], t[(q + 1) % 3])] = (t, t[(q + 2) % 3])
    for (u, v), (t1, w) in sorted(edge.items()):
        if (v, u) not in edge:
            continue
        t2, z = edge[(v, u)]
        # the quadrilateral u, z, v, w must be strictly convex, and the flip must break the empty circle
        if M.orient2d(P[w], P[z], P[v]) > 0 and M.orient2d(P[z], P[w], P[u]) > 0 \
                and M.incircle(P[u], P[v], P[w], P[z]) < 0:
            rest = [t for t in T if t not in (t1, t2)]
            return M.canonical(rest + [(w, z, v), (z, w, u)])
    raise AssertionError("no flippable edge")


@pytest.mark.parametrize("make", [lambda: M.uniform(64), M.circle12_around], ids=["uniform64", "circle12_around"])
def test_verifier_rejects_broken_triangulations(make):
    xy = make()
    ref = M.delaunay_ref(xy)
    M.check_delaunay(xy, ref)
    with pytest.raises(AssertionError, match="opposite vertex inside"):
        M.check_delaunay(xy, flip_one_interior_edge(xy, ref))
    with pytest.raises(AssertionError):
        M.check_delaunay(xy, np.delete(ref, len(ref) // 2, 0))                  # one triangle removed
    with pytest.raises(AssertionError):
        M.check_delaunay(xy, np.insert(ref, 3, ref[3], 0))                      # one duplicated
    with pytest.raises(AssertionError, match="order"):
        M.check_delaunay(xy, ref[::-1].copy())
    with pytest.raises(AssertionError):
        M.check_delaunay(xy, ref[:, [0, 2, 1]].copy())                          # clockwise


HOST_SETS = [M.grid, M.circle12, M.circle12_centre, M.circle12_around, M.circle_nudged, M.duplicates, M.collinear,
             M.collinear_plus_one] + [lambda n=n: M.uniform(n) for n in (0, 1, 2, 3, 4, 5, 17, 63, 64, 150)]


@pytest.mark.parametrize("make", HOST_SETS, ids=lambda f: getattr(f, "__name__", "uniform"))
def test_host_entry_equals_the_reference(make):
    """slam_delaunay_2d_host: the path scene.make_mesh takes below 64 points; it
    shares exact_pred.h and the tie rule with the kernel"""
    xy = make()
    got = api.delaunay2dHost(xy)
    ref = M.delaunay_ref(xy)
    assert got.dtype == np.int32 and got.shape == ref.shape and got.tobytes() == ref.tobytes()


@pytest.mark.parametrize("name,make,_", M.ADVERSARIAL, ids=[a[0] for a in M.ADVERSARIAL])
def test_host_entry_equals_the_reference_on_adversarial_sets(name, make, _):
    """the sets of tests/test_mesh_gpu.py, so that the fixtures, the reference's
    own tie rule (its assert len(win) == 1) and the host twin are checked
    where there is no device"""
    xy, ref = M.cached_ref(name, make)
    assert M.in_range(xy)
    M.check_delaunay(xy, ref)
    got = api.delaunay2dHost(xy)
    assert got.dtype == np.int32 and got.shape == ref.shape and got.tobytes() == ref.tobytes()
    if name.startswith("lattice_circle_s") or name == "lattice_circle_32045":
        assert len(xy) in (108, 324) and len(ref) == len(xy) - 2 and (ref[:, 0] == 0).all()     # one fan from vertex 0
    if name.startswith("dups"):
        assert len(M.vertices(xy)) < len(xy) and set(got.ravel().tolist()) == set(M.vertices(xy))


@pytest.mark.parametrize("make,n,count", M.HULL_COUNTS, ids=[f"{f.__name__}_{n}" for f, n, _ in M.HULL_COUNTS])
def test_host_entry_at_power_of_two_triangle_counts(make, n, count):
    xy, ref = M.cached_ref(f"{make.__name__}_{n}", lambda: make(n))
    assert len(xy) == n and len(ref) == count                      # Euler: the fixture proves itself
    M.check_delaunay(xy, ref)
    got = api.delaunay2dHost(xy)
    assert got.dtype == np.int32 and got.shape == ref.shape and got.tobytes() == ref.tobytes()


def test_host_entry_status_codes():
    import ctypes
    from slamhip import _lib as L
    lib = L.lib()
    xy = M.uniform(17)
    ref = M.delaunay_ref(xy)
    tris = np.zeros((len(ref), 3), np.int32)
    nt = ctypes.c_int(-1)
    assert lib.slam_delaunay_2d_host(L.ptr(xy), 17, L.ptr(tris), len(ref) - 1, ctypes.byref(nt)) == L.SLAM_E_CAPACITY
    assert nt.value == len(ref)
    assert lib.slam_delaunay_2d_host(L.ptr(xy), 17, L.ptr(tris), len(ref), ctypes.byref(nt)) == L.SLAM_OK
    assert nt.value == len(ref) and np.array_equal(tris, ref)
    for bad in (np.nan, np.inf, 100000.0):
        b = xy.copy()
        b[3, 1] = bad
        assert lib.slam_delaunay_2d_host(L.ptr(b), 17, L.ptr(tris), len(ref), ctypes.byref(nt)) == L.SLAM_E_INVALID_ARG
        assert nt.value == 0
        with pytest.raises(L.SlamError):
            api.delaunay2dHost(b)
    b = xy.copy()
    b[3] = (-100000.0, 5.0)
    M.check_delaunay(b, api.delaunay2dHost(b))
    assert lib.slam_delaunay_2d_host(None, 0, None, 0, ctypes.byref(nt)) == L.SLAM_OK and nt.value == 0
    assert lib.slam_delaunay_2d_host(None, 3, None, 0, ctypes.byref(nt)) == L.SLAM_E_INVALID_ARG


def test_make_mesh_of_a_small_component_runs_on_the_host():
    rng = np.random.default_rng(8)
    xy = rng.uniform(-3, 3, (40, 2)).astype(F32)
    pts = np.stack([xy[:, 0], np.zeros(40, F32), xy[:, 1]], 1)
    pts[7] = (20000.0, 0.0, 0.0)                                   # its edges are longer than 10000
    xy[7] = (20000.0, 0.0)
    seg = scene.Segment(np.arange(100, 140, dtype=np.int32), pts, np.zeros((40, 3), np.uint8), xy)
    m = scene.make_mesh(seg)
    full = M.delaunay_ref(xy)
    want = M.mesh_filter(pts, full)
    assert 0 < len(want) < len(full) and 7 not in want
    assert np.array_equal(m.triangles, want) and np.array_equal(m.faces, want + 100)


def test_mesh_filter_is_strict_at_10000():
    up = float(np.nextafter(F32(10000), F32(np.inf)))
    pts = np.array([[0, 0, 0], [10000, 0, 0], [5000, 1, 0],        # edge 0-1 exactly 10000: kept
                    [0, 0, 5], [up, 0, 5], [5000, 1, 5],           # edge 3-4 one ulp above: dropped
                    [0, 6000, 8000], [0, 3000, 4000]], F32)        # |(0, 6000, 8000)| = 10000 exactly
    tris = np.array([[0, 1, 2], [3, 4, 5], [0, 7, 6], [3, 5, 4], [0, 6, 7]], np.int32)
    ref = M.mesh_filter(pts, tris)
    assert ref.tolist() == [[0, 1, 2], [0, 7, 6], [0, 6, 7]]
    got = api.meshFilter(pts, tris)
    assert got.dtype == np.int32 and np.array_equal(got, ref)      # the order is kept
    assert api.meshFilter(pts, tris, max_size=9999.5).tolist() == []
    assert api.meshFilter(pts, np.zeros((0, 3), np.int32)).shape == (0, 3)
    # f32 differences: 16777216 - 0.5 rounds to 16777216 (distance(Point3f, Point3f))
    big = np.array([[16777216, 0, 0], [0.5, 0, 0], [0, 1, 0]], F32)
    one = np.array([[0, 1, 2]], np.int32)
    assert api.meshFilter(big, one, max_size=16777215.75).tolist() == M.mesh_filter(big, one, 16777215.75).tolist() == []
    with pytest.raises(Exception):
        api.meshFilter(pts, np.array([[0, 1, 8]], np.int32))       # an index outside the points


def test_write_mesh_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    pts = rng.normal(0, 3, (50, 3))
    cols = rng.integers(0, 256, (50, 3)).astype(np.uint8)
    m1 = scene.Mesh(np.array([[0, 1, 2]], np.int32), np.array([[7, 9, 11]], np.int32))
    m2 = scene.Mesh(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.int32))
    m3 = scene.Mesh(np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.array([[20, 21, 22], [20, 22, 49]], np.int32))
    path = str(tmp_path / "mesh.ply")
    scene.write_mesh(pts, cols, [m1, None, m2, m3], path)
    v, c, f = M.parse_ply(path)
    assert np.array_equal(v.astype(F32), pts.astype(F32))           # repr of the f32 value round-trips
    assert np.array_equal(c, cols[:, ::-1])                          # Vec3b is blue-green-red
    assert f.tolist() == [[3, 7, 9, 11], [3, 20, 21, 22], [3, 20, 22, 49]]
    scene.write_mesh(pts, cols, [], path)
    assert M.parse_ply(path)[2].shape == (0, 4)
    with pytest.raises(ValueError):
        scene.write_mesh(pts, cols[:-1], [], path)


def segment_of(xy):
    n = len(xy)
    return scene.Segment(np.arange(10, 10 + n, dtype=np.int32), np.zeros((n, 3), F32), np.zeros((n, 3), np.uint8),
                         np.asarray(xy, F32))


def test_make_mesh_skips_what_subdiv2d_rejects():
    """decided on the host before any launch, so this runs without a device"""
    ok = [[0, 0], [1, 0], [0, 1], [5, 5]]
    for bad in ([np.nan, 0], [0, np.inf], [-np.inf, 0], [100000, 0], [0, 100000],
                [float(np.nextafter(F32(-100000), F32(-np.inf))), 0]):
        assert scene.make_mesh(segment_of(ok + [bad])) is None
        assert scene.make_mesh(segment_of([bad])) is None
        assert not M.in_range(np.array(ok + [bad], F32))
    # -100000 is inside the rectangle, and so is the last f32 below 100000
    edge = [[-100000, float(np.nextafter(F32(100000), F32(0)))]]
    assert M.in_range(np.array(edge, F32))
    m = scene.make_mesh(segment_of(edge + [[0, -100000]]))
    assert m is not None and m.triangles.shape == (0, 3) and m.faces.shape == (0, 3)      # fewer than 3 points
    assert scene.mesh([segment_of([[np.nan, 0]]), segment_of(edge)])[0] is None

"""GPU tests of the scene post-processing (csrc/cluster.hip): every result is
compared with tests/scene_ref.py, the numpy restatement of the reference.
Clusterings are compared as the list of sorted components ordered by first
member, which must be identical; projections bit for bit."""
import ctypes

import numpy as np
import pytest

import scene_ref as R
import slamhip
from slamhip import _lib as L
from slamhip import api

pytestmark = pytest.mark.gpu

F32 = np.float32
T = 256                                   # cluster.hip's tile: points per workgroup
UP5 = float(np.nextafter(F32(5), F32(np.inf)))


def gpu_comps(ctx, pts, cols, prm):
    return [c.tolist() for c in slamhip.clusterizePoints(pts, cols, prm, ctx=ctx)]


def check_cluster(ctx, pts, cols, prm):
    """prm = (max, euclid weight, colour weight); returns the reference components"""
    ref = R.canonical(R.clusterize(pts, cols, *prm))
    got = gpu_comps(ctx, pts, cols, prm)
    assert got == ref
    labels, nc = api.clusterLabels(pts, cols, prm, ctx=ctx)
    assert nc == len(ref)
    for comp in ref:
        assert (labels[comp] == comp[0]).all()        # label = the smallest index of the component
    return ref


def scattered(n, seed):
    """n points, dense enough that components of many sizes form at max = 0.6"""
    rng = np.random.default_rng(seed)
    side = max(1.0, (n / 3.0) ** (1.0 / 3.0))
    return rng.uniform(0, side, (n, 3)).astype(F32), rng.integers(0, 256, (n, 3)).astype(np.uint8)


@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 2 * T + 1])
def test_cluster_sizes_around_the_tile_edge(gpu_ctx, n):
    pts, cols = scattered(n, n)
    ref = check_cluster(gpu_ctx, pts, cols, (0.6, 1.0, 0.0005))
    if n >= T - 1:
        sizes = [len(c) for c in ref]
        assert max(sizes) >= 3 and min(sizes) == 1 and len(ref) > 10     # a fixture with structure


@pytest.fixture(scope="module")
def cloud():
    return R.clustered_cloud(1500)


@pytest.mark.parametrize("prm", [(0.25, 1.0, 0.02), (0.15, 1.0, 0.0)])
def test_cluster_clustered_cloud(gpu_ctx, cloud, prm):
    pts, cols = cloud
    ref = R.canonical(R.clusterize(pts, cols, *prm))
    sizes = np.array([len(c) for c in ref])
    assert (sizes >= 3).sum() >= 30 and (sizes == 1).sum() >= 1          # no vacuous pass
    assert gpu_comps(gpu_ctx, pts, cols, prm) == ref


def test_cluster_chain_across_every_tile(gpu_ctx):
    rng = np.random.default_rng(21)
    x = rng.permutation(1000).astype(F32)
    pts = np.stack([x, np.zeros(1000, F32), np.zeros(1000, F32)], 1)
    cols = np.full((1000, 3), 9, np.uint8)
    ref = check_cluster(gpu_ctx, pts, cols, (1.5, 1.0, 1.0))
    assert len(ref) == 1
    # the same chain cut in the middle: two components
    pts[x >= 500, 0] += 1
    assert len(check_cluster(gpu_ctx, pts, cols, (1.5, 1.0, 1.0))) == 2


def test_cluster_blob_of_identical_points(gpu_ctx):
    pts = np.full((1000, 3), 1.25, F32)
    cols = np.full((1000, 3), 200, np.uint8)
    got = gpu_comps(gpu_ctx, pts, cols, (0.5, 1.0, 1.0))
    assert got == [list(range(1000))]
    pairs, exact = ctypes.c_uint64(0), ctypes.c_uint64(0)
    L.check(slamhip.lib().slam_cluster_last_stats(gpu_ctx.handle, ctypes.byref(pairs), ctypes.byref(exact)),
            gpu_ctx.handle)
    assert pairs.value == 1000 * 999 // 2 and exact.value == pairs.value   # every pair once


def test_cluster_borderline_345(gpu_ctx):
    pts = np.array([[0, 0, 0], [3, 4, 0]], F32)
    zero = np.zeros((2, 3), np.uint8)
    assert gpu_comps(gpu_ctx, pts, zero, (5.0, 1.0, 0.0)) == [[0], [1]]
    assert gpu_comps(gpu_ctx, pts, zero, (UP5, 1.0, 0.0)) == [[0, 1]]
    same = np.ones((2, 3), F32)
    cols = np.array([[10, 20, 30], [13, 16, 30]], np.uint8)
    assert gpu_comps(gpu_ctx, same, cols, (5.0, 1.0, 1.0)) == [[0], [1]]
    assert gpu_comps(gpu_ctx, same, cols, (UP5, 1.0, 1.0)) == [[0, 1]]


def test_cluster_arithmetic_cases(gpu_ctx):
    zero = np.zeros((2, 3), np.uint8)
    # the difference is rounded in f32: 16777216 - 0.5 -> 16777216, not < max
    big = np.array([[16777216, 0, 0], [0.5, 0, 0]], F32)
    assert R.clusterize(big, zero, 16777216.0, 1.0, 0.0) == [[0], [1]]
    assert gpu_comps(gpu_ctx, big, zero, (16777216.0, 1.0, 0.0)) == [[0], [1]]
    # a NaN point is a singleton, the points around it still join
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [0, np.inf, 0]], F32)
    cols = np.zeros((4, 3), np.uint8)
    assert check_cluster(gpu_ctx, pts, cols, (1.0, 1.0, 1.0)) == [[0, 2], [1], [3]]
    # max = 0 (and below): no edges at all
    pts, cols = scattered(300, 5)
    pts[7] = pts[8]
    cols[7] = cols[8]
    assert len(check_cluster(gpu_ctx, pts, cols, (0.0, 1.0, 1.0))) == 300
    assert len(check_cluster(gpu_ctx, pts, cols, (-1.0, 1.0, 1.0))) == 300
    # colour weight 0 with wildly different colours: geometry alone decides
    ref = check_cluster(gpu_ctx, pts, cols, (0.6, 1.0, 0.0))
    assert ref == R.canonical(R.clusterize(pts, np.zeros_like(cols), 0.6, 1.0, 0.0)) and len(ref) < 300
    # weights the rejects do not cover (negative) and a zero distance weight
    check_cluster(gpu_ctx, pts, cols, (0.3, 1.0, -0.001))
    check_cluster(gpu_ctx, pts, cols, (0.0, -1.0, 0.0))
    check_cluster(gpu_ctx, pts, cols, (3.0, 0.0, 0.02))


def test_cluster_pairs_within_4_ulp_of_max(gpu_ctx):
    """200 random pairs whose realDistance + colorDistance (the reference's own
    f64 sum) lies within 4 ulp of max on either side.  max is an f32 config
    value, so the ulp is max's f32 ulp: max = the f32 nearest the sum moved by
    k in [-4, 4] f32 steps (k = 0 lands on either side of the sum, whichever
    way the rounding went).  A reject that drops an edge, or an inexact sqrt,
    shows here."""
    rng = np.random.default_rng(99)
    edges = 0
    for t in range(200):
        scale = 10.0 ** rng.uniform(-3, 3)
        pts = (rng.normal(0, 1, (2, 3)) * scale).astype(F32)
        cols = rng.integers(0, 256, (2, 3)).astype(np.uint8)
        dw = F32(rng.uniform(0.1, 3.0)) if t % 4 else F32(1.0)
        cw = F32(rng.uniform(0, 0.05) * scale) if t % 3 else F32(0.0)
        total = R.pair_sums(pts, cols, np.array([0]), np.float64(dw), np.float64(cw))[0, 1]
        mx = F32(total)
        k = int(rng.integers(-4, 5))
        for _ in range(abs(k)):
            mx = np.nextafter(mx, F32(np.inf) if k > 0 else F32(-np.inf))
        prm = (float(mx), float(dw), float(cw))
        ref = R.canonical(R.clusterize(pts, cols, *prm))
        assert ref == ([[0, 1]] if total < np.float64(mx) else [[0], [1]])
        assert gpu_comps(gpu_ctx, pts, cols, prm) == ref, (t, k, prm, pts.tolist(), cols.tolist())
        edges += len(ref) == 1
    assert 40 <= edges <= 160                            # both sides of the comparison are covered


def test_cluster_n0_and_argument_checks(gpu_ctx):
    lib = slamhip.lib()
    nc = ctypes.c_int(5)
    assert lib.slam_cluster_points(gpu_ctx.handle, None, None, 0, 1.0, 1.0, 1.0, None, ctypes.byref(nc)) == L.SLAM_OK
    assert nc.value == 0
    assert lib.slam_cluster_points_dev(gpu_ctx.handle, None, None, None, 0, 1.0, 1.0, 1.0, None) == L.SLAM_OK
    assert slamhip.clusterizePoints(np.zeros((0, 3), F32), np.zeros((0, 3), np.uint8), (1, 1, 1), ctx=gpu_ctx) == []
    pts = np.zeros((2, 3), F32)
    assert lib.slam_cluster_points(gpu_ctx.handle, L.ptr(pts), None, 2, 1.0, 1.0, 1.0, None,
                                   ctypes.byref(nc)) == L.SLAM_E_INVALID_ARG
    assert lib.slam_cluster_points(gpu_ctx.handle, None, None, -1, 1.0, 1.0, 1.0, None,
                                   ctypes.byref(nc)) == L.SLAM_E_INVALID_ARG


def test_cluster_device_pointer_entry(gpu_ctx, cloud):
    import torch
    pts, cols = cloud
    prm = api.cluster_params((0.25, 1.0, 0.02))
    host, _ = api.clusterLabels(pts, cols, prm, ctx=gpu_ctx)
    dev = torch.device("cuda", gpu_ctx.device)
    d_pts, d_cols = torch.from_numpy(pts).to(dev), torch.from_numpy(cols).to(dev)
    d_lab = torch.full((len(pts),), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    L.check(slamhip.lib().slam_cluster_points_dev(gpu_ctx.handle, None, ctypes.c_void_p(d_pts.data_ptr()),
                                                  ctypes.c_void_p(d_cols.data_ptr()), len(pts), *prm,
                                                  ctypes.c_void_p(d_lab.data_ptr())), gpu_ctx.handle)
    L.check(slamhip.lib().slam_synchronize(gpu_ctx.handle), gpu_ctx.handle)
    assert np.array_equal(d_lab.cpu().numpy(), host)


# ---- plane -----------------------------------------------------------------------------

def test_project_to_plane_bit_exact(gpu_ctx):
    rng = np.random.default_rng(17)
    pts = (rng.normal(0, 4, (2000, 3)) + [1.5, -2.0, 7.0]).astype(F32)
    centroid = np.array([1.4375, -2.03125, 7.11], F32)
    normal = np.array([0.12, 0.97, -0.21])
    normal /= np.linalg.norm(normal)
    # rows that sit on the normal through the centroid: x = z = 0 after centring (0 / 0 and y^2 / 0)
    axis = np.array([0.0, 1.0, 0.0])
    c0 = np.array([0.5, 0.25, -1.0], F32)
    on_axis = np.array([[0.5, 3.25, -1.0], [0.5, 0.25, -1.0], [0.5, -8.0, -1.0]], F32)
    for p, c, nrm in ((pts, centroid, normal), (pts, centroid, 3.0 * normal), (on_axis, c0, axis),
                      (np.concatenate([on_axis, pts[:5]]), c0, axis)):
        ref = R.project_to_plane(p, c, nrm)
        got = slamhip.projectToPlane(p, c, nrm, ctx=gpu_ctx)
        assert got.dtype == F32 and got.shape == ref.shape
        assert np.array_equal(got, ref, equal_nan=True)
    assert np.isnan(R.project_to_plane(on_axis, c0, axis)[1]).all()       # the fixture reaches 0 / 0
    assert slamhip.projectToPlane(np.zeros((0, 3), F32), c0, axis, ctx=gpu_ctx).shape == (0, 2)


def slab(seed, n=5000):
    """a noisy slab: standard deviations 3 : 0.8 : 0.05 along a random rotation
    (covariance eigenvalues 9 : 0.64 : 0.0025, each separated by more than 10x)"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
    local = rng.normal(0, 1, (n, 3)) * [3.0, 0.8, 0.05]
    return (local @ q.T + rng.uniform(-2, 2, 3)).astype(F32)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fit_plane(gpu_ctx, seed):
    pts = slab(seed)
    n = len(pts)
    p64 = pts.astype(np.float64)
    mean, m = R.plane_moments(pts)
    w = np.linalg.eigvalsh(m)
    assert w[1] >= 10 * w[0] and w[2] >= 10 * w[1]
    centroid, normal = slamhip.getBestFittingPlaneByPoints(pts, ctx=gpu_ctx)
    # centroid: numpy's f64 mean rounded to f32, give or take the one f32 ulp a double rounding can cost
    want = mean.astype(F32)
    assert centroid.dtype == F32
    assert (np.abs(centroid.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    # sums and moments: the summation error bound n * 2^-52 * sum |terms|
    s, mean_d, mom = api.planeMoments(pts, ctx=gpu_ctx)
    eps = 2.0 ** -52
    assert (np.abs(s - p64.sum(0)) <= n * eps * np.abs(p64).sum(0)).all()
    d = p64 - mean
    k = 0
    for a in range(3):
        for b in range(a, 3):
            assert abs(mom[k] - m[a, b]) <= n * eps * np.abs(d[:, a] * d[:, b]).sum(), (a, b)
            k += 1
    # normal: Davis-Kahan with a few-ulp backward error for Jacobi
    _, nref = R.fit_plane(pts)
    assert abs(np.linalg.norm(normal) - 1) < 1e-15 and normal[np.argmax(np.abs(normal))] > 0
    sine = np.linalg.norm(np.cross(normal, nref))
    assert sine <= 64 * eps * w[2] / (w[1] - w[0])
    # deterministic sums: a second call returns the same bits
    c2, n2 = slamhip.getBestFittingPlaneByPoints(pts, ctx=gpu_ctx)
    s2, mean2, mom2 = api.planeMoments(pts, ctx=gpu_ctx)
    assert centroid.tobytes() == c2.tobytes() and normal.tobytes() == n2.tobytes()
    assert s.tobytes() == s2.tobytes() and mean_d.tobytes() == mean2.tobytes() and mom.tobytes() == mom2.tobytes()


def test_segment_end_to_end_on_result_files(gpu_ctx, cloud, tmp_path):
    """slamhip.scene.segment on a cloud written as cycle.py writes it"""
    from slamhip import cycle, scene
    pts, cols = cloud
    gd = cycle.GlobalData()
    gd.push_points(pts.astype(np.float64), cols)
    logs = cycle.Logs(str(tmp_path))
    logs.pose(np.eye(3), np.zeros((3, 1)))
    logs.close(gd)
    loaded = scene.load_global_data(str(tmp_path))
    p32 = loaded.spatialPoints.astype(F32)
    cfg = slamhip.reference_example()
    cfg.update(TriangleMaxDistance=0.25, TriangleEuclidDistanceWeight=1.0, TriangleColorDistance=0.02,
               TriangleMinimumPoints=3)
    segs = scene.segment(loaded, slamhip.ConfigService(cfg), ctx=gpu_ctx)
    ref = [c for c in R.canonical(R.clusterize(p32, cols, 0.25, 1.0, 0.02)) if len(c) >= 3]
    assert [s.indices.tolist() for s in segs] == ref and len(ref) >= 30
    centroid, normal = slamhip.getBestFittingPlaneByPoints(p32, ctx=gpu_ctx)
    for s in segs:
        assert np.array_equal(s.xy, R.project_to_plane(p32[s.indices], centroid, normal), equal_nan=True)

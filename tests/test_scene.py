"""CPU tests of the scene post-processing: the numpy restatement (scene_ref)
against hand-worked cases, the result-file round trip, segment()'s filtering
and ordering (numeric steps patched to scene_ref: no GPU here) and the
host-only behaviour of the new ABI entry points."""
import ctypes
import json
import os

import numpy as np
import pytest

import scene_ref as R
import slamhip
from slamhip import _lib as L
from slamhip import api, cycle, scene

F32 = np.float32
UP5 = float(np.nextafter(F32(5), F32(np.inf)))     # the f32 after 5


# ---- scene_ref against hand-worked cases --------------------------------------------

def test_ref_345_in_space_is_strict():
    pts = np.array([[0, 0, 0], [3, 4, 0]], F32)
    cols = np.zeros((2, 3), np.uint8)
    # sqrt(9 + 16) * 1 + 0 = 5 exactly: 5 < 5 is false
    assert R.clusterize(pts, cols, 5.0, 1.0, 0.0) == [[0], [1]]
    assert R.clusterize(pts, cols, UP5, 1.0, 0.0) == [[0, 1]]


def test_ref_345_in_colour_only():
    pts = np.ones((2, 3), F32)
    cols = np.array([[10, 20, 30], [13, 16, 30]], np.uint8)      # (3, -4, 0)
    assert R.clusterize(pts, cols, 5.0, 1.0, 1.0) == [[0], [1]]
    assert R.clusterize(pts, cols, UP5, 1.0, 1.0) == [[0, 1]]
    assert R.clusterize(pts, cols, 5.0, 1.0, 0.0) == [[0, 1]]    # weight 0: colour ignored, 0 < 5


def test_ref_difference_is_taken_in_f32():
    # 16777216 - 0.5 rounds to 16777216 in f32 (ties to even): 16777216 < 16777216 is false;
    # an f64 subtraction would give 16777215.5 and an edge
    pts = np.array([[16777216, 0, 0], [0.5, 0, 0]], F32)
    cols = np.zeros((2, 3), np.uint8)
    assert R.clusterize(pts, cols, 16777216.0, 1.0, 0.0) == [[0], [1]]
    assert not (np.float64(16777216) - 0.5 >= 16777216)


def test_ref_dfs_preorder_and_discovery_order():
    # a path 0 - 3 - 1 and a pair 2 - 4 (spacing 1 along x, max 1.5)
    x = np.array([0, 2, 10, 1, 11], F32)
    pts = np.stack([x, np.zeros(5, F32), np.zeros(5, F32)], 1)
    cols = np.zeros((5, 3), np.uint8)
    comps = R.clusterize(pts, cols, 1.5, 1.0, 0.0)
    assert comps == [[0, 3, 1], [2, 4]]                # pre-order inside, smallest member first
    assert R.canonical(comps) == [[0, 1, 3], [2, 4]]


def test_ref_nan_point_is_a_singleton_and_max_zero_has_no_edges():
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0]], F32)
    cols = np.zeros((3, 3), np.uint8)
    assert R.canonical(R.clusterize(pts, cols, 1.0, 1.0, 1.0)) == [[0, 2], [1]]
    assert R.clusterize(pts, cols, 0.0, 1.0, 1.0) == [[0], [1], [2]]


def test_ref_projection_hand_case():
    # plane y = 0 through the origin: (3, 4, 0) drops to (3, 0, 0), coef = sqrt(0 / 9 + 1) = 1
    xy = R.project_to_plane(np.array([[3, 4, 0]], F32), np.zeros(3, F32), np.array([0.0, 1.0, 0.0]))
    assert np.array_equal(xy, np.array([[3, 0]], F32))
    # a point on the normal through the centroid: 0 / 0 -> NaN, as the reference's division gives
    xy = R.project_to_plane(np.array([[0, 2, 0]], F32), np.zeros(3, F32), np.array([0.0, 1.0, 0.0]))
    assert np.isnan(xy).all()


def test_ref_fit_plane_of_a_flat_slab():
    rng = np.random.default_rng(3)
    p = np.stack([rng.normal(0, 3, 500), rng.normal(0, 2, 500), np.full(500, 0.5)], 1).astype(F32)
    c, n = R.fit_plane(p)
    assert c.dtype == F32 and abs(c[2] - 0.5) < 1e-6
    assert np.allclose(n, [0, 0, 1], atol=1e-9) and n[2] > 0


# ---- result files ----------------------------------------------------------------------

def _write_run(tmp_path, npts=7, nposes=3):
    rng = np.random.default_rng(11)
    gd = cycle.GlobalData()
    pts = np.round(rng.uniform(-8, 8, (npts, 3)) * 4096) / 4096       # exact in 12 decimals
    cols = rng.integers(0, 256, (npts, 3)).astype(np.uint8)
    gd.push_points(pts, cols)
    logs = cycle.Logs(str(tmp_path))
    poses = []
    for k in range(nposes):
        Rm = np.round(rng.uniform(-1, 1, (3, 3)) * 4096) / 4096
        t = np.round(rng.uniform(-1, 1, (3, 1)) * 4096) / 4096
        logs.pose(Rm, t)
        poses.append((Rm, t))
    logs.close(gd)
    return pts, cols, poses


def test_load_global_data_round_trip(tmp_path):
    pts, cols, poses = _write_run(tmp_path)
    gd = scene.load_global_data(str(tmp_path))
    assert np.array_equal(gd.spatialPoints, pts)
    assert gd.spatialPointsColors.dtype == np.uint8 and np.array_equal(gd.spatialPointsColors, cols)
    assert len(gd.cameraRotations) == len(gd.spatialCameraPositions) == len(poses)
    for (Rm, t), r2, t2 in zip(poses, gd.cameraRotations, gd.spatialCameraPositions):
        assert np.array_equal(Rm, r2) and np.array_equal(t, t2) and t2.shape == (3, 1)


def test_load_global_data_rejects_mismatched_counts(tmp_path):
    _write_run(tmp_path)
    colors = os.path.join(str(tmp_path), "colors.txt")
    lines = open(colors).read().splitlines()
    with open(colors, "w") as f:
        f.write("\n".join(lines[:-1]) + "\n")
    with pytest.raises(ValueError, match="points and their colors"):
        scene.load_global_data(str(tmp_path))
    _write_run(tmp_path)
    rot = os.path.join(str(tmp_path), "rotations.txt")
    lines = open(rot).read().splitlines()
    with open(rot, "w") as f:
        f.write("\n".join(lines[:-3]) + "\n")
    with pytest.raises(ValueError, match="rotations and translations"):
        scene.load_global_data(str(tmp_path))


# ---- segment ---------------------------------------------------------------------------

def _cfg(**over):
    d = slamhip.reference_example()
    d.update(over)
    return slamhip.ConfigService(d)


def _patch_to_ref(monkeypatch):
    calls = {"fit": []}

    def clusterize(points, colors, config, ctx=None):
        mx, dw, cw = api.cluster_params(config)
        return [np.array(c, np.int32) for c in R.canonical(R.clusterize(points, colors, mx, dw, cw))]

    def fit(points, ctx=None):
        calls["fit"].append(len(points))
        return R.fit_plane(points)

    monkeypatch.setattr(api, "clusterizePoints", clusterize)
    monkeypatch.setattr(api, "getBestFittingPlaneByPoints", fit)
    monkeypatch.setattr(api, "projectToPlane", lambda p, c, n, ctx=None: R.project_to_plane(p, c, n))
    return calls


def _three_groups():
    # groups of 4, 1 and 3 points, interleaved: {0, 2, 5, 7}, {1}, {3, 4, 6}
    rng = np.random.default_rng(5)
    base = {0: (0, 0, 0), 1: (50, 0, 0), 2: (0, 0, 50)}
    group = [0, 1, 0, 2, 2, 0, 2, 0]
    pts = np.array([base[g] for g in group], np.float64) + rng.uniform(-0.2, 0.2, (8, 3))
    gd = cycle.GlobalData()
    gd.push_points(pts, np.full((8, 3), 100, np.uint8))
    return gd


def test_segment_filters_small_components_and_keeps_discovery_order(monkeypatch):
    calls = _patch_to_ref(monkeypatch)
    gd = _three_groups()
    cfg = _cfg(TriangleMaxDistance=2.0, TriangleEuclidDistanceWeight=1.0, TriangleColorDistance=0.0,
               TriangleMinimumPoints=3)
    segs = scene.segment(gd, cfg)
    assert [s.indices.tolist() for s in segs] == [[0, 2, 5, 7], [3, 4, 6]]
    assert calls["fit"] == [8]                          # the plane is fitted once, on ALL points
    p32 = gd.spatialPoints.astype(F32)
    c, n = R.fit_plane(p32)
    for s in segs:
        assert s.points.dtype == F32 and np.array_equal(s.points, p32[s.indices])
        assert np.array_equal(s.colors, gd.spatialPointsColors[s.indices])
        assert s.xy.shape == (len(s.indices), 2)
        assert np.array_equal(s.xy, R.project_to_plane(p32[s.indices], c, n), equal_nan=True)
    # the threshold is "size < TriangleMinimumPoints": 4 keeps only the group of four, 1 keeps all
    assert [s.indices.tolist() for s in scene.segment(gd, _cfg(
        TriangleMaxDistance=2.0, TriangleEuclidDistanceWeight=1.0, TriangleColorDistance=0.0,
        TriangleMinimumPoints=4))] == [[0, 2, 5, 7]]
    assert len(scene.segment(gd, _cfg(TriangleMaxDistance=2.0, TriangleEuclidDistanceWeight=1.0,
                                      TriangleColorDistance=0.0, TriangleMinimumPoints=1))) == 3


def test_scene_main_writes_clusters_for_only_viz(monkeypatch, tmp_path):
    _patch_to_ref(monkeypatch)
    gd = _three_groups()
    logs = cycle.Logs(str(tmp_path))
    logs.pose(np.eye(3), np.zeros((3, 1)))
    logs.close(gd)
    cfg = slamhip.reference_example()
    cfg.update(onlyViz=True, outputDataDir=str(tmp_path), TriangleMaxDistance=2.0, TriangleColorDistance=0.0)
    path = os.path.join(str(tmp_path), "config.json")
    with open(path, "w") as f:
        json.dump(cfg, f)
    scene.main(path)
    assert open(os.path.join(str(tmp_path), "clusters.txt")).read() == "0 2 5 7\n3 4 6\n"
    cfg["onlyViz"] = False
    with open(path, "w") as f:
        json.dump(cfg, f)
    with pytest.raises(ValueError):
        scene.main(path)


def test_components_from_labels():
    comps = api.components_from_labels(np.array([0, 1, 0, 3, 1, 0], np.int32))
    assert [c.tolist() for c in comps] == [[0, 2, 5], [1, 4], [3]]
    assert all(c.dtype == np.int32 for c in comps)
    assert api.components_from_labels(np.zeros(0, np.int32)) == []


def test_cluster_params_round_through_f32():
    cfg = _cfg(TriangleMaxDistance=0.1, TriangleEuclidDistanceWeight=1.0, TriangleColorDistance=0.02)
    assert api.cluster_params(cfg) == (float(F32(0.1)), 1.0, float(F32(0.02)))
    assert api.cluster_params((0.1, 1, 0.02)) == api.cluster_params(cfg)


# ---- host-only ABI behaviour ---------------------------------------------------------------

def test_scene_abi_rejects_a_null_context_and_bad_sizes():
    lib = slamhip.lib()
    pts = np.zeros((4, 3), F32)
    cols = np.zeros((4, 3), np.uint8)
    labels = np.zeros(4, np.int32)
    nc = ctypes.c_int(7)
    f3, d3, xy = np.zeros(3, F32), np.zeros(3), np.zeros((4, 2), F32)
    bad = L.SLAM_E_INVALID_ARG
    for n in (4, 0, -1):
        assert lib.slam_cluster_points(None, L.ptr(pts), L.ptr(cols), n, 1.0, 1.0, 1.0, L.ptr(labels),
                                       ctypes.byref(nc)) == bad
        assert lib.slam_cluster_points_dev(None, None, L.ptr(pts), L.ptr(cols), n, 1.0, 1.0, 1.0, L.ptr(labels)) == bad
        assert lib.slam_fit_plane(None, L.ptr(pts), n, L.ptr(f3), L.ptr(d3)) == bad
        assert lib.slam_plane_moments(None, L.ptr(pts), n, L.ptr(d3), L.ptr(d3), L.ptr(np.zeros(6))) == bad
        assert lib.slam_project_to_plane(None, L.ptr(pts), n, L.ptr(f3), L.ptr(d3), L.ptr(xy)) == bad
    u = ctypes.c_uint64(0)
    assert lib.slam_cluster_last_stats(None, ctypes.byref(u), ctypes.byref(u)) == bad
    assert nc.value == 7                                 # nothing was written
    assert lib.slam_abi_version() == 3

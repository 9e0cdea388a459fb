"""GPU tests of the semi-global aggregation (mvs_volume in csrc/mvs.hip, sgm_path and
sgm_winner in csrc/mvs_sgm.hip, behind slam_mvs_cost_volume_dev,
slam_mvs_sgm_aggregate_dev, slam_mvs_depth_sgm* and slamhip.dense): every device
result equals tests/mvs_sgm_ref.py bit for bit; the cases are those of
tests/test_mvs_sgm.py.
"""
import ctypes
import json

import numpy as np
import pytest

import mvs_ref as R
import mvs_sgm_ref as G
import slamhip
from slamhip import _lib as L
from slamhip import cycle, dense, scene

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel elements on each side of an output buffer


def dev(gpu_ctx, sc, r, uq, mv, p1, p2, paths):
    return slamhip.planeSweepDepthSgm(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], r, uq, mv, p1, p2, paths, ctx=gpu_ctx)


def assert_same(got, want, tag):
    for g, w, what in zip(got, want, ("plane", "cost", "inv_depth")):
        assert R.same_bits(g, w), (tag, what, int((np.asarray(g) != np.asarray(w)).sum()))


def _pad4(a, S, k):
    return np.pad(np.asarray(a, np.float64).reshape(S, k), ((0, 4 - S), (0, 0)))[None]


# ---- each stage alone ----------------------------------------------------------------------

@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_volume_equals_reference(gpu_ctx, name):
    import torch
    sc, r, _, _ = R.sweep_cases()[name]
    C, nv = G.volume(name)
    S = len(sc["srcs"])
    frames = torch.from_numpy(np.stack([sc["ref"]] + list(sc["srcs"]))).cuda()
    gC, gnv = slamhip.planeSweepCostVolume(frames, [0], [list(range(1, S + 1))], _pad4(sc["M"], S, 9), _pad4(sc["v"], S, 3),
                                           sc["planes"][None], r, ctx=gpu_ctx)
    assert gC.dtype == torch.uint16 and gnv.dtype == torch.uint8 and tuple(gC.shape) == (1,) + C.shape[1:] + C.shape[:1]
    assert np.array_equal(gC[0].cpu().numpy().transpose(2, 0, 1), C)
    assert np.array_equal(gnv[0].cpu().numpy().transpose(2, 0, 1), nv)


@pytest.mark.parametrize("paths", [4, 8])
def test_aggregate_on_random_maximal_volumes(gpu_ctx, paths):
    """the shapes of the CPU test plus one plane count per register count of the path kernel (K = 1 .. 4) and its
    partly filled last register, lines shorter and longer than the wave count of a workgroup"""
    rng = np.random.RandomState(17 + paths)
    for (n, h, w, D), (P1, P2) in (((2, 7, 9, 256), (G.MAX_P2, G.MAX_P2)), ((1, 9, 7, 65), (0, G.MAX_P2)),
                                   ((3, 5, 4, 4), (1, 2)), ((1, 1, 1, 64), (7, 9)), ((1, 33, 67, 12), (250, 3000)),
                                   ((1, 6, 5, 129), (100, 40000)), ((2, 3, 11, 192), (G.MAX_P2, G.MAX_P2)),
                                   ((1, 4, 3, 63), (0, 0))):
        C = G.random_volume(rng, n, h, w, D, maxima=True)
        got = slamhip.sgmAggregate(C, P1, P2, paths, ctx=gpu_ctx)
        assert R.same_bits(got, G.aggregate_public(C, P1, P2, paths)), (n, h, w, D)


# ---- the depth maps ----------------------------------------------------------------------------

@pytest.mark.parametrize("setting", G.SETTINGS, ids=lambda s: "p%d_%d_%d" % s)
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_depth_equals_reference(gpu_ctx, name, setting):
    sc, r, uq, mv = R.sweep_cases()[name]
    assert_same(dev(gpu_ctx, sc, r, uq, mv, *setting), G.case(name, *setting), name)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_zero_penalties_are_winner_take_all(gpu_ctx, name):
    sc, r, uq, mv, (plane, cost, inv) = R.case(name)
    for paths in (4, 8):
        gp, gc, gi = dev(gpu_ctx, sc, r, uq, mv, 0, 0, paths)
        assert R.same_bits(gp, plane) and R.same_bits(gi, inv) and np.array_equal(gc, paths * cost)


@pytest.mark.parametrize("shape", G.EDGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_depth_on_edge_shapes(gpu_ctx, shape):
    h, w = shape
    sc = G.pose_scene(h, w, 12, 31)
    for setting in G.SETTINGS:
        want = G.depth(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], 1, 80, 1, *setting)
        assert_same(dev(gpu_ctx, sc, 1, 80, 1, *setting), want, (shape, setting))


@pytest.mark.parametrize("D", G.EDGE_PLANES)
def test_depth_on_plane_counts(gpu_ctx, D):
    sc = G.pose_scene(20, 24, D, 32, S=2)
    for setting in ((10, 120, 8), (255, 255, 4)):
        want = G.depth(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], 2, 80, 1, *setting)
        assert_same(dev(gpu_ctx, sc, 2, 80, 1, *setting), want, (D, setting))


@pytest.mark.parametrize("paths", [4, 8])
def test_wall_scene_on_device(gpu_ctx, paths):
    sc = G.wall_scene()
    wta = slamhip.planeSweepDepth(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], 2, 80, 1, ctx=gpu_ctx)
    assert (wta[2][sc["interior"]] == 0).all()
    for p1, p2 in ((10, 120), (2, 12)):
        plane, _, inv = dev(gpu_ctx, sc, 2, 80, 1, p1, p2, paths)
        box = sc["interior"]
        assert (plane[box] == 5).all() and (inv[box] > 0).all() and (np.abs(inv[box].astype(np.float64) - 5.0) < 0.5).all()
        assert (plane[sc["region"]] == 5).all()


# ---- batches, the scratch budget, sentinels -----------------------------------------------------

def _batch_scene():
    """four frames, three references that share sources, S = 2, 1 and 2 (the scene of tests/test_mvs_gpu.py)"""
    a = R.general_pose(33, 67, 3, 12, 9)
    frames = np.stack([a["ref"]] + a["srcs"])
    ref_idx = [0, 1, 2]
    src_idx = [[1, 2], [0], [3, 1]]
    M = np.zeros((3, 4, 9))
    v = np.zeros((3, 4, 3))
    rng = np.random.RandomState(4)
    for i, s in enumerate(src_idx):
        for n in range(len(s)):
            M[i, n] = a["M"][(i + n) % 3] + rng.uniform(-1e-3, 1e-3, 9)
            v[i, n] = a["v"][(i + n) % 3]
    planes = np.stack([np.linspace(0.05, 1.2, 12), np.linspace(0.1, 0.9, 12), np.linspace(0.02, 1.5, 12)])
    return frames, ref_idx, src_idx, M, v, planes


@pytest.fixture(scope="module")
def batch_want():
    frames, ref_idx, src_idx, M, v, planes = _batch_scene()
    out = []
    for i in range(3):
        S = len(src_idx[i])
        out.append(G.depth(frames[ref_idx[i]], [frames[j] for j in src_idx[i]], M[i, :S], v[i, :S], planes[i], 2, 85, 1, 10, 120, 8))
    return out


def test_batch_equals_single_calls(gpu_ctx, batch_want):
    import torch
    frames, ref_idx, src_idx, M, v, planes = _batch_scene()
    d = torch.from_numpy(frames).cuda()
    plane, cost, inv = slamhip.planeSweepDepthSgmBatch(d, ref_idx, src_idx, M, v, planes, 2, 85, 1, 10, 120, 8, ctx=gpu_ctx)
    for i in range(3):
        S = len(src_idx[i])
        one = slamhip.planeSweepDepthSgm(frames[ref_idx[i]], [frames[j] for j in src_idx[i]], M[i, :S], v[i, :S], planes[i],
                                         2, 85, 1, 10, 120, 8, ctx=gpu_ctx)
        for g, o, w in zip((plane[i], cost[i], inv[i]), one, batch_want[i]):
            assert R.same_bits(g.cpu().numpy(), o) and R.same_bits(o, w)


@pytest.mark.parametrize("budget", [250_000, 400_000])
def test_small_budget_splits_the_batch_and_changes_nothing(gpu_ctx, batch_want, budget):
    """a reference takes 7 bytes per pixel and plane = 185 724 bytes here: 250 000 bytes hold one reference a group
    (three groups), 400 000 two (groups of two and one)"""
    import torch
    frames, ref_idx, src_idx, M, v, planes = _batch_scene()
    assert 7 * 33 * 67 * 12 == 185_724
    d = torch.from_numpy(frames).cuda()
    whole = slamhip.planeSweepDepthSgmBatch(d, ref_idx, src_idx, M, v, planes, 2, 85, 1, 10, 120, 8, ctx=gpu_ctx)
    split = slamhip.planeSweepDepthSgmBatch(d, ref_idx, src_idx, M, v, planes, 2, 85, 1, 10, 120, 8, ctx=gpu_ctx, budget=budget)
    for a, b in zip(whole, split):
        assert R.same_bits(a.cpu().numpy(), b.cpu().numpy())
    for i in range(3):
        for g, w in zip(split, batch_want[i]):
            assert R.same_bits(g[i].cpu().numpy(), w)


def _guarded(torch, n, dtype, fill):
    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return t, ctypes.c_void_p(t.data_ptr() + GUARD * t.element_size())


def _guards_intact(t, n, fill):
    a = t.cpu().numpy()
    return (a[:GUARD] == fill).all() and (a[GUARD + n:] == fill).all()


@pytest.mark.parametrize("D", [12, 16])
def test_sentinels_around_device_outputs(gpu_ctx, D):
    """the volume, the valid counts, S and the three maps are written inside their elements only; D = 12 takes the
    plane-by-plane stores of mvs_volume and the scalar loads of sgm_winner, D = 16 the staged 16-byte ones"""
    import torch
    frames, ref_idx, src_idx, M, v, planes = _batch_scene()
    planes = np.stack([np.linspace(p[0], p[-1], D) for p in planes])
    n, h, w = frames.shape[:3]
    d = torch.from_numpy(frames).cuda()
    c = gpu_ctx.handle
    lib = slamhip.lib()
    nref = 3
    vol = nref * h * w * D
    ref = np.array(ref_idx, np.int32)
    nsrc = np.array([len(s) for s in src_idx], np.int32)
    src = np.full((nref, 4), -1, np.int32)
    for i, s in enumerate(src_idx):
        src[i, :len(s)] = s
    Mc, vc, pc = np.ascontiguousarray(M.reshape(nref, 36)), np.ascontiguousarray(v.reshape(nref, 12)), np.ascontiguousarray(planes)
    fp = ctypes.c_void_p(d.data_ptr())
    C, pC = _guarded(torch, vol, torch.int16, -77)
    nv, pnv = _guarded(torch, vol, torch.uint8, 199)
    assert lib.slam_mvs_cost_volume_dev(c, None, fp, n, w, h, 1, nref, L.ptr(ref), L.ptr(nsrc), L.ptr(src), L.ptr(Mc), L.ptr(vc),
                                        L.ptr(pc), D, 3, pC, pnv) == L.SLAM_OK
    assert _guards_intact(C, vol, -77) and _guards_intact(nv, vol, 199)
    body = C.cpu().numpy()[GUARD:GUARD + vol]
    assert (body >= 0).all() and (nv.cpu().numpy()[GUARD:GUARD + vol] <= 2).all()      # every element inside was written
    S, pS = _guarded(torch, vol, torch.int32, -77)
    assert lib.slam_mvs_sgm_aggregate_dev(c, None, pC, nref, w, h, D, 490, 5880, 8, pS) == L.SLAM_OK
    assert _guards_intact(S, vol, -77)
    want = G.aggregate_public(body.view(np.uint16).reshape(nref, h, w, D), 490, 5880, 8)
    assert R.same_bits(S.cpu().numpy()[GUARD:GUARD + vol].reshape(nref, h, w, D), want)
    pl, pp = _guarded(torch, nref * h * w, torch.int16, -77)
    co, pco = _guarded(torch, nref * h * w, torch.int32, -77)
    iv, pi = _guarded(torch, nref * h * w, torch.float32, -77.0)
    assert lib.slam_mvs_depth_sgm_batch_dev(c, None, fp, n, w, h, 1, nref, L.ptr(ref), L.ptr(nsrc), L.ptr(src), L.ptr(Mc),
                                            L.ptr(vc), L.ptr(pc), D, 3, 80, 1, 10, 120, 8, pp, pco, pi) == L.SLAM_OK
    assert _guards_intact(pl, nref * h * w, -77) and _guards_intact(co, nref * h * w, -77) and _guards_intact(iv, nref * h * w, -77.0)
    assert (iv.cpu().numpy()[GUARD:GUARD + nref * h * w] != -77.0).all()
    ms = np.zeros(3)
    assert lib.slam_mvs_sgm_last_timing(c, L.ptr(ms)) == L.SLAM_OK and (ms > 0).all()


def test_argument_errors_on_device(gpu_ctx):
    import torch
    sc, r, uq, mv, _ = R.case("planted")
    args = (sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], 2, 80, 1)
    for bad in ((121, 120, 8), (-1, 120, 8), (10, 256, 8), (10, 120, 6), (10, 120, 0)):
        with pytest.raises(L.SlamError) as e:
            slamhip.planeSweepDepthSgm(*args, *bad, ctx=gpu_ctx)
        assert e.value.code == L.SLAM_E_INVALID_ARG
    for bad in (dict(planes=np.arange(3.0)), dict(planes=sc["planes"], radius=4), dict(planes=sc["planes"], min_views=2)):
        with pytest.raises(L.SlamError) as e:
            slamhip.planeSweepDepthSgm(sc["ref"], sc["srcs"], sc["M"], sc["v"], ctx=gpu_ctx, **bad)
        assert e.value.code == L.SLAM_E_INVALID_ARG
    wide = np.zeros((2, 4097), np.uint8)
    with pytest.raises(L.SlamError) as e:
        slamhip.planeSweepDepthSgm(wide, [wide], sc["M"], sc["v"], sc["planes"], ctx=gpu_ctx)
    assert e.value.code == L.SLAM_E_UNSUPPORTED
    C = torch.zeros((1, 2, 3, 4), dtype=torch.int16, device="cuda").view(torch.uint16)
    for P1, P2, paths in ((3, 2, 8), (1, G.MAX_P2 + 1, 8), (-1, 2, 8), (1, 2, 5)):
        with pytest.raises(L.SlamError) as e:
            slamhip.sgmAggregate(C, P1, P2, paths, ctx=gpu_ctx)
        assert e.value.code == L.SLAM_E_INVALID_ARG
    with pytest.raises(L.SlamError) as e:
        slamhip.sgmAggregate(torch.zeros((1, 1, 4097, 4), dtype=torch.int16, device="cuda").view(torch.uint16), 1, 2, 8, ctx=gpu_ctx)
    assert e.value.code == L.SLAM_E_UNSUPPORTED
    assert int(slamhip.sgmAggregate(C, 1, G.MAX_P2, 8, ctx=gpu_ctx).abs().max()) == 0


# ---- densify and slam_main ---------------------------------------------------------------------

def test_densify_equals_the_host_path(gpu_ctx):
    """the planted sequence of tests/test_mvs_gpu.py with aggregated maps: the device path, the host path and the
    contract's pipeline (mvs_sgm_ref.depth + mvs_ref.fuse) emit the same points"""
    h, w, k = 40, 52, 5
    tex = R.noise(h, w, 7, 3)
    frames = [tex, R.shifted(tex, k)]
    K = np.array([[64.0, 0, 26.0], [0, 64.0, 20.0], [0, 0, 1.0]])
    rot, pos = [np.eye(3), np.eye(3)], [np.zeros((3, 1)), np.array([[1.0], [0.0], [0.0]])]
    sparse = np.stack([np.zeros(20), np.zeros(20), np.array([8.0] * 10 + [64.0 / 1.5] * 10)], 1)
    sg = dense.SgmParams()
    prm = dense.DenseParams(D=12, sources=1, radius=2, uniq=80, min_views=1, eps=0.25, min_consistent=1, step=4, sgm=sg)
    pts, cols = dense.densify(frames, K, rot, pos, sparse, prm, ctx=gpu_ctx)
    hp, hc = dense.densify(frames, K, rot, pos, sparse, prm, host=True)
    assert R.same_bits(hp, pts) and R.same_bits(hc, cols) and len(pts) > 0
    P = dense.plan(frames[0].shape, K, rot, pos, sparse, prm)
    maps = [G.depth(frames[i], [frames[j] for j in P["src"][m]], P["M"][m, :1], P["v"][m, :1], P["planes"][m], 2, 80, 1,
                    sg.p1, sg.p2, sg.paths) for m, i in enumerate(P["ref"])]
    want_p, want_c = R.fuse(frames, [m[2] for m in maps], P["nbr"], P["nbrM"], P["nbrv"], P["B"], P["c"], 0.25, 1, 4, 2)
    assert R.same_bits(pts, want_p) and R.same_bits(cols, want_c)


def test_slam_main_dense_sgm(gpu_ctx, tmp_path):
    from test_cycle import K_VGA, _cfg
    frames = slamhip.synth_frames(640, 480, 0, 16, seed=1234)
    cfg = _cfg()
    prm = dense.DenseParams(D=16, sources=2, step=16, sgm=dense.SgmParams())
    outs = {}
    for name, dp in (("plain", None), ("dense", prm)):
        K = K_VGA.copy()
        gd, logs = cycle.slam_main(cycle.MediaSources(list(frames)), K, cfg, cycle.GpuOps(gpu_ctx), out_dir=str(tmp_path / name),
                                   dense=dp)
        outs[name] = (gd, logs, K)
    for f in ("poses.txt", "rotations.txt", "points.txt", "colors.txt"):
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "dense" / f).read_bytes(), f
    gd, logs, K = outs["dense"]
    assert len(logs.frames) == len(gd.cameraRotations) >= 3
    hp, hc = dense.densify(logs.frames, K, gd.cameraRotations, gd.spatialCameraPositions, gd.spatialPoints, prm, host=True)
    assert R.same_bits(hp, gd.densePoints) and R.same_bits(hc, gd.denseColors) and len(hp) > 0
    import io
    for arr, f in ((hp, "dense_points.txt"), (hc, "dense_colors.txt")):
        s = io.StringIO()
        cycle.raw_output(arr, s)
        assert (tmp_path / "dense" / f).read_text() == s.getvalue()
    d = slamhip.reference_example()
    d.update(onlyViz=True, outputDataDir=str(tmp_path / "dense"))
    (tmp_path / "config.json").write_text(json.dumps(d))
    scene.main(str(tmp_path / "config.json"), cloud="dense")
    loaded = scene.load_global_data(str(tmp_path / "dense"), cloud="dense")
    assert len(loaded.spatialPoints) == len(hp) and np.array_equal(loaded.spatialPointsColors, hc)

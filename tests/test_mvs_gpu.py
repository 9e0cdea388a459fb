"""GPU tests of plane-sweep stereo (csrc/mvs.hip behind slam_mvs_census_dev,
slam_mvs_depth*, slam_mvs_fuse* and slamhip.dense): every device result equals
tests/mvs_ref.py bit for bit; the cases are those of tests/test_mvs.py.
"""
import ctypes
import json

import numpy as np
import pytest

import mvs_ref as R
import slamhip
from slamhip import _lib as L
from slamhip import cycle, dense, scene

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel elements on each side of an output buffer


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (40, 52), (33, 67)])
def test_census_equals_reference(gpu_ctx, shape, ch):
    f = R.noise(shape[0], shape[1], 3 + ch, ch)
    got = slamhip.censusTransform(f, ctx=gpu_ctx)
    want = R.census(f)
    assert got.dtype == np.uint64 and R.same_bits(got, want)
    assert int(got.max()) < (1 << 62)


def test_census_batch(gpu_ctx):
    import torch
    fr = np.stack([R.noise(33, 67, 40 + i, 3) for i in range(3)])
    got = slamhip.censusTransform(torch.from_numpy(fr).cuda(), ctx=gpu_ctx)
    for i in range(3):
        assert R.same_bits(got[i], R.census(fr[i]))


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_sweep_equals_reference(gpu_ctx, name):
    sc, r, uq, mv, want = R.case(name)
    got = slamhip.planeSweepDepth(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], r, uq, mv, ctx=gpu_ctx)
    for g, w, what in zip(got, want, ("plane", "cost", "inv_depth")):
        assert R.same_bits(g, w), (name, what, int((g != w).sum()))


def test_planted_plane_on_device(gpu_ctx):
    sc, r, uq, mv, _ = R.case("planted")
    plane, cost, inv = slamhip.planeSweepDepth(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], r, uq, mv, ctx=gpu_ctx)
    H, W = plane.shape
    k = sc["k"]
    reg = (slice(5, H - 5), slice(6, W - 6 - k))
    assert (plane[reg] == k).all() and (cost[reg] == 0).all() and (inv[reg] > 0).all()


def _batch_scene():
    """four frames, three references that share sources, S = 2, 1 and 2"""
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


def test_batch_equals_single_calls(gpu_ctx):
    import torch
    frames, ref_idx, src_idx, M, v, planes = _batch_scene()
    dev = torch.from_numpy(frames).cuda()
    plane, cost, inv = slamhip.planeSweepDepthBatch(dev, ref_idx, src_idx, M, v, planes, 2, 85, 1, ctx=gpu_ctx)
    for i in range(3):
        S = len(src_idx[i])
        one = slamhip.planeSweepDepth(frames[ref_idx[i]], [frames[j] for j in src_idx[i]], M[i, :S], v[i, :S], planes[i],
                                      2, 85, 1, ctx=gpu_ctx)
        want = R.depth(frames[ref_idx[i]], [frames[j] for j in src_idx[i]], M[i, :S], v[i, :S], planes[i], 2, 85, 1)
        for g, o, w in zip((plane[i], cost[i], inv[i]), one, want):
            assert R.same_bits(g.cpu().numpy(), o) and R.same_bits(o, w)


def _guarded(torch, n, dtype, fill):
    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return t, ctypes.c_void_p(t.data_ptr() + GUARD * t.element_size())


def _guards_intact(t, n, fill):
    a = t.cpu().numpy()
    return (a[:GUARD] == fill).all() and (a[GUARD + n:] == fill).all()


def test_sentinels_around_device_outputs(gpu_ctx):
    """census, plane, cost and inv_depth are written inside their n x h x w elements only (odd sizes: the
    last tiles of a row and of the image are partial)"""
    import torch
    frames, ref_idx, src_idx, M, v, planes = _batch_scene()
    n, h, w = frames.shape[:3]
    dev = torch.from_numpy(frames).cuda()
    c = gpu_ctx.handle
    lib = slamhip.lib()
    cen, pc = _guarded(torch, n * h * w, torch.int64, -7)
    assert lib.slam_mvs_census_dev(c, None, ctypes.c_void_p(dev.data_ptr()), n, w, h, 1, pc) == L.SLAM_OK
    assert _guards_intact(cen, n * h * w, -7)
    nref = 3
    pl, pp = _guarded(torch, nref * h * w, torch.int16, -77)
    co, pco = _guarded(torch, nref * h * w, torch.int32, -77)
    iv, pi = _guarded(torch, nref * h * w, torch.float32, -77.0)
    ref = np.array(ref_idx, np.int32)
    nsrc = np.array([len(s) for s in src_idx], np.int32)
    src = np.full((nref, 4), -1, np.int32)
    for i, s in enumerate(src_idx):
        src[i, :len(s)] = s
    Mc, vc, pc_ = np.ascontiguousarray(M.reshape(nref, 36)), np.ascontiguousarray(v.reshape(nref, 12)), np.ascontiguousarray(planes)
    assert lib.slam_mvs_depth_batch_dev(c, None, ctypes.c_void_p(dev.data_ptr()), n, w, h, 1, nref, L.ptr(ref), L.ptr(nsrc),
                                        L.ptr(src), L.ptr(Mc), L.ptr(vc), L.ptr(pc_), 12, 3, 80, 1, pp, pco, pi) == L.SLAM_OK
    assert _guards_intact(pl, nref * h * w, -77) and _guards_intact(co, nref * h * w, -77) and _guards_intact(iv, nref * h * w, -77.0)
    body = iv.cpu().numpy()[GUARD:GUARD + nref * h * w]
    assert (body != -77.0).all()          # and every element inside was written


@pytest.mark.parametrize("min_consistent", [1, 2])
@pytest.mark.parametrize("step", [1, 4])
def test_fuse_equals_reference(gpu_ctx, step, min_consistent):
    fs = R.fuse_scene()
    want_p, want_c = R.fuse(fs["frames"], fs["inv"], fs["nbrs"], fs["M"], fs["v"], fs["B"], fs["c"], 0.01, min_consistent, step, 2)
    assert len(want_p) >= 20
    # host-pointer entry, into buffers of exactly the needed size between sentinels
    n = len(want_p)
    pts = np.full((n + 2, 3), -5.0)
    cols = np.full((n + 2, 3), 99, np.uint8)
    nmaps = len(fs["inv"])
    nn = np.array([len(r) for r in fs["nbrs"]], np.int32)
    nb = np.full((nmaps, 4), -1, np.int32)
    for i, r in enumerate(fs["nbrs"]):
        nb[i, :len(r)] = r
    fr = [np.ascontiguousarray(f) for f in fs["frames"]]
    h, w = fr[0].shape[:2]
    inv = np.ascontiguousarray(np.stack(fs["inv"]), np.float32)
    n_out = ctypes.c_int(0)
    arr = (ctypes.c_void_p * nmaps)(*[f.ctypes.data for f in fr])
    M, v, B, c = (np.ascontiguousarray(fs[k].reshape(nmaps, -1)) for k in ("M", "v", "B", "c"))
    rc = slamhip.lib().slam_mvs_fuse(gpu_ctx.handle, arr, w, h, w * 3, 3, nmaps, L.ptr(inv), L.ptr(nn), L.ptr(nb), L.ptr(M),
                                     L.ptr(v), L.ptr(B), L.ptr(c), 0.01, min_consistent, step, 2,
                                     ctypes.c_void_p(pts.ctypes.data + 24), ctypes.c_void_p(cols.ctypes.data + 3), n,
                                     ctypes.byref(n_out))
    assert rc == L.SLAM_OK and n_out.value == n
    assert R.same_bits(pts[1:-1], want_p) and R.same_bits(cols[1:-1], want_c)
    assert (pts[0] == -5.0).all() and (pts[-1] == -5.0).all() and (cols[0] == 99).all() and (cols[-1] == 99).all()
    # the resident entry through the package
    import torch
    got_p, got_c = slamhip.fuseDepthMaps(torch.from_numpy(np.stack(fr)).cuda(), torch.from_numpy(inv).cuda(), fs["nbrs"],
                                         fs["M"], fs["v"], fs["B"], fs["c"], 0.01, min_consistent, step, 2, ctx=gpu_ctx)
    assert R.same_bits(got_p, want_p) and R.same_bits(got_c, want_c)


def test_fuse_zero_survivors_and_capacity(gpu_ctx):
    fs = R.fuse_scene()
    zero = [np.zeros_like(m) for m in fs["inv"]]
    p, c = slamhip.fuseDepthMaps(fs["frames"], zero, fs["nbrs"], fs["M"], fs["v"], fs["B"], fs["c"], ctx=gpu_ctx)
    assert p.shape == (0, 3) and c.shape == (0, 3)
    want_p, _ = R.fuse(fs["frames"], fs["inv"], fs["nbrs"], fs["M"], fs["v"], fs["B"], fs["c"], 0.01, 1, 1, 2)
    with pytest.raises(L.SlamError) as e:
        slamhip.fuseDepthMaps(fs["frames"], fs["inv"], fs["nbrs"], fs["M"], fs["v"], fs["B"], fs["c"], 0.01, 1, 1, 2,
                              cap=len(want_p) - 1, ctx=gpu_ctx)
    assert e.value.code == L.SLAM_E_CAPACITY and e.value.needed == len(want_p)
    p, _ = slamhip.fuseDepthMaps(fs["frames"], fs["inv"], fs["nbrs"], fs["M"], fs["v"], fs["B"], fs["c"], 0.01, 1, 1, 2,
                                 cap=len(want_p), ctx=gpu_ctx)
    assert R.same_bits(p, want_p)


def test_argument_errors_on_device(gpu_ctx):
    sc, r, uq, mv, _ = R.case("planted")
    args = (sc["ref"], sc["srcs"], sc["M"], sc["v"])
    for bad in (dict(planes=np.arange(3.0)), dict(planes=np.arange(257.0)), dict(planes=sc["planes"], radius=4),
                dict(planes=np.array([0, 1, np.inf, 3.0])), dict(planes=sc["planes"], min_views=2)):
        kw = dict(radius=2)
        kw.update(bad)
        with pytest.raises(L.SlamError) as e:
            slamhip.planeSweepDepth(*args, ctx=gpu_ctx, **kw)
        assert e.value.code == L.SLAM_E_INVALID_ARG
    with pytest.raises(L.SlamError) as e:
        slamhip.planeSweepDepth(sc["ref"], sc["srcs"], np.full((1, 9), np.nan), sc["v"], sc["planes"], ctx=gpu_ctx)
    assert e.value.code == L.SLAM_E_INVALID_ARG
    wide = np.zeros((2, 4097), np.uint8)
    with pytest.raises(L.SlamError) as e:
        slamhip.planeSweepDepth(wide, [wide], sc["M"], sc["v"], sc["planes"], ctx=gpu_ctx)
    assert e.value.code == L.SLAM_E_UNSUPPORTED


# ---- densify -------------------------------------------------------------------------------

def planted_sequence():
    """two frames of one fronto-parallel textured wall: K with f = 64 (M = K K^-1 = I exactly), a
    baseline of one unit along x (v = (+-64, 0, 0)), sparse points whose 5 % / 95 % depths put the 12
    planes at disparities 1 .. 12, so the wall at disparity 5 is plane 4 in both frames"""
    h, w, k = 40, 52, 5
    tex = R.noise(h, w, 7, 3)
    frames = [tex, R.shifted(tex, k)]
    K = np.array([[64.0, 0, 26.0], [0, 64.0, 20.0], [0, 0, 1.0]])
    rot = [np.eye(3), np.eye(3)]
    pos = [np.zeros((3, 1)), np.array([[1.0], [0.0], [0.0]])]
    z = np.array([8.0] * 10 + [64.0 / 1.5] * 10)
    sparse = np.stack([np.zeros(20), np.zeros(20), z], 1)
    return frames, K, rot, pos, sparse, k


def test_densify_planted_scene(gpu_ctx):
    """The device path equals the contract's pipeline (mvs_ref.depth + mvs_ref.fuse on dense.plan's
    matrices) bit for bit, every guaranteed-interior pixel of the step grid is emitted, and each point's z
    is 1 / (double)inv_depth of the reference's map: with B's last row (0, 0, 1) and c_z = 0 the product
    is exact.  The sub-plane offset moves inv_depth off w[k] by less than half a plane spacing, a tenth
    of w[k] here, so two maps agree within 0.23 relative: eps = 0.25 keeps every accepted pixel."""
    frames, K, rot, pos, sparse, k = planted_sequence()
    prm = dense.DenseParams(D=12, sources=1, radius=2, uniq=80, min_views=1, eps=0.25, min_consistent=1, step=4)
    pts, cols = dense.densify(frames, K, rot, pos, sparse, prm, ctx=gpu_ctx)
    P = dense.plan(frames[0].shape, K, rot, pos, sparse, prm)
    assert P["ref"] == [0, 1] and P["nbr"] == [[1], [0]]
    assert np.array_equal(P["M"][0, 0], np.eye(3).reshape(9)) and np.array_equal(P["v"][0, 0], [64.0, 0, 0])
    maps = [R.depth(frames[i], [frames[j] for j in P["src"][m]], P["M"][m, :1], P["v"][m, :1], P["planes"][m], 2, 80, 1)
            for m, i in enumerate(P["ref"])]
    want_p, want_c = R.fuse(frames, [m[2] for m in maps], P["nbr"], P["nbrM"], P["nbrv"], P["B"], P["c"], 0.25, 1, 4, 2)
    assert R.same_bits(pts, want_p) and R.same_bits(cols, want_c)
    h, w = frames[0].shape[:2]
    masks = R.fuse_masks([m[2] for m in maps], P["nbr"], P["nbrM"], P["nbrv"], 0.25, 1, 4, 2)
    n0 = 0
    for m in range(2):
        inv, wpl = maps[m][2], P["planes"][m]
        for y, x in zip(*np.nonzero(masks[m])):
            assert pts[n0][2] == 1.0 / np.float64(inv[y, x])
            n0 += 1
        for y in range(8, h - 6, 4):                   # the rows and columns the planted rule guarantees
            x0, x1 = ((6, w - 6 - k), (6 + k, w - 6))[m]
            for x in range(-(-x0 // 4) * 4, x1, 4):
                assert masks[m][y, x] and maps[m][0][y, x] == 4, (m, y, x)
                assert abs(np.float64(inv[y, x]) - wpl[4]) < 0.5 * (wpl[5] - wpl[4])
    assert n0 == len(pts)
    hp, hc = dense.densify(frames, K, rot, pos, sparse, prm, host=True)
    assert R.same_bits(hp, pts) and R.same_bits(hc, cols)


def test_slam_main_dense(gpu_ctx, tmp_path):
    from test_cycle import K_VGA, _cfg
    frames = slamhip.synth_frames(640, 480, 0, 16, seed=1234)
    cfg = _cfg()
    prm = dense.DenseParams(D=16, sources=2, step=16)
    outs = {}
    for name, dp in (("plain", None), ("dense", prm)):
        K = K_VGA.copy()
        gd, logs = cycle.slam_main(cycle.MediaSources(list(frames)), K, cfg, cycle.GpuOps(gpu_ctx), out_dir=str(tmp_path / name),
                                   dense=dp)
        outs[name] = (gd, logs, K)
    for f in ("poses.txt", "rotations.txt", "points.txt", "colors.txt"):
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "dense" / f).read_bytes(), f
    assert not (tmp_path / "plain" / "dense_points.txt").exists() and outs["plain"][1].frames is None
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
    assert len(scene.load_global_data(str(tmp_path / "dense")).spatialPoints) == len(gd.spatialPoints)

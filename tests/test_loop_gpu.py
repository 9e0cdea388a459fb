"""GPU tests of loop closing (csrc/loop.hip): every device output against the contract
(tests/loop_ref.py) by bits, between 64-element sentinels that must stay intact; the
staged host-pointer calls; every refusal on the device path.
"""
import ctypes

import numpy as np
import pytest

import loop_ref as R
from slamhip import _lib as L
from slamhip import loopclose as LC
from loop_checks import MIN_PAIRS, TAU, check_world, check_wrong_world, pgo_refusals, refusals

pytestmark = pytest.mark.gpu

GUARD = 64


def _guarded(torch, n, dtype, fill):
    """a device buffer of n elements between GUARD sentinels: (whole, payload view)"""
    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return t, t[GUARD:GUARD + n]


def _intact(t, n, fill):
    h = t.cpu()
    return bool((h[:GUARD] == fill).all()) and bool((h[GUARD + n:] == fill).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t.numel() else None


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


@pytest.mark.parametrize("name", R.RANSAC_NAMES)
def test_ransac_equals_reference(gpu_ctx, name):
    import torch
    a, b, off, c, H = R.ransac_cases()[name]
    sim, mask, count, status = R.ransac_expected(name)
    n, nl = len(a), len(off) - 1
    da, db = _dev(torch, a), _dev(torch, b)
    st, sp = _guarded(torch, 8 * nl, torch.float64, -7.0)
    mt, mp = _guarded(torch, n, torch.uint8, 0xA5)
    ct, cp = _guarded(torch, nl, torch.int32, -7)
    tt, tp = _guarded(torch, nl, torch.int32, -7)
    torch.cuda.synchronize()
    h = gpu_ctx.handle
    cen = np.ascontiguousarray(c, np.float64)
    L.check(L.lib().slam_sim3_ransac_dev(h, None, _p(da), _p(db), L.ptr(off), nl, L.ptr(cen), H, R.TAU, R.SEED, _p(sp), _p(mp),
                                         _p(cp), _p(tp)), h)
    assert R.same_bits(tp.cpu().numpy(), status), (name, tp.cpu().numpy(), status)
    assert R.same_bits(cp.cpu().numpy(), count), (name, cp.cpu().numpy(), count)
    assert R.same_bits(mp.cpu().numpy(), mask), name
    assert R.same_bits(sp.cpu().numpy().reshape(nl, 8), sim), (name, sp.cpu().numpy().reshape(nl, 8) - sim)
    assert _intact(st, 8 * nl, -7.0) and _intact(mt, n, 0xA5) and _intact(ct, nl, -7) and _intact(tt, nl, -7)
    # host arrays in give the same through the staged entry point
    got = LC.sim3_from_pairs(a, b, off, c, H, R.TAU, R.SEED, ctx=gpu_ctx)
    for w, g in zip((sim, mask, count, status), got):
        assert R.same_bits(g, w), name
    # and device tensors through the Python layer
    got = LC.sim3_from_pairs(da, db, off, c, H, R.TAU, R.SEED, ctx=gpu_ctx)
    for w, g in zip((sim, mask, count, status), got):
        assert R.same_bits(g.cpu().numpy(), w), name


def test_ransac_offsets_inside_a_larger_array(gpu_ctx):
    """offsets that start above 0 and stop short of the end: the other pairs' mask bytes stay"""
    import torch
    a, b, off, c = R.batch_case([10, 70])
    want = R.sim3_ransac(a, b, off, c, 32, R.TAU, R.SEED)
    pad = np.full((5, 3), np.nan)
    a2, b2 = np.concatenate([pad, a, pad]), np.concatenate([pad, b, pad])
    got = LC.sim3_from_pairs(a2, b2, off + 5, c, 32, R.TAU, R.SEED, ctx=gpu_ctx)
    assert R.same_bits(got[0], want[0]) and R.same_bits(got[1][5:-5], want[1]) and not got[1][:5].any() and not got[1][-5:].any()
    assert R.same_bits(got[2], want[2]) and R.same_bits(got[3], want[3])
    mask = torch.full((len(a2),), 0xA5, dtype=torch.uint8, device="cuda")
    sim = torch.zeros((2, 8), dtype=torch.float64, device="cuda")
    cs = torch.zeros(4, dtype=torch.int32, device="cuda")
    da, db = _dev(torch, a2), _dev(torch, b2)
    torch.cuda.synchronize()
    h = gpu_ctx.handle
    o5 = np.ascontiguousarray(off + 5, np.int32)
    cen = np.ascontiguousarray(c, np.float64)
    L.check(L.lib().slam_sim3_ransac_dev(h, None, _p(da), _p(db), L.ptr(o5), 2, L.ptr(cen), 32, R.TAU,
                                         R.SEED, _p(sim), _p(mask), _p(cs[:2]), _p(cs[2:])), h)
    m = mask.cpu().numpy()
    assert (m[:5] == 0xA5).all() and (m[-5:] == 0xA5).all() and R.same_bits(m[5:-5], want[1])


@pytest.mark.parametrize("n", R.APPLY_COUNTS)
def test_apply_points_equals_reference(gpu_ctx, n):
    import torch
    pts, anchor, nodes, new = R.apply_case(n)
    want = R.apply_points(pts, anchor, nodes, new)
    dp, da = _dev(torch, pts), _dev(torch, anchor)
    ot, op = _guarded(torch, 3 * n, torch.float64, -7.0)
    torch.cuda.synchronize()
    h = gpu_ctx.handle
    L.check(L.lib().slam_sim3_apply_points_dev(h, None, _p(dp), _p(da), n, L.ptr(nodes), L.ptr(new), len(nodes), _p(op)), h)
    assert R.same_bits(op.cpu().numpy().reshape(n, 3), want) and _intact(ot, 3 * n, -7.0)
    assert R.same_bits(LC.apply_points(pts, anchor, nodes, new, ctx=gpu_ctx), want)
    assert R.same_bits(LC.apply_points(dp, da, nodes, new, ctx=gpu_ctx).cpu().numpy(), want)
    # unchanged nodes: the points' own bits
    assert R.same_bits(LC.apply_points(pts, anchor, nodes, nodes, ctx=gpu_ctx), pts)
    if n:
        # an anchor outside the nodes in device memory keeps its point (the host-pointer call refuses it)
        wild = anchor.copy()
        wild[0] = 99
        got = LC.apply_points(dp, _dev(torch, wild), nodes, new, ctx=gpu_ctx).cpu().numpy()
        assert R.same_bits(got[0], pts[0]) and R.same_bits(got[1:], want[1:])


def test_refusals_device(gpu_ctx):
    import torch
    n = refusals(lambda a, b, off, c, H, tau: LC.sim3_from_pairs(a, b, off, c, H, tau, R.SEED, ctx=gpu_ctx),
                 lambda p, an, nd, nn: LC.apply_points(p, an, nd, nn, ctx=gpu_ctx))
    n += refusals(lambda a, b, off, c, H, tau: LC.sim3_from_pairs(_dev(torch, a), _dev(torch, b), off, c, H, tau, R.SEED, ctx=gpu_ctx),
                  lambda p, an, nd, nn: LC.apply_points(_dev(torch, p), _dev(torch, an), nd, nn, ctx=gpu_ctx))
    assert n == 26
    pts, anchor, nodes, new = R.apply_case(8)
    anchor[3] = 5
    with pytest.raises(L.SlamError) as e:
        LC.apply_points(pts, anchor, nodes, new, ctx=gpu_ctx)
    assert e.value.code == L.SLAM_E_INVALID_ARG
    sim, mask, count, status = LC.sim3_from_pairs(np.zeros((0, 3)), np.zeros((0, 3)), [0], np.zeros((0, 6)), 4, ctx=gpu_ctx)
    assert sim.shape == (0, 8) and len(mask) == 0


@pytest.mark.parametrize("name", R.PGO_NAMES)
def test_pgo_equals_reference(gpu_ctx, name):
    import torch
    S, e, m, w, ell, kw = R.pgo_cases()[name]
    want, cost, iters, _ = R.pgo_expected(name)
    n = len(S)
    nt, nodes = _guarded(torch, 8 * n, torch.float64, -7.0)
    nodes.copy_(torch.from_numpy(np.ascontiguousarray(S).reshape(-1)))
    torch.cuda.synchronize()
    h = gpu_ctx.handle
    k = dict(lambda0=1e-4, max_lm=10, max_pcg=200, pcg_tol=1e-12, cost_tol=1e-9)
    k.update(kw)
    c, it = np.zeros(2), np.zeros(3, np.int32)
    ed, ms, wt = np.ascontiguousarray(e, np.int32), np.ascontiguousarray(m, np.float64), np.ascontiguousarray(w, np.float64)
    L.check(L.lib().slam_pgo_sim3_dev(h, None, _p(nodes), n, L.ptr(ed), L.ptr(ms), L.ptr(wt), len(ed), ell, k["lambda0"],
                                      k["max_lm"], k["max_pcg"], k["pcg_tol"], k["cost_tol"], L.ptr(c), L.ptr(it)), h)
    got = nodes.cpu().numpy().reshape(n, 8)
    assert tuple(int(v) for v in it) == iters and (float(c[0]), float(c[1])) == cost, (name, it, iters, c, cost)
    assert R.same_bits(got, want), (name, np.abs(got - want).max())
    assert _intact(nt, 8 * n, -7.0)
    # host nodes through the staged call, device nodes through the Python layer
    g2 = LC.optimize_pose_graph(S, e, m, w, ell, ctx=gpu_ctx, **kw)
    assert R.same_bits(g2[0], want) and g2[1] == cost and g2[2] == iters
    g3 = LC.optimize_pose_graph(_dev(torch, S), e, m, w, ell, ctx=gpu_ctx, **kw)
    assert R.same_bits(g3[0].cpu().numpy(), want) and g3[1] == cost and g3[2] == iters


def test_pgo_stop_flag_between_reads(gpu_ctx):
    """the stop flag turns launched iterations into no-ops: a cap that is no multiple of the 8 iterations
    between two reads, and a tolerance met inside a chunk, give the reference's counts and bits"""
    S, e, m, w, ell, _ = R.pgo_cases()["double_loop"]
    for kw in (dict(max_lm=2, max_pcg=13, pcg_tol=1e-12), dict(max_lm=2, max_pcg=64, pcg_tol=1e-3), dict(max_lm=2, max_pcg=0)):
        want = R.pgo_sim3(S, e, m, w, ell, **kw)
        got = LC.optimize_pose_graph(S, e, m, w, ell, ctx=gpu_ctx, **kw)
        assert R.same_bits(got[0], want[0]) and got[1] == want[1] and got[2] == want[2], (kw, got[1:], want[1:])


def test_pgo_refusals_device(gpu_ctx):
    import torch
    assert pgo_refusals(lambda *a, **k: LC.optimize_pose_graph(*a, ctx=gpu_ctx, **k)) == 21
    assert pgo_refusals(lambda S, *a, **k: LC.optimize_pose_graph(_dev(torch, S), *a, ctx=gpu_ctx, **k)) == 21


def test_close_loops_on_a_synthetic_world(gpu_ctx):
    """the device run passes the host run's checks and equals it by bits"""
    def dev(W):
        return LC.close_loops(W["rotations"], W["motions"], W["points"], W["colors"], W["obs"], W["loops"], tau=TAU,
                              min_pairs=MIN_PAIRS, ctx=gpu_ctx)
    got = check_world(dev)
    W = R.world_case()
    want = LC.close_loops(W["rotations"], W["motions"], W["points"], W["colors"], W["obs"], W["loops"], tau=TAU,
                          min_pairs=MIN_PAIRS, host=True)
    for k in ("rotations", "motions", "points", "colors", "dropped", "nodes"):
        assert R.same_bits(got[k], want[k]), k
    assert got["costs"] == want["costs"] and got["iters"] == want["iters"]
    for a, b in zip(got["constraints"], want["constraints"]):
        assert R.same_bits(a["sim"], b["sim"]) and R.same_bits(a["mask"], b["mask"]) and a["count"] == b["count"]
    check_wrong_world(dev)


# ---- through slam_main ---------------------------------------------------------------------------------

def test_slam_main_closes_its_loops(gpu_ctx, tmp_path):
    """the 16-frame sequence of test_slam_main_with_loops: the four result files and loops.txt do not change
    with close=True; the closed files have the open files' rows minus the merged points and equal close_loops
    called by hand on the run's frames, observations and loops; without a loop they repeat the open files"""
    import os
    import slamhip
    from slamhip import cycle
    frames = slamhip.synth_frames(640, 480, 0, 16, seed=1234)
    d = slamhip.reference_example()
    d.update({"featureExtractingThreshold": 10, "requiredExtractedPointsCount": 2000, "framesBatchSize": 4,
              "requiredMatchedPointsCount": 300, "useFM-SIFT-FLANN": False, "useFM-SIFT-BF": True, "useFM-ORB": False,
              "useBundleAdjustment": False, "BAMaxFramesCnt": 4})
    cfg = slamhip.ConfigService(d)
    K0 = np.array([[1724.676 / 3, 0, 995.966 / 3], [0, 1730.482 / 3, 550.192 / 3], [0, 0, 1.0]])
    open_names = ("points.txt", "poses.txt", "rotations.txt", "colors.txt", "loops.txt")
    closed_names = ("poses_closed.txt", "rotations_closed.txt", "points_closed.txt", "colors_closed.txt")

    def run(out, prm):
        K = K0.copy()
        gd, logs = cycle.slam_main(cycle.MediaSources(list(frames)), K, cfg, cycle.GpuOps(gpu_ctx), out_dir=str(out), loops=prm)
        return gd, logs, K

    def read(out, names):
        return {n: open(os.path.join(out, n), "rb").read() for n in names}

    def rows(b):
        return len([r for r in b.decode().splitlines() if r])

    base = dict(K=1024, iters=3, gap=2, k=2, alpha=0.3, min_inliers=30)
    # 5 keyframes, gap 2: the "loops" join near neighbours, nothing has drifted, and a loop's pairs are map points
    # that tracking split in two.  They reach 3 .. 12 inliers of 300 .. 615 pairs, below the
    # default min_pairs of 30; 12 lets the strongest one through so that the accepted path (optimiser, moved points,
    # merged duplicates, corrected cameras) runs through slam_main as well
    low = 12
    g0, l0, _ = run(tmp_path / "open", slamhip.LoopParams(**base))
    g1, l1, K1 = run(tmp_path / "closed", slamhip.LoopParams(close=True, min_pairs=low, **base))
    f0, f1 = read(tmp_path / "open", open_names), read(tmp_path / "closed", open_names)
    assert f0 == f1 and rows(f0["poses.txt"]) >= 3
    assert l0.obs is None and not hasattr(g0, "closed") and not os.path.exists(tmp_path / "open" / "poses_closed.txt")
    # the observations: one set per logged frame, indices into the final points, positions of the frame's keypoints
    assert len(l1.obs) == len(l1.frames) == len(g1.cameraRotations)
    npts = len(g1.spatialPoints)
    for xy, idx in l1.obs:
        assert xy.dtype == np.float32 and xy.shape == (len(idx), 2) and idx.dtype == np.int64
        assert idx.max(initial=-1) < npts and idx.min(initial=-1) >= -1
    seen = np.unique(np.concatenate([idx[idx >= 0] for _, idx in l1.obs]))
    print("points", npts, "observed by a logged frame", len(seen))
    assert npts > 0 and len(seen) == npts           # every map point was born in a logged frame
    c = g1.closed
    fc = read(tmp_path / "closed", closed_names)
    print("loops", [(l[0], l[1], l[4]) for l in g1.loops], "constraints",
          [(k["i"], k["j"], len(k["ia"]), k["count"], k["status"], k["accepted"]) for k in c["constraints"]], "dropped", len(c["dropped"]))
    assert rows(fc["poses_closed.txt"]) == rows(f1["poses.txt"]) and rows(fc["rotations_closed.txt"]) == rows(f1["rotations.txt"])
    assert rows(fc["points_closed.txt"]) == rows(f1["points.txt"]) - len(c["dropped"]) == rows(fc["colors_closed.txt"])
    # by hand
    cond, ops = cycle.Conditions(cfg), cycle.GpuOps(gpu_ctx)
    matches = LC.loop_matches(l1.frames, g1.loops, cond, ops)
    want = LC.close_loops(g1.cameraRotations, [np.reshape(t, 3) for t in g1.spatialCameraPositions], g1.spatialPoints,
                          g1.spatialPointsColors, l1.obs, matches, min_pairs=low, ctx=gpu_ctx)
    assert len(want["constraints"]) == len(g1.loops)
    for k in ("rotations", "motions", "points", "colors", "dropped"):
        assert R.same_bits(c[k], np.asarray(want[k], c[k].dtype)), k
    # the default bar accepts none of these and returns the run's own result
    dflt = LC.close_loops(g1.cameraRotations, [np.reshape(t, 3) for t in g1.spatialCameraPositions], g1.spatialPoints,
                          g1.spatialPointsColors, l1.obs, matches, ctx=gpu_ctx)
    assert not any(k["accepted"] for k in dflt["constraints"]) and R.same_bits(dflt["points"], np.asarray(g1.spatialPoints, np.float64))
    # every constraint pairs two different map points that both frames really observe
    for k in c["constraints"]:
        assert np.isin(k["ia"], l1.obs[k["i"]][1]).all() and np.isin(k["ib"], l1.obs[k["j"]][1]).all()
    # no loop kept (an inlier bar nothing reaches): the closed files repeat the open ones exactly
    g2, l2, _ = run(tmp_path / "none", slamhip.LoopParams(close=True, **dict(base, min_inliers=10 ** 9)))
    assert g2.loops == [] and len(g2.closed["dropped"]) == 0
    f2, fc2 = read(tmp_path / "none", open_names), read(tmp_path / "none", closed_names)
    assert f2["loops.txt"] == b"" and all(f2[n] == f0[n] for n in open_names[:4])
    for n in ("poses", "rotations", "points", "colors"):
        assert fc2[n + "_closed.txt"] == f2[n + ".txt"], n
    with pytest.raises(ValueError):
        cycle.slam_main(cycle.MediaSources(list(frames)), K0.copy(), cfg, cycle.GpuOps(gpu_ctx), loops=slamhip.LoopParams(close=True, **base),
                        tracker="klt")

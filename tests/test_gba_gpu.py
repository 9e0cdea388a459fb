"""GPU tests of global bundle adjustment (csrc/gba.hip): slam_gba_dev against the contract (tests/gba_ref.py) by
bits on every named case, between 64-element sentinels that must stay intact; the staged call and the Python
layer with host arrays and with device tensors; the stop flag; every refusal on the device path; the synthetic
world; the switch through slam_main.
"""
import ctypes

import numpy as np
import pytest

import gba_ref as R
from gba_checks import REFUSALS, WORLD_K, check_case, check_world, closed_world, gba_refusals
from slamhip import _lib as L
from slamhip import globalba as G
from slamhip import loopclose as LC

pytestmark = pytest.mark.gpu

GUARD = 64


def _guarded(torch, values, fill):
    """a device buffer holding values between GUARD sentinels: (whole, payload view)"""
    n = values.size
    t = torch.full((n + 2 * GUARD,), fill, dtype=torch.float64, device="cuda")
    if n:
        t[GUARD:GUARD + n].copy_(torch.from_numpy(np.ascontiguousarray(values).reshape(-1)))
    return t, t[GUARD:GUARD + n]


def _intact(t, n, fill):
    h = t.cpu()
    return bool((h[:GUARD] == fill).all()) and bool((h[GUARD + n:] == fill).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t.numel() else None


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


@pytest.mark.parametrize("name", R.GBA_NAMES)
def test_device_equals_reference(gpu_ctx, name):
    import torch
    W, kw = R.gba_cases()[name]
    C, X, want, _ = R.gba_expected(name)
    n, m = len(C), len(X)
    ct, cp = _guarded(torch, W["cams"], -7.0)
    xt, xp = _guarded(torch, W["points"], -7.0)
    k = dict(R.DEFAULTS, **kw)
    prm = L.GbaParams(k["loss"], k["loss_param"], k["zmin"], k["lambda0"], k["max_lm"], k["max_pcg"], k["pcg_tol"], k["cost_tol"])
    out = L.GbaSummary()
    K4 = np.array(W["K"], np.float64)
    oc, op, xy = (np.ascontiguousarray(W["obs_cam"], np.int32), np.ascontiguousarray(W["obs_point"], np.int32),
                  np.ascontiguousarray(W["obs_xy"], np.float64))
    torch.cuda.synchronize()
    h = gpu_ctx.handle
    L.check(L.lib().slam_gba_dev(h, None, L.ptr(K4), _p(cp), n, _p(xp), m, L.ptr(oc), L.ptr(op), L.ptr(xy), len(oc),
                                 ctypes.byref(prm), ctypes.byref(out)), h)
    got = {f: getattr(out, f) for f in R.SUMMARY}
    assert got == want, (name, got, want)
    assert R.same_bits(cp.cpu().numpy().reshape(n, 7), C), name
    assert R.same_bits(xp.cpu().numpy().reshape(m, 3), X), name
    assert _intact(ct, 7 * n, -7.0) and _intact(xt, 3 * m, -7.0)
    # host arrays through the staged call, then through device tensors of the Python layer's own
    check_case(name, lambda *a, **q: G.solve(*a, ctx=gpu_ctx, **q))
    check_case(name, lambda *a, **q: G.solve(*a, ctx=gpu_ctx, staged=False, **q))

    def tensors(K, cams, pts, *a, **q):
        c, p, s = G.solve(K, _dev(torch, cams), _dev(torch, pts), *a, ctx=gpu_ctx, **q)
        return c.cpu().numpy(), p.cpu().numpy(), s
    check_case(name, tensors)


def test_stop_flag_between_reads(gpu_ctx):
    """the stop flag turns launched iterations into no-ops: no iteration at all, a cap that is no multiple of the 8
    iterations between two reads, and a tolerance met inside a chunk give the reference's counts and bits; so does a
    tolerance met exactly when a chunk ends or later"""
    for name in ("pcg0", "pcg13", "pcg_loose"):
        check_case(name, lambda *a, **q: G.solve(*a, ctx=gpu_ctx, **q))
    W, _ = R.gba_cases()["pcg13"]
    for kw in (dict(max_lm=2, max_pcg=8, pcg_tol=0.0), dict(max_lm=2, max_pcg=64, pcg_tol=1e-6), dict(max_lm=1, max_pcg=1)):
        C, X, s = R.gba(W["K"], W["cams"], W["points"], W["obs_cam"], W["obs_point"], W["obs_xy"], **kw)
        c, p, s2 = G.solve(W["K"], W["cams"], W["points"], W["obs_cam"], W["obs_point"], W["obs_xy"], ctx=gpu_ctx, **kw)
        assert s2 == s and R.same_bits(c, C) and R.same_bits(p, X), (kw, s2, s)


def test_refusals_device(gpu_ctx):
    import torch
    assert gba_refusals(lambda *a, **k: G.solve(*a, ctx=gpu_ctx, **k)) == REFUSALS
    assert gba_refusals(lambda K, c, p, *a, **k: G.solve(K, _dev(torch, c), _dev(torch, p), *a, ctx=gpu_ctx, **k)) == REFUSALS
    # a refused call leaves the device arrays alone
    W, _ = R.gba_cases()["lists"]
    dc, dp = _dev(torch, W["cams"]), _dev(torch, W["points"])
    with pytest.raises(L.SlamError):
        G.solve(W["K"], dc, dp, W["obs_cam"], W["obs_point"], W["obs_xy"], ctx=gpu_ctx, zmin=0.0)
    assert R.same_bits(dc.cpu().numpy(), W["cams"]) and R.same_bits(dp.cpu().numpy(), W["points"])


def test_world_is_refined(gpu_ctx):
    """the device run passes the host run's checks and equals it by bits, with host arrays and with device tensors"""
    import torch
    rot, mot, pts, s = check_world(lambda K, r, t, p, obs: G.global_bundle_adjust(K, r, t, p, obs, ctx=gpu_ctx))
    W, closed, obs2 = closed_world()
    want = G.global_bundle_adjust(WORLD_K, closed["rotations"], closed["motions"], closed["points"], obs2, host=True)
    for g, w in zip((rot, mot, pts), want[:3]):
        assert R.same_bits(g, w)
    assert s == want[3]
    got = G.global_bundle_adjust(WORLD_K, _dev(torch, closed["rotations"]), _dev(torch, closed["motions"]), _dev(torch, closed["points"]),
                                 obs2, ctx=gpu_ctx)
    for g, w in zip(got[:3], want[:3]):
        assert R.same_bits(g.cpu().numpy(), w)
    assert got[3] == want[3]
    import slamhip
    Ww, cw, _ = closed_world(wrong=True)
    res = G.refine_closed(cw, Ww["obs"], WORLD_K, slamhip.LoopParams(close=True, global_ba=True), ctx=gpu_ctx)
    for k in ("rotations", "motions", "points", "colors"):
        assert R.same_bits(res[k], cw[k]), k


# ---- through slam_main ---------------------------------------------------------------------------------

def test_slam_main_refines_its_closed_map(gpu_ctx, tmp_path):
    """the 16-frame sequence of test_slam_main_closes_its_loops with min_pairs=12: with global_ba=True the four result
    files, loops.txt and the four closed files do not change; the refined files equal refine_closed called by hand on
    the run's closed map and observations; their reprojection RMS is not above the closed one; without an accepted loop
    they repeat the closed files"""
    import os
    import slamhip
    from slamhip import cycle, scene
    frames = slamhip.synth_frames(640, 480, 0, 16, seed=1234)
    d = slamhip.reference_example()
    d.update({"featureExtractingThreshold": 10, "requiredExtractedPointsCount": 2000, "framesBatchSize": 4,
              "requiredMatchedPointsCount": 300, "useFM-SIFT-FLANN": False, "useFM-SIFT-BF": True, "useFM-ORB": False,
              "useBundleAdjustment": False, "BAMaxFramesCnt": 4})
    cfg = slamhip.ConfigService(d)
    K0 = np.array([[1724.676 / 3, 0, 995.966 / 3], [0, 1730.482 / 3, 550.192 / 3], [0, 0, 1.0]])
    kept_names = ("points.txt", "poses.txt", "rotations.txt", "colors.txt", "loops.txt", "poses_closed.txt", "rotations_closed.txt",
                  "points_closed.txt", "colors_closed.txt")
    stems = ("poses", "rotations", "points", "colors")

    def run(out, prm):
        K = K0.copy()
        gd, logs = cycle.slam_main(cycle.MediaSources(list(frames)), K, cfg, cycle.GpuOps(gpu_ctx), out_dir=str(out), loops=prm)
        return gd, logs, K

    def read(out, names):
        return {n: open(os.path.join(out, n), "rb").read() for n in names}

    base = dict(K=1024, iters=3, gap=2, k=2, alpha=0.3, min_inliers=30)
    g0, l0, _ = run(tmp_path / "closed", slamhip.LoopParams(close=True, min_pairs=12, **base))
    g1, l1, K1 = run(tmp_path / "refined", slamhip.LoopParams(close=True, global_ba=True, min_pairs=12, **base))
    assert read(tmp_path / "closed", kept_names) == read(tmp_path / "refined", kept_names)
    assert not hasattr(g0, "refined") and not os.path.exists(tmp_path / "closed" / "poses_refined.txt")
    assert any(c["accepted"] for c in g1.closed["constraints"])
    for k in ("rotations", "motions", "points", "colors", "dropped"):
        assert R.same_bits(g1.closed[k], g0.closed[k]), k
    # by hand
    prm = slamhip.LoopParams(close=True, global_ba=True, min_pairs=12, **base)
    want = G.refine_closed(g1.closed, l1.obs, K1, prm, ctx=gpu_ctx)
    for k in ("rotations", "motions", "points", "colors"):
        assert R.same_bits(g1.refined[k], want[k]), k
    s = g1.refined["summary"]
    assert s == want["summary"] and s["kept_obs"] > 0 and s["cost"] <= s["cost0"]
    print("refined:", s, "rms", np.sqrt(s["cost0"] / s["kept_obs"]), "->", np.sqrt(s["cost"] / s["kept_obs"]))
    # the files hold the refined rows in rawOutput's format
    fr = read(tmp_path / "refined", [n + "_refined.txt" for n in stems])
    fc = read(tmp_path / "refined", [n + "_closed.txt" for n in stems])
    for stem in stems:      # as many rows as the closed file: the same cameras, the same merged cloud
        assert len(fr[stem + "_refined.txt"].splitlines()) == len(fc[stem + "_closed.txt"].splitlines()) > 0, stem
    assert fr["points_refined.txt"] != fc["points_closed.txt"] and fr["colors_refined.txt"] == fc["colors_closed.txt"]
    gd = scene.load_global_data(str(tmp_path / "refined"), cloud="refined")
    assert np.allclose(gd.spatialPoints, g1.refined["points"], rtol=0, atol=1e-9 * max(1.0, float(np.abs(g1.refined["points"]).max())))
    # no loop kept: the refined files repeat the closed ones exactly
    g2, l2, _ = run(tmp_path / "none", slamhip.LoopParams(close=True, global_ba=True, **dict(base, min_inliers=10 ** 9)))
    assert g2.loops == [] and g2.refined["summary"] is None
    f2 = read(tmp_path / "none", [n + s_ + ".txt" for n in stems for s_ in ("_closed", "_refined")])
    for n in stems:
        assert f2[n + "_refined.txt"] == f2[n + "_closed.txt"], n
    with pytest.raises(ValueError):
        cycle.slam_main(cycle.MediaSources(list(frames)), K0.copy(), cfg, cycle.GpuOps(gpu_ctx), loops=slamhip.LoopParams(global_ba=True, **base))

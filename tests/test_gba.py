"""CPU tests of global bundle adjustment: known behaviour of the contract (tests/gba_ref.py), the host twin
against it bit for bit on every named case, the Jacobians against central differences, argument errors, the
synthetic world end to end, the observation merge, and the twin under AddressSanitizer + UBSan as a stand-alone
program (tests/cpp/gba_host_test.cpp).  No GPU.
"""
import os
import subprocess

import numpy as np
import pytest

import gba_ref as R
from gba_checks import REFUSALS, WORLD_K, check_case, check_world, closed_world, gba_refusals
from slamhip import globalba as G
from slamhip import loopclose as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _twin(*a, **k):
    return G.solve(*a, host=True, **k)


# ---- the reference's own behaviour ----------------------------------------------------------------------

def test_reference_known_behaviour():
    exp = {name: R.gba_expected(name) for name in R.GBA_NAMES}
    for name in ("tree", "lists", "repeat", "two", "behind", "many", "huber", "reject"):
        s = exp[name][2]
        assert s["cost"] < s["cost0"] and s["accepted"] >= 1, name
    # counts of the plan
    W, _ = R.gba_cases()["tree"]
    P = R.Plan(W["cams"], W["points"], W["obs_cam"], W["obs_point"], W["obs_xy"], 0.1)
    assert P.cam_cnt.tolist() == [129, 0, 1, 63, 64, 65, 129] and exp["tree"][2]["cams_held"] == 2
    W, _ = R.gba_cases()["lists"]
    P = R.Plan(W["cams"], W["points"], W["obs_cam"], W["obs_point"], W["obs_xy"], 0.1)
    assert P.pt_cnt.min() == 2 and P.pt_cnt.max() == 5 == P.n
    W, _ = R.gba_cases()["repeat"]
    assert int(((W["obs_cam"] == 2) & (W["obs_point"] == 1)).sum()) == 3 and exp["repeat"][2]["kept_obs"] == len(W["obs_cam"])
    # two stages of the exclusion: two observations behind camera 3, then point 1's last one goes, uncounted
    s = exp["behind"][2]
    W, _ = R.gba_cases()["behind"]
    assert (s["behind_obs"], s["points_held"], s["cams_held"], s["kept_obs"]) == (2, 1, 2, len(W["obs_cam"]) - 3)
    assert R.same_bits(exp["behind"][1][1], W["points"][1]) and R.same_bits(exp["behind"][0][3], W["cams"][3])
    assert not R.same_bits(exp["behind"][1][0], W["points"][0])
    # nothing to do
    for name in ("one", "empty", "lm0"):
        W, _ = R.gba_cases()[name]
        C, X, s, tr = exp[name]
        assert R.same_bits(C, W["cams"]) and R.same_bits(X, W["points"]) and s["lm_steps"] == 0 and s["cost"] == s["cost0"] and tr == []
    assert exp["one"][2]["cost0"] == 0.0 and exp["lm0"][2]["cost0"] > 0.0
    # camera 0 never moves
    for name in R.GBA_NAMES:
        assert R.same_bits(exp[name][0][0], R.gba_cases()[name][0]["cams"][0]), name
    # two parallel rays: without damping the rank-2 block has no Cholesky factor and the point is frozen for that step;
    # with damping it is solved
    assert exp["parallel_l0"][3][0][4] == 1 and all(t[4] == 0 for t in exp["parallel"][3])
    assert len(R.gba_cases()["many"][0]["cams"]) > R.PCG_LANES
    # a rejected step: lambda rises tenfold and the state stays
    tr = exp["huber_off"][3]
    k = [t[2] for t in tr].index(False)
    assert tr[k + 1][0] == tr[k][0] * 10.0 and not exp["reject"][3][-1][2]
    assert any(not t[2] for t in exp["reject"][3])
    # a trial that brings a kept observation to z_c <= zmin costs +inf and is rejected; no observation ends there
    tr = exp["zreject"][3]
    assert np.isinf(tr[0][1]) and not tr[0][2] and tr[1][2] and exp["zreject"][2]["behind_obs"] == 0
    W, kw = R.gba_cases()["zreject"]
    assert (R.residuals(W["K"], exp["zreject"][0], exp["zreject"][1], W["obs_cam"], W["obs_point"], W["obs_xy"])[1] > kw["zmin"]).all()
    # the caps: none, one that is no multiple of the 8 iterations between two reads, a tolerance met inside a chunk
    assert [t[3] for t in exp["pcg0"][3]] == [0, 0] and [t[3] for t in exp["pcg13"][3]] == [13, 13]
    assert all(0 < t[3] < 8 for t in exp["pcg_loose"][3])
    # Huber: the outliers pull the plain fit away from the true cameras, the robust one much less
    W, _ = R.gba_cases()["huber"]
    err = [float(np.abs(exp[n][0][:, 4:] - W["gt_cams"][:, 4:]).max()) for n in ("huber", "huber_off")]
    print("camera translation error: Huber", err[0], "squares", err[1])
    assert err[0] < err[1]


def test_jacobians_match_central_differences():
    """analytic Jacobians against central differences with h = 1e-6 on unit-scale cases (focal lengths near 1, depths
    2 to 4): within 1e-6 absolute, the bound test_loop.py uses for pgo_edge (truncation h^2 / 6 times a third
    derivative of order one, plus the rounding eps / h of that step)"""
    rng = np.random.default_rng(0)
    h, worst = 1e-6, 0.0
    K = (1.2, 0.9, 0.1, -0.05)
    for _ in range(25):
        cam = np.concatenate([R._quat(rng, 1.0), rng.uniform(-0.5, 0.5, 3)])[None]
        X = np.array([[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 4)]])
        xy = rng.uniform(-0.5, 0.5, (1, 2))
        no = np.array([False])
        _, _, Jc, Jp = R.obs_lin(cam, X, K, xy, 0, 1.0, 0.1, no)
        res = lambda c, x: R.obs_lin(c, x, K, xy, 0, 1.0, 0.1, no)[0][0]
        for c in range(6):
            d = np.zeros((1, 6))
            d[0, c] = h
            fd = (res(R.cam_step(cam, d), X) - res(R.cam_step(cam, -d), X)) / (2 * h)
            worst = max(worst, float(np.abs(Jc[0, :, c] - fd).max()))
        for c in range(3):
            d = np.zeros((1, 3))
            d[0, c] = h
            fd = (res(cam, X + d) - res(cam, X - d)) / (2 * h)
            worst = max(worst, float(np.abs(Jp[0, :, c] - fd).max()))
    print("worst Jacobian difference", worst)
    assert worst <= 1e-6
    # a held camera's Jacobian is 0, its point's is not; Huber scales r and J by sqrt(rho') and keeps rho = 2 a sqrt(s) - a^2
    r, rho, Jc, Jp = R.obs_lin(cam, X, K, xy, 0, 1.0, 0.1, np.array([True]))
    assert not Jc.any() and Jp.any()
    far = xy + 3.0
    r0, rho0, _, Jp0 = R.obs_lin(cam, X, K, far, 0, 1.0, 0.1, no)
    r1, rho1, _, Jp1 = R.obs_lin(cam, X, K, far, 1, 0.5, 0.1, no)
    s = float(rho0[0])
    w = np.sqrt(0.5 / np.sqrt(s))
    assert s > 0.25 and rho1[0] == (2.0 * 0.5) * np.sqrt(s) - 0.25 and R.same_bits(r1, w * r0) and R.same_bits(Jp1, w * Jp0)
    # behind the camera: the cost is +inf
    assert np.isinf(R.obs_lin(cam, X - np.array([[0, 0, 50.0]]), K, xy, 0, 1.0, 0.1, no)[1][0])


# ---- the host twin against the reference, by bits -------------------------------------------------------

@pytest.mark.parametrize("name", R.GBA_NAMES)
def test_twin_equals_reference(name):
    check_case(name, _twin)


def test_refusals_host():
    assert gba_refusals(_twin) == REFUSALS


# ---- the Python layer -----------------------------------------------------------------------------------

def test_global_bundle_adjust_wraps_the_solve():
    W, kw = R.gba_cases()["lists"]
    n, m = len(W["cams"]), len(W["points"])
    rot = np.array([np.array(LC.quat_matrix(c[:4])) for c in W["cams"]])
    obs = []
    for k in range(n):
        sel = W["obs_cam"] == k
        # an index of -1 and one past the end are no observations
        obs.append((np.concatenate([W["obs_xy"][sel], [[1.0, 2.0], [3.0, 4.0]]]).astype(np.float32),
                    np.concatenate([W["obs_point"][sel], [-1, m]]).astype(np.int64)))
    r2, m2, p2, s = G.global_bundle_adjust(np.array([[W["K"][0], 0, W["K"][2]], [0, W["K"][1], W["K"][3]], [0, 0, 1]]), rot,
                                           W["cams"][:, 4:], W["points"], obs, host=True, **kw)
    cams = np.array([np.concatenate([LC.matrix_quat(R_), t]) for R_, t in zip(rot, W["cams"][:, 4:])])
    oc, op, xy = G.flatten_observations(obs, m)
    assert len(oc) == len(W["obs_cam"])
    C, X, want = R.gba(W["K"], cams, W["points"], oc, op, xy, **kw)
    assert s == want and R.same_bits(p2, X) and R.same_bits(m2, C[:, 4:])
    assert R.same_bits(r2[1:], np.array([np.array(LC.quat_matrix(c[:4])) for c in C[1:]])) and R.same_bits(r2[0], rot[0])
    assert s["cost"] < s["cost0"]
    with pytest.raises(ValueError):
        G.global_bundle_adjust(W["K"], rot, W["cams"][:2, 4:], W["points"], obs, host=True)


def test_merge_observations_follows_the_chain():
    """6 points, merges 5 -> 3 -> 1 (a chain, given out of order) and 4 -> 2; 0 is untouched.  The dropped indices 3, 4, 5
    go to the roots 1, 2, 1, and the kept 0, 1, 2 are compacted to 0, 1, 2"""
    cons = [{"accepted": True, "ia": np.array([5, 4]), "ib": np.array([3, 2]), "mask": np.array([True, True])},
            {"accepted": True, "ia": np.array([3, 0]), "ib": np.array([1, 5]), "mask": np.array([True, False])},
            {"accepted": False, "ia": np.array([0]), "ib": np.array([2]), "mask": np.array([True])}]
    root = LC.merged_roots(6, cons)
    assert root.tolist() == [0, 1, 2, 1, 2, 1]
    dropped = np.array([3, 4, 5])
    xy = np.arange(14, dtype=np.float32).reshape(7, 2)
    obs = [(xy, np.array([0, 1, 2, 3, 4, 5, -1])), (xy[:3], np.array([5, 3, 9]))]
    out = G.merge_observations(obs, 6, cons, dropped)
    assert out[0][1].tolist() == [0, 1, 2, 1, 2, 1, -1] and out[1][1].tolist() == [1, 1, -1]      # both copies stay
    assert out[0][0] is xy
    # a gap in the kept indices is compacted: points 1 and 2 merged, 3 .. 5 shift down
    cons = [{"accepted": True, "ia": np.array([2]), "ib": np.array([1]), "mask": np.array([True])}]
    out = G.merge_observations([(xy[:6], np.arange(6))], 6, cons, np.array([2]))
    assert out[0][1].tolist() == [0, 1, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        G.merge_observations(obs, 6, cons, dropped)


def test_world_is_refined_host():
    import slamhip
    rot, mot, pts, s = check_world(lambda K, r, t, p, obs: G.global_bundle_adjust(K, r, t, p, obs, host=True))
    W, closed, obs2 = closed_world()
    # refine_closed is the same call with LoopParams' settings
    res = G.refine_closed(closed, W["obs"], WORLD_K, slamhip.LoopParams(close=True, global_ba=True), host=True)
    assert R.same_bits(res["points"], pts) and R.same_bits(res["rotations"], rot) and R.same_bits(res["motions"], mot)
    assert res["summary"] == s and np.array_equal(res["colors"], closed["colors"])
    # and the twin's solve is the reference's
    cams = np.array([np.concatenate([LC.matrix_quat(r), t]) for r, t in zip(closed["rotations"], closed["motions"])])
    oc, op, xy = G.flatten_observations(obs2, len(closed["points"]))
    C, X, want = R.gba(G._k4(WORLD_K), cams, closed["points"], oc, op, xy)
    assert want == s and R.same_bits(X, pts) and R.same_bits(C[:, 4:], mot)
    # no accepted loop: the closed result by bits
    Ww, cw, _ = closed_world(wrong=True)
    res = G.refine_closed(cw, Ww["obs"], WORLD_K, slamhip.LoopParams(close=True, global_ba=True), host=True)
    for k in ("rotations", "motions", "points", "colors"):
        assert R.same_bits(res[k], cw[k]), k
    assert res["summary"] is None


def test_switch_parameters_and_reload(tmp_path):
    import slamhip
    from slamhip import cycle, scene
    p = slamhip.LoopParams()
    assert p.global_ba is False and (p.gba_loss, p.gba_loss_param, p.gba_max_lm, p.gba_max_pcg, p.gba_zmin) == (0, 1.0, 10, 200, 0.1)
    with pytest.raises(ValueError):
        cycle.slam_main(None, None, None, loops=slamhip.LoopParams(global_ba=True))
    W, closed, _ = closed_world()
    for name, rows in (("poses", closed["motions"]), ("rotations", closed["rotations"]), ("points", closed["points"]),
                       ("colors", closed["colors"])):
        with open(tmp_path / (name + "_refined.txt"), "w") as f:
            for r in rows:
                cycle.raw_output(r, f)
    gd = scene.load_global_data(str(tmp_path), cloud="refined")
    assert len(gd.spatialPoints) == len(closed["points"]) and len(gd.cameraRotations) == 40
    assert np.allclose(gd.spatialPoints, closed["points"], rtol=0, atol=1e-11)


# ---- the twin under ASan + UBSan, as a stand-alone program ----------------------------------------------

def test_host_twin_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "slam-indoor-code_amd", "csrc")
    exe = str(tmp_path / "gba_host_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", os.path.join(ROOT, "tests", "cpp", "gba_host_test.cpp"), os.path.join(csrc, "gba_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines()[-1].startswith("OK: ")

"""CPU tests of loop closing: known answers for the contract (tests/loop_ref.py), the host
twins against it bit for bit, argument errors, and the twins under AddressSanitizer +
UBSan as a stand-alone program (tests/cpp/loop_host_test.cpp).  No GPU.
"""
import os
import subprocess

import numpy as np
import pytest

import loop_ref as R
from slamhip import _lib as L
from slamhip import loopclose as LC
from loop_checks import MIN_PAIRS, TAU, check_world, check_wrong_world, pgo_refusals, refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(S, T, tol):
    """similarities equal up to the quaternion's sign"""
    S, T = np.array(S, np.float64), np.array(T, np.float64)
    if np.dot(S[1:5], T[1:5]) < 0:
        T = T.copy()
        T[1:5] = -T[1:5]
    return float(np.abs(S - T).max()) <= tol


# ---- the reference's own algebra ---------------------------------------------------------------

def test_similarity_algebra():
    rng = np.random.default_rng(1)
    for _ in range(10):
        A, B = R.random_sim(rng), R.random_sim(rng)
        x = tuple(rng.uniform(-3, 3, 3))
        # compose applies B first; inverse undoes; a few ulps of unit-scale values
        assert np.allclose(R.apply(R.compose(A, B), x), R.apply(A, R.apply(B, x)), rtol=0, atol=1e-13)
        assert np.allclose(R.apply(R.inverse(A), R.apply(A, x)), x, rtol=0, atol=1e-13)
        assert _close(R.compose(A, R.inverse(A)), R.IDENTITY, 1e-13)
        assert np.allclose(np.array(R.quat_matrix(R.matrix_quat(R.quat_matrix(A[1:5])))), R.quat_matrix(A[1:5]), atol=1e-14)


def test_samples_are_three_distinct_indices():
    for n in (3, 4, 5, 64, 1000):
        seen = set()
        for h in range(200):
            s = R.sample(R.SEED, 2, h, n)
            assert len(set(s)) == 3 and all(0 <= i < n for i in s)
            seen.update(s)
        assert len(seen) == min(n, len(seen)) and (n > 5 or seen == set(range(n)))
    # a counter-based generator: a draw depends on (seed, loop, hypothesis) alone
    assert R.sample(1, 0, 0, 100) != R.sample(2, 0, 0, 100) or R.sample(1, 0, 1, 100) != R.sample(2, 0, 1, 100)
    assert R.sample(9, 3, 7, 50) == R.sample(9, 3, 7, 50)


def test_hypothesis_maps_its_triangle():
    a, b, _, S = R.pairs_case(11, 3, noise=0.0)
    Hs = R.hypothesis(a[0], a[1], a[2], b[0], b[1], b[2])
    assert _close(Hs, S, 1e-12)
    # collinear and repeated points give no frame
    assert R.hypothesis(a[0], a[0], a[2], b[0], b[1], b[2]) is None
    assert R.hypothesis(a[0], a[1], a[2], b[0], 2 * b[1] - b[0], b[1]) is None


def test_exact_recovery():
    """noise-free pairs of an exactly representable similarity: it comes back (to the rounding of the
    sqrt-normalised triangle frames and four Gauss-Newton steps, far below 1e-12) with every pair in"""
    a, b, c, S = R.exact_case()
    sim, mask, count, status = R.ransac_expected("exact")
    assert status[0] == R.OK and count[0] == len(a) and mask.all()
    assert _close(sim[0], S, 1e-12)


def test_outliers_are_masked():
    a, b, c, S = R.pairs_case(257, 257, 0.5)
    sim, mask, count, status = R.ransac_expected("n257_h64")
    true_in = np.linalg.norm(b - np.stack(R.apply(S, R._cols(a)), axis=1), axis=1) < 0.02
    assert status[0] == R.OK and count[0] == mask.sum() and np.array_equal(mask.astype(bool), true_in)
    assert _close(sim[0], S, 1e-3)


def test_special_statuses():
    assert R.ransac_expected("collinear")[3][0] == R.NO_MODEL
    assert R.ransac_expected("one_point")[3][0] == R.NO_MODEL
    sim, mask, count, status = R.ransac_expected("batch3_two")
    assert status.tolist() == [R.OK, R.TOO_FEW, R.OK] and count[1] == 0 and tuple(sim[1]) == R.IDENTITY
    sim, mask, count, status = R.ransac_expected("batch3_empty")
    assert status.tolist() == [R.OK, R.TOO_FEW, R.OK] and tuple(sim[1]) == R.IDENTITY
    sim, mask, count, status = R.ransac_expected("duplicates")
    assert status[0] == R.OK and count[0] == 40


def test_tie_goes_to_the_lower_hypothesis():
    """4 clean pairs: hypotheses 0 and 1 come from different triangles and both hold all 4 pairs, so
    the call with two hypotheses must return what the call with hypothesis 0 alone returns"""
    a, b, c, _ = R.pairs_case(4, 4)
    off = np.array([0, 4], np.int32)
    assert set(R.sample(R.SEED, 0, 0, 4)) != set(R.sample(R.SEED, 0, 1, 4))
    one = R.sim3_ransac(a, b, off, c, 1, R.TAU, R.SEED)
    two = R.sim3_ransac(a, b, off, c, 2, R.TAU, R.SEED)
    only1 = R.hypothesis(*[a[i] for i in R.sample(R.SEED, 0, 1, 4)], *[b[i] for i in R.sample(R.SEED, 0, 1, 4)])
    only0 = R.hypothesis(*[a[i] for i in R.sample(R.SEED, 0, 0, 4)], *[b[i] for i in R.sample(R.SEED, 0, 0, 4)])
    assert only0 != only1 and one[2][0] == 4 and two[2][0] == 4
    assert all(R.same_bits(x, y) for x, y in zip(one, two))
    g1 = LC.sim3_from_pairs(a, b, off, c, 1, R.TAU, R.SEED, host=True)
    g2 = LC.sim3_from_pairs(a, b, off, c, 2, R.TAU, R.SEED, host=True)
    assert all(R.same_bits(x, y) for x, y in zip(g1, g2)) and R.same_bits(g1[0], one[0])
    # the same two calls are cases of ransac_cases(), so the device runs them too (test_loop_gpu.py)
    assert all(R.same_bits(x, y) for x, y in zip(R.ransac_expected("tie_h1"), R.ransac_expected("tie_h2")))


# ---- the host twins against the reference, by bits ------------------------------------------------

@pytest.mark.parametrize("name", R.RANSAC_NAMES)
def test_ransac_twin_equals_reference(name):
    a, b, off, c, H = R.ransac_cases()[name]
    want = R.ransac_expected(name)
    got = LC.sim3_from_pairs(a, b, off, c, H, R.TAU, R.SEED, host=True)
    for w, g, what in zip(want, got, ("sim", "mask", "count", "status")):
        assert R.same_bits(g, w), (name, what)


def test_ransac_twin_leaves_other_pairs_alone():
    """offsets that start above 0 and stop short of the end: only their pairs are read or written"""
    a, b, off, c = R.batch_case([10, 70])
    pad = np.full((5, 3), np.nan)
    a2, b2 = np.concatenate([pad, a, pad]), np.concatenate([pad, b, pad])
    want = R.sim3_ransac(a, b, off, c, 32, R.TAU, R.SEED)
    got = LC.sim3_from_pairs(a2, b2, off + 5, c, 32, R.TAU, R.SEED, host=True)
    assert R.same_bits(got[0], want[0]) and R.same_bits(got[1][5:-5], want[1]) and not got[1][:5].any() and not got[1][-5:].any()
    assert R.same_bits(got[2], want[2]) and R.same_bits(got[3], want[3])


@pytest.mark.parametrize("n", R.APPLY_COUNTS)
def test_apply_points_twin_equals_reference(n):
    pts, anchor, nodes, new = R.apply_case(n)
    want = R.apply_points(pts, anchor, nodes, new)
    got = LC.apply_points(pts, anchor, nodes, new, host=True)
    assert R.same_bits(got, want)
    keep = (anchor == -1) | (anchor == 2)            # no anchor, or the unchanged node
    assert R.same_bits(got[keep], pts[keep])
    if n:
        assert not np.array_equal(got[~keep], pts[~keep]) or not (~keep).any()
    # unchanged nodes: every point comes back with its bits
    assert R.same_bits(LC.apply_points(pts, anchor, nodes, nodes, host=True), pts)


def test_apply_points_moves_with_the_node():
    """a point seen by a camera keeps its place relative to that camera: S'(X') = S(X)"""
    pts, anchor, nodes, new = R.apply_case(65)
    got = LC.apply_points(pts, anchor, nodes, new, host=True)
    for i in np.flatnonzero(anchor >= 0):
        assert np.allclose(R.apply(tuple(new[anchor[i]]), tuple(got[i])), R.apply(tuple(nodes[anchor[i]]), tuple(pts[i])),
                           rtol=0, atol=1e-12)


# ---- the pose graph -----------------------------------------------------------------------------------

def _one(S):
    return tuple(np.array([float(v)]) for v in S)


def test_jacobians_match_central_differences():
    """analytic Jacobians of the edge residual against central differences with h = 1e-6 on unit-scale
    cases: within 1e-6 absolute (the truncation h^2 / 6 times a third derivative of order one, plus the
    rounding eps / h ~ 1e-10 of that step)"""
    rng = np.random.default_rng(0)
    h, worst = 1e-6, 0.0
    for _ in range(25):
        Si, Sj = R.random_sim(rng), R.random_sim(rng)
        Z = R.compose(R.relative(Si, Sj), R.random_sim(rng, (0.9, 1.1)))
        w, ell = float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.5, 2.0))
        _, J = R.edge_terms(_one(Si), _one(Sj), _one(R.inverse(Z)), np.array([np.sqrt(w)]), ell, np.array([False]), np.array([False]))
        for side in range(2):
            for c in range(7):
                d = [0.0] * 7
                d[c] = h
                m = [-v for v in d]
                if side == 0:
                    rp, rm = R.residual(R.step(Si, d), Sj, Z, w, ell), R.residual(R.step(Si, m), Sj, Z, w, ell)
                else:
                    rp, rm = R.residual(Si, R.step(Sj, d), Z, w, ell), R.residual(Si, R.step(Sj, m), Z, w, ell)
                worst = max(worst, float(np.abs(J[0, side, :, c] - (rp - rm) / (2 * h)).max()))
    print("worst Jacobian difference", worst)
    assert worst <= 1e-6
    # a consistent edge has residual 0 (to rounding), and the fixed node's Jacobian is 0
    Si, Sj = R.random_sim(rng), R.random_sim(rng)
    assert np.abs(R.residual(Si, Sj, R.relative(Si, Sj), 1.0, 1.0)).max() < 1e-14
    _, J = R.edge_terms(_one(Si), _one(Sj), _one(R.inverse(R.relative(Si, Sj))), np.ones(1), 1.0, np.array([True]), np.array([False]))
    assert not J[0, 0].any() and J[0, 1].any()


def test_ring_of_40_is_corrected():
    """40 keyframes on a ring, 1 % scale drift per step, small rotation and translation noise, one
    loop edge: after optimisation the cost, the loop edge's residual and the RMS camera-centre error
    against ground truth are all lower"""
    est, e, m, w, ell, gt = R.ring_case(40)
    S, (c0, c1), (lm, acc, pcg) = R.pgo_sim3(est, e, m, w, ell, max_lm=10, max_pcg=300, pcg_tol=1e-12)
    r0 = float(np.linalg.norm(R.residual(est[39], est[0], m[-1], 1.0, ell)))
    r1 = float(np.linalg.norm(R.residual(S[39], S[0], m[-1], 1.0, ell)))
    e0 = float(np.sqrt(((R.centres_of(est) - R.centres_of(gt)) ** 2).sum(1).mean()))
    e1 = float(np.sqrt(((R.centres_of(S) - R.centres_of(gt)) ** 2).sum(1).mean()))
    print(f"cost {c0:.4f} -> {c1:.6f}, loop residual {r0:.4f} -> {r1:.6f}, rms centre {e0:.4f} -> {e1:.4f}, "
          f"last scale {est[39, 0]:.4f} -> {S[39, 0]:.4f}, lm {lm} ({acc} accepted), pcg {pcg}")
    assert c1 < c0 and r1 < r0 and e1 < e0
    assert R.same_bits(S[0], est[0])                       # node 0 is fixed
    got = LC.optimize_pose_graph(est, e, m, w, ell, max_lm=10, max_pcg=300, pcg_tol=1e-12, host=True)
    assert R.same_bits(got[0], S) and got[1] == (c0, c1) and got[2] == (lm, acc, pcg)


@pytest.mark.parametrize("name", R.PGO_NAMES)
def test_pgo_twin_equals_reference(name):
    S, e, m, w, ell, kw = R.pgo_cases()[name]
    want, cost, iters, trace = R.pgo_expected(name)
    got = LC.optimize_pose_graph(S, e, m, w, ell, host=True, **kw)
    assert R.same_bits(got[0], want) and got[1] == cost and got[2] == iters, (name, got[1:], cost, iters)
    assert R.same_bits(got[0][0], S[0])


def test_pgo_known_behaviour():
    want, cost, iters, trace = R.pgo_expected("two_consistent")
    assert cost == (0.0, 0.0) and iters == (0, 0, 0) and R.same_bits(want, R.pgo_cases()["two_consistent"][0])
    want, cost, iters, trace = R.pgo_expected("reject")
    # the first step is rejected: lambda rises tenfold and the next solve starts from the same nodes
    assert trace[0][2] is False and trace[1][0] == trace[0][0] * 10.0 and iters[1] < iters[0] and cost[1] < cost[0]
    for name in ("three", "ring65", "ring257", "star70", "double_loop"):
        _, cost, iters, _ = R.pgo_expected(name)
        assert cost[1] < cost[0] and iters[1] >= 1, name


def test_pgo_refusals_host():
    assert pgo_refusals(lambda *a, **k: LC.optimize_pose_graph(*a, host=True, **k)) == 21


# ---- end to end without images ------------------------------------------------------------------------

def _close_world(W, **kw):
    return LC.close_loops(W["rotations"], W["motions"], W["points"], W["colors"], W["obs"], W["loops"], tau=TAU,
                          min_pairs=MIN_PAIRS, **kw)


def test_close_loops_on_a_synthetic_world_host():
    check_world(lambda W: _close_world(W, host=True))
    check_wrong_world(lambda W: _close_world(W, host=True))


def test_close_loops_without_loops_returns_the_input():
    W = R.world_case()
    res = LC.close_loops(W["rotations"], W["motions"], W["points"], W["colors"], W["obs"], [], host=True)
    for k in ("rotations", "motions", "points", "colors"):
        assert R.same_bits(res[k], np.asarray(W[k], res[k].dtype)), k
    # min_pairs above every loop's pair count rejects them all
    res = LC.close_loops(W["rotations"], W["motions"], W["points"], W["colors"], W["obs"], W["loops"], tau=TAU, min_pairs=1000,
                         host=True)
    assert not any(c["accepted"] for c in res["constraints"]) and R.same_bits(res["points"], W["points"])


def test_anchors_and_lookup():
    obs = [(np.array([[1.5, 2.0], [3.0, 4.0]], np.float32), np.array([2, -1])),
           (np.array([[1.5, 2.0], [9.0, 9.0]], np.float32), np.array([0, 2]))]
    assert LC.anchors_of(obs, 4).tolist() == [1, -1, 0, -1]
    assert LC._lookup(obs[0], np.array([[3.0, 4.0], [1.5, 2.0], [7.0, 7.0]], np.float32)).tolist() == [-1, 2, -1]


# ---- the slam_main switch, as far as it goes without a device ---------------------------------------------

def test_close_parameters_and_unsupported_modes():
    import slamhip
    from slamhip import cycle
    p = slamhip.LoopParams()
    assert p.close is False and (p.tau, p.min_pairs) == (TAU, MIN_PAIRS)
    assert (p.hypotheses, p.max_lm, p.max_pcg, p.loop_weight) == (256, 10, 400, 1.0)
    on = slamhip.LoopParams(close=True)
    with pytest.raises(ValueError):
        cycle.slam_main(None, None, None, loops=on, tracker="klt")
    with pytest.raises(ValueError):
        cycle.slam_main(None, None, None, loops=on, dist=np.zeros(5), undistort="points")


def test_scene_reloads_the_closed_files(tmp_path):
    from slamhip import cycle, scene
    W = R.world_case()
    res = _close_world(W, host=True)
    sets = {"": (W["motions"], W["rotations"], W["points"], W["colors"]),
            "_closed": (res["motions"], res["rotations"], res["points"], res["colors"])}
    for suffix, (mot, rot, pts, col) in sets.items():
        for name, rows in (("poses", mot), ("rotations", rot), ("points", pts), ("colors", col)):
            with open(tmp_path / (name + suffix + ".txt"), "w") as f:
                for r in rows:
                    cycle.raw_output(r, f)
    gd = scene.load_global_data(str(tmp_path), cloud="closed")
    assert len(gd.spatialPoints) == len(res["points"]) < len(W["points"]) and len(gd.cameraRotations) == 40
    assert np.allclose(gd.spatialPoints, res["points"], rtol=0, atol=1e-11)          # twelve decimals in the files
    assert np.allclose(np.array(gd.cameraRotations), res["rotations"], rtol=0, atol=1e-11)
    assert np.array_equal(gd.spatialPointsColors, res["colors"])
    assert len(scene.load_global_data(str(tmp_path)).spatialPoints) == len(W["points"])
    with pytest.raises(ValueError):
        scene.load_global_data(str(tmp_path), cloud="other")

# ---- refusals ---------------------------------------------------------------------------------------

def test_refusals_host():
    n = refusals(lambda a, b, off, c, H, tau: LC.sim3_from_pairs(a, b, off, c, H, tau, R.SEED, host=True),
                 lambda p, an, nd, nn: LC.apply_points(p, an, nd, nn, host=True))
    assert n == 13
    pts, anchor, nodes, new = R.apply_case(8)
    for v in (5, -2):
        an = anchor.copy()
        an[3] = v
        with pytest.raises(L.SlamError) as e:
            LC.apply_points(pts, an, nodes, new, host=True)
        assert e.value.code == L.SLAM_E_INVALID_ARG
    # legal edge cases: no loop, no point
    sim, mask, count, status = LC.sim3_from_pairs(np.zeros((0, 3)), np.zeros((0, 3)), [0], np.zeros((0, 6)), 4, host=True)
    assert sim.shape == (0, 8) and len(mask) == 0


# ---- the host twins under ASan + UBSan, as a stand-alone program ------------------------------------

def test_host_twins_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "slam-indoor-code_amd", "csrc")
    exe = str(tmp_path / "loop_host_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", os.path.join(ROOT, "tests", "cpp", "loop_host_test.cpp"),
           os.path.join(csrc, "loop_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines()[-1].startswith("OK: ")

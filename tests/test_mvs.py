"""CPU tests of plane-sweep stereo: the contract (tests/mvs_ref.py) on scenes with
a known answer, the host twin slam_mvs_depth_host against it bit for bit, the
rule's edge cases, argument errors, the helpers of slamhip.dense, and the host
twin under AddressSanitizer + UBSan as a stand-alone program
(tests/cpp/mvs_host_test.cpp).  No GPU.
"""
import os
import subprocess

import numpy as np
import pytest

import mvs_ref as R
import slamhip
from slamhip import _lib as L
from slamhip import dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(sc, r, uq, mv):
    return slamhip.planeSweepDepth(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], r, uq, mv, host=True)


# ---- the contract on scenes with a known answer ----------------------------------------

@pytest.mark.parametrize("name", ["planted", "planted_bgr"])
def test_planted_plane(name):
    """noise texture 52 x 40, the source shifted by k = 5, M = I, v = (1, 0, 0), w[d] = d: every pixel
    whose window and census see only in-image pixels at plane k must win at k with cost 0, accepted"""
    sc, r, uq, mv, (plane, cost, inv) = R.case(name)
    H, W = plane.shape
    k = sc["k"]
    assert (H, W) == (40, 52) and k == 5 and uq == 80
    reg = (slice(5, H - 5), slice(6, W - 6 - k))
    assert (plane[reg] == k).all() and (cost[reg] == 0).all() and (inv[reg] > 0).all()
    # the sub-plane offset stays within half a plane
    assert (np.abs(inv[reg].astype(np.float64) - k) < 0.5).all()
    hp, hc, hi = host(sc, r, uq, mv)
    assert (hp[reg] == k).all() and (hc[reg] == 0).all() and (hi[reg] > 0).all()


def test_depth_step():
    sc, r, uq, mv, (plane, cost, inv) = R.case("step")
    H, W = plane.shape
    half, k0, k1 = sc["half"], sc["k0"], sc["k1"]
    left = (slice(5, H - 5), slice(6, half - 6))
    right = (slice(5, H - 5), slice(half + 6, W - 6 - k1))
    assert (plane[left] == k0).all() and (cost[left] == 0).all() and (inv[left] > 0).all()
    assert (plane[right] == k1).all() and (cost[right] == 0).all() and (inv[right] > 0).all()


# ---- the host twin equals the contract ------------------------------------------------

@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_host_twin_equals_reference(name):
    sc, r, uq, mv, want = R.case(name)
    got = host(sc, r, uq, mv)
    for g, w, what in zip(got, want, ("plane", "cost", "inv_depth")):
        assert R.same_bits(g, w), (name, what, int((g != w).sum()))


def test_cases_cover_the_issue():
    c = R.sweep_cases()
    shapes = {c[n][0]["ref"].shape[:2] for n in R.CASE_NAMES}
    assert {(40, 52), (33, 67), (8, 8), (20, 24)} <= shapes
    assert {len(c[n][0]["srcs"]) for n in R.CASE_NAMES} >= {1, 2, 4}
    assert {c[n][1] for n in R.CASE_NAMES} >= {0, 2, 3}
    assert {len(c[n][0]["planes"]) for n in R.CASE_NAMES} >= {4, 12, 256}
    assert len(c["pose_24x20_S2_r2_D256"][0]["planes"]) == 256
    # the general poses exercise the sub-plane refinement: accepted pixels off the plane values
    sc, _, _, _, (plane, _, inv) = R.case("pose_52x40_S1_r0_D12")
    acc = inv > 0
    assert acc.sum() > 100 and (inv[acc].astype(np.float64) != sc["planes"][plane[acc]].astype(np.float32)).sum() > 20


# ---- rule cases ----------------------------------------------------------------------------

def test_constant_image_is_plane_zero_and_rejected():
    _, _, _, _, (plane, cost, inv) = R.case("rule_constant")
    assert (plane == 0).all() and (cost == 0).all() and (inv == 0).all()


def test_equal_planes_give_the_lower_index():
    sc, _, _, _, (plane, cost, inv) = R.case("rule_equal_w")
    H, W = plane.shape
    reg = (slice(5, H - 5), slice(6, W - 6 - 2))
    assert sc["planes"][2] == sc["planes"][3]
    assert (plane[reg] == 2).all() and (cost[reg] == 0).all()
    assert not (plane == 3).any()


@pytest.mark.parametrize("name,S,r", [("rule_behind", 1, 2), ("rule_out_of_view", 1, 2), ("rule_out_of_view_S2", 2, 3)])
def test_invisible_sources_cost_the_maximum_and_are_rejected(name, S, r):
    _, rr, _, _, (plane, cost, inv) = R.case(name)
    assert rr == r
    assert (plane == 0).all() and (cost == 64 * (2 * r + 1) ** 2 * S).all() and (inv == 0).all()


def test_huge_entries_are_invalid_never_an_index():
    sc, r, uq, mv, (plane, cost, inv) = R.case("rule_huge")
    assert ((plane >= 0) & (plane < len(sc["planes"]))).all() and np.isfinite(cost).all()
    M = np.full((1, 9), 1e300)
    M[0, ::2] = -1e300
    got = slamhip.planeSweepDepth(sc["ref"], sc["srcs"], M, [[1e300, 1e300, -1e300]], [1e300, -1e300, 1e-300, 0.0], host=True)
    want = R.depth(sc["ref"], sc["srcs"], M, [[1e300, 1e300, -1e300]], [1e300, -1e300, 1e-300, 0.0])
    for g, w in zip(got, want):
        assert R.same_bits(g, w)


def test_streamed_winner_equals_the_volume_rule_on_adversarial_costs():
    """ties everywhere, the minimum at either end, neighbours of the winner holding the next
    smallest costs: exactly the cases where a top-4 stream could differ from the full rule"""
    tex = R.noise(9, 12, 3)
    flat = np.full((9, 12), 7, np.uint8)
    for ref, src in ((tex, tex), (flat, tex), (tex, flat)):
        for planes in (np.zeros(5), np.array([3.0, 0, 0, 0, 3, 3, 0]), np.arange(7.0)[::-1].copy(), np.array([0, 5.0, 0, 5, 0, 5])):
            for uq in (1, 100):
                got = slamhip.planeSweepDepth(ref, [src], np.eye(3).reshape(1, 9), [[1.0, 0, 0]], planes, 1, uq, 1, host=True)
                want = R.depth(ref, [src], np.eye(3).reshape(1, 9), [[1.0, 0, 0]], planes, 1, uq, 1)
                for g, w in zip(got, want):
                    assert R.same_bits(g, w)


# ---- argument errors --------------------------------------------------------------------

def test_argument_errors():
    sc, r, uq, mv, _ = R.case("planted")
    ok = dict(ref=sc["ref"], srcs=sc["srcs"], M=sc["M"], v=sc["v"], planes=sc["planes"], radius=2, uniq=80, min_views=1)

    def code(**kw):
        a = dict(ok)
        a.update(kw)
        try:
            slamhip.planeSweepDepth(host=True, **a)
        except L.SlamError as e:
            return e.code
        return L.SLAM_OK

    assert code() == L.SLAM_OK
    five = [sc["srcs"][0]] * 5
    assert code(srcs=[], M=np.zeros((0, 9)), v=np.zeros((0, 3))) == L.SLAM_E_INVALID_ARG
    assert code(srcs=five, M=np.tile(sc["M"], (5, 1)), v=np.tile(sc["v"], (5, 1))) == L.SLAM_E_INVALID_ARG
    assert code(planes=np.arange(3.0)) == L.SLAM_E_INVALID_ARG
    assert code(planes=np.arange(257.0)) == L.SLAM_E_INVALID_ARG
    assert code(planes=np.arange(256.0)) == L.SLAM_OK
    assert code(radius=4) == L.SLAM_E_INVALID_ARG
    assert code(radius=-1) == L.SLAM_E_INVALID_ARG
    assert code(uniq=0) == L.SLAM_E_INVALID_ARG and code(uniq=101) == L.SLAM_E_INVALID_ARG
    assert code(min_views=0) == L.SLAM_E_INVALID_ARG and code(min_views=2) == L.SLAM_E_INVALID_ARG
    for bad in (np.nan, np.inf, -np.inf):
        M = sc["M"].copy()
        M[0, 7] = bad
        assert code(M=M) == L.SLAM_E_INVALID_ARG
        v = sc["v"].copy()
        v[0, 1] = bad
        assert code(v=v) == L.SLAM_E_INVALID_ARG
        p = sc["planes"].copy()
        p[-1] = bad
        assert code(planes=p) == L.SLAM_E_INVALID_ARG
    wide = np.zeros((2, 4097), np.uint8)
    assert code(ref=wide, srcs=[wide]) == L.SLAM_E_UNSUPPORTED
    assert slamhip.lib().slam_abi_version() == 3


# ---- slamhip.dense helpers ----------------------------------------------------------------

def test_sweep_matrices_hand_cases():
    K = np.array([[64.0, 0, 26.0], [0, 64.0, 20.0], [0, 0, 1.0]])
    # pure baseline b along x: M = I, v = (f b, 0, 0)
    M, v = dense.sweep_matrices(K, np.eye(3), np.zeros(3), np.eye(3), [0.5, 0, 0])
    assert np.array_equal(M, np.eye(3)) and np.array_equal(v, [32.0, 0, 0])
    # the reference's own pose cancels: ref = src gives the identity and no parallax
    Rz = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    M, v = dense.sweep_matrices(K, Rz, [1.0, 2, 3], Rz, [1.0, 2, 3])
    assert np.array_equal(M, np.eye(3)) and np.array_equal(v, np.zeros(3))
    # a quarter turn about the optical axis between the views: pixel (x, y) - c -> (-(y - cy), x - cx)
    M, v = dense.sweep_matrices(K, np.eye(3), np.zeros(3), Rz, np.zeros(3))
    assert np.array_equal(M, [[0, -1, 26 + 20], [1, 0, 20 - 26], [0, 0, 1]]) and np.array_equal(v, np.zeros(3))
    # x_cam = R X + t: a point at depth z in the reference lands where the matrices say
    rng = np.random.RandomState(1)
    a = 0.1
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rr, tr, Rs, ts = Ry, rng.rand(3), Ry @ Ry, rng.rand(3)
    M, v = dense.sweep_matrices(K, Rr, tr, Rs, ts)
    X = np.array([0.3, -0.2, 4.0])
    pr, ps = K @ (Rr @ X + tr), K @ (Rs @ X + ts)
    z = pr[2]
    hh = M @ (pr / z) + v / z
    np.testing.assert_allclose(hh[:2] / hh[2], ps[:2] / ps[2], rtol=1e-12)
    np.testing.assert_allclose(hh[2], ps[2] / z, rtol=1e-12)
    B, c = dense.backproject_matrices(K, Rr, tr)
    np.testing.assert_allclose(c + B @ (pr / z) * z, X, rtol=1e-12)


def test_depth_planes_hand_cases():
    K = np.array([[64.0, 0, 26.0], [0, 64.0, 20.0], [0, 0, 1.0]])
    z = np.arange(1.0, 41.0)                               # 40 points on the axis: n // 20 = 2
    pts = np.stack([np.zeros(40), np.zeros(40), z], 1)
    w = dense.depth_planes(K, np.eye(3), np.zeros(3), pts, (40, 52), 5)
    lo, hi = 3.0, 38.0                                     # z[2], z[40 - 1 - 2]
    assert w.shape == (5,) and w[0] == 1 / (1.5 * hi) and w[-1] == 1.5 / lo
    np.testing.assert_allclose(np.diff(w), (w[-1] - w[0]) / 4, rtol=1e-12)
    # behind the camera and outside the image do not count: 7 good points are too few, 8 are enough
    good = np.stack([np.zeros(8), np.zeros(8), np.full(8, 2.0)], 1)
    junk = np.array([[0, 0, -1.0], [100.0, 0, 1.0], [0, -100.0, 1.0]])
    assert dense.depth_planes(K, np.eye(3), np.zeros(3), np.concatenate([good[:7], junk]), (40, 52), 8) is None
    w = dense.depth_planes(K, np.eye(3), np.zeros(3), np.concatenate([good, junk]), (40, 52), 8)
    assert w[0] == 1 / 3.0 and w[-1] == 0.75
    # the pose moves the points: t = (0, 0, 2) puts z = 2 at depth 4
    w = dense.depth_planes(K, np.eye(3), [0, 0, 2.0], good, (40, 52), 4)
    assert w[0] == 1 / 6.0 and w[-1] == 1.5 / 4


def test_source_order_and_params():
    assert dense.source_order(3, 8, 4) == [2, 4, 1, 5]
    assert dense.source_order(0, 8, 3) == [1, 2, 3]
    assert dense.source_order(7, 8, 2) == [6, 5]
    assert dense.source_order(0, 2, 4) == [1]
    p = dense.DenseParams()
    assert (p.D, p.sources, p.radius, p.uniq, p.min_views, p.eps, p.min_consistent, p.step) == (64, 2, 2, 80, 1, 0.01, 1, 4)
    for bad in (dict(D=3), dict(D=257), dict(sources=5), dict(radius=4), dict(uniq=0), dict(min_views=3), dict(step=0)):
        with pytest.raises(ValueError):
            dense.DenseParams(**bad)


def test_densify_host_path_on_planted_sequence():
    """two views of a wall at disparity 5 = plane 4 (planes at disparities 1 .. 12): the host path emits the
    contract's points; every guaranteed-interior grid pixel is among them at plane 4"""
    h, w, k = 40, 52, 5
    tex = R.noise(h, w, 7, 3)
    frames = [tex, R.shifted(tex, k)]
    K = np.array([[64.0, 0, 26.0], [0, 64.0, 20.0], [0, 0, 1.0]])
    rot, pos = [np.eye(3), np.eye(3)], [np.zeros((3, 1)), np.array([[1.0], [0.0], [0.0]])]
    sparse = np.stack([np.zeros(20), np.zeros(20), np.array([8.0] * 10 + [64.0 / 1.5] * 10)], 1)
    prm = dense.DenseParams(D=12, sources=1, eps=0.25, step=4)
    pts, cols = dense.densify(frames, K, rot, pos, sparse, prm, host=True)
    P = dense.plan(frames[0].shape, K, rot, pos, sparse, prm)
    np.testing.assert_allclose(P["planes"][0] * 64, np.arange(1.0, 13.0), rtol=1e-14)
    maps = [R.depth(frames[i], [frames[j] for j in P["src"][m]], P["M"][m, :1], P["v"][m, :1], P["planes"][m], 2, 80, 1)
            for m, i in enumerate(P["ref"])]
    want_p, want_c = R.fuse(frames, [m[2] for m in maps], P["nbr"], P["nbrM"], P["nbrv"], P["B"], P["c"], 0.25, 1, 4, 2)
    assert R.same_bits(pts, want_p) and R.same_bits(cols, want_c) and len(pts) >= 100
    masks = R.fuse_masks([m[2] for m in maps], P["nbr"], P["nbrM"], P["nbrv"], 0.25, 1, 4, 2)
    for m, (x0, x1) in enumerate(((6, w - 6 - k), (6 + k, w - 6))):
        for y in range(8, h - 6, 4):
            for x in range(-(-x0 // 4) * 4, x1, 4):
                assert masks[m][y, x] and maps[m][0][y, x] == 4
    # too few frames or sparse points: nothing, not an error
    assert len(dense.densify(frames[:1], K, rot[:1], pos[:1], sparse, prm, host=True)[0]) == 0
    assert len(dense.densify(frames, K, rot, pos, sparse[:7], prm, host=True)[0]) == 0


def test_slam_main_refuses_a_frame_count_that_differs(monkeypatch):
    from slamhip import cycle

    def fake_cycle(media, K, cond, deque, gd, logs, ops, stats=None):
        logs.pose(np.eye(3), np.zeros(3), np.zeros((4, 4, 3), np.uint8))     # a pose logged, none moved to gd
        return cycle.EMPTY_BATCH
    monkeypatch.setattr(cycle, "main_cycle", fake_cycle)
    cfg = slamhip.ConfigService(slamhip.reference_example())
    with pytest.raises(RuntimeError):
        cycle.slam_main(None, np.eye(3), cfg, ops=object(), dense=dense.DenseParams())
    gd, logs = cycle.slam_main(None, np.eye(3), cfg, ops=object())
    assert logs.frames is None and not hasattr(gd, "densePoints")


# ---- the host twin under ASan + UBSan, as a stand-alone program ---------------------------

def test_host_twin_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "slam-indoor-code_amd", "csrc")
    exe = str(tmp_path / "mvs_host_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread",
           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-static-libasan",
           os.path.join(ROOT, "tests", "cpp", "mvs_host_test.cpp"), os.path.join(csrc, "mvs_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines()[-1].startswith("OK: ")

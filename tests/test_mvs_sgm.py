"""CPU tests of the semi-global aggregation of the plane-sweep cost volume: the
contract (tests/mvs_sgm_ref.py) on scenes with a known answer, the host twins
(slam_mvs_cost_volume_host, slam_mvs_sgm_aggregate_host, slam_mvs_depth_sgm_host)
against it bit for bit, argument errors, DenseParams(sgm=...), the densify host
path, and the twins under AddressSanitizer + UBSan as a stand-alone program
(tests/cpp/mvs_sgm_host_test.cpp).  No GPU.
"""
import os
import subprocess

import numpy as np
import pytest

import mvs_ref as R
import mvs_sgm_ref as G
import slamhip
from slamhip import _lib as L
from slamhip import dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(sc, r, uq, mv, p1, p2, paths):
    return slamhip.planeSweepDepthSgm(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], r, uq, mv, p1, p2, paths, host=True)


def assert_same(got, want, tag):
    for g, w, what in zip(got, want, ("plane", "cost", "inv_depth")):
        assert R.same_bits(g, w), (tag, what, int((np.asarray(g) != np.asarray(w)).sum()))


# ---- the contract on scenes with a known answer ----------------------------------------

@pytest.fixture(scope="module")
def wall():
    sc = G.wall_scene()
    C, nv = R.cost_volume(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], 2)
    C.setflags(write=False)
    nv.setflags(write=False)
    return sc, C, nv


def test_wall_winner_take_all_rejects_the_box(wall):
    sc, C, nv = wall
    _, _, inv = R.winner(C, nv, sc["planes"], 80, 1)
    assert inv[sc["interior"]].shape == (8, 7) and (inv[sc["interior"]] == 0).all()


@pytest.mark.parametrize("p1,p2", [(10, 120), (2, 12)])
@pytest.mark.parametrize("paths", [4, 8])
def test_wall_sgm_fills_the_box(wall, paths, p1, p2):
    sc, C, nv = wall
    plane, cost, inv = G.depth_from_volume(C, nv, sc["planes"], 1, 2, 80, 1, p1, p2, paths)
    box = sc["interior"]
    assert (plane[box] == 5).all() and (inv[box] > 0).all()
    assert (np.abs(inv[box].astype(np.float64) - 5.0) < 0.5).all()
    assert (plane[sc["region"]] == 5).all()
    assert_same(host(sc, 2, 80, 1, p1, p2, paths), (plane, cost, inv), "wall")


@pytest.mark.parametrize("paths", [4, 8])
def test_depth_step_keeps_both_planes(paths):
    """plane 3 left of column half - 8, plane 7 right of half + 8; as in tests/test_mvs.py the 5 rows and 6 columns
    next to the image border, where census and window clamp, and the k1 columns that left the source are left out"""
    sc = R.sweep_cases()["step"][0]
    plane, _, inv = G.case("step", 10, 120, paths)
    H, W = plane.shape
    half = sc["half"]
    left, right = (slice(5, H - 5), slice(6, half - 8)), (slice(5, H - 5), slice(half + 8, W - 6 - sc["k1"]))
    assert (plane[left] == 3).all() and (inv[left] > 0).all()
    assert (plane[right] == 7).all() and (inv[right] > 0).all()


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_zero_penalties_are_winner_take_all(name):
    sc, r, uq, mv, (plane, cost, inv) = R.case(name)
    for paths in (4, 8):
        gp, gc, gi = G.case(name, 0, 0, paths)
        assert R.same_bits(gp, plane) and R.same_bits(gi, inv) and np.array_equal(gc, paths * cost)
    assert_same(host(sc, r, uq, mv, 0, 0, 8), G.case(name, 0, 0, 8), name)


def test_bounds_of_the_reference():
    """C <= L_r <= C + P2 is asserted inside path(); the largest penalties on the largest costs stay in uint16"""
    rng = np.random.RandomState(3)
    C = G.random_volume(rng, 1, 5, 6, 9, maxima=True)[0].transpose(2, 0, 1)
    S = G.aggregate(C, G.MAX_P2, G.MAX_P2, 8)
    assert S.dtype == np.int32 and int(S.max()) <= 8 * 65535 and (S >= 8 * C.astype(np.int64)).all()
    assert G.effective(255, 3, 4) == 49980 == G.MAX_P2 - 3011 and 8 * (G.MAX_COST + 49980) == 500192
    with pytest.raises(ValueError):
        G.aggregate(C, 5, 4, 8)
    with pytest.raises(ValueError):
        G.aggregate(C, 1, G.MAX_P2 + 1, 8)
    with pytest.raises(ValueError):
        G.aggregate(C, 1, 2, 6)


# ---- the host twins equal the contract ------------------------------------------------

@pytest.mark.parametrize("setting", G.SETTINGS, ids=lambda s: "p%d_%d_%d" % s)
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_host_twin_equals_reference(name, setting):
    sc, r, uq, mv = R.sweep_cases()[name]
    assert_same(host(sc, r, uq, mv, *setting), G.case(name, *setting), name)


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_host_volume_equals_reference(name):
    sc, r, _, _ = R.sweep_cases()[name]
    C, nv = G.volume(name)
    S = len(sc["srcs"])
    gC, gnv = slamhip.planeSweepCostVolume([sc["ref"]] + list(sc["srcs"]), [0], [list(range(1, S + 1))],
                                           np.pad(sc["M"].reshape(S, 9), ((0, 4 - S), (0, 0)))[None],
                                           np.pad(sc["v"].reshape(S, 3), ((0, 4 - S), (0, 0)))[None], sc["planes"][None], r,
                                           host=True)
    assert gC.dtype == np.uint16 and gnv.dtype == np.uint8
    assert np.array_equal(gC[0].transpose(2, 0, 1), C) and np.array_equal(gnv[0].transpose(2, 0, 1), nv)


@pytest.mark.parametrize("shape", G.EDGE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_twin_on_edge_shapes(shape):
    h, w = shape
    sc = G.pose_scene(h, w, 12, 31)
    for setting in G.SETTINGS:
        want = G.depth(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], 1, 80, 1, *setting)
        assert_same(host(sc, 1, 80, 1, *setting), want, (shape, setting))


@pytest.mark.parametrize("D", G.EDGE_PLANES)
def test_host_twin_on_plane_counts(D):
    sc = G.pose_scene(20, 24, D, 32, S=2)
    for setting in ((10, 120, 8), (255, 255, 4)):
        want = G.depth(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], 2, 80, 1, *setting)
        assert_same(host(sc, 2, 80, 1, *setting), want, (D, setting))


@pytest.mark.parametrize("paths", [4, 8])
def test_host_aggregate_on_random_maximal_volumes(paths):
    rng = np.random.RandomState(17 + paths)
    for (n, h, w, D), (P1, P2) in (((2, 7, 9, 256), (G.MAX_P2, G.MAX_P2)), ((1, 9, 7, 65), (0, G.MAX_P2)),
                                   ((3, 5, 4, 4), (1, 2)), ((1, 1, 1, 64), (7, 9)), ((1, 33, 67, 12), (250, 3000))):
        C = G.random_volume(rng, n, h, w, D, maxima=True)
        got = slamhip.sgmAggregate(C, P1, P2, paths, host=True)
        assert R.same_bits(got, G.aggregate_public(C, P1, P2, paths)), (n, h, w, D)


# ---- argument errors --------------------------------------------------------------------

def test_argument_errors():
    sc, r, uq, mv, _ = R.case("planted")
    ok = dict(ref=sc["ref"], srcs=sc["srcs"], M=sc["M"], v=sc["v"], planes=sc["planes"], radius=2, uniq=80, min_views=1,
              p1=10, p2=120, paths=8)

    def code(**kw):
        a = dict(ok)
        a.update(kw)
        try:
            slamhip.planeSweepDepthSgm(host=True, **a)
        except L.SlamError as e:
            return e.code
        return L.SLAM_OK

    assert code() == L.SLAM_OK
    assert code(p1=121) == L.SLAM_E_INVALID_ARG
    assert code(p1=-1) == L.SLAM_E_INVALID_ARG and code(p2=256) == L.SLAM_E_INVALID_ARG
    assert code(p1=255, p2=255) == L.SLAM_OK and code(p1=0, p2=0) == L.SLAM_OK
    for paths in (0, 1, 5, 6, 16):
        assert code(paths=paths) == L.SLAM_E_INVALID_ARG
    assert code(paths=4) == L.SLAM_OK
    # everything slam_mvs_depth_host refuses
    assert code(srcs=[], M=np.zeros((0, 9)), v=np.zeros((0, 3))) == L.SLAM_E_INVALID_ARG
    assert code(planes=np.arange(3.0)) == L.SLAM_E_INVALID_ARG and code(planes=np.arange(257.0)) == L.SLAM_E_INVALID_ARG
    assert code(radius=4) == L.SLAM_E_INVALID_ARG and code(uniq=0) == L.SLAM_E_INVALID_ARG
    assert code(min_views=2) == L.SLAM_E_INVALID_ARG
    M = sc["M"].copy()
    M[0, 7] = np.nan
    assert code(M=M) == L.SLAM_E_INVALID_ARG
    wide = np.zeros((2, 4097), np.uint8)
    assert code(ref=wide, srcs=[wide]) == L.SLAM_E_UNSUPPORTED

    def agg(shape=(1, 2, 3, 4), P1=1, P2=2, paths=8):
        try:
            slamhip.sgmAggregate(np.zeros(shape, np.uint16), P1, P2, paths, host=True)
        except L.SlamError as e:
            return e.code
        return L.SLAM_OK

    assert agg() == L.SLAM_OK and agg(P2=G.MAX_P2, P1=G.MAX_P2) == L.SLAM_OK
    assert agg(P2=G.MAX_P2 + 1) == L.SLAM_E_INVALID_ARG and agg(P1=3) == L.SLAM_E_INVALID_ARG
    assert agg(P1=-1) == L.SLAM_E_INVALID_ARG and agg(paths=2) == L.SLAM_E_INVALID_ARG
    assert agg(shape=(1, 2, 3, 3)) == L.SLAM_E_INVALID_ARG and agg(shape=(1, 2, 3, 257)) == L.SLAM_E_INVALID_ARG
    assert agg(shape=(1, 1, 4097, 4)) == L.SLAM_E_UNSUPPORTED
    assert slamhip.lib().slam_abi_version() == 3


def test_sgm_and_dense_params():
    s = dense.SgmParams()
    assert (s.p1, s.p2, s.paths) == (10, 120, 8)
    for bad in (dict(p1=-1), dict(p1=121), dict(p2=256), dict(paths=6), dict(p1=3, p2=2)):
        with pytest.raises(ValueError):
            dense.SgmParams(**bad)
    assert dense.DenseParams().sgm is None
    assert dense.DenseParams(sgm=s).sgm is s and slamhip.SgmParams is dense.SgmParams
    with pytest.raises(ValueError):
        dense.DenseParams(sgm=(10, 120, 8))
    assert "not tuned" in " ".join(dense.SgmParams.__doc__.split())


# ---- densify ------------------------------------------------------------------------------

def test_densify_host_path_on_planted_sequence():
    """the sequence of tests/test_mvs.py: with sgm set the host path emits the contract's points (aggregated maps
    through mvs_ref.fuse), and without it exactly what it emitted before"""
    h, w, k = 40, 52, 5
    tex = R.noise(h, w, 7, 3)
    frames = [tex, R.shifted(tex, k)]
    K = np.array([[64.0, 0, 26.0], [0, 64.0, 20.0], [0, 0, 1.0]])
    rot, pos = [np.eye(3), np.eye(3)], [np.zeros((3, 1)), np.array([[1.0], [0.0], [0.0]])]
    sparse = np.stack([np.zeros(20), np.zeros(20), np.array([8.0] * 10 + [64.0 / 1.5] * 10)], 1)
    sg = dense.SgmParams(2, 12, 4)
    prm = dense.DenseParams(D=12, sources=1, eps=0.25, step=4, sgm=sg)
    pts, cols = dense.densify(frames, K, rot, pos, sparse, prm, host=True)
    P = dense.plan(frames[0].shape, K, rot, pos, sparse, prm)
    maps = [G.depth(frames[i], [frames[j] for j in P["src"][m]], P["M"][m, :1], P["v"][m, :1], P["planes"][m], 2, 80, 1,
                    sg.p1, sg.p2, sg.paths) for m, i in enumerate(P["ref"])]
    want_p, want_c = R.fuse(frames, [m[2] for m in maps], P["nbr"], P["nbrM"], P["nbrv"], P["B"], P["c"], 0.25, 1, 4, 2)
    assert R.same_bits(pts, want_p) and R.same_bits(cols, want_c) and len(pts) > 0
    plain = dense.DenseParams(D=12, sources=1, eps=0.25, step=4)
    wta = [R.depth(frames[i], [frames[j] for j in P["src"][m]], P["M"][m, :1], P["v"][m, :1], P["planes"][m], 2, 80, 1)
           for m, i in enumerate(P["ref"])]
    wp, wc = R.fuse(frames, [m[2] for m in wta], P["nbr"], P["nbrM"], P["nbrv"], P["B"], P["c"], 0.25, 1, 4, 2)
    pp, pc = dense.densify(frames, K, rot, pos, sparse, plain, host=True)
    assert R.same_bits(pp, wp) and R.same_bits(pc, wc)


# ---- the host twins under ASan + UBSan, as a stand-alone program ---------------------------

def test_host_twin_under_sanitizers(tmp_path):
    csrc = os.path.join(ROOT, "slam-indoor-code_amd", "csrc")
    exe = str(tmp_path / "mvs_sgm_host_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           os.path.join(ROOT, "tests", "cpp", "mvs_sgm_host_test.cpp"), os.path.join(csrc, "mvs_host.cpp"),
           os.path.join(csrc, "mvs_sgm_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines()[-1].startswith("OK: ")

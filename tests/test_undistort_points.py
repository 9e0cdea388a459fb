"""CPU tests of the numpy restatement of cv::undistortPoints
(tests/undistort_points_ref.py), the checker of tests/test_undistort_points_gpu.py:
its forward model against the map restatement of tests/undistort_ref.py, the
round trip inside the fold of the samsung-hv lens, the shares of pixels it can
and cannot undistort, every exit of its loop, and what undistorted keypoints
buy the essential-matrix step.

Fixture: tests/golden/calib_samsung_hv.xml (see tests/test_undistort.py).
"""
import functools
import os

import numpy as np
import pytest

import slamhip
import undistort_points_ref as R
import undistort_ref as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CALIB = os.path.join(GOLDEN, "calib_samsung_hv.xml")

D8 = np.array([-0.21, 0.07, 0.0013, -0.0021, 0.011, 0.05, -0.02, 0.004])
D12 = np.concatenate([D8, [0.002, -0.001, 0.0015, 0.0007]])


@functools.lru_cache(maxsize=None)
def calib():
    K = slamhip.load_calibration(CALIB)
    D = slamhip.load_calibration(CALIB, "DC").ravel()
    K.setflags(write=False)
    D.setflags(write=False)
    return K, D


def scaled(K, s):
    K = np.array(K)
    K[:2] *= s
    return K


def camera(w, h):
    f = 0.9 * max(w, h, 4)
    return np.array([[f, 0, w / 2 + 0.31], [0, 1.01 * f, h / 2 - 0.17], [0, 0, 1.0]])


def pixels(w, h):
    gx, gy = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return np.stack([gx.ravel(), gy.ravel()], 1)


# ---------------- 1. the forward model is section 12's ----------------

@pytest.mark.parametrize("w,h", [(200, 37), (333, 70)])
@pytest.mark.parametrize("model", ["samsung", "d8", "d12"])
def test_forward_model_is_the_map_polynomial(w, h, model):
    """distort_points at the integer pixels is initUndistortRectifyMap's u, v up
    to the last bits of the serial row walk: cvRound(32 u) within 1 of the map's"""
    D = {"samsung": calib()[1], "d8": D8, "d12": D12}[model]
    K = camera(w, h)
    iu, iv = U.fixed_point(w, h, K, D, K)
    uv = R.distort_points(pixels(w, h), K, D, K)
    du = np.abs(U.cv_round(uv[:, 0] * 32.0).reshape(h, w) - iu)
    dv = np.abs(U.cv_round(uv[:, 1] * 32.0).reshape(h, w) - iv)
    print(model, w, h, "differing:", int((du > 0).sum()), int((dv > 0).sum()), "of", iu.size)
    assert du.max() <= 1 and dv.max() <= 1
    assert (du == 0).mean() > 0.9 and (dv == 0).mean() > 0.9      # and not off by one throughout


# ---------------- 2. round trip inside the fold ----------------

def test_round_trip_inside_the_fold():
    """Ideal points with r <= 0.5, distorted, then undistorted at (50, 0.01): every
    residual is <= 0.01 px and the result within 0.02 px of the ideal.

    The bound: a residual e in distorted pixels is an error of at most
    e * (f_max / f_min) / s in ideal pixels, s the smallest stretch of the
    forward model between the two points.  For samsung-hv on r <= 0.52 (the
    margin covers the estimate's own offset) the radial stretch d(r cdist)/dr
    is >= 0.5917, the tangential stretch cdist >= 0.9374, and the decentring
    terms change the Jacobian by at most 6 max(|p1|, |p2|) r <= 0.017: s >=
    0.574, f_max / f_min = 1.0034, so 0.01 px of residual is <= 0.0175 px of
    error, plus float32 rounding of the input and the output (2 * 2^-14 px at
    coordinates below 2048)."""
    K, D = calib()
    k1, k2, p1, p2, k3 = D
    r = np.linspace(0, 0.52, 4001)
    radial = (1 + 3 * k1 * r ** 2 + 5 * k2 * r ** 4 + 7 * k3 * r ** 6).min()
    tangential = (1 + k1 * r ** 2 + k2 * r ** 4 + k3 * r ** 6).min()
    s = min(radial, tangential) - 6 * max(abs(p1), abs(p2)) * 0.52
    print("stretch: radial %.4f tangential %.4f, with decentring >= %.4f" % (radial, tangential, s))
    assert s >= 0.574
    assert 0.01 * (K[1, 1] / K[0, 0]) / s + 4 * 2.0 ** -14 < 0.02
    rng = np.random.default_rng(5)
    rad = 0.5 * np.sqrt(rng.random(20000))
    ang = rng.random(20000) * 2 * np.pi
    ideal = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    ideal[:64] *= (0.5 / rad[:64])[:, None]                     # some exactly on r = 0.5
    raw = R.distort_points(ideal, K, D, normalized=True).astype(np.float32)
    xy, err, ex, it = R.undistort_points(raw, K, D, K, (50, 0.01), details=True)
    want = np.stack([ideal[:, 0] * K[0, 0] + K[0, 2], ideal[:, 1] * K[1, 1] + K[1, 2]], 1)
    off = np.hypot(*(xy.astype(np.float64) - want).T)
    print("max residual %.5f px, max offset %.5f px, iterations up to %d" % (err.max(), off.max(), it.max()))
    assert (err <= 0.01).all()
    assert off.max() <= 0.02
    assert (ex == R.EXIT_EPS).all()


# ---------------- 3. the measured shares ----------------

CRITERIA = ((5, 0.0), (50, 0.01), (500, 0.01))
# share with err <= 0.01 px per criterion, share leaving through icdist < 0 per criterion
SHARES = {(1920, 1080): ((0.7504, 0.8697, 0.8706), (0.066, 0.1283, 0.1294)),
          (640, 480): ((0.6711, 0.7888, 0.7893), None)}


@functools.lru_cache(maxsize=None)
def run(w, h, criteria):
    K, D = calib()
    Ks = scaled(K, w / 1920)
    out = R.undistort_points(pixels(w, h), Ks, D, Ks, criteria, details=True)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("w,h", list(SHARES))
def test_measured_shares(w, h):
    """over every integer pixel of the samsung-hv camera: the radial polynomial
    folds over at r = 0.61, pixels beyond its image have no preimage, and
    OpenCV's default 5 iterations leave 12 % of the reachable ones > 0.01 px off"""
    ok_want, ic_want = SHARES[(w, h)]
    ok, ic = [], []
    for c in CRITERIA:
        xy, err, ex, it = run(w, h, c)
        ok.append(float((err <= 0.01).mean()))
        ic.append(float((ex == R.EXIT_ICDIST).mean()))
    print(w, h, "err <= 0.01:", ok, "icdist < 0:", ic)
    for got, want in zip(ok, ok_want):
        assert abs(got - want) <= 0.005
    if ic_want is not None:
        for got, want in zip(ic, ic_want):
            assert abs(got - want) <= 0.005
    assert ok[0] < ok[1] <= ok[2]


# ---------------- 4. every exit, and lanes that leave at different j ----------------

def test_every_exit_is_exercised():
    xy, err, ex, it = run(640, 480, (50, 0.01))
    for e in (R.EXIT_COUNT, R.EXIT_EPS, R.EXIT_ICDIST):
        assert (ex == e).sum() >= 100, e
    assert (it[ex == R.EXIT_COUNT] == 50).all()
    assert it[ex == R.EXIT_EPS].min() >= 1
    # COUNT only: nothing leaves through eps, the rest through icdist or the count
    _, _, ex5, it5 = run(640, 480, (5, 0.0))
    assert not (ex5 == R.EXIT_EPS).any() and (ex5 == R.EXIT_ICDIST).any()
    assert (it5[ex5 == R.EXIT_COUNT] == 5).all()
    # one wave of 64 consecutive points whose lanes leave all over 1..50
    chunks = it[:len(it) // 64 * 64].reshape(-1, 64)
    spread = np.array([len(np.unique(c)) for c in chunks[::7]])
    best = chunks[::7][spread.argmax()]
    print("most divergent wave:", sorted(set(best.tolist())))
    assert best.min() <= 5 and best.max() == 50 and len(np.unique(best)) >= 16


def test_eps_mode_residual_is_the_loops_last_error():
    """COUNT|EPS without the icdist exit: err is the error the loop last computed,
    so a point that left through eps has err < eps and one that ran out of
    iterations has err >= eps or converged on the last one"""
    xy, err, ex, it = run(640, 480, (50, 0.01))
    assert (err[ex == R.EXIT_EPS] < 0.01).all()
    assert (err[ex == R.EXIT_ICDIST] > 0.01).all()              # back at the start value: far off


def test_criteria_are_checked():
    K, D = calib()
    p = np.zeros((1, 2), np.float32)
    for bad in ((0, 0.0), (1001, 0.0), (None, 0.01), (5, -1.0), (5, np.nan), (5, np.inf)):
        with pytest.raises(ValueError):
            R.undistort_points(p, K, D, None, bad)
    with pytest.raises(ValueError):
        R.undistort_points(p, K, np.zeros(14))
    xy, err = R.undistort_points(np.zeros((0, 2), np.float32), K, D)
    assert xy.shape == (0, 2) and err.shape == (0,)


def test_no_distortion_is_the_pinhole_inverse():
    K, _ = calib()
    p = np.array([[K[0, 2], K[1, 2]], [100.25, 900.5], [1919, 0]], np.float32)
    xy, err = R.undistort_points(p, K, np.zeros(5), K)
    np.testing.assert_allclose(xy, p, atol=2e-4)
    assert (err < 1e-9).all()
    n, _ = R.undistort_points(p, K, np.zeros(4))                # P absent: normalised coordinates
    np.testing.assert_allclose(n[:, 0], (p[:, 0].astype(np.float64) - K[0, 2]) / K[0, 0], rtol=1e-6, atol=1e-9)


# ---------------- 5. why it matters ----------------

def test_undistorted_points_give_a_better_relative_pose():
    """two views of a synthetic scene through the distorted samsung-hv camera:
    the essential-matrix step on the undistorted points is closer to the true
    motion, in rotation and in translation direction, than on the raw points"""
    from oracle_ops import OracleOps
    K, D = calib()
    rng = np.random.default_rng(11)
    X = np.stack([rng.uniform(-2.2, 2.2, 1500), rng.uniform(-1.6, 1.6, 1500), rng.uniform(4.5, 9.0, 1500)], 1)
    rv = np.array([0.02, -0.06, 0.03])
    th = np.linalg.norm(rv)
    kx = np.array([[0, -rv[2], rv[1]], [rv[2], 0, -rv[0]], [-rv[1], rv[0], 0]]) / th
    Rt = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
    tt = np.array([0.5, 0.05, 0.1])
    X2 = X @ Rt.T + tt
    n1, n2 = X[:, :2] / X[:, 2:], X2[:, :2] / X2[:, 2:]
    keep = (np.hypot(*n1.T) <= 0.5) & (np.hypot(*n2.T) <= 0.5)
    n1, n2 = n1[keep], n2[keep]
    assert len(n1) >= 500
    raw = [R.distort_points(n, K, D, normalized=True).astype(np.float32) for n in (n1, n2)]
    und = []
    for p in raw:
        xy, err = R.undistort_points(p, K, D, K, (50, 0.01))
        assert (err <= 0.01).all()
        und.append(xy)

    def errors(p1, p2):
        ok, Re, te, _ = OracleOps().estimate_transformation(p1, p2, np.array(K), True, 0.999, 1.0, 50.0)
        Re, te = np.asarray(Re, np.float64).reshape(3, 3), np.asarray(te, np.float64).reshape(3)
        rot = np.degrees(np.arccos(np.clip((np.trace(Re @ Rt.T) - 1) / 2, -1, 1)))
        tr = np.degrees(np.arccos(np.clip(te @ tt / np.linalg.norm(te) / np.linalg.norm(tt), -1, 1)))
        return rot, tr

    r_raw, t_raw = errors(*raw)
    r_und, t_und = errors(*und)
    print("rotation error (deg): raw %.4f undistorted %.4f; translation direction: raw %.4f undistorted %.4f"
          % (r_raw, r_und, t_raw, t_und))
    assert r_und < r_raw
    assert t_und < t_raw

"""GPU tests of cv::undistortPoints on the device (undist_points in
csrc/undistort.hip behind slam_undistort_points and slam_undistort_points_dev):
the undistorted points and the residuals equal the numpy restatement
(tests/undistort_points_ref.py) bit for bit, and slam_main(undistort="points")
writes the files of the same run over the CPU oracle with that restatement.

Fixture: tests/golden/calib_samsung_hv.xml (see tests/test_undistort_gpu.py).
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import slamhip
import undistort_points_ref as R
import undistort_ref as U
from slamhip import _lib as L
from slamhip import cycle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CALIB = os.path.join(GOLDEN, "calib_samsung_hv.xml")

D12 = np.array([-0.21, 0.07, 0.0013, -0.0021, 0.011, 0.05, -0.02, 0.004, 0.002, -0.001, 0.0015, 0.0007])
CRITERIA = [(5, 0.0), (1, 0.0), (50, 0.01), (1000, 1e-9)]
SIZES = [0, 1, 63, 64, 65, 257, 10007]


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


def general_p():
    """a P whose third row is at work: the division by ww matters"""
    return np.array([[1650.0, 3.5, 970.25], [-2.25, 1655.5, 541.0], [1e-2, -2e-2, 1.05]])


def fold_radius(D):
    """the distorted radius at which the radial polynomial of a 5-coefficient model folds over"""
    k1, k2, _, _, k3 = D
    r = np.linspace(0, 2, 200001)
    rd = r * (1 + k1 * r ** 2 + k2 * r ** 4 + k3 * r ** 6)
    return rd[np.argmax(np.diff(rd) < 0)]


def points(n, K, D, seed):
    """n points over and around a 1920 x 1080 image of camera K, the special ones first"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-200, 2120, n), rng.uniform(-200, 1280, n)], 1).astype(np.float32)
    whole = rng.random(n) < 0.3
    p[whole] = np.round(p[whole])                                          # FAST's integer pixels among them
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    rf = fold_radius(calib()[1])
    a = np.linspace(0, 2 * np.pi, 12, endpoint=False)
    special = [[cx, cy], [np.float32(cx), np.float32(cy)]]
    for scale in (1 - 1e-6, 1.0, 1 + 1e-6, 1.2, 2.0):                      # on the fold, and past it (icdist < 0 there)
        special += [[cx + scale * rf * fx * np.cos(t), cy + scale * rf * fy * np.sin(t)] for t in a]
    special += [[np.inf, 3], [3, -np.inf], [np.nan, 5], [7, np.nan], [np.inf, np.nan], [1e6, 1e6], [-1e6, 1e6],
                [1e6, -1e6], [-1e6, -1e6], [0, 0], [1919, 1079]]
    special = np.array(special, np.float32)
    m = min(n, len(special))
    # spread over the array when there is room, so they fall into several blocks
    idx = (np.arange(m) * max(1, n // max(m, 1))) % max(n, 1) if n >= len(special) else np.arange(m)
    p[idx] = special[:m]
    return p


def keypoints(p, seed):
    """a slam_keypoint array around the points: the other fields hold values a wrong stride would read"""
    rng = np.random.default_rng(seed)
    k = np.zeros(len(p), L.KEYPOINT_DTYPE)
    k["x"], k["y"] = p[:, 0], p[:, 1]
    k["size"], k["angle"], k["response"] = 7.0, rng.uniform(0, 360, len(p)), rng.uniform(10, 250, len(p))
    k["octave"], k["class_id"] = rng.integers(0, 1 << 30, len(p)), -1
    return k


def same(got, want):
    np.testing.assert_array_equal(got[0], want[0], err_msg="points")
    np.testing.assert_array_equal(got[1], want[1], err_msg="residuals")        # NaN where the reference has NaN


# ---------------- 6. bit-exact against the reference ----------------

@pytest.mark.parametrize("criteria", CRITERIA, ids=lambda c: "%dx%g" % c)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_criteria(gpu_ctx, n, criteria):
    K, D = calib()
    p = points(n, K, D, 100 + n)
    want = R.undistort_points(p, K, D, K, criteria)
    same(slamhip.undistortPoints(p, K, D, K, criteria, ctx=gpu_ctx), want)
    # stride 28, over a real keypoint array
    k = keypoints(p, n)
    before = k.copy()
    same(slamhip.undistortPoints(k, K, D, K, criteria, ctx=gpu_ctx), want)
    assert k.tobytes() == before.tobytes()                                     # read in place, nothing written


def test_special_points_take_the_exits_they_should(gpu_ctx):
    K, D = calib()
    p = points(10007, K, D, 7)
    xy, err, ex, it = R.undistort_points(p, K, D, K, (50, 0.01), details=True)
    assert (ex == R.EXIT_ICDIST).sum() >= 24 and (ex == R.EXIT_EPS).any() and (ex == R.EXIT_COUNT).any()
    assert np.isnan(err).sum() >= 5 and np.isnan(xy).any()
    far = np.abs(p).max(1) == 1e6
    assert far.sum() == 4 and (ex[far] == R.EXIT_ICDIST).all()          # +-1e6: far past the fold
    centre = (p == np.array([K[0, 2], K[1, 2]], np.float32)).all(1)
    assert centre.any() and (err[centre] < 1e-3).all()
    got = slamhip.undistortPoints(p, K, D, K, (50, 0.01), ctx=gpu_ctx)
    same(got, (xy, err))
    # consumers test err <= tol: a NaN residual counts as invalid
    assert not (got[1][np.isnan(err)] <= 0.01).any()


@pytest.mark.parametrize("nd", [4, 5, 8, 12])
@pytest.mark.parametrize("with_p", ["P", "noP"])
def test_models_skew_and_projection(gpu_ctx, nd, with_p):
    """rational and prism terms, a skew entry in K (ignored), a general P or none"""
    K = np.array(calib()[0])
    K[0, 1] = 0.8
    D = D12[:nd]
    P = general_p() if with_p == "P" else None
    p = points(257, K, D, 50 + nd)
    for criteria in ((5, 0.0), (50, 0.01)):
        want = R.undistort_points(p, K, D, P, criteria)
        same(slamhip.undistortPoints(p, K, D, P, criteria, ctx=gpu_ctx), want)
    noskew = K.copy()
    noskew[0, 1] = 0
    same(slamhip.undistortPoints(p, noskew, D, P, (5, 0.0), ctx=gpu_ctx), R.undistort_points(p, K, D, P, (5, 0.0)))
    if nd == 12:
        # the strong lens with rational and prism terms added: all three exits
        K0, D5 = calib()
        Dw = np.concatenate([D5, [0.05, -0.02, 0.004, 0.002, -0.001, 0.0015, 0.0007]])
        xy, err, ex, _ = R.undistort_points(p, K0, Dw, P, (50, 0.01), details=True)
        assert len(set(ex.tolist())) == 3
        same(slamhip.undistortPoints(p, K0, Dw, P, (50, 0.01), ctx=gpu_ctx), (xy, err))


def test_in_place_through_the_c_entry(gpu_ctx):
    K, D = calib()
    Kc, Dc = np.ascontiguousarray(K.ravel()), np.ascontiguousarray(D)
    p = points(257, K, D, 3)
    want = R.undistort_points(p, K, D, K, (50, 0.01))
    buf = p.copy()
    err = np.empty(len(p), np.float32)
    rc = L.lib().slam_undistort_points(gpu_ctx.handle, L.ptr(buf), 8, len(buf), L.ptr(Kc), L.ptr(Dc), 5, L.ptr(Kc), 50,
                                       0.01, L.ptr(buf), L.ptr(err))
    L.check(rc, gpu_ctx.handle)
    same((buf, err), want)
    # no residual output
    out = np.empty_like(p)
    rc = L.lib().slam_undistort_points(gpu_ctx.handle, L.ptr(p), 8, len(p), L.ptr(Kc), L.ptr(Dc), 5, L.ptr(Kc), 50,
                                       0.01, L.ptr(out), None)
    L.check(rc, gpu_ctx.handle)
    np.testing.assert_array_equal(out, want[0])


# ---------------- 7. the VGA sample of the CPU suite ----------------

@pytest.mark.parametrize("criteria", [(5, 0.0), (50, 0.01)], ids=lambda c: "%dx%g" % c)
def test_vga_every_seventh_pixel(gpu_ctx, criteria):
    K, D = calib()
    Ks = scaled(K, 1 / 3)
    gx, gy = np.meshgrid(np.arange(640, dtype=np.float32), np.arange(480, dtype=np.float32))
    p = np.stack([gx.ravel(), gy.ravel()], 1)[::7]
    xy, err, ex, it = R.undistort_points(p, Ks, D, Ks, criteria, details=True)
    assert (ex == R.EXIT_ICDIST).any() and (ex == R.EXIT_COUNT).any()
    if criteria[1] > 0:
        assert (ex == R.EXIT_EPS).any() and len(np.unique(it)) >= 30
    same(slamhip.undistortPoints(p, Ks, D, Ks, criteria, ctx=gpu_ctx), (xy, err))


# ---------------- 8. device entry ----------------

def _dev_call(ctx, stream, src, stride, n, K, D, P, criteria, dst, err):
    Kc, Dc = np.ascontiguousarray(K, np.float64).ravel(), np.ascontiguousarray(D, np.float64).ravel()
    Pc = None if P is None else np.ascontiguousarray(P, np.float64).ravel()
    return L.lib().slam_undistort_points_dev(ctx.handle, stream, ctypes.c_void_p(src), stride, n, L.ptr(Kc), L.ptr(Dc),
                                             Dc.size, L.ptr(Pc), criteria[0], criteria[1], ctypes.c_void_p(dst),
                                             None if err is None else ctypes.c_void_p(err))


def test_device_entry_on_a_callers_stream(gpu_ctx):
    """stride 8 and 28, in place, two cameras back to back on one stream"""
    import torch
    K, D = calib()
    K2, D2, P2 = scaled(K, 1 / 3), D12[:8], general_p()
    p = points(10007, K, D, 9)
    k = keypoints(p, 9)
    want1 = R.undistort_points(p, K, D, K, (50, 0.01))
    want2 = R.undistort_points(p, K2, D2, P2, (5, 0.0))
    d_p = torch.from_numpy(p).cuda()
    d_k = torch.from_numpy(k.view(np.uint8).reshape(len(k), 28)).cuda()
    out1 = torch.full((len(p), 2), -7.0, dtype=torch.float32, device="cuda")
    out2 = torch.full((len(p), 2), -7.0, dtype=torch.float32, device="cuda")
    e1 = torch.zeros(len(p), dtype=torch.float32, device="cuda")
    e2 = torch.zeros(len(p), dtype=torch.float32, device="cuda")
    torch.cuda.current_stream().synchronize()
    s = torch.cuda.Stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    L.check(_dev_call(gpu_ctx, sp, d_p.data_ptr(), 8, len(p), K, D, K, (50, 0.01), out1.data_ptr(), e1.data_ptr()),
            gpu_ctx.handle)
    L.check(_dev_call(gpu_ctx, sp, d_k.data_ptr(), 28, len(p), K2, D2, P2, (5, 0.0), out2.data_ptr(), e2.data_ptr()),
            gpu_ctx.handle)
    # in place, after the two reads of d_p's neighbours on the same stream
    L.check(_dev_call(gpu_ctx, sp, d_p.data_ptr(), 8, len(p), K, D, K, (50, 0.01), d_p.data_ptr(), None), gpu_ctx.handle)
    s.synchronize()
    same((out1.cpu().numpy(), e1.cpu().numpy()), want1)
    same((out2.cpu().numpy(), e2.cpu().numpy()), want2)
    np.testing.assert_array_equal(d_p.cpu().numpy(), want1[0])
    np.testing.assert_array_equal(d_k.cpu().numpy(), k.view(np.uint8).reshape(len(k), 28))   # the records are only read


def test_status_codes(gpu_ctx):
    import torch
    K, D = calib()
    n = 16
    src = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    dst = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    err = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.current_stream().synchronize()
    lib, c = L.lib(), gpu_ctx.handle
    a, b, e = src.data_ptr(), dst.data_ptr(), err.data_ptr()

    def dev(src=a, stride=28, n=n, K=K, D=D, criteria=(5, 0.0), dst=b, err=e):
        return _dev_call(gpu_ctx, None, src, stride, n, K, D, K, criteria, dst, err)

    def message():
        return lib.slam_last_error(c).decode()

    assert dev() == L.SLAM_OK
    assert dev(D=np.zeros(14)) == L.SLAM_E_UNSUPPORTED and "tilt" in message()
    for nd in (0, 3, 6, 13):
        assert dev(D=np.zeros(max(nd, 1))[:nd]) == L.SLAM_E_INVALID_ARG and "coefficients" in message()
    assert dev(n=-1) == L.SLAM_E_INVALID_ARG and "count" in message()
    assert dev(src=0) == L.SLAM_E_INVALID_ARG and "null" in message()
    assert dev(dst=0) == L.SLAM_E_INVALID_ARG and "null" in message()
    for criteria in ((0, 0.0), (1001, 0.0), (-3, 0.01), (5, -0.5), (5, float("nan")), (5, float("inf"))):
        assert dev(criteria=criteria) == L.SLAM_E_INVALID_ARG and "criteria" in message(), criteria
    for stride in (0, 4, 7, 10, 30):
        assert dev(stride=stride) == L.SLAM_E_INVALID_ARG and "stride" in message(), stride
    assert dev(src=a + 2) == L.SLAM_E_INVALID_ARG and "aligned" in message()
    assert dev(dst=b + 1) == L.SLAM_E_INVALID_ARG and "aligned" in message()
    assert dev(err=e + 2) == L.SLAM_E_INVALID_ARG and "aligned" in message()
    assert dev(dst=a) == L.SLAM_E_INVALID_ARG and "overlap" in message()       # in place needs stride 8
    assert dev(stride=8, dst=a + 8, n=8) == L.SLAM_E_INVALID_ARG and "overlap" in message()
    assert dev(stride=8, dst=a, n=8) == L.SLAM_OK
    assert dev(n=0) == L.SLAM_OK
    assert dev(n=0, src=0, dst=0, err=None) == L.SLAM_OK                       # no points: nothing is touched
    # null camera or coefficients
    Dc = np.ascontiguousarray(D)
    Kc = np.ascontiguousarray(K).ravel()
    assert lib.slam_undistort_points_dev(c, None, ctypes.c_void_p(a), 28, n, None, L.ptr(Dc), 5, None, 5, 0.0,
                                         ctypes.c_void_p(b), None) == L.SLAM_E_INVALID_ARG
    assert lib.slam_undistort_points_dev(c, None, ctypes.c_void_p(a), 28, n, L.ptr(Kc), None, 5, None, 5, 0.0,
                                         ctypes.c_void_p(b), None) == L.SLAM_E_INVALID_ARG
    assert lib.slam_undistort_points_dev(None, None, ctypes.c_void_p(a), 28, n, L.ptr(Kc), L.ptr(Dc), 5, None, 5, 0.0,
                                         ctypes.c_void_p(b), None) == L.SLAM_E_INVALID_ARG
    # the host entry refuses the same way
    h = np.zeros((n, 2), np.float32)
    assert lib.slam_undistort_points(c, L.ptr(h), 8, n, L.ptr(Kc), L.ptr(Dc), 14, None, 5, 0.0, L.ptr(h),
                                     None) == L.SLAM_E_UNSUPPORTED
    assert lib.slam_undistort_points(c, L.ptr(h), 6, n, L.ptr(Kc), L.ptr(Dc), 5, None, 5, 0.0, L.ptr(h),
                                     None) == L.SLAM_E_INVALID_ARG
    assert lib.slam_undistort_points(c, None, 8, n, L.ptr(Kc), L.ptr(Dc), 5, None, 5, 0.0, L.ptr(h),
                                     None) == L.SLAM_E_INVALID_ARG
    assert lib.slam_undistort_points(c, L.ptr(h), 8, n, L.ptr(Kc), L.ptr(Dc), 5, None, 0, 0.01, L.ptr(h),
                                     None) == L.SLAM_E_INVALID_ARG
    with pytest.raises(slamhip.SlamError) as ei:
        slamhip.undistortPoints(h, K, np.zeros(14), ctx=gpu_ctx)
    assert ei.value.code == L.SLAM_E_UNSUPPORTED
    assert lib.slam_synchronize(c) == L.SLAM_OK


# ---------------- 9, 10. pipeline ----------------

K_VGA = np.array([[1724.676 / 3, 0, 995.966 / 3], [0, 1730.482 / 3, 550.192 / 3], [0, 0, 1.0]])   # tests/test_cycle.py
FILES = ("points.txt", "colors.txt", "poses.txt", "rotations.txt")
REQUIRED_EXTRACTED, REQUIRED_MATCHED = 2000, 300


def _cfg(required=REQUIRED_EXTRACTED):
    d = slamhip.reference_example()
    d.update({"featureExtractingThreshold": 10, "requiredExtractedPointsCount": required, "framesBatchSize": 4,
              "requiredMatchedPointsCount": REQUIRED_MATCHED, "useFM-SIFT-FLANN": False, "useFM-SIFT-BF": True,
              "useFM-ORB": False, "useBundleAdjustment": False, "BAMaxFramesCnt": 4})
    return slamhip.ConfigService(d)


def _run(media, cfg, ops, out_dir, **kw):
    gd, logs = cycle.slam_main(media, K_VGA.copy(), cfg, ops, out_dir=str(out_dir), **kw)
    return logs, {f: open(os.path.join(out_dir, f), "rb").read() for f in FILES}


def _oracle_ops():
    from oracle_ops import OracleOps

    class RefPointsOps(OracleOps):
        """the CPU oracle with the numpy restatement of cv::undistortPoints"""

        def undistort_points(self, kps, K, dist, P=None, criteria=(5, 0.0)):
            return R.undistort_points(np.stack([kps["x"], kps["y"]], 1), K, dist, P, criteria)

    return RefPointsOps()


@pytest.fixture(scope="module")
def seq16():
    return slamhip.synth_frames(640, 480, 0, 16, seed=1234)


@pytest.fixture(scope="module")
def oracle_runs(seq16, tmp_path_factory):
    """the CPU oracle's files without coefficients and with undistort="points",
    and what the validity filter took from each winner's match list"""
    _, D = calib()
    out = tmp_path_factory.mktemp("oracle")
    lg, today = _run(cycle.MediaSources(list(seq16)), _cfg(), _oracle_ops(), out / "today")
    assert len(lg.pose_list) >= 3
    lost = []
    orig = cycle.drop_invalid_matches

    def spy(prev, nxt, matches):
        kept = orig(prev, nxt, matches)
        lost.append(len(matches) - len(kept))
        return kept

    cycle.drop_invalid_matches = spy
    try:
        lg, pts = _run(cycle.MediaSources(list(seq16)), _cfg(), _oracle_ops(), out / "points", dist=D,
                       undistort="points")
    finally:
        cycle.drop_invalid_matches = orig
    return today, pts, len(lg.pose_list), lost


def test_pipeline_undistorts_the_keypoints(gpu_ctx, seq16, oracle_runs, tmp_path):
    """slam_main(dist=DC, undistort="points") over GpuOps writes the files of the
    same call over the CPU oracle with the numpy cv::undistortPoints, from
    MediaSources and from DeviceMedia, and never remaps a frame.

    requiredExtractedPointsCount 2000 and requiredMatchedPointsCount 300, the
    values of the run without coefficients (the raw frames are what FAST sees
    in this mode): the oracle run then logs 5 poses, each of its 4 winners loses
    between 281 and 316 of about 1500 matches to the validity filter, and all
    four files differ from the run without coefficients."""
    import torch
    _, D = calib()
    today, want, poses, lost = oracle_runs
    assert poses >= 3
    assert len(lost) == poses - 1 and min(lost) >= 1
    for name in FILES:
        assert want[name] != today[name], name
    ops = cycle.GpuOps(gpu_ctx)
    remaps = []
    ops.undistort = lambda *a, **k: remaps.append(1) or pytest.fail("undistort=\"points\" remapped a frame")
    und = slamhip.api.undistortBatch
    try:
        cycle_calls = []
        slamhip.api.undistortBatch = lambda *a, **k: cycle_calls.append(1) or und(*a, **k)
        _, got = _run(cycle.MediaSources(list(seq16)), _cfg(), ops, tmp_path / "media", dist=D, undistort="points")
        for name in FILES:
            assert got[name] == want[name], name
        dev = torch.from_numpy(np.ascontiguousarray(seq16)).cuda()
        torch.cuda.current_stream().synchronize()
        _, got = _run(cycle.DeviceMedia(seq16, dev), _cfg(), ops, tmp_path / "dev", dist=D, undistort="points")
        for name in FILES:
            assert got[name] == want[name], name
    finally:
        slamhip.api.undistortBatch = und
    assert not remaps and not cycle_calls


def test_pipeline_unchanged_paths(gpu_ctx, seq16, oracle_runs, tmp_path):
    """undistort="points" without coefficients, or with all-zero ones, writes
    today's files; undistort="frames" is the default path"""
    _, D = calib()
    today = oracle_runs[0]
    ops = cycle.GpuOps(gpu_ctx)
    _, none = _run(cycle.MediaSources(list(seq16)), _cfg(), ops, tmp_path / "none", dist=None, undistort="points")
    _, zeros = _run(cycle.MediaSources(list(seq16)), _cfg(), ops, tmp_path / "zeros", dist=np.zeros(5),
                    undistort="points")
    for name in FILES:
        assert none[name] == today[name], name
        assert zeros[name] == today[name], name
    # "frames": the files of a run over frames undistorted beforehand by the reference
    # (tests/test_undistort_gpu.py has the run and its requiredExtractedPointsCount of 1000)
    xy, frac = U.undistort_map(640, 480, K_VGA, D)
    pre = np.stack([U.remap(f, xy, frac) for f in seq16])
    lg, want = _run(cycle.MediaSources(list(pre)), _cfg(1000), ops, tmp_path / "pre")
    assert len(lg.pose_list) >= 3
    _, frames = _run(cycle.MediaSources(list(seq16)), _cfg(1000), ops, tmp_path / "frames", dist=D,
                     undistort="frames")
    _, default = _run(cycle.MediaSources(list(seq16)), _cfg(1000), ops, tmp_path / "default", dist=D)
    for name in FILES:
        assert frames[name] == want[name], name
        assert default[name] == want[name], name
    with pytest.raises(ValueError):
        cycle.slam_main(cycle.MediaSources([]), K_VGA.copy(), _cfg(), ops, dist=D, undistort="pixels")

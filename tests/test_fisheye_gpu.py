"""GPU tests of the fisheye lens model on the device (fisheye_map and
fisheye_points in csrc/fisheye.hip behind the slam_fisheye_undistort* entry
points): maps, frames, points and residuals equal the numpy definition
(tests/fisheye_ref.py) byte for byte, the context's map cache tells the two
lens models apart, and slam_main(lens_model="fisheye") hands the search the
definition's frames, or geometry the definition's points.
"""
import ctypes

import numpy as np
import pytest

import fisheye_ref as F
import slamhip
import undistort_ref as U
from slamhip import _lib as L
from slamhip import cycle
from test_fisheye import FOLD_D, STRONG_D, half, integer_camera

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (161, 97), (748, 480)]


def prototype(w, h):
    return F.CAMERA_K * np.array([[w / 748], [h / 480], [1]])


def frames(n, w, h, ch, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w, ch) if ch == 3 else (n, h, w), dtype=np.uint8)


# ---------------- the map ----------------

@pytest.mark.parametrize("w,h", SIZES)
def test_map_equals_the_definition(gpu_ctx, w, h):
    for K, D, newK in ((prototype(w, h), F.CAMERA_D, None), (integer_camera(w, h), STRONG_D, half(integer_camera(w, h)))):
        want = F.fisheye_map(w, h, K, D, newK)
        got = slamhip.fisheyeUndistortMap(w, h, K, D, newK, ctx=gpu_ctx)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
    # the strong lens on an integer principal point: the centre pixel takes the r == 0 branch
    assert tuple(want[0][h // 2, w // 2]) == (w // 2, h // 2) and want[1][h // 2, w // 2] == 0


# ---------------- frames ----------------

@pytest.mark.parametrize("ch", [1, 3])
def test_frames_equal_the_definitions_remap(gpu_ctx, ch):
    import torch
    w, h = 161, 97
    K, D = integer_camera(w, h), STRONG_D
    newK = half(K)
    xy, frac = F.fisheye_map(w, h, K, D, newK)
    src = frames(3, w, h, ch, 5 + ch)
    want = np.stack([U.remap(f, xy, frac) for f in src])
    # one host frame, then the batch of three in one launch
    np.testing.assert_array_equal(slamhip.fisheyeUndistort(src[0], K, D, newK, ctx=gpu_ctx), want[0])
    dev = torch.from_numpy(src).cuda()
    out = slamhip.fisheyeUndistortBatch(dev, K, D, newK, ctx=gpu_ctx)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    assert want.any() and (want == 0).any()          # the half-scale view shows the source's border


# ---------------- points ----------------

def points(n, K, seed):
    """n points over and around a 748 x 480 image, the special ones first: the
    centre, its float neighbour, |pw| beyond pi/2, a NaN and an infinity"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-100, 850, n), rng.uniform(-100, 580, n)], 1).astype(np.float32)
    whole = rng.random(n) < 0.3
    p[whole] = np.round(p[whole])
    special = np.array([[K[0, 2], K[1, 2]], [K[0, 2] + 1e-5, K[1, 2]], [5000, 5000], [-1e6, 1e6], [np.nan, 3],
                        [np.inf, 7], [0, 0], [747, 479]], np.float32)
    m = min(n, len(special))
    p[:m] = special[:m]
    return p


def keypoints(p, seed):
    rng = np.random.default_rng(seed)
    k = np.zeros(len(p), L.KEYPOINT_DTYPE)
    k["x"], k["y"] = p[:, 0], p[:, 1]
    k["size"], k["angle"], k["response"] = 7.0, rng.uniform(0, 360, len(p)), rng.uniform(10, 250, len(p))
    k["octave"], k["class_id"] = rng.integers(0, 1 << 30, len(p)), -1
    return k


def same(got, want):
    np.testing.assert_array_equal(got[0], want[0], err_msg="points")
    np.testing.assert_array_equal(got[1], want[1], err_msg="residuals")        # NaN where the definition has NaN


@pytest.mark.parametrize("criteria", [(10, 1e-8), (10, 0.0), (3, 1e-8)], ids=lambda c: "%dx%g" % c)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_points_equal_the_definition(gpu_ctx, n, criteria):
    K = integer_camera(748, 480)
    p = points(n, K, 100 + n)
    for D, P in ((FOLD_D, K), (F.CAMERA_D, None), (STRONG_D, half(K))):
        want = F.undistort_points(p, K, D, P, criteria)
        same(slamhip.fisheyeUndistortPoints(p, K, D, P, criteria, ctx=gpu_ctx), want)
        k = keypoints(p, n)                                                     # stride 28, read in place
        before = k.copy()
        same(slamhip.fisheyeUndistortPoints(k, K, D, P, criteria, ctx=gpu_ctx), want)
        assert k.tobytes() == before.tobytes()


def test_points_take_every_exit(gpu_ctx):
    K = integer_camera(748, 480)
    p = points(1000, K, 7)
    xy, err, ex, it = F.undistort_points(p, K, FOLD_D, K, (10, 1e-8), details=True)
    assert set(ex.tolist()) == {F.EXIT_CENTRE, F.EXIT_EPS, F.EXIT_NOT_CONVERGED, F.EXIT_FLIPPED}
    assert ex[0] == F.EXIT_CENTRE and ex[2] != F.EXIT_EPS and len(np.unique(it)) >= 5
    rejected = np.isin(ex, (F.EXIT_NOT_CONVERGED, F.EXIT_FLIPPED))
    assert (xy[rejected] == F.REJECTED).all() and np.isnan(err[rejected]).all()
    got = slamhip.fisheyeUndistortPoints(p, K, FOLD_D, K, (10, 1e-8), ctx=gpu_ctx)
    same(got, (xy, err))
    assert not (got[1][rejected] <= 0.01).any()        # consumers test err <= tol


def _dev_call(ctx, stream, src, stride, n, K, D, P, criteria, dst, err, entry="slam_fisheye_undistort_points_dev"):
    Kc = None if K is None else np.ascontiguousarray(K, np.float64).ravel()
    Dc = None if D is None else np.ascontiguousarray(D, np.float64).ravel()
    Pc = None if P is None else np.ascontiguousarray(P, np.float64).ravel()
    return getattr(L.lib(), entry)(ctx.handle, stream, ctypes.c_void_p(src), stride, n, L.ptr(Kc), L.ptr(Dc),
                                   0 if Dc is None else Dc.size, L.ptr(Pc), criteria[0], criteria[1],
                                   ctypes.c_void_p(dst), None if err is None else ctypes.c_void_p(err))


def test_device_entry_in_place(gpu_ctx):
    import torch
    K = integer_camera(748, 480)
    p = points(1000, K, 9)
    want = F.undistort_points(p, K, FOLD_D, K, (10, 1e-8))
    d_p = torch.from_numpy(p).cuda()
    out = torch.full((len(p), 2), -7.0, dtype=torch.float32, device="cuda")
    e = torch.zeros(len(p), dtype=torch.float32, device="cuda")
    torch.cuda.current_stream().synchronize()
    L.check(_dev_call(gpu_ctx, None, d_p.data_ptr(), 8, len(p), K, FOLD_D, K, (10, 1e-8), out.data_ptr(), e.data_ptr()),
            gpu_ctx.handle)
    L.check(_dev_call(gpu_ctx, None, d_p.data_ptr(), 8, len(p), K, FOLD_D, K, (10, 1e-8), d_p.data_ptr(), None),
            gpu_ctx.handle)
    assert L.lib().slam_synchronize(gpu_ctx.handle) == L.SLAM_OK
    same((out.cpu().numpy(), e.cpu().numpy()), want)
    np.testing.assert_array_equal(d_p.cpu().numpy(), want[0])


def test_status_codes(gpu_ctx):
    import torch
    K, D = integer_camera(748, 480), F.CAMERA_D
    n = 16
    src = torch.zeros((n, 7), dtype=torch.float32, device="cuda")
    dst = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    err = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.current_stream().synchronize()
    lib, c = L.lib(), gpu_ctx.handle
    a, b, e = src.data_ptr(), dst.data_ptr(), err.data_ptr()

    def dev(src=a, stride=28, n=n, K=K, D=D, criteria=(10, 1e-8), dst=b, err=e):
        return _dev_call(gpu_ctx, None, src, stride, n, K, D, K, criteria, dst, err)

    def message():
        return lib.slam_last_error(c).decode()

    assert dev() == L.SLAM_OK
    for nd in (0, 3, 5, 8, 12, 14):
        assert dev(D=np.zeros(max(nd, 1))[:nd] if nd else None) == L.SLAM_E_INVALID_ARG, nd
    assert dev(D=np.zeros(5)) == L.SLAM_E_INVALID_ARG and "4 distortion" in message()
    assert dev(D=np.array([0, np.nan, 0, 0])) == L.SLAM_E_INVALID_ARG and "finite" in message()
    assert dev(K=None) == L.SLAM_E_INVALID_ARG and "null" in message()
    assert dev(n=-1) == L.SLAM_E_INVALID_ARG and "count" in message()
    assert dev(src=0) == L.SLAM_E_INVALID_ARG and "null" in message()
    assert dev(dst=0) == L.SLAM_E_INVALID_ARG and "null" in message()
    for criteria in ((0, 0.0), (1001, 0.0), (5, -0.5), (5, float("nan")), (5, float("inf"))):
        assert dev(criteria=criteria) == L.SLAM_E_INVALID_ARG and "criteria" in message(), criteria
    for stride in (0, 4, 7, 10, 30):
        assert dev(stride=stride) == L.SLAM_E_INVALID_ARG and "stride" in message(), stride
    assert dev(src=a + 2) == L.SLAM_E_INVALID_ARG and "aligned" in message()
    assert dev(dst=a) == L.SLAM_E_INVALID_ARG and "overlap" in message()       # in place needs stride 8
    assert dev(stride=8, dst=a, n=8) == L.SLAM_OK
    assert dev(n=0, src=0, dst=0, err=None) == L.SLAM_OK                       # no points: nothing is touched
    # frames and the map
    w, h = 64, 48
    Kf = integer_camera(w, h)
    f = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    o = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()

    def batch(src=f.data_ptr(), dst=o.data_ptr(), nframes=2, K=Kf, D=D, newK=None, ch=1):
        Kc, Dc = np.ascontiguousarray(K, np.float64).ravel(), np.ascontiguousarray(D, np.float64).ravel()
        Nc = None if newK is None else np.ascontiguousarray(newK, np.float64).ravel()
        return lib.slam_fisheye_undistort_batch(c, None, ctypes.c_void_p(src), ctypes.c_void_p(dst), nframes, w, h, ch,
                                                L.ptr(Kc), L.ptr(Dc), Dc.size, L.ptr(Nc))

    assert batch() == L.SLAM_OK
    assert batch(nframes=0, src=0, dst=0) == L.SLAM_OK                          # no frames: no map, no launch
    assert batch(nframes=-1) == L.SLAM_E_INVALID_ARG
    assert batch(ch=2) == L.SLAM_E_INVALID_ARG
    assert batch(src=0) == L.SLAM_E_INVALID_ARG and "null" in message()
    assert batch(dst=f.data_ptr()) == L.SLAM_E_INVALID_ARG and "overlap" in message()
    assert batch(D=np.zeros(5)) == L.SLAM_E_INVALID_ARG and "4 distortion" in message()
    assert batch(D=np.array([np.inf, 0, 0, 0])) == L.SLAM_E_INVALID_ARG and "finite" in message()
    singular = Kf.copy()
    singular[0, 0] = 0
    assert batch(newK=singular) == L.SLAM_E_INVALID_ARG and "singular" in message()
    projective = Kf.copy()
    projective[2, 0] = 1e-4
    assert batch(newK=projective) == L.SLAM_E_INVALID_ARG and "last row" in message()
    with pytest.raises(slamhip.SlamError):
        slamhip.fisheyeUndistortMap(w, h, Kf, np.zeros(5), ctx=gpu_ctx)
    assert lib.slam_synchronize(c) == L.SLAM_OK


# ---------------- the map cache ----------------

@pytest.mark.parametrize("first", ["brown", "fisheye"])
def test_map_cache_tells_the_models_apart(gpu_ctx, first):
    """the same K and the same four numbers as k1 k2 p1 p2 and as k1 k2 k3 k4,
    one after the other in either order: each call gets its own model's map"""
    w, h = 161, 97
    K = integer_camera(w, h)
    D = np.array([-0.3, 0.1, 0.002, -0.001])
    src = frames(1, w, h, 3, 3)[0]
    brown = U.remap(src, *U.undistort_map(w, h, K, D))
    fish = U.remap(src, *F.fisheye_map(w, h, K, D))
    assert not np.array_equal(brown, fish)
    order = ["brown", "fisheye", "brown"] if first == "brown" else ["fisheye", "brown", "fisheye"]
    ctx = slamhip.Context(0)       # a cache of its own: nothing left by other tests
    try:
        for model in order:
            if model == "brown":
                np.testing.assert_array_equal(slamhip.undistort(src, K, D, ctx=ctx), brown, err_msg=model)
            else:
                np.testing.assert_array_equal(slamhip.fisheyeUndistort(src, K, D, ctx=ctx), fish, err_msg=model)
    finally:
        ctx.close()


# ---------------- the pipeline ----------------

W, H = 160, 120
K_SMALL = np.array([[60.0, 0, 80], [0, 60.0, 60], [0, 0, 1.0]])
NEW_K = np.array([[40.0, 0, 80], [0, 40.0, 60], [0, 0, 1.0]])
K_POINTS = np.array([[120.0, 0, 80], [0, 120.0, 60], [0, 0, 1.0]])


def _cfg():
    d = slamhip.reference_example()
    d.update({"featureExtractingThreshold": 10, "requiredExtractedPointsCount": 50, "framesBatchSize": 3,
              "requiredMatchedPointsCount": 20, "useFM-SIFT-FLANN": False, "useFM-SIFT-BF": True,
              "useFM-ORB": False, "useBundleAdjustment": False, "BAMaxFramesCnt": 3})
    return slamhip.ConfigService(d)


@pytest.fixture(scope="module")
def seq6():
    return slamhip.synth_frames(W, H, 0, 6, seed=1234)


def test_pipeline_frames(gpu_ctx, seq6, tmp_path):
    """undistort="frames": every frame the search is handed is the definition's remap of a source frame, in order"""
    xy, frac = F.fisheye_map(W, H, K_SMALL, F.CAMERA_D, NEW_K)
    want = [U.remap(f, xy, frac) for f in seq6]
    ops = cycle.GpuOps(gpu_ctx)
    seen = []
    inner = ops.undistort

    def spy(frame, K, dist, newK=None, **kw):
        assert kw == {"lens_model": "fisheye"}
        out = inner(frame, K, dist, newK, **kw)
        seen.append(np.array(out))
        return out

    ops.undistort = spy
    cycle.slam_main(cycle.MediaSources(list(seq6)), K_SMALL.copy(), _cfg(), ops, out_dir=str(tmp_path), dist=F.CAMERA_D,
                    newK=NEW_K, lens_model="fisheye")
    assert len(seen) >= 2
    for got, ref in zip(seen, want):
        np.testing.assert_array_equal(got, ref)
    # a resident sequence goes through one slam_fisheye_undistort_batch
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(seq6)).cuda()
    torch.cuda.current_stream().synchronize()
    media = cycle.UndistortedMedia(cycle.DeviceMedia(seq6, dev), K_SMALL, F.CAMERA_D, ops, NEW_K, "fisheye")
    for ref in want:
        np.testing.assert_array_equal(np.array(media.next_frame()), ref)


def test_pipeline_points(gpu_ctx, seq6, tmp_path):
    """undistort="points": the coordinates and validity masks geometry reads are the definition's"""
    ops = cycle.GpuOps(gpu_ctx)
    ops.undistort = lambda *a, **k: pytest.fail('undistort="points" remapped a frame')
    calls = []
    holder = cycle.TemporalImageData.allExtractedFeatures.fset

    def spy(self, v):
        holder(self, v)
        if self.lens is not None:
            calls.append((np.array(v), self.undistorted, self.valid))

    criteria, tol = (10, 1e-8), 0.01
    cycle.TemporalImageData.allExtractedFeatures = property(cycle.TemporalImageData.allExtractedFeatures.fget, spy)
    try:
        cycle.slam_main(cycle.MediaSources(list(seq6)), K_POINTS.copy(), _cfg(), ops, out_dir=str(tmp_path),
                        dist=FOLD_D, newK=NEW_K, undistort="points", criteria=criteria, max_residual=tol,
                        lens_model="fisheye")
    finally:
        cycle.TemporalImageData.allExtractedFeatures = property(cycle.TemporalImageData.allExtractedFeatures.fget, holder)
    assert calls and max(len(k) for k, _, _ in calls) >= 50
    for kps, xy, valid in calls:
        wxy, werr = F.undistort_points(np.stack([kps["x"], kps["y"]], 1), K_POINTS, FOLD_D, NEW_K, criteria)
        np.testing.assert_array_equal(xy, wxy)
        np.testing.assert_array_equal(valid, werr <= np.float32(tol))
    # the lens itself over every fourth pixel: FOLD_D folds 84 pixels from the centre, so the corners have no position
    gx, gy = np.meshgrid(np.arange(0, W, 4, dtype=np.float32), np.arange(0, H, 4, dtype=np.float32))
    grid = np.stack([gx.ravel(), gy.ravel()], 1)
    lens = cycle.PointLens(cycle.GpuOps(gpu_ctx), K_POINTS, FOLD_D, NEW_K, criteria, tol, "fisheye")
    xy, valid = lens(keypoints(grid, 1))
    wxy, werr = F.undistort_points(grid, K_POINTS, FOLD_D, NEW_K, criteria)
    np.testing.assert_array_equal(xy, wxy)
    np.testing.assert_array_equal(valid, werr <= np.float32(tol))
    assert valid.any() and (~valid).any() and (xy[~valid] == F.REJECTED).all()


# ---------------- calibration from the committed photos ----------------

def test_photos_calibration_on_the_device(gpu_ctx):
    """decode, candidates and cornerSubPix on the device, the growing labeller and
    the solver on the host: the definition's boards, and the camera of the CPU
    test's solve on the definition's corners"""
    import calib_ref as C
    from slamhip import calibration
    from test_fisheye import BOARD, PHOTOS, real_corners
    names, want = real_corners()
    rms, K, D, R, T, pts = calibration.chessboard_photos_calibration(PHOTOS, 15, 1.0, BOARD, ctx=gpu_ctx, with_corners=True,
                                                                     decoder="gpu", model="fisheye")
    assert len(pts) == len(names) >= calibration.MINIMAL_FOUND_FRAMES_COUNT
    np.testing.assert_array_equal(pts, want)
    ref = slamhip.fisheyeCalibrate(C.board_points(BOARD, 1.0), want, (748, 480))
    assert abs(rms - ref[0]) <= 1e-9 and np.abs(K - ref[1]).max() <= 1e-9 and np.abs(D - ref[2]).max() <= 1e-9
    assert D.shape == (4,) and len(R) == len(T) == len(names)

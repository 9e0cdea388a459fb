"""GPU tests of undistortion (csrc/undistort.hip behind slam_undistort_batch,
slam_undistort and slam_undistort_map): for every case the device map (xy, frac)
and the device image equal the numpy restatement of cv::undistort
(tests/undistort_ref.py) exactly.

Fixture: tests/golden/calib_samsung_hv.xml is a copy of the reference's
config/samsung-hv.xml (K, DC, R, T as its calibration step writes them,
IOmisc.cpp:68-76); settings only.  The photos are those of
tests/golden/make_real_fixtures.py.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import slamhip
import undistort_ref as U
from slamhip import _lib as L
from slamhip import cycle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CALIB = os.path.join(GOLDEN, "calib_samsung_hv.xml")

# undist_remap's tile and frame chunk (csrc/slamhip_internal.h: kUndistTileW, kUndistTileH, kUndistFrames)
TILE_W, TILE_H, F = 128, 8, 8

ZERO5 = np.zeros(5)
# a mild lens for the shape tests: every term of the 5-coefficient model at work
MILD = np.array([-0.21, 0.07, 0.0013, -0.0021, 0.011])


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
    """a camera that fits a w x h frame, principal point off-centre"""
    f = 0.9 * max(w, h, 4)
    return np.array([[f, 0, w / 2 + 0.31], [0, 1.01 * f, h / 2 - 0.17], [0, 0, 1.0]])


def frames(n, w, h, ch, seed, low=0):
    rng = np.random.default_rng(seed)
    return rng.integers(low, 256, (n, h, w, ch) if ch > 1 else (n, h, w), dtype=np.uint8)


def device_undistort(ctx, src, K, D, newK=None, stream=None):
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    torch.cuda.current_stream().synchronize()
    out = slamhip.undistortBatch(dev, K, D, newK, ctx=ctx, stream=stream)
    if stream is not None:
        L.check(L.lib().slam_order_after(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                         stream), ctx.handle)
    return out.cpu().numpy()


def check_case(ctx, src, K, D, newK=None):
    """map and image against the reference; returns the reference's (xy, frac, taps)"""
    h, w = src.shape[1:3]
    xy, frac = U.undistort_map(w, h, K, D, newK)
    gxy, gfrac = slamhip.undistortMap(w, h, K, D, newK, ctx=ctx)
    np.testing.assert_array_equal(gxy, xy)
    np.testing.assert_array_equal(gfrac, frac)
    got = device_undistort(ctx, src, K, D, newK)
    assert got.shape == src.shape
    for f in range(len(src)):
        np.testing.assert_array_equal(got[f], U.remap(src[f], xy, frac), err_msg=f"frame {f}")
    return xy, frac, U.taps(xy, w, h)


# ---------------- real lens, real photos ----------------

def test_real_lens_1080p(gpu_ctx):
    K, D = calib()
    src = np.load(os.path.join(GOLDEN, "real_1080p.npz"))["bgr"]
    xy, frac, ok = check_case(gpu_ctx, src, K, D)
    assert int((ok.any(-1) & ~ok.all(-1)).sum()) == 201     # a tap outside the source
    assert int((~ok.any(-1)).sum()) == 0                    # none fully outside


def test_real_lens_vga_four_frames_one_launch(gpu_ctx):
    K, D = calib()
    src = np.load(os.path.join(GOLDEN, "real_vga.npz"))["bgr"]
    assert src.shape == (4, 480, 640, 3)
    check_case(gpu_ctx, src, scaled(K, 1 / 3), D)


def test_real_lens_gray_frames(gpu_ctx):
    K, D = calib()
    src = np.load(os.path.join(GOLDEN, "real_vga.npz"))["gray"]
    assert src.shape == (2, 480, 748)
    check_case(gpu_ctx, src, scaled(K, 748 / 1920), D)


# ---------------- the tie family: every u * 32 on a half ----------------

@pytest.mark.parametrize("w,h", [(200, 37), (333, 70), (2100, 5)])
def test_tie_family(gpu_ctx, w, h):
    K, nk = U.tie_family(w, h)
    if w == 2100:
        assert U.stripe_rows(w, h) == 1
    check_case(gpu_ctx, frames(2, w, h, 3, 10 + w), K, ZERO5, nk)


# ---------------- border ----------------

def test_border_constant(gpu_ctx):
    K, D = calib()
    K = scaled(K, 1 / 6)
    nk = K.copy()
    nk[0, 0] /= 2
    nk[1, 1] /= 2
    xy, frac, ok = check_case(gpu_ctx, frames(2, 320, 180, 3, 21, low=1), K, D, nk)
    outside = ~ok.any(-1)
    assert outside.mean() >= 0.25
    assert int((ok.any(-1) & ~ok.all(-1)).sum()) > 0        # some straddle the border
    check_case(gpu_ctx, frames(1, 320, 180, 1, 22, low=1), K, ZERO5, nk)


# ---------------- kept quirks ----------------

def test_short_wrap_samples_inside(gpu_ctx):
    w, h = 640, 8
    K = np.array([[500.0, 0, 1.5], [0, 500.0, h / 2], [0, 0, 1.0]])
    nk = K.copy()
    nk[0, 0] = K[0, 0] / 103
    src = frames(2, w, h, 3, 31, low=1)
    iu, _ = U.fixed_point(w, h, K, ZERO5, nk)
    xy, frac, ok = check_case(gpu_ctx, src, K, ZERO5, nk)
    wrapped = (iu >> 5) >= 65536
    assert wrapped.any()
    ref = U.remap(src[0], xy, frac)
    assert ref[wrapped].any()          # pixels sampled through the wrap, not border zeros


def test_int_min_conversion(gpu_ctx):
    w, h = 640, 8
    K = np.array([[500.0, 0, 1.5], [0, 500.0, h / 2], [0, 0, 1.0]])
    nk = K.copy()
    nk[0, 0] = K[0, 0] / 2 ** 20
    iu, _ = U.fixed_point(w, h, K, ZERO5, nk)
    assert (iu == U.INT_MIN).any()
    check_case(gpu_ctx, frames(1, w, h, 3, 32, low=1), K, ZERO5, nk)


# ---------------- sizes ----------------

SIZES = [(1, 1), (1, 7), (7, 1), (3, 3), (5, 4), (333, 251)]
TILE_SIZES = [(TILE_W + dw, TILE_H + dh) for dw in (-1, 0, 1) for dh in (-1, 0, 1)]


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h", SIZES + TILE_SIZES)
def test_sizes(gpu_ctx, w, h, ch):
    """odd row and frame strides: with 3 frames, frames 1 and 2 start unaligned"""
    check_case(gpu_ctx, frames(3, w, h, ch, 100 * w + h + ch), camera(w, h), MILD)


def test_frame_counts(gpu_ctx):
    w, h = 37, 21
    K = camera(w, h)
    src = frames(F + 1, w, h, 3, 41)
    xy, frac = U.undistort_map(w, h, K, MILD)
    ref = np.stack([U.remap(f, xy, frac) for f in src])
    for n in (0, 1, F - 1, F, F + 1):
        got = device_undistort(gpu_ctx, src[:n], K, MILD)
        assert got.shape == (n, h, w, 3)
        np.testing.assert_array_equal(got, ref[:n], err_msg=f"n = {n}")


def test_unaligned_views_of_a_sequence(gpu_ctx):
    """source and destination that start inside a larger allocation at odd byte offsets"""
    import torch
    w, h, n = 35, 9, 5                      # 945-byte frames
    K = camera(w, h)
    src = frames(n, w, h, 3, 43)
    xy, frac = U.undistort_map(w, h, K, MILD)
    dev = torch.from_numpy(src).cuda()
    out = torch.zeros_like(dev)
    torch.cuda.current_stream().synchronize()
    slamhip.undistortBatch(dev[1:4], K, MILD, ctx=gpu_ctx, out=out[2:5])
    got = out.cpu().numpy()
    assert not got[:2].any()
    for k in range(3):
        np.testing.assert_array_equal(got[2 + k], U.remap(src[1 + k], xy, frac))


# ---------------- wider models ----------------

@pytest.mark.parametrize("nd", [4, 8, 12])
def test_rational_and_prism_models_skewed_camera(gpu_ctx, nd):
    w, h = 161, 67
    K = camera(w, h)
    K[0, 1] = 0.8                           # skew: every row starts elsewhere
    nk = K.copy()
    nk[0, 1] = 1.3
    nk[0, 2] += 0.4
    D = np.array([-0.21, 0.07, 0.0013, -0.0021, 0.011, 0.05, -0.02, 0.004, 0.002, -0.001, 0.0015, 0.0007])[:nd]
    check_case(gpu_ctx, frames(2, w, h, 3, 50 + nd), K, D, nk)


# ---------------- the cached map ----------------

def test_map_cache_follows_the_camera(gpu_ctx):
    import torch
    w, h = 150, 40
    K1 = camera(w, h)
    K2 = scaled(K1, 1.1)
    a, b = frames(2, w, h, 3, 61), frames(2, w, h, 3, 62)
    ctx = slamhip.Context(0)
    s = torch.cuda.Stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    try:
        for K, src in ((K1, a), (K2, a), (K1, b), (K1, a)):     # K1's map serves two frame sets
            xy, frac = U.undistort_map(w, h, K, MILD)
            got = device_undistort(ctx, src, K, MILD, stream=sp)
            for f in range(2):
                np.testing.assert_array_equal(got[f], U.remap(src[f], xy, frac))
            gxy, gfrac = slamhip.undistortMap(w, h, K, MILD, ctx=ctx)
            np.testing.assert_array_equal(gxy, xy)
            np.testing.assert_array_equal(gfrac, frac)
        # another size, coefficient set and newK each rebuild it
        check_case(ctx, frames(1, w + 1, h, 3, 63), camera(w + 1, h), MILD)
        check_case(ctx, frames(1, w + 1, h, 3, 63), camera(w + 1, h), MILD * 0.5)
        check_case(ctx, frames(1, w + 1, h, 3, 63), camera(w + 1, h), MILD * 0.5, scaled(camera(w + 1, h), 0.9))
    finally:
        ctx.close()


# ---------------- host entry ----------------

def test_host_entry_strided_rows(gpu_ctx):
    w, h = 131, 23
    K = camera(w, h)
    wide = frames(1, w + 9, h, 3, 71)[0]
    src = wide[:, 4:4 + w]                                     # step = 3 (w + 9)
    assert src.strides[0] > 3 * w
    ref = U.undistort(np.ascontiguousarray(src), K, MILD)
    np.testing.assert_array_equal(slamhip.undistort(src, K, MILD, ctx=gpu_ctx), ref)
    # output rows strided too, through the C entry; the padding stays untouched
    out = np.full((h, 3 * w + 7), 0xAB, np.uint8)
    Kc, Dc = np.ascontiguousarray(K.ravel()), np.ascontiguousarray(MILD)
    rc = L.lib().slam_undistort(gpu_ctx.handle, L.ptr(src), w, h, src.strides[0], 3, L.ptr(Kc), L.ptr(Dc), 5, None,
                                L.ptr(out), out.strides[0])
    L.check(rc, gpu_ctx.handle)
    np.testing.assert_array_equal(out[:, :3 * w].reshape(h, w, 3), ref)
    assert (out[:, 3 * w:] == 0xAB).all()
    gray = frames(1, w, h, 1, 72)[0]
    np.testing.assert_array_equal(slamhip.undistort(gray, K, MILD, ctx=gpu_ctx), U.undistort(gray, K, MILD))


# ---------------- status codes ----------------

def test_status_codes(gpu_ctx):
    import torch
    w, h = 16, 8
    K = camera(w, h)
    dev = torch.zeros((3, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.current_stream().synchronize()
    lib, c = L.lib(), gpu_ctx.handle
    Kc = np.ascontiguousarray(K.ravel())
    D = np.zeros(14)
    p = dev.data_ptr()
    fb = w * h * 3

    def batch(src, dst, n, ndist, newK=None):
        return lib.slam_undistort_batch(c, None, ctypes.c_void_p(src), ctypes.c_void_p(dst), n, w, h, 3, L.ptr(Kc),
                                        L.ptr(D), ndist, L.ptr(newK))

    def message():
        return lib.slam_last_error(c).decode()

    assert batch(p, p + fb, 2, 5) == L.SLAM_E_INVALID_ARG and "overlap" in message()
    assert batch(p, p, 1, 5) == L.SLAM_E_INVALID_ARG and "overlap" in message()
    assert batch(p, p + 2 * fb, 1, 14) == L.SLAM_E_UNSUPPORTED and "tilt" in message()
    assert batch(p, p + 2 * fb, 1, 3) == L.SLAM_E_INVALID_ARG and "coefficients" in message()
    singular = np.array([1.0, 0, 0, 2.0, 0, 0, 0, 0, 1.0])
    assert batch(p, p + 2 * fb, 1, 5, singular) == L.SLAM_E_INVALID_ARG and "singular" in message()
    assert batch(p, p + fb, 0, 5) == L.SLAM_OK                 # no frames: a success, nothing launched
    assert batch(p, p + 2 * fb, 1, 5) == L.SLAM_OK
    with pytest.raises(slamhip.SlamError) as e:
        slamhip.undistortMap(w, h, K, np.zeros(14), ctx=gpu_ctx)
    assert e.value.code == L.SLAM_E_UNSUPPORTED
    gpu_ctx_sync = lib.slam_synchronize(c)
    assert gpu_ctx_sync == L.SLAM_OK


# ---------------- pipeline ----------------

K_VGA = np.array([[1724.676 / 3, 0, 995.966 / 3], [0, 1730.482 / 3, 550.192 / 3], [0, 0, 1.0]])   # tests/test_cycle.py
FILES = ("points.txt", "colors.txt", "poses.txt", "rotations.txt")


def _cfg(required):
    d = slamhip.reference_example()
    d.update({"featureExtractingThreshold": 10, "requiredExtractedPointsCount": required, "framesBatchSize": 4,
              "requiredMatchedPointsCount": 300, "useFM-SIFT-FLANN": False, "useFM-SIFT-BF": True,
              "useFM-ORB": False, "useBundleAdjustment": False, "BAMaxFramesCnt": 4})
    return slamhip.ConfigService(d)


def _run(media, cfg, ops, out_dir, **kw):
    gd, logs = cycle.slam_main(media, K_VGA.copy(), cfg, ops, out_dir=str(out_dir), **kw)
    return logs, {f: open(os.path.join(out_dir, f), "rb").read() for f in FILES}


@pytest.fixture(scope="module")
def seq16():
    return slamhip.synth_frames(640, 480, 0, 16, seed=1234)


def test_pipeline_undistorts_at_the_seam(gpu_ctx, seq16, tmp_path):
    """slam_main(dist=DC) over MediaSources and over DeviceMedia writes the files
    of a run over the same frames undistorted beforehand by the reference.  The
    undistorted frames hold 1600-1850 FAST keypoints (the lens model shrinks
    the texture), hence requiredExtractedPointsCount 1000."""
    import torch
    _, D = calib()
    cfg = _cfg(1000)
    xy, frac = U.undistort_map(640, 480, K_VGA, D)
    pre = np.stack([U.remap(f, xy, frac) for f in seq16])
    ops = cycle.GpuOps(gpu_ctx)
    lg, want = _run(cycle.MediaSources(list(pre)), cfg, ops, tmp_path / "pre")
    assert len(lg.pose_list) >= 3
    _, got = _run(cycle.MediaSources(list(seq16)), cfg, ops, tmp_path / "media", dist=D)
    for name in FILES:
        assert got[name] == want[name], name
    dev = torch.from_numpy(np.ascontiguousarray(seq16)).cuda()
    torch.cuda.current_stream().synchronize()
    calls = []
    fb = ops.fast_batch
    ops.fast_batch = lambda fr, thr: calls.append(len(fr)) or fb(fr, thr)
    _, got = _run(cycle.DeviceMedia(seq16, dev), cfg, ops, tmp_path / "dev", dist=D)
    assert calls and max(calls) > 1                            # take(n) kept working: batched intake
    for name in FILES:
        assert got[name] == want[name], name


def test_pipeline_without_coefficients_is_unchanged(gpu_ctx, seq16, tmp_path):
    cfg = _cfg(2000)
    from oracle_ops import OracleOps
    ops = cycle.GpuOps(gpu_ctx)
    # today's output: the CPU oracle's run, which tests/test_cycle.py holds the GPU path to
    lg, today = _run(cycle.MediaSources(list(seq16)), cfg, OracleOps(), tmp_path / "today")
    assert len(lg.pose_list) >= 3
    _, none = _run(cycle.MediaSources(list(seq16)), cfg, ops, tmp_path / "none", dist=None)
    _, zeros = _run(cycle.MediaSources(list(seq16)), cfg, ops, tmp_path / "zeros", dist=np.zeros(5))
    for name in FILES:
        assert none[name] == today[name], name
        assert zeros[name] == today[name], name

"""GPU tests of the chessboard calibration stage (csrc/calib.hip behind
slam_chess_candidates*, slam_find_chessboard*, slam_corner_subpix*, and
slamhip.calibration): every device result equals tests/calib_ref.py bit for bit;
the solver's result is held to the cost margin of tests/test_calib.py.

Fixture: tests/golden/real_calib_boards.npz (tests/golden/make_calib_fixtures.py): ten
of the reference's chessboard photos, downscaled by 4 and cropped to one window.
"""
import functools
import json
import os

import numpy as np
import pytest

import calib_ref as C
import slamhip
from slamhip import _lib as L
from slamhip import calibration
from test_calib import COST_MARGIN_REL, ref_cost_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOARD = (7, 7)


@functools.lru_cache(maxsize=None)
def boards():
    g = np.load(os.path.join(GOLDEN, "real_calib_boards.npz"))["gray"]
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def ref_pipeline():
    """the reference pipeline on the ten boards: detected and refined corners"""
    found, first, refined = [], [], []
    for im in boards():
        ok, c = C.find_chessboard(im, BOARD)
        found.append(ok)
        first.append(c)
        refined.append(C.corner_subpix(im, c, (11, 11), (30, 1e-4)))
    return found, np.stack(first), np.stack(refined)


def checker(w, h, period, seed=None, amp=8, ch=1):
    y, x = np.mgrid[:h, :w]
    a = np.where(((x + 4) // period + (y + 4) // period) % 2 == 0, 200, 40)
    if ch == 3:
        a = np.stack([a, a // 2 + 60, 255 - a], 2)
    if seed is not None:
        a = a + np.random.default_rng(seed).integers(-amp, amp + 1, a.shape)
    return np.ascontiguousarray(a.astype(np.uint8))


def quadrant(w, h, cx, cy, seed):
    y, x = np.mgrid[:h, :w]
    a = np.where((x < cx) ^ (y < cy), 200, 40) + np.random.default_rng(seed).integers(-8, 9, (h, w))
    return a.astype(np.uint8)


def same_candidates(img, ctx, at_least=1):
    ref, s = C.candidates(img)
    got, gs = slamhip.chessCandidates(img, ctx=ctx)
    assert gs == s
    assert len(ref) >= at_least, "the input exercises nothing"
    assert got.shape == ref.shape and np.array_equal(got, ref)
    return ref


# ---- candidates -----------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(11, 11), (12, 17), (63, 65), (64, 64), (65, 63)])
def test_candidates_tile_edges(gpu_ctx, w, h):
    """one scored pixel; a level narrower than a tile; one pixel under, at and over the 64 x 16 tile"""
    img = quadrant(w, h, 5.5, 5.5, 1) if (w, h) == (11, 11) else checker(w, h, 9, seed=100 * w + h)
    same_candidates(img, gpu_ctx)


def test_candidates_small_frames_have_none(gpu_ctx):
    """narrower than the ring: every response is in the border"""
    for w, h in ((10, 40), (40, 10), (1, 1)):
        got, s = slamhip.chessCandidates(checker(w, h, 9, seed=3), ctx=gpu_ctx)
        assert s == 1 and got.shape == (0, 3)


def test_candidates_row_stride(gpu_ctx):
    wide = checker(150, 70, 9, seed=7)
    view = wide[:, 13:13 + 101]
    assert view.strides[0] > view.shape[1]
    same_candidates(view, gpu_ctx, at_least=20)


def test_candidates_bgr(gpu_ctx):
    """3-channel input: the gray FAST sees, then the same detector"""
    img = checker(131, 77, 9, seed=11, ch=3)
    ref = same_candidates(img, gpu_ctx, at_least=20)
    assert np.array_equal(ref, C.candidates(C.gray(img))[0])


@pytest.mark.parametrize("w,h,s,ch", [(1027, 770, 2, 1), (2050, 1537, 3, 1), (1027, 770, 2, 3)])
def test_candidates_downscaled_level(gpu_ctx, w, h, s, ch):
    """s = 2 and 3 with a dropped right / bottom remainder"""
    assert C.scale_of(w, h) == s and (w % s or h % s)
    img = np.repeat(np.repeat(checker(w // s + 1, h // s + 1, 11, seed=s, ch=ch), s, 0), s, 1)[:h, :w]
    img = img + np.random.default_rng(5).integers(0, 3, img.shape, dtype=np.uint8)      # rounding of the area mean at work
    same_candidates(np.ascontiguousarray(img), gpu_ctx, at_least=100)


def test_candidates_noise_compaction_order(gpu_ctx):
    """u8 noise: candidates in many tiles and rows; the list is in raster order"""
    img = np.random.default_rng(21).integers(0, 256, (150, 200), dtype=np.uint8)
    ref = same_candidates(img, gpu_ctx, at_least=100)
    key = ref[:, 1].astype(np.int64) * 200 + ref[:, 0]
    assert np.all(np.diff(key) > 0)
    d = np.abs(ref[:, None, :2] - ref[None, :, :2]).max(2)
    assert d[~np.eye(len(ref), dtype=bool)].min() > 7


@pytest.mark.parametrize("period,expect", [(4, 1), (6, 1), (12, None)])
def test_candidates_plateau_tie_rule(gpu_ctx, period, expect):
    """a noiseless checker: hundreds of equal maxima.  With several inside one
    window only the first in raster order is a candidate (each later one has an
    equal earlier cell); at period 12 the corners are in windows of their own and
    each gives one candidate: the first pixel of its small plateau."""
    img = checker(64, 48, period)
    R = C.response(img)
    assert (R == R.max()).sum() > 20 and R.max() > 0
    ref = same_candidates(img, gpu_ctx)
    if expect is not None:
        assert len(ref) == expect
    else:
        assert 10 < len(ref) < (R == R.max()).sum()


def test_candidates_batch_equals_single_calls(gpu_ctx):
    import torch
    g = boards()[:3]
    batch, s = slamhip.chessCandidates(torch.from_numpy(np.array(g)).cuda(), ctx=gpu_ctx)
    assert s == 1 and len(batch) == 3
    for f in range(3):
        one, _ = slamhip.chessCandidates(g[f], ctx=gpu_ctx)
        assert np.array_equal(batch[f], one)
        assert np.array_equal(one, C.candidates(g[f])[0])


def test_candidates_capacity_status(gpu_ctx):
    import ctypes
    img = np.array(boards()[0])
    h, w = img.shape
    out = np.zeros((4, 3), np.int32)
    n, s = ctypes.c_int(0), ctypes.c_int(0)
    rc = L.lib().slam_chess_candidates(gpu_ctx.handle, L.ptr(img), w, h, w, 1, L.ptr(out), 4, ctypes.byref(n), ctypes.byref(s))
    assert rc == L.SLAM_E_CAPACITY and n.value == len(C.candidates(img)[0])


def test_find_chessboard_on_the_fixture(gpu_ctx):
    import torch
    found, first, _ = ref_pipeline()
    assert all(found)
    got = slamhip.findChessboardCorners(torch.from_numpy(np.array(boards())).cuda(), BOARD, ctx=gpu_ctx)
    for f, (ok, c) in enumerate(got):
        assert ok and np.array_equal(c, first[f])
    ok, c = slamhip.findChessboardCorners(boards()[4], BOARD, ctx=gpu_ctx)
    assert ok and np.array_equal(c, first[4])
    assert slamhip.findChessboardCorners(np.full((80, 90), 127, np.uint8), BOARD, ctx=gpu_ctx) == (False, None)


# ---- cornerSubPix ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def corners490():
    """all ten boards' detected corners, refined on board 0 (they share one window)"""
    _, first, _ = ref_pipeline()
    pts = first.reshape(-1, 2)
    return pts, C.corner_subpix(boards()[0], pts, (11, 11), (30, 1e-4))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 490])
def test_subpix_counts(gpu_ctx, n):
    pts, ref = corners490()
    got = slamhip.cornerSubPix(boards()[0], pts[:n], (11, 11), (30, 1e-4), ctx=gpu_ctx)
    assert got.shape == (n, 2) and np.array_equal(got, ref[:n])
    if n:
        assert not np.array_equal(got, pts[:n])


@pytest.mark.parametrize("win", [(5, 5), (11, 11), (15, 3)])
@pytest.mark.parametrize("criteria", [(30, 1e-4), (1, 0.0), (100, 1e-9)])
def test_subpix_windows_and_criteria(gpu_ctx, win, criteria):
    _, first, _ = ref_pipeline()
    pts = first[1][::3]
    info = []
    ref = C.corner_subpix(boards()[1], pts, win, criteria, info=info)
    got = slamhip.cornerSubPix(boards()[1], pts, win, criteria, ctx=gpu_ctx)
    assert np.array_equal(got, ref)
    if criteria[0] == 1:
        assert all(it == 1 for _, it, _ in info)


def test_subpix_replicated_border(gpu_ctx):
    """corners within the window of every edge and corner of the image, gray and BGR"""
    img = np.array(boards()[2])
    h, w = img.shape
    pts = np.array([[0.0, 0.0], [3.3, 4.7], [w - 1.0, h - 1.0], [w - 2.5, 100.2], [200.5, h - 1.2], [0.4, h - 0.6],
                    [w - 0.25, 0.75], [11.9, 12.1], [w - 13.0, h - 13.0], [150.5, 5.5]], np.float32)
    for win in ((5, 5), (11, 11)):
        assert np.array_equal(slamhip.cornerSubPix(img, pts, win, ctx=gpu_ctx), C.corner_subpix(img, pts, win))
    bgr = checker(90, 70, 13, seed=4, ch=3)
    p3 = np.array([[2.0, 3.0], [40.2, 30.7], [88.5, 68.5], [48.0, 35.0]], np.float32)
    assert np.array_equal(slamhip.cornerSubPix(bgr, p3, (5, 5), ctx=gpu_ctx), C.corner_subpix(bgr, p3, (5, 5)))


def test_subpix_update_leaves_the_image(gpu_ctx):
    """a horizontal edge with little noise: the normal matrix is nearly singular
    along x and the update jumps out of the image: the break after the update"""
    y = np.mgrid[:40, :48][0]
    for seed, starts in ((2, [(1.0, 20.3), (0.5, 19.0), (2.0, 18.0)]), (3, [(46.5, 21.0), (0.5, 19.0)])):
        img = (np.where(y < 20, 200, 40) + np.random.default_rng(seed).integers(-2, 3, (40, 48))).astype(np.uint8)
        info = []
        ref = C.corner_subpix(img, starts, (5, 5), info=info)
        assert all(why == "outside" for why, _, _ in info)
        got = slamhip.cornerSubPix(img, starts, (5, 5), ctx=gpu_ctx)
        assert np.array_equal(got, ref)
        assert (ref[:, 0] < 0).any() or (ref[:, 0] >= 48).any() or any(r for _, _, r in info)


def test_subpix_flat_patch_and_revert(gpu_ctx):
    """a flat patch: det == 0, the corner stays; noise: updates beyond the window are reverted"""
    flat = np.full((60, 70), 128, np.uint8)
    info = []
    ref = C.corner_subpix(flat, [[30.5, 20.25]], info=info)
    assert info[0][0] == "det" and np.array_equal(ref, [[30.5, 20.25]])
    assert np.array_equal(slamhip.cornerSubPix(flat, [[30.5, 20.25]], ctx=gpu_ctx), ref)
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (80, 90), dtype=np.uint8)
    pts = np.stack([rng.uniform(0, 90, 96), rng.uniform(0, 80, 96)], 1).astype(np.float32)
    info = []
    ref = C.corner_subpix(noise, pts, (5, 5), info=info)
    reverted = np.array([r for _, _, r in info])
    assert 10 < reverted.sum() < 86
    assert np.array_equal(ref[reverted], pts[reverted])
    assert np.array_equal(slamhip.cornerSubPix(noise, pts, (5, 5), ctx=gpu_ctx), ref)


def test_subpix_argument_statuses(gpu_ctx):
    img = np.array(boards()[0])
    with pytest.raises(L.SlamError) as e:
        slamhip.cornerSubPix(img, [[10.0, 10.0]], zeroZone=(2, 2), ctx=gpu_ctx)
    assert e.value.code == L.SLAM_E_UNSUPPORTED
    with pytest.raises(L.SlamError) as e:
        slamhip.cornerSubPix(img, [[10.0, 10.0]], winSize=(16, 5), ctx=gpu_ctx)
    assert e.value.code == L.SLAM_E_UNSUPPORTED
    with pytest.raises(L.SlamError) as e:
        slamhip.cornerSubPix(img, [[-1.0, 10.0]], ctx=gpu_ctx)
    assert e.value.code == L.SLAM_E_INVALID_ARG


def test_subpix_resident_frame_equals_host_frame(gpu_ctx):
    import torch
    _, first, refined = ref_pipeline()
    dev = torch.from_numpy(np.array(boards()[3])).cuda()
    assert np.array_equal(slamhip.cornerSubPix(dev, first[3], ctx=gpu_ctx), refined[3])


# ---- end to end --------------------------------------------------------------------------

def test_end_to_end_on_the_ten_boards(gpu_ctx):
    """chessboard_photos_calibration over the fixture: all ten boards, the
    reference pipeline's corners bit for bit, and a calibration within the cost
    margin of the reference's solve of those corners.  The RMS it reaches (a
    property of the photos at a quarter of their resolution) is in DESIGN.md."""
    frames = [np.array(b) for b in boards()]
    rms, K, D, R, T, pts = calibration.chessboard_photos_calibration(frames, ctx=gpu_ctx, with_corners=True)
    _, _, refined = ref_pipeline()
    assert pts.shape == (10, 49, 2) and np.array_equal(pts, refined)
    obj = C.board_points(BOARD, 23.0)
    h, w = frames[0].shape
    cost = C.cost(obj, pts, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), D, R, T)
    ref = ref_cost_of(obj, pts, (h, w))
    print(f"end to end: rms {rms:.6f} px, cost {cost!r}, reference cost {ref!r}")
    assert cost <= ref * (1 + COST_MARGIN_REL)
    assert abs(rms - np.sqrt(cost / 490)) <= 1e-12 * rms
    assert R.shape == (10, 3) and T.shape == (10, 3) and np.all(T[:, 2] > 0)


def test_calibration_main_writes_the_file(gpu_ctx, tmp_path):
    for k, b in enumerate(boards()):
        np.save(tmp_path / f"board_{k:02d}.npy", b)
    (tmp_path / "board_05b.npy").write_bytes(b"")           # an unreadable photo: imread's empty frame
    cfg = slamhip.reference_example()
    out = tmp_path / "calibration.xml"
    cfg.update({"calibrate": True, "usePhotosCycle": True, "photosPathPattern": str(tmp_path / "board_*.npy"),
                "calibrationPath": str(out), "visualCalibration": False})
    path = tmp_path / "config.json"
    path.write_text(json.dumps(cfg))
    rms, K, D, R, T = calibration.main(str(path), ctx=gpu_ctx)
    assert np.array_equal(slamhip.load_calibration(str(out)), K)
    assert np.array_equal(slamhip.load_calibration(str(out), "DC").ravel(), D)
    assert np.array_equal(slamhip.load_calibration(str(out), "R"), R)
    assert np.array_equal(slamhip.load_calibration(str(out), "T"), T)
    assert len(R) == 10 and rms > 0
    cfg["usePhotosCycle"] = False
    path.write_text(json.dumps(cfg))
    with pytest.raises(NotImplementedError):
        calibration.main(str(path), ctx=gpu_ctx)

"""CPU tests of the chessboard calibration stage: tests/calib_ref.py on the
fixture, the host-only parts of the library (slam_label_chessboard,
slam_calibrate_camera, save_calibration) against it, and the 10-board rule of
slamhip.calibration.  The device parts are in tests/test_calib_gpu.py.

Fixtures: tests/golden/real_calib_boards.npz (tests/golden/make_calib_fixtures.py) and
tests/golden/calib_samsung_hv.xml (the reference's config/samsung-hv.xml: K, DC
and 13 recorded board poses R, T; settings only).
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import calib_ref as C
import slamhip
from slamhip import _lib as L
from slamhip import calibration

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CALIB = os.path.join(GOLDEN, "calib_samsung_hv.xml")
BOARD = (7, 7)

# The library's final cost may exceed the reference's by this fraction of it.
# Measured: calib_ref.calibrate on the 13 recorded views with xtol = ftol = gtol in
# {1e-15, 1e-12, 1e-10} and x_scale in {"jac", 1.0} ends at costs between
# 4.0616524340e-07 and 4.0616524450e-07, a spread of 1.10e-15 = 2.7e-9 of the cost
# (on the first 10 views 1.3e-17 = 4.2e-11 of 3.2176e-07); times 10.
COST_MARGIN_REL = 2.7e-8


@functools.lru_cache(maxsize=None)
def boards():
    z = np.load(os.path.join(GOLDEN, "real_calib_boards.npz"))
    g = z["gray"]
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def detections():
    """(candidates, s) of calib_ref on each fixture image"""
    return [C.candidates(im) for im in boards()]


@functools.lru_cache(maxsize=None)
def recorded():
    K = slamhip.load_calibration(CALIB)
    D = slamhip.load_calibration(CALIB, "DC").ravel()
    R = slamhip.load_calibration(CALIB, "R")
    T = slamhip.load_calibration(CALIB, "T")
    obj = C.board_points(BOARD, 23.0)
    img = np.stack([C.project(obj, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), D, R[v], T[v]) for v in range(len(R))])
    return K, D, R, T, obj, img.astype(np.float32)


_solved = {}


def ref_solve(obj, img, size):
    """calib_ref's scipy solve, once per input"""
    key = (obj.tobytes(), img.tobytes(), tuple(size))
    if key not in _solved:
        _solved[key] = C.calibrate(obj, img, size)
    return _solved[key]


def ref_cost_of(obj, img, size):
    return ref_solve(obj, np.asarray(img, np.float32), size)[5]


# ---- 1. calib_ref on the fixture -----------------------------------------------------------

def test_ref_detects_every_fixture_board():
    assert boards().shape[0] == 10
    for (cand, s), im in zip(detections(), boards()):
        assert s == 1 and len(cand) > 50
        v = cand[C.strongest(cand, 50), 2]
        assert v[49] < v[48]                       # measured: at most 0.2 of it on these windows
        sel = cand[C.strongest(cand, 49)]
        grid = C.label_board(sel[:, :2], 7, 7)
        assert grid is not None and sorted(grid.ravel().tolist()) == list(range(49))
        P = sel[grid.ravel(), :2].reshape(7, 7, 2).astype(np.int64)
        # right-handed in every cell, y down
        ex, ey = P[:-1, 1:] - P[:-1, :-1], P[1:, :-1] - P[:-1, :-1]
        assert np.all(ex[..., 0] * ey[..., 1] - ex[..., 1] * ey[..., 0] > 0)
        # canonical: no other corner of the board is nearer the origin in x + y
        key = lambda p: (int(p[0] + p[1]), int(p[1]))
        assert key(P[0, 0]) == min(key(P[i, j]) for i in (0, 6) for j in (0, 6))
        # a lattice: neighbours 20 .. 40 level pixels apart
        d = np.linalg.norm(ex, axis=2)
        assert 15 < d.min() and d.max() < 45


def test_library_labelling_equals_the_reference():
    for (cand, s), im in zip(detections(), boards()):
        ok, ref = C.find_chessboard(im, BOARD)
        found, got = slamhip.labelChessboard(cand, s, BOARD)
        assert ok and found and got.dtype == np.float32 and np.array_equal(got, ref)
    # scaled coordinates: s * x + (s - 1) / 2
    cand, _ = detections()[0]
    _, c1 = slamhip.labelChessboard(cand, 1, BOARD)
    _, c4 = slamhip.labelChessboard(cand, 4, BOARD)
    assert np.array_equal(c4, 4 * c1 + np.float32(1.5))


@pytest.mark.parametrize("bw,bh", [(7, 7), (9, 6), (4, 5)])
@pytest.mark.parametrize("turn", [0, 90, 180, 270, "mirror"])
def test_labelling_of_synthetic_boards_is_canonical(bw, bh, turn):
    """a projected lattice in every orientation, points shuffled: both labellings
    agree, and give the same canonical order whatever the input order was"""
    rng = np.random.default_rng(bw * 100 + bh)
    j, i = np.meshgrid(np.arange(bw), np.arange(bh))
    p = np.stack([j.ravel() * 30.0, i.ravel() * 30.0], 1) - [15.0 * (bw - 1), 15.0 * (bh - 1)]
    if turn == "mirror":
        p = p * [-1, 1]
    else:
        a = np.deg2rad(turn + 7.0)
        p = p @ np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]).T
    w = 1 + p @ [4e-4, -3e-4]                      # mild perspective
    p = np.rint(p / w[:, None] + 400).astype(np.int32)
    order = rng.permutation(len(p))
    cand = np.concatenate([p[order], rng.integers(1000, 2000, (len(p), 1)).astype(np.int32)], 1)
    clutter = np.array([[5, 5, 10], [790, 6, 20]], np.int32)           # weaker than every corner
    found, got = slamhip.labelChessboard(np.concatenate([cand, clutter]), 1, (bw, bh))
    grid = C.label_board(cand[:, :2], bw, bh)
    assert found and grid is not None
    ref = cand[grid.ravel(), :2].astype(np.float32)
    assert np.array_equal(got, ref)
    G = ref.reshape(bh, bw, 2)
    ex, ey = G[0, 1] - G[0, 0], G[1, 0] - G[0, 0]
    assert ex[0] * ey[1] - ex[1] * ey[0] > 0
    assert sorted(map(tuple, ref.tolist())) == sorted(map(tuple, p.astype(np.float32).tolist()))


def test_labelling_rejects_what_is_no_board():
    cand, s = detections()[0]
    sel = cand[C.strongest(cand, 49)].copy()
    assert slamhip.labelChessboard(sel[:48], s, BOARD) == (False, None)          # too few
    moved = sel.copy()
    moved[10, :2] += 15                                                         # one corner between the nodes
    assert slamhip.labelChessboard(moved, s, BOARD)[0] is False
    assert C.label_board(moved[:, :2], 7, 7) is None
    line = np.stack([np.arange(49) * 9, np.full(49, 50), np.full(49, 100)], 1).astype(np.int32)
    assert slamhip.labelChessboard(line, 1, BOARD)[0] is False
    assert C.label_board(line[:, :2], 7, 7) is None


# ---- 2. pixel replication ---------------------------------------------------------------------

@pytest.mark.parametrize("rep", [2, 3])
def test_replicated_pixels_give_the_same_candidates(rep):
    """the area mean of a replicated block is the pixel itself: s = rep, same list"""
    im = boards()[0][:, :342]
    im = np.ascontiguousarray(np.concatenate([im, im[:277]], 0))       # 342 x 700: s = rep for rep 2 and 3
    big = np.repeat(np.repeat(im, rep, 0), rep, 1)
    assert C.scale_of(big.shape[1], big.shape[0]) == rep
    ref, s1 = C.candidates(im)
    got, s = C.candidates(big)
    assert s1 == 1 and s == rep and len(ref) > 50 and np.array_equal(got, ref)


# ---- 3. slam_calibrate_camera on the recorded poses -----------------------------------------------

@pytest.mark.parametrize("nviews", [13, 10])
def test_calibrate_recovers_the_recorded_camera(nviews):
    K, D, R, T, obj, img = recorded()
    img = np.ascontiguousarray(img[:nviews])
    assert img.min() >= 0 and img[..., 0].max() < 1920 and img[..., 1].max() < 1080
    rms, K2, D2, rv, tv = slamhip.calibrateCamera(obj, img, (1920, 1080))
    ref_rms, Kr, Dr, rvr, tvr, ref_cost = ref_solve(obj, img, (1920, 1080))
    cost = C.cost(obj, img, (K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2]), D2, rv, tv)
    print(f"{nviews} views: library cost {cost!r} rms {rms!r}; reference cost {ref_cost!r} rms {ref_rms!r}")
    assert cost <= ref_cost * (1 + COST_MARGIN_REL)
    assert abs(rms - np.sqrt(cost / (nviews * 49))) <= 1e-9 * rms
    four = lambda M: np.array([M[0, 0], M[1, 1], M[0, 2], M[1, 2]])
    ref_dist = np.abs(four(Kr) - four(K)).max()
    print(f"  |K - file| library {np.abs(four(K2) - four(K)).max():.3e}, reference {ref_dist:.3e}")
    assert ref_dist <= 4.5e-4                       # the reference's own distance, as measured for the issue
    assert np.abs(four(K2) - four(K)).max() <= 2 * ref_dist
    assert np.abs(rv - R[:nviews]).max() <= 2 * max(np.abs(rvr - R[:nviews]).max(), 6e-7)
    assert K2[0, 1] == 0 and K2[1, 0] == 0 and K2[2].tolist() == [0, 0, 1]


def test_calibrate_is_deterministic_and_ignores_the_size_quirk():
    """Size(rows, cols) instead of (cols, rows) moves the initial principal point only"""
    K, D, R, T, obj, img = recorded()
    a = slamhip.calibrateCamera(obj, img[:10], (1920, 1080))
    b = slamhip.calibrateCamera(obj, img[:10], (1920, 1080))
    assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])) and a[0] == b[0]
    c = slamhip.calibrateCamera(obj, img[:10], (1080, 1920))
    cost = lambda r: C.cost(obj, img[:10], (r[1][0, 0], r[1][1, 1], r[1][0, 2], r[1][1, 2]), r[2], r[3], r[4])
    assert cost(c) <= cost(a) * (1 + COST_MARGIN_REL)


# ---- 4. error paths ------------------------------------------------------------------------------

def _raw_calibrate(obj, img, nviews, npts):
    obj = np.ascontiguousarray(obj, np.float32)
    img = np.ascontiguousarray(img, np.float32)
    K, D, rv, tv = np.zeros(9), np.zeros(5), np.zeros((nviews, 3)), np.zeros((nviews, 3))
    rms, it = ctypes.c_double(0), ctypes.c_int(0)
    return L.lib().slam_calibrate_camera(L.ptr(obj), L.ptr(img), nviews, npts, 1920, 1080, L.ptr(K), L.ptr(D), L.ptr(rv),
                                         L.ptr(tv), ctypes.byref(rms), ctypes.byref(it))


def test_calibrate_error_statuses():
    K, D, R, T, obj, img = recorded()
    assert _raw_calibrate(obj, img[:2], 2, 49) == L.SLAM_E_INVALID_ARG              # two views
    bent = obj.copy()
    bent[7, 2] = 1.0
    assert _raw_calibrate(bent, img[:5], 5, 49) == L.SLAM_E_INVALID_ARG             # not planar
    same = np.full((5, 49, 2), 300.0, np.float32)
    assert _raw_calibrate(obj, same, 5, 49) == L.SLAM_E_SOLVER                      # all points identical
    line = np.stack([np.linspace(100, 900, 49), np.linspace(50, 700, 49)], 1).astype(np.float32)
    assert _raw_calibrate(obj, np.stack([line] * 4), 4, 49) == L.SLAM_E_SOLVER      # collinear: no homography
    nan = img[:4].copy()
    nan[1, 3, 0] = np.nan
    assert _raw_calibrate(obj, nan, 4, 49) == L.SLAM_E_INVALID_ARG
    with pytest.raises(L.SlamError):
        slamhip.calibrateCamera(obj, img[:2], (1920, 1080))


# ---- 5. the calibration file ------------------------------------------------------------------------

@pytest.mark.parametrize("nviews", [1, 10, 13])
def test_save_calibration_round_trip(tmp_path, nviews):
    K, D, R, T, _, _ = recorded()
    rng = np.random.default_rng(nviews)
    K = K + np.array([[rng.random(), 0, rng.random()], [0, rng.random(), rng.random()], [0, 0, 0]]) * 1e-3
    D = D * (1 + rng.random(5) * 1e-9)
    R, T = R[:nviews] + 1e-17, T[:nviews] * (1 + 1e-16)
    R[0, 0] = 5e-324                                  # a denormal and a large value survive too
    T[0, 1] = -1.7976931348623157e308
    path = str(tmp_path / "calib.xml")
    slamhip.save_calibration(path, K, D, R, T)
    for key, want in (("K", K), ("DC", D.reshape(1, 5)), ("R", R), ("T", T)):
        got = slamhip.load_calibration(path, key)
        assert got.shape == want.shape and got.tobytes() == want.tobytes()
    text = open(path).read()
    assert text.count('<dt>"3d"</dt>') == 2 and "<opencv_storage>" in text and f"<rows>{nviews}</rows>" in text


# ---- 6. the 10-board rule -----------------------------------------------------------------------------

class RefOps:
    """calib_ref's detector in the place of the device's"""

    def __init__(self):
        self.seen = 0

    def detect(self, frames, board_size):
        out = []
        for f in frames:
            self.seen += 1
            ok, c = C.find_chessboard(f, board_size)
            out.append((ok, C.corner_subpix(f, c) if ok else None))
        return out


def test_nine_boards_are_not_enough():
    frames = [np.array(b) for b in boards()[:9]] + [np.zeros((423, 366), np.uint8)]
    with pytest.raises(calibration.CalibrationError, match="Cannot detect chessboard on enough count of photos"):
        calibration.chessboard_photos_calibration(frames, ops=RefOps())


def test_blank_and_empty_frames_are_skipped(tmp_path):
    g = [np.array(b) for b in boards()]
    np.save(tmp_path / "b9.npy", g[9])
    frames = g[:4] + [np.full((423, 366), 200, np.uint8), None, str(tmp_path / "missing.npy")] + g[4:9] + \
        [str(tmp_path / "b9.npy"), g[0]]
    ops = RefOps()
    rms, K, D, R, T, pts = calibration.chessboard_photos_calibration(frames, ops=ops, with_corners=True)
    assert pts.shape == (10, 49, 2) and R.shape == (10, 3)
    assert ops.seen == 11                              # the blank one and ten boards; the twelfth is never examined
    want = np.stack([C.corner_subpix(f, C.find_chessboard(f, BOARD)[1]) for f in g])
    assert np.array_equal(pts, want)
    assert np.isfinite(rms) and K[0, 0] > 0 and K[1, 1] > 0

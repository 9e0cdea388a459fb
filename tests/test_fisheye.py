"""CPU tests of the fisheye lens model: the definition's
own checks (tests/fisheye_ref.py), the two measurements its header quotes, the
calibration file's model node and the exports.  The device side is
tests/test_fisheye_gpu.py.
"""
import functools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import fisheye_ref as F
import slamhip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

STRONG_D = np.array([-0.3, 0.1, 0.0, 0.0])
# theta (1 - 0.3 theta^2) peaks at theta_d = 0.703: beyond it a pixel has no preimage and Newton cannot converge
FOLD_D = np.array([-0.3, 0.0, 0.0, 0.0])


def integer_camera(w, h):
    """the prototype's focal lengths on an integer principal point: r == 0 is hit"""
    return np.array([[208.08 * w / 748, 0, w // 2], [0, 208.11 * h / 480, h // 2], [0, 0, 1.0]])


def half(K):
    n = np.array(K, np.float64)
    n[0, 0] *= 0.5
    n[1, 1] *= 0.5
    return n


def ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def neighbours(v, n=4):
    out, a, b = [v], v, v
    for _ in range(n):
        a, b = np.nextafter(a, np.inf), np.nextafter(b, -np.inf)
        out += [a, b]
    return [x for x in out if 0 <= x <= math.pi / 2]


# ---------------- fe_atan / fe_tan ----------------

def test_hand_worked_values():
    # atan: 0 and 1 leave the polynomial at 0 (t = 0), so the result is the table's high + low word
    assert F.fe_atan(0.0) == 0.0
    assert F.fe_atan(1.0) == F.AT_HI[1] + F.AT_LO[1] == math.pi / 4
    assert ulps(F.fe_atan(math.pi / 4), 0.6657737500283538) <= 1          # atan(pi/4), from tables
    assert F.fe_atan(np.inf) == math.pi / 2
    assert np.isnan(F.fe_atan(np.nan))
    # tan: the double nearest pi/4 is 3.06e-17 below it: (1 - u) / (1 + u) rounds to 1 exactly
    assert F.fe_tan(0.0) == 0.0
    assert F.fe_tan(math.pi / 4) == 1.0
    assert ulps(F.fe_tan(1.0), 1.5574077246549023) <= 2                  # tan(1), from tables
    # the double nearest pi/2 is 6.12e-17 below it: tan is the inverse of that gap
    assert F.fe_tan(math.pi / 2) == 1.0 / F.PIO2_LO
    assert np.isnan(F.fe_tan(np.nan))


def test_ulp_deviation_from_libm():
    """the measurement fisheye_ref's header and DESIGN section 19 quote"""
    x = np.concatenate([np.linspace(0, math.pi / 2, 2_000_001), neighbours(0.0), neighbours(math.pi / 4),
                        neighbours(math.pi / 2)])
    ua = ulps(F.fe_atan(x), np.array([math.atan(v) for v in x]))
    ut = ulps(F.fe_tan(x), np.array([math.tan(v) for v in x]))
    print("fe_atan: max %.1f ulp from math.atan; fe_tan: max %.1f ulp from math.tan" % (ua.max(), ut.max()))
    assert ua.max() <= 1 and ut.max() <= 2
    # the map's arguments r = tan(theta) reach far beyond pi/2
    r = np.concatenate([np.linspace(0, 50, 500_001), [1e3, 1e10, 1e300]])
    assert ulps(F.fe_atan(r), np.array([math.atan(v) for v in r])).max() <= 1


# ---------------- the forward model, the map, the points ----------------

def test_zero_coefficients_at_the_principal_point():
    K = integer_camera(64, 48)
    u, v = F.distort(0.0, 0.0, K, np.zeros(4))
    assert (u, v) == (32.0, 24.0)
    xy, frac = F.fisheye_map(64, 48, K, np.zeros(4))
    assert tuple(xy[24, 32]) == (32, 24) and frac[24, 32] == 0
    p, err = F.undistort_points(np.array([[32, 24]], np.float32), K, np.zeros(4), K)
    assert p.tolist() == [[32.0, 24.0]] and err.tolist() == [0.0]


@pytest.mark.parametrize("D", [F.CAMERA_D, np.zeros(4)], ids=["prototype", "zero"])
def test_forward_then_inverse_is_the_identity(D):
    """on a polar grid out to theta = 1.4: distort a normalised point, round the
    pixel to float32 as the entry point takes it, undistort, distort again"""
    K = F.CAMERA_K
    theta = np.linspace(0, 1.4, 57)[:, None]
    phi = np.linspace(0, 2 * math.pi, 24, endpoint=False)[None, :]
    a, b = (np.tan(theta) * np.cos(phi)).ravel(), (np.tan(theta) * np.sin(phi)).ravel()
    u, v = F.distort(a, b, K, D)
    src = np.stack([u, v], 1).astype(np.float32)
    xy, err, ex, _ = F.undistort_points(src, K, D, None, (10, 1e-8), details=True)
    assert np.isin(ex, (F.EXIT_EPS, F.EXIT_CENTRE)).all()
    u2, v2 = F.distort(xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64), K, D)
    # xy is float32: its rounding moves the pixel by up to 2^-24 * r * fx * d(theta)/dr; measure on f64 instead
    assert err.max() <= 1e-9
    inner = np.hypot(a, b) < 1.0
    assert np.abs(u2 - src[:, 0])[inner].max() < 1e-4 and np.abs(v2 - src[:, 1])[inner].max() < 1e-4


def cameras():
    out = []
    for w, h in ((64, 48), (161, 97), (748, 480)):
        out.append((w, h, F.CAMERA_K * np.array([[w / 748], [h / 480], [1]]), F.CAMERA_D, None))
        K = integer_camera(w, h)
        out.append((w, h, K, STRONG_D, half(K)))
    return out


def test_maps_differ_from_libm_maps_by_one_step_at_most():
    """fe_atan against np.arctan through the whole map: a few ulp of theta move u
    by 1e-13 px, so only a rounding knife-edge may flip, by one 1/32-px step"""
    total = 0
    for w, h, K, D, newK in cameras():
        iu, iv = F.fixed_point(w, h, K, D, newK)
        ju, jv = F.fixed_point(w, h, K, D, newK, atan=np.arctan)
        du, dv = np.abs(iu - ju), np.abs(iv - jv)
        assert du.max() <= 1 and dv.max() <= 1 and not ((du > 0) & (dv > 0)).any()
        n = int((du > 0).sum() + (dv > 0).sum())
        print("%d x %d%s: %d of %d entries differ" % (w, h, " strong" if newK is not None else "", n, 2 * w * h))
        total += n
    assert total <= 8          # knife-edges are rare: none on these six maps when measured


def test_map_refuses_a_projective_new_camera_matrix():
    K = integer_camera(64, 48)
    bad = K.copy()
    bad[2] = [1e-4, 0, 1]
    with pytest.raises(ValueError):
        F.fisheye_map(64, 48, K, F.CAMERA_D, bad)
    with pytest.raises(ValueError):
        F.fisheye_map(64, 48, K, np.zeros(5))


def test_points_exits():
    """the centre, |pw| beyond pi/2, a rejected point, eps = 0"""
    K = integer_camera(748, 480)
    p = np.array([[374, 240], [374.5, 240], [5000, 5000], [700, 400], [10, 470], [np.nan, 3]], np.float32)
    xy, err, ex, it = F.undistort_points(p, K, FOLD_D, K, (10, 1e-8), details=True)
    assert ex[0] == F.EXIT_CENTRE and xy[0].tolist() == [374.0, 240.0] and err[0] == 0
    assert ex[1] == F.EXIT_EPS and err[1] < 1e-9
    # |pw| is clamped to pi/2, far beyond the fold of FOLD_D
    assert ex[2] in (F.EXIT_NOT_CONVERGED, F.EXIT_FLIPPED)
    assert xy[2].tolist() == [F.REJECTED, F.REJECTED] and np.isnan(err[2])
    # eps = 0 is COUNT alone: never rejected for not converging
    xy0, err0, ex0, it0 = F.undistort_points(p, K, FOLD_D, K, (10, 0.0), details=True)
    assert (it0[1:5] == 10).all() and not (ex0 == F.EXIT_NOT_CONVERGED).any()
    assert np.isnan(xy[5]).all() and ex[5] == F.EXIT_CENTRE      # a NaN clamps to -pi/2 and is passed through


# ---------------- the solver ----------------

# The library's final cost may exceed the reference's by this fraction of it.
# Measured as tests/test_calib.py measures its margin: fisheye_ref.fisheye_calibrate
# on the 13 synthetic views below with xtol = ftol = gtol in {1e-15, 1e-12, 1e-10}
# ends at costs 7.458943912304e-08, 7.458943912645e-08 and 7.458943914918e-08, a
# spread of 2.6e-17 = 3.5e-10 of the cost; times 10.  (The library ended at
# 7.458943911537e-08, 1.0e-10 below the reference's best.)
COST_MARGIN_REL = 3.5e-9


def synthetic_views(nviews=13, seed=3):
    """13 poses of a 6 x 8 board pushed through the definition's forward model
    with the prototype's camera, rounded to float32 as corners are"""
    import calib_ref as C
    rng = np.random.default_rng(seed)
    obj = C.board_points((6, 8), 1.0)
    K4 = (F.CAMERA_K[0, 0], F.CAMERA_K[1, 1], F.CAMERA_K[0, 2], F.CAMERA_K[1, 2])
    rv, tv, img = [], [], []
    for _ in range(nviews):
        r = rng.uniform(-0.5, 0.5, 3) * [1, 1, 0.4]
        t = np.array([rng.uniform(-6, 1), rng.uniform(-6, 0), rng.uniform(5, 11)])
        rv.append(r)
        tv.append(t)
        img.append(F.project(obj, K4, F.CAMERA_D, r, t))
    return obj, np.array(img).astype(np.float32), np.array(rv), np.array(tv)


def test_calibrate_recovers_the_synthetic_camera():
    obj, img, rv0, tv0 = synthetic_views()
    assert img[..., 0].min() >= 0 and img[..., 0].max() < 748 and img[..., 1].min() >= 0 and img[..., 1].max() < 480
    rms, K, D, rv, tv = slamhip.fisheyeCalibrate(obj, img, (748, 480))
    ref_rms, Kr, Dr, rvr, tvr, ref_cost = F.fisheye_calibrate(obj, img, (748, 480))
    cost = F.cost(obj, img, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), D, rv, tv)
    print(f"library cost {cost!r} rms {rms!r}; reference cost {ref_cost!r} rms {ref_rms!r}")
    assert cost <= ref_cost * (1 + COST_MARGIN_REL)
    assert abs(rms - np.sqrt(cost / (13 * 48))) <= 1e-9 * rms
    # float32 corners: the camera comes back to 1e-4 px and 1e-5 in the coefficients, for both solvers alike
    four = lambda M: np.array([M[0, 0], M[1, 1], M[0, 2], M[1, 2]])
    assert np.abs(four(K) - four(F.CAMERA_K)).max() <= 1e-4 and np.abs(D - F.CAMERA_D).max() <= 1e-5
    assert np.abs(four(K) - four(Kr)).max() <= 1e-6 and np.abs(D - Dr).max() <= 1e-6
    assert np.abs(rv - rv0).max() <= 1e-5 and np.abs(tv - tv0).max() <= 1e-4
    assert K[0, 1] == 0 and K[1, 0] == 0 and K[2].tolist() == [0, 0, 1]
    again = slamhip.fisheyeCalibrate(obj, img, (748, 480))
    assert again[0] == rms and all(np.array_equal(x, y) for x, y in zip(again[1:], (K, D, rv, tv)))


def test_calibrate_status_codes():
    from slamhip import _lib as L
    obj, img, _, _ = synthetic_views(4)
    obj = np.ascontiguousarray(obj, np.float32)

    def raw(obj=obj, img=img, nviews=4, npts=48, size=(748, 480), K=True):
        Km, D, rv, tv = np.zeros(9), np.zeros(4), np.zeros((4, 3)), np.zeros((4, 3))
        import ctypes
        rms, it = ctypes.c_double(0), ctypes.c_int(0)
        return L.lib().slam_fisheye_calibrate(L.ptr(obj), L.ptr(img), nviews, npts, size[0], size[1],
                                              L.ptr(Km) if K else None, L.ptr(D), L.ptr(rv), L.ptr(tv),
                                              ctypes.byref(rms), ctypes.byref(it))

    assert raw() == L.SLAM_OK
    assert raw(nviews=2) == L.SLAM_E_INVALID_ARG
    assert raw(npts=3) == L.SLAM_E_INVALID_ARG
    assert raw(size=(0, 480)) == L.SLAM_E_INVALID_ARG
    assert raw(obj=None) == L.SLAM_E_INVALID_ARG and raw(img=None) == L.SLAM_E_INVALID_ARG and raw(K=False) == L.SLAM_E_INVALID_ARG
    lifted = obj.copy()
    lifted[5, 2] = 0.5
    assert raw(obj=lifted) == L.SLAM_E_INVALID_ARG            # a planar target with z = 0
    bad = img.copy()
    bad[1, 7, 0] = np.nan
    assert raw(img=bad) == L.SLAM_E_INVALID_ARG
    point = img.copy()
    point[2] = 100.0                                           # a view whose corners coincide: no homography
    assert raw(img=point) == L.SLAM_E_SOLVER


# ---------------- the labeller and the real set ----------------

PHOTOS = [os.path.join(GOLDEN, "fisheye", "Fisheye2_%d.jpg" % i) for i in range(1, 16)]
BOARD = (6, 8)


@functools.lru_cache(maxsize=None)
def photos():
    """(frame, candidates, scale, the definition's grid or None) per committed photo"""
    import calib_ref as C
    import jpeg_ref
    out = []
    for path in PHOTOS:
        img = jpeg_ref.decode(open(path, "rb").read())
        cand, s = C.candidates(img)
        out.append((img, cand, s, F.label_board_grow(cand, *BOARD)))
    return out


@functools.lru_cache(maxsize=None)
def real_corners():
    """the definition's corners of every labelled photo, refined in a (5, 5) window: (names, nviews x 48 x 2 f32)"""
    import calib_ref as C
    names, views = [], []
    for path, (img, cand, s, g) in zip(PHOTOS, photos()):
        if g is not None:
            xy = np.float32(s) * cand[g.ravel(), :2].astype(np.float32) + np.float32((s - 1) / 2)
            views.append(C.corner_subpix(img, xy, (5, 5), (30, 1e-4)))
            names.append(os.path.basename(path))
    return names, np.array(views, np.float32)


def test_labeller_on_the_photos():
    import calib_ref as C
    found = [g is not None for _, _, _, g in photos()]
    print("labelled:", [i + 1 for i, f in enumerate(found) if f])
    assert sum(found) >= 10                                  # MINIMAL_FOUND_FRAMES_COUNT; measured: 12 of 15
    peeled = 0
    for (img, cand, s, g), path in zip(photos(), PHOTOS):
        ok, corners = C.find_chessboard(img, BOARD)
        if ok:                                               # what the line-peeling labeller finds, the grower finds alike
            peeled += 1
            assert g is not None, path
            assert np.array_equal(corners, F.find_chessboard(img, BOARD)[1]), path
    assert peeled == 5


def test_labeller_agrees_on_straight_boards():
    import calib_ref as C
    z = np.load(os.path.join(GOLDEN, "real_calib_boards.npz"))
    for im in z["gray"]:
        cand, s = C.candidates(im)
        sel = cand[C.strongest(cand, 49)]
        g0 = C.label_board(sel[:, :2], 7, 7)
        assert g0 is not None
        g = F.label_board_grow(cand, 7, 7)
        assert g is not None and np.array_equal(cand[g.ravel(), :2], sel[g0.ravel(), :2])
        ok, c = slamhip.labelChessboard(cand, s, (7, 7), labeller="grow")
        assert ok and np.array_equal(c, cand[g.ravel(), :2].astype(np.float32))


def test_host_labeller_equals_the_definition():
    from slamhip import _lib as L
    for (img, cand, s, g), path in zip(photos(), PHOTOS):
        for board in (BOARD, (8, 6), (5, 5), (4, 3)):
            want = g if board == BOARD else F.label_board_grow(cand, *board)
            ok, c = slamhip.labelChessboard(cand, s, board, labeller="grow")
            assert ok == (want is not None), (path, board)
            if ok:
                assert np.array_equal(c, cand[want.ravel(), :2].astype(np.float32)), (path, board)
    # status codes, and inputs that are no board
    import ctypes
    cand = np.ascontiguousarray(photos()[0][1], np.int32)
    out, found = np.zeros((48, 2), np.float32), ctypes.c_int(7)
    call = lambda c, n, s, bw, bh, o=out: L.lib().slam_label_chessboard_grow(L.ptr(c), n, s, bw, bh, L.ptr(o), ctypes.byref(found))
    assert call(cand, len(cand), 1, 6, 8) == L.SLAM_OK and found.value == 1
    assert call(cand, 47, 1, 6, 8) == L.SLAM_OK and found.value == 0           # fewer candidates than corners
    assert call(cand, 0, 1, 6, 8) == L.SLAM_OK and found.value == 0
    assert call(None, 5, 1, 6, 8) == L.SLAM_E_INVALID_ARG
    assert call(cand, -1, 1, 6, 8) == L.SLAM_E_INVALID_ARG
    assert call(cand, len(cand), 0, 6, 8) == L.SLAM_E_INVALID_ARG
    assert call(cand, len(cand), 1, 1, 8) == L.SLAM_E_INVALID_ARG
    assert call(cand, len(cand), 1, 17, 16) == L.SLAM_E_INVALID_ARG           # more than 256 corners
    far = cand.copy()
    far[3, 0] = 8193                                                          # coordinates within +-8192
    assert call(far, len(far), 1, 6, 8) == L.SLAM_E_INVALID_ARG
    far[3, 0] = -8193
    assert call(far, len(far), 1, 6, 8) == L.SLAM_E_INVALID_ARG
    twice = np.concatenate([cand[:60], cand[:60]])
    assert call(twice, len(twice), 1, 6, 8) == L.SLAM_OK and found.value == 0  # coincident candidates
    assert slamhip.labelChessboard(np.zeros((0, 3), np.int32), 1, BOARD, labeller="grow") == (False, None)
    with pytest.raises(ValueError):
        slamhip.labelChessboard(cand, 1, BOARD, labeller="spiral")


def test_host_labeller_at_the_coordinate_bound():
    """boards that span the whole admitted range, +-8192: differences reach 2^14 and
    the labeller's largest product, 4 (u.w)^2, 2^58; the definition computes in
    Python's unbounded integers, the library in 64 bits, and they agree"""
    rng = np.random.default_rng(11)
    for bw, bh in ((2, 2), (3, 2), (6, 8)):
        for skew in (0, 37):
            gx, gy = np.meshgrid(np.arange(bw), np.arange(bh))
            step = 16384 // (max(bw, bh) - 1)              # square cells; the longer side spans the whole range
            x = -8192 + step * gx - skew * gy * (gx > 0) * (gx < bw - 1)
            y = 8192 - step * (bh - 1 - gy) + skew * gx * (gy > 0) * (gy < bh - 1)
            n = bw * bh
            cand = np.stack([x.ravel(), y.ravel(), rng.integers(1000, 2 ** 31 - 1, n)], 1).astype(np.int32)
            clutter = np.stack([rng.integers(-8192, 8193, n), rng.integers(-8192, 8193, n), rng.integers(1, 900, n)], 1)
            for c in (cand, np.concatenate([cand, clutter.astype(np.int32)])[rng.permutation(2 * n)]):
                want = F.label_board_grow(c, bw, bh)
                ok, got = slamhip.labelChessboard(c, 1, (bw, bh), labeller="grow")
                assert ok == (want is not None), (bw, bh, skew)
                if ok:
                    assert np.array_equal(got, c[want.ravel(), :2].astype(np.float32))
            assert F.label_board_grow(cand, bw, bh) is not None, (bw, bh, skew)      # the clean board is found


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_host_program_under_sanitizers(tmp_path):
    """the labeller and the solver, compiled from their sources into a stand-alone
    program with the address and undefined-behaviour sanitizers, on random and
    degenerate candidate sets and point sets: it must exit clean.  Host code only:
    no device, nothing loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "slam-indoor-code_amd", "csrc")
    exe = str(tmp_path / "fisheye_host_test")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                    *[f for s in san for f in ("-Xarch_host", s)], "-o", exe,
                    os.path.join(root, "tests", "cpp", "fisheye_host_test.cpp"), os.path.join(csrc, "calib_board.cpp"),
                    os.path.join(csrc, "calib_solve.cpp"), san[0]], check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    tally = dict(zip(r.stdout.split()[0::2], map(int, r.stdout.split()[1::2])))
    # every outcome is reached: boards found and not, cameras solved, arguments refused, point sets without a solution
    assert tally["labelled"] >= 50 and tally["unlabelled"] >= 100
    assert tally["solved"] >= 12 and tally["refused"] >= 5 and tally["unsolved"] >= 3


def test_calibrate_the_real_set():
    import calib_ref as C
    names, img = real_corners()
    obj = C.board_points(BOARD, 1.0)
    rms, K, D, rv, tv = slamhip.fisheyeCalibrate(obj, img, (748, 480))
    ref_rms, Kr, Dr, rvr, tvr, ref_cost = F.fisheye_calibrate(obj, img, (748, 480))
    K4 = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    cost = F.cost(obj, img, K4, D, rv, tv)
    print(f"{len(img)} views: rms {rms!r} (reference {ref_rms!r}), K {K4}, D {D.tolist()}")
    assert cost <= ref_cost * (1 + COST_MARGIN_REL)
    p = np.concatenate([K4, D] + [np.r_[r, t] for r, t in zip(rv, tv)])
    r = F.residuals(p, obj.astype(np.float64), img.astype(np.float64)).reshape(len(img), -1, 2)
    per_view = np.sqrt((r ** 2).sum(2).mean(1))
    print("per view:", dict(zip(names, np.round(per_view, 3))))
    assert per_view.max() <= 3 * np.median(per_view)        # a view beyond is a labelling error


# ---------------- the calibration file ----------------

def test_xml_names_the_model(tmp_path):
    K = F.CAMERA_K
    R, T = np.arange(6.0).reshape(2, 3), np.arange(6.0).reshape(2, 3) + 0.5
    path = str(tmp_path / "fisheye.xml")
    slamhip.save_calibration(path, K, F.CAMERA_D, R, T, model="fisheye")
    assert slamhip.calibration_model(path) == "fisheye"
    assert np.array_equal(slamhip.load_calibration(path), K)
    assert np.array_equal(slamhip.load_calibration(path, "DC", model="fisheye").ravel(), F.CAMERA_D)
    assert np.array_equal(slamhip.load_calibration(path, "R"), R)
    with pytest.raises(ValueError):
        slamhip.load_calibration(path, "DC")                      # k1 k2 k3 k4 are never read as k1 k2 p1 p2
    with pytest.raises(ValueError):
        slamhip.save_calibration(path, K, np.zeros(5), R, T, model="fisheye")
    # a file without the node is the polynomial model, as before
    brown = str(tmp_path / "brown.xml")
    slamhip.save_calibration(brown, K, [0.1, 0.2, 0.3, 0.4], R, T)
    assert "model" not in open(brown).read()
    assert slamhip.calibration_model(brown) is None
    assert slamhip.load_calibration(brown, "DC").tolist() == [[0.1, 0.2, 0.3, 0.4]]
    with pytest.raises(ValueError):
        slamhip.load_calibration(brown, "DC", model="fisheye")
    ref = os.path.join(GOLDEN, "calib_samsung_hv.xml")
    assert slamhip.calibration_model(ref) is None and slamhip.load_calibration(ref, "DC").shape == (1, 5)


def test_exports():
    lib = slamhip.lib()
    for name in ("slam_fisheye_undistort_map", "slam_fisheye_undistort", "slam_fisheye_undistort_batch",
                 "slam_fisheye_undistort_points", "slam_fisheye_undistort_points_dev", "slam_fisheye_calibrate",
                 "slam_label_chessboard_grow"):
        assert hasattr(lib, name), name
    assert lib.slam_abi_version() == 3
    for name in ("fisheyeUndistortMap", "fisheyeUndistort", "fisheyeUndistortBatch", "fisheyeUndistortPoints",
                 "fisheyeCalibrate", "calibration_model"):
        assert callable(getattr(slamhip, name)), name


def test_slam_main_refuses_a_wrong_model():
    from slamhip import cycle
    cfg = slamhip.ConfigService(slamhip.reference_example())
    with pytest.raises(ValueError):
        cycle.slam_main(cycle.MediaSources([]), np.eye(3), cfg, ops=object(), dist=np.zeros(4), lens_model="equidistant")
    with pytest.raises(ValueError):
        cycle.slam_main(cycle.MediaSources([]), np.eye(3), cfg, ops=object(), dist=np.zeros(5), lens_model="fisheye")

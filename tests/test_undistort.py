"""CPU tests of the undistortion feature: the calibration-file reader and the
numpy restatement of cv::undistort (tests/undistort_ref.py) that the GPU tests
compare against.

Fixture: tests/golden/calib_samsung_hv.xml is a copy of the reference's
config/samsung-hv.xml, the file its calibration step writes (K, DC, R, T as
OpenCV XML storage, IOmisc.cpp:68-76).  It holds settings only.
"""
import os
import re

import numpy as np
import pytest

import slamhip
import undistort_ref as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CALIB = os.path.join(GOLDEN, "calib_samsung_hv.xml")


def _file_doubles(key):
    """the doubles of <key>'s <data> as the file's text gives them"""
    txt = open(CALIB).read()
    m = re.search(r"<%s type_id=\"opencv-matrix\">.*?<data>(.*?)</data>" % key, txt, re.S)
    return [float(t) for t in m.group(1).split()]


# ---------------- loader ----------------

def test_load_calibration_k_and_dc_exact():
    K = slamhip.load_calibration(CALIB)
    assert K.shape == (3, 3) and K.dtype == np.float64
    assert K.ravel().tolist() == _file_doubles("K")
    assert K.ravel().tolist() == slamhip.load_calibration(CALIB, "K").ravel().tolist()
    assert K[0, 0] == 1.7246758288831063e+03 and K[1, 2] == 5.5019214056476358e+02 and K[2, 2] == 1.0
    D = slamhip.load_calibration(CALIB, "DC")
    assert D.shape == (1, 5)
    assert D.ravel().tolist() == _file_doubles("DC")
    assert D[0, 4] == -2.0091088850887786e+00


def test_load_calibration_multichannel_and_missing_key():
    R = slamhip.load_calibration(CALIB, "R")
    assert R.shape == (13, 3)
    assert R.ravel().tolist() == _file_doubles("R")
    assert slamhip.load_calibration(CALIB, "T").shape == (13, 3)
    with pytest.raises(KeyError):
        slamhip.load_calibration(CALIB, "nope")


# ---------------- reference known answers ----------------

def _img(w, h, ch, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, ch) if ch > 1 else (h, w), dtype=np.uint8)


K0 = np.array([[517.3, 0, 31.5], [0, 519.1, 20.25], [0, 0, 1.0]])


def test_ref_identity():
    for ch in (1, 3):
        src = _img(67, 41, ch, 1)
        xy, frac = U.undistort_map(67, 41, K0, np.zeros(5), K0)
        assert not frac.any()
        gx, gy = np.meshgrid(np.arange(67), np.arange(41))
        assert np.array_equal(xy[..., 0], gx) and np.array_equal(xy[..., 1], gy)
        assert np.array_equal(U.remap(src, xy, frac), src)
        assert np.array_equal(U.undistort(src, K0, np.zeros(4)), src)     # newK absent = K


def test_ref_integer_shift_brings_zeros_in():
    src = _img(67, 41, 3, 2)
    nk = K0.copy()
    nk[0, 2] -= 3
    out = U.undistort(src, K0, np.zeros(5), nk)
    assert np.array_equal(out[:, :-3], src[:, 3:])
    assert not out[:, -3:].any()


def test_ref_half_pixel_shift_averages():
    src = _img(67, 41, 1, 3)
    nk = K0.copy()
    nk[0, 2] -= 0.5
    out = U.undistort(src, K0, np.zeros(5), nk)
    s = src.astype(np.int64)
    assert np.array_equal(out[:, :-1], (s[:, :-1] + s[:, 1:] + 1) >> 1)
    assert np.array_equal(out[:, -1], (s[:, -1] + 1) >> 1)                # the right tap is outside: 0


def test_ref_weight_sets_sum_to_scale():
    wt = U.weights()
    assert wt.shape == (1024, 4) and (wt >= 0).all()
    assert (wt.sum(axis=1) == 32768).all()
    assert (wt % 32 == 0).all()


def test_ref_round_and_wrap_quirks():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 2147483647.4, 2147483647.5, -2147483648.5, -2147483649.0, np.nan,
                  np.inf, -np.inf])
    assert U.cv_round(v).tolist() == [0, 2, 2, 0, -2, 2147483647, U.INT_MIN, U.INT_MIN, U.INT_MIN, U.INT_MIN,
                                      U.INT_MIN, U.INT_MIN]
    # (short)(iu >> 5) wraps: u = 65536 + 7 -> 7
    nk = np.array([[1.0, 0, -65543.0], [0, 1.0, 0], [0, 0, 1.0]])
    k = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])
    xy, frac = U.undistort_map(4, 1, k, np.zeros(5), nk)
    assert xy[0, :, 0].tolist() == [7, 8, 9, 10] and not frac.any()


def test_ref_rejects_bad_models():
    with pytest.raises(ValueError):
        U.undistort_map(4, 4, K0, np.zeros(3))
    with pytest.raises(ValueError):
        U.undistort_map(4, 4, K0, np.zeros(5), np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 0, 1.0]]))


# ---------------- teeth: the tie family tells the wrong variants apart ----------------

tie_family = U.tie_family


def test_teeth_mul_variant_differs():
    K, nk = tie_family(200, 37)
    iu, iv = U.fixed_point(200, 37, K, np.zeros(5), nk)
    mu, mv = U.fixed_point(200, 37, K, np.zeros(5), nk, mode="mul")
    nd = int((iu != mu).sum())
    print("mul variant, 200x37: iu differs in", nd, "of", iu.size)
    assert nd >= 1000


def test_teeth_nostripe_and_mul_differ_with_stripes():
    K, nk = tie_family(333, 70)
    assert U.stripe_rows(333, 70) == 12
    iu, iv = U.fixed_point(333, 70, K, np.zeros(5), nk)
    su, sv = U.fixed_point(333, 70, K, np.zeros(5), nk, mode="nostripe")
    mu, mv = U.fixed_point(333, 70, K, np.zeros(5), nk, mode="mul")
    ns = int((iv != sv).sum())
    nm = int((iu != mu).sum()) + int((iv != mv).sum())
    print("333x70: nostripe iv differs in", ns, "; mul differs in", nm, "of", iu.size)
    assert ns >= 1000
    assert nm >= 1000


def test_samsung_map_moves_pixels_far():
    """the real lens is not a small correction: the 1080p map displaces pixels by
    more than 200 px (rows sampled: the full map is the GPU test's business)"""
    K = slamhip.load_calibration(CALIB)
    D = slamhip.load_calibration(CALIB, "DC")
    iu, iv = U.fixed_point(1920, 8, K, D)     # the top 8 rows (stripe 2)
    gx = np.arange(1920)[None, :]
    gy = np.arange(8)[:, None]
    disp = np.hypot(iu / 32.0 - gx, iv / 32.0 - gy)
    assert disp.max() > 200

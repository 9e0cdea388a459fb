"""CPU oracle checks (no GPU): known-answer tests restated from the reference's
upstream algorithms (OpenCV 4.8 / Ceres 2.2), independent
numpy / scipy cross-checks, and the committed golden fixtures (tests/golden).

The reference ships no tests or fixtures and cannot be built
here (no OpenCV / Ceres), so parity with the reference itself is UNPINNED; these
tests pin the restatement to the published algorithms.
"""
import math
import os

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import oracle_ffi as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------- gray ----------------
def test_bgr2gray_fixed_point():
    rng = np.random.default_rng(0)
    bgr = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    b, g, r = (bgr[..., i].astype(np.int64) for i in range(3))
    ref = ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)
    np.testing.assert_array_equal(O.gray(bgr), ref)
    # coefficient sum is 1 << 14: gray of a gray pixel is itself
    for v in (0, 1, 127, 128, 254, 255):
        assert O.gray(np.full((1, 1, 3), v, np.uint8))[0, 0] == v


# ---------------- FAST ----------------
CIRCLES = {16: [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2),
                (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)],
           12: [(0, 2), (1, 2), (2, 1), (2, 0), (2, -1), (1, -2), (0, -2), (-1, -2), (-2, -1), (-2, 0), (-2, 1),
                (-1, 2)],
           8: [(0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1)]}
PS_OF_TYPE = {O.FAST_9_16: 16, O.FAST_7_12: 12, O.FAST_5_8: 8}


def numpy_fast(img, t, nms=True, ps=16):
    """independent vectorised restatement of FAST_t<ps> + cornerScore<ps> + NMS:
    OpenCV's pair prefilter over the wrapped pixel[0..15] (implied by a 9-arc for
    16, a filter of its own for 12 and 8), a K+1 arc (K = ps / 2) all darker /
    brighter, score = max over K+1 arcs of the min |d| on the consistent side - 1"""
    img = img.astype(np.int32)
    h, w = img.shape
    K = ps // 2
    circ = CIRCLES[ps]
    v = img[3:h - 3, 3:w - 3]
    P = np.stack([img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in circ], -1)
    d = v[..., None] - P
    dark, bright = d > t, d < -t
    tab = dark * 1 + bright * 2
    pre = np.full(v.shape, 3)
    for k in range(8):
        pre &= tab[..., k % ps] | tab[..., (k + 8) % ps]

    def run(m):
        m2 = np.concatenate([m, m], -1)
        ok = np.zeros(m.shape[:-1], bool)
        for s in range(ps):
            ok |= m2[..., s:s + K + 1].all(-1)
        return ok
    corner = ((pre & 1) > 0) & run(dark) | ((pre & 2) > 0) & run(bright)
    dd = np.concatenate([d, d], -1)
    best = np.full(v.shape, t, np.int32)
    for s in range(ps):
        arc = dd[..., s:s + K + 1]
        best = np.maximum(best, arc.min(-1))
        best = np.maximum(best, (-arc).min(-1))
    score = np.where(corner, best - 1, 0)
    full = np.zeros((h, w), np.int32)
    full[3:h - 3, 3:w - 3] = score
    cf = np.zeros((h, w), bool)
    cf[3:h - 3, 3:w - 3] = corner
    keep = cf.copy()
    if nms:
        pad = np.pad(full, 1)
        nb = np.max(np.stack([pad[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                              if (dx, dy) != (0, 0)]), 0)
        keep &= full > nb
    ys, xs = np.nonzero(keep)
    return xs, ys, (full[ys, xs] if nms else np.zeros(len(xs)))


def test_fast_single_pixel_known_answer():
    img = np.zeros((32, 32), np.uint8)
    img[16, 16] = 255
    k = O.fast(img, 10, True)
    assert len(k) == 1
    assert (k[0]["x"], k[0]["y"], k[0]["response"], k[0]["size"], k[0]["angle"]) == (16, 16, 254, 7, -1)
    assert k[0]["octave"] == 0 and k[0]["class_id"] == -1


@pytest.mark.parametrize("ftype", [O.FAST_5_8, O.FAST_7_12, O.FAST_9_16])
def test_fast_types_single_pixel_known_answer(ftype):
    """fastExtractor.h:19-21's detector types (docs/FastExtractor.md:13-16): a
    lone 255 on 0 is a corner of every pattern size with score 255 - 1"""
    img = np.zeros((32, 32), np.uint8)
    img[16, 16] = 255
    k = O.fast(img, 10, True, ftype)
    assert len(k) == 1
    assert (k[0]["x"], k[0]["y"], k[0]["response"], k[0]["size"]) == (16, 16, 254, 7)


@pytest.mark.parametrize("ftype", [O.FAST_5_8, O.FAST_7_12])
@pytest.mark.parametrize("nms", [True, False])
def test_fast_types_vs_numpy(ftype, nms):
    """on a synthetic frame and on noise (OpenCV's pair prefilter over the wrapped
    pixel[0..15] makes TYPE_5_8 need all 8 neighbours beyond the threshold:
    isolated peaks, which noise has)"""
    import slamhip
    imgs = [O.gray(slamhip.synth_frames(160, 120, seed, 1, seed=seed + 10)[0]) for seed in (0, 1)]
    imgs += [np.random.default_rng(s).integers(0, 256, (90, 120), dtype=np.uint8) for s in (3, 4)]
    total = 0
    for g in imgs:
        for t in (5, 15, 30):
            k = O.fast(g, t, nms, ftype)
            xs, ys, sc = numpy_fast(g, t, nms, PS_OF_TYPE[ftype])
            total += len(xs)
            np.testing.assert_array_equal(k["x"], xs)
            np.testing.assert_array_equal(k["y"], ys)
            np.testing.assert_array_equal(k["response"], sc)
    assert total > 100


def test_fast_flat_and_edges_have_no_corners():
    assert len(O.fast(np.full((50, 50), 99, np.uint8), 0, True)) == 0
    step = np.zeros((50, 50), np.uint8)
    step[:, 25:] = 200
    assert len(O.fast(step, 10, True)) == 0
    assert len(O.fast(np.zeros((6, 6), np.uint8), 0, True)) == 0


def test_fast_threshold_clamped():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (40, 40), dtype=np.uint8)
    np.testing.assert_array_equal(O.fast(img, -5, True), O.fast(img, 0, True))
    np.testing.assert_array_equal(O.fast(img, 400, True), O.fast(img, 255, True))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("nms", [True, False])
def test_fast_vs_numpy(seed, nms):
    import slamhip
    f = slamhip.synth_frames(160, 120, seed, 1, seed=seed + 10)[0]
    g = O.gray(f)
    for t in (5, 15, 30):
        k = O.fast(g, t, nms)
        xs, ys, sc = numpy_fast(g, t, nms)
        np.testing.assert_array_equal(k["x"], xs)
        np.testing.assert_array_equal(k["y"], ys)
        np.testing.assert_array_equal(k["response"], sc)


def test_fast_raster_order():
    import slamhip
    f = slamhip.synth_frames(320, 240, 0, 1)[0]
    k = O.fast(f, 10, True)
    key = k["y"].astype(np.int64) * 10000 + k["x"]
    assert np.all(np.diff(key) > 0)


# ---------------- SIFT helpers ----------------
def test_sift_constants():
    s = O.oracle().orc_sift_sigma_diff()
    assert abs(s - math.sqrt(1.6 ** 2 - 0.25)) < 1e-6
    k = np.zeros(13, np.float32)
    O.oracle().orc_gauss_kernel_f32(13, float(s), O.vp(k))
    x = np.arange(13) - 6
    ref = np.exp(-x * x / (2 * float(s) ** 2))
    ref /= ref.sum()
    np.testing.assert_allclose(k, ref, rtol=2e-7)
    np.testing.assert_array_equal(k, k[::-1])
    k7 = np.zeros(7, np.float32)
    O.oracle().orc_gauss_kernel_f32(7, 2.0, O.vp(k7))
    x = np.arange(7) - 3
    ref = np.exp(-x * x / 8.0)
    np.testing.assert_allclose(k7, ref / ref.sum(), rtol=2e-7)


def test_fast_atan2_accuracy_and_quadrants():
    rng = np.random.default_rng(2)
    ys, xs = rng.normal(size=2000), rng.normal(size=2000)
    got = np.array([O.oracle().orc_fast_atan2_deg(float(y), float(x)) for y, x in zip(ys, xs)])
    ref = np.degrees(np.arctan2(ys, xs)) % 360
    err = np.abs(((got - ref) + 180) % 360 - 180)
    assert err.max() < 0.02          # hal::fastAtan2 polynomial accuracy (~0.01 deg)
    assert np.all((got >= 0) & (got <= 360))
    assert O.oracle().orc_fast_atan2_deg(0.0, 1.0) == 0.0
    assert abs(O.oracle().orc_fast_atan2_deg(1.0, 0.0) - 90.0) < 1e-3


def test_exp32f_accuracy():
    xs = np.linspace(-10, 2, 3001)
    got = np.array([O.oracle().orc_exp32f(float(x)) for x in xs])
    np.testing.assert_allclose(got, np.exp(xs), rtol=2e-6)   # OpenCV exp32f: ~1e-6 relative


def test_sift_constant_image_zero_descriptor():
    img = np.full((80, 90, 3), 120, np.uint8)
    kps = np.zeros(2, O.KP)
    kps["x"], kps["y"], kps["size"], kps["angle"] = [40, 5], [40, 70], 7, -1
    d = O.sift(img, kps)
    assert d.shape == (2, 128) and np.all(d == 0)


def test_sift_descriptor_properties():
    import slamhip
    f = slamhip.synth_frames(320, 240, 0, 1)[0]
    k = O.fast(f, 10, True)
    d = O.sift(f, k)
    assert np.all(d == np.round(d)) and d.min() >= 0 and d.max() <= 255
    n = np.linalg.norm(d, axis=1)
    nz = n > 0
    assert nz.mean() > 0.95
    assert np.all(np.abs(n[nz] - 512) < 8)       # renormalised x512, then rounded


# ---------------- ORB ----------------
def test_orb_border_filter_in_place_order():
    import slamhip
    f = slamhip.synth_frames(200, 150, 0, 1)[0]
    k = O.fast(f, 8, True)
    kk, d = O.orb(f, k)
    inside = (k["x"] >= 31) & (k["x"] < 200 - 31) & (k["y"] >= 31) & (k["y"] < 150 - 31)
    np.testing.assert_array_equal(kk, k[inside])
    assert d.shape == (inside.sum(), 32)
    small = np.zeros((60, 60, 3), np.uint8)
    kk, d = O.orb(small, k[:5])
    assert len(kk) == 0 and len(d) == 0


def test_orb_pattern_table_matches_source():
    import subprocess
    import sys
    # the table itself is kept under tests/golden (256 x 4 offsets, scikit-image's
    # orb_descriptor_positions.txt = OpenCV's bit_pattern_31_)
    subprocess.check_call([sys.executable, os.path.join(O.ORACLE_DIR, "gen_orb_pattern.py"),
                           os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                        "orb_bit_pattern_31.npy")])


def test_orb_descriptor_brute_force():
    """recompute bits with the pattern rows read back from the header"""
    import re
    import slamhip
    txt = open(os.path.join(O.ORACLE_DIR, "orb_pattern.h")).read()
    pat = np.array(re.findall(r"-?\d+", txt.split("{", 1)[1].split("}", 1)[0]), int).reshape(256, 4)
    f = slamhip.synth_frames(160, 120, 1, 1)[0]
    k, d = O.orb(f, O.fast(f, 8, True))
    assert len(k) > 5
    # blurred image from the oracle (via the sampling of axis-aligned -1 deg offsets)
    g = O.gray(f)
    blur = np.zeros_like(g)
    O.oracle().orc_orb_blur(O.vp(g), g.shape[1], g.shape[0], O.vp(blur))
    a, b = np.float32(math.cos(np.float32(-1 * np.float32(math.pi / 180)))), \
        np.float32(math.sin(np.float32(-1 * np.float32(math.pi / 180))))
    for j in range(len(k)):
        cx, cy = int(k[j]["x"]), int(k[j]["y"])
        bits = []
        for t in range(256):
            x0, y0, x1, y1 = pat[t].astype(np.float32)
            p0 = (np.float32(x0 * a) - np.float32(y0 * b), np.float32(x0 * b) + np.float32(y0 * a))
            p1 = (np.float32(x1 * a) - np.float32(y1 * b), np.float32(x1 * b) + np.float32(y1 * a))
            v0 = blur[cy + int(np.rint(p0[1])), cx + int(np.rint(p0[0]))]
            v1 = blur[cy + int(np.rint(p1[1])), cx + int(np.rint(p1[0]))]
            bits.append(int(v0 < v1))
        ref = np.packbits(np.array(bits, np.uint8).reshape(32, 8)[:, ::-1], axis=1).ravel()
        np.testing.assert_array_equal(d[j], ref)


# ---------------- kNN + ratio ----------------
def test_knn_l2_vs_numpy_with_ties():
    rng = np.random.default_rng(4)
    q = rng.integers(0, 30, (200, 128)).astype(np.float32)
    t = rng.integers(0, 30, (300, 128)).astype(np.float32)
    t[250] = t[7]
    q[0] = t[7]
    idx, dist = O.knn2(q, t, O.NORM_L2)
    D = np.sqrt(((q[:, None, :].astype(np.float64) - t[None]) ** 2).sum(-1)).astype(np.float32)
    order = np.lexsort((np.broadcast_to(np.arange(len(t)), D.shape), D), axis=1)[:, :2]
    np.testing.assert_array_equal(idx, order)
    np.testing.assert_array_equal(dist, np.take_along_axis(D, order, 1))
    assert idx[0, 0] == 7 and idx[0, 1] == 250 and dist[0, 0] == 0 and dist[0, 1] == 0


@pytest.mark.parametrize("hi", [30, 256])
def test_knn_l2_u8_path_equals_f32_path(hi):
    """orc_knn2_l2_u8 (integer sums) is orc_knn2's f32 scan for integer-valued
    descriptors: same indices, same distances, same tie rule"""
    rng = np.random.default_rng(hi)
    q = rng.integers(0, hi, (300, 128)).astype(np.float32)
    t = rng.integers(0, hi, (400, 128)).astype(np.float32)
    t[5] = t[300] = q[3]                                 # exact ties: lower train index first
    t[17] = t[18]
    a_i, a_d = O.knn2(q, t, O.NORM_L2)
    b_i, b_d = O.knn2(q, t, O.NORM_L2, exact_f32=True)
    np.testing.assert_array_equal(a_i, b_i)
    np.testing.assert_array_equal(a_d, b_d)
    assert a_i[3].tolist() == [5, 300]


def test_knn_hamming_vs_numpy():
    rng = np.random.default_rng(5)
    q = rng.integers(0, 256, (100, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (150, 32), dtype=np.uint8)
    idx, dist = O.knn2(q, t, O.NORM_HAMMING)
    D = np.unpackbits(q[:, None, :] ^ t[None], axis=-1).sum(-1)
    order = np.lexsort((np.broadcast_to(np.arange(len(t)), D.shape), D), axis=1)[:, :2]
    np.testing.assert_array_equal(idx, order)
    np.testing.assert_array_equal(dist, np.take_along_axis(D, order, 1))


def test_ratio_strict_and_edge_cases():
    idx = np.array([[0, 1], [2, 3], [4, -1], [-1, -1], [5, 6]], np.int32)
    dist = np.array([[7.0, 10.0], [6.9, 10.0], [1.0, 3e38], [3e38, 3e38], [0.0, 0.0]], np.float32)
    m = O.ratio(idx, dist, 0.7)
    # float distances are promoted to double and compared strictly against ratio * d1
    exp = [i for i in range(len(idx)) if idx[i, 0] >= 0 and idx[i, 1] >= 0 and
           float(dist[i, 0]) < 0.7 * float(dist[i, 1])]
    assert list(m["queryIdx"]) == exp and 1 in exp and 4 not in exp
    assert list(m["trainIdx"]) == [idx[i, 0] for i in exp]
    d0 = np.float32(0.7) * np.float32(10)
    m2 = O.ratio(np.array([[0, 1]], np.int32), np.array([[d0, 10.0]], np.float32), 0.7)
    assert len(m2) == (1 if float(d0) < 0.7 * 10.0 else 0)


def test_select_good_rule():
    c = [600, 100, 700, 700, 50]
    assert O.select_good(c, 500, 0, True) == 3          # tail-first, first fit
    assert O.select_good(c, 500, 0, False) == 2         # max count, ties -> lowest index
    assert O.select_good(c, 800, 0, False) == -1
    assert O.select_good(c, 500, 3, False) == 3         # skipFramesFromBatchHead
    assert O.select_good([], 0, 0, True) == -1
    assert O.select_good([0, 0], 0, 0, False) == 0


def test_flann_is_close_to_bruteforce():
    import slamhip
    f = slamhip.synth_frames(320, 240, 0, 2)
    k0, k1 = O.fast(f[0], 10, True), O.fast(f[1], 10, True)
    d0, d1 = O.sift(f[0], k0), O.sift(f[1], k1)
    bi, bd = O.knn2(d0, d1, O.NORM_L2)
    fi, fd = np.zeros_like(bi), np.zeros_like(bd)
    O.oracle().orc_flann_knn2(O.vp(d0), len(d0), O.vp(d1), len(d1), 128, 4, 32, 1, O.vp(fi), O.vp(fd))
    assert (fi[:, 0] == bi[:, 0]).mean() > 0.8
    assert np.all(fd[:, 0] >= bd[:, 0] - 1e-3)     # approximate never beats exact


# ---------------- BA ----------------
def test_aa_rotate_vs_rodrigues():
    from slamhip.api import rodrigues_to_matrix
    rng = np.random.default_rng(6)
    for _ in range(20):
        aa = rng.normal(size=3) * rng.choice([1e-9, 0.3, 2.0])
        p = rng.normal(size=3)
        out = np.zeros(3)
        O.oracle().orc_aa_rotate(O.vp(aa), O.vp(p), O.vp(out))
        np.testing.assert_allclose(out, rodrigues_to_matrix(aa) @ p, atol=1e-12)


def test_loss_functions_match_ceres_formulas():
    rho = np.zeros(3)
    for loss, a in [(O.LOSS_HUBER, 2.0), (O.LOSS_CAUCHY, 2.0), (O.LOSS_ARCTAN, 2.0), (O.LOSS_TUKEY, 2.0)]:
        for s in (0.5, 3.0, 9.0):
            O.oracle().orc_loss_eval(loss, a, s, O.vp(rho))
            if loss == O.LOSS_HUBER:
                ref = s if s <= a * a else 2 * a * math.sqrt(s) - a * a
            elif loss == O.LOSS_CAUCHY:
                ref = a * a * math.log1p(s / (a * a))
            elif loss == O.LOSS_ARCTAN:
                ref = a * math.atan2(s, a)
            else:
                ref = a * a / 3 * (1 - (1 - s / (a * a)) ** 3) if s <= a * a else a * a / 3
            assert abs(rho[0] - ref) < 1e-12
            h = 1e-6
            r1, r2 = np.zeros(3), np.zeros(3)
            O.oracle().orc_loss_eval(loss, a, s + h, O.vp(r1))
            O.oracle().orc_loss_eval(loss, a, s - h, O.vp(r2))
            assert abs((r1[0] - r2[0]) / (2 * h) - rho[1]) < 1e-5


def test_ba_zero_noise_converges():
    from slamhip import synthba
    w = synthba.make_window(nframes=3, npoints=200, seed=1, noise=0.0)
    # exact (non-rounded) observations of the ground truth
    xy = np.concatenate([synthba.project(w["gt_K4"], w["gt_ext"][f], w["gt_pts"][[p]])[0]
                         for f, p in zip(w["obs_frame"], w["obs_point"])])
    c0 = O.ba_cost(w["gt_K4"], w["gt_ext"], w["gt_pts"], w["obs_frame"], w["obs_point"], xy)
    assert c0 < 1e-18
    K, E, P, s = O.ba(w["K4"], w["ext"], w["pts"], w["obs_frame"], w["obs_point"], xy)
    assert s.initial_cost > 1.0
    assert s.final_cost < 1e-8 and s.usable == 1   # gauge (scale / focal) valley: slow final approach
    assert s.num_residuals == 2 * len(xy)


def test_ba_trivial_loss_is_scipy_stationary():
    """trivial loss: scipy's least-squares solver started at the oracle's LM
    solution cannot lower the cost (the oracle reached the optimum of the same
    residual, frame 0 held constant as in bundleAdjustment.cpp:86)."""
    from scipy.optimize import least_squares
    from slamhip import synthba
    w = synthba.make_window(nframes=3, npoints=60, seed=2, single_share=0.0)
    K, E, P, s = O.ba(w["K4"], w["ext"], w["pts"], w["obs_frame"], w["obs_point"], w["obs_xy"], O.LOSS_TRIVIAL,
                      0.0, 200)
    assert s.final_cost < 0.01 * s.initial_cost
    nf, npt = w["ext"].shape[0], w["pts"].shape[0]

    def res(x):
        k = x[:4]
        e = np.vstack([w["ext"][:1], x[4:4 + 6 * (nf - 1)].reshape(nf - 1, 6)])
        p = x[4 + 6 * (nf - 1):].reshape(npt, 3)
        out = []
        for f in range(nf):
            sel = w["obs_frame"] == f
            xy, _ = synthba.project(k, e[f], p[w["obs_point"][sel]])
            out.append((xy - w["obs_xy"][sel]).ravel())
        return np.concatenate(out)
    x1 = np.concatenate([K, E[1:].ravel(), P.ravel()])
    r1 = res(x1)
    assert abs(0.5 * float(r1 @ r1) - s.final_cost) <= 1e-9 * s.final_cost
    sp = least_squares(res, x1, method="trf", x_scale="jac", max_nfev=40)
    polished = 0.5 * float(sp.fun @ sp.fun)
    assert polished >= s.final_cost * (1 - 1e-5)   # LM stops at function_tolerance 1e-6 (Ceres default)
    # per-pixel RMS agrees to far better than the 1e-4 px bar
    assert abs(math.sqrt(s.final_cost / s.num_residuals) - math.sqrt(polished / s.num_residuals)) < 1e-4


def test_ba_robust_losses_reduce_cost():
    from slamhip import synthba
    w = synthba.make_window(nframes=4, npoints=150, seed=3)
    for loss, a in [(O.LOSS_HUBER, 4.0), (O.LOSS_CAUCHY, 4.0), (O.LOSS_ARCTAN, 2.0), (O.LOSS_TUKEY, 4.0)]:
        _, E, _, s = O.ba(w["K4"], w["ext"], w["pts"], w["obs_frame"], w["obs_point"], w["obs_xy"], loss, a)
        assert s.final_cost < s.initial_cost and s.usable == 1
        np.testing.assert_array_equal(E[0], w["ext"][0])


# ---------------- golden fixtures ----------------
def golden_files():
    # real_*.npz (real-image inputs) are checked by tests/test_real_images.py
    return sorted(f for f in os.listdir(GOLDEN) if f.endswith(".npz") and not f.startswith("real_")) \
        if os.path.isdir(GOLDEN) else []


@pytest.mark.parametrize("name", golden_files())
def test_golden_fixture(name):
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    kind = str(z["kind"])
    if kind == "fast":
        k = O.fast(z["image"], int(z["threshold"]), bool(z["nms"]))
        np.testing.assert_array_equal(np.stack([k["x"], k["y"], k["response"]], 1), z["expected"])
    elif kind == "sift":
        np.testing.assert_array_equal(O.sift(z["image"], z["keypoints"].view(O.KP).ravel()), z["expected"])
    elif kind == "orb":
        k, d = O.orb(z["image"], z["keypoints"].view(O.KP).ravel())
        np.testing.assert_array_equal(d, z["expected"])
        np.testing.assert_array_equal(k.view(np.uint8).reshape(len(k), 28), z["expected_kps"])
    elif kind == "knn":
        idx, dist = O.knn2(z["query"], z["train"], int(z["norm"]))
        np.testing.assert_array_equal(idx, z["expected_idx"])
        np.testing.assert_array_equal(dist, z["expected_dist"])
    elif kind == "siftdet":
        k, d = O.sift_detect(z["image"])
        np.testing.assert_array_equal(k.view(np.uint8).reshape(len(k), 28), z["expected_kps"])
        np.testing.assert_array_equal(d, z["expected"])
    elif kind == "ba":
        K, E, P, s = O.ba(z["K4"], z["ext"], z["pts"], z["obs_frame"], z["obs_point"], z["obs_xy"], int(z["loss"]),
                          float(z["loss_param"]))
        assert abs(s.final_cost - float(z["final_cost"])) <= 1e-9 * float(z["final_cost"]) + 1e-12
    elif kind == "ba_windows":
        # the searched-frame pipeline's BA windows (GPU parity data): each window is
        # the problem the GPU solved -- the oracle's initial cost equals the cost the
        # GPU reported for it when the fixture was dumped
        k = 0
        while f"w{k}_K4" in z.files:
            c = O.ba_cost(z[f"w{k}_K4"], z[f"w{k}_ext"], z[f"w{k}_pts"], z[f"w{k}_obs_frame"], z[f"w{k}_obs_point"],
                          z[f"w{k}_obs_xy"], int(z[f"w{k}_loss"]), float(z[f"w{k}_loss_param"]))
            g0 = float(z[f"w{k}_r4_gpu_summary"][0])
            assert abs(c - g0) <= 1e-12 * g0, (k, c, g0)
            k += 1
        assert k == 3
    else:
        raise AssertionError(kind)


# ---------------- full SIFT detector (oracle/siftdet.c) ----------------
def _np_blur(img, sigma):
    """float64 separable Gaussian with the oracle's f32 kernel and REFLECT_101"""
    ks = O.oracle().orc_blur_ksize(float(sigma))
    k = np.zeros(ks, np.float32)
    O.oracle().orc_gauss_kernel_f32(ks, float(sigma), O.vp(k))
    k = k.astype(np.float64)
    r = ks // 2
    a = np.pad(img.astype(np.float64), r, mode="reflect")
    rows = sum(k[i] * a[:, i:i + img.shape[1]] for i in range(ks))
    return sum(k[i] * rows[i:i + img.shape[0], :] for i in range(ks))


@pytest.mark.parametrize("sigma", [1.2489996, 1.2262735, 1.5450416, 1.9465878, 2.4525194, 3.0900490])
def test_siftdet_blur_vs_float64(sigma):
    img = np.random.default_rng(3).uniform(0, 255, (37, 53)).astype(np.float32)
    got = O.gauss_blur_f32(img, sigma)
    np.testing.assert_allclose(got, _np_blur(img, sigma), rtol=2e-6, atol=2e-4)


def test_siftdet_blur_wider_than_image():
    # 27-tap kernel on a 9 x 7 top octave: REFLECT_101 folds more than once
    img = np.random.default_rng(4).uniform(0, 255, (7, 9)).astype(np.float32)
    got = O.gauss_blur_f32(img, 3.0900490)
    ks, r = 27, 13
    k = np.zeros(ks, np.float32)
    O.oracle().orc_gauss_kernel_f32(ks, 3.0900490, O.vp(k))

    def refl(p, n):
        while not 0 <= p < n:
            p = -p if p < 0 else 2 * n - p - 2
        return p
    rows = np.array([[sum(k[i] * float(img[y, refl(x - r + i, 9)]) for i in range(ks)) for x in range(9)]
                     for y in range(7)])
    ref = np.array([[sum(k[i] * rows[refl(y - r + i, 7), x] for i in range(ks)) for x in range(9)]
                    for y in range(7)])
    np.testing.assert_allclose(got, ref, rtol=2e-6, atol=2e-4)


def test_siftdet_resize2x_vs_formula():
    img = np.random.default_rng(5).integers(0, 256, (11, 13)).astype(np.float32)
    got = O.resize2x_linear(img)
    h, w = img.shape
    ref = np.zeros((2 * h, 2 * w))
    for dy in range(2 * h):
        fy = (dy + 0.5) * 0.5 - 0.5
        sy = math.floor(fy)
        fy -= sy
        for dx in range(2 * w):
            fx = (dx + 0.5) * 0.5 - 0.5
            sx = math.floor(fx)
            fx -= sx
            if sx < 0:
                sx, fx = 0, 0.0
            if sx >= w - 1:
                sx, fx = w - 1, 0.0

            def hv(y):
                y = min(max(y, 0), h - 1)
                return img[y, sx] * (1 - fx) + (img[y, sx + 1] * fx if fx else 0.0)
            ref[dy, dx] = hv(sy) * (1 - fy) + hv(sy + 1) * fy
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-4)


def test_siftdet_pyramid_structure():
    g = O.gray(slamhip_frames(160, 120))
    pyr = O.sift_pyramid(g)
    assert len(pyr) == int(round(math.log2(240) - 2)) + 1          # doubled base, firstOctave = -1
    assert pyr[0][0][0].shape == (240, 320)
    for o, (gs, ds) in enumerate(pyr):
        for i in range(5):
            np.testing.assert_array_equal(ds[i], gs[i + 1] - gs[i])
        if o > 0:
            prev = pyr[o - 1][0][3]
            H, W = gs[0].shape
            sy = np.minimum(np.floor(np.arange(H) * (prev.shape[0] / H)).astype(int), prev.shape[0] - 1)
            sx = np.minimum(np.floor(np.arange(W) * (prev.shape[1] / W)).astype(int), prev.shape[1] - 1)
            np.testing.assert_array_equal(gs[0], prev[np.ix_(sy, sx)])
    sig = np.zeros(6)
    O.oracle().orc_sift_sigmas(O.vp(sig))
    k = 2 ** (1 / 3)
    for i in range(1, 6):
        assert abs(sig[i] ** 2 - ((1.6 * k ** i) ** 2 - (1.6 * k ** (i - 1)) ** 2)) < 1e-12


def slamhip_frames(w, h, seed=21):
    import slamhip
    return slamhip.synth_frames(w, h, 1, 1, seed=seed)[0]


def test_siftdet_extrema_vs_bruteforce():
    """every refined keypoint sits within one Newton step of a brute-force DoG extremum"""
    f = slamhip_frames(200, 150)
    pyr = O.sift_pyramid(O.gray(f))
    ext = []
    for o, (gs, ds) in enumerate(pyr):
        D = np.stack(ds)
        if D.shape[1] <= 10 or D.shape[2] <= 10:
            continue
        for i in (1, 2, 3):
            c = D[i, 5:-5, 5:-5]
            nb = np.stack([D[i + a, 5 + b:D.shape[1] - 5 + b, 5 + e:D.shape[2] - 5 + e]
                           for a in (-1, 0, 1) for b in (-1, 0, 1) for e in (-1, 0, 1)])
            mx = (c > 0) & (c[None] >= nb).all(0)
            mn = (c < 0) & (c[None] <= nb).all(0)
            ys, xs = np.nonzero((mx | mn) & (np.abs(c) > 1))
            ext += [(o, float(x + 5), float(y + 5)) for y, x in zip(ys, xs)]
    k, _ = O.sift_detect(f, with_desc=False)
    assert len(k) > 20
    ext = np.array(ext)
    for kp in k:
        o = (int(kp["octave"]) & 255)
        o = o - 256 if o >= 128 else o
        pi = o + 1
        # keypoint -> pyramid octave pixel coordinates (input * 2 / 2^pi)
        x, y = kp["x"] * 2 / 2 ** pi, kp["y"] * 2 / 2 ** pi
        sel = ext[ext[:, 0] == pi]
        assert len(sel) and np.min(np.hypot(sel[:, 1] - x, sel[:, 2] - y)) < 5.5


def test_siftdet_blob_known_answer():
    yy, xx = np.mgrid[0:128, 0:128]
    b = (255 * np.exp(-((xx - 64.) ** 2 + (yy - 64.) ** 2) / (2 * 3.0 ** 2))).astype(np.uint8)
    k, d = O.sift_detect(np.repeat(b[..., None], 3, 2))
    assert len(k) >= 1
    # OpenCV's doubled-base mapping shifts keypoints by +0.25 px
    assert np.all(np.abs(k["x"] - 64.25) < 0.05) and np.all(np.abs(k["y"] - 64.25) < 0.05)
    assert np.all((k["size"] > 2 * 2.4) & (k["size"] < 2 * 3.4))
    assert len(O.sift_detect(np.full((64, 64, 3), 100, np.uint8))[0]) == 0


def test_siftdet_output_contract():
    f = slamhip_frames(240, 180, seed=9)
    k, d = O.sift_detect(f)
    assert len(k) > 50 and d.shape == (len(k), 128)
    assert np.all(d == np.round(d)) and d.min() >= 0 and d.max() <= 255
    assert np.all(k["class_id"] == -1) and np.all(k["response"] >= 0.04 / 3 - 1e-7)
    assert np.all((k["angle"] >= 0) & (k["angle"] < 360))
    # sorted by (x asc, y asc, size desc, ...) and duplicate-free in (x, y, size, angle)
    keys = list(zip(k["x"], k["y"], -k["size"], k["angle"]))
    assert keys == sorted(keys)
    assert len(set(keys)) == len(keys)


# ---------------- two-view triangulation (oracle/geom.c) ----------------
def two_view_scene(n, seed, noise=0.0):
    """points in front of two cameras (world = camera 1), their float32 projections"""
    rng = np.random.default_rng(seed)
    K = np.array([[1724.676, 0, 995.966], [0, 1730.482, 550.192], [0, 0, 1.0]])
    R1, t1 = np.eye(3), np.zeros(3)
    ang = np.deg2rad(3.0)
    R2 = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    t2 = np.array([-0.2, 0.01, 0.02])
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1, 1, n), rng.uniform(3, 8, n)], 1)

    def proj(R, t):
        c = X @ R.T + t
        u = c @ K.T
        return (u[:, :2] / u[:, 2:]).astype(np.float32) + rng.normal(0, noise, (n, 2)).astype(np.float32)
    return K, R1, t1, R2, t2, proj(R1, t1), proj(R2, t2), X


def test_triangulate_vs_numpy_svd():
    K, R1, t1, R2, t2, p1, p2, X = two_view_scene(300, 1, noise=0.3)
    got = O.reconstruct(K, R1, t1, R2, t2, p1, p2)
    P1 = K @ np.hstack([R1, t1[:, None]])
    P2 = K @ np.hstack([R2, t2[:, None]])
    ref = []
    for (x1, y1), (x2, y2) in zip(p1.astype(np.float64), p2.astype(np.float64)):
        A = np.stack([x1 * P1[2] - P1[0], y1 * P1[2] - P1[1], x2 * P2[2] - P2[0], y2 * P2[2] - P2[1]])
        v = np.linalg.svd(A)[2][-1]
        ref.append(v[:3] / v[3])
    np.testing.assert_allclose(got, np.array(ref), rtol=1e-9, atol=1e-9)


def test_triangulate_noise_free_recovers_points():
    K, R1, t1, R2, t2, p1, p2, X = two_view_scene(500, 2)
    got = O.reconstruct(K, R1, t1, R2, t2, p1, p2)
    # float32 pixel rounding only: ~1e-4 px -> well under a millimetre at 3-8 m
    assert np.max(np.abs(got - X)) < 2e-3


# ---------------- relative pose: findEssentialMat (RANSAC) + recoverPose (oracle/essential.c) ----------------
def _rot(ax, a):
    ax = np.asarray(ax, float) / np.linalg.norm(ax)
    k = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * k @ k


def relpose_scene(n, seed, noise=0.5, outliers=0.3):
    rng = np.random.default_rng(seed)
    K = np.array([[1724.676, 0, 995.966], [0, 1730.482, 550.192], [0, 0, 1.0]])
    R = _rot([0.1, 1, 0.05], np.deg2rad(4))
    t = np.array([-0.3, 0.02, 0.05])
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 10, n)], 1)

    def proj(P):
        u = P @ K.T
        return u[:, :2] / u[:, 2:]
    p1 = proj(X) + rng.normal(0, noise, (n, 2))
    p2 = proj(X @ R.T + t) + rng.normal(0, noise, (n, 2))
    out = rng.random(n) < outliers
    p2[out] = rng.uniform([0, 0], [1920, 1080], (int(out.sum()), 2))
    return K, R, t, p1.astype(np.float32), p2.astype(np.float32), out


def test_five_point_constraints_and_truth():
    rng = np.random.default_rng(0)
    for trial in range(5):
        R = _rot(rng.normal(size=3), np.deg2rad(rng.uniform(1, 10)))
        t = rng.normal(size=3)
        X = np.stack([rng.uniform(-2, 2, 5), rng.uniform(-1, 1, 5), rng.uniform(3, 8, 5)], 1)
        q1 = X[:, :2] / X[:, 2:]
        Xc = X @ R.T + t
        q2 = Xc[:, :2] / Xc[:, 2:]
        Es = O.five_point(q1, q2)
        assert 1 <= len(Es) <= 10
        Et = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
        Et /= np.linalg.norm(Et)
        for E in Es:
            h1, h2 = np.c_[q1, np.ones(5)], np.c_[q2, np.ones(5)]
            assert np.max(np.abs(np.einsum("ni,ij,nj->n", h2, E, h1))) < 1e-10
            assert abs(np.linalg.det(E)) < 1e-10
            assert np.max(np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E)) < 1e-10
        assert min(min(np.linalg.norm(E - Et), np.linalg.norm(E + Et)) for E in Es) < 1e-9


def test_ransac_subsets_match_cv_rng():
    """cv::RNG((uint64)-1) multiply-with-carry + getSubset's distinct draws, restated independently"""
    state = (1 << 64) - 1
    def nxt():
        nonlocal state
        state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & ((1 << 64) - 1)
        return state & 0xFFFFFFFF
    count, iters = 737, 50
    ref = []
    for _ in range(iters):
        sub = []
        while len(sub) < 5:
            v = nxt() % count
            if v not in sub:
                sub.append(v)
        ref.append(sub)
    got = np.zeros(iters * 5, np.int32)
    O.oracle().orc_ep_subsets(count, iters, O.vp(got))
    assert got.reshape(iters, 5).tolist() == ref


def test_ransac_update_iters():
    for p, ep, it in [(0.999, 0.3, 1000), (0.999, 0.0, 1000), (0.99, 0.9, 1000), (0.999, 0.5, 40)]:
        num = np.log(max(1 - p, np.finfo(float).tiny))
        den = np.log(1 - (1 - ep) ** 5) if 1 - (1 - ep) ** 5 >= np.finfo(float).tiny else None
        want = 0 if den is None else (it if den >= 0 or -num >= it * (-den) else int(np.rint(num / den)))
        assert O.oracle().orc_ransac_update_iters(p, ep, 5, it) == want


@pytest.mark.parametrize("seed,outliers", [(1, 0.3), (2, 0.0), (3, 0.5)])
def test_estimate_transformation_recovers_pose(seed, outliers):
    K, R, t, p1, p2, out = relpose_scene(1500, seed, outliers=outliers)
    ok, Rg, tg, cm, rm, passed = O.estimate_transformation(p1, p2, K, True, 0.999, 5.0, 200.0)
    assert ok and passed > 0
    ang = np.degrees(np.arccos(np.clip((np.trace(Rg.T @ R) - 1) / 2, -1, 1)))
    # the best minimal-sample model (no refinement, as findEssentialMat): ~1 deg at 0.5 px noise
    assert ang < 2.0
    assert np.degrees(np.arccos(np.clip(tg @ t / np.linalg.norm(t), -1, 1))) < 6.0
    assert ((rm == 1) == ~out).mean() >= 0.95   # a few outliers fall within 5 px of their epipolar line


# ---------------- solvePnPRansac (oracle/pnp.c) ----------------
def pnp_scene(n, seed, noise=0.5, outliers=0.3, K=None):
    """3D map points (Point3f) seen by a camera at (R, t) with pixel noise and
    uniformly scattered outliers, as mainCycle.cpp:136-161 feeds solvePnPRansac"""
    rng = np.random.default_rng(seed)
    if K is None:
        K = np.array([[1724.676, 0, 995.966], [0, 1730.482, 550.192], [0, 0, 1.0]])
    rvec = rng.normal(size=3) * 0.2
    R = Rotation.from_rotvec(rvec).as_matrix()
    t = np.array([0.4, -0.1, 0.3]) + rng.normal(size=3) * 0.1
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 10, n)], 1)
    X = ((X - t) @ R).astype(np.float32)             # world points whose camera-frame depth is 3..10
    Xc = X.astype(np.float64) @ R.T + t
    uv = Xc[:, :2] / Xc[:, 2:] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]] + rng.normal(0, noise, (n, 2))
    out = rng.random(n) < outliers
    uv[out] = rng.uniform([0, 0], [1920, 1080], (int(out.sum()), 2))
    return K, rvec, t, X, uv.astype(np.float32), out


def test_rodrigues_matches_scipy_and_fd_jacobian():
    rng = np.random.default_rng(0)
    for _ in range(20):
        rv = rng.normal(size=3) * rng.uniform(0.01, 3)
        R, J = O.rodrigues(rv)
        np.testing.assert_allclose(R, Rotation.from_rotvec(rv).as_matrix(), atol=1e-14)
        back = O.rodrigues(R)                           # |theta| <= pi representative
        assert np.linalg.norm(back) <= np.pi + 1e-12
        np.testing.assert_allclose(O.rodrigues(back)[0], R, atol=1e-12)
        h = 1e-6
        for i in range(3):
            d = np.zeros(3)
            d[i] = h
            fd = (O.rodrigues(rv + d)[0] - O.rodrigues(rv - d)[0]).ravel() / (2 * h)
            np.testing.assert_allclose(J[i], fd, atol=1e-8)
    # zero vector and the theta = pi branch of matrix -> vector
    R, J = O.rodrigues(np.zeros(3))
    np.testing.assert_array_equal(R, np.eye(3))
    rv = np.array([0.0, np.pi, 0.0])
    back = O.rodrigues(Rotation.from_rotvec(rv).as_matrix())
    assert np.allclose(back, rv) or np.allclose(back, -rv)
    # checkRange failure -> zero vector
    np.testing.assert_array_equal(O.rodrigues(np.full((3, 3), 1e3)), np.zeros(3))


@pytest.mark.parametrize("n", [5, 6, 50, 500])
def test_epnp_noise_free(n):
    K, rv, t, X, uv, _ = pnp_scene(n, n, noise=0.0, outliers=0.0)
    R, tt = O.epnp(X.astype(np.float64), uv, K)
    Rt = Rotation.from_rotvec(rv).as_matrix()
    assert np.abs(R - Rt).max() < 1e-5       # f32 image points: ~1e-4 px of rounding
    assert np.abs(tt - t).max() < 1e-4
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)


def test_pnp_iterative_converges_and_matches_fd():
    K, rv, t, X, uv, _ = pnp_scene(300, 9, noise=0.0, outliers=0.0)
    r, tt, it = O.pnp_iterative(X, uv.astype(np.float64), K, rv + 0.02, t - 0.05)
    assert it <= 20
    np.testing.assert_allclose(r, rv, atol=1e-6)
    np.testing.assert_allclose(tt, t, atol=1e-5)


@pytest.mark.parametrize("seed,outliers", [(1, 0.3), (2, 0.0), (3, 0.5)])
def test_solve_pnp_ransac_recovers_pose(seed, outliers):
    K, rv, t, X, uv, out = pnp_scene(1500, seed, outliers=outliers)
    st, r, tt, mask, ni = O.solve_pnp_ransac(X, uv, K)
    assert st == 1 and ni == int(mask.sum())
    ang = np.degrees(np.linalg.norm((Rotation.from_rotvec(r).inv() * Rotation.from_rotvec(rv)).as_rotvec()))
    assert ang < 0.05                                  # LM-refined over ~1000 inliers at 0.5 px
    assert np.linalg.norm(tt - t) < 0.01
    assert ((mask == 1) == ~out).mean() >= 0.99


def test_solve_pnp_ransac_edges():
    K, rv, t, X, uv, out = pnp_scene(5, 4, noise=0.0, outliers=0.0)
    st, r, tt, mask, ni = O.solve_pnp_ransac(X, uv, K)     # npoints == 5: one EPnP, no refinement
    assert st == 1 and ni == 5 and mask.all()
    np.testing.assert_allclose(r, rv, atol=1e-4)
    assert O.solve_pnp_ransac(X[:4], uv[:4], K)[0] == -1   # P3P path not restated
    # all outliers: no model reaches 5 inliers
    rng = np.random.default_rng(3)
    st, r, tt, mask, ni = O.solve_pnp_ransac(X.repeat(20, 0) + rng.normal(size=(100, 3)).astype(np.float32),
                                             rng.uniform(0, 1000, (100, 2)), K)
    assert st in (0, 1)
    if st == 0:
        assert ni == 0 and not mask.any()


def test_gray_input_equals_expanded_bgr():
    """1-channel frames: the gray -> BGR expansion the oracle wrappers apply is
    lossless (cvtColor of B = G = R = g is g), so SIFT / ORB of a gray frame equal
    those of its 3-channel copy"""
    rng = np.random.default_rng(9)
    g = rng.integers(0, 256, (90, 130), dtype=np.uint8)
    bgr = np.repeat(g[..., None], 3, 2)
    np.testing.assert_array_equal(O.gray(bgr), g)
    k = O.fast(g, 10, True)
    assert len(k) > 20
    np.testing.assert_array_equal(O.sift(g, k), O.sift(bgr, k))
    np.testing.assert_array_equal(O.orb(g, k)[1], O.orb(bgr, k)[1])

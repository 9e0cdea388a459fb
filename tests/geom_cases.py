"""Adversarial fixtures for the geometry stage (seeded numpy only) -- TEST INFRASTRUCTURE.

Relative pose (csrc/essential.hip), solvePnPRansac (csrc/pnp.hip) and the
two-view triangulation (csrc/geom.hip) are promised bit for bit against
oracle/essential.c, oracle/pnp.c and oracle/geom.c.  Every case below names the
property it was built for:

  relative pose   the chunk of hypotheses the RANSAC replay needs (relative_pose
                  launches [0, 64), [64, 320), [320, 1000)), the branches of the
                  five-point solver only degenerate samples reach (singular
                  Gauss-Jordan, dropped polynomial degree, roots next to the
                  |im| <= 1e-10 rule, NaN models), counts a call leaves behind
                  for the next, n at the block edges of ep_score / ep_mask (256)
                  and ep_cheir (128), and the option grid
  solvePnPRansac  the inlier count m at the seams of pnp_reduce (groups of 8 and
                  16 rows, chunks of 256), the longest run of rejected LM steps
                  (the host evaluates 3 dampings per launch), planar and
                  duplicated object points, n = 5 / 6 and the option edges
  triangulation   rank-deficient systems (same pixel, parallel rays, a point on
                  the baseline), points behind the cameras, n at the block edge 128

tests/test_geom_cases.py proves each property with the oracle alone (exact
conditions, no tolerances); tests/test_geom_gpu.py compares the library with the
oracle on every case.
"""
import functools
from collections import namedtuple

import numpy as np

from test_oracle import _rot, pnp_scene, relpose_scene, two_view_scene

K_REF = np.array([[1724.676, 0, 995.966], [0, 1730.482, 550.192], [0, 0, 1.0]])
# a principal point that float32 pixels hit exactly: normalised coordinates 0
K_INT = np.array([[1000.0, 0, 960.0], [0, 1000.0, 540.0], [0, 0, 1.0]])

# ---- relative pose -----------------------------------------------------------------
# klass: the property the case was built for.  expect: what the oracle must say -- any of
# ok, passed, rmask (RANSAC mask sum), cmask (chirality mask sum), chunk (the class
# of the needed-hypothesis count), nan (R and t hold NaN)
RelCase = namedtuple("RelCase", "name klass p1 p2 K ransac prob threshold dist expect")

CHUNKS = ("le64", "65_320", "321_999", "1000")


def chunk_of(needed):
    """the class of a needed-hypothesis count: relative_pose's launches cover
    [0, 64), [64, 320) and [320, 1000); exactly 1000 is the cap kMaxIters"""
    return CHUNKS[0] if needed <= 64 else CHUNKS[1] if needed <= 320 else CHUNKS[2] if needed <= 999 else CHUNKS[3]


def _rel(name, klass, p1, p2, K=K_REF, ransac=True, prob=0.999, threshold=5.0, dist=200.0, **expect):
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
    return RelCase(name, klass, p1, p2, np.array(K, np.float64), ransac, prob, threshold, dist, expect)


def _proj(P, K=K_REF):
    u = P @ K.T
    return u[:, :2] / u[:, 2:]


_R = _rot([0.1, 1, 0.05], np.deg2rad(4))
_T = np.array([-0.3, 0.02, 0.05])

# (n, seed, outliers) of relpose_scene -> needed hypotheses (measured by test_geom_cases.py)
REL_CHUNK_SCENES = (
    ((100, 29, 0.1), 5), ((40, 5, 0.2), 38),                          # <= 64: one launch
    ((200, 27, 0.45), 85), ((300, 26, 0.5), 167), ((300, 28, 0.55), 320),   # 65..320; 320: the second chunk's last
    ((64, 25, 0.6), 358), ((600, 21, 0.6), 813),                      # 321..999: the third launch, cut short
    ((600, 22, 0.7), 1000), ((400, 23, 0.75), 1000), ((300, 24, 0.8), 1000),   # the full 1000
)
REL_EDGE_N = (6, 7, 8, 127, 128, 129, 255, 256, 257)
REL_PROBS, REL_THRESHOLDS, REL_DISTS = (0.5, 0.999, 1.0), (0.5, 5.0, 50.0), (5.0, 200.0)

# five collinear image points, shifted along their line in the second view: every
# five-point model of this sample is NaN (10 of them)
_LINE5 = np.array([300.0, 200.0]) + np.array([0, 40, 90, 150, 199.0])[:, None] * np.array([6.0, 0.0])
NAN5 = (_LINE5, _LINE5 + [6.0, 0.0])
# five points at the principal point of K_INT in both views: every row of the
# 5 x 9 system is (0, .., 0, 1), the Gauss-Jordan elimination meets a zero pivot
# and the solver returns no model before it reaches the root finder
ZERO5 = (np.tile([960.0, 540.0], (5, 1)), np.tile([960.0, 540.0], (5, 1)))
# RANSAC's first sample of a six-point set (cv::RNG(-1), getSubset)
FIRST_SUBSET_OF_6 = (3, 4, 2, 5, 0)


def rel_chunk(n, seed, outliers, needed):
    K, R, t, p1, p2, out = relpose_scene(n, seed, outliers=outliers)
    return _rel(f"chunk-{n}-{seed}", "chunk:" + chunk_of(needed), p1, p2, K, ok=True, needed=needed,
                chunk=chunk_of(needed))


# A stale-count trap for the last block of a hypothesis launch: relative_pose's
# scratch layout depends only on n, so a call on the same points leaves its
# counts where the next call expects its own.  "wide" is a chunk scene at prob 1
# (all 1000 hypotheses run) and a 50 px threshold; the chunk case after it needs
# `needed` hypotheses, and the wide call's count for hypothesis needed - 1 is
# larger than the chunk case's best: were that slot not rewritten, the replay
# would take it.  (wide case, chunk case)
REL_STALE_TRAPS = (("wide-600-21", "chunk-600-21"), ("wide-400-23", "chunk-400-23"))


def rel_wide(n, seed, outliers):
    K, R, t, p1, p2, out = relpose_scene(n, seed, outliers=outliers)
    return _rel(f"wide-{n}-{seed}", "stale:wide", p1, p2, K, prob=1.0, threshold=50.0, ok=True, chunk="1000")


def rel_degenerate():
    rng = np.random.default_rng(77)
    n = 200
    out = []
    a, b = np.array([[700.25, 400.5]]), np.array([[720.75, 398.25]])
    # every sample is five times the same correspondence: 10 NaN models each, no inlier ever
    out.append(_rel("identical", "degenerate:identical", np.repeat(a, n, 0), np.repeat(b, n, 0),
                    ok=False, passed=0, rmask=0, cmask=0, chunk="1000"))
    p = rng.uniform([0, 0], [1920, 1080], (n, 2))
    # zero motion: every E fits every point (x' E x = 0 for skew E); no pose passes the chirality test
    out.append(_rel("same_points", "degenerate:p1_eq_p2", p, p, ok=False, passed=0, rmask=n, chunk="le64"))
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 10, n)], 1)
    out.append(_rel("pure_rotation", "degenerate:pure_rotation", _proj(X), _proj(X @ _R.T),
                    ok=False, passed=0, rmask=n, chunk="le64"))
    Xp = X.copy()
    Xp[:, 2] = 6 + 0.3 * Xp[:, 0] - 0.2 * Xp[:, 1]          # a wall
    q1 = _proj(Xp) + rng.normal(0, 0.5, (n, 2))
    q2 = _proj(Xp @ _R.T + _T) + rng.normal(0, 0.5, (n, 2))
    out.append(_rel("planar", "degenerate:planar", q1, q2, ok=True, passed=n, rmask=n, chunk="le64"))
    out.append(_rel("planar-no_ransac", "degenerate:planar_no_ransac", q1, q2, ransac=False, ok=True, passed=93,
                    rmask=173, chunk="le64"))
    s = np.linspace(0, 1, n)[:, None]
    line = np.array([300.0, 200.0]) + s * np.array([1194.0, 0.0])
    # a line of image points shifted along itself: models (where not NaN) fit every point, none gives a pose
    out.append(_rel("collinear", "degenerate:collinear", line, line + [6.0, 0.0], ok=False, passed=0, rmask=n,
                    chunk="le64"))
    g = np.stack(np.meshgrid(np.arange(12) * 100 + 400.0, np.arange(12) * 60 + 200.0), -1).reshape(-1, 2)
    out.append(_rel("grid", "degenerate:grid", g, g, ok=False, passed=0, rmask=144, chunk="le64"))
    out.append(_rel("grid-shifted", "degenerate:grid_shifted", g, g + [7.0, 0.0], ok=False, passed=0, rmask=144,
                    chunk="le64"))
    out.append(_rel("zeros", "degenerate:zeros", np.zeros((50, 2)), np.zeros((50, 2)), ok=True, passed=50, rmask=50))
    out.append(_rel("noise", "degenerate:noise", rng.uniform([0, 0], [1920, 1080], (n, 2)),
                    rng.uniform([0, 0], [1920, 1080], (n, 2)), ok=True, passed=156, rmask=14, chunk="1000"))
    # six points: the first sample is NAN5, the sixth point is free
    p1, p2 = np.zeros((6, 2)), np.zeros((6, 2))
    p1[list(FIRST_SUBSET_OF_6)], p2[list(FIRST_SUBSET_OF_6)] = NAN5
    p1[1], p2[1] = [900.0, 100.0], [880.0, 130.0]
    out.append(_rel("six-nan_first", "degenerate:six_nan_first", p1, p2, ok=True, passed=6, rmask=6))
    # a static camera and moving clutter: 45 % unmoved points, the rest anywhere.  RANSAC goes on
    # into the second launch, and samples with unmoved points give polynomials of degree 9
    rng = np.random.default_rng(78)
    p2 = p.copy()
    moved = rng.random(n) < 0.55
    p2[moved] = rng.uniform([0, 0], [1920, 1080], (int(moved.sum()), 2))
    out.append(_rel("same_points-clutter", "degenerate:p1_eq_p2_clutter", p, p2, ok=True, chunk="65_320"))
    return out


# Walking straight at a fronto-parallel wall (no rotation, no noise): the
# five-point polynomial has double roots, which Durand-Kerner leaves as pairs
# with imaginary parts around 1e-9.  In each of these (n, seed) the first sample
# has a root with 1e-10 < |im| <= 1e-9: complex under the solver's 1e-10 rule,
# real under any laxer one, and the result changes with it.
REL_FORWARD_WALL = ((5, 431), (5, 495), (30, 430), (30, 487), (200, 455))
IM_RULE = 1e-10


def rel_forward_wall(n, seed):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-1.5, 1.5, n), np.full(n, 6.0)], 1)
    return _rel(f"forward_wall-{n}-{seed}", "five_point:near_real_root", _proj(X), _proj(X + [0, 0, -0.3]))


def rel_small():
    K, R, t, p1, p2, _ = relpose_scene(5, 4, outliers=0.0)
    return [
        _rel("n5-solvable", "n5:solvable", p1, p2, K, ok=True, passed=2, rmask=5),
        _rel("n5-identical", "n5:identical", *ZERO5, K=K_INT, ok=False, passed=0, rmask=0, cmask=0),
        # n == 5 takes the first model as it is: NaN, "found", every point an inlier, no pose
        _rel("n5-nan_models", "n5:nan_models", *NAN5, ok=False, passed=0, rmask=5, cmask=0, nan=True),
        _rel("n0", "n:0", p1[:0], p2[:0], K, ok=False, passed=0),
        _rel("n4", "n:4", p1[:4], p2[:4], K, ok=False, passed=0, rmask=0, cmask=0),
    ]


def rel_edge(n):
    K, R, t, p1, p2, _ = relpose_scene(n, 100 + n, outliers=0.2)
    return _rel(f"edge-{n}", f"edge:{n}", p1, p2, K, ok=True, chunk="le64")


def rel_param(prob, threshold, dist):
    K, R, t, p1, p2, _ = relpose_scene(300, 31, outliers=0.3)
    return _rel(f"param-{prob}-{threshold}-{dist}", "param", p1, p2, K, prob=prob, threshold=threshold, dist=dist,
                ok=True)


# ---- solvePnPRansac ----------------------------------------------------------------
# m: the inlier count the case was built for (None: not part of the case).  displaced:
# how many leading image points were moved off.  lm_run: the longest run of rejected
# LM steps (None: not part of the case).  st: the oracle's status (None: not fixed)
PnpCase = namedtuple("PnpCase", "name klass X uv K iters reproj conf m displaced lm_run st")

PNP_SWEEP_M = (6, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 255, 256, 257, 263, 264, 265, 271, 272, 511, 512, 513,
               520, 769)
PNP_PAIRWISE_M = (7, 8, 9, 256, 257, 513)
# pnp_scene(n, seed, noise, outliers), reprojectionError -> (longest run, rejected steps in all)
PNP_LM_SCENES = (
    ((30, 1008, 1.0, 0.2), 8.0, 1), ((60, 1004, 3.0, 0.4), 30.0, 2), ((12, 1009, 30.0, 0.5), 2000.0, 3),
    ((50, 1009, 2.0, 0.3), 15.0, 4), ((12, 1006, 30.0, 0.5), 2000.0, 4), ((20, 1006, 20.0, 0.5), 1000.0, 5),
    ((40, 1002, 6.0, 0.3), 60.0, 7), ((200, 1000, 4.0, 0.5), 200.0, 14), ((6, 2138, 100.0, 0.0), 1e5, 18),
)
PNP_PAIRWISE_LM = ("lm-run2-60-1004", "lm-run7-40-1002")


def _pnp(name, klass, X, uv, K=K_REF, iters=100, reproj=8.0, conf=0.99, m=None, displaced=0, lm_run=None, st=None):
    X = np.ascontiguousarray(X, np.float32).reshape(-1, 3)
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    return PnpCase(name, klass, X, uv, np.array(K, np.float64), iters, reproj, conf, m, displaced, lm_run, st)


def pnp_sweep(m):
    """exactly m inliers: a noise-free scene of m + k points whose first k image
    points are moved far off (k = 3 by +250 px up to m = 33, k = 40 by +-300 px above)"""
    k = 3 if m <= 33 else 40
    K, rv, t, X, uv, _ = pnp_scene(m + k, 200 + m, noise=0.0, outliers=0.0)
    uv = uv.copy()
    if k == 3:
        uv[:k] += np.float32(250.0)
    else:
        uv[:k] += np.where(np.arange(k) % 2 == 0, 300.0, -300.0).astype(np.float32)[:, None]
    return _pnp(f"sweep-{m}", f"sweep:{m}", X, uv, K, m=m, displaced=k, st=1)


def pnp_lm(scene, reproj, run):
    n, seed, noise, outliers = scene
    K, rv, t, X, uv, _ = pnp_scene(n, seed, noise=noise, outliers=outliers)
    return _pnp(f"lm-run{run}-{n}-{seed}", f"lm:run{run}", X, uv, K, reproj=reproj, lm_run=run, st=1)


def _planar_scene(n, seed, exact):
    """object points on a wall 6 m before the camera, 0.5 px noise, 20 % outliers.
    exact: the wall is the world plane z = 0, so the third coordinate is exactly
    zero and EPnP's control points are rank-deficient to the last bit (every
    hypothesis fails: "no model"); otherwise the plane is tilted in the world
    frame and planar only up to float32 rounding (a model is found)"""
    rng = np.random.default_rng(seed)
    rv = rng.normal(size=3) * 0.2
    R = _rot(rv, np.linalg.norm(rv))
    t = np.array([0.4, -0.1, 6.0]) + rng.normal(size=3) * 0.1
    a, b = rng.uniform(-3, 3, n), rng.uniform(-1.5, 1.5, n)
    X = np.stack([a, b, np.zeros(n) if exact else 0.5 * a - 0.25 * b], 1).astype(np.float32)
    uv = _proj(X.astype(np.float64) @ R.T + t) + rng.normal(0, 0.5, (n, 2))
    out = rng.random(n) < 0.2
    uv[out] = rng.uniform([0, 0], [1920, 1080], (int(out.sum()), 2))
    return X, uv


def pnp_misc():
    out = []
    for n in (60, 200):
        X, uv = _planar_scene(n, 300 + n, True)
        out.append(_pnp(f"planar-{n}", f"planar:{n}", X, uv, st=0))
        X, uv = _planar_scene(n, 300 + n, False)
        out.append(_pnp(f"planar_tilted-{n}", f"planar_tilted:{n}", X, uv, st=1))
    # duplicated object points: every third point a copy of its predecessor (object and image)
    K, rv, t, X, uv, _ = pnp_scene(90, 41, outliers=0.2)
    X, uv = X.copy(), uv.copy()
    X[2::3], uv[2::3] = X[1::3], uv[1::3]
    out.append(_pnp("duplicates", "duplicates", X, uv, K))
    # the same object point under different pixels: whole samples can be one point
    X2 = X.copy()
    X2[:30] = X2[0]
    out.append(_pnp("duplicates-one_point_30", "duplicates", X2, uv, K))
    K, rv, t, X, uv, _ = pnp_scene(6, 43, noise=0.5, outliers=0.0)
    out.append(_pnp("n6", "n:6", X, uv, K))
    out.append(_pnp("n5", "n:5", X[:5], uv[:5], K, st=1, m=5))
    K, rv, t, X, uv, _ = pnp_scene(120, 44, outliers=0.3)
    out.append(_pnp("iterations-1", "option:iterations1", X, uv, K, iters=1))
    out.append(_pnp("confidence-0.5", "option:confidence0.5", X, uv, K, conf=0.5))
    out.append(_pnp("confidence-0.999999", "option:confidence0.999999", X, uv, K, conf=0.999999))
    return out


# ---- triangulation -----------------------------------------------------------------
TriCase = namedtuple("TriCase", "name klass K R1 t1 R2 t2 p1 p2")
TRI_N = (1, 255, 256, 257)


def _tri(name, klass, K, R1, t1, R2, t2, p1, p2):
    return TriCase(name, klass, K, R1, t1, R2, t2, np.ascontiguousarray(p1, np.float32).reshape(-1, 2),
                   np.ascontiguousarray(p2, np.float32).reshape(-1, 2))


def tri_cases():
    K, R1, t1, R2, t2, p1, p2, X = two_view_scene(130, 51, noise=0.3)
    out = [
        # the same pixel in both views: the rays meet (if at all) far behind or before the cameras
        _tri("same_pixel", "same_pixel", K, R1, t1, R2, t2, p1, p1),
        # the second camera only translated, same pixel: parallel rays, the point at infinity (w = 0)
        _tri("parallel_rays", "parallel_rays", K, R1, t1, R1, t2, p1, p1),
        # the views swapped: each pixel under the other camera's projection
        _tri("swapped_views", "swapped_views", K, R1, t1, R2, t2, p2, p1),
        # the scene mirrored through the first camera's centre: every point at negative depth in both cameras
        _tri("behind_cameras", "behind_cameras", K, R1, t1, R2, t2, _proj(-X @ R1.T + t1, K), _proj(-X @ R2.T + t2, K)),
    ]
    # points on the line through both camera centres: they project to the two epipoles,
    # every such point gives the same (rank-deficient) system
    c2 = -R2.T @ t2
    Xb = np.array([-50.0, -75.0, -120.0])[:, None] * c2[None]
    out.append(_tri("on_baseline", "on_baseline", K, R1, t1, R2, t2, _proj(Xb @ R1.T + t1, K),
                    _proj(Xb @ R2.T + t2, K)))
    for n in TRI_N:
        K, R1, t1, R2, t2, p1, p2, X = two_view_scene(n, 60 + n, noise=0.5)
        out.append(_tri(f"n-{n}", f"n:{n}", K, R1, t1, R2, t2, p1, p2))
    return out


# ---- the registries: name -> builder ------------------------------------------------
def _many(reg, fn):
    cached = functools.lru_cache(None)(fn)
    for k, c in enumerate(cached()):
        reg[c.name] = (lambda k=k: cached()[k])


def _rel_registry():
    reg = {}
    for (n, seed, o), needed in REL_CHUNK_SCENES:
        reg[f"chunk-{n}-{seed}"] = functools.partial(rel_chunk, n, seed, o, needed)
        if f"wide-{n}-{seed}" in [w for w, _ in REL_STALE_TRAPS]:
            reg[f"wide-{n}-{seed}"] = functools.partial(rel_wide, n, seed, o)
    _many(reg, rel_degenerate)
    _many(reg, rel_small)
    for n, seed in REL_FORWARD_WALL:
        reg[f"forward_wall-{n}-{seed}"] = functools.partial(rel_forward_wall, n, seed)
    for n in REL_EDGE_N:
        reg[f"edge-{n}"] = functools.partial(rel_edge, n)
    for prob in REL_PROBS:
        for thr in REL_THRESHOLDS:
            for dist in REL_DISTS:
                reg[f"param-{prob}-{thr}-{dist}"] = functools.partial(rel_param, prob, thr, dist)
    return reg


def _pnp_registry():
    reg = {}
    for m in PNP_SWEEP_M:
        reg[f"sweep-{m}"] = functools.partial(pnp_sweep, m)
    for scene, reproj, run in PNP_LM_SCENES:
        reg[f"lm-run{run}-{scene[0]}-{scene[1]}"] = functools.partial(pnp_lm, scene, reproj, run)
    _many(reg, pnp_misc)
    return reg


def _tri_registry():
    reg = {}
    _many(reg, tri_cases)
    return reg


REL, PNP, TRI = _rel_registry(), _pnp_registry(), _tri_registry()
REL_NAMES, PNP_NAMES, TRI_NAMES = tuple(REL), tuple(PNP), tuple(TRI)


@functools.lru_cache(None)
def rel(name):
    c = REL[name]()
    assert c.name == name, (c.name, name)
    return c


@functools.lru_cache(None)
def pnp(name):
    c = PNP[name]()
    assert c.name == name, (c.name, name)
    return c


@functools.lru_cache(None)
def tri(name):
    c = TRI[name]()
    assert c.name == name, (c.name, name)
    return c


# ---- the oracle's answer to a case, computed once and shared (read-only arrays) -------
RelRef = namedtuple("RelRef", "ok R t cmask rmask passed")
PnpRef = namedtuple("PnpRef", "st rvec tvec mask ninliers lm")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


def needed_iters(prob, n, inliers):
    """RANSACUpdateNumIters for the final inlier count, from the full 1000"""
    import oracle_ffi as O
    return O.oracle().orc_ransac_update_iters(float(prob), (n - inliers) / n, 5, 1000)


def rel_needed(case, rmask):
    """the hypotheses the RANSAC loop runs before it stops, from a final RANSAC mask
    (with RANSAC off the ABI uses findEssentialMat's default prob 0.999)"""
    return needed_iters(case.prob if case.ransac else 0.999, len(case.p1), int(rmask.sum()))


def rel_hypothesis_counts(case, it, threshold):
    """the inlier counts of RANSAC hypothesis `it`'s models at a pixel threshold, as
    findEssentialMat scores them (the sample from cv::RNG's stream, the five-point
    models, the float Sampson distance against the float threshold)"""
    import oracle_ffi as O
    n = len(case.p1)
    sub = np.zeros(5 * 1000, np.int32)
    O.oracle().orc_ep_subsets(n, 1000, O.vp(sub))
    K = case.K
    q = [(np.asarray(p, np.float32).astype(np.float64) - [K[0, 2], K[1, 2]]) / [K[0, 0], K[1, 1]]
         for p in (case.p1, case.p2)]
    s = sub[5 * it:5 * it + 5]
    thr = threshold / ((K[0, 0] + K[1, 1]) / 2)
    thr2 = np.float32(thr * thr)
    counts = []
    for E in O.five_point(q[0][s], q[1][s]):
        e = np.ascontiguousarray(E.ravel())
        counts.append(sum(bool(np.float32(O.oracle().orc_sampson(O.vp(e), *q[0][i], *q[1][i])) <= thr2)
                          for i in range(n)))
    return counts


@functools.lru_cache(None)
def rel_ref(name):
    import oracle_ffi as O
    c = rel(name)
    ok, R, t, cm, rm, passed = O.estimate_transformation(c.p1, c.p2, c.K, c.ransac, c.prob, c.threshold, c.dist)
    _frozen(R, t, cm, rm)
    return RelRef(ok, R, t, cm, rm, passed)


@functools.lru_cache(None)
def pnp_ref(name):
    import oracle_ffi as O
    c = pnp(name)
    st, r, t, mask, ni = O.solve_pnp_ransac(c.X, c.uv, c.K, c.iters, c.reproj, c.conf)
    lm = O.pnp_last_lm() if st == 1 and len(c.X) > 5 else None
    _frozen(r, t, mask)
    return PnpRef(st, r, t, mask, ni, lm)


@functools.lru_cache(None)
def tri_ref(name):
    import oracle_ffi as O
    c = tri(name)
    out = O.reconstruct(c.K, c.R1, c.t1, c.R2, c.t2, c.p1, c.p2)
    _frozen(out)
    return out

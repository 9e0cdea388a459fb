"""The geometry kernels (csrc/essential.hip, csrc/pnp.hip, csrc/geom.hip) against
the oracle on the adversarial cases of tests/geom_cases.py: every chunk of the
relative-pose hypothesis launches, the five-point solver's degenerate branches
(no model, NaN models), the block edges, the option grid; pnp_reduce's seams in
the inlier count, the LM's rejection runs across the speculated dampings, planar
and duplicated object points; rank-deficient triangulations.

Bit-exact: every output is compared with assert_array_equal, NaN and inf
included.  tests/test_geom_cases.py proves on the CPU that each case has the
property it is named for; here the property is re-derived from the library's
own output where it can be (the chunk class from the library's RANSAC mask).
"""
import ctypes

import numpy as np
import pytest

import geom_cases as G
import slamhip
from slamhip import _lib as L

pytestmark = pytest.mark.gpu


# ---------------- relative pose ----------------
def _rel_abi(ctx, c):
    """slam_estimate_transformation as slamhip.estimateTransformation calls it, with the
    passed count the wrapper folds into ok: (R, t, chirality, ransac mask, passed)"""
    n = len(c.p1)
    R, t = np.zeros((3, 3)), np.zeros(3)
    cm, rm = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    passed = ctypes.c_int(-1)
    L.check(slamhip.lib().slam_estimate_transformation(
        ctx.handle, L.ptr(c.p1), L.ptr(c.p2), n, L.ptr(np.ascontiguousarray(c.K)), int(c.ransac), float(c.prob),
        float(c.threshold), float(c.dist), L.ptr(R), L.ptr(t), L.ptr(cm), L.ptr(rm), ctypes.byref(passed)), ctx.handle)
    return R, t, cm[:n], rm[:n], passed.value


def check_rel(ctx, name):
    c, ref = G.rel(name), G.rel_ref(name)
    ok, R, t, cm, rm = slamhip.estimateTransformation(c.p1, c.p2, c.K, c.ransac, c.prob, c.threshold, c.dist, ctx=ctx)
    assert ok == ref.ok
    np.testing.assert_array_equal(R, ref.R)
    np.testing.assert_array_equal(t, ref.t)
    np.testing.assert_array_equal(cm, ref.cmask)
    np.testing.assert_array_equal(rm, ref.rmask)
    R2, t2, cm2, rm2, passed = _rel_abi(ctx, c)
    assert passed == ref.passed
    for a, b in ((R2, R), (t2, t), (cm2, cm), (rm2, rm)):
        np.testing.assert_array_equal(a, b)
    # independent of the oracle
    assert set(np.unique(cm)) <= {0, 1} and set(np.unique(rm)) <= {0, 1}
    assert passed == int(cm.sum()) and ok == (passed > 0)
    if ok:
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12
        assert abs(np.linalg.det(R) - 1.0) <= 1e-12
        assert abs(np.linalg.norm(t) - 1.0) <= 1e-12
    # the hypotheses the library's own mask asks for fall in the chunk the case was built for
    if "chunk" in c.expect:
        assert G.chunk_of(G.rel_needed(c, rm)) == c.expect["chunk"]
    return ok, R, t, cm, rm


@pytest.mark.parametrize("name", G.REL_NAMES)
def test_relative_pose_cases(gpu_ctx, name):
    check_rel(gpu_ctx, name)


REL_STALE = ("chunk-600-22", "edge-8", "n5-solvable", "identical", "chunk-600-22")
PNP_STALE = ("sweep-769", "sweep-7", "n5", "planar-60", "sweep-769")


def test_relative_pose_stale_state():
    """the shared geom scratch only grows: a small, a five-point and a no-model call after the
    largest one read nothing it left behind, and the largest gives the same bits again"""
    ctx = slamhip.Context(0)
    try:
        outs = [check_rel(ctx, name) for name in REL_STALE]
    finally:
        ctx.close()
    assert outs[0][0] and outs[2][0] and not outs[3][0]
    for a, b in zip(outs[0], outs[-1]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("wide,chunk", G.REL_STALE_TRAPS)
def test_relative_pose_rewrites_every_count(wide, chunk):
    """the wide call leaves, in the slot of the chunk case's last needed hypothesis, a count
    above the chunk case's best (tests/test_geom_cases.py): the launch that ends there has to
    rewrite it"""
    ctx = slamhip.Context(0)
    try:
        check_rel(ctx, wide)
        check_rel(ctx, chunk)
    finally:
        ctx.close()


# ---------------- solvePnPRansac ----------------
def check_pnp(ctx, name):
    c, ref = G.pnp(name), G.pnp_ref(name)
    ok, rv, tv, inl = slamhip.solvePnPRansac(c.X, c.uv, c.K, None, iterationsCount=c.iters,
                                             reprojectionError=c.reproj, confidence=c.conf, ctx=ctx)
    assert ok == (ref.st == 1)
    np.testing.assert_array_equal(rv.ravel(), ref.rvec)
    np.testing.assert_array_equal(tv.ravel(), ref.tvec)
    if not ok:
        assert inl is None and not rv.any() and not tv.any()
        return ok, rv, tv, np.zeros(0, np.int32)
    np.testing.assert_array_equal(inl.ravel(), np.flatnonzero(ref.mask))
    # independent of the oracle
    i = inl.ravel()
    assert len(i) >= 5 and (np.diff(i) > 0).all() and i[0] >= 0 and i[-1] < len(c.X)
    if c.m is not None:
        assert len(i) == c.m and (i >= c.displaced).all()
    return ok, rv, tv, i


@pytest.mark.parametrize("name", G.PNP_NAMES)
def test_solve_pnp_ransac_cases(gpu_ctx, name):
    check_pnp(gpu_ctx, name)


def test_solve_pnp_ransac_stale_state():
    ctx = slamhip.Context(0)
    try:
        outs = [check_pnp(ctx, name) for name in PNP_STALE]
    finally:
        ctx.close()
    assert outs[0][0] and outs[2][0] and not outs[3][0]
    for a, b in zip(outs[0], outs[-1]):
        np.testing.assert_array_equal(a, b)


def test_solve_pnp_ransac_refuses_confidence_outside_0_1(gpu_ctx):
    c = G.pnp("n6")
    for conf in (0.0, 1.0, float("nan")):
        with pytest.raises(slamhip.SlamError):
            slamhip.solvePnPRansac(c.X, c.uv, c.K, confidence=conf, ctx=gpu_ctx)


@pytest.fixture(scope="module")
def pairwise_ctx():
    ctx = slamhip.Context(0)
    ctx.set_option(L.OPT_PNP_SUMS, L.PNP_SUMS_PAIRWISE)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", [f"sweep-{m}" for m in G.PNP_PAIRWISE_M] + list(G.PNP_PAIRWISE_LM))
def test_solve_pnp_ransac_pairwise_sums_cases(pairwise_ctx, name):
    """SLAM_PNP_SUMS_PAIRWISE on the seams of its strided per-thread sums (m around 8 and
    256) and across rejected LM steps: the contract of test_solve_pnp_ransac_pairwise_sums
    -- the same inlier mask, rvec / tvec within 1e-9 (relative to |t| for tvec), and the
    same value on a second run"""
    c, ref = G.pnp(name), G.pnp_ref(name)
    assert ref.st == 1
    kw = dict(iterationsCount=c.iters, reprojectionError=c.reproj, confidence=c.conf, ctx=pairwise_ctx)
    ok, rg, tg, inl = slamhip.solvePnPRansac(c.X, c.uv, c.K, None, **kw)
    assert ok
    np.testing.assert_array_equal(inl.ravel(), np.flatnonzero(ref.mask))
    assert np.abs(rg.ravel() - ref.rvec).max() <= 1e-9, (rg.ravel(), ref.rvec)
    assert np.abs(tg.ravel() - ref.tvec).max() <= 1e-9 * max(1.0, np.linalg.norm(ref.tvec)), (tg.ravel(), ref.tvec)
    ok2, rg2, tg2, inl2 = slamhip.solvePnPRansac(c.X, c.uv, c.K, None, **kw)
    assert ok2
    np.testing.assert_array_equal(rg2, rg)
    np.testing.assert_array_equal(tg2, tg)
    np.testing.assert_array_equal(inl2, inl)


# ---------------- triangulation ----------------
@pytest.mark.parametrize("name", G.TRI_NAMES)
def test_reconstruct_cases(gpu_ctx, name):
    c = G.tri(name)
    got = slamhip.reconstruct(c.K, c.R1, c.t1, c.R2, c.t2, c.p1, c.p2, ctx=gpu_ctx)
    assert got.shape == (len(c.p1), 3)
    np.testing.assert_array_equal(got, G.tri_ref(name))

"""The adversarial geometry fixtures (tests/geom_cases.py) proved on the CPU: this
tests the fixtures with the oracle alone, not the kernels.  Every property a case
was built for is an exact assertion here, so tests/test_geom_gpu.py can rely on it.
A case that stops meeting its condition is replaced, never loosened."""
import ctypes

import numpy as np
import pytest

import geom_cases as G
import oracle_ffi as O


def _norm(p, K):
    """pixels -> normalised coordinates as relative_pose / orc_find_essential compute them"""
    p = np.asarray(p, np.float32).astype(np.float64)
    return (p - [K[0, 2], K[1, 2]]) / [K[0, 0], K[1, 1]]


# ---------------- relative pose ----------------
@pytest.mark.parametrize("name", G.REL_NAMES)
def test_rel_case_verdict_and_chunk(name):
    c, r = G.rel(name), G.rel_ref(name)
    n = len(c.p1)
    assert len(c.p2) == n and c.p1.dtype == c.p2.dtype == np.float32
    e = c.expect
    assert r.ok == (r.passed > 0) and r.passed == int(r.cmask.sum())
    assert set(np.unique(r.cmask)) <= {0, 1} and set(np.unique(r.rmask)) <= {0, 1}
    if "ok" in e:
        assert r.ok == e["ok"]
    if "passed" in e:
        assert r.passed == e["passed"]
    if "rmask" in e:
        assert int(r.rmask.sum()) == e["rmask"]
    if "cmask" in e:
        assert int(r.cmask.sum()) == e["cmask"]
    assert bool(np.isnan(r.R).any() or np.isnan(r.t).any()) == bool(e.get("nan", False))
    if n > 5:
        needed = G.rel_needed(c, r.rmask)
        print(f"{name}: n {n} needed hypotheses {needed} ok {r.ok} passed {r.passed} ransac inliers {int(r.rmask.sum())}")
        if "needed" in e:
            assert needed == e["needed"]
        if "chunk" in e:
            assert G.chunk_of(needed) == e["chunk"]
        if c.klass.startswith("chunk:"):
            assert c.klass == "chunk:" + G.chunk_of(needed)
        # the oracle's own loop counter: RANSAC ran the needed hypotheses (more only where the
        # best model came later than that; never in a chunk case)
        if c.ransac:
            used = ctypes.c_int(-1)
            E, m = np.zeros(9), np.zeros(n, np.uint8)
            found = O.oracle().orc_find_essential(O.vp(c.p1), O.vp(c.p2), n, O.vp(c.K.ravel().copy()), c.prob,
                                                  c.threshold, O.vp(E), O.vp(m), ctypes.byref(used))
            if not found:
                assert used.value == 1000 and not r.rmask.any()
            else:
                np.testing.assert_array_equal(m, r.rmask)
                assert needed <= used.value <= 1000
                if c.klass.startswith("chunk:"):
                    assert used.value == needed


def test_rel_chunk_classes_all_present():
    seen = {G.chunk_of(G.rel_needed(G.rel(n), G.rel_ref(n).rmask)) for n in G.REL_NAMES if n.startswith("chunk-")}
    assert seen == set(G.CHUNKS)
    # one case ends exactly at the second launch's last hypothesis
    assert G.rel_needed(G.rel("chunk-300-28"), G.rel_ref("chunk-300-28").rmask) == 320


@pytest.mark.parametrize("wide,chunk", G.REL_STALE_TRAPS)
def test_rel_stale_trap(wide, chunk):
    """the wide call runs all 1000 hypotheses on the same points (same scratch layout), and
    what it counts for the chunk case's last needed hypothesis beats the chunk case's best"""
    w, c = G.rel(wide), G.rel(chunk)
    np.testing.assert_array_equal(w.p1, c.p1)
    np.testing.assert_array_equal(w.p2, c.p2)
    assert G.rel_needed(w, G.rel_ref(wide).rmask) == 1000
    needed, best = G.rel_needed(c, G.rel_ref(chunk).rmask), int(G.rel_ref(chunk).rmask.sum())
    own = G.rel_hypothesis_counts(c, needed - 1, c.threshold)
    stale = G.rel_hypothesis_counts(w, needed - 1, w.threshold)
    print(f"{chunk}: needed {needed} best {best}; hypothesis {needed - 1} counts {own} (own), {stale} (wide)")
    assert len(own) == len(stale) >= 1
    assert max(own) <= best < max(stale)


def test_five_point_minimal_sets():
    # five correspondences at the principal point: the elimination meets a zero pivot -> no model
    Es = O.five_point(_norm(G.ZERO5[0], G.K_INT), _norm(G.ZERO5[1], G.K_INT))
    assert len(Es) == 0
    np.testing.assert_array_equal(_norm(G.ZERO5[0], G.K_INT), np.zeros((5, 2)))
    # five collinear points shifted along their line: models are returned, every entry NaN
    Es = O.five_point(_norm(G.NAN5[0], G.K_REF), _norm(G.NAN5[1], G.K_REF))
    assert len(Es) == 10 and np.isnan(Es).all()
    # five times one correspondence (the "identical" case's every sample): NaN models too
    c = G.rel("identical")
    Es = O.five_point(_norm(c.p1[:5], c.K), _norm(c.p2[:5], c.K))
    assert len(Es) > 0 and np.isnan(Es).all()
    # a generic sample for contrast: finite models
    c = G.rel("n5-solvable")
    Es = O.five_point(_norm(c.p1, c.K), _norm(c.p2, c.K))
    assert 1 <= len(Es) <= 10 and np.isfinite(Es).all()


@pytest.mark.parametrize("n,seed", G.REL_FORWARD_WALL)
def test_forward_wall_first_sample_has_a_near_real_root(n, seed):
    """the first sample's polynomial has a root the solver's |im| <= 1e-10 rule drops by less
    than a factor of 10; the getter changes nothing"""
    c = G.rel(f"forward_wall-{n}-{seed}")
    sub = np.arange(5, dtype=np.int32)
    if n > 5:
        O.oracle().orc_ep_subsets(n, 1, O.vp(sub))
    q1, q2 = _norm(c.p1[sub], c.K), _norm(c.p2[sub], c.K)
    Es = O.five_point(q1, q2)
    roots = O.five_point_last_roots()
    np.testing.assert_array_equal(roots, O.five_point_last_roots())
    np.testing.assert_array_equal(O.five_point(q1, q2), Es)
    near = [z for z in roots if G.IM_RULE < abs(z.imag) <= 10 * G.IM_RULE]
    print(f"forward_wall-{n}-{seed}: degree {len(roots)} models {len(Es)} near-real roots {near}")
    assert 1 <= len(roots) <= 10 and len(near) >= 1
    assert len(Es) == sum(abs(z.imag) <= G.IM_RULE for z in roots)      # no root lost to the |xy1[2]| rule here
    # a solver that returns before the root finder reports no roots
    assert len(O.five_point(_norm(G.ZERO5[0], G.K_INT), _norm(G.ZERO5[1], G.K_INT))) == 0
    assert len(O.five_point_last_roots()) == 0


def _hypothesis_stats(c, count):
    """(degree, models, roots within the |im| rule) of the first `count` RANSAC samples"""
    n = len(c.p1)
    sub = np.zeros(5 * 1000, np.int32)
    O.oracle().orc_ep_subsets(n, 1000, O.vp(sub))
    q1, q2 = _norm(c.p1, c.K), _norm(c.p2, c.K)
    out = []
    for it in range(count):
        s = sub[5 * it:5 * it + 5]
        nm = len(O.five_point(q1[s], q2[s]))
        roots = O.five_point_last_roots()
        out.append((len(roots), nm, int(sum(abs(z.imag) <= G.IM_RULE for z in roots))))
    return out


def test_degree_drop_and_skipped_roots_are_replayed():
    """the branches behind `while (cdet[n] == 0) n--` (another root-finder instantiation) and
    `|xy1[2]| < 1e-10` (a real root without a model) in samples whose counts RANSAC reads"""
    # all zeros: the first sample, which decides the case, has degree 9 and loses real roots
    deg, nm, real = _hypothesis_stats(G.rel("zeros"), 1)[0]
    assert deg == 9 and 0 < nm < real
    # static camera with clutter: RANSAC reads every sample up to the needed count
    c = G.rel("same_points-clutter")
    needed = G.rel_needed(c, G.rel_ref(c.name).rmask)
    stats = _hypothesis_stats(c, needed)
    degrees = sorted({s[0] for s in stats})
    print(f"same_points-clutter: needed {needed}, degrees {degrees}, "
          f"samples with a skipped real root {sum(s[1] < s[2] for s in stats)}")
    assert needed > 64 and degrees == [9, 10]
    assert any(s[0] < 10 and s[1] > 0 for s in stats)


def test_six_point_first_sample_is_the_nan_set():
    sub = np.zeros(5, np.int32)
    O.oracle().orc_ep_subsets(6, 1, O.vp(sub))
    assert tuple(sub) == G.FIRST_SUBSET_OF_6
    c = G.rel("six-nan_first")
    np.testing.assert_array_equal(c.p1[sub], G.NAN5[0].astype(np.float32))
    np.testing.assert_array_equal(c.p2[sub], G.NAN5[1].astype(np.float32))
    Es = O.five_point(_norm(c.p1[sub], c.K), _norm(c.p2[sub], c.K))
    assert len(Es) == 10 and np.isnan(Es).all()
    assert G.rel_ref("six-nan_first").ok          # a later sample still finds the model


def test_rel_param_grid_reaches_the_clamps():
    """prob = 1 is clamped to log(DBL_MIN): the count never drops below 1000; the 5-unit distance
    threshold cuts points the 200-unit one keeps; the thresholds give three different masks"""
    for thr in G.REL_THRESHOLDS:
        for dist in G.REL_DISTS:
            c = G.rel(f"param-1.0-{thr}-{dist}")
            assert G.rel_needed(c, G.rel_ref(c.name).rmask) == 1000
        near, far = G.rel_ref(f"param-0.999-{thr}-5.0"), G.rel_ref(f"param-0.999-{thr}-200.0")
        np.testing.assert_array_equal(near.rmask, far.rmask)
        np.testing.assert_array_equal(near.R, far.R)
        assert 0 < near.passed < far.passed
    sums = {int(G.rel_ref(f"param-0.999-{thr}-200.0").rmask.sum()) for thr in G.REL_THRESHOLDS}
    assert len(sums) == 3
    needed = {G.rel_needed(G.rel(n), G.rel_ref(n).rmask) for n in G.REL_NAMES if n.startswith("param-0.5-")}
    assert max(needed) <= 320 and min(needed) <= 64       # prob 0.5 stops early


# ---------------- solvePnPRansac ----------------
@pytest.mark.parametrize("m", G.PNP_SWEEP_M)
def test_pnp_sweep_inlier_count(m):
    c, r = G.pnp(f"sweep-{m}"), G.pnp_ref(f"sweep-{m}")
    assert c.m == m and len(c.X) == m + c.displaced
    assert r.st == 1 and r.ninliers == m == int(r.mask.sum())
    assert not r.mask[:c.displaced].any() and r.mask[c.displaced:].all()


@pytest.mark.parametrize("name", [n for n in G.PNP_NAMES if n.startswith("lm-")])
def test_pnp_lm_run_length(name):
    c, r = G.pnp(name), G.pnp_ref(name)
    assert r.st == 1 and r.lm is not None
    print(f"{name}: inliers {r.ninliers} {r.lm}")
    assert r.lm.longest_run == c.lm_run
    assert r.lm.rejected >= r.lm.longest_run and 1 <= r.lm.iterations <= 20
    assert r.lm.max_lambda_lg10 <= 16                # no case reaches the cap (none was found)


def test_pnp_lm_getter_is_read_only_and_fresh():
    """the getter reports the last refinement and changes nothing: the same call gives the
    same bits before and after reading it, and a refinement without rejections resets it"""
    c = G.pnp("lm-run7-40-1002")
    a = O.solve_pnp_ransac(c.X, c.uv, c.K, c.iters, c.reproj, c.conf)
    s1 = O.pnp_last_lm()
    assert s1 == O.pnp_last_lm()
    b = O.solve_pnp_ransac(c.X, c.uv, c.K, c.iters, c.reproj, c.conf)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    assert O.pnp_last_lm() == s1 and s1.longest_run == 7 and s1.rejected == 7
    # orc_pnp_iterative alone: its return value is the iteration count the getter reports
    from test_oracle import pnp_scene
    K, rv, t, X, uv, _ = pnp_scene(300, 9, noise=0.0, outliers=0.0)
    r, tt, it = O.pnp_iterative(X, uv.astype(np.float64), K, rv + 0.02, t - 0.05)
    s2 = O.pnp_last_lm()
    assert s2.iterations == it and s2.rejected == s2.longest_run == 0 and s2.max_lambda_lg10 == -3


@pytest.mark.parametrize("name", [n for n in G.PNP_NAMES if not n.startswith(("sweep-", "lm-"))])
def test_pnp_misc_case(name):
    c, r = G.pnp(name), G.pnp_ref(name)
    assert r.ninliers == int(r.mask.sum())
    if c.st is not None:
        assert r.st == c.st
    if c.m is not None:
        assert r.ninliers == c.m
    if r.st == 0:
        assert r.ninliers == 0 and not r.rvec.any() and not r.tvec.any()
    if c.klass.startswith("planar:"):
        assert r.st == 0                              # a wall: EPnP RANSAC finds no model
        assert not c.X[:, 2].any() and np.ptp(c.X[:, 0]) > 1 and np.ptp(c.X[:, 1]) > 1
    if c.klass == "duplicates":
        assert len(np.unique(c.X, axis=0)) < len(c.X)


# ---------------- triangulation ----------------
def test_tri_cases_are_what_they_claim():
    for name in G.TRI_NAMES:
        c = G.tri(name)
        assert len(c.p1) == len(c.p2) == len(G.tri_ref(name))
    np.testing.assert_array_equal(G.tri("same_pixel").p1, G.tri("same_pixel").p2)
    c = G.tri("parallel_rays")
    np.testing.assert_array_equal(c.p1, c.p2)
    np.testing.assert_array_equal(c.R1, c.R2)
    assert np.abs(G.tri_ref("parallel_rays")).min(axis=1).max() > 1e6     # the points at "infinity"
    a, b = G.tri("swapped_views"), G.tri("same_pixel")
    np.testing.assert_array_equal(a.p2, b.p1)
    assert (G.tri_ref("behind_cameras")[:, 2] < 0).all()
    c = G.tri("behind_cameras")
    assert ((G.tri_ref("behind_cameras") @ c.R2.T + c.t2)[:, 2] < 0).all()
    c = G.tri("on_baseline")                          # all three project to one pixel pair: the epipoles
    assert np.abs(c.p1 - c.p1[0]).max() < 0.01 and np.abs(c.p2 - c.p2[0]).max() < 0.01
    assert [len(G.tri(f"n-{n}").p1) for n in G.TRI_N] == list(G.TRI_N)


# ---------------- the registry covers the issue's list ----------------
def test_registry_covers_the_issue_list():
    for names in (G.REL_NAMES, G.PNP_NAMES, G.TRI_NAMES):
        assert len(set(names)) == len(names)
    rel = {G.rel(n).klass for n in G.REL_NAMES}
    assert {"chunk:" + k for k in G.CHUNKS} <= rel
    assert {"degenerate:" + k for k in ("identical", "p1_eq_p2", "pure_rotation", "planar", "planar_no_ransac",
                                        "collinear", "grid", "grid_shifted", "zeros", "noise",
                                        "six_nan_first")} <= rel
    assert {"n5:solvable", "n5:identical", "n:0", "n:4"} <= rel
    # beyond the issue's list: NaN models at n == 5, near-real roots, degree drops, the stale-count traps
    assert {"n5:nan_models", "five_point:near_real_root", "degenerate:p1_eq_p2_clutter", "stale:wide"} <= rel
    assert {f"edge:{n}" for n in (6, 7, 8, 127, 128, 129, 255, 256, 257)} <= rel
    grid = {(c.prob, c.threshold, c.dist) for c in map(G.rel, G.REL_NAMES) if c.klass == "param"}
    assert grid == {(p, t, d) for p in (0.5, 0.999, 1.0) for t in (0.5, 5.0, 50.0) for d in (5.0, 200.0)}
    assert [c.klass for c in map(G.rel, G.REL_NAMES) if not c.ransac] == ["degenerate:planar_no_ransac"]
    pnp = {G.pnp(n).klass for n in G.PNP_NAMES}
    assert {f"sweep:{m}" for m in (6, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 255, 256, 257, 263, 264, 265, 271,
                                   272, 511, 512, 513, 520, 769)} <= pnp
    runs = {G.pnp(n).lm_run for n in G.PNP_NAMES if n.startswith("lm-")}
    assert {1, 2, 3, 4} <= runs and max(runs) >= 7
    assert {"planar:60", "planar:200", "duplicates", "n:5", "n:6", "option:iterations1", "option:confidence0.5",
            "option:confidence0.999999"} <= pnp
    assert set(G.PNP_PAIRWISE_M) == {7, 8, 9, 256, 257, 513} and set(G.PNP_PAIRWISE_M) <= set(G.PNP_SWEEP_M)
    assert len(G.PNP_PAIRWISE_LM) == 2 and set(G.PNP_PAIRWISE_LM) <= set(G.PNP_NAMES)
    tri = {G.tri(n).klass for n in G.TRI_NAMES}
    assert {"same_pixel", "swapped_views", "on_baseline", "n:1", "n:255", "n:256", "n:257"} <= tri
    # the stated size limit: a few hundred points, but for the 769-inlier case
    assert max(len(G.rel(n).p1) for n in G.REL_NAMES) <= 600
    assert sorted(len(G.pnp(n).X) for n in G.PNP_NAMES)[-2:] == [560, 809]

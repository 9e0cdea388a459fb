"""The adversarial BA windows are what they claim, and the reference side is
sound (CPU only): ba_cases.structure restates ba_solve's host bookkeeping,
oracle/ba.c ends every case cleanly, and its one-iteration result sits within
a derived distance of the dense extended-precision step of ba_dense_ref.py.
"""
import numpy as np
import pytest

import ba_cases as C
import ba_checks as B
import ba_dense_ref as D

CASES = C.cases()
NAMES = list(CASES)
DENSE = [n for n in NAMES if CASES[n]["dense"] and len(CASES[n]["obs_frame"])]

# The oracle against the dense step, relative to the step's size.  The damped,
# Jacobi-scaled normal matrix has diagonal entries in [1e-6 / radius, 1 + 1 /
# radius] (radius 1e4), so its condition number is far below 1e12 and a
# float64 solve loses at most ~12 of its 16 digits: 1e-4 bounds rounding from
# above.  The windows' real conditioning is ~1e7 (measured distances 1e-12 ..
# 5e-8), and a formula error in either side shows at 1e-3 or more:
# 1e-6 separates the two with two decades to spare on each side.
STEP_BOUND = {"K": 1e-6, "ext": 1e-6, "pts": 1e-6, "cost": 1e-6}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_the_issue_list_is_covered():
    need = [f"nf{n:02d}" for n in (1, 2, 3, 11, 12, 17, 21, 22, 23, 24)]
    need += ["hash", "hash_shuffled", "per_n1", "per_n3", "per_n5", "gram_32_33", "unobserved_points",
             "unobserved_frames", "same_frame_twice", "obs64", "obs65", "no_obs", "zero_rotation", "near_pi",
             "behind_camera", "z_zero", "nan_observation", "inf_point", "tukey_all_outside", "huber_all_outside",
             "zero_residual", "huber_at_threshold", "ground_truth_start", "converges_at_3", "converges_at_4",
             "converges_at_12", "converges_at_14"]
    need += [f"outliers_loss{k}" for k in range(6)] + [f"max_iters{k}" for k in (1, 2, 3, 4, 5)]
    assert sorted(need) == sorted(NAMES)
    decisive = {n for n in NAMES if CASES[n]["decisive"]}
    assert decisive >= {"nf01", "z_zero", "tukey_all_outside", "huber_all_outside", "ground_truth_start",
                        "converges_at_4", "converges_at_14"} | {f"max_iters{k}" for k in (1, 2, 3, 4, 5)}


@pytest.mark.parametrize("name", NAMES)
def test_case_has_its_stated_property(name):
    w = CASES[name]
    st = C.structure(w)
    assert w["expect"], "a case without a stated property"
    for k, v in w["expect"].items():
        assert st[k] == v, (name, k, st[k], v)
    assert st["kernel"] == C.solve_kernel(st["nc"])
    assert w["obs_frame"].dtype == np.int32 and w["obs_point"].dtype == np.int32
    if st["no"]:
        assert 0 <= w["obs_frame"].min() and w["obs_frame"].max() < st["nf"]
        assert 0 <= w["obs_point"].min() and w["obs_point"].max() < st["np"]
    if w["dense"]:
        assert st["N"] <= 500


def test_structure_facts_the_cases_rely_on():
    s = {n: C.structure(w) for n, w in CASES.items()}
    # every solve kernel of ba_solve's dispatch is reached, the exact fits included
    assert {s[n]["kernel"] for n in NAMES} == {"lane<16>", "lane<28>", "lane<48>", "lane<64>", "rows<96,2>",
                                              "rows<128,2>", "lds<1024,10>", "refused"}
    assert s["nf11"]["nc"] == 64 and s["nf23"]["nc"] == C.K_MAX_NC and s["nf22"]["nc"] == 130
    assert s["nf01"]["nc"] == 4 and s["nf01"]["unobserved_frames"] == []
    # the hash window: more than 512 distinct tuples, nearly all of them no
    # consecutive track, many descending; the shuffled one differs in its tuples
    assert s["hash"]["tuples"] > 512 and s["hash"]["hashed_tuples"] > 500 and s["hash"]["descending_tuples"] > 400
    assert s["hash_shuffled"]["tuples"] > 512 and s["hash_shuffled"]["regrows"] == 1
    # make_window's shape never regrows the table nor leaves a block unobserved
    from slamhip import synthba
    m = dict(synthba.make_window(20, 300, seed=20), loss_param=0.0)
    sm = C.structure(m)
    assert sm["regrows"] == 0 and sm["hashed_tuples"] == 0 and sm["unobserved_frames"] == []
    # the 64-observation point fills one chunk alone; 65 is one too many
    assert (64, 1) in s["obs64"]["chunks"] and s["obs65"]["max_point_obs"] == C.K_CHUNK + 1
    assert (0, 3) in s["unobserved_points"]["chunks"]           # the nobs = 0 chunk
    assert s["zero_residual"]["zero_residuals"] == 1 and s["huber_at_threshold"]["sq_equal_a2"] == 1
    assert s["tukey_all_outside"]["beyond_a"] == s["tukey_all_outside"]["no"]
    assert s["zero_rotation"]["free_small_angle"] == 5 and s["nf12"]["free_small_angle"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_oracle_ends_each_case_cleanly(name):
    w = CASES[name]
    runs = B.oracle_runs(w)
    ints = {B.ints(r[3]) for r in runs}
    finite_in = np.isfinite(w["K4"]).all() and np.isfinite(w["ext"]).all() and np.isfinite(w["pts"]).all()
    m = B.untouched(w, runs)
    st = C.structure(w)
    for K, E, P, sm in runs:
        assert sm.termination in (0, 1, 2, 3) and 0 <= sm.iterations <= w["max_iters"]
        if sm.termination == 3:
            assert sm.usable == 0 and same_bits(K, w["K4"]) and same_bits(E, w["ext"]) and same_bits(P, w["pts"])
        elif finite_in:
            assert np.isfinite(K).all() and np.isfinite(E).all() and np.isfinite(P).all()
            assert np.isfinite(sm.final_cost) and sm.final_cost <= sm.initial_cost
    # unobserved blocks (and the constant frame 0) come back bit-identical
    assert m["ext"][:6].all()
    for f in st["unobserved_frames"]:
        assert m["ext"][6 * f:6 * f + 6].all()
    for p in st["unobserved_points"]:
        assert m["pts"][3 * p:3 * p + 3].all()
    if w["decisive"]:
        assert len(ints) == 1, (name, sorted(ints))
        if w["summary"] is not None:
            assert ints == {tuple(w["summary"])}


@pytest.mark.parametrize("name", DENSE)
def test_oracle_one_step_near_dense_step(name):
    w = CASES[name]
    K, E, P, cost, info = B.dense(w)
    runs = B.oracle_runs(w, 1)
    ints = {B.ints(r[3]) for r in runs}
    assert len(ints) == 1, (name, sorted(ints))
    it, succ, term, usable = next(iter(ints))
    c0 = float(D.cost_at(w, w["loss"], w["loss_param"], info["x0"]))
    # (absolute term: a float64 residual carries a few ulp of the pixel coordinate, which is all
    # there is of the cost at the ground-truth start)
    ulp = 4 * np.finfo(np.float64).eps * max(1.0, float(np.abs(w["obs_xy"]).max()))
    assert abs(runs[0][3].initial_cost - c0) <= 1e-12 * c0 + len(w["obs_xy"]) * ulp * ulp
    start = (w["K4"], w["ext"], w["pts"])
    if it == 0:
        # the gradient exit before the first iteration: the dense gradient agrees
        assert term == 1 and float(np.abs(info["grad"]).max()) <= 1e-10
    elif succ == 0:
        # a rejected step: the dense candidate is no improvement either
        assert cost > c0
    if succ == 0:
        for r in runs:
            assert all(same_bits(a, b) for a, b in zip(r[:3], start))
        return
    dmax, _ = B.oracle_distances(w, (K, E, P), 1)
    dmax["cost"] = max(abs(r[3].final_cost - cost) for r in runs) / cost
    print("BA_ORACLE_VS_DENSE", name, " ".join(f"{k} {v:.2e}" for k, v in dmax.items()))
    for k, v in dmax.items():
        assert v <= STEP_BOUND[k], (name, k, v)


def test_paths_that_differ_are_the_recorded_ones():
    differ = {(n, k) for n in NAMES for k in (2, 3)
              if CASES[n]["refused"] is None and CASES[n]["max_iters"] >= 3 and not B.same_path(CASES[n], k)}
    assert differ == set(C.PATHS_DIFFER)


def test_dense_reference_pieces():
    # the Cholesky against numpy on a random SPD system, in extended precision
    rng = np.random.default_rng(1)
    M = rng.normal(size=(40, 30))
    A = (M.T @ M + 0.1 * np.eye(30)).astype(np.longdouble)
    b = rng.normal(size=30).astype(np.longdouble)
    y = D.cholesky_solve(A, b)
    assert float(np.abs(A @ y - b).max()) < 1e-15
    assert np.isnan(D.cholesky_solve(-A, b)).any()
    # rho, rho', rho'' are consistent: complex-step derivatives of rho and rho'
    s = np.array([0.3, 2.0, 24.0, 26.0, 900.0], np.longdouble)
    h = np.longdouble("1e-40")
    for loss, a in ((C.LOSS_HUBER, 5.0), (C.LOSS_CAUCHY, 2.0), (C.LOSS_ARCTAN, 4.0), (C.LOSS_TUKEY, 6.0)):
        r0, r1, r2 = D.rho(loss, a, s)
        e = np.longdouble("1e-6")
        n1 = (D.rho(loss, a, s + e)[0] - D.rho(loss, a, s - e)[0]) / (2 * e)
        n2 = (D.rho(loss, a, s + e)[1] - D.rho(loss, a, s - e)[1]) / (2 * e)
        assert float(np.abs(n1 - r1).max()) < 1e-9 and float(np.abs(n2 - r2).max()) < 1e-9, loss
    # the complex-step Jacobian against central differences of the residuals
    w = CASES["near_pi"]
    info = B.dense(w)[4]
    x0 = info["x0"]
    i = 4 + 6 * 1 + 2                                   # frame 2's third rotation component
    xp, xm = x0.copy(), x0.copy()
    e = np.longdouble("1e-7")
    xp[i] += e
    xm[i] -= e
    num = float((D.cost_at(w, 0, 0.0, xp) - D.cost_at(w, 0, 0.0, xm)) / (2 * e))
    assert abs(num - float(info["grad"][i])) <= 1e-7 * abs(num)

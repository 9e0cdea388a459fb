"""Checks shared by the CPU tests (tests/test_gba.py) and the GPU tests (tests/test_gba_gpu.py) of global bundle
adjustment: a named case against the reference by bits, every refusal, and the synthetic world, each written once
against a callable so that the host path and the device path run the same assertions.
"""
import functools

import numpy as np
import pytest

import gba_ref as R
from loop_checks import MIN_PAIRS, TAU
from slamhip import _lib as L
from slamhip import globalba as G
from slamhip import loopclose as LC

WORLD_K = np.array([[300.0, 0.0, 320.0], [0.0, 300.0, 240.0], [0.0, 0.0, 1.0]])      # loop_ref.world_case's camera

# Measured with the reference (tests/gba_ref.py) on the closed world, DESIGN section 25: reprojection RMS over the
# kept observations 4.859 px -> 9.51e-6 px, similarity-aligned RMS centre error 7.63e-2 -> 9.43e-8.  The twin and
# the device equal the reference by bits, so the factor 2 is only slack against later edits of the fixture.
WORLD_RMS = (4.859, 9.51e-6)
WORLD_CENTRE = (7.63e-2, 9.43e-8)


def check_case(name, run):
    """run(K4, cams, points, obs_cam, obs_point, obs_xy, **kw) -> (cams, points, summary) on a named case"""
    W, kw = R.gba_cases()[name]
    C, X, s, _ = R.gba_expected(name)
    c, p, s2 = run(W["K"], W["cams"], W["points"], W["obs_cam"], W["obs_point"], W["obs_xy"], **kw)
    assert s2 == s, (name, s2, s)
    assert R.same_bits(c, C), (name, "cameras", np.abs(np.asarray(c) - C).max() if len(C) else 0)
    assert R.same_bits(p, X), (name, "points", np.abs(np.asarray(p) - X).max() if len(X) else 0)
    assert list(s2) == list(R.SUMMARY)


def gba_refusals(run):
    """every bad argument through run(K4, cams, points, obs_cam, obs_point, obs_xy, **kw); returns their number"""
    W, _ = R.gba_cases()["lists"]
    K, C, X, oc, op, xy = W["K"], W["cams"], W["points"], W["obs_cam"], W["obs_point"], W["obs_xy"]
    n, m = len(C), len(X)
    count = []

    def expect(*args, **kw):
        with pytest.raises(L.SlamError) as x:
            run(*args, **kw)
        assert x.value.code == L.SLAM_E_INVALID_ARG
        count.append(1)

    run(K, C, X, oc, op, xy, max_lm=1, max_pcg=2)
    for v in (n, -1):                                          # an index out of range
        o2 = oc.copy()
        o2[3] = v
        expect(K, C, X, o2, op, xy)
    for v in (m, -1):
        o2 = op.copy()
        o2[5] = v
        expect(K, C, X, oc, o2, xy)
    C2 = C.copy()
    C2[2, :4] = 0.0                                            # a zero quaternion
    expect(K, C2, X, oc, op, xy)
    for k, v in ((0, 0.0), (1, -1.0), (0, float("nan"))):      # fx or fy <= 0
        K2 = list(K)
        K2[k] = v
        expect(K2, C, X, oc, op, xy)
    for v in (0.0, -1.0):
        expect(K, C, X, oc, op, xy, zmin=v)
    for key in ("max_lm", "max_pcg", "pcg_tol", "cost_tol", "lambda0"):      # a negative cap or tolerance
        expect(K, C, X, oc, op, xy, **{key: -1})
    for v in (2, -1):                                          # an unknown loss
        expect(K, C, X, oc, op, xy, loss=v)
    for v in (0.0, -1.0):                                      # Huber with a <= 0
        expect(K, C, X, oc, op, xy, loss=1, loss_param=v)
    for v in (float("nan"), float("inf")):                     # a pixel that is not finite
        x2 = xy.copy()
        x2[7, 1] = v
        expect(K, C, X, oc, op, x2)
    return len(count)


REFUSALS = 21


def _centres(rot, mot):
    return np.array([-r.T @ m for r, m in zip(rot, mot)])


def aligned_rms(c, gt):
    """RMS distance of the centres c to gt after the best similarity (Umeyama)"""
    A, B = c - c.mean(0), gt - gt.mean(0)
    U, S, Vt = np.linalg.svd(B.T @ A)
    D = np.diag([1.0, 1.0, float(np.sign(np.linalg.det(U @ Vt)))])
    s = float((S * np.diag(D)).sum() / (A ** 2).sum())
    return float(np.sqrt((((s * (U @ D @ Vt @ A.T)).T - B) ** 2).sum(1).mean()))


@functools.lru_cache(maxsize=None)
def closed_world(wrong=False):
    """(world, close_loops' result on the host, the observations merged onto the closed cloud)"""
    W = R.world_case(wrong=wrong)
    closed = LC.close_loops(W["rotations"], W["motions"], W["points"], W["colors"], W["obs"], W["loops"], tau=TAU,
                            min_pairs=MIN_PAIRS, host=True)
    obs2 = G.merge_observations(W["obs"], len(W["points"]), closed["constraints"], closed["dropped"])
    return W, closed, obs2


def check_world(ba):
    """the world through ba(K, rotations, motions, points, obs) -> (rotations, motions, points, summary)"""
    W, closed, obs2 = closed_world()
    rot, mot, pts, s = ba(WORLD_K, closed["rotations"], closed["motions"], closed["points"], obs2)
    rms0, rms1 = float(np.sqrt(s["cost0"] / s["kept_obs"])), float(np.sqrt(s["cost"] / s["kept_obs"]))
    e0 = aligned_rms(_centres(closed["rotations"], closed["motions"]), W["gt_centres"])
    e1 = aligned_rms(_centres(np.asarray(rot), np.asarray(mot)), W["gt_centres"])
    print(f"reprojection rms over {s['kept_obs']} kept observations {rms0:.4f} -> {rms1:.3e} px, aligned rms centre {e0:.4e} -> {e1:.3e}, "
          f"summary {s}")
    assert rms1 < rms0 and e1 < e0
    assert WORLD_RMS[0] / 2 <= rms0 <= WORLD_RMS[0] * 2 and rms1 <= WORLD_RMS[1] * 2
    assert WORLD_CENTRE[0] / 2 <= e0 <= WORLD_CENTRE[0] * 2 and e1 <= WORLD_CENTRE[1] * 2
    # the held points (fewer than two observations) keep their bits, and no other point does
    oc, op, _ = G.flatten_observations(obs2, len(closed["points"]))
    held = np.bincount(op, minlength=len(closed["points"])) < 2
    same = (np.asarray(pts) == closed["points"]).all(1)
    assert int(held.sum()) == s["points_held"] and np.array_equal(same, held)
    assert R.same_bits(np.asarray(rot)[0], closed["rotations"][0]) and R.same_bits(np.asarray(mot)[0], closed["motions"][0])
    return rot, mot, pts, s

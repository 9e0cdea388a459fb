"""Checks shared by the CPU tests (tests/test_loop.py) and the GPU tests (tests/test_loop_gpu.py) of loop
closing: every refusal of the library calls, and the checks of the synthetic world, each written once
against a callable so that the host path and the device path run the same assertions.
"""
import numpy as np
import pytest

import loop_ref as R
from slamhip import _lib as L
from slamhip import loopclose as LC


def pgo_refusals(run):
    """every bad argument of the optimiser through run(nodes, edges, meas, weight, ell, **kw)"""
    S, e, m, w, ell, _ = R.pgo_cases()["three"]
    count = []

    def expect(*args, **kw):
        with pytest.raises(L.SlamError) as x:
            run(*args, **kw)
        assert x.value.code == L.SLAM_E_INVALID_ARG
        count.append(1)

    run(S, e, m, w, ell, max_lm=1, max_pcg=2)
    for bad in ([1, 1], [0, 3], [-1, 2], [3, 0]):                     # i == j, an index outside [0, n)
        e2 = e.copy()
        e2[1] = bad
        expect(S, e2, m, w, ell)
    for v in (0.0, -2.0, float("nan")):                              # a non-positive sigma or ell
        S2, m2 = S.copy(), m.copy()
        S2[2, 0] = v
        m2[0, 0] = v
        expect(S2, e, m, w, ell)
        expect(S, e, m2, w, ell)
        expect(S, e, m, w, v)
    S2, m2 = S.copy(), m.copy()
    S2[1, 1:5] = 0.0                                                  # a zero quaternion
    m2[2, 1:5] = 0.0
    expect(S2, e, m, w, ell)
    expect(S, e, m2, w, ell)
    expect(np.concatenate([S, S[:1]]), e, m, w, ell)                  # node 3 has no edge
    expect(S, e[:1], m[:1], w[:1], ell)                               # node 2 has no edge
    w2 = w.copy()
    w2[0] = -1.0
    expect(S, e, m, w2, ell)
    expect(S, e, m, w, ell, max_lm=-1)
    expect(S, e, m, w, ell, max_pcg=-1)
    expect(S, e, m, w, ell, lambda0=-1.0)
    return len(count)


TAU, MIN_PAIRS = 0.01, 30      # true pairings 135 / 133 inliers of 207 / 182 pairs, wrong pairing 0


def _centres(rot, mot):
    return np.array([-r.T @ m for r, m in zip(rot, mot)])


def _rms(a, b):
    return float(np.sqrt(((a - b) ** 2).sum(1).mean()))


def check_world(run):
    """the checks of the synthetic world through run(world) -> close_loops' result; returns the result"""
    W = R.world_case()
    res = run(W)
    cons = res["constraints"]
    assert [(c["i"], c["j"]) for c in cons] == [(39, 0), (38, 0)] and all(c["accepted"] for c in cons)
    e0 = _rms(_centres(W["rotations"], W["motions"]), W["gt_centres"])
    e1 = _rms(_centres(res["rotations"], res["motions"]), W["gt_centres"])
    # the two copies of the duplicated points, before (open map) and after (moved, before merging)
    nodes = LC.nodes_from_poses(W["rotations"], W["motions"])
    moved = LC.apply_points(W["points"], LC.anchors_of(W["obs"], len(W["points"])), nodes, res["nodes"], host=True)
    d = W["dup"]
    g0 = float(np.linalg.norm(W["points"][d[:, 0]] - W["points"][d[:, 1]], axis=1).mean())
    g1 = float(np.linalg.norm(moved[d[:, 0]] - moved[d[:, 1]], axis=1).mean())
    print(f"rms centre {e0:.4f} -> {e1:.4f}, duplicate gap {g0:.4f} -> {g1:.4f}, inliers {[c['count'] for c in cons]} of "
          f"{[len(c['ia']) for c in cons]}, dropped {len(res['dropped'])}, costs {res['costs']}, iters {res['iters']}")
    assert e1 < e0 and g1 < g0
    # exactly the duplicates that the inlier masks name are dropped: the higher index of every inlier pair
    named = set()
    for c in cons:
        named |= {int(max(a, b)) for a, b in zip(c["ia"][c["mask"]], c["ib"][c["mask"]])}
    assert set(res["dropped"].tolist()) == named and len(named) > 0
    assert len(res["points"]) == len(W["points"]) - len(named) == len(res["colors"])
    keep = np.setdiff1d(np.arange(len(W["points"])), res["dropped"])
    assert np.array_equal(res["colors"], W["colors"][keep]) and R.same_bits(res["points"], moved[keep])
    assert {tuple(sorted(p)) for c in cons for p in zip(c["ia"][c["mask"]].tolist(), c["ib"][c["mask"]].tolist())} \
        <= {tuple(sorted(p)) for p in d.tolist()}
    return res


def check_wrong_world(run):
    W = R.world_case(wrong=True)
    res = run(W)
    assert len(res["constraints"]) == 1 and not res["constraints"][0]["accepted"]
    print("wrong pairing:", res["constraints"][0]["count"], "inliers of", len(res["constraints"][0]["ia"]), "status",
          res["constraints"][0]["status"])
    for k in ("rotations", "motions", "points", "colors"):
        assert R.same_bits(res[k], np.asarray(W[k], res[k].dtype)), k
    assert len(res["dropped"]) == 0


def refusals(ransac, apply):
    """every bad argument of the two calls, through ransac(a, b, off, c, H, tau) and
    apply(pts, anchor, nodes, new): each must raise SlamError(SLAM_E_INVALID_ARG)"""
    a, b, off, c = R.batch_case([5, 6])
    pts, anchor, nodes, new = R.apply_case(8)
    bad = []

    def expect(fn, *args):
        with pytest.raises(L.SlamError) as e:
            fn(*args)
        assert e.value.code == L.SLAM_E_INVALID_ARG
        bad.append(1)

    expect(ransac, a, b, np.array([0, 7, 5], np.int32), c, 8, R.TAU)          # descending offsets
    expect(ransac, a, b, off, c, 0, R.TAU)                                    # H < 1
    expect(ransac, a, b, off, c, -3, R.TAU)
    expect(ransac, a, b, off, c, 65537, R.TAU)
    expect(ransac, a, b, off, c, 8, 0.0)                                      # tau
    expect(ransac, a, b, off, c, 8, float("nan"))
    for k, v in ((0, 0.0), (0, -1.0), (0, float("nan"))):                    # a non-positive sigma
        n2 = new.copy()
        n2[3, k] = v
        expect(apply, pts, anchor, nodes, n2)
        expect(apply, pts, anchor, n2, new)
    n2 = new.copy()
    n2[1, 1:5] = 0.0                                                          # a zero quaternion
    expect(apply, pts, anchor, nodes, n2)
    return len(bad)

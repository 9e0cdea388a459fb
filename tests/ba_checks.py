"""Shared measurements for tests/test_ba_cases.py (CPU) and tests/test_ba_gpu.py
-- TEST INFRASTRUCTURE.

The oracle's variety on one window: oracle/ba.c over 16 observation orders
(ba_envelope.oracle_order: 0 as given, odd = shuffled inside each frame, even =
shuffled globally with the points relabelled) times its three reduced-system
arithmetics (LL', LDL', the FMA Gauss elimination): 48 runs, every one a valid
way to sum and solve the same problem.  Results are cached per (case,
max_iters) and never modified.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import ba_dense_ref as D
import ba_envelope as BE
import oracle_ffi as O

ORDERS = 16
SOLVERS = (O.BA_SOLVER_LLT, O.BA_SOLVER_LDLT, O.BA_SOLVER_GAUSS_FMA)
KINDS = ("K", "ext", "pts")
MARGIN = 4.0          # the GPU may sit this many oracle spreads from the target

_runs, _dense = {}, {}


def oracle_run(w, s, solver, max_iters):
    """one oracle run, the points back in the caller's labelling"""
    K, E, P, sm = BE.oracle_order(w, s, max_iters=max_iters, solver=solver)
    if s > 0 and s % 2 == 0:
        perm = np.random.default_rng(1_000_003 + s).permutation(len(w["pts"]))
        Q = np.empty_like(P)
        Q[perm] = P
        P = Q
    return K, E, P, sm


def oracle_runs(w, max_iters=None):
    """the 48 runs of case w: [(K4, ext, pts, summary)], run 0 = order 0, LL'"""
    mi = w["max_iters"] if max_iters is None else max_iters
    key = (w["name"], mi)
    if key not in _runs:
        jobs = [(s, sv) for sv in SOLVERS for s in range(ORDERS)]
        with ThreadPoolExecutor(8) as ex:
            _runs[key] = list(ex.map(lambda j: oracle_run(w, j[0], j[1], mi), jobs))
    return _runs[key]


def dense(w):
    """dense_step of case w: (K4, ext, pts, cost, info)"""
    if w["name"] not in _dense:
        _dense[w["name"]] = D.dense_step(w, w["loss"], w["loss_param"])
    return _dense[w["name"]]


def ints(sm):
    return (int(sm.iterations), int(sm.successful_steps), int(sm.termination), int(sm.usable))


def blocks(K, E, P):
    return {"K": np.asarray(K).ravel(), "ext": np.asarray(E).ravel(), "pts": np.asarray(P).ravel()}


def distances(x, target, start):
    """per block kind: max |x - target| relative to the step's own size
    max |target - start| (x, target, start: (K4, ext, pts) triples)"""
    bx, bt, bs = blocks(*x), blocks(*target), blocks(*start)
    out = {}
    for k in KINDS:
        if bt[k].size == 0:
            out[k] = 0.0
            continue
        size = float(np.abs(bt[k] - bs[k]).max())
        out[k] = float(np.abs(bx[k] - bt[k]).max()) / size if size > 0 else float(np.abs(bx[k] - bt[k]).max())
    return out


def oracle_distances(w, target, max_iters=1):
    """(per-kind max over the 48 runs, the per-run list) of distances to target"""
    start = (w["K4"], w["ext"], w["pts"])
    per = [distances(r[:3], target, start) for r in oracle_runs(w, max_iters)]
    return {k: max(d[k] for d in per) for k in KINDS}, per


def same_path(w, max_iters):
    """all 48 runs capped at max_iters made the same decisions"""
    return len({ints(r[3]) for r in oracle_runs(w, max_iters)}) == 1


def untouched(w, runs):
    """element masks (K, ext, pts) of what every oracle run left bit-identical"""
    s = blocks(w["K4"], w["ext"], w["pts"])
    m = {k: np.ones(s[k].shape, bool) for k in KINDS}
    for r in runs:
        b = blocks(*r[:3])
        for k in KINDS:
            m[k] &= b[k].view(np.uint64) == s[k].view(np.uint64)
    return m

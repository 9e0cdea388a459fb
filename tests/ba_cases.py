"""Named adversarial windows for the windowed bundle adjustment -- TEST
INFRASTRUCTURE (tests/test_ba_cases.py proves each is what it claims on the
CPU, tests/test_ba_gpu.py runs them on the device).

Every case is a dict in synthba.make_window's format (K4, ext, pts, obs_frame,
obs_point, obs_xy, gt_*) plus
  loss, loss_param, max_iters
  dense     the window is small enough for ba_dense_ref.dense_step (N <= ~500)
  decisive  the integer summary must agree over all oracle runs and on the GPU
  refused   None, or the name of the status the library must answer with
  summary   for most decisive cases: the (iterations, successful_steps,
            termination, usable) every oracle run must end with
  expect    {property: value} of structure(case): the property the case exists
            for, asserted by test_ba_cases.py.  A case's defining edit is
            marked "# defining edit"; without it the expectation fails.
Built from synthba's ground-truth scene (same camera path, depths, noise and
perturbation), the observation lists restructured.  numpy only, deterministic.
"""
import math

import numpy as np

from slamhip import synthba

LOSS_NONE, LOSS_TRIVIAL, LOSS_HUBER, LOSS_CAUCHY, LOSS_ARCTAN, LOSS_TUKEY = range(6)
K_CHUNK, K_GCHUNK, K_ITER_CHUNK, K_MAX_NC = 64, 32, 4, 136
DBL_EPS = float(np.finfo(np.float64).eps)


# ---- what ba_solve derives from the arrays (csrc/ba.hip, host bookkeeping) ----

def solve_kernel(nc):
    """the reduced camera system's kernel for nc columns (ba_solve's camera_solve)"""
    for cap, name in ((16, "lane<16>"), (28, "lane<28>"), (48, "lane<48>"), (64, "lane<64>"), (96, "rows<96,2>"),
                      (128, "rows<128,2>"), (K_MAX_NC, "lds<1024,10>")):
        if nc <= cap:
            return name
    return "refused"


def structure(w):
    """The grouping ba_solve makes of window w, restated: per-point frame tuples
    in the caller's observation order, which of them take the direct track[]
    slot and which the hash table, table regrows, chunk cuts, gram chunks --
    and the geometry / residual facts the cases are named after."""
    nf, npt = len(w["ext"]), len(w["pts"])
    of, op = np.asarray(w["obs_frame"]), np.asarray(w["obs_point"])
    tup = [[] for _ in range(npt)]
    for f, p in zip(of.tolist(), op.tolist()):
        tup[p].append(f)
    tup = [tuple(t) for t in tup]
    groups = {}
    for t in tup:
        groups[t] = groups.get(t, 0) + 1
    is_track = lambda t: all(t[k] == t[0] + k for k in range(len(t)))
    # the table holds every distinct tuple (a track is entered on first sight
    # too); it regrows when 2 * groups > mask
    mask, regrows = 1023, 0
    for n in range(1, len(groups) + 1):
        if 2 * n > mask:
            mask, regrows = 2 * mask + 1, regrows + 1
    chunks = []                                  # (nobs, len) in group order
    for t, cnt in groups.items():
        per = max(1, K_CHUNK // max(len(t), 1))
        chunks += [(len(t), min(per, cnt - s)) for s in range(0, cnt, per)]
    fcnt = np.bincount(of, minlength=nf) if len(of) else np.zeros(nf, int)
    pcnt = np.bincount(op, minlength=npt) if len(of) else np.zeros(npt, int)
    s = {
        "nf": nf, "np": npt, "no": int(len(of)), "nc": 4 + 6 * (nf - 1), "N": 4 + 6 * (nf - 1) + 3 * npt,
        "kernel": solve_kernel(4 + 6 * (nf - 1)),
        "tuples": len(groups), "hashed_tuples": sum(1 for t in groups if len(t) and not is_track(t)),
        "descending_tuples": sum(1 for t in groups if any(t[k] > t[k + 1] for k in range(len(t) - 1))),
        "regrows": regrows, "chunks": sorted(set(chunks)),
        "frame_obs": fcnt.tolist(), "gram_chunk_lens": sorted({min(K_GCHUNK, int(c) - s0) for c in fcnt
                                                              for s0 in range(0, int(c), K_GCHUNK)}),
        "unobserved_points": np.flatnonzero(pcnt == 0).tolist(),
        "unobserved_frames": np.flatnonzero(fcnt == 0).tolist(),
        "max_point_obs": int(pcnt.max()) if npt else 0,
        "repeated_frame_points": [p for p, t in enumerate(tup) if len(set(t)) < len(t)],
        "point_major": bool(np.all(np.diff(op) >= 0)) if len(of) else True,
        "loss": int(w.get("loss", 0)), "max_iters": int(w.get("max_iters", 50)),
    }
    ext, pts = np.asarray(w["ext"]), np.asarray(w["pts"])
    th = np.linalg.norm(ext[:, :3], axis=1)
    s["free_small_angle"] = int(np.sum(th[1:] ** 2 <= DBL_EPS))
    s["max_theta"] = float(th.max())
    s["finite"] = bool(np.isfinite(ext).all() and np.isfinite(pts).all() and np.isfinite(np.asarray(w["obs_xy"])).all())
    if len(of) and s["finite"]:
        with np.errstate(all="ignore"):
            r, z = residuals64(w)
        sq = (r * r).sum(1)
        a = float(w.get("loss_param", 0.0))
        s.update(behind_points=int(len(set(op[z < 0].tolist()))), z0_obs=int(np.sum(z == 0)),
                 zero_residuals=int(np.sum(sq == 0.0)), sq_equal_a2=int(np.sum(sq == a * a)),
                 beyond_a=int(np.sum(sq > a * a)), gross=int(np.sum(np.sqrt(sq) > 150.0)),
                 max_residual=float(np.sqrt(np.nanmax(sq))) if np.isfinite(sq).any() else math.inf)
    return s


def residuals64(w):
    """reprojection residuals (no, 2) and camera depths (no,) at the start, float64"""
    of, op = np.asarray(w["obs_frame"]), np.asarray(w["obs_point"])
    r = np.zeros((len(of), 2))
    z = np.zeros(len(of))
    for f in np.unique(of):
        m = of == f
        xy, z[m] = synthba.project(w["K4"], w["ext"][f], w["pts"][op[m]])
        r[m] = xy - np.asarray(w["obs_xy"])[m]
    return r, z


# ---- the scene ----

def std_tracks(rng, nf, npt, single_share=0.25, maxlen=4):
    """consecutive tracks 1..maxlen frames long, starting anywhere (frame 0
    included); the first nf points start at frame p so that every frame is seen"""
    tr = []
    for p in range(npt):
        n = 1 if rng.random() < single_share else int(rng.integers(2, maxlen + 1))
        n = min(n, nf)
        first = p % nf if p < nf else int(rng.integers(0, nf))
        first = min(first, nf - n)
        tr.append(list(range(first, first + n)))
    return tr


def build(nf, tracks, seed, noise=0.5, perturb=True, rounded=True, K4=synthba.K_1080P, gt_ext=None, **kw):
    """tracks[p] = the frames observing point p, in observation order (point-major)"""
    rng = np.random.default_rng(seed)
    npt = len(tracks)
    K4 = np.array(K4, np.float64)
    if gt_ext is None:
        gt_ext = np.zeros((nf, 6))
        for i in range(nf):
            gt_ext[i, :3] = (0.0, math.radians(0.5 * i), 0.0)
            gt_ext[i, 3:] = (0.0, 0.0, -0.02 * i)
    fx, fy, cx, cy = synthba.K_1080P               # the scene's geometry, whatever camera K4 views it
    u, v = rng.uniform(400, 1500, npt), rng.uniform(100, 980, npt)
    z = rng.uniform(2.0, 8.0, npt)
    pts = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    of, op, oxy = [], [], []
    for p, fr in enumerate(tracks):
        for f in fr:
            xy, _ = synthba.project(K4, gt_ext[f], pts[p:p + 1])
            xy = xy[0] + rng.normal(0, noise, 2)
            of.append(f)
            op.append(p)
            oxy.append(np.round(xy) if rounded else xy)
    w = dict(gt_K4=K4.copy(), gt_ext=gt_ext.copy(), gt_pts=pts.copy(), obs_frame=np.array(of, np.int32),
             obs_point=np.array(op, np.int32), obs_xy=np.array(oxy, np.float64).reshape(-1, 2))
    ext = gt_ext.copy()
    if perturb:
        K4 = K4 * (1 + rng.normal(0, 0.005, 4))
        ext[1:, :3] += rng.normal(0, math.radians(0.5), (nf - 1, 3))
        ext[1:, 3:] += rng.normal(0, 0.01, (nf - 1, 3))
        pts = pts + rng.normal(0, 0.02, pts.shape)
    w.update(K4=np.ascontiguousarray(K4), ext=np.ascontiguousarray(ext), pts=np.ascontiguousarray(pts),
             loss=LOSS_NONE, loss_param=0.0, max_iters=50, dense=True, decisive=False, refused=None, expect={},
             summary=None)
    w.update(kw)
    return w


def reorder(w, idx):
    for k in ("obs_frame", "obs_point", "obs_xy"):
        w[k] = np.ascontiguousarray(w[k][idx])
    return w


def add_obs(w, frame, point, n, rng, noise=0.5):
    """n more observations of `point` by `frame`, each with its own noise"""
    xy, _ = synthba.project(w["gt_K4"], w["gt_ext"][frame], w["gt_pts"][point:point + 1])
    new = np.round(xy[0] + rng.normal(0, noise, (n, 2)))
    w["obs_frame"] = np.concatenate([w["obs_frame"], np.full(n, frame, np.int32)])
    w["obs_point"] = np.concatenate([w["obs_point"], np.full(n, point, np.int32)])
    w["obs_xy"] = np.concatenate([w["obs_xy"], new])
    return w


def _std(nf, npt, seed, **kw):
    return build(nf, std_tracks(np.random.default_rng(1000 + seed), nf, npt), seed, **kw)


# ---- the cases ----

def _solve_paths(c):
    for nf in (1, 2, 3, 11, 12, 17, 21, 22, 23):
        nc = 4 + 6 * (nf - 1)
        # (one frame: every point observed twice, so that the optimum's cost is
        # not an exact fit's rounding noise, which no relative bar can compare)
        tr = [[0, 0]] * 60 if nf == 1 else std_tracks(np.random.default_rng(1010 + nf), nf, 60)
        c[f"nf{nf:02d}"] = build(nf, tr, 10 + nf, decisive=nf == 1,                # defining edit: nf
                                 summary=(3, 2, 1, 1) if nf == 1 else None,
                                 expect={"nc": nc, "kernel": solve_kernel(nc), "unobserved_frames": []})
    c["nf24"] = _std(24, 60, 34, dense=False, refused="SLAM_E_UNSUPPORTED",       # defining edit: nf = 24
                     expect={"nc": 142, "kernel": "refused"})
    assert [solve_kernel(4 + 6 * (nf - 1)) for nf in (3, 11, 12, 17, 21, 22, 23)] == \
        ["lane<16>", "lane<64>", "rows<96,2>", "rows<128,2>", "rows<128,2>", "lds<1024,10>", "lds<1024,10>"]


def _hash_tracks(nf=12, npt=700, seed=5):
    rng = np.random.default_rng(seed)
    return [rng.permutation(nf)[:int(rng.integers(2, 6))].tolist() for _ in range(npt)]   # defining edit: subsets


def _grouping(c):
    w = build(12, _hash_tracks(), 41, dense=False)
    n = len({tuple(t) for t in _hash_tracks()})
    w["expect"] = {"tuples": n, "regrows": 1, "point_major": True}
    assert n > 512
    c["hash"] = w
    w = build(12, _hash_tracks(), 41, dense=False)
    reorder(w, np.random.default_rng(42).permutation(len(w["obs_frame"])))        # defining edit: global shuffle
    w["expect"] = {"regrows": 1, "point_major": False}
    c["hash_shuffled"] = w
    # groups of exactly per and per + 1 points, per = 64 / nobs
    for nobs, tuples in ((1, ((2,), (3,))), (3, ((1, 3, 4), (0, 2, 5))), (5, ((0, 2, 3, 5, 6), (6, 4, 3, 1, 0)))):
        per = K_CHUNK // nobs
        tr = [list(tuples[0])] * per + [list(tuples[1])] * (per + 1)              # defining edit: per, per + 1
        tr += std_tracks(np.random.default_rng(50 + nobs), 7, 30, single_share=0.0, maxlen=2 if nobs == 3 else 4)[7:]
        w = build(7, tr, 50 + nobs)
        st = structure(w)
        w["expect"] = {"chunks": st["chunks"]}
        assert (nobs, per) in st["chunks"] and (nobs, 1) in st["chunks"] and \
            not any(n == nobs and ln not in (per, 1) for n, ln in st["chunks"]), st["chunks"]
        c[f"per_n{nobs}"] = w
    # a frame with exactly 32 observations and one with 33 (gram chunks of 32, then 32 + 1)
    tr = [[0, 1]] * 32 + [[2, 3]] * 33 + [[0, 3]] * 6                             # defining edit: 32 / 33
    c["gram_32_33"] = build(4, tr, 60, expect={"frame_obs": [38, 32, 33, 39], "gram_chunk_lens": [1, 6, 7, 32]})


def _degenerate(c):
    tr = std_tracks(np.random.default_rng(70), 6, 60)
    for p in (0, 17, 59):
        tr[p] = []                                                                # defining edit: no observation
    c["unobserved_points"] = build(6, tr, 70, expect={"unobserved_points": [0, 17, 59], "unobserved_frames": []})
    tr = [[f for f in t if f not in (3, 5)] or [1, 2] for t in std_tracks(np.random.default_rng(71), 6, 60)]  # defining edit
    c["unobserved_frames"] = build(6, tr, 71, expect={"unobserved_frames": [3, 5]})
    tr = std_tracks(np.random.default_rng(72), 6, 60)
    tr[5] = [2, 3, 2]                                                             # defining edit: frame 2 twice
    c["same_frame_twice"] = build(6, tr, 72, expect={"repeated_frame_points": [5]})
    for n in (64, 65):
        w = _std(8, 50, 73)
        have = int(np.sum(w["obs_point"] == 7))
        rng = np.random.default_rng(74)
        for k in range(n - have):                                                 # defining edit: n observations
            add_obs(w, k % 8, 7, 1, rng)
        w["expect"] = {"max_point_obs": n}
        if n == 65:
            w.update(refused="SLAM_E_UNSUPPORTED", dense=False)
        c[f"obs{n}"] = w
    w = _std(4, 40, 75, decisive=True, summary=(0, 0, 1, 1))
    reorder(w, np.zeros(0, int))                                                  # defining edit: nobs = 0
    w["expect"] = {"no": 0, "np": 40}
    c["no_obs"] = w


def _geometry(c):
    w = _std(6, 60, 80)
    w["ext"][:, :3] = 0.0                                                         # defining edit: zero rotation
    w["expect"] = {"free_small_angle": 5}
    c["zero_rotation"] = w
    gt = np.zeros((5, 6))
    for i in range(5):
        gt[i, :3] = (0.0, math.radians(0.5 * i), 0.0)
        gt[i, 3:] = (0.0, 0.0, -0.02 * i)
    gt[2, :3] = (0.0, 0.0, math.pi - 1e-3)                                        # defining edit: roll of almost pi
    w = build(5, std_tracks(np.random.default_rng(81), 5, 60), 81, gt_ext=gt)
    w["ext"][2, :3] = gt[2, :3] + np.array([2e-4, -3e-4, 2e-3])                   # |aa| straddles pi along the path
    w["expect"] = {"max_theta": float(np.linalg.norm(w["ext"][2, :3]))}
    assert abs(w["expect"]["max_theta"] - math.pi) < 2e-3
    c["near_pi"] = w
    w = _std(6, 60, 82)
    w["pts"][:20] *= -1.0                                                         # defining edit: mirrored behind
    w["expect"] = {"behind_points": 20}
    c["behind_camera"] = w
    # frame 0 (identity) sees every z = 0 point at depth exactly 0; the other
    # frames at a depth of a few centimetres, either sign
    w = _std(6, 60, 83, decisive=True, dense=False, summary=(5, 0, 3, 0))
    w["pts"][:, 2] = 0.0                                                          # defining edit: z = 0
    w["expect"] = {"z0_obs": int(np.sum(w["obs_frame"] == 0))}
    assert w["expect"]["z0_obs"] > 0
    c["z_zero"] = w
    w = _std(6, 60, 84, decisive=True, dense=False, summary=(5, 0, 3, 0))
    w["obs_xy"][11, 0] = np.nan                                                   # defining edit
    w["expect"] = {"finite": False}
    c["nan_observation"] = w
    w = _std(6, 60, 85, decisive=True, dense=False, summary=(5, 0, 3, 0))
    w["pts"][int(w["obs_point"][3]), 1] = np.inf                                  # defining edit
    w["expect"] = {"finite": False}
    c["inf_point"] = w


def _losses(c):
    for loss, a in ((LOSS_NONE, 0.0), (LOSS_TRIVIAL, 0.0), (LOSS_HUBER, 2.0), (LOSS_CAUCHY, 2.0), (LOSS_ARCTAN, 4.0),
                    (LOSS_TUKEY, 400.0)):
        w = _std(6, 63, 90, loss=loss, loss_param=a)
        w["obs_xy"][::9, 0] += 300.0                                              # defining edit: gross outliers
        w["expect"] = {"gross": len(w["obs_xy"][::9]), "loss": loss}
        c[f"outliers_loss{loss}"] = w
    for name, loss, sm in (("tukey", LOSS_TUKEY, (0, 0, 1, 1)), ("huber", LOSS_HUBER, (50, 50, 0, 1))):
        w = _std(6, 60, 91, loss=loss, loss_param=1e-3, decisive=True, summary=sm)   # defining edit: a below every |r|
        w["expect"] = {"beyond_a": len(w["obs_frame"])}
        c[f"{name}_all_outside"] = w
    # exact residuals: a point on frame 0's optical axis projects to (cx, cy) in
    # any arithmetic (x / z = 0), so the residual is the plain difference
    for name, off, loss, a, key in (("zero_residual", (0.0, 0.0), LOSS_HUBER, 2.0, "zero_residuals"),
                                    ("huber_at_threshold", (3.0, 4.0), LOSS_HUBER, 5.0, "sq_equal_a2")):
        tr = std_tracks(np.random.default_rng(92), 6, 60)
        tr[0] = [0, 1, 2]
        w = build(6, tr, 92, loss=loss, loss_param=a)
        w["pts"][0] = (0.0, 0.0, 3.5)
        # cx in [512, 1024) and cx - 3 too (cy, cy - 4 likewise): the subtraction is exact
        w["obs_xy"][0] = (w["K4"][2] - off[0], w["K4"][3] - off[1])               # defining edit
        w["expect"] = {key: 1}
        c[name] = w


def _exits(c):
    # ground truth start, unrounded noise-free observations, a normalised camera
    # (fx = fy = 1, cx = cy = 0): residuals of a few ulp(0.5), so the gradient is
    # ~1e-16, far under the 1e-10 tolerance in any arithmetic
    w = build(5, std_tracks(np.random.default_rng(100), 5, 60), 100, noise=0.0, perturb=False, rounded=False,
              K4=(1.0, 1.0, 0.0, 0.0), decisive=True, summary=(0, 0, 1, 1))       # defining edit
    w["expect"] = {"max_residual": structure(w)["max_residual"]}
    assert w["expect"]["max_residual"] < 1e-14
    c["ground_truth_start"] = w
    for k in (1, 2, 3, 4, 5):
        c[f"max_iters{k}"] = _std(8, 80, 101, max_iters=k, decisive=True,          # defining edit: max_iters
                                  summary=(k, min(k, 4), 0, 1), expect={"max_iters": k})
    # converging windows: every point seen by every frame (twice by the only
    # frame of the one-frame windows, so that the optimum is no exact fit).
    # (frames, seed, noise, rounded, the iteration at which every oracle run
    # meets a tolerance), found by a search over seeds 0..15: inside the first
    # chunk of 4 queued iterations, exactly at its end, at a later chunk's end,
    # and inside a later chunk
    for nf, seed, noise, rnd, it, succ in ((1, 14, 0.5, True, 3, 2), (1, 10, 0.5, True, 4, 3),
                                           (4, 5, 0.05, False, 12, 11), (4, 8, 0.05, False, 14, 12)):
        tr = [[0, 0]] * 40 if nf == 1 else [list(range(nf))] * 40
        c[f"converges_at_{it}"] = build(nf, tr, seed, noise=noise, rounded=rnd,    # defining edit: seed
                                        decisive=True, summary=(it, succ, 1, 1), expect={"tuples": 1})


# (case, k): the oracle's own 48 runs capped at k iterations do not all take the
# same accept / reject path, so there is no envelope for the device at that k
# (test_ba_cases.py asserts that this list is exact)
PATHS_DIFFER = ()


def make_cases():
    c = {}
    _solve_paths(c)
    _grouping(c)
    _degenerate(c)
    _geometry(c)
    _losses(c)
    _exits(c)
    for name, w in c.items():
        w["name"] = name
    return c


_CASES = None


def cases():
    """the cases, built once; callers copy what they modify (fresh(case))"""
    global _CASES
    if _CASES is None:
        _CASES = make_cases()
    return _CASES


def fresh(w):
    """a deep copy of the arrays the solvers update in place"""
    v = dict(w)
    for k in ("K4", "ext", "pts"):
        v[k] = w[k].copy()
    return v

"""Semi-global aggregation of the plane-sweep cost volume: the definition (DESIGN.md
section 28), plain numpy on top of tests/mvs_ref.py.

Everything is integer arithmetic, so any schedule of the sums gives the same bits.
The device kernels (csrc/mvs_sgm.hip) and the host twin (csrc/mvs_sgm_host.cpp)
equal these results bit for bit.  Nothing here is fast.
"""
import numpy as np

import mvs_ref as R

PATHS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))
MAX_COST = 64 * 49 * 4            # C <= 64 (2r + 1)^2 S at r = 3, S = 4
MAX_P2 = 65535 - MAX_COST         # so that C + P2 fits uint16
_BIG = np.int64(1) << 40


def effective(p, radius, S):
    """the penalty of a reference with S sources at radius r from the per-pixel, per-source one"""
    return int(p) * (2 * int(radius) + 1) ** 2 * int(S)


def _step(c, prev, P1, P2):
    """L_r of a row of pixels (D, n) from their costs and the predecessors' L_r"""
    m = prev.min(0, keepdims=True)
    pad = np.full_like(prev[:1], _BIG)
    below = np.concatenate([pad, prev[:-1]]) + P1        # L_r(q, d - 1), absent at d = 0
    above = np.concatenate([prev[1:], pad]) + P1         # L_r(q, d + 1), absent at d = D - 1
    return c + np.minimum(np.minimum(prev, below), np.minimum(above, m + P2)) - m


def path(C, dx, dy, P1, P2):
    """L_r of one direction: (D, h, w) int64"""
    C = np.asarray(C).astype(np.int64)
    D, H, W = C.shape
    L = np.empty_like(C)
    if dy != 0:
        xs = np.arange(W)
        qx = xs - dx
        inside = (qx >= 0) & (qx < W)
        qc = np.clip(qx, 0, W - 1)
        for y in (range(H) if dy > 0 else range(H - 1, -1, -1)):
            qy = y - dy
            if not 0 <= qy < H:
                L[:, y] = C[:, y]
                continue
            L[:, y] = np.where(inside[None], _step(C[:, y], L[:, qy][:, qc], P1, P2), C[:, y])
    else:
        for x in (range(W) if dx > 0 else range(W - 1, -1, -1)):
            qx = x - dx
            if not 0 <= qx < W:
                L[:, :, x] = C[:, :, x]
                continue
            L[:, :, x] = _step(C[:, :, x], L[:, :, qx], P1, P2)
    assert (L >= C).all() and (L <= C + P2).all() and int(L.max()) <= 65535      # a path value fits uint16
    return L


def aggregate(C, P1, P2, paths=8):
    """S = the sum of L_r over the first `paths` directions: (D, h, w) int32"""
    P1, P2 = int(P1), int(P2)
    if paths not in (4, 8) or not 0 <= P1 <= P2 <= MAX_P2:
        raise ValueError("paths 4 or 8, 0 <= P1 <= P2 <= 65535 - 12544")
    C = np.asarray(C)
    assert C.min() >= 0 and C.max() <= MAX_COST
    S = np.zeros(C.shape, np.int64)
    for dx, dy in PATHS[:paths]:
        S += path(C, dx, dy, P1, P2)
    assert int(S.max()) <= 8 * 65535                     # 500192 with penalties from p <= 255: int32 with room
    return S.astype(np.int32)


_VOL = {}


def volume(name):
    """(C, nvalid) of a mvs_ref case, computed once; read-only"""
    if name not in _VOL:
        sc, r, _, _ = R.sweep_cases()[name]
        C, nv = R.cost_volume(sc["ref"], sc["srcs"], sc["M"], sc["v"], sc["planes"], r)
        C.setflags(write=False)
        nv.setflags(write=False)
        _VOL[name] = (C, nv)
    return _VOL[name]


def depth_from_volume(C, nvalid, planes, S, radius, uniq, min_views, p1, p2, paths):
    if not 0 <= p1 <= p2 <= 255:
        raise ValueError("0 <= p1 <= p2 <= 255")
    agg = aggregate(C, effective(p1, radius, S), effective(p2, radius, S), paths)
    return R.winner(agg, nvalid, planes, uniq, min_views)


def depth(ref, srcs, M, v, planes, radius=2, uniq=80, min_views=1, p1=10, p2=120, paths=8):
    """(plane int16, cost int32 = S[best], inv_depth float32): mvs_ref.winner on the aggregated volume"""
    C, nv = R.cost_volume(ref, srcs, M, v, planes, radius)
    return depth_from_volume(C, nv, planes, len(srcs), radius, uniq, min_views, p1, p2, paths)


_CACHE = {}


def case(name, p1, p2, paths):
    """the aggregated result of a mvs_ref case, computed once"""
    key = (name, p1, p2, paths)
    if key not in _CACHE:
        sc, r, uq, mv = R.sweep_cases()[name]
        C, nv = volume(name)
        out = depth_from_volume(C, nv, sc["planes"], len(sc["srcs"]), r, uq, mv, p1, p2, paths)
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


SETTINGS = ((10, 120, 8), (2, 12, 4), (0, 255, 8), (255, 255, 4))


# ---- scenes ------------------------------------------------------------------------------

def wall_scene():
    """a 64 x 48 noise texture with a constant-gray box, one source shifted by 5 planes"""
    ref = R.noise(48, 64, 7)
    ref[14:35, 20:45] = 128
    return dict(ref=ref, srcs=[R.shifted(ref, 5)], M=np.eye(3).reshape(1, 9), v=np.array([[1.0, 0.0, 0.0]]),
                planes=np.arange(12, dtype=np.float64), k=5, interior=(slice(20, 28), slice(26, 33)),
                region=(slice(5, 43), slice(6, 53)))


def pose_scene(h, w, D, seed, S=1):
    """a general-pose scene of any shape (the path kernel's edge shapes and plane counts)"""
    return R.general_pose(h, w, S, D, seed)


EDGE_SHAPES = ((1, 1), (1, 9), (9, 1), (8, 8), (33, 67), (67, 33))      # (h, w)
EDGE_PLANES = (4, 63, 64, 65, 128, 129, 256)                             # at 24 x 20


def random_volume(rng, n, h, w, D, maxima=False):
    """n x h x w x D uint16 costs in the public layout; with maxima most values sit at 12544 or 0"""
    if maxima:
        C = rng.choice(np.array([0, MAX_COST, MAX_COST - 1, 1], np.uint16), size=(n, h, w, D), p=[0.3, 0.5, 0.1, 0.1])
    else:
        C = rng.randint(0, MAX_COST + 1, (n, h, w, D)).astype(np.uint16)
    return np.ascontiguousarray(C, np.uint16)


def aggregate_public(C, P1, P2, paths):
    """aggregate() in the public layout: (n, h, w, D) uint16 -> (n, h, w, D) int32"""
    C = np.asarray(C)
    return np.ascontiguousarray(np.stack([aggregate(c.transpose(2, 0, 1), P1, P2, paths).transpose(1, 2, 0) for c in C]))

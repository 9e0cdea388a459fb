"""Adversarial kNN fixtures and an exact k = 2 reference (pure numpy) -- TEST INFRASTRUCTURE.

The matcher (csrc/knn.hip) ranks train rows by a key whose form depends on the
descriptors: api.cpp's knn_host picks the key mode from the largest row norms
mq (query) and mt (train) of a SIFT pair,

    NORM_L1                        -> MODE_L1P   packed (L1 << 17) | row
    mq + mt > 2048                 -> MODE_SQRT  float bits of sqrtf(d^2)
    (mq + mt)^2 < 2^21 - 1         -> MODE_L2P   packed (d^2 field << 10) | row
    otherwise                      -> MODE_L2    unpacked i32 keys

and ORB descriptors always take MODE_HAMP (packed float keys).  Every case
below names the mode it was built for; tests/test_knn_cases.py proves on the
CPU that its norms fall in that mode's interval, tests/test_knn_gpu.py asserts
through slam_last_knn_launch that the kernel of that mode really ran.

Run as a program it is the child process of test_knn_gpu.py's variant tests:
the kernel variant is chosen by environment variables that the library reads
once per process, so each variant runs the cases in a process of its own and
writes what the library returned to an .npz file.
"""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

# include/slamhip.h
SIFT_BF, ORB_BF = 0, 2
NORM_L1, NORM_L2, NORM_HAMMING = 2, 4, 6
MODE_L2, MODE_SQRT, MODE_L2P, MODE_HAMP, MODE_L1P = 0, 2, 3, 4, 5
V_MFMA, V_PK_QT2, V_PK_QT1, V_PIPE_QT2, V_PIPE_QT1, V_L1 = 1, 2, 3, 4, 5, 6
V_XCD = 0x100
FLT_MAX = np.float32(np.finfo(np.float32).max)
DM = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])

# api.cpp knn_host: the two thresholds on the norm sum s = mq + mt
SQRT_ABOVE = 2048.0                    # s > 2048 -> MODE_SQRT
PACKED_BELOW_SQ = float((1 << 21) - 1)   # s * s < 2^21 - 1 -> MODE_L2P

# name: the case's id.  tsplit: the split count the launch must report (None:
# not part of the case).  ratios: ratio-test thresholds the case is also run
# through slam_match with.  expect: (idx, dist) the case was constructed to
# give for its first queries, where it was constructed for one (must equal knn2_exact's).
Case = namedtuple("Case", "name q t matcher norm mode tsplit ratios expect")


def _case(name, q, t, matcher, norm, mode, tsplit=None, ratios=(), expect=None):
    if matcher == ORB_BF:
        q, t = np.ascontiguousarray(q, np.uint8).reshape(-1, 32), np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    else:
        q, t = (np.ascontiguousarray(q, np.float32).reshape(-1, 128),
                np.ascontiguousarray(t, np.float32).reshape(-1, 128))
    return Case(name, q, t, matcher, norm, mode, tsplit, tuple(ratios), expect)


# ---- the exact reference ---------------------------------------------------------

def _bits(a):
    return np.unpackbits(np.ascontiguousarray(a, np.uint8), axis=1).astype(np.float32)


def distances_exact(q, t, norm):
    """(nq, nt) f32 distances as the reference matcher reports them, from exact
    integer arithmetic.  L2: d2 = sum (q - t)^2 = |q|^2 + |t|^2 - 2 <q, t>; every
    term is an integer below 2^24, so the f64 matrix product and the int64 sum
    are exact and so is the cast of d2 to f32; the f32 square root is IEEE's."""
    if norm == NORM_L2:
        qi, ti = q.astype(np.float64), t.astype(np.float64)
        dot = (qi @ ti.T).astype(np.int64)
        d2 = (qi * qi).sum(1).astype(np.int64)[:, None] + (ti * ti).sum(1).astype(np.int64)[None, :] - 2 * dot
        assert d2.size == 0 or (d2.min() >= 0 and d2.max() < 1 << 24)
        return np.sqrt(d2.astype(np.float32))
    if norm == NORM_L1:
        qi, ti = q.astype(np.int32), t.astype(np.int32)
        out = np.zeros((len(q), len(t)), np.int64)
        for i in range(len(q)):
            out[i] = np.abs(ti - qi[i]).sum(1)
        return out.astype(np.float32)
    if norm == NORM_HAMMING:
        # popcount(a ^ b) = |a| + |b| - 2 <a, b> over the 256 bits (integers <= 256: exact in f32)
        qb, tb = _bits(q), _bits(t)
        return (qb.sum(1)[:, None] + tb.sum(1)[None, :] - 2 * (qb @ tb.T)).astype(np.float32)
    raise ValueError(norm)


def sq_dist_exact(q, t):
    """(nq, nt) int64 squared L2 distances, summed directly."""
    qi, ti = q.astype(np.int64), t.astype(np.int64)
    return np.stack([((ti - qi[i]) ** 2).sum(1) for i in range(len(q))]) if len(q) else np.zeros((0, len(t)), np.int64)


def top2(d):
    """the two smallest of each row of d by (value, index); -1 / FLT_MAX where a
    row has fewer than two entries, as the C ABI returns them"""
    nq, nt = d.shape
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), FLT_MAX, np.float32)
    if nq == 0 or nt == 0:
        return idx, dist
    r = np.arange(nq)
    i0 = np.argmin(d, axis=1)                 # the first of equal minima: the lower index
    idx[:, 0], dist[:, 0] = i0, d[r, i0]
    if nt >= 2:
        m = d.astype(np.float64)
        m[r, i0] = np.inf
        i1 = np.argmin(m, axis=1)
        idx[:, 1], dist[:, 1] = i1, d[r, i1]
    return idx, dist


def knn2_exact(q, t, norm):
    """DescriptorMatcher::knnMatch(q, t, k = 2): (idx nq x 2 i32, dist nq x 2 f32)."""
    return top2(distances_exact(q, t, norm))


def ratio_exact(idx, dist, ratio):
    """getGoodMatches on knn2 output: query order, d0 < ratio * d1 in double, both neighbours present"""
    ok = (idx[:, 0] >= 0) & (idx[:, 1] >= 0)
    ok &= dist[:, 0].astype(np.float64) < float(ratio) * dist[:, 1].astype(np.float64)
    qi = np.nonzero(ok)[0]
    out = np.zeros(len(qi), DM)
    out["queryIdx"], out["trainIdx"], out["distance"] = qi, idx[qi, 0], dist[qi, 0]
    return out


def norm_sum(q, t):
    """mq + mt as api.cpp computes it: the largest f64 row norm of each side"""
    def mx(a):
        return float(np.sqrt((a.astype(np.float64) ** 2).sum(1)).max()) if len(a) else 0.0
    return mx(q) + mx(t)


def mode_for(q, t, matcher, norm):
    """the key mode api.cpp's knn_host picks for a pair"""
    if matcher == ORB_BF:
        return MODE_HAMP
    if norm == NORM_L1:
        return MODE_L1P
    s = norm_sum(q, t)
    if s > SQRT_ABOVE:
        return MODE_SQRT
    if s * s < PACKED_BELOW_SQ:
        return MODE_L2P
    return MODE_L2


def expected_variant(mode, pipe=0, xcd=0):
    """SLAM_KNN_VARIANT_* that launch_knn runs for a key mode under
    SLAMHIP_KNN_PIPE = pipe and SLAMHIP_KNN_XCD = xcd"""
    xb = V_XCD if xcd else 0
    if mode in (MODE_L2, MODE_SQRT):
        return V_MFMA
    if mode == MODE_L1P:
        return V_L1
    if mode == MODE_L2P:
        return {0: V_PK_QT2 | xb, 1: V_PIPE_QT2, 2: V_PIPE_QT1, 3: V_PK_QT1 | xb}[pipe]
    if mode == MODE_HAMP:
        return V_PIPE_QT2 if pipe == 1 else V_PK_QT2 | xb
    raise ValueError(mode)


def row_with_sqnorm(n):
    """a 128-entry row of integers 0..255 whose squares sum to exactly n (greedy:
    the largest square that fits, again and again)"""
    row, left = [], int(n)
    while left > 0:
        v = min(255, int(np.floor(np.sqrt(left))))
        while v * v > left:
            v -= 1
        row.append(v)
        left -= v * v
    assert len(row) <= 128, (n, len(row))
    out = np.zeros(128, np.float32)
    out[:len(row)] = row
    assert int((out.astype(np.int64) ** 2).sum()) == int(n)
    return out


# ---- descriptor families: the value range fixes the key mode ----------------------
# SIFT rows uniform in 0..hi have a norm near sqrt(128 hi (2 hi + 1) / 6):
#   0..40   ~ 266   (sum ~ 530: packed)      0..128 ~ 838 (sum ~ 1680: L2)
#   150..255 ~ 2320 (sum ~ 4600: sqrt keys); L1 uses the full 0..255
FAMILIES = {
    "pk": (SIFT_BF, NORM_L2, MODE_L2P, 0, 41),
    "l2": (SIFT_BF, NORM_L2, MODE_L2, 0, 129),
    "sqrt": (SIFT_BF, NORM_L2, MODE_SQRT, 150, 256),
    "l1": (SIFT_BF, NORM_L1, MODE_L1P, 0, 256),
    "ham": (ORB_BF, NORM_HAMMING, MODE_HAMP, 0, 256),
}


def _rows(rng, fam, n):
    matcher, _, _, lo, hi = FAMILIES[fam]
    if matcher == ORB_BF:
        return rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return rng.integers(lo, hi, (n, 128)).astype(np.float32)


def _fam_case(name, fam, q, t, **kw):
    matcher, norm, mode, _, _ = FAMILIES[fam]
    return _case(name, q, t, matcher, norm, mode, **kw)


def _seed(*parts):
    """a reproducible seed from a case's parameters"""
    s = 0
    for p in parts:
        for ch in str(p):
            s = (s * 131 + ord(ch)) % (1 << 31)
    return s


def _perturb(row, fam, d):
    """a copy of row at distance exactly d (L2, L1: entry 0 raised by d; Hamming: the first d bits flipped)"""
    out = row.copy()
    if FAMILIES[fam][0] == ORB_BF:
        bits = np.unpackbits(out)
        bits[:d] ^= 1
        return np.packbits(bits)
    out[0] += d if out[0] + d <= 255 else -d
    return out


# ---- the named cases -------------------------------------------------------------

def mode_l2_random(nq, nt):
    rng = np.random.default_rng(_seed("l2r", nq, nt))
    q, t = _rows(rng, "l2", nq), _rows(rng, "l2", nt)
    # three planted duplicates: the lower train index must win each tie
    t[nt // 2] = t[1]
    t[nt - 1] = t[2]
    t[nt // 3] = t[5]
    q[0], q[1], q[2] = t[1], t[2], t[5]
    return _fam_case(f"mode_l2_random-{nq}x{nt}", "l2", q, t)


def _edge_sqnorm():
    """the smallest N with (1024 + sqrt(N))^2 >= 2^21 - 1 in f64, as api.cpp evaluates it"""
    n = 179000
    while (1024.0 + np.sqrt(float(n))) ** 2 < PACKED_BELOW_SQ:
        n += 1
    return n


def mode_edges():
    """one query of norm exactly 1024 against train sets whose largest norm puts the
    sum just below / above the packed threshold, at 2048 exactly and just above it"""
    rng = np.random.default_rng(7)
    q = np.zeros((1, 128), np.float32)
    q[0, :64] = 128                                   # |q|^2 = 64 * 2^14 = 2^20
    far = rng.integers(0, 9, (5, 128)).astype(np.float32)      # norms below 100: never the largest
    n = _edge_sqnorm()
    out = []
    for tag, sq, mode in (("below_packed", n - 1, MODE_L2P), ("above_packed", n, MODE_L2)):
        t = np.vstack([far[:2], row_with_sqnorm(sq)[None], far[2:], row_with_sqnorm(sq)[None]])
        out.append(_case(f"mode_edges-{tag}", q, t, SIFT_BF, NORM_L2, mode))
    hi = np.zeros(128, np.float32)
    hi[64:] = 128                                     # |t| = 1024, d^2 to q = 2^21
    t = np.vstack([far[:3], hi[None], q, far[3:], hi[None]])
    out.append(_case("mode_edges-sum_2048", q, t, SIFT_BF, NORM_L2, MODE_L2))
    hi2 = hi.copy()
    hi2[64] = 129
    t = np.vstack([far[:3], hi2[None], q, far[3:], hi2[None]])
    out.append(_case("mode_edges-above_2048", q, t, SIFT_BF, NORM_L2, MODE_SQRT))
    return out


def adjacent_d2_below_2p22():
    """a zero query against rows with |t|^2 = 2^22 - 300 .. 2^22 - 1: the largest
    d^2 the unpacked kernel is used for; all 300 have distinct f32 roots"""
    rng = np.random.default_rng(22)
    sq = (1 << 22) - 300 + rng.permutation(300)
    t = np.vstack([np.stack([row_with_sqnorm(int(s)) for s in sq]), _rows(rng, "l2", 37)])
    t = t[rng.permutation(len(t))]
    return _case("adjacent_d2_below_2p22", np.zeros((1, 128), np.float32), t, SIFT_BF, NORM_L2, MODE_L2)


SQRT_TIES_BASE, SQRT_TIES_BASE_TOP2 = 6000000, 6000002


def sqrt_ties_seed(base):
    """the first shuffle seed that puts a larger d^2 at a lower index than an
    equal-root smaller one within the zero query's top two (None: no shuffle can)"""
    v = base + np.arange(300)
    for seed in range(64):
        sq = base + np.random.default_rng(seed).permutation(300)
        by_root, _ = top2(np.sqrt(sq.astype(np.float32))[None])
        by_d2 = np.lexsort((np.arange(300), sq))[:2]
        if by_root[0].tolist() != by_d2.tolist():
            return seed
    r = np.sqrt(v[:3].astype(np.float32))
    assert r[0] < r[1] < r[2]                 # the two smallest roots are distinct from all others
    return None


def adjacent_d2_sqrt_ties(base, zero_only=False):
    """a zero query (and a few random ones) against rows with |t|^2 = base .. base
    + 299 in a shuffled order: distinct d^2 with equal f32 roots tie and the lower
    index wins.  From 6,000,000 the roots of the three smallest d^2 are distinct,
    so no shuffle shows such a tie in the zero query's top two; from 6,000,002 the
    two smallest share a root, and the seed puts the larger d^2 at the lower
    index -- a kernel that ranks by d^2 fails.  zero_only: without the random
    queries the norm sum is 2449.5, just past the 2048 threshold (with them ~4770)."""
    seed = sqrt_ties_seed(base)
    rng = np.random.default_rng(3 if seed is None else seed)
    sq = base + rng.permutation(300)
    t = np.stack([row_with_sqnorm(int(s)) for s in sq])
    q = np.vstack([np.zeros((1, 128), np.float32), _rows(rng, "sqrt", 4)])[:1 if zero_only else 5]
    return _case(f"adjacent_d2_sqrt_ties-{base}" + ("-zero_only" if zero_only else ""), q, t, SIFT_BF, NORM_L2,
                 MODE_SQRT)


def field_extremes():
    out = []
    # (i) everything zero: |q'|^2 = |t'|^2 = <q', t'> = 2^21, every packed field is 0
    q, t = np.zeros((3, 128), np.float32), np.zeros((70, 128), np.float32)
    exp = (np.tile(np.array([0, 1], np.int32), (3, 1)), np.zeros((3, 2), np.float32))
    out.append(_case("field_extremes-zeros", q, t, SIFT_BF, NORM_L2, MODE_L2P, expect=exp))
    # (ii) q = all 127 (|q| ~ 1436.8), t rows of norm <= 11.2: the largest fields (d^2 ~ 2^21 - 32k)
    rng = np.random.default_rng(5)
    t = np.zeros((70, 128), np.float32)
    for i in range(70):
        a, b = rng.integers(0, 128, 2)
        t[i, a] = rng.integers(0, 9)
        t[i, b] = rng.integers(0, 8)
    t[69] = t[3]
    t[40, :] = 0
    t[40, 17], t[40, 90] = 8, 7
    out.append(_case("field_extremes-all127", np.full((2, 128), 127, np.float32), t, SIFT_BF, NORM_L2, MODE_L2P))
    # (iii) q = 0 against rows of |t|^2 up to 2^21 - 2: d^2 just under the packed limit
    top = (1 << 21) - 2
    sq = [top - k for k in rng.permutation(66)] + [top - 70, top - 70, top - 1, top - 1]
    t = np.stack([row_with_sqnorm(int(s)) for s in sq])
    out.append(_case("field_extremes-d2_limit", np.zeros((1, 128), np.float32), t, SIFT_BF, NORM_L2, MODE_L2P))
    return out


def seam_ties(fam, nt, step, swapped=False, tsplit=None, copies=2):
    """duplicates across a seam of the kernel's row layout: rows step k - 1 and
    step k (swapped: step k and step k + 1) are copies of a pattern that query k
    equals.  Both are at distance 0: the lower index must come first.  copies = 3
    adds a third copy in the row after them: knn_finish re-sorts the two
    candidates a split hands it, so the order the kernel's own merges keep
    between equal keys shows only when three tie."""
    rng = np.random.default_rng(_seed("seam", fam, nt, step, swapped))
    t = _rows(rng, fam, nt)
    pairs = [(step * k, step * k + 1) for k in range(nt) if step * k + 1 < nt] if swapped else \
            [(step * k - 1, step * k) for k in range(1, nt) if step * k < nt]
    q = _rows(rng, fam, len(pairs))            # fresh patterns: no other row equals one
    if copies == 3:
        pairs = [p for p in pairs if p[1] + 1 < nt]
        q = q[:len(pairs)]
    for k, (a, b) in enumerate(pairs):
        t[a:b + copies - 1] = q[k]
    exp = (np.array(pairs, np.int32), np.zeros((len(pairs), 2), np.float32))
    name = f"seam_ties-{fam}-{nt}-{step}" + ("-swapped" if swapped else "") + ("-triple" if copies == 3 else "")
    return _fam_case(name, fam, q, t, tsplit=tsplit, ratios=(0.7,), expect=exp)


def all_equal(fam, nt):
    rng = np.random.default_rng(_seed("eq", fam, nt))
    t = np.repeat(_rows(rng, fam, 1), nt, axis=0)
    q = _rows(rng, fam, 37)
    q[5] = t[0]
    case = _fam_case(f"all_equal-{fam}-{nt}", fam, q, t)
    d = distances_exact(case.q, case.t[:1], case.norm)
    exp = (np.tile(np.array([0, 1], np.int32), (len(q), 1)), np.repeat(d, 2, axis=1))
    return case._replace(expect=exp)


def empty_splits(fam):
    """nq = 10, nt = 5000: one query block, so the launch is split 64 ways and the
    64-row-aligned chunks leave the last splits empty.  Query 0's best two are the
    last two rows, query 1's the first row and the last."""
    rng = np.random.default_rng(_seed("empty", fam))
    t, q = _rows(rng, fam, 5000), _rows(rng, fam, 10)
    base = _rows(rng, fam, 1)[0]
    if FAMILIES[fam][0] != ORB_BF:
        base = np.clip(base, 0, 250)
    one, other = _perturb(base, fam, 1), base.copy()
    if FAMILIES[fam][0] == ORB_BF:
        other[31] ^= 1                         # one bit, not among _perturb's
    else:
        other[1] += 1
    t[4999], t[4998], t[0] = base, one, other
    q[0], q[1] = one, other
    case = _fam_case(f"empty_splits-{fam}", fam, q, t, tsplit=64)
    idx, _ = knn2_exact(case.q[:2], case.t, case.norm)
    assert idx.tolist() == [[4998, 4999], [0, 4999]]
    return case


SWEEP_NQ = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
SWEEP_NT = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 129)
SWEEP_PAIRS = tuple((SWEEP_NQ[i % 13], SWEEP_NT[i % 11]) for i in range(24))   # 13 and 11 are coprime: 24 distinct pairs


def size_sweep(fam, nq, nt):
    rng = np.random.default_rng(_seed("sweep", fam, nq, nt))
    q, t = _rows(rng, fam, nq), _rows(rng, fam, nt)
    t[nt - 1] = t[0]                           # a tie between the first row and the last
    q[nq - 1] = t[0]
    return _fam_case(f"size_sweep-{fam}-{nq}x{nt}", fam, q, t, ratios=(0.8,))


def hamming_extremes():
    rng = np.random.default_rng(256)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    na = ~a
    out = []
    # distances 0, 1, 2 and 256 with ties among them, in an order that makes every one matter
    q = np.stack([a, na, _perturb(a, "ham", 1)])
    t = np.stack([na, _perturb(a, "ham", 2), _perturb(a, "ham", 1), a, a, na, _perturb(na, "ham", 1),
                  _perturb(a, "ham", 2)])
    out.append(_case("hamming_extremes-small", q, t, ORB_BF, NORM_HAMMING, MODE_HAMP, ratios=(0.7,)))
    # two rows: the equal one after the complement; then only complements (every distance is 256,
    # and past row 1023 of a split the float key 768 + 256 + row / 1024 has crossed 1024)
    out.append(_case("hamming_extremes-equal_and_complement", a[None], np.stack([na, a]), ORB_BF, NORM_HAMMING,
                     MODE_HAMP))
    exp = (np.array([[0, 1]], np.int32), np.full((1, 2), 256, np.float32))
    out.append(_case("hamming_extremes-all_complement", a[None], np.repeat(na[None], 1100, axis=0), ORB_BF,
                     NORM_HAMMING, MODE_HAMP, expect=exp))
    return out


def hamming_extremes_65536():
    """the complement of query 0 at loc = 1023 of a split (its float key 768 + 256
    + 1023 / 1024 is the largest there is) and the equal row at loc = 0 of the
    next split; query 1 is the complement, so for it the roles swap"""
    rng = np.random.default_rng(65536)
    t = rng.integers(0, 256, (65536, 32), dtype=np.uint8)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    s = 37
    t[1024 * s + 1023] = ~a
    t[1024 * (s + 1)] = a
    t[1024 * 63 + 1023] = _perturb(a, "ham", 1)        # the last row of the last split
    t[0] = _perturb(~a, "ham", 1)
    q = np.vstack([a[None], (~a)[None], rng.integers(0, 256, (8, 32), dtype=np.uint8)])
    exp_idx = np.array([[1024 * (s + 1), 65535], [1024 * s + 1023, 0]], np.int32)
    return _case("hamming_extremes-65536", q, t, ORB_BF, NORM_HAMMING, MODE_HAMP, tsplit=64,
                 expect=(exp_idx, np.array([[0, 1], [0, 1]], np.float32)))


def l1_extremes():
    out = []
    q = np.vstack([np.zeros((1, 128)), np.full((1, 128), 255)]).astype(np.float32)
    t = np.full((3, 128), 255, np.float32)
    exp = (np.array([[0, 1], [0, 1]], np.int32), np.array([[32640, 32640], [0, 0]], np.float32))
    out.append(_case("l1_extremes-32640", q, t, SIFT_BF, NORM_L1, MODE_L1P, expect=exp))
    # distances 0 and 1 and ties across the 64-row staged tile
    rng = np.random.default_rng(64)
    t = _rows(rng, "l1", 130)
    t[:, 0] = np.minimum(t[:, 0], 250)
    t[63] = t[64] = t[20]
    t[127] = t[128] = _perturb(t[30], "l1", 1)
    q = np.stack([t[20], t[30], t[127], _perturb(t[63], "l1", 1)])
    out.append(_case("l1_extremes-tile_ties", q, t, SIFT_BF, NORM_L1, MODE_L1P, ratios=(0.7,)))
    return out


RATIO_EQ, RATIO_ABOVE = 0.75, float(np.nextafter(0.75, 1.0))


def ratio_edge(fam):
    """best and second-best distances exactly 3 and 4: 3 < 0.75 * 4 is false (the
    test is strict and evaluated in double), with the next double above 0.75 it holds"""
    rng = np.random.default_rng(_seed("ratio", fam))
    base = _rows(rng, fam, 1)[0]
    t = np.vstack([_rows(rng, fam, 40), _perturb(base, fam, 4)[None], _rows(rng, fam, 30),
                   _perturb(base, fam, 3)[None], _rows(rng, fam, 3)])
    if fam == "pk":                            # d^2 = 16 and 9 from a zero query
        base = np.zeros(128, np.float32)
        t[40], t[71] = _perturb(base, fam, 4), _perturb(base, fam, 3)
    exp = (np.array([[71, 40]], np.int32), np.array([[3, 4]], np.float32))
    return _fam_case(f"ratio_edge-{fam}", fam, base[None], t, ratios=(RATIO_EQ, RATIO_ABOVE), expect=exp)


def ratio_edge_700(fam):
    """700 queries, each with a train row at distance 3 and one at distance 4 (no
    match at ratio 0.75) or 5 (match): the survivors are exactly the queries with
    q % 3 == 0, and the compaction runs over a partial last block of 256"""
    rng = np.random.default_rng(_seed("ratio700", fam))
    q = _rows(rng, fam, 700)
    t = np.stack([_perturb(q[i // 2], fam, 3 if i % 2 == 0 else (5 if (i // 2) % 3 == 0 else 4))
                  for i in range(1400)])
    t = t[::-1].copy()                         # best at the higher index
    i = np.arange(700)
    exp = (np.stack([1399 - 2 * i, 1398 - 2 * i], 1).astype(np.int32),
           np.stack([np.full(700, 3), np.where(i % 3 == 0, 5, 4)], 1).astype(np.float32))
    return _fam_case(f"ratio_edge_700-{fam}", fam, q, t, ratios=(RATIO_EQ,), expect=exp)


# ---- the registry: name -> builder (built on first use, the big ones are 33 MB) ---

def _registry():
    reg = {}

    def one(name, fn, *a, **kw):
        reg[name] = lambda: fn(*a, **kw)

    def many(names, fn):
        for k, n in enumerate(names):
            reg[n] = (lambda k=k: fn()[k])

    for nq, nt in ((33, 65), (300, 1000)):
        one(f"mode_l2_random-{nq}x{nt}", mode_l2_random, nq, nt)
    many([f"mode_edges-{x}" for x in ("below_packed", "above_packed", "sum_2048", "above_2048")],
         functools.lru_cache(None)(mode_edges))
    one("adjacent_d2_below_2p22", adjacent_d2_below_2p22)
    for base in (SQRT_TIES_BASE, SQRT_TIES_BASE_TOP2):
        one(f"adjacent_d2_sqrt_ties-{base}", adjacent_d2_sqrt_ties, base)
    one(f"adjacent_d2_sqrt_ties-{SQRT_TIES_BASE_TOP2}-zero_only", adjacent_d2_sqrt_ties, SQRT_TIES_BASE_TOP2, True)
    many([f"field_extremes-{x}" for x in ("zeros", "all127", "d2_limit")], functools.lru_cache(None)(field_extremes))
    for sw in (False, True):
        sfx = "-swapped" if sw else ""
        for fam in ("pk", "l2", "sqrt", "ham"):
            for step in (4, 32, 64):
                nt = 200 if step < 64 else 330
                one(f"seam_ties-{fam}-{nt}-{step}{sfx}", seam_ties, fam, nt, step, sw)
            one(f"seam_ties-{fam}-200-4{sfx}-triple", seam_ties, fam, 200, 4, sw, None, 3)
        for fam in ("pk", "ham"):
            one(f"seam_ties-{fam}-65537-1024{sfx}", seam_ties, fam, 65537, 1024, sw, 65)
            one(f"seam_ties-{fam}-65536-1024{sfx}", seam_ties, fam, 65536, 1024, sw, 64)
    for fam in FAMILIES:
        for nt in (2, 5, 33, 65, 1025):
            one(f"all_equal-{fam}-{nt}", all_equal, fam, nt)
        one(f"empty_splits-{fam}", empty_splits, fam)
        for nq, nt in SWEEP_PAIRS:
            one(f"size_sweep-{fam}-{nq}x{nt}", size_sweep, fam, nq, nt)
    many([f"hamming_extremes-{x}" for x in ("small", "equal_and_complement", "all_complement")],
         functools.lru_cache(None)(hamming_extremes))
    one("hamming_extremes-65536", hamming_extremes_65536)
    many(["l1_extremes-32640", "l1_extremes-tile_ties"], functools.lru_cache(None)(l1_extremes))
    for fam in ("pk", "l1", "ham"):
        one(f"ratio_edge-{fam}", ratio_edge, fam)
        one(f"ratio_edge_700-{fam}", ratio_edge_700, fam)
    return reg


REGISTRY = _registry()
NAMES = tuple(REGISTRY)
BIG = tuple(n for n in NAMES if "-6553" in n)
# the cases every kernel variant runs in a process of its own (test_knn_gpu.py)
VARIANT_PREFIXES = ("size_sweep", "seam_ties", "all_equal", "field_extremes", "hamming_extremes", "empty_splits",
                    "ratio_edge")
VARIANT_NAMES = tuple(n for n in NAMES if n.startswith(VARIANT_PREFIXES))


@functools.lru_cache(maxsize=4)
def _build_big(name):
    return REGISTRY[name]()


def get(name):
    """the named case (the 65536-row ones are kept for the next few uses)"""
    c = _build_big(name) if name in BIG else REGISTRY[name]()
    assert c.name == name, (c.name, name)
    return c


# ---- child process: run cases through the library, record what it returned --------

def run_case(slamhip, ctx, case):
    """(idx, dist, [mode, tsplit, variant], {ratio: matches}) from the library"""
    idx, dist = slamhip.knnMatch2(case.q, case.t, case.matcher, norm=case.norm, ctx=ctx)
    launch = slamhip.lastKnnLaunch(ctx)
    matches = {r: slamhip.matchFeatures(case.q, case.t, case.matcher, r, norm=case.norm, ctx=ctx)
               for r in case.ratios}
    return idx, dist, np.array(launch, np.int32), matches


def main(argv):
    out_path, names = argv[1], argv[2:] or list(VARIANT_NAMES)
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "slam-indoor-code_amd"))
    import slamhip
    ctx = slamhip.Context(0)
    res = {}
    for k, name in enumerate(names):
        case = get(name)
        idx, dist, launch, matches = run_case(slamhip, ctx, case)
        res[f"{k}.idx"], res[f"{k}.dist"], res[f"{k}.launch"] = idx, dist, launch
        for j, r in enumerate(case.ratios):
            res[f"{k}.m{j}"] = matches[r]
    ctx.close()
    np.savez(out_path, names=np.array(names), **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

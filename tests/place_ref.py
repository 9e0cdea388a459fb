"""The contract of place recognition (numpy, the definition): a flat visual
vocabulary, tf-idf bag-of-words vectors, their score, the top-k and loop detection.

All arithmetic is integer except the one IEEE division of a score, so the device
kernels (csrc/place.hip), the host twins (csrc/place_host.cpp) and this file agree
bit for bit.  Kinds: "sift" rows of 128 u8 by squared L2, "orb" rows of 32 bytes by
Hamming distance.  Also the shared case lists of tests/test_place.py and
tests/test_place_gpu.py.
"""
import functools

import numpy as np

from slamhip.place import idf  # noqa: F401  (the one shared function: the only logarithm)

SIFT, ORB = "sift", "orb"
BYTES = {SIFT: 128, ORB: 32}
FULL_RANGE_D2 = 128 * 255 * 255     # 8 323 200


def distances(desc, cent, kind):
    """(n, K) int64 distance matrix"""
    if kind == SIFT:
        x, c = desc.astype(np.int64), cent.astype(np.int64)
        return (x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2 * (x @ c.T)
    a = np.unpackbits(desc, axis=1).astype(np.int64)
    b = np.unpackbits(cent, axis=1).astype(np.int64)
    return a @ (1 - b).T + (1 - a) @ b.T


def assign(desc, cent, kind=SIFT):
    """(word i32[n], dist i32[n]): the nearest centroid, ties to the lowest index"""
    desc, cent = np.asarray(desc, np.uint8), np.asarray(cent, np.uint8)
    word, dist = np.zeros(len(desc), np.int32), np.zeros(len(desc), np.int32)
    for lo in range(0, len(desc), 4096):
        d = distances(desc[lo:lo + 4096], cent, kind)
        w = d.argmin(axis=1)             # the first minimum: the lowest centroid index
        word[lo:lo + 4096] = w
        dist[lo:lo + 4096] = d[np.arange(len(w)), w]
    return word, dist


def update(desc, word, cent, kind):
    """one Lloyd update: the new centroids (an empty cluster keeps its own)"""
    new = cent.copy()
    for c in range(len(cent)):
        rows = desc[word == c]
        n = len(rows)
        if n == 0:
            continue
        if kind == SIFT:
            S = rows.astype(np.int64).sum(0)
            new[c] = ((2 * S + n) // (2 * n)).astype(np.uint8)
        else:
            ones = np.unpackbits(rows, axis=1, bitorder="little").astype(np.int64).sum(0)
            new[c] = np.packbits((2 * ones > n).astype(np.uint8), bitorder="little")
    return new


def train(desc, K, iters, kind=SIFT):
    """Lloyd's algorithm in integers: (cent (K, B) u8, iters_run)"""
    desc = np.asarray(desc, np.uint8)
    N = len(desc)
    cent = desc[[(c * N) // K for c in range(K)]].copy()
    run = 0
    while run < iters:
        word, _ = assign(desc, cent, kind)
        new = update(desc, word, cent, kind)
        run += 1
        same = np.array_equal(new, cent)
        cent = new
        if same:
            break
    return cent, run


def histogram(word, offsets, K):
    """per-image counts (m, K) i32; at most 65535 descriptors per image"""
    m = len(offsets) - 1
    h = np.zeros((m, K), np.int32)
    for r in range(m):
        assert 0 <= offsets[r + 1] - offsets[r] <= 65535
        h[r] = np.bincount(word[offsets[r]:offsets[r + 1]], minlength=K)
    return h


def vector(h, w):
    """(v u32 (m, K) = h w, A u64 (m) = sum v)"""
    v = np.asarray(h, np.int64) * np.asarray(w, np.int64)[None, :]
    assert v.max(initial=0) <= 1 << 26
    return v.astype(np.uint32), v.sum(1).astype(np.uint64)


def score(a, A, b, B):
    """one pair: num = sum_k min(a_k B, b_k A) in int64, one division"""
    A, B = int(A), int(B)
    if A == 0 or B == 0:
        return 0.0
    num = int(np.minimum(a.astype(np.int64) * B, b.astype(np.int64) * A).sum())
    assert num <= A * B <= 1 << 52
    return np.float64(num) / (np.float64(A) * np.float64(B))


def scores(q, qt, db, dbt):
    out = np.zeros((len(q), len(db)), np.float64)
    for i in range(len(q)):
        for r in range(len(db)):
            out[i, r] = score(q[i], qt[i], db[r], dbt[r])
    return out


def topk(s, first, last, k):
    """rows [first, last) of one score row by (score descending, index ascending), padded"""
    assert k <= 32
    order = sorted(range(first, last), key=lambda i: (-s[i], i))[:k]
    idx = np.full(k, -1, np.int32)
    out = np.zeros(k, np.float64)
    idx[:len(order)] = order
    out[:len(order)] = [s[i] for i in order]
    return idx, out


def detect(vec, tot, gap=10, k=4, alpha=0.3):
    """rows (i, j, score): for keyframe i with ref = score(i, i - 1) > 0, the top-k of rows
    [0, i - gap + 1) whose score is >= alpha ref"""
    out = []
    for i in range(1, len(vec)):
        ref = score(vec[i], tot[i], vec[i - 1], tot[i - 1])
        last = i - gap + 1
        if not ref > 0 or last <= 0:
            continue
        s = np.array([score(vec[i], tot[i], vec[j], tot[j]) for j in range(last)])
        idx, sc = topk(s, 0, last, k)
        out += [(i, int(j), float(v)) for j, v in zip(idx, sc) if j >= 0 and v >= alpha * ref]
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes()


# ---- the shared case lists ----------------------------------------------------------------------

ASSIGN_SHAPES = [(1, 1), (63, 2), (64, 31), (65, 64), (257, 65), (1000, 300)]
ASSIGN_SPECIAL = ["dup", "equal", "zeros_vs_255", "255_vs_zeros", "last_row"]
ASSIGN_NAMES = [f"noise_{n}x{k}" for n, k in ASSIGN_SHAPES] + ASSIGN_SPECIAL
TRAIN_CASES = {"k_gt_n": (5, 8, 10), "n_eq_k": (64, 64, 10), "n300_k7": (300, 7, 10), "n1000_k65": (1000, 65, 4),
               "one_iter": (300, 7, 1)}


def _noise(rng, n, kind):
    return rng.integers(0, 256, (n, BYTES[kind]), dtype=np.uint8)


def _blobs(rng, n, nc, kind):
    """n points around nc centres: Lloyd has something to move"""
    centres = _noise(rng, nc, kind)
    pick = centres[rng.integers(0, nc, n)]
    if kind == SIFT:
        return np.clip(pick.astype(np.int32) + rng.integers(-40, 41, pick.shape), 0, 255).astype(np.uint8)
    flip = (rng.random((n, 256)) < 0.15).astype(np.uint8)
    return pick ^ np.packbits(flip, axis=1)


@functools.lru_cache(maxsize=None)
def assign_case(name, kind):
    """(desc, cent, (word, dist)) of one named case; computed once, shared, never written to"""
    rng = np.random.default_rng(sum(map(ord, name + kind)))
    B = BYTES[kind]
    if name.startswith("noise_"):
        n, k = map(int, name[6:].split("x"))
        desc, cent = _noise(rng, n, kind), _noise(rng, k, kind)
    elif name == "dup":
        desc, cent = _noise(rng, 100, kind), _noise(rng, 40, kind)
        cent[7] = cent[3]
        desc[:10] = cent[3]
    elif name == "equal":
        cent = _noise(rng, 50, kind)
        desc = cent.copy()
    elif name == "zeros_vs_255":
        desc, cent = np.zeros((70, B), np.uint8), np.full((33, B), 255, np.uint8)
    elif name == "255_vs_zeros":
        desc, cent = np.full((70, B), 255, np.uint8), np.zeros((33, B), np.uint8)
    elif name == "last_row":
        cent = _noise(rng, 128, kind)
        desc = np.repeat(cent[127:128], 130, axis=0)
        desc[1::2, 5] ^= 1           # every other one a step away: still nearest to row 127
    else:
        raise KeyError(name)
    for a in (desc, cent):
        a.setflags(write=False)
    want = assign(desc, cent, kind)
    for a in want:
        a.setflags(write=False)
    return desc, cent, want


@functools.lru_cache(maxsize=None)
def train_case(name, kind):
    """(desc, K, iters, (cent, iters_run))"""
    n, K, iters = TRAIN_CASES[name]
    rng = np.random.default_rng(1000 + sum(map(ord, name + kind)))
    if name == "n_eq_k":
        desc = _noise(rng, n, kind)             # distinct points, one per centroid
    else:
        desc = _blobs(rng, n, max(2, min(K, 12)), kind)
    desc.setflags(write=False)
    cent, run = train(desc, K, iters, kind)
    cent.setflags(write=False)
    return desc, K, iters, (cent, run)


BOW_SHAPES = [(m, K) for m in (1, 2, 65) for K in (1, 64, 300)]
# the last K whose histogram and query tile fit 64 KB of LDS, and the first ones that do not (with and
# without 16-byte rows)
BOW_EDGE_SHAPES = [(3, 16384), (3, 16385), (9, 16388)]


@functools.lru_cache(maxsize=None)
def bow_case(m, K):
    """(word, offsets, weights, (vec, total, scores m x m)): image 1 (when present) is empty,
    images 3 and 4 repeat image 2's words (exact score ties)"""
    rng = np.random.default_rng(77 + 1000 * m + K)
    counts = rng.integers(1, 40, m)
    if m > 1:
        counts[1] = 0
    words = [rng.integers(0, K, c).astype(np.int32) for c in counts]
    if m > 4:
        words[3] = words[2].copy()
        words[4] = words[2][::-1].copy()
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int32)
    word = np.concatenate(words).astype(np.int32)
    weights = rng.integers(0, 1024, K).astype(np.int32)
    if K > 2:
        weights[1] = 0
        weights[2] = 1023
    vec, tot = vector(histogram(word, offsets, K), weights)
    s = scores(vec, tot, vec, tot)
    for a in (word, offsets, weights, vec, tot, s):
        a.setflags(write=False)
    return word, offsets, weights, (vec, tot, s)


def limit_case():
    """65535 descriptors in word 0 with weight 1023: v = A = 67 042 305 <= 2^26, num = A^2 < 2^52;
    the second image spreads 65535 descriptors over two words"""
    K = 4
    word = np.concatenate([np.zeros(65535, np.int32), np.zeros(30000, np.int32), np.full(35535, 3, np.int32)])
    offsets = np.array([0, 65535, 131070], np.int32)
    weights = np.array([1023, 5, 0, 1023], np.int32)
    return word, offsets, weights

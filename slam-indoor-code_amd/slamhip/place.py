"""Place recognition: a flat visual vocabulary, bag-of-words retrieval and loop
detection (csrc/place.hip; the contract is tests/place_ref.py).

All arithmetic is integer except the one IEEE division of a score, so the device
(ctx), the host twins (host=True) and the reference agree bit for bit.  Host
arrays in give host arrays out; torch device tensors in (u8 descriptors, int32
words and vectors, int64 totals: the bits of the library's u32 / u64) give device
tensors out.

    voc = Vocabulary.train(desc_list, K=4096)
    db = Database(voc)
    for d in desc_list: db.add(d)
    ids, scores = db.query(desc, k=4)
    loops = detect_loops(db, gap=10, k=4, alpha=0.3)
"""
import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib as L
from ._lib import check, lib, ptr

SIFT, ORB = "sift", "orb"
_KIND = {SIFT: L.VOC_SIFT, ORB: L.VOC_ORB, L.VOC_SIFT: L.VOC_SIFT, L.VOC_ORB: L.VOC_ORB}
_BYTES = {L.VOC_SIFT: 128, L.VOC_ORB: 32}
MAX_PER_IMAGE = 65535
MAX_WEIGHT = 1023
MAX_TOPK = 32
MIN_PAIR_MATCHES = 8        # fewer matched points cannot give an essential matrix


def _kind(kind):
    if kind not in _KIND:
        raise ValueError('kind: "sift" or "orb"')
    return _KIND[kind]


def _is_dev(a):
    return not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")


def _dp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _handle(ctx):
    from .api import default_context
    return (ctx or default_context()).handle


def _sync():
    import torch
    torch.cuda.synchronize()      # the library runs on its own stream: torch's writes must have landed


def descriptors_u8(desc, kind=SIFT):
    """(n, B) uint8 rows of a descriptor matrix: u8 as it is, or the CV_32F integer values
    0..255 that extractDescriptor emits for SIFT, converted (anything else raises)."""
    B = _BYTES[_kind(kind)]
    if _is_dev(desc):
        import torch
        if desc.dtype != torch.uint8:
            raise TypeError("device descriptors are uint8")
        return desc.reshape(-1, B).contiguous()
    a = np.asarray(desc)
    if a.size == 0:
        return np.zeros((0, B), np.uint8)
    if a.dtype != np.uint8:
        if _kind(kind) != L.VOC_SIFT or a.dtype.kind != "f":
            raise TypeError("descriptors are uint8 (or float SIFT values 0..255)")
        u = a.astype(np.uint8)
        if not np.array_equal(u.astype(a.dtype), a):
            raise ValueError("float SIFT descriptors must hold the integers 0..255")
        a = u
    if a.ndim != 2 or a.shape[1] != B:
        raise ValueError(f"{kind} descriptors are n x {B}")
    return np.ascontiguousarray(a)


def idf(hists):
    """w_k = 0 when no image has word k, else floor(64 ln(M / n_k) + 0.5) with n_k the
    number of images that contain word k of M: int32 in [0, 1023].  The one place a
    logarithm is taken (the library receives w)."""
    h = np.asarray(hists)
    M = h.shape[0]
    nk = (h > 0).sum(axis=0)
    w = np.zeros(h.shape[1], np.int32)
    for k in np.flatnonzero(nk):
        w[k] = min(MAX_WEIGHT, int(math.floor(64.0 * math.log(M / int(nk[k])) + 0.5)))
    return w


# ---- the primitives ------------------------------------------------------------------------

def assign(desc, cent, kind=SIFT, ctx=None, host=False):
    """(word int32[n], dist int32[n]): the nearest centroid of every descriptor (squared L2 for
    SIFT, Hamming for ORB), ties to the lowest centroid index."""
    kd = _kind(kind)
    d, c = descriptors_u8(desc, kind), descriptors_u8(cent, kind)
    n, K = len(d), len(c)
    if _is_dev(d) != _is_dev(c):
        raise TypeError("descriptors and centroids: both host arrays or both device tensors")
    if _is_dev(d):
        import torch
        word = torch.empty(n, dtype=torch.int32, device=d.device)
        dist = torch.empty(n, dtype=torch.int32, device=d.device)
        _sync()
        h = _handle(ctx)
        check(lib().slam_voc_assign_dev(h, None, _dp(d), n, _dp(c), K, kd, _dp(word), _dp(dist)), h)
        return word, dist
    word, dist = np.empty(n, np.int32), np.empty(n, np.int32)
    if host:
        check(lib().slam_voc_assign_host(ptr(d), n, ptr(c), K, kd, ptr(word), ptr(dist)))
    else:
        h = _handle(ctx)
        check(lib().slam_voc_assign(h, ptr(d), n, ptr(c), K, kd, ptr(word), ptr(dist)), h)
    return word, dist


def train(desc, K, iters=10, kind=SIFT, ctx=None, host=False):
    """Lloyd's algorithm in integers (slam_voc_train): (centroids (K, B) uint8, iterations run)."""
    kd = _kind(kind)
    d = descriptors_u8(desc, kind)
    n, K, iters = len(d), int(K), int(iters)
    run = ctypes.c_int32(0)
    if _is_dev(d):
        import torch
        cent = torch.empty((max(K, 0), _BYTES[kd]), dtype=torch.uint8, device=d.device)
        _sync()
        h = _handle(ctx)
        check(lib().slam_voc_train_dev(h, None, _dp(d), n, K, iters, kd, _dp(cent), ctypes.byref(run)), h)
        return cent, int(run.value)
    cent = np.empty((max(K, 0), _BYTES[kd]), np.uint8)
    if host:
        check(lib().slam_voc_train_host(ptr(d), n, K, iters, kd, ptr(cent), ctypes.byref(run)))
    else:
        h = _handle(ctx)
        check(lib().slam_voc_train(h, ptr(d), n, K, iters, kd, ptr(cent), ctypes.byref(run)), h)
    return cent, int(run.value)


def vectors(word, offsets, weights, ctx=None, host=False):
    """tf-idf vectors of m images: image r owns word[offsets[r]:offsets[r + 1]].  Returns
    (vec (m, K) uint32, total (m) uint64) with vec = counts * weights and total its row sum."""
    off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
    w = np.ascontiguousarray(weights, np.int32).reshape(-1)
    m, K = len(off) - 1, len(w)
    if m < 0:
        raise ValueError("offsets holds m + 1 values")
    if _is_dev(word):
        import torch
        if word.dtype != torch.int32:
            raise TypeError("device words are int32")
        word = word.contiguous()
        if m > 0 and off.max() > word.numel():
            raise ValueError("offsets run past the words")
        vec = torch.empty((m, K), dtype=torch.int32, device=word.device)
        tot = torch.empty(m, dtype=torch.int64, device=word.device)
        _sync()
        h = _handle(ctx)
        check(lib().slam_bow_vectors_dev(h, None, _dp(word), ptr(off), m, ptr(w), K, _dp(vec), _dp(tot)), h)
        return vec, tot
    wd = np.ascontiguousarray(word, np.int32).reshape(-1)
    if m > 0 and off.max() > len(wd):
        raise ValueError("offsets run past the words")
    vec, tot = np.empty((m, K), np.uint32), np.empty(m, np.uint64)
    if host:
        check(lib().slam_bow_vectors_host(ptr(wd), ptr(off), m, ptr(w), K, ptr(vec), ptr(tot)))
    else:
        h = _handle(ctx)
        check(lib().slam_bow_vectors(h, ptr(wd), ptr(off), m, ptr(w), K, ptr(vec), ptr(tot)), h)
    return vec, tot


def _vec2(a, t, dev):
    if dev:
        return a.reshape(-1, a.shape[-1]).contiguous(), t.reshape(-1).contiguous()
    a = np.ascontiguousarray(a, np.uint32)
    return a.reshape(-1, a.shape[-1]), np.ascontiguousarray(t, np.uint64).reshape(-1)


def score(q, qtotal, db, dbtotal, ctx=None, host=False):
    """scores (nq, m) float64 of the query vectors against the database rows: the histogram
    intersection of the L1-normalised vectors, 0.0 against an empty image."""
    dev = _is_dev(db)
    if dev != _is_dev(q):
        raise TypeError("queries and database: both host arrays or both device tensors")
    q, qt = _vec2(q, qtotal, dev)
    b, bt = _vec2(db, dbtotal, dev)
    nq, m, K = len(q), len(b), q.shape[1]
    if b.shape[1] != K or len(qt) != nq or len(bt) != m:
        raise ValueError("score: vectors of one K with one total each")
    if dev:
        import torch
        out = torch.empty((nq, m), dtype=torch.float64, device=b.device)
        _sync()
        h = _handle(ctx)
        check(lib().slam_bow_score_dev(h, None, _dp(q), _dp(qt), nq, _dp(b), _dp(bt), m, K, _dp(out)), h)
        return out
    out = np.empty((nq, m), np.float64)
    if host:
        check(lib().slam_bow_score_host(ptr(q), ptr(qt), nq, ptr(b), ptr(bt), m, K, ptr(out)))
        return out
    # the device's scores through slam_bow_query's staging would drop the matrix: score on device tensors
    import torch
    t = lambda a, dt: torch.from_numpy(a.view(dt).copy()).cuda()
    return score(t(q, np.int32), t(qt, np.int64), t(b, np.int32), t(bt, np.int64), ctx=ctx).cpu().numpy()


def topk(scores, first, last, k, ctx=None, host=False):
    """The k best columns of [first, last) of every row of `scores` by (score descending, index
    ascending): (idx (nq, k) int32, score (nq, k) float64), padded with -1 and 0.0."""
    first, last, k = int(first), int(last), int(k)
    if _is_dev(scores):
        import torch
        s = scores.reshape(-1, scores.shape[-1]).contiguous()
        nq, m = s.shape
        idx = torch.empty((nq, k), dtype=torch.int32, device=s.device)
        out = torch.empty((nq, k), dtype=torch.float64, device=s.device)
        _sync()
        h = _handle(ctx)
        check(lib().slam_bow_topk_dev(h, None, _dp(s), nq, m, first, last, k, _dp(idx), _dp(out)), h)
        return idx, out
    s = np.ascontiguousarray(scores, np.float64)
    s = s.reshape(-1, s.shape[-1])
    if host:
        nq, m = s.shape
        if not (0 <= first <= last <= m and 1 <= k <= MAX_TOPK):
            raise L.SlamError(L.SLAM_E_INVALID_ARG, "topk: 0 <= first <= last <= m and 1 <= k <= 32")
        idx, out = np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.float64)
        cols = np.arange(first, last)
        for i in range(nq):
            order = cols[np.lexsort((cols, -s[i, first:last]))][:k]
            idx[i, :len(order)] = order
            out[i, :len(order)] = s[i, order]
        return idx, out
    import torch
    idx, out = topk(torch.from_numpy(s).cuda(), first, last, k, ctx=ctx)
    return idx.cpu().numpy(), out.cpu().numpy()


def query(q, qtotal, db, dbtotal, k, first=0, last=None, ctx=None, host=False):
    """score + top-k of host vectors in one library call (slam_bow_query); with host=True the twins."""
    q, qt = _vec2(q, qtotal, False)
    b, bt = _vec2(db, dbtotal, False)
    nq, m, K = len(q), len(b), q.shape[1]
    last = m if last is None else int(last)
    if host:
        return topk(score(q, qt, b, bt, host=True), first, last, k, host=True) if m else \
            (np.full((nq, k), -1, np.int32), np.zeros((nq, k)))
    idx, out = np.empty((nq, int(k)), np.int32), np.empty((nq, int(k)), np.float64)
    h = _handle(ctx)
    check(lib().slam_bow_query(h, ptr(q), ptr(qt), nq, ptr(b), ptr(bt), m, K, int(first), last, int(k), ptr(idx),
                               ptr(out)), h)
    return idx, out


# ---- vocabulary and database ---------------------------------------------------------------

class Vocabulary:
    """K centroids of one descriptor kind and the idf weight of every word."""

    def __init__(self, centroids, weights, kind=SIFT):
        self.kind = SIFT if _kind(kind) == L.VOC_SIFT else ORB
        self.centroids = descriptors_u8(np.asarray(centroids), self.kind)
        self.weights = np.ascontiguousarray(weights, np.int32).reshape(-1)
        if len(self.weights) != len(self.centroids) or len(self.centroids) < 1:
            raise ValueError("one weight per centroid")
        if self.weights.min() < 0 or self.weights.max() > MAX_WEIGHT:
            raise ValueError("weights are in [0, 1023]")

    @property
    def K(self):
        return len(self.centroids)

    @classmethod
    def train(cls, desc_list, K, iters=10, kind=SIFT, ctx=None, host=False):
        """Lloyd's algorithm over the descriptors of all images, then the idf weights from the
        images' own histograms."""
        per = [descriptors_u8(d, kind) for d in desc_list]
        if any(_is_dev(d) for d in per):
            raise TypeError("Vocabulary.train takes host descriptor arrays")
        allv = np.concatenate(per) if per else np.zeros((0, _BYTES[_kind(kind)]), np.uint8)
        cent, _ = train(allv, K, iters, kind, ctx=ctx, host=host)
        word, _ = assign(allv, cent, kind, ctx=ctx, host=host)
        off = np.concatenate([[0], np.cumsum([len(d) for d in per])]).astype(np.int32)
        hists, _ = vectors(word, off, np.ones(int(K), np.int32), ctx=ctx, host=host)
        return cls(cent, idf(hists), kind)

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, centroids=self.centroids, weights=self.weights, kind=np.array(self.kind))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(z["centroids"], z["weights"], str(z["kind"]))

    def transform_batch(self, desc_list, ctx=None, host=False):
        """(vec (m, K) uint32, total (m) uint64) of m images' descriptors."""
        per = [descriptors_u8(d, self.kind) for d in desc_list]
        if any(len(d) > MAX_PER_IMAGE for d in per):
            raise L.SlamError(L.SLAM_E_INVALID_ARG, "at most 65535 descriptors per image")
        allv = np.concatenate(per) if per else np.zeros((0, _BYTES[_kind(self.kind)]), np.uint8)
        word, _ = assign(allv, self.centroids, self.kind, ctx=ctx, host=host)
        off = np.concatenate([[0], np.cumsum([len(d) for d in per])]).astype(np.int32)
        return vectors(word, off, self.weights, ctx=ctx, host=host)

    def transform(self, desc, ctx=None, host=False):
        """(vec (K) uint32, total int) of one image."""
        v, t = self.transform_batch([desc], ctx=ctx, host=host)
        return v[0], int(t[0])


class Database:
    """The tf-idf vectors of the keyframes added so far: rows on the device (grown by
    doubling), or in host memory with host=True."""

    def __init__(self, vocab, ctx=None, host=False, capacity=64):
        self.vocab, self.ctx, self.host = vocab, ctx, bool(host)
        self.m = 0
        self._cap = 0
        self._rows = self._tot = None
        self._grow(max(1, int(capacity)))

    def __len__(self):
        return self.m

    def _grow(self, cap):
        K = self.vocab.K
        if self.host:
            rows, tot = np.zeros((cap, K), np.uint32), np.zeros(cap, np.uint64)
        else:
            import torch
            rows = torch.zeros((cap, K), dtype=torch.int32, device="cuda")
            tot = torch.zeros(cap, dtype=torch.int64, device="cuda")
        if self.m:
            rows[:self.m] = self._rows[:self.m]
            tot[:self.m] = self._tot[:self.m]
        self._rows, self._tot, self._cap = rows, tot, cap

    def add_vector(self, vec, total):
        if self.m == self._cap:
            self._grow(2 * self._cap)
        v = np.ascontiguousarray(vec, np.uint32).reshape(-1)
        if self.host:
            self._rows[self.m] = v
            self._tot[self.m] = total
        else:
            import torch
            self._rows[self.m] = torch.from_numpy(v.view(np.int32)).to(self._rows.device)
            self._tot[self.m] = int(total)
        self.m += 1
        return self.m - 1

    def add(self, desc):
        """quantise one image's descriptors and append its vector: the new row's id"""
        v, t = self.vocab.transform(desc, ctx=self.ctx, host=self.host)
        return self.add_vector(v, t)

    def rows(self):
        """the m stored vectors and totals (device tensors, or host arrays with host=True)"""
        return self._rows[:self.m], self._tot[:self.m]

    def vectors(self):
        """host copies: (vec (m, K) uint32, total (m) uint64)"""
        r, t = self.rows()
        if self.host:
            return r.copy(), t.copy()
        return r.cpu().numpy().view(np.uint32), t.cpu().numpy().view(np.uint64)

    def query(self, desc, k, last=None):
        """(ids int32[k], scores float64[k]): the k best rows of [0, last) (all when None) for
        one image's descriptors, padded with -1 / 0.0."""
        v, t = self.vocab.transform(desc, ctx=self.ctx, host=self.host)
        last = self.m if last is None else int(last)
        r, rt = self.rows()
        if self.host:
            s = score(v[None], np.array([t], np.uint64), r, rt, host=True)
            idx, out = topk(s, 0, last, k, host=True) if self.m else (np.full((1, k), -1, np.int32), np.zeros((1, k)))
            return idx[0], out[0]
        import torch
        if self.m == 0:
            return np.full(k, -1, np.int32), np.zeros(k)
        qv = torch.from_numpy(np.ascontiguousarray(v).view(np.int32)[None]).to(r.device)
        qt = torch.tensor([t], dtype=torch.int64, device=r.device)
        idx, out = topk(score(qv, qt, r, rt, ctx=self.ctx), 0, last, k, ctx=self.ctx)
        return idx[0].cpu().numpy(), out[0].cpu().numpy()


# ---- loop detection ------------------------------------------------------------------------

def detect_loops(vectors_or_db, gap=10, k=4, alpha=0.3, ctx=None, host=False):
    """Loop candidates of every keyframe i against the rows [0, i - gap + 1): with ref_i =
    score(i, i - 1) > 0, the top-k rows whose score is >= alpha ref_i (DLoopDetector's
    normalisation).  `vectors_or_db`: (vec, total) or a Database.  Returns [(i, j, score)]."""
    if isinstance(vectors_or_db, Database):
        db = vectors_or_db
        vec, tot = db.rows()
        ctx, host = db.ctx, db.host
    else:
        vec, tot = vectors_or_db
        if not _is_dev(vec):
            vec, tot = _vec2(vec, tot, False)
            if not host:
                import torch
                vec = torch.from_numpy(vec.view(np.int32)).cuda()
                tot = torch.from_numpy(tot.view(np.int64)).cuda()
    m = len(vec)
    gap, k = int(gap), int(k)
    if gap < 1:
        raise ValueError("gap >= 1")
    out = []
    if m < 2:
        return out
    s = score(vec, tot, vec, tot, ctx=ctx, host=host)
    sh = s if isinstance(s, np.ndarray) else s.cpu().numpy()
    for i in range(1, m):
        ref, last = float(sh[i, i - 1]), i - gap + 1
        if not ref > 0.0 or last <= 0:
            continue
        idx, sc = topk(s[i:i + 1], 0, last, k, ctx=ctx, host=host)
        if not isinstance(idx, np.ndarray):
            idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
        for j, v in zip(idx[0], sc[0]):
            if j >= 0 and v >= alpha * ref:
                out.append((i, int(j), float(v)))
    return out


def verify_loop(frame_i, kps_i, desc_i, frame_j, kps_j, desc_j, K, cond, ops):
    """Geometric check of a loop candidate with the pipeline's own steps: the ratio-test match
    of frame i's descriptors against frame j (ops.match_frame, which describes frame j's
    keypoints as the cycle does; desc_j only says whether there is anything to match) and
    ops.estimate_transformation.  Returns (n_matches, n_inliers, R, t): t is up to scale,
    R and t are None when no model was found."""
    from .cycle import key_point_coords
    if len(desc_i) == 0 or len(desc_j) == 0:
        return 0, 0, None, None
    kj, matches = ops.match_frame(desc_i, frame_j, kps_j, cond.matcherType, cond.knnMatcherDistance)
    n = len(matches)
    if n < MIN_PAIR_MATCHES:
        return n, 0, None, None
    p1, p2 = key_point_coords(kps_i, kj, matches)
    ok, R, t, chir = ops.estimate_transformation(p1, p2, K, cond.rpUseRansac, cond.rpProb, cond.rpThreshold,
                                                 cond.rpDistance)
    if R is None:
        return n, 0, None, None
    return (n, int((np.asarray(chir, np.uint8) > 0).sum()), np.array(R, np.float64).reshape(3, 3),
            np.array(t, np.float64).reshape(3))


@dataclass
class LoopParams:
    """slam_main(loops=...): K words trained for `iters` iterations on the run's own keyframes
    (or the vocabulary loaded from the .npz `vocabulary`), candidates by detect_loops(gap, k,
    alpha), kept when verify_loop finds at least min_inliers.  close=True adds the loop-closing
    stage (loopclose.close_loops over the kept loops): `hypotheses` RANSAC hypotheses per loop,
    the angular inlier threshold `tau`, at least `min_pairs` pairs and inliers per accepted loop,
    the optimiser's caps `max_lm` / `max_pcg` and the weight of a loop edge.  global_ba=True (with close)
    then re-fits the closed map to the pixels (globalba.refine_closed): the loss `gba_loss` (0 squares,
    1 Huber with `gba_loss_param` pixels), the caps `gba_max_lm` / `gba_max_pcg`, the least depth `gba_zmin`."""
    K: int = 4096
    iters: int = 10
    gap: int = 10
    k: int = 4
    alpha: float = 0.3
    min_inliers: int = 30
    vocabulary: Optional[str] = None
    close: bool = False
    hypotheses: int = 256
    tau: float = 0.01
    min_pairs: int = 30
    max_lm: int = 10
    max_pcg: int = 400
    loop_weight: float = 1.0
    global_ba: bool = False
    gba_loss: int = 0
    gba_loss_param: float = 1.0
    gba_max_lm: int = 10
    gba_max_pcg: int = 200
    gba_zmin: float = 0.1


def find_loops(frames, K, cond, ops, prm, ctx=None, host=False):
    """The loop stage over the kept good frames: describe, train or load the vocabulary, build
    the database, detect and verify.  Returns [(i, j, score, n_matches, n_inliers, R, t)]."""
    kind = ORB if cond.matcherType == L.ORB_BF else SIFT
    feats = []
    for f in frames:
        kps = ops.fast(f, cond.featureExtractingThreshold)
        feats.append(ops.describe(f, kps, cond.matcherType))
    descs = [descriptors_u8(d, kind) for _, d in feats]
    if prm.vocabulary:
        voc = Vocabulary.load(prm.vocabulary)
        if voc.kind != kind:
            raise ValueError(f"vocabulary of {voc.kind} descriptors for a {kind} run")
    else:
        n = sum(len(d) for d in descs)
        if n == 0:
            return []
        voc = Vocabulary.train(descs, int(prm.K), prm.iters, kind, ctx=ctx, host=host)
    db = Database(voc, ctx=ctx, host=host)
    for d in descs:
        db.add(d)
    out = []
    for i, j, s in detect_loops(db, prm.gap, prm.k, prm.alpha):
        n, inl, R, t = verify_loop(frames[i], feats[i][0], feats[i][1], frames[j], feats[j][0], feats[j][1], K, cond, ops)
        if R is not None and inl >= prm.min_inliers:
            out.append((i, j, s, n, inl, R, t))
    return out

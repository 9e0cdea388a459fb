"""GPU tests of place recognition (csrc/place.hip): every device output against the
contract (tests/place_ref.py) by bits, between 64-element sentinels that must stay
intact; the Database across a growth step; loop detection + verification end to end
and through slam_main(loops=...).
"""
import ctypes
import os

import numpy as np
import pytest

import place_ref as R
import slamhip
from slamhip import _lib as L
from slamhip import cycle, place

pytestmark = pytest.mark.gpu

GUARD = 64
KINDS = [R.SIFT, R.ORB]
KIND_ID = {R.SIFT: L.VOC_SIFT, R.ORB: L.VOC_ORB}
MIN_INLIERS = 30        # true pairs 312 / 319 inliers, false pairs 0, at 320 x 240


def _guarded(torch, n, dtype, fill):
    """a device buffer of n elements between GUARD sentinels: (whole, payload view)"""
    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return t, t[GUARD:GUARD + n]


def _intact(t, n, fill):
    h = t.cpu()
    return bool((h[:GUARD] == fill).all()) and bool((h[GUARD + n:] == fill).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev(torch, a, dt=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dt) if dt is not None else a.copy()).cuda()


# ---- assign ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", R.ASSIGN_NAMES)
def test_assign_equals_reference(gpu_ctx, name, kind):
    import torch
    desc, cent, (word, dist) = R.assign_case(name, kind)
    n, K = len(desc), len(cent)
    d, c = _dev(torch, desc), _dev(torch, cent)
    wt, wp = _guarded(torch, n, torch.int32, -7)
    dt, dp = _guarded(torch, n, torch.int32, -7)
    torch.cuda.synchronize()
    h = gpu_ctx.handle
    L.check(L.lib().slam_voc_assign_dev(h, None, _p(d), n, _p(c), K, KIND_ID[kind], _p(wp), _p(dp)), h)
    assert R.same_bits(wp.cpu().numpy(), word) and R.same_bits(dp.cpu().numpy(), dist), name
    assert _intact(wt, n, -7) and _intact(dt, n, -7)
    # host arrays in give the same
    hw, hd = place.assign(desc, cent, kind, ctx=gpu_ctx)
    assert R.same_bits(hw, word) and R.same_bits(hd, dist)


# ---- train -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(R.TRAIN_CASES))
def test_train_equals_reference(gpu_ctx, name, kind):
    import torch
    desc, K, iters, (cent, run) = R.train_case(name, kind)
    B = R.BYTES[kind]
    d = _dev(torch, desc)
    ct, cp = _guarded(torch, K * B, torch.uint8, 0xA5)
    got = ctypes.c_int32(-1)
    torch.cuda.synchronize()
    h = gpu_ctx.handle
    # the payload starts GUARD = 64 bytes in: 16-byte aligned as the entry point asks
    L.check(L.lib().slam_voc_train_dev(h, None, _p(d), len(desc), K, iters, KIND_ID[kind], _p(cp), ctypes.byref(got)), h)
    assert got.value == run and R.same_bits(cp.cpu().numpy().reshape(K, B), cent), name
    assert _intact(ct, K * B, 0xA5)
    hc, hr = place.train(desc, K, iters, kind, ctx=gpu_ctx)
    assert hr == run and R.same_bits(hc, cent)


# ---- vectors / score / topk --------------------------------------------------------------------

@pytest.mark.parametrize("m,K", R.BOW_SHAPES + R.BOW_EDGE_SHAPES)
def test_vectors_score_topk_equal_reference(gpu_ctx, m, K):
    import torch
    word, off, w, (vec, tot, s) = R.bow_case(m, K)
    h = gpu_ctx.handle
    wd = _dev(torch, word)
    vt, vp = _guarded(torch, m * K, torch.int32, -7)
    tt, tp = _guarded(torch, m, torch.int64, -7)
    torch.cuda.synchronize()
    L.check(L.lib().slam_bow_vectors_dev(h, None, _p(wd) if len(word) else None, L.ptr(off), m, L.ptr(w), K, _p(vp), _p(tp)), h)
    assert R.same_bits(vp.cpu().numpy().reshape(m, K), vec) and R.same_bits(tp.cpu().numpy(), tot)
    assert _intact(vt, m * K, -7) and _intact(tt, m, -7)

    st, sp = _guarded(torch, m * m, torch.float64, -7.0)
    L.check(L.lib().slam_bow_score_dev(h, None, _p(vp), _p(tp), m, _p(vp), _p(tp), m, K, _p(sp)), h)
    batch = sp.cpu().numpy().reshape(m, m)
    assert R.same_bits(batch, s) and _intact(st, m * m, -7.0)
    # a batch of queries equals the single calls
    for i in sorted({0, m // 2, m - 1}):
        one = place.score(vp.reshape(m, K)[i:i + 1], tp[i:i + 1], vp.reshape(m, K), tp, ctx=gpu_ctx)
        assert R.same_bits(one.cpu().numpy()[0], s[i])

    for first, last, k in [(0, m, 4), (0, m, 32), (m, m, 3), (m // 2, m, 1), (0, max(1, m // 3), 5)]:
        it, ip = _guarded(torch, m * k, torch.int32, -7)
        ot, op = _guarded(torch, m * k, torch.float64, -7.0)
        L.check(L.lib().slam_bow_topk_dev(h, None, _p(sp), m, m, first, last, k, _p(ip), _p(op)), h)
        idx, sc = ip.cpu().numpy().reshape(m, k), op.cpu().numpy().reshape(m, k)
        for i in range(m):
            ri, rs = R.topk(s[i], first, last, k)
            assert R.same_bits(idx[i], ri) and R.same_bits(sc[i], rs), (i, first, last, k)
        assert _intact(it, m * k, -7) and _intact(ot, m * k, -7.0)

    # host arrays in: the same bits through the staged entry points
    hv, ht = place.vectors(word, off, w, ctx=gpu_ctx)
    assert R.same_bits(hv, vec) and R.same_bits(ht, tot)
    assert R.same_bits(place.score(vec, tot, vec, tot, ctx=gpu_ctx), s)
    qi, qs = place.query(vec, tot, vec, tot, 3, 0, m, ctx=gpu_ctx)
    for i in range(m):
        ri, rs = R.topk(s[i], 0, m, 3)
        assert R.same_bits(qi[i], ri) and R.same_bits(qs[i], rs)


def test_limit_case_needs_64_bits(gpu_ctx):
    """A = 65535 * 1023: num = A^2 is above 2^51; a 32-bit or f32 sum cannot give 1.0 and the
    second row's 0.4577..."""
    word, off, w = R.limit_case()
    vec, tot = R.vector(R.histogram(word, off, 4), w)
    want = R.scores(vec, tot, vec, tot)
    assert want[0, 0] == 1.0 and want[1, 1] == 1.0 and 0 < want[0, 1] < 1
    hv, ht = place.vectors(word, off, w, ctx=gpu_ctx)
    assert R.same_bits(hv, vec) and R.same_bits(ht, tot)
    assert R.same_bits(place.score(hv, ht, hv, ht, ctx=gpu_ctx), want)


def test_invalid_arguments_device(gpu_ctx):
    import torch
    h, lib = gpu_ctx.handle, L.lib()
    d = torch.zeros((4, 128), dtype=torch.uint8, device="cuda")
    o = torch.zeros(4, dtype=torch.int32, device="cuda")
    bad = L.SLAM_E_INVALID_ARG
    assert lib.slam_voc_assign_dev(h, None, _p(d), 4, _p(d), 4, 2, _p(o), _p(o)) == bad          # unknown kind
    assert lib.slam_voc_assign_dev(h, None, _p(d), 4, _p(d), 0, 0, _p(o), _p(o)) == bad
    assert lib.slam_voc_assign_dev(h, None, _p(d), 4, _p(d), 65537, 0, _p(o), _p(o)) == bad
    assert lib.slam_voc_assign_dev(h, None, _p(d), 0, _p(d), 4, 0, None, None) == L.SLAM_OK      # n = 0
    run = ctypes.c_int32(0)
    assert lib.slam_voc_train_dev(h, None, _p(d), 0, 2, 3, 0, _p(d), ctypes.byref(run)) == bad
    w = np.zeros(70000, np.int32)
    for off, wt in [([0, 65536], [1]), ([0, 5, 3], [1]), ([0, 3], [1024]), ([0, 3], [-1])]:
        with pytest.raises(L.SlamError) as e:
            place.vectors(w, off, wt, ctx=gpu_ctx)
        assert e.value.code == bad
    v, t = place.vectors(w[:0], [0, 0], [7, 7], ctx=gpu_ctx)          # an image without descriptors
    assert not v.any() and t[0] == 0
    s = torch.zeros((1, 4), dtype=torch.float64, device="cuda")
    i4 = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert lib.slam_bow_topk_dev(h, None, _p(s), 1, 4, 0, 4, 33, _p(i4), _p(s)) == bad
    assert lib.slam_bow_topk_dev(h, None, _p(s), 1, 4, 3, 2, 1, _p(i4), _p(s)) == bad
    assert lib.slam_bow_topk_dev(h, None, _p(s), 1, 4, 0, 5, 1, _p(i4), _p(s)) == bad


# ---- Database ----------------------------------------------------------------------------------

def test_database_grows_and_queries(gpu_ctx):
    rng = np.random.default_rng(9)
    imgs = [R._blobs(rng, int(rng.integers(20, 60)), 8, R.SIFT) for _ in range(70)]
    cent, _ = R.train(np.concatenate(imgs[:10]), 16, 3, R.SIFT)
    words = [R.assign(d, cent, R.SIFT)[0] for d in imgs]
    off = np.concatenate([[0], np.cumsum([len(x) for x in words])]).astype(np.int32)
    hist = R.histogram(np.concatenate(words), off, 16)
    voc = slamhip.Vocabulary(cent, R.idf(hist), "sift")
    vec, tot = R.vector(hist, voc.weights)
    db = slamhip.Database(voc, ctx=gpu_ctx, capacity=64)
    for i, d in enumerate(imgs):
        assert db.add(d) == i                   # row 64 crosses the growth step
    assert len(db) == 70 and db._cap == 128
    gv, gt = db.vectors()
    assert R.same_bits(gv, vec) and R.same_bits(gt, tot)
    s = R.scores(vec, tot, vec, tot)
    for q in (0, 33, 64, 69):
        ids, sc = db.query(imgs[q], 5)
        ri, rs = R.topk(s[q], 0, 70, 5)
        assert R.same_bits(ids, ri) and R.same_bits(sc, rs)
    ids, sc = db.query(imgs[69], 4, last=60)
    ri, rs = R.topk(s[69], 0, 60, 4)
    assert R.same_bits(ids, ri) and R.same_bits(sc, rs)
    assert place.detect_loops(db, 10, 4, 0.3) == R.detect(vec, tot, 10, 4, 0.3)


# ---- end to end --------------------------------------------------------------------------------

def _cond(**kw):
    d = slamhip.reference_example()
    d.update({"featureExtractingThreshold": 20, "useFM-SIFT-FLANN": False, "useFM-SIFT-BF": True, "useFM-ORB": False})
    d.update(kw)
    return cycle.Conditions(slamhip.ConfigService(d))


def test_place_end_to_end(gpu_ctx):
    """seven 320 x 240 keyframes: two of seed 22, two of seed 11, two of seed 33, then seed 22
    again: the last keyframe's verified loops point only at rows 0 and 1"""
    spec = [(22, 0), (22, 6), (11, 0), (11, 6), (33, 0), (33, 6), (22, 3)]
    frames = [slamhip.synth_frames(320, 240, i, 1, seed=s, path=slamhip.SYNTH_STEADY)[0] for s, i in spec]
    K = np.array([[1724.676 / 6, 0, 995.966 / 6], [0, 1730.482 / 6, 550.192 / 6], [0, 0, 1.0]])
    prm = slamhip.LoopParams(K=64, iters=10, gap=2, k=4, alpha=0.3, min_inliers=MIN_INLIERS)
    loops = place.find_loops(frames, K, _cond(), cycle.GpuOps(gpu_ctx), prm, ctx=gpu_ctx)
    print([(i, j, round(s, 4), n, inl) for i, j, s, n, inl, _, _ in loops])
    last = [l for l in loops if l[0] == 6]
    assert len(last) >= 1 and {l[1] for l in last} <= {0, 1}
    for i, j, *_ in loops:
        assert spec[i][0] == spec[j][0], (i, j)          # no loop ends in a frame of another seed


def test_slam_main_with_loops(gpu_ctx, tmp_path):
    frames = slamhip.synth_frames(640, 480, 0, 16, seed=1234)
    d = slamhip.reference_example()
    d.update({"featureExtractingThreshold": 10, "requiredExtractedPointsCount": 2000, "framesBatchSize": 4,
              "requiredMatchedPointsCount": 300, "useFM-SIFT-FLANN": False, "useFM-SIFT-BF": True, "useFM-ORB": False,
              "useBundleAdjustment": False, "BAMaxFramesCnt": 4})
    cfg = slamhip.ConfigService(d)
    K0 = np.array([[1724.676 / 3, 0, 995.966 / 3], [0, 1730.482 / 3, 550.192 / 3], [0, 0, 1.0]])
    names = ("points.txt", "poses.txt", "rotations.txt", "colors.txt")
    prm = slamhip.LoopParams(K=1024, iters=3, gap=2, k=2, alpha=0.3, min_inliers=MIN_INLIERS)

    def run(out, **kw):
        K = K0.copy()
        gd, logs = cycle.slam_main(cycle.MediaSources(list(frames)), K, cfg, cycle.GpuOps(gpu_ctx), out_dir=str(out), **kw)
        return gd, logs, K, {n: open(os.path.join(out, n), "rb").read() for n in names}

    g0, l0, _, f0 = run(tmp_path / "plain")
    g1, l1, K1, f1 = run(tmp_path / "loops", loops=prm)
    assert f0 == f1 and len(f0["poses.txt"]) > 0
    assert not os.path.exists(tmp_path / "plain" / "loops.txt") and not hasattr(g0, "loops") and l0.frames is None
    assert os.path.exists(tmp_path / "loops" / "loops.txt")
    assert len(l1.frames) == len(g1.cameraRotations) >= 3

    # by hand on the kept frames
    cond, ops = cycle.Conditions(cfg), cycle.GpuOps(gpu_ctx)
    feats = [ops.describe(f, ops.fast(f, cond.featureExtractingThreshold), cond.matcherType) for f in l1.frames]
    descs = [place.descriptors_u8(x) for _, x in feats]
    voc = slamhip.Vocabulary.train(descs, prm.K, prm.iters, "sift", ctx=gpu_ctx)
    db = slamhip.Database(voc, ctx=gpu_ctx)
    for x in descs:
        db.add(x)
    want = []
    for i, j, s in slamhip.detect_loops(db, prm.gap, prm.k, prm.alpha):
        n, inl, R_, t_ = slamhip.verify_loop(l1.frames[i], feats[i][0], feats[i][1], l1.frames[j], feats[j][0],
                                             feats[j][1], K1, cond, ops)
        if R_ is not None and inl >= prm.min_inliers:
            want.append((i, j, s, n, inl, R_, t_))
    assert len(g1.loops) == len(want)
    for a, b in zip(g1.loops, want):
        assert a[:5] == b[:5] and np.array_equal(a[5], b[5]) and np.array_equal(a[6], b[6])
    rows = [r for r in open(tmp_path / "loops" / "loops.txt").read().splitlines() if r]
    assert len(rows) == len(want) and all(len(r.split()) == 17 for r in rows)

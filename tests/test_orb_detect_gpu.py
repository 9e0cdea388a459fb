"""GPU parity of the full ORB detector (csrc/orbdet.hip; slam_orb_detect and
slam_orb_detect_batch) with its CPU definition tests/orb_detect_ref.py: every
keypoint field, the order and the descriptors byte for byte."""
import ctypes

import numpy as np
import pytest

import oracle_ffi as O
import orb_detect_ref as R
import slamhip
from slamhip import _lib as L

pytestmark = pytest.mark.gpu

_frames = {}


def frame(w, h, seed=31):
    """a textured BGR frame, made once per size"""
    key = (w, h, seed)
    if key not in _frames:
        f = slamhip.synth_frames(w, h, 0, 1, seed=seed)[0]
        f.setflags(write=False)
        _frames[key] = f
    return _frames[key]


_refs = {}


def ref(key, img, **kw):
    """the CPU definition's result, computed once per case and shared"""
    if key not in _refs:
        _refs[key] = R.detect_and_compute(img, return_levels=True, **kw)
    return _refs[key]


def same(got, want):
    gk, gd = got
    wk, wd = want[0], want[1]
    assert len(gk) == len(wk), (len(gk), len(wk))
    for name in wk.dtype.names:
        assert np.array_equal(gk[name].view(np.uint32), wk[name].view(np.uint32)), name
    assert gk.tobytes() == wk.tobytes()
    assert gd.dtype == np.uint8 and gd.shape == wd.shape and np.array_equal(gd, wd)


def periodic_256():
    """a 16-pixel-period texture: every corner repeats in every tile with the same scores"""
    rng = np.random.default_rng(11)
    tile = np.kron(rng.integers(0, 256, (4, 4)).astype(np.float64), np.ones((4, 4)))
    for _ in range(2):
        tile = (tile + np.roll(tile, 1, 0) + np.roll(tile, -1, 0) + np.roll(tile, 1, 1) + np.roll(tile, -1, 1)) / 5
    return np.ascontiguousarray(np.tile(tile.astype(np.uint8), (16, 16)))


@pytest.mark.parametrize("score", [R.HARRIS_SCORE, R.FAST_SCORE])
@pytest.mark.parametrize("wh", [(320, 240), (161, 97)])
def test_matches_ref(gpu_ctx, wh, score):
    img = frame(*wh)
    want = ref((wh, score), img, score_type=score)
    if wh == (161, 97):
        # levels 3..7 are 93 x 56 and smaller: skipped
        assert want[2][3:] == [0] * 5 and sum(want[2][:3]) > 0
    else:
        assert sum(1 for c in want[2] if c > 0) >= 6
    same(slamhip.orbDetectAndCompute(img, scoreType=score, ctx=gpu_ctx), want)


@pytest.mark.parametrize("case", ["64x64", "flat200", "63x200", "200x63"])
def test_no_keypoints(gpu_ctx, case):
    if case == "64x64":
        img = np.ascontiguousarray(frame(320, 240)[:64, :64])
    elif case == "flat200":
        img = np.full((200, 200), 117, np.uint8)
    elif case == "63x200":
        img = np.ascontiguousarray(frame(320, 240)[:200, :63])      # level 0 is one column inside the border
    else:
        img = np.ascontiguousarray(frame(320, 240)[:63, :200])
    assert len(R.detect_and_compute(img)[0]) == 0
    k, d = slamhip.orbDetectAndCompute(img, ctx=gpu_ctx)
    assert len(k) == 0 and d.shape == (0, 32)


def test_level0_too_small(gpu_ctx):
    """62 px across: runByImageBorder(31) leaves nothing on level 0 or below it"""
    img = np.ascontiguousarray(frame(320, 240)[:200, :62])
    assert len(R.detect_and_compute(img)[0]) == 0
    k, d = slamhip.orbDetectAndCompute(img, ctx=gpu_ctx)
    assert len(k) == 0 and d.shape == (0, 32)


def test_one_level(gpu_ctx):
    img = frame(320, 240)
    want = ref("one", img, nlevels=1)
    assert (want[0]["octave"] == 0).all() and len(want[0]) > 100
    same(slamhip.orbDetectAndCompute(img, nlevels=1, ctx=gpu_ctx), want)


@pytest.mark.parametrize("score", [R.HARRIS_SCORE, R.FAST_SCORE])
def test_ties_all_kept(gpu_ctx, score):
    img = periodic_256()
    want = ref(("ties", score), img, nfeatures=40, score_type=score)
    assert max(want[2]) > 40                 # the precondition: one level alone returns more than nfeatures
    same(slamhip.orbDetectAndCompute(img, nfeatures=40, scoreType=score, ctx=gpu_ctx), want)


@pytest.mark.parametrize("score", [R.HARRIS_SCORE, R.FAST_SCORE])
def test_no_cut(gpu_ctx, score):
    img = frame(320, 240)
    want = ref(("all", score), img, nfeatures=100000, score_type=score)
    assert len(want[0]) > len(ref(((320, 240), score), img, score_type=score)[0])
    same(slamhip.orbDetectAndCompute(img, nfeatures=100000, scoreType=score, ctx=gpu_ctx), want)


def test_other_parameters(gpu_ctx):
    """a scale factor whose source tiles exceed the staged tile, few levels, another threshold"""
    img = frame(320, 240)
    want = ref("sf2", img, nfeatures=300, scale_factor=2.0, nlevels=3, fast_threshold=9)
    assert want[2][1] > 0
    same(slamhip.orbDetectAndCompute(img, nfeatures=300, scaleFactor=2.0, nlevels=3, fastThreshold=9, ctx=gpu_ctx), want)
    want = ref("sf105", img, nfeatures=200, scale_factor=1.05, nlevels=16)
    same(slamhip.orbDetectAndCompute(img, nfeatures=200, scaleFactor=1.05, nlevels=16, ctx=gpu_ctx), want)


def test_capacity(gpu_ctx):
    img = np.ascontiguousarray(frame(320, 240))
    want = ref(((320, 240), R.HARRIS_SCORE), img, score_type=R.HARRIS_SCORE)
    total = len(want[0])
    cap = 100
    assert total > cap
    kps = np.zeros(cap + 8, L.KEYPOINT_DTYPE)
    desc = np.full((cap + 8, 32), 0xEE, np.uint8)
    n = ctypes.c_int(0)
    rc = L.lib().slam_orb_detect(gpu_ctx.handle, L.ptr(img), 320, 240, img.strides[0], 3, 500, 1.2, 8, 20, 0,
                                 L.ptr(kps), cap, ctypes.byref(n), L.ptr(desc))
    assert rc == L.SLAM_E_CAPACITY and n.value == total
    assert kps[:cap].tobytes() == want[0][:cap].tobytes() and np.array_equal(desc[:cap], want[1][:cap])
    # nothing past the capacity is written
    assert (desc[cap:] == 0xEE).all() and kps[cap:].tobytes() == bytes(8 * L.KEYPOINT_DTYPE.itemsize)


def test_invalid_arguments(gpu_ctx):
    img = np.ascontiguousarray(frame(320, 240))
    kps = np.zeros(16, L.KEYPOINT_DTYPE)
    n = ctypes.c_int(0)

    def call(ch=3, nf=500, sf=1.2, nl=8, st=0):
        return L.lib().slam_orb_detect(gpu_ctx.handle, L.ptr(img), 320, 240, img.strides[0], ch, nf, sf, nl, 20, st,
                                       L.ptr(kps), 16, ctypes.byref(n), None)

    for kw in ({"nl": 0}, {"nl": 17}, {"sf": 1.0}, {"sf": 0.5}, {"nf": -1}, {"ch": 2}, {"st": 2}):
        assert call(**kw) == L.SLAM_E_INVALID_ARG, kw
    with pytest.raises(slamhip.SlamError):
        slamhip.orbDetectAndCompute(img, nlevels=17, ctx=gpu_ctx)


def test_channels_and_stride(gpu_ctx):
    bgr = frame(320, 240)
    gray = O.gray(bgr)
    want = ref("gray", gray)
    same(slamhip.orbDetectAndCompute(gray, ctx=gpu_ctx), want)
    same(slamhip.orbDetectAndCompute(bgr, ctx=gpu_ctx), want)
    bgra = np.ascontiguousarray(np.dstack([bgr, np.full(bgr.shape[:2], 9, np.uint8)]))
    same(slamhip.orbDetectAndCompute(bgra, ctx=gpu_ctx), want)
    # a strided host image: rows of a wider buffer
    wide = np.zeros((240, 352, 3), np.uint8)
    wide[:, :320] = bgr
    view = wide[:, :320]
    assert view.strides[0] == 352 * 3
    cap = 1024
    kps = np.zeros(cap, L.KEYPOINT_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    n = ctypes.c_int(0)
    rc = L.lib().slam_orb_detect(gpu_ctx.handle, L.ptr(wide), 320, 240, view.strides[0], 3, 500, 1.2, 8, 20, 0,
                                 L.ptr(kps), cap, ctypes.byref(n), L.ptr(desc))
    assert rc == L.SLAM_OK
    same((kps[:n.value], desc[:n.value]), want)
    # keypoints alone
    k, d = slamhip.orbDetectAndCompute(bgr, with_descriptors=False, ctx=gpu_ctx)
    assert d is None and k.tobytes() == want[0].tobytes()


def test_batch(gpu_ctx):
    import torch
    frames = np.stack([frame(320, 240, seed=s) for s in (31, 32, 33)] + [np.full((240, 320, 3), 60, np.uint8)])
    for score in (R.HARRIS_SCORE, R.FAST_SCORE):
        out = slamhip.orbDetectAndComputeBatch(torch.from_numpy(frames).cuda(), scoreType=score, ctx=gpu_ctx)
        assert len(out) == 4 and out.counts[3] == 0
        for f in range(4):
            same(out.host(f), ref(("batch", f, score), frames[f], score_type=score))
    # a small capacity: the wrapper grows it to the largest count
    out = slamhip.orbDetectAndComputeBatch(torch.from_numpy(frames).cuda(), ctx=gpu_ctx, cap=64)
    for f in range(4):
        same(out.host(f), ref(("batch", f, R.HARRIS_SCORE), frames[f]))
    # gray frames, and no frames at all
    g = np.stack([O.gray(frames[f]) for f in range(2)])
    out = slamhip.orbDetectAndComputeBatch(torch.from_numpy(g).cuda(), ctx=gpu_ctx)
    for f in range(2):
        same(out.host(f), ref(("batch", f, R.HARRIS_SCORE), frames[f]))
    empty = slamhip.orbDetectAndComputeBatch(torch.zeros((0, 240, 320, 3), dtype=torch.uint8, device="cuda"), ctx=gpu_ctx)
    assert len(empty) == 0


def test_batch_capacity_status(gpu_ctx):
    import torch
    frames = np.stack([frame(320, 240, seed=s) for s in (31, 32)])
    dev = torch.from_numpy(frames).cuda()
    cap = 50
    kps = torch.zeros((2, cap, 28), dtype=torch.uint8, device="cuda")
    desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device="cuda")
    cnt = np.zeros(2, np.int32)
    rc = L.lib().slam_orb_detect_batch(gpu_ctx.handle, None, ctypes.c_void_p(dev.data_ptr()), 2, 320, 240, 3, 500, 1.2,
                                       8, 20, 0, ctypes.c_void_p(kps.data_ptr()), cap, L.ptr(cnt),
                                       ctypes.c_void_p(desc.data_ptr()))
    assert rc == L.SLAM_E_CAPACITY
    for f in range(2):
        want = ref(("batch", f, R.HARRIS_SCORE), frames[f])
        assert cnt[f] == len(want[0]) > cap
        assert kps[f].cpu().numpy().tobytes() == want[0][:cap].tobytes()
        assert np.array_equal(desc[f].cpu().numpy(), want[1][:cap])


def test_descriptors_match_with_orb_bf(gpu_ctx):
    """the descriptors go straight into the Hamming matcher; a rolled camera keeps its matches"""
    img = O.gray(frame(320, 240))
    rot = np.ascontiguousarray(np.rot90(img))
    k0, d0 = slamhip.orbDetectAndCompute(img, ctx=gpu_ctx)
    k1, d1 = slamhip.orbDetectAndCompute(rot, ctx=gpu_ctx)
    m = slamhip.matchFeatures(d0, d1, slamhip.ORB_BF, 0.7, ctx=gpu_ctx)
    idx, dist = O.knn2(d0, d1, O.NORM_HAMMING)
    assert np.array_equal(m, O.ratio(idx, dist, 0.7))
    assert len(m) > len(k0) // 2


def test_existing_orb_descriptor_unchanged_after_detector(gpu_ctx):
    """the generalised orb_blur / orb_desc launch paths: extractDescriptor(ORB_BF) after a detector call"""
    img = frame(320, 240)
    slamhip.orbDetectAndCompute(img, ctx=gpu_ctx)
    k = slamhip.fastExtractor(img, 20, True, ctx=gpu_ctx)
    gk, gd = slamhip.extractDescriptor(img, k, slamhip.ORB_BF, ctx=gpu_ctx)
    rk, rd = O.orb(img, O.fast(img, 20, True))
    assert gk.tobytes() == rk.tobytes() and np.array_equal(gd, rd)

"""slam_klt_pyramid / slam_klt_track* on the device against tests/klt_ref.py, byte
for byte: next_pts, status and err of every point, status == 0 points included
(DESIGN.md section 15).  The point set and the configurations are those whose
reference trace takes every exit of the tracker (tests/test_klt.py)."""
import ctypes

import numpy as np
import pytest

import klt_ref as R
import slamhip
from slamhip import _lib as L
from slamhip.batch import DeviceBatch

pytestmark = pytest.mark.gpu

W, H = 160, 120


@pytest.fixture(scope="module")
def frames():
    return slamhip.synth_frames(W, H, 0, 3, seed=7)


@pytest.fixture(scope="module")
def fast_xy(frames, gpu_ctx):
    k = slamhip.fastExtractor(frames[0], 20, True, ctx=gpu_ctx)
    assert 50 <= len(k) <= 400
    return np.stack([k["x"], k["y"]], 1)


def same(got, ref):
    for g, r, name in zip(got, ref, ("next_pts", "status", "err")):
        assert g.dtype == r.dtype and g.shape == r.shape, name
        if g.tobytes() != r.tobytes():
            bad = np.nonzero((g.view(np.uint8).reshape(len(g), -1) != r.view(np.uint8).reshape(len(r), -1)).any(1))[0]
            raise AssertionError((name, len(bad), bad[:5], g[bad[:5]], r[bad[:5]]))


@pytest.mark.parametrize("w,h,ch,pad", [(97, 61, 3, 13), (160, 120, 1, 0)])
def test_pyramid_levels_and_derivatives(gpu_ctx, w, h, ch, pad):
    rng = np.random.default_rng(w)
    buf = rng.integers(0, 256, (h, w * ch + pad), dtype=np.uint8)
    img = buf[:, :w * ch].reshape(h, w, ch) if ch > 1 else buf[:, :w]
    assert img.strides[0] == w * ch + pad
    for win, ml in (((21, 21), 3), ((5, 5), 8), ((31, 31), 2), ((21, 21), 0)):
        n, levels, derivs = slamhip.buildOpticalFlowPyramid(img, win, ml, True, ctx=gpu_ctx)
        rl, rd = R.build_pyramid(img, win, ml, True)
        assert n == len(rl) == len(levels) == len(derivs)
        for a, b, c, d in zip(levels, rl, derivs, rd):
            assert a.shape == b.shape and np.array_equal(a, b)
            assert c.shape == d.shape and c.dtype == np.int16 and np.array_equal(c, d)
        n2, levels2, none = slamhip.buildOpticalFlowPyramid(img, win, ml, False, ctx=gpu_ctx)
        assert n2 == n and none is None and all(np.array_equal(a, b) for a, b in zip(levels2, rl))


def test_pyramid_of_bgra_is_the_bgr_one(gpu_ctx, frames):
    bgra = np.concatenate([frames[0], np.full((H, W, 1), 200, np.uint8)], 2)
    a = slamhip.buildOpticalFlowPyramid(bgra, (21, 21), 3, ctx=gpu_ctx)
    b = slamhip.buildOpticalFlowPyramid(frames[0], (21, 21), 3, ctx=gpu_ctx)
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1] + a[2], b[1] + b[2]))


@pytest.mark.parametrize("win", R.PARITY_WINDOWS)
@pytest.mark.parametrize("variant", R.PARITY_VARIANTS)
def test_track_parity(gpu_ctx, frames, fast_xy, win, variant):
    ml, crit, flags = variant
    pts = R.parity_points(frames[0], fast_xy, win)
    init = R.parity_initial_flow(pts, W, H) if flags & R.USE_INITIAL_FLOW else None
    ref = R.track(frames[0], frames[1], pts, init, win, ml, crit, flags)
    got = slamhip.calcOpticalFlowPyrLK(frames[0], frames[1], pts, init, win, ml, crit, flags, ctx=gpu_ctx)
    same(got, ref)
    assert 0 < ref[1].sum() < len(pts)          # both kinds of status are compared


def test_track_gray_input_and_threshold(gpu_ctx, frames, fast_xy):
    g0, g1 = R.gray(frames[0]), R.gray(frames[1])
    pts = R.parity_points(frames[0], fast_xy)
    ref = R.track(frames[0], frames[1], pts)
    same(slamhip.calcOpticalFlowPyrLK(g0, g1, pts, ctx=gpu_ctx), ref)
    ref = R.track(g0, g1, pts, min_eig_threshold=0.05)
    assert ref[1].sum() < R.track(g0, g1, pts)[1].sum()
    same(slamhip.calcOpticalFlowPyrLK(g0, g1, pts, minEigThreshold=0.05, ctx=gpu_ctx), ref)


@pytest.mark.parametrize("n", [0, 1, 5, 65])
def test_track_point_counts(gpu_ctx, frames, fast_xy, n):
    pts = R.parity_points(frames[0], fast_xy)[:n]
    got = slamhip.calcOpticalFlowPyrLK(frames[0], frames[1], pts, ctx=gpu_ctx)
    same(got, R.track(frames[0], frames[1], pts))
    assert got[0].shape == (n, 2)


def test_track_odd_size_frames(gpu_ctx):
    """97 x 61: every level has an odd side somewhere; the window rule stops at 25 x 16"""
    f = slamhip.synth_frames(97, 61, 0, 2, seed=3)
    rng = np.random.default_rng(1)
    pts = (rng.uniform(0, 1, (80, 2)) * (97, 61)).astype(np.float32)
    for win in ((21, 21), (9, 15)):
        same(slamhip.calcOpticalFlowPyrLK(f[0], f[1], pts, None, win, 3, ctx=gpu_ctx), R.track(f[0], f[1], pts, None, win, 3))


def test_invalid_arguments(gpu_ctx, frames):
    lib, c = slamhip.lib(), gpu_ctx.handle
    a, b = np.ascontiguousarray(frames[0]), np.ascontiguousarray(frames[1])
    pts = np.array([[50, 50]], np.float32)
    out, st, er = np.zeros((1, 2), np.float32), np.zeros(1, np.uint8), np.zeros(1, np.float32)

    def call(win=(21, 21), ml=3, mc=30, eps=0.01, flags=0, ch=3, n=1, p=pts, step=W * 3):
        return lib.slam_klt_track(c, L.ptr(a), step, L.ptr(b), W * 3, W, H, ch, L.ptr(p), n, L.ptr(out), L.ptr(st),
                                  L.ptr(er), win[0], win[1], ml, mc, eps, flags, 1e-4)
    assert call() == L.SLAM_OK
    bad = [dict(win=(2, 21)), dict(win=(21, 32)), dict(win=(33, 3)), dict(ml=-1), dict(ml=9), dict(mc=0), dict(eps=-1.0),
           dict(eps=float("nan")), dict(flags=1), dict(flags=16), dict(ch=2), dict(n=-1), dict(p=None), dict(step=W * 3 - 1)]
    for kw in bad:
        assert call(**kw) == L.SLAM_E_INVALID_ARG, kw
    assert call(n=0, p=None) == L.SLAM_OK
    # the pyramid call takes the same window and level range
    nl, need = ctypes.c_int(0), ctypes.c_size_t(0)
    sizes, gray = np.zeros((9, 2), np.int32), np.zeros(W * H * 2, np.uint8)

    def pyr(win=(21, 21), ml=3, cap=W * H * 2):
        return lib.slam_klt_pyramid(c, L.ptr(a), W, H, W * 3, 3, win[0], win[1], ml, ctypes.byref(nl), L.ptr(sizes),
                                    L.ptr(gray), None, cap, ctypes.byref(need))
    assert pyr() == L.SLAM_OK and nl.value == 3
    assert pyr(win=(1, 21)) == L.SLAM_E_INVALID_ARG and pyr(ml=9) == L.SLAM_E_INVALID_ARG
    assert pyr(cap=W * H) == L.SLAM_E_CAPACITY and need.value == W * H + 80 * 60 + 40 * 30
    with pytest.raises(ValueError):
        slamhip.calcOpticalFlowPyrLK(a, b, pts, None, flags=L.KLT_USE_INITIAL_FLOW, ctx=gpu_ctx)


def test_batch_of_candidates(gpu_ctx, frames, fast_xy):
    """three candidates, the middle one the previous frame itself: each equals its
    single-frame call, counts are the status sums, and a point tracked into its own
    frame does not move and has no error"""
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    cand = torch.stack([dev[1], dev[0], dev[2]])
    torch.cuda.synchronize()
    db = DeviceBatch(gpu_ctx)
    pts = R.parity_points(frames[0], fast_xy)
    out, st, er, cnt = db.track(dev[0], cand, pts)
    again = db.track(dev[0], cand, pts)
    for x, y in zip((out, st, er, cnt), again):
        assert x.tobytes() == y.tobytes()                  # deterministic: the same bytes twice in a row
    assert np.array_equal(cnt, st.sum(1)) and cnt.min() > 0
    for f, k in enumerate((1, 0, 2)):
        same((out[f], st[f], er[f]), R.track(frames[0], frames[k], pts))
        same((out[f], st[f], er[f]), slamhip.calcOpticalFlowPyrLK(dev[0], dev[k], pts, ctx=gpu_ctx))
    ok = st[1] == 1
    assert ok.sum() > 50 and np.array_equal(out[1][ok], pts[ok]) and not er[1][ok].any()
    # counts alone: nothing else crosses the bus
    none = db.track(dev[0], cand, pts, counts_only=True)
    assert none[0] is None and none[1] is None and none[2] is None and np.array_equal(none[3], cnt)
    # initial positions per candidate
    init = np.stack([R.parity_initial_flow(pts, W, H, seed=s) for s in (1, 2, 3)])
    out, st, er, cnt = db.track(dev[0], cand, pts, init, flags=L.KLT_USE_INITIAL_FLOW)
    for f, k in enumerate((1, 0, 2)):
        same((out[f], st[f], er[f]), R.track(frames[0], frames[k], pts, init[f], flags=R.USE_INITIAL_FLOW))
    assert np.array_equal(cnt, st.sum(1))
    # no points, no candidates
    e = db.track(dev[0], cand, np.zeros((0, 2), np.float32))
    assert e[0].shape == (3, 0, 2) and not e[3].any()
    assert len(db.track(dev[0], cand[:0], pts)[3]) == 0


@pytest.mark.parametrize("shift", R.TRUTH_SHIFTS)
def test_ground_truth_on_the_device(gpu_ctx, shift):
    """the closed-form texture of tests/test_klt.py: at least 80 % of the interior
    points tracked, displacement error below twice the reference's own maximum
    (0.0146 px and 0.0190 px)"""
    w, h = R.TRUTH_SIZE
    a, b = R.analytic_texture(w, h), R.analytic_texture(w, h, *shift)
    pts = R.truth_points()
    out, st, err = slamhip.calcOpticalFlowPyrLK(a, b, pts, ctx=gpu_ctx)
    assert st.sum() >= 0.8 * len(pts)
    e = np.abs(out - pts - np.float32(shift)).max(1)[st == 1].max()
    print("device max displacement error", shift, e)
    assert e < 2 * R.TRUTH_REF_MAX_ERR[shift]


FILES = ("points.txt", "colors.txt", "poses.txt", "rotations.txt")


def test_pipeline_tracker_mode(gpu_ctx, tmp_path, monkeypatch):
    """slam_main(tracker="klt") over GpuOps (host frames, resident frames, and
    resident frames searched in early-exit chunks) against the same control flow
    over the CPU oracle with klt_ref as its `track`: the same selections, features,
    matches, poses and points.  320 x 240, 8 frames, batches of 3, BA off."""
    import os

    import torch
    from slamhip import cycle
    from test_klt import K_QVGA, tracker_cfg, tracker_oracle_ops
    frames = slamhip.synth_frames(320, 240, 0, 8, seed=1234)
    found = []
    orig = cycle.find_good_frame_from_batch

    def spy(*a):
        r = orig(*a)
        found.append((r[0], None if r[2] is None else r[2].tobytes(), None if r[3] is None else r[3].tobytes()))
        return r

    monkeypatch.setattr(cycle, "find_good_frame_from_batch", spy)

    def run(media, ops, out):
        found.clear()
        gd, logs = cycle.slam_main(media, K_QVGA.copy(), tracker_cfg(), ops, out_dir=str(out), tracker="klt")
        return list(found), {f: open(os.path.join(out, f), "rb").read() for f in FILES}, len(logs.pose_list)

    want_sel, want, poses = run(cycle.MediaSources(list(frames)), tracker_oracle_ops(), tmp_path / "ref")
    assert poses >= 3 and sum(1 for s in want_sel if s[0] >= 0) >= 2
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    torch.cuda.current_stream().synchronize()
    runs = (("media", cycle.MediaSources(list(frames)), 0), ("dev", cycle.DeviceMedia(frames, dev), 0),
            ("chunks", cycle.DeviceMedia(frames, dev), 1))
    for name, media, early in runs:
        ops = cycle.GpuOps(gpu_ctx, early_exit=early)
        ops.describe = ops.search = None        # no descriptor may be computed in this mode
        try:
            sel, got, n = run(media, ops, tmp_path / name)
        finally:
            ops.close()
        assert n == poses and len(sel) == len(want_sel), name
        for i, (a, b) in enumerate(zip(sel, want_sel)):
            assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2], (name, i, a[0], b[0])
        for f in FILES:
            assert got[f] == want[f], (name, f)

"""sift_desc_band's slot layout: five columns per orientation position.

The band kernel keeps no slots for histogram column -1 (the c0 = -1 samples'
left share, outside the descriptor): those junk shares land in the quirk
column's discarded slots, one position up.  The quirk column's position 0 is
kept (column 3's slot 9, the 361-degree wrap), so a junk write that reached it,
or any other kept slot, would change a descriptor.

Linear ramps make that visible: every window sample of every keypoint has the
same orientation, so all of a keypoint's shares go to one or two orientation
positions, the wrap slots included.  Small frames and keypoints up to 3 px from
the edge put most windows into the zero border.  Compared bit for bit with the
oracle, under the default kernel, both part-walk forms and the position-plane
form.
"""
import numpy as np
import pytest

import oracle_ffi as O
import slamhip
from slamhip import _lib as L

pytestmark = pytest.mark.gpu

W, H = 192, 160
THETAS = [45.0 * j + 0.5 for j in range(8)] + [0.0, 90.0, 180.0, 359.6]
COUNTS = [1, 31, 32, 33, 65]      # one lane, a wave's 32 keypoints less / exactly / more, three groups


def _ramp(theta_deg):
    t = np.deg2rad(theta_deg)
    x = np.arange(W, dtype=np.float64)[None, :] - W / 2
    y = np.arange(H, dtype=np.float64)[:, None] - H / 2
    g = np.clip(128 + 0.6 * (x * np.cos(t) + y * np.sin(t)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g[..., None], 3, 2))


def _keypoints(n, rng):
    k = np.zeros(n, O.fast(np.zeros((16, 16), np.uint8), 10).dtype)
    k["x"] = rng.integers(3, W - 3, n)          # [3, W - 4]
    k["y"] = rng.integers(3, H - 3, n)
    k["size"], k["angle"], k["octave"], k["class_id"] = 7.0, -1.0, 0, -1
    return k


@pytest.fixture(scope="module")
def cases():
    """[(frame, keypoints, oracle descriptors, is_ramp)], computed once"""
    rng = np.random.default_rng(20230707)
    frames = [(_ramp(t), True) for t in THETAS]
    frames.append((rng.integers(0, 256, (H, W, 3), dtype=np.uint8), False))
    out = []
    for f, is_ramp in frames:
        for n in COUNTS:
            k = _keypoints(n, rng)
            out.append((f, k, O.sift(f, k), is_ramp))
    return out


def _bins(d):
    """orientation bins with a non-zero element somewhere in the descriptors"""
    return {int(o) for o in np.nonzero(d.reshape(-1, 16, 8).any(axis=(0, 1)))[0]}


def test_ramp_set_reaches_every_slot_position(cases):
    """preconditions, from the oracle's output alone"""
    union, wrap = set(), False
    for f, k, ref, is_ramp in cases:
        assert ref.shape == (len(k), 128)
        assert ref.any(axis=1).all(), "a zero descriptor checks nothing"
        if is_ramp:
            b = _bins(ref)
            union |= b
            wrap |= {0, 7} <= b
    assert union == set(range(8)), union
    assert wrap, "no ramp fills bins 7 and 0 together (the wrap slots)"


@pytest.mark.parametrize("mode", ["default", "all", "all4", "posplane"])
def test_sift_slots_bitexact(cases, mode, monkeypatch):
    ctx = slamhip.Context(0)
    try:
        if mode == "posplane":
            monkeypatch.setenv("SLAMHIP_SIFT_POSPLANE", "1")
        if mode != "default":
            ctx.set_option(L.OPT_SIFT_KERNEL, L.SIFT_KERNEL_BAND)
        if mode in ("all", "all4"):
            ctx.set_option(L.OPT_SIFT_BAND_SPLIT, L.BAND_SPLIT_ALL if mode == "all" else L.BAND_SPLIT_ALL4)
        for f, k, ref, _ in cases:
            gk, got = slamhip.extractDescriptor(f, k, slamhip.SIFT_FLANN, ctx=ctx)
            assert len(gk) == len(k)
            np.testing.assert_array_equal(got, ref)
            if mode != "default":
                assert slamhip.lib().slam_last_sift_kernel(ctx.handle) == L.SIFT_KERNEL_BAND
    finally:
        ctx.close()


def test_pipelined_searches_equal_plain_searches():
    """three SIFT searches of three 640 x 480 frames each through PipelinedScan
    (overlap desc_start: the next extraction queued beside this search's
    descriptor kernel and kNN) return the counts, selection, winner keypoints and
    matches of the same searches through a plain ShardedScan"""
    import torch
    from slamhip.batch import Conditions, PipelinedScan, ShardedScan
    host = slamhip.synth_frames(640, 480, 300, 10, seed=7)
    frames = torch.from_numpy(host).cuda()
    cond = Conditions(featureExtractingThreshold=20, requiredExtractedPointsCount=200,
                      requiredMatchedPointsCount=30, matcherType=slamhip.SIFT_FLANN, knnMatcherDistance=0.7)
    batches = [(1, 4), (4, 7), (7, 10)]
    nbytes = slamhip.lib().slam_batch_desc_bytes(slamhip.SIFT_FLANN, 64 * 1024)

    def run(pipelined):
        ctx = None if pipelined else slamhip.Context(0)
        scan = PipelinedScan(0, 1, 0, overlap="desc_start") if pipelined else ShardedScan(0, 1, ctx=ctx)
        first = scan.scans[1].db if pipelined else scan.db
        first.extract(frames[:1], 20, slamhip.SIFT_FLANN)
        prev = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        _, nprev = first.export_desc(0, prev)
        owner, out = 0, []
        if pipelined:
            scan.queue(frames[1:4], cond)
        for b, (lo, hi) in enumerate(batches):
            if pipelined:
                nxt = frames[batches[b + 1][0]:batches[b + 1][1]] if b + 1 < len(batches) else None
                good, kp_all, mc_all, in_batch, dc_all = scan.search(frames[lo:hi], prev, nprev, owner, cond,
                                                                     next_frames=nxt)
            else:
                good, kp_all, mc_all, in_batch, dc_all = scan.search(frames[lo:hi], prev, nprev, owner, cond)
            kps, mts = scan.winner(good, in_batch, dc_all, mc_all, nprev)
            out.append((good, kp_all.copy(), mc_all.copy(), in_batch.copy(), dc_all.copy(), kps, mts))
            owner, nprev = scan.advance(good, in_batch, dc_all, prev, owner, nprev)
        if pipelined:
            scan.close()
        else:
            ctx.close()
        return out

    plain, piped = run(False), run(True)
    wins = 0
    for a, b in zip(plain, piped):
        assert a[0] == b[0]
        for x, y in zip(a[1:5], b[1:5]):
            np.testing.assert_array_equal(x, y)
        if a[0] >= 0:
            wins += 1
            np.testing.assert_array_equal(a[5], b[5])
            np.testing.assert_array_equal(a[6], b[6])
            assert len(a[5]) > 0 and len(a[6]) > 0
    assert wins >= 2, "the searches must select winners for the comparison to mean something"

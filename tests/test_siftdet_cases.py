"""The detector fixtures of tests/siftdet_cases.py are not vacuous: with the
oracle alone (no GPU), they reach the descriptor-window limit, the largest
orientation radius, clipped windows, extra orientation peaks and five octaves,
the degenerate pictures give no keypoint, and every sweep size gives hundreds.

The bounds sit well under what the oracle measures (in the comments): if one
fails, the fixture changed, not the detector.
"""
import numpy as np
import pytest

import oracle_ffi as O
import siftdet_cases as S


def test_blocky_builder():
    a = S.blocky(7, 10, 4, 5)
    assert a.shape == (7, 10) and a.dtype == np.uint8 and a.flags.c_contiguous
    r = np.random.default_rng(5).integers(0, 256, (2, 3), dtype=np.uint8)
    np.testing.assert_array_equal(a, np.kron(r, np.ones((4, 4), np.uint8))[:7, :10])
    np.testing.assert_array_equal(a, S.blocky(7, 10, 4, 5))
    assert set(np.unique(S.image("two_level")).tolist()) == {0, 255}
    for p in (4, 8, 16):
        v = S.image(f"vbars{p}")
        assert (v == v[:1]).all() and (v[0, :p] == [0] * (p // 2) + [255] * (p // 2)).all()
        np.testing.assert_array_equal(v[:, p:], v[:, :-p])          # exactly periodic
        np.testing.assert_array_equal(S.image(f"hbars{p}"), S.bars(128, 96, p, True).T)
    assert S.image("low_contrast").min() >= 100 and S.image("low_contrast").max() <= 107
    assert [S.image(n).shape for n in S.STRIPS] == [(20, 300), (12, 400), (300, 11)]


def test_images_are_shared_and_read_only():
    assert S.image("blocky4") is S.image("blocky4")
    assert not S.image("blocky4").flags.writeable
    k, d = S.reference("blobs")
    assert S.reference("blobs")[0] is k and not k.flags.writeable and not d.flags.writeable


def test_kp_stats_known_answers():
    # octave byte 255 = OpenCV octave -1 = pyramid octave 0 (2w x 2h), units doubled
    k = np.zeros(3, O.KP)
    k["octave"] = [255 | (1 << 8), 0 | (2 << 8), 2 | (3 << 8)]
    k["size"] = [3.6, 7.2, 28.8]            # scl = 3.6 in each keypoint's octave
    k["x"] = [50, 50, 50]
    k["y"] = [40, 40, 40]
    st = S.kp_stats(k, 100, 120)
    assert st["octave"].tolist() == [0, 1, 3]
    assert st["desc_radius"].tolist() == [38, 38, 38]      # rint(3 * 3.6 * sqrt(2) * 2.5) = rint(38.18)
    assert st["ori_radius"].tolist() == [16, 16, 16]       # rint(4.5 * 3.6) = rint(16.2)
    # octave 0: 240 x 200, centre (100, 80): clear; octave 1: 120 x 100, centre (50, 40): clear by 2 rows;
    # octave 3: 30 x 25, centre rint(50 / 4) = 12, rint(40 / 4) = 10: clipped
    assert st["clipped"].tolist() == [False, False, True]
    k["y"] = [40, 38, 40]                   # octave 1: 38 - 38 = 0 is not an interior row
    assert S.kp_stats(k, 100, 120)["clipped"].tolist() == [False, True, True]
    e = np.zeros(4, O.KP)
    e["angle"] = [10, 20, 20, 30]
    e["x"] = [1, 1, 2, 2]
    assert S.extra_orientations(e) == 2


@pytest.mark.parametrize("name", S.SWEEP_NAMES)
def test_sweep_sizes_are_dense(name):
    _, w, h = S.SWEEP[S.SWEEP_NAMES.index(name)]
    assert S.image(name).shape == (h, w)
    k, d = S.reference(name)                 # measured: 253 - 330 per image
    assert len(k) >= 200 and d.shape == (len(k), 128)
    assert (S.kp_stats(k, h, w)["octave"] <= 1).sum() >= 150      # the two octaves the sweep is about


def test_sweep_covers_every_fast_path_edge():
    """the widths and heights on both sides of each interior-path condition of
    sd_blur (second tile column / row of octave 1) and of sd_extrema"""
    ws = {w for _, w, h in S.SWEEP_W}
    hs = {h for _, w, h in S.SWEEP_H}
    for R in (5, 6, 8, 10, 13):
        assert {64 + 64 + R + 3 - 1, 64 + 64 + R + 3} <= ws
        assert {32 + 32 + R - 1, 32 + 32 + R} <= hs
        # and of the widest frame at which the float4 row would be wrong: the tile's last column not a real pixel
        assert {64 + 64 + R - 1, 64 + 64 + R} <= ws
    assert {69 - 1 + 68 - 1, 69 - 1 + 68} <= ws and {53 - 1 + 18 - 1, 53 - 1 + 18} <= hs
    assert all(h == 77 for _, w, h in S.SWEEP_W) and all(w == 144 for _, w, h in S.SWEEP_H)


def test_named_cases_reach_the_limits():
    r37 = r38 = o16 = clipped = extra = 0
    octaves = set()
    for name in S.NAMED:
        k, _ = S.reference(name)
        st = S.kp_stats(k, *S.image(name).shape)
        r37 += int((st["desc_radius"] >= 37).sum())
        r38 += int((st["desc_radius"] == 38).sum())
        assert (st["desc_radius"] <= 38).all() and (st["ori_radius"] <= 16).all()     # kSdW / kOriMaxR hold
        o16 += int((st["ori_radius"] == 16).sum())
        clipped += int(st["clipped"].sum())
        extra += S.extra_orientations(k)
        octaves |= set(st["octave"].tolist())
    assert r37 >= 20 and r38 >= 1            # measured: 101 and 35
    assert o16 >= 1                          # measured: 100
    assert clipped >= 300                    # measured: 2 038
    assert extra >= 400                      # measured: 1 662
    assert len(octaves) >= 5                 # measured: octaves 0 .. 4


def test_dense_case_counts():
    k, _ = S.reference("blocky4")            # measured: 2 259 keypoints, 523 extra orientations, octaves 0 .. 3
    st = S.kp_stats(k, 240, 320)
    assert len(k) >= 2000 and S.extra_orientations(k) >= 400 and len(set(st["octave"].tolist())) >= 4
    assert (st["desc_radius"] >= 37).sum() >= 20
    assert S.kp_stats(S.reference("mix3")[0], 240, 320)["octave"].max() >= 4
    assert S.reference("square64")[0]["size"].max() > 40 and S.reference("square65")[0]["size"].max() > 40
    for name in S.STRIPS:                    # measured: 99, 39 and 34, every window clipped
        k, _ = S.reference(name)
        assert len(k) >= 20 and S.kp_stats(k, *S.image(name).shape)["clipped"].all()
    k, _ = S.reference("blobs")              # measured: 13, every window clipped
    assert len(k) >= 7 and S.kp_stats(k, 128, 128)["clipped"].all()
    assert len(S.reference("two_level")[0]) >= 500 and len(S.reference("mirrored")[0]) >= 500


@pytest.mark.parametrize("name", S.ZERO)
def test_degenerate_pictures_give_no_keypoint(name):
    assert len(S.reference(name)[0]) == 0


@pytest.mark.parametrize("hw", S.EMPTY_PYRAMID + ((1, 1), (2, 2), (1, 4096)))
def test_empty_pyramid_sizes_give_no_keypoint(hw):
    h, w = hw
    k, d = O.sift_detect(S.small(h, w))
    assert len(k) == 0 and d.shape == (0, 128)
    if min(h, w) == 1:
        assert O.oracle().orc_sift_octaves(w, h) == 0      # cvRound(log2(2) - 2) + 1


def test_no_interior_sizes():
    got = {hw: len(O.sift_detect(S.small(*hw))[0]) for hw in S.NO_INTERIOR}
    assert got[(5, 5)] == 0 and got[(11, 11)] == 0
    assert got[(12, 400)] >= 10              # measured: 41 (octave 0 is 24 x 800: interior rows 5 .. 18)

"""GPU tests of the scene renderer (csrc/render.hip): every frame, id plane and
depth plane is compared with tests/render_ref.py for equality, byte for byte.
Viewports: 33 x 17 with the principal point off centre, 64 x 64 with a camera
whose numbers are powers of two (so that vertices can sit exactly on pixel
centres and borders), and one 1000 x 1000 case with fewer than 50 primitives."""
import json
import math

import numpy as np
import pytest

import render_ref as RR
import scene_ref as R
import slamhip
from slamhip import _lib as L
from slamhip import api, cycle, scene
from test_render import decode_png, rot

pytestmark = pytest.mark.gpu

I3, O3 = np.eye(3), np.zeros(3)
CAM33 = (30.0, 28.0, 14.3, 9.6, 0.5, 100.0)          # 33 x 17
CAM64 = (32.0, 32.0, 32.0, 32.0, 0.5, 100.0)         # 64 x 64: at Z = 4, u = 8 X + 32 exactly
NO_PTS, NO_COLS = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8)
NO_FACES, NO_LINES = np.zeros((0, 3), np.int32), np.zeros((0, 6), np.float32)


def at(u, v, z=4.0, cam=CAM64):
    """the camera-space point that projects to (u, v) at depth z"""
    return [(u - cam[2]) / cam[0] * z, (v - cam[3]) / cam[1] * z, z]


def colours(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def both(ctx, pts, cols, faces, lines, lcols, views, cam, size, point_size=1, **kw):
    """(device result, reference result, device stats, reference stats); asserts equality"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    cols = np.asarray(cols, np.uint8).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    lines = np.asarray(lines, np.float32).reshape(-1, 6)
    lcols = np.asarray(lcols, np.uint8).reshape(-1, 3)
    got = api.renderViews(pts, cols, faces, lines, lcols, views, camera=cam, size=size, point_size=point_size, ids=True,
                          depth=True, ctx=ctx, **kw)
    stats = api.renderStats(ctx)[0]
    rs = RR.Stats()
    want = RR.render(pts, cols, faces, lines, lcols, views, cam, size, point_size, stats=rs)
    for name, g, w in zip(("frames", "ids", "depth"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), (name, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())
    assert tuple(stats[k] for k in ("primitives", "skipped", "clipped", "rasterised", "fragments")) == rs.tuple()
    return got, want, stats


def kinds(ids):
    """(kind, index) planes of an id plane; the background has kind -1"""
    u = ids.view(np.uint32)
    return np.where(ids == -1, -1, (u >> 30).astype(np.int64)), np.where(ids == -1, -1, (u & ((1 << 30) - 1)).astype(np.int64))


V0 = [(I3, O3)]
FORCED_MODES = (L.RENDER_THREAD, L.RENDER_WAVE, L.RENDER_WAVE_FULL_LIST)


def every_mode_equals(ctx, first, pts, cols, faces, lines, lcols, views, cam, size, point_size=1):
    """the forced raster modes (slam_render_views_dev: a thread per face; a wave per
    tile; a wave per tile with a list of 64 entries, whose overflow the appending
    threads walk) against `first` = both(...) of the same input, which is already
    equal to the reference: frames, ids, depth and statistics"""
    args = [np.asarray(a, t).reshape(-1, k) for a, t, k in ((pts, np.float32, 3), (cols, np.uint8, 3), (faces, np.int32, 3),
                                                            (lines, np.float32, 6), (lcols, np.uint8, 3))]
    for mode in FORCED_MODES:
        got = api.renderViews(*args, views, camera=cam, size=size, point_size=point_size, ids=True, depth=True, ctx=ctx,
                              raster_mode=mode)
        for name, g, w in zip(("frames", "ids", "depth"), got, first[0]):
            assert g.tobytes() == w.tobytes(), (mode, name, int((g != w).sum()))
        assert api.renderStats(ctx)[0] == first[2], mode


def test_triangle_in_each_winding(gpu_ctx):
    pts = [at(5.3, 3.1, 4, CAM33), at(28.9, 6.7, 6, CAM33), at(11.2, 15.8, 3, CAM33)]
    a = both(gpu_ctx, pts, colours(3), [[0, 1, 2]], NO_LINES, NO_COLS, V0, CAM33, (33, 17))[0]
    b = both(gpu_ctx, pts, colours(3), [[2, 1, 0]], NO_LINES, NO_COLS, V0, CAM33, (33, 17))[0]
    assert (kinds(a[1])[0] == L.RENDER_FACE).sum() > 100
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_shared_edge_through_pixel_centres_and_vertex_on_a_centre(gpu_ctx):
    """the diagonal (10.5, 10.5) - (40.5, 40.5) passes through 31 pixel centres, the
    other edges through centres too: each is covered by exactly one triangle"""
    pts = [at(10.5, 10.5), at(40.5, 40.5), at(40.5, 10.5), at(10.5, 40.5)]
    faces = [[0, 2, 1], [0, 1, 3]]
    got = both(gpu_ctx, pts, colours(4), faces, NO_LINES, NO_COLS, V0, CAM64, (64, 64))[0]
    kind, index = kinds(got[1][0])
    face = kind == L.RENDER_FACE
    square = np.zeros((64, 64), bool)
    square[10:40, 10:40] = True                                         # [10.5, 40.5)^2 by the top-left rule
    assert face[square].sum() == 899 and kind[10, 10] == L.RENDER_POINT and not face[~square].any()
    count = RR.coverage(np.asarray(pts, np.float32), faces, V0[0], CAM64, (64, 64))
    assert count.max() == 1 and count.sum() == 900
    d = np.arange(10, 40)
    assert set(index[d, d][face[d, d]].tolist()) == {0}                 # the diagonal belongs to the upper-right triangle only
    assert kind[10, 10] == L.RENDER_POINT                               # the vertex on a centre: the cloud point wins the tie


def test_zero_area_triangles(gpu_ctx):
    pts = [at(5, 5), at(25, 25), at(45, 45), at(50, 10)]
    got, _, stats = both(gpu_ctx, pts, colours(4), [[0, 1, 2], [0, 0, 3], [1, 1, 1]], NO_LINES, NO_COLS, V0, CAM64, (64, 64))
    assert (kinds(got[1])[0] == L.RENDER_FACE).sum() == 0
    assert stats["clipped"] == 3


def test_triangle_covering_the_viewport_from_far_outside(gpu_ctx):
    pts = [at(-3000, -3000), at(6000, -3000), at(-3000, 6000)]
    got = both(gpu_ctx, pts, colours(3), [[0, 1, 2]], NO_LINES, NO_COLS, V0, CAM64, (64, 64))
    assert (kinds(got[0][1])[0] == L.RENDER_FACE).all()
    every_mode_equals(gpu_ctx, got, pts, colours(3), [[0, 1, 2]], NO_LINES, NO_COLS, V0, CAM64, (64, 64))
    far_out = [at(-2e6, -2e6), at(4e6, -2e6), at(-2e6, 4e6)]            # beyond the guard band: clipped to it, not lost
    got = both(gpu_ctx, far_out, colours(3), [[0, 1, 2]], NO_LINES, NO_COLS, V0, CAM33, (33, 17))[0]
    assert (kinds(got[1])[0] == L.RENDER_FACE).all()


@pytest.mark.parametrize("behind", [1, 2, 3])
def test_vertices_behind_the_camera(gpu_ctx, behind):
    z = [3.0, 2.0, 5.0]
    for i in range(behind):
        z[i] = -1.0 - i
    pts = [[-1.1, -1.8, z[0]], [1.0, -1.0, z[1]], [0.3, 1.4, z[2]]]
    got, _, stats = both(gpu_ctx, pts, colours(3), [[0, 1, 2]], NO_LINES, NO_COLS, V0, CAM64, (64, 64))
    n = (kinds(got[1])[0] == L.RENDER_FACE).sum()
    assert (n == 0 and stats["clipped"] == 4) if behind == 3 else n > 100


def test_triangle_beyond_the_far_plane_and_across_it(gpu_ctx):
    beyond = [at(10, 10, 200), at(50, 12, 300), at(20, 50, 250)]
    got, _, stats = both(gpu_ctx, beyond, colours(3), [[0, 1, 2]], NO_LINES, NO_COLS, V0, CAM64, (64, 64))
    assert (got[1] == -1).all() and stats["clipped"] == 4
    across = [at(10, 10, 50), at(50, 12, 300), at(20, 50, 250)]
    got = both(gpu_ctx, across, colours(3), [[0, 1, 2]], NO_LINES, NO_COLS, V0, CAM64, (64, 64))[0]
    assert 10 < (kinds(got[1])[0] == L.RENDER_FACE).sum() < 600
    assert got[2][got[1] != -1].min() >= np.float32(1 / 100.0)


def test_interpenetrating_and_identical_triangles(gpu_ctx):
    pts = [at(8, 8, 2), at(56, 10, 8), at(30, 56, 5), at(8, 10, 8), at(56, 8, 2), at(32, 56, 5)]
    got = both(gpu_ctx, pts, colours(6), [[0, 1, 2], [3, 4, 5]], NO_LINES, NO_COLS, V0, CAM64, (64, 64))[0]
    kind, index = kinds(got[1][0])
    assert ((kind == 2) & (index == 0)).sum() > 200 and ((kind == 2) & (index == 1)).sum() > 200
    got = both(gpu_ctx, pts, colours(6), [[0, 1, 2], [1, 2, 0], [2, 0, 1]], NO_LINES, NO_COLS, V0, CAM64, (64, 64))[0]
    kind, index = kinds(got[1][0])
    assert set(index[kind == 2].tolist()) == {0}                        # equal depth everywhere: the lower index wins


def test_points_against_a_triangle_and_the_border(gpu_ctx):
    tri = [at(10.5, 10.5), at(50.5, 12.5), at(20.5, 50.5)]
    pts = tri + [at(25.5, 25.5, 3.0), at(30.5, 20.5, 5.0),               # in front of / behind the triangle
                 at(0, 0), at(63.99, 63.99), at(64, 32), at(32, 64), at(-0.01, 5),      # on / just off the border
                 at(40.5, 40.5, 0.5), at(41.5, 40.5, 0.4999), at(42.5, 40.5, 100.0), at(43.5, 40.5, 100.01)]   # Z = near, far
    got, want, stats = both(gpu_ctx, pts, colours(len(pts)), [[0, 1, 2]], NO_LINES, NO_COLS, V0, CAM64, (64, 64))
    kind, index = kinds(got[1][0])
    assert (kind[10, 10], index[10, 10]) == (L.RENDER_POINT, 0)          # at the vertex: equal depth, the point wins
    assert (kind[25, 25], index[25, 25]) == (L.RENDER_POINT, 3)
    assert (kind[20, 30], index[20, 30]) == (L.RENDER_FACE, 0)
    assert (kind[0, 0], index[0, 0]) == (L.RENDER_POINT, 5) and (kind[63, 63], index[63, 63]) == (L.RENDER_POINT, 6)
    assert (kind[40, 40], index[40, 40]) == (L.RENDER_POINT, 10) and kind[40, 41] == -1
    assert (kind[40, 42], index[40, 42]) == (L.RENDER_POINT, 12) and kind[40, 43] == -1
    assert got[2][0, 40, 40] == np.float32(2.0)
    assert stats["clipped"] == 5                                         # three off the border, one nearer than near, one beyond far


@pytest.mark.parametrize("point_size", [3, 7])
def test_point_size_at_the_corners(gpu_ctx, point_size):
    pts = [at(0.5, 0.5, 4, CAM33), at(32.5, 16.5, 5, CAM33), at(31.2, 1.7, 3, CAM33), at(16.5, 8.5, 6, CAM33), at(17.5, 8.5, 2, CAM33)]
    got = both(gpu_ctx, pts, colours(5), NO_FACES, NO_LINES, NO_COLS, V0, CAM33, (33, 17), point_size=point_size)[0]
    r = (point_size - 1) // 2
    kind, index = kinds(got[1][0])
    assert (index[:r + 1, :r + 1] == 0).all() and (index[16 - r:, 32 - r:] == 1).all()
    assert index[8, 16] == 4 and index[8, 16 - r] == 3                   # the nearer square on top


def line_cases():
    z = 4.0
    seg = lambda a, b: np.concatenate([a, b])
    return np.array([
        seg(at(3.5, 5.5, 1.5, CAM33), at(29.5, 5.5, 1.5, CAM33)),        # horizontal, nearer than all that cross it
        seg(at(6.5, 1.5, z, CAM33), at(6.5, 15.5, 5, CAM33)),            # vertical
        seg(at(10.2, 2.3, 3, CAM33), at(22.2, 14.3, 6, CAM33)),          # +45 degrees
        seg(at(30.7, 2.4, 3, CAM33), at(18.7, 14.4, 3, CAM33)),          # -45 degrees
        seg(at(12.5, 0.5, 2, CAM33), at(15.5, 16.5, 7, CAM33)),          # steep
        seg(at(20.5, 9.5, 5, CAM33), at(20.5, 9.5, 5, CAM33)),           # zero length
        seg(at(2.5, 12.5, 3, CAM33), [3.0, -0.5, -2.0]),                 # through the near plane
        seg([0.0, 0.0, -1.0], [1.0, 1.0, -3.0]),                         # wholly behind
        seg(at(-40.0, 8.0, 4, CAM33), at(90.0, 11.0, 4, CAM33)),         # across the viewport from outside
        seg(at(1.5, 15.5, 6, CAM33), at(31.5, 9.5, 2, CAM33)),           # a pair ...
        seg(at(31.5, 9.5, 2, CAM33), at(1.5, 15.5, 6, CAM33)),           # ... reversed
    ], np.float32)


def test_lines(gpu_ctx):
    lines = line_cases()
    lcols = colours(len(lines), 4)
    got, _, stats = both(gpu_ctx, NO_PTS, NO_COLS, NO_FACES, lines, lcols, V0, CAM33, (33, 17))
    kind, index = kinds(got[1][0])
    assert (index[5, 3:30] == 0).all() and (kind[5, 3:30] == L.RENDER_LINE).all()
    assert stats["clipped"] == 1 and stats["skipped"] == 0
    for i in range(len(lines)):                                          # each alone, so that nothing hides it
        one = both(gpu_ctx, NO_PTS, NO_COLS, NO_FACES, lines[i:i + 1], lcols[i:i + 1], V0, CAM33, (33, 17))[0]
        n = int((one[1] != -1).sum())
        assert n == {5: 1, 7: 0}.get(i, n) and (n >= 10 or i in (5, 7))
    fwd = api.renderViews(NO_PTS, NO_COLS, NO_FACES, lines[9:10], lcols[:1], V0, camera=CAM33, size=(33, 17), ids=True,
                          depth=True, ctx=gpu_ctx)
    rev = api.renderViews(NO_PTS, NO_COLS, NO_FACES, lines[10:11], lcols[:1], V0, camera=CAM33, size=(33, 17), ids=True,
                          depth=True, ctx=gpu_ctx)
    for x, y in zip(fwd, rev):
        assert x.tobytes() == y.tobytes()


def small_scene(seed=2):
    """a few faces, points and lines that overlap, for the multi-view and determinism tests"""
    rng = np.random.default_rng(seed)
    pts = (rng.normal(0, 1.2, (40, 3)) + [0, 0, 5]).astype(np.float32)
    faces = rng.integers(0, 40, (25, 3)).astype(np.int32)
    lines = np.concatenate([pts[rng.integers(0, 40, 6)], pts[rng.integers(0, 40, 6)] + 0.3], 1).astype(np.float32)
    return pts, colours(40, seed), faces, lines, colours(6, seed + 1)


def test_bad_face_index_and_nan_vertex_are_skipped(gpu_ctx):
    pts, cols, faces, lines, lcols = small_scene()
    clean = both(gpu_ctx, pts, cols, faces, lines, lcols, V0, CAM64, (64, 64))
    bad_pts = np.concatenate([pts, [[np.nan, 0, 5], [0, np.inf, 5]]]).astype(np.float32)
    bad_cols = np.concatenate([cols, colours(2, 9)])
    bad_faces = np.concatenate([faces, [[0, 1, 40], [2, 41, 3], [0, 1, 42], [-1, 2, 3], [0, 1, 2 ** 31 - 1]]]).astype(np.int32)
    bad_lines = np.concatenate([lines, [[0, 0, 5, np.nan, 0, 5]]]).astype(np.float32)
    bad = both(gpu_ctx, bad_pts, bad_cols, bad_faces, bad_lines, np.concatenate([lcols, colours(1, 8)]), V0, CAM64, (64, 64))
    for x, y in zip(clean[0], bad[0]):
        assert x.tobytes() == y.tobytes()
    assert clean[2]["skipped"] == 0 and bad[2]["skipped"] == 2 + 5 + 1
    assert bad[2]["primitives"] == clean[2]["primitives"] + 8


def test_no_primitives(gpu_ctx):
    for size, cam in (((33, 17), CAM33), ((1, 1), (1.0, 1.0, 0.5, 0.5, 0.5, 2.0))):
        got = both(gpu_ctx, NO_PTS, NO_COLS, NO_FACES, NO_LINES, NO_COLS, V0 * 2, cam, size)[0]
        assert (got[0] == 255).all() and (got[1] == -1).all() and (got[2] == 0).all() and len(got[0]) == 2
    empty = api.renderViews(NO_PTS, NO_COLS, NO_FACES, NO_LINES, NO_COLS, [], camera=CAM33, size=(33, 17), ctx=gpu_ctx)
    assert empty.shape == (0, 17, 33, 3)


def test_views_chunks_and_repeats(gpu_ctx):
    pts, cols, faces, lines, lcols = small_scene(3)
    views = [(I3, O3), (rot([0, 1, 0], 0.3), np.array([1.5, 0.2, 0.5])), (rot([1, 0.2, 0], -0.4), np.array([0.1, -2.0, 1.0]))]
    together = both(gpu_ctx, pts, cols, faces, lines, lcols, views, CAM33, (33, 17), point_size=3)[0]
    chunked = api.renderViews(pts, cols, faces, lines, lcols, views, camera=CAM33, size=(33, 17), point_size=3, ids=True,
                              depth=True, ctx=gpu_ctx, chunk_views=1)
    again = api.renderViews(pts, cols, faces, lines, lcols, views, camera=CAM33, size=(33, 17), point_size=3, ids=True,
                            depth=True, ctx=gpu_ctx)
    for a, b, c in zip(together, chunked, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    for i, v in enumerate(views):
        single = api.renderViews(pts, cols, faces, lines, lcols, [v], camera=CAM33, size=(33, 17), point_size=3, ids=True,
                                 depth=True, ctx=gpu_ctx)            # slam_render: host buffers, one view
        for a, b in zip(together, single):
            assert a[i].tobytes() == b[0].tobytes()
    assert len({together[0][i].tobytes() for i in range(3)}) == 3       # three different pictures


@pytest.mark.parametrize("planes", ["ids_depth", "frame_only"])
def test_host_buffers_tiny_odd_view(gpu_ctx, planes):
    """slam_render (host buffers, one view) at 5 x 3 pixels with three vertices, one face and one line:
    every staged array has an odd byte count; the reference's bits, and nothing past an output's end"""
    cam, size = (4.0, 4.0, 2.5, 1.5, 0.5, 100.0), (5, 3)
    pts = np.asarray([at(0.5, 0.5, 4.0, cam), at(4.5, 0.5, 4.0, cam), at(0.5, 2.5, 4.0, cam)], np.float32)
    cols, faces = colours(3, 3), np.array([[0, 1, 2]], np.int32)
    lines = np.asarray([at(0.5, 2.5, 3.0, cam) + at(4.5, 2.5, 3.0, cam)], np.float32)
    lcols = colours(1, 4)
    want = RR.render(pts, cols, faces, lines, lcols, V0, cam, size)
    assert len(np.unique(kinds(want[1])[0])) > 2                     # the face, the line or a point, and background
    wh, tail = 15, 64
    out = np.full(wh * 3 + tail, 0xA5, np.uint8)
    ids = np.full(wh + tail, -77, np.int32) if planes == "ids_depth" else None
    depth = np.full(wh + tail, -77.0, np.float32) if planes == "ids_depth" else None
    vw, cm = api._views(V0), np.ascontiguousarray(cam, np.float64)
    h = gpu_ctx.handle
    L.check(L.lib().slam_render(h, L.ptr(pts), L.ptr(cols), 3, L.ptr(faces), 1, L.ptr(lines), L.ptr(lcols), 1, L.ptr(vw),
                                L.ptr(cm), 5, 3, 1, L.ptr(out), L.ptr(ids), L.ptr(depth)), h)
    assert out[:wh * 3].tobytes() == want[0].tobytes() and (out[wh * 3:] == 0xA5).all()
    if planes == "ids_depth":
        assert ids[:wh].tobytes() == want[1].tobytes() and (ids[wh:] == -77).all()
        assert depth[:wh].tobytes() == want[2].tobytes() and (depth[wh:] == -77.0).all()


def test_resident_tensors(gpu_ctx):
    import torch
    pts, cols, faces, lines, lcols = small_scene(4)
    dev = torch.device("cuda", gpu_ctx.device)
    t = [torch.from_numpy(a).to(dev) for a in (pts, cols, faces, lines, lcols)]
    got = api.renderViews(*t, V0, camera=CAM64, size=(64, 64), ids=True, depth=True, ctx=gpu_ctx)
    want = RR.render(pts, cols, faces, lines, lcols, V0, CAM64, (64, 64))
    for g, w in zip(got, want):
        assert g.device.type == "cuda" and g.cpu().numpy().tobytes() == w.tobytes()


def test_thousands_of_small_triangles_on_both_paths(gpu_ctx):
    rng = np.random.default_rng(6)
    n = 3000
    centre = np.stack([rng.uniform(-4.5, 4.5, n), rng.uniform(-4.5, 4.5, n), rng.uniform(3, 6, n)], 1)
    pts = (centre[:, None, :] + rng.normal(0, 0.12, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    cols = colours(3 * n, 7)
    first = both(gpu_ctx, pts, cols, faces, NO_LINES, NO_COLS, V0, CAM64, (64, 64))
    assert len(np.unique(kinds(first[0][1])[1])) > 500                  # hundreds of different faces are visible
    # each visible face is at least one tile: far more than the 64-entry list of the last forced mode
    every_mode_equals(gpu_ctx, first, pts, cols, faces, NO_LINES, NO_COLS, V0, CAM64, (64, 64))


def test_one_numpy_view_forwards_mode_and_chunk(gpu_ctx):
    """one numpy view with a forced mode or chunk goes through slam_render_views_dev, which takes them"""
    pts = [at(-3000, -3000), at(6000, -3000), at(-3000, 6000)]
    with pytest.raises(L.SlamError):
        api.renderViews(np.asarray(pts, np.float32), colours(3), np.array([[0, 1, 2]], np.int32), NO_LINES, NO_COLS, V0,
                        camera=CAM64, size=(64, 64), ctx=gpu_ctx, raster_mode=9)
    with pytest.raises(L.SlamError):
        api.renderViews(np.asarray(pts, np.float32), colours(3), np.array([[0, 1, 2]], np.int32), NO_LINES, NO_COLS, V0,
                        camera=CAM64, size=(64, 64), ctx=gpu_ctx, chunk_views=-1)


def test_megapixel_view_with_few_primitives(gpu_ctx):
    """1000 x 1000, the default camera: a face over the whole viewport with its vertices
    far outside, faces that straddle the camera plane, big points, long lines"""
    cam = RR.default_camera((1000, 1000))
    view = (rot([0, 1, 0], 0.2), np.array([0.1, -0.1, -1.0]))
    world = lambda q: np.asarray(q, np.float64) @ view[0].T + view[1]
    c = lambda u, v, z: at(u, v, z, cam)
    pts = np.array([world(p) for p in (
        c(-4000, -3000, 9), c(9000, -2000, 9), c(300, 12000, 9),          # covers everything
        c(100.5, 100.5, 3), c(900.5, 150.5, 2), c(480.5, 800.5, -0.5),     # one vertex behind
        c(200, 900, 1), c(800, 950, -2), c(500, 400, -1),                  # two behind
        c(510.5, 20.5, 1), c(-0.5, 999.5, 1), c(999.99, 999.99, 1))], np.float32)
    faces = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [3, 9, 4]]
    lines = np.array([np.concatenate([world(c(-500, 30, 5)), world(c(1500, 970, 1))]),
                      np.concatenate([world(c(10, 990, 1)), world(c(990, 10, 8))]),
                      np.concatenate([world(c(500, 500, 2)), world(c(500, 2500, -1))])], np.float32)
    first = both(gpu_ctx, pts, colours(12, 5), faces, lines, colours(3, 6), [view], cam, (1000, 1000), point_size=7)
    every_mode_equals(gpu_ctx, first, pts, colours(12, 5), faces, lines, colours(3, 6), [view], cam, (1000, 1000), point_size=7)
    got = first[0]
    kind, index = kinds(got[1][0])
    assert (kind != -1).all()
    assert ((kind == 2) & (index == 1)).sum() > 10000 and (kind == 1).sum() > 1500 and (kind == 0).sum() > 100


def test_bad_arguments(gpu_ctx):
    lib = slamhip.lib()
    c = gpu_ctx.handle
    view = np.concatenate([np.eye(3).ravel(), np.zeros(3)])
    cam33 = np.asarray(CAM33, np.float64)
    out = np.zeros((17, 33, 3), np.uint8)

    def call(cam=CAM33, w=33, h=17, point_size=1, v=view, n_faces=0, faces=None):
        cam = np.asarray(cam, np.float64)
        return lib.slam_render(c, None, None, 0, faces, n_faces, None, None, 0, L.ptr(np.asarray(v, np.float64)), L.ptr(cam), w, h,
                               point_size, L.ptr(out), None, None)

    assert call() == L.SLAM_OK
    st = api.renderStats(gpu_ctx)[0]
    bad = [dict(w=0), dict(w=8193), dict(h=0), dict(h=8193), dict(point_size=0), dict(point_size=2), dict(point_size=9),
           dict(cam=(0.0,) + CAM33[1:]), dict(cam=CAM33[:1] + (0.0,) + CAM33[2:]), dict(cam=(math.nan,) + CAM33[1:]),
           dict(cam=CAM33[:4] + (2.0, 2.0)), dict(cam=CAM33[:4] + (3.0, 2.0)), dict(cam=CAM33[:4] + (0.0, 2.0)),
           dict(v=np.full(12, np.inf)), dict(n_faces=-1), dict(n_faces=1, faces=None)]
    for kw in bad:
        assert call(**kw) == L.SLAM_E_INVALID_ARG, kw
    assert api.renderStats(gpu_ctx)[0] == st                             # nothing ran
    assert lib.slam_render_views_dev(c, None, None, None, 0, None, 0, None, None, 0, L.ptr(view), 1, L.ptr(cam33),
                                     33, 17, 1, None, None, None, 0, 0) == L.SLAM_E_INVALID_ARG
    assert lib.slam_render_views_dev(c, None, None, None, 0, None, 0, None, None, 0, L.ptr(view), 0, L.ptr(cam33),
                                     33, 17, 1, None, None, None, 0, 7) == L.SLAM_E_INVALID_ARG
    with pytest.raises(L.SlamError):
        api.renderViews(NO_PTS, NO_COLS, NO_FACES, NO_LINES, NO_COLS, V0, camera=CAM33, size=(33, 17), point_size=4, ctx=gpu_ctx)
    assert lib.slam_render_last_stats(c, None, None) == L.SLAM_E_INVALID_ARG


E2E_CAM = (96.0, 96.0, 48.0, 48.0, 0.01, 100.0)


def test_end_to_end_scene(gpu_ctx, tmp_path):
    """clustered cloud -> segment -> mesh -> render at 96 x 96 from a view one unit
    in front of the largest blob, with three camera poses beside it; then
    scene.main(render=...) on the same data written as result files"""
    pts, cols = R.clustered_cloud(3000, blobs=4)
    gd = cycle.GlobalData()
    gd.push_points(pts.astype(np.float64), cols)
    cfg = slamhip.reference_example()
    cfg.update(TriangleMaxDistance=0.25, TriangleEuclidDistanceWeight=1.0, TriangleColorDistance=0.02,
               TriangleMinimumPoints=6, onlyViz=True, outputDataDir=str(tmp_path))
    segs = scene.segment(gd, slamhip.ConfigService(cfg), ctx=gpu_ctx)
    centre = max(segs, key=lambda s: len(s.indices)).points.astype(np.float64).mean(0)
    poses = [centre + d for d in ([-0.3, 0.1, -0.2], [0.0, -0.1, -0.25], [0.3, 0.15, -0.2])]
    gd.cameraRotations = [rot([0, 1, 0], 0.2 * i) for i in range(3)]
    gd.spatialCameraPositions = [p.reshape(3, 1) for p in poses]
    meshes = scene.mesh(segs, ctx=gpu_ctx)
    view = (I3, centre - [0, 0, 1.0])
    prims = scene.scene_primitives(gd, meshes)
    want = RR.render(*prims, [view], E2E_CAM, (96, 96))
    kind = kinds(want[1][0])[0]
    assert (kind == L.RENDER_FACE).sum() >= 200 and (kind == L.RENDER_POINT).sum() >= 50 and (kind == L.RENDER_LINE).sum() >= 10
    got = scene.render(gd, meshes, views=[view], camera=E2E_CAM, size=(96, 96), ids=True, depth=True, ctx=gpu_ctx)
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()

    logs = cycle.Logs(str(tmp_path))
    for Rm, p in zip(gd.cameraRotations, gd.spatialCameraPositions):
        logs.pose(Rm, p)
    logs.close(gd)
    cfg_path = tmp_path / "config.json"
    cfg_path.write_text(json.dumps(cfg))
    scene.main(str(cfg_path), render="view.png")
    loaded = scene.load_global_data(str(tmp_path))
    frame = scene.render(loaded, scene.mesh(scene.segment(loaded, slamhip.ConfigService(cfg))))[0]
    w, h, rgb = decode_png((tmp_path / "view.png").read_bytes())
    assert (w, h) == (1000, 1000) and np.array_equal(rgb, frame[:, :, ::-1])
    scene.main(str(cfg_path), render=("fly_%02d.ppm", "ws"))
    assert (tmp_path / "fly_00.ppm").exists() and (tmp_path / "fly_01.ppm").exists() and not (tmp_path / "fly_02.ppm").exists()

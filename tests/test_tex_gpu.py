"""GPU tests of the per-face texture atlas (csrc/tex.hip behind slam_tex_select*, slam_tex_fill* and
slamhip.surface.texture): every device result equals tests/tex_ref.py bit for bit; the cases are those of
tests/test_tex.py.
"""
import ctypes

import numpy as np
import pytest

import tex_ref as R
import slamhip
from slamhip import _lib as L
from slamhip import cycle, dense, scene, surface

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel elements on each side of an output buffer
SELECT = R.select_cases()
FILL = R.fill_cases()


def _guarded(torch, n, dtype, fill, body=None, shift=0):
    t = torch.full((n + 2 * GUARD + shift,), fill, dtype=dtype, device="cuda")
    if body is not None:
        t[GUARD + shift:GUARD + shift + n] = body
    return t, ctypes.c_void_p(t.data_ptr() + (GUARD + shift) * t.element_size())


def _guards_intact(t, n, fill, shift=0):
    a = t.cpu().numpy()
    return bool((a[:GUARD + shift] == fill).all() and (a[GUARD + shift + n:] == fill).all())


def _body(t, n, shift=0):
    return t.cpu().numpy()[GUARD + shift:GUARD + shift + n]


def _select_guarded(torch, ctx, ids, view0, nf, state=None):
    """slam_tex_select_dev into a state of exactly nf elements between sentinels -> (best_count, best_view)"""
    bc, pbc = _guarded(torch, nf, torch.int32, -77, 0 if state is None else torch.from_numpy(state[0]).cuda())
    bv, pbv = _guarded(torch, nf, torch.int32, -78, -1 if state is None else torch.from_numpy(state[1]).cuda())
    d_ids = torch.from_numpy(np.ascontiguousarray(ids)).cuda()
    torch.cuda.synchronize()
    rc = slamhip.lib().slam_tex_select_dev(ctx.handle, None, ctypes.c_void_p(d_ids.data_ptr()), ids.shape[0], ids.shape[1],
                                           ids.shape[2], view0, nf, pbc, pbv)
    assert rc == L.SLAM_OK
    assert _guards_intact(bc, nf, -77) and _guards_intact(bv, nf, -78)
    return _body(bc, nf), _body(bv, nf)


@pytest.mark.parametrize("case", SELECT, ids=[c[0] for c in SELECT])
def test_select_device_equals_contract(gpu_ctx, case):
    """h w no multiple of 64, runs across wave boundaries, one face on every pixel, every pixel another face,
    nf = 1; the resident entry between sentinels and the host-pointer entry"""
    import torch
    _, ids, nf = case
    want = R.select(R.empty_state(nf), ids, 3, nf)
    got = _select_guarded(torch, gpu_ctx, ids, 3, nf)
    assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1])
    host = slamhip.texSelect(ids, 3, nf, ctx=gpu_ctx)
    assert R.same_bits(host[0], want[0]) and R.same_bits(host[1], want[1])
    assert slamhip.texLastTiming(gpu_ctx)["select"] > 0


@pytest.mark.parametrize("parts", [[(0, 1), (1, 2), (2, 3)], [(0, 2), (2, 3)], [(2, 3), (1, 2), (0, 1)], [(2, 3), (0, 2)]],
                         ids=["1+1+1", "2+1", "1+1+1-reversed", "2+1-reversed"])
def test_select_split_over_calls(gpu_ctx, parts):
    import torch
    for _, ids, nf in (SELECT[0], SELECT[-1]):
        want = R.select(R.empty_state(nf), ids[:3], 0, nf)
        st = None
        for a, b in parts:
            st = _select_guarded(torch, gpu_ctx, ids[a:b], a, nf, st)
        assert R.same_bits(st[0], want[0]) and R.same_bits(st[1], want[1])


@pytest.fixture(scope="module")
def contract_fill():
    return {c[0]: R.fill(*c[1:]) for c in FILL}


def _fill_guarded(torch, ctx, case, nbytes, shift=0):
    name, V, C, F, frames, fidx, P, bc, bv, mp, T, page = case
    atlas, pa = _guarded(torch, nbytes, torch.uint8, 0xEE, shift=shift)
    fr = torch.from_numpy(np.stack(frames)).cuda()
    ch = 1 if fr.dim() == 3 else 3
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (V, C, F, bc, bv)]
    Pc = np.ascontiguousarray(np.stack(P), np.float64).reshape(-1, 12)
    fi = np.ascontiguousarray(fidx, np.int32)
    torch.cuda.synchronize()
    rc = slamhip.lib().slam_tex_fill_dev(ctx.handle, None, *[ctypes.c_void_p(t.data_ptr()) for t in d[:3]], len(V), len(F),
                                         ctypes.c_void_p(fr.data_ptr()), fr.shape[0], fr.shape[1], fr.shape[2], ch, L.ptr(fi),
                                         L.ptr(Pc), len(Pc), ctypes.c_void_p(d[3].data_ptr()), ctypes.c_void_p(d[4].data_ptr()),
                                         mp, T, page, pa)
    return rc, atlas


@pytest.mark.parametrize("case", FILL, ids=[c[0] for c in FILL])
def test_fill_device_equals_contract(gpu_ctx, contract_fill, case):
    """both halves and an odd nf, three pages, gray and BGR, behind the camera and outside the image, below
    min_pixels, non-finite P, a one-cell page: the atlas of exactly the needed size between sentinels, at an
    aligned and at an odd address, and through the host-pointer entry"""
    import torch
    name, V, C, F, frames, fidx, P, bc, bv, mp, T, page = case
    want = np.concatenate([p.ravel() for p in contract_fill[name]])
    for shift in (0, 1):
        rc, atlas = _fill_guarded(torch, gpu_ctx, case, len(want), shift)
        assert rc == L.SLAM_OK
        assert _guards_intact(atlas, len(want), 0xEE, shift)
        assert R.same_bits(_body(atlas, len(want), shift), want), shift
    assert slamhip.texLastTiming(gpu_ctx)["fill"] > 0
    got = slamhip.texFill(V, C, F, frames, P, bc, bv, mp, T, page, frame_idx=fidx, ctx=gpu_ctx)
    assert all(R.same_bits(a, b) for a, b in zip(got, contract_fill[name]))


def test_argument_errors_on_device(gpu_ctx):
    import torch
    case = list(FILL[0])
    F, bv = case[3], case[8]
    n = sum(p.size for p in R.fill(*case[1:]))
    badF, bigv = F.copy(), bv.copy()
    badF[6, 2] = len(case[1])
    bigv[5] = 3
    for k, val in ((3, badF), (8, bigv), (9, 0), (10, 65), (11, 8), (5, [0, 1, 3])):
        bad = list(case)
        bad[k] = val
        rc, atlas = _fill_guarded(torch, gpu_ctx, bad, n)
        assert rc == L.SLAM_E_INVALID_ARG, k
        assert (atlas.cpu().numpy() == 0xEE).all(), k          # nothing is filled
    one = torch.zeros(16, dtype=torch.int32, device="cuda")
    p = ctypes.c_void_p(one.data_ptr())
    lib = slamhip.lib()
    assert lib.slam_tex_select_dev(gpu_ctx.handle, None, None, 1, 2, 2, 0, 4, p, p) == L.SLAM_E_INVALID_ARG
    assert lib.slam_tex_select_dev(gpu_ctx.handle, None, p, 1, 2, 2, 0, (1 << 30) + 1, p, p) == L.SLAM_E_UNSUPPORTED
    assert lib.slam_tex_select_dev(gpu_ctx.handle, None, None, 0, 2, 2, 0, 0, None, None) == L.SLAM_OK
    assert lib.slam_tex_fill_dev(gpu_ctx.handle, None, None, None, None, 0, 0, None, 0, 4, 4, 3, None, None, 0, None, None, 4, 5, 64,
                                 None) == L.SLAM_OK


def _known_case(make, prm):
    case = make()
    views = list(range(len(case["frames"])))
    case["params"] = prm
    case["ids"] = case.get("ids", None)
    if case["ids"] is None:
        case["ids"] = R.render_ids(case["V"], case["C"], case["F"], case["K"], case["rotations"], case["positions"], views, case["size"])
    case["want"] = R.texture(case["V"], case["C"], case["F"], case["frames"], case["K"], case["rotations"], case["positions"], prm,
                             ids=case["ids"])
    return case


@pytest.mark.parametrize("which", ["plane", "occlusion"])
def test_surface_texture_equals_contract_pipeline(gpu_ctx, which):
    """surface.texture with the device rasteriser's ids equals the contract with render_ref's ids: the ids, the
    selection, the atlas and the UVs; chunks of one view and of all views alike"""
    if which == "plane":
        case = _known_case(R.plane_case, surface.TextureParams(texel=12, page=128, min_pixels=4))
    else:
        case = _known_case(R.occlusion_case, surface.TextureParams(texel=6, page=128, min_pixels=2))
    uv, fp, atlas, bv, bc = case["want"]
    for chunk in (1, 8):
        got = surface.texture(case["V"], case["C"], case["F"], case["frames"], case["K"], case["rotations"], case["positions"],
                              case["params"], ctx=gpu_ctx, chunk=chunk)
        assert R.same_bits(got.best_count, bc) and R.same_bits(got.best_view, bv), chunk
        assert R.same_bits(got.uv, uv) and R.same_bits(got.page, fp)
        assert len(got.atlas) == len(atlas) and all(R.same_bits(a, b) for a, b in zip(got.atlas, atlas)), chunk
    if which == "plane":
        assert got.textured.all()
    else:
        assert (bv[case["hidden"]] == 1).all()
    two = surface.texture(case["V"], case["C"], case["F"], case["frames"], case["K"], case["rotations"], case["positions"],
                          surface.TextureParams(texel=case["params"].texel, page=128, min_pixels=case["params"].min_pixels, max_views=1),
                          ctx=gpu_ctx)
    assert two.views == [len(case["frames"]) // 2] and set(two.best_view.tolist()) <= {-1, 0}


def test_slam_main_texture(gpu_ctx, tmp_path):
    """the 16-frame synthetic sequence of test_tsdf_gpu.py: the texture option adds surface.obj, surface.mtl and the
    atlas pages and changes no other file; more than half of the faces are textured"""
    from test_cycle import K_VGA, _cfg
    frames = slamhip.synth_frames(640, 480, 0, 16, seed=1234)
    cfg = _cfg()
    prm = dense.DenseParams(D=16, sources=2, step=16)
    tp = surface.TextureParams(texel=4, page=256)
    outs = {}
    for name, t in (("plain", None), ("textured", tp)):
        K = K_VGA.copy()
        gd, logs = cycle.slam_main(cycle.MediaSources(list(frames)), K, cfg, cycle.GpuOps(gpu_ctx), out_dir=str(tmp_path / name),
                                   dense=prm, surface=surface.SurfaceParams(max_dim=48, min_weight=1, texture=t))
        outs[name] = (gd, logs, K)
    plain = sorted(p.name for p in (tmp_path / "plain").iterdir())
    assert "surface.ply" in plain and not any(n.endswith((".obj", ".mtl", ".png")) for n in plain)
    for f in plain:
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "textured" / f).read_bytes(), f
    assert not hasattr(outs["plain"][0], "surfaceTexture")
    gd, logs, K = outs["textured"]
    tx = gd.surfaceTexture
    nf = len(gd.surfaceFaces)
    share = float(tx.textured.mean()) if nf else 0.0
    print("texture:", nf, "faces,", len(tx.atlas), "pages,", len(tx.views), "views, textured share", share)
    extra = sorted(set(p.name for p in (tmp_path / "textured").iterdir()) - set(plain))
    assert extra == ["surface.mtl", "surface.obj"] + [f"surface_atlas_{p}.png" for p in range(len(tx.atlas))] and len(tx.atlas) >= 1
    assert nf > 0 and share > 0.5
    lv, lf, luv, lp, la = scene.load_textured_mesh(str(tmp_path / "textured" / "surface.obj"))
    assert R.same_bits(lf, gd.surfaceFaces) and R.same_bits(luv, tx.uv) and R.same_bits(lp, tx.page)
    assert all(R.same_bits(a, b) for a, b in zip(la, tx.atlas))
    # the host twins on the device's state give the same atlas
    host = slamhip.texFill(gd.surfaceVertices, gd.surfaceColors, gd.surfaceFaces, [np.asarray(f) for f in _host_frames(logs.frames)],
                           [surface.projection_matrix(K, gd.cameraRotations[i], gd.spatialCameraPositions[i]) for i in tx.views],
                           tx.best_count, tx.best_view, tp.min_pixels, tp.texel, tp.page, frame_idx=tx.views, host=True)
    assert all(R.same_bits(a, b) for a, b in zip(host, tx.atlas))


def _host_frames(frames):
    return dense.stage_frames(frames, True)

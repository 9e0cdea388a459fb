"""GPU tests of TSDF fusion and marching cubes (csrc/tsdf.hip behind slam_tsdf_integrate*, slam_tsdf_mesh*
and slamhip.surface): every device result equals tests/tsdf_ref.py bit for bit; the cases are those of
tests/test_tsdf.py.
"""
import ctypes
import json

import numpy as np
import pytest

import tsdf_ref as R
import slamhip
from slamhip import _lib as L
from slamhip import cycle, dense, scene, surface

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel elements on each side of an output buffer
CASES = R.integrate_cases()


def _guarded(torch, n, dtype, fill, body=None):
    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    if body is not None:
        t[GUARD:GUARD + n] = body
    return t, ctypes.c_void_p(t.data_ptr() + GUARD * t.element_size())


def _guards_intact(t, n, fill):
    a = t.cpu().numpy()
    return bool((a[:GUARD] == fill).all() and (a[GUARD + n:] == fill).all())


@pytest.fixture(scope="module")
def contract():
    """per case: the contract's volume and its meshes at min_weight 1 and 2, computed once"""
    out = {}
    for name, fr, inv, P, dims, origin, voxel, trunc in CASES:
        vol = R.integrate(R.empty_volume(*dims), fr, inv, P, origin, voxel, trunc)
        out[name] = (vol, {mw: R.mesh(vol, origin, voxel, mw) for mw in (1, 2)})
    return out


def _integrate_guarded(torch, ctx, fr, inv, P, dims, origin, voxel, trunc, frame_idx=None, start=None):
    """slam_tsdf_integrate_dev into a volume between sentinels -> (the guarded tensor, its body's pointer, n)"""
    nx, ny, nz = dims
    n = 6 * nx * ny * nz
    vol, pv = _guarded(torch, n, torch.int32, -77, 0 if start is None else torch.from_numpy(start.reshape(-1)).cuda())
    frames = torch.from_numpy(np.stack(fr)).cuda()
    maps = torch.from_numpy(np.stack(inv)).cuda()
    h, w = inv[0].shape
    Pc = np.ascontiguousarray(np.stack(P), np.float64).reshape(-1, 12)
    fi = None if frame_idx is None else np.ascontiguousarray(frame_idx, np.int32)
    org = np.ascontiguousarray(origin, np.float64)
    torch.cuda.synchronize()
    rc = slamhip.lib().slam_tsdf_integrate_dev(ctx.handle, None, pv, nx, ny, nz, L.ptr(org), float(voxel), float(trunc),
                                               ctypes.c_void_p(frames.data_ptr()), len(fr), w, h, 1 if fr[0].ndim == 2 else 3,
                                               L.ptr(fi), ctypes.c_void_p(maps.data_ptr()), L.ptr(Pc), len(Pc))
    assert rc == L.SLAM_OK
    return vol, pv, n


def _mesh_guarded(torch, ctx, pv, dims, origin, voxel, mw, nv, nf):
    """slam_tsdf_mesh_dev into outputs of exactly nv / nf elements between sentinels"""
    v, pvv = _guarded(torch, 3 * nv, torch.float64, -5.0)
    c, pc = _guarded(torch, 3 * nv, torch.uint8, 99)
    f, pf = _guarded(torch, 3 * nf, torch.int32, -9)
    gv, gf = ctypes.c_int(-1), ctypes.c_int(-1)
    org = np.ascontiguousarray(origin, np.float64)
    torch.cuda.synchronize()
    rc = slamhip.lib().slam_tsdf_mesh_dev(ctx.handle, None, pv, *dims, L.ptr(org), float(voxel), mw, pvv, pc, pf, nv, nf,
                                          ctypes.byref(gv), ctypes.byref(gf))
    return rc, gv.value, gf.value, (v, c, f)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_contract(gpu_ctx, contract, case):
    """the volume after integration and the vertices, colours and faces at both weights, each output of exactly
    the needed size between 64 sentinels on each side"""
    import torch
    name, fr, inv, P, dims, origin, voxel, trunc = case
    want_vol, want_mesh = contract[name]
    vol, pv, n = _integrate_guarded(torch, gpu_ctx, fr, inv, P, dims, origin, voxel, trunc)
    assert _guards_intact(vol, n, -77)
    assert R.same_bits(vol.cpu().numpy()[GUARD:GUARD + n].reshape(want_vol.shape), want_vol)
    for mw in (1, 2):
        wv, wc, wf = want_mesh[mw]
        rc, nv, nf, (v, c, f) = _mesh_guarded(torch, gpu_ctx, pv, dims, origin, voxel, mw, len(wv), len(wf))
        assert rc == L.SLAM_OK and (nv, nf) == (len(wv), len(wf))
        assert _guards_intact(v, 3 * nv, -5.0) and _guards_intact(c, 3 * nv, 99) and _guards_intact(f, 3 * nf, -9)
        assert R.same_bits(v.cpu().numpy()[GUARD:GUARD + 3 * nv].reshape(-1, 3), wv)
        assert R.same_bits(c.cpu().numpy()[GUARD:GUARD + 3 * nv].reshape(-1, 3), wc)
        assert R.same_bits(f.cpu().numpy()[GUARD:GUARD + 3 * nf].reshape(-1, 3), wf)


@pytest.mark.parametrize("vol", R.planted_mesh_volumes(), ids=[n for n, _ in R.planted_mesh_volumes()])
def test_device_mesh_on_planted_volumes(gpu_ctx, vol):
    """the sphere, random signs (every ambiguous case), D == 0 at nodes, unknown nodes inside the grid, the empty
    and the all-inside volume, through the resident and the host-pointer entry"""
    import torch
    name, vol = vol
    origin, voxel = (0.5, -1.0, 2.0), 0.25
    dv = torch.from_numpy(vol).cuda()
    for mw in (1, 2):
        want = R.mesh(vol, origin, voxel, mw)
        got = slamhip.tsdfMesh(dv, origin, voxel, mw, ctx=gpu_ctx)
        assert all(R.same_bits(a, b) for a, b in zip(want, got)), mw
        got = slamhip.tsdfMesh(vol, origin, voxel, mw, ctx=gpu_ctx)
        assert all(R.same_bits(a, b) for a, b in zip(want, got)), mw
        if name in ("empty", "all-inside"):
            assert len(got[0]) == 0 and len(got[2]) == 0


def test_capacity_error_reports_both_counts_and_writes_nothing(gpu_ctx, contract):
    import torch
    name, fr, inv, P, dims, origin, voxel, trunc = next(c for c in CASES if c[0] == "9x7x5-3maps-3ch")
    wv, wc, wf = contract[name][1][1]
    assert len(wv) > 50 and len(wf) > 50
    dv = torch.from_numpy(contract[name][0]).cuda()
    pv = ctypes.c_void_p(dv.data_ptr())
    for cv, cf in ((len(wv) - 1, len(wf)), (len(wv), len(wf) - 1), (0, 0)):
        rc, nv, nf, (v, c, f) = _mesh_guarded(torch, gpu_ctx, pv, dims, origin, voxel, 1, cv, cf)
        assert rc == L.SLAM_E_CAPACITY and (nv, nf) == (len(wv), len(wf))
        assert (v.cpu().numpy() == -5.0).all() and (c.cpu().numpy() == 99).all() and (f.cpu().numpy() == -9).all()
    with pytest.raises(L.SlamError) as e:
        slamhip.tsdfMesh(dv, origin, voxel, 1, cap=(len(wv), len(wf) - 1), ctx=gpu_ctx)
    assert e.value.code == L.SLAM_E_CAPACITY and e.value.needed == (len(wv), len(wf))
    old = slamhip.api.TSDF_MESH_CAP
    try:
        slamhip.api.TSDF_MESH_CAP = (3, 3)          # cap=None: one retry with the needed counts
        got = slamhip.tsdfMesh(dv, origin, voxel, 1, ctx=gpu_ctx)
    finally:
        slamhip.api.TSDF_MESH_CAP = old
    assert R.same_bits(got[0], wv) and R.same_bits(got[2], wf)


def test_chunked_integration_equals_single_call(gpu_ctx, contract):
    """maps [0, 1, 2] in one call, [2] then [0, 1], and one map per call: the same volume bits; the host-pointer
    entry too"""
    import torch
    name, fr, inv, P, dims, origin, voxel, trunc = next(c for c in CASES if c[0] == "17^3-3maps-3ch")
    want = contract[name][0]
    frames = torch.from_numpy(np.stack(fr)).cuda()
    maps = torch.from_numpy(np.stack(inv)).cuda()
    Pa = np.stack(P)
    for split in ([[2], [0, 1]], [[0], [1], [2]], [[1, 2, 0]]):
        vol = torch.zeros(want.shape, dtype=torch.int32, device="cuda")
        for part in split:
            slamhip.tsdfIntegrate(vol, frames, maps[part], Pa[part], origin, voxel, trunc, frame_idx=part, ctx=gpu_ctx)
        assert R.same_bits(vol.cpu().numpy(), want), split
    hv = slamhip.tsdfIntegrate(R.empty_volume(*dims), fr, inv, P, origin, voxel, trunc, ctx=gpu_ctx)
    assert R.same_bits(hv, want)
    t = slamhip.tsdfLastTiming(gpu_ctx)
    assert t["integrate"] > 0


def test_frustum_cuts_through_a_workgroup(gpu_ctx):
    """a 70 x 9 x 5 volume (70 nodes in x: more than one wave) and one map whose frustum covers only part of it:
    nodes left of, inside and right of the image within one row of a workgroup"""
    import torch
    fr, inv, P = R.scene(1, 3, seed=4)
    dims, origin, voxel, trunc = (70, 9, 5), (-1.4, -0.4, 1.9), 0.04, 0.3
    want = R.integrate(R.empty_volume(*dims), fr, inv, P, origin, voxel, trunc)
    seen = want[1][2, 4]
    assert seen[0] == 0 and seen[-1] == 0 and seen.max() == 1 and 10 < seen.sum() < 60
    vol, pv, n = _integrate_guarded(torch, gpu_ctx, fr, inv, P, dims, origin, voxel, trunc)
    assert _guards_intact(vol, n, -77)
    got = vol.cpu().numpy()[GUARD:GUARD + n].reshape(want.shape)
    assert R.same_bits(got, want)
    assert R.same_bits(slamhip.tsdfIntegrate(R.empty_volume(*dims), fr, inv, P, origin, voxel, trunc, host=True), want)
    wm = R.mesh(want, origin, voxel, 1)
    gm = slamhip.tsdfMesh(torch.from_numpy(got).cuda(), origin, voxel, 1, ctx=gpu_ctx)
    assert len(wm[2]) > 0 and all(R.same_bits(a, b) for a, b in zip(wm, gm))


def test_argument_errors_on_device(gpu_ctx):
    import torch
    fr, inv, P = R.scene(1, 3)
    frames, maps = torch.from_numpy(np.stack(fr)).cuda(), torch.from_numpy(np.stack(inv)).cuda()
    vol = torch.zeros((6, 3, 3, 3), dtype=torch.int32, device="cuda")
    bad = np.stack(P)
    bad[0, 0, 0] = np.nan
    for kw in (dict(voxel=0.0), dict(trunc=-1.0), dict(trunc=np.inf), dict(P=bad), dict(frame_idx=[1]),
               dict(origin=(np.inf, 0.0, 0.0))):
        a = dict(P=np.stack(P), origin=(0.0, 0.0, 1.0), voxel=0.1, trunc=0.4, frame_idx=None)
        a.update(kw)
        with pytest.raises(L.SlamError) as e:
            slamhip.tsdfIntegrate(vol, frames, maps, a["P"], a["origin"], a["voxel"], a["trunc"], frame_idx=a["frame_idx"],
                                  ctx=gpu_ctx)
        assert e.value.code == L.SLAM_E_INVALID_ARG, kw
    assert int(vol.abs().sum()) == 0
    with pytest.raises(L.SlamError) as e:
        slamhip.tsdfMesh(vol, (0, 0, 0), 1.0, min_weight=0, ctx=gpu_ctx)
    assert e.value.code == L.SLAM_E_INVALID_ARG
    nv, nf = ctypes.c_int(0), ctypes.c_int(0)
    org = np.zeros(3)
    for dims in ((1, 3, 3), (2, 2, 2049), (2048, 2048, 512)):
        rc = slamhip.lib().slam_tsdf_mesh_dev(gpu_ctx.handle, None, ctypes.c_void_p(vol.data_ptr()), *dims, L.ptr(org), 1.0, 1,
                                              None, None, None, 0, 0, ctypes.byref(nv), ctypes.byref(nf))
        assert rc == L.SLAM_E_UNSUPPORTED, dims


def test_reconstruct_planted_sequence(gpu_ctx):
    """the planted wall: the device path equals host=True bit for bit and the surface is not empty"""
    frames, K, rot, pos, sparse = R.planted_sequence()
    prm = dense.DenseParams(D=12, sources=1, eps=0.25, step=4)
    sp = surface.SurfaceParams(max_dim=48, min_weight=1)
    got = surface.reconstruct(frames, K, rot, pos, sparse, prm, sp, ctx=gpu_ctx)
    want = surface.reconstruct(frames, K, rot, pos, sparse, prm, sp, host=True)
    assert len(want[2]) > 0 and want[2].max() < len(want[0])
    assert all(R.same_bits(a, b) for a, b in zip(got, want))
    # chunk size does not matter
    one = surface.reconstruct(frames, K, rot, pos, sparse, prm, sp, ctx=gpu_ctx, chunk=1)
    assert all(R.same_bits(a, b) for a, b in zip(one, want))


def test_slam_main_surface(gpu_ctx, tmp_path):
    from test_cycle import K_VGA, _cfg
    frames = slamhip.synth_frames(640, 480, 0, 16, seed=1234)
    cfg = _cfg()
    prm = dense.DenseParams(D=16, sources=2, step=16)
    sp = surface.SurfaceParams(max_dim=48, min_weight=1)
    outs = {}
    for name, s in (("dense", None), ("surface", sp)):
        K = K_VGA.copy()
        gd, logs = cycle.slam_main(cycle.MediaSources(list(frames)), K, cfg, cycle.GpuOps(gpu_ctx), out_dir=str(tmp_path / name),
                                   dense=prm, surface=s)
        outs[name] = (gd, logs, K)
    for f in ("poses.txt", "rotations.txt", "points.txt", "colors.txt", "dense_points.txt", "dense_colors.txt"):
        assert (tmp_path / "dense" / f).read_bytes() == (tmp_path / "surface" / f).read_bytes(), f
    assert not (tmp_path / "dense" / "surface.ply").exists() and not hasattr(outs["dense"][0], "surfaceFaces")
    gd, logs, K = outs["surface"]
    want = surface.reconstruct(logs.frames, K, gd.cameraRotations, gd.spatialCameraPositions, gd.spatialPoints, prm, sp, host=True)
    print("surface:", len(gd.surfaceVertices), "vertices,", len(gd.surfaceFaces), "faces")
    assert len(gd.surfaceFaces) > 0 and gd.surfaceFaces.max() < len(gd.surfaceVertices)
    assert R.same_bits(want[0], gd.surfaceVertices) and R.same_bits(want[1], gd.surfaceColors)
    assert R.same_bits(want[2], gd.surfaceFaces)
    scene.write_mesh(want[0], want[1], [scene.Mesh(want[2], want[2])], str(tmp_path / "host.ply"))
    assert (tmp_path / "host.ply").read_bytes() == (tmp_path / "surface" / "surface.ply").read_bytes()
    d = slamhip.reference_example()
    d.update(onlyViz=True, outputDataDir=str(tmp_path / "surface"))
    (tmp_path / "config.json").write_text(json.dumps(d))
    assert scene.main(str(tmp_path / "config.json"), render="view.png", cloud="surface") == []
    png = (tmp_path / "surface" / "view.png").read_bytes()
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and len(png) > 1000
    assert not (tmp_path / "surface" / "clusters.txt").exists() and not (tmp_path / "surface" / "mesh.ply").exists()
    lv, lc, lf = scene.load_surface(str(tmp_path / "surface" / "surface.ply"))
    assert len(lv) == len(want[0]) and np.array_equal(lc, want[1]) and np.array_equal(lf, want[2])

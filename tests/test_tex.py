"""CPU tests of the per-face texture atlas: the contract tests/tex_ref.py against
itself (layout properties, known answers), the host twins against the contract bit for bit, the surface
and scene modules' helpers, and the host twins under sanitizers as a stand-alone program."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import tex_ref as R
import slamhip
from slamhip import _lib as L
from slamhip import scene, surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-indoor-code_amd", "csrc")


# ---- layout ------------------------------------------------------------------------------------------

def _layout_cases():
    for T in (1, 2, 5, 12):
        S = T + 4
        for page in (S, 64, 100):
            cpp = (page // S) ** 2
            for nf in (0, 1, 2, 3, 2 * cpp - 1, 2 * cpp, 2 * cpp + 1):
                yield T, page, nf


def _near_triangle(tri, hgt, wid):
    """(H, W) bool: texels whose centre is less than one texel (Chebyshev) from the closed triangle `tri` (3 x 2,
    texel coordinates): the open square of half-width 1 about the centre meets the triangle.  Separating axes
    of two convex shapes: the square's (x, y) and the triangle's edge normals."""
    y, x = np.mgrid[0:hgt, 0:wid]
    cx, cy = x + 0.5, y + 0.5
    near = (cx + 1 > tri[:, 0].min()) & (cx - 1 < tri[:, 0].max()) & (cy + 1 > tri[:, 1].min()) & (cy - 1 < tri[:, 1].max())
    for k in range(3):
        a, b, c = tri[k], tri[(k + 1) % 3], tri[(k + 2) % 3]
        n = np.array([b[1] - a[1], a[0] - b[0]])
        if n @ (c - a) > 0:
            n = -n                                           # outward
        # the square's least projection on the outward normal must lie below the edge's
        least = n[0] * cx + n[1] * cy - (abs(n[0]) + abs(n[1]))
        near &= least < n @ a
    return near


@pytest.mark.parametrize("T,page,nf", list(_layout_cases()))
def test_layout_properties(T, page, nf):
    S = T + 4
    cells_x = page // S
    pw, ph, uv, fp = R.layout(nf, T, page)
    g = slamhip.texLayout(nf, T, page)
    assert g[0] == pw and g[1] == ph and R.same_bits(g[2], uv) and R.same_bits(g[3], fp)
    # page sizes as stated
    assert pw == cells_x * S
    rows = -(-((nf + 1) // 2) // cells_x)
    assert sum(ph) == rows * S and all(p == cells_x * S for p in ph[:-1]) and len(ph) == -(-rows // cells_x)
    assert all(0 < p <= cells_x * S and p % S == 0 for p in ph)
    if nf == 0:
        assert ph == [] and uv.shape == (0, 3, 2)
        return
    assert uv.min() >= 0.0 and uv.max() <= 1.0
    own = R.owners(nf, T, page)
    assert [o.shape for o in own] == [(p, pw) for p in ph]
    claimed = [np.full(o.shape, -1, np.int64) for o in own]
    for f in range(nf):
        p = fp[f]
        tri = np.stack([uv[f, :, 0] * pw, (1.0 - uv[f, :, 1]) * ph[p]], axis=1)
        assert np.abs(tri - np.round(tri)).max() < 1e-9
        tri = np.round(tri)
        assert abs((tri[1, 0] - tri[0, 0]) * (tri[2, 1] - tri[0, 1]) - (tri[2, 0] - tri[0, 0]) * (tri[1, 1] - tri[0, 1])) == T * T
        near = _near_triangle(tri, ph[p], pw)
        assert near.sum() >= (T + 2) * (T + 3) // 2
        assert (own[p][near] == f).all(), f                  # the margin: a bilinear lookup reads only the face's own texels
        assert (claimed[p][near] == -1).all(), f             # and no texel is near two faces
        claimed[p][near] = f
    # one owner per texel, by construction of owners(); every face owns texels on its page only
    allown = np.concatenate([o.ravel() for o in own])
    assert set(np.unique(allown[allown >= 0])) == set(range(nf))


# ---- selection ---------------------------------------------------------------------------------------

SELECT = R.select_cases()


@pytest.mark.parametrize("case", SELECT, ids=[c[0] for c in SELECT])
def test_select_twin_equals_contract(case):
    _, ids, nf = case
    want = R.select(R.empty_state(nf), ids, 0, nf)
    got = slamhip.texSelect(ids, 0, nf, host=True)
    assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1])


def test_select_hand_case():
    _, ids, nf = SELECT[0]
    bc, bv = R.select(R.empty_state(nf), ids, 0, nf)
    assert bc.tolist() == [2 * 67, 3 * 67, 0, 0, 8 * 37, 0, 0, 0, 1]     # points, lines, -1 and faces >= nf count for nothing
    assert bv.tolist() == [0, 2, -1, -1, 0, -1, -1, -1, 2]              # equal counts: the lowest view; unseen: -1
    cnt = R.count(ids, nf)
    assert cnt[0, 5] == 0 and cnt.sum() == int((((ids.astype(np.int64) & 0xFFFFFFFF) >> 30) == 2).sum()) - 2 * 67


@pytest.mark.parametrize("host", [False, True], ids=["contract", "twin"])
def test_select_any_split_any_order(host):
    _, ids, nf = SELECT[-1]
    assert len(ids) == 4

    def run(parts):
        st = R.empty_state(nf)
        for a, b in parts:
            st = slamhip.texSelect(ids[a:b], a, nf, st, host=True) if host else R.select(st, ids[a:b], a, nf)
        return st

    want = run([(0, 4)])
    assert (want[0] > 0).any() and len(set(want[1].tolist())) >= 4
    splits = [[(0, 1), (1, 2), (2, 3), (3, 4)], [(0, 2), (2, 4)], [(0, 1), (1, 4)], [(0, 3), (3, 4)]]
    for parts in splits:
        for order in itertools.islice(itertools.permutations(parts), 24):
            got = run(list(order))
            assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1]), order
    one = run([(0, 0)])
    assert (one[0] == 0).all() and (one[1] == -1).all()


# ---- fill --------------------------------------------------------------------------------------------

FILL = R.fill_cases()


@pytest.fixture(scope="module")
def contract_fill():
    return {c[0]: R.fill(*c[1:]) for c in FILL}


@pytest.mark.parametrize("case", FILL, ids=[c[0] for c in FILL])
def test_fill_twin_equals_contract(case, contract_fill):
    name, V, C, F, frames, fidx, P, bc, bv, mp, T, page = case
    want = contract_fill[name]
    got = slamhip.texFill(V, C, F, frames, P, bc, bv, mp, T, page, frame_idx=fidx, host=True)
    assert len(got) == len(want) and all(R.same_bits(a, b) for a, b in zip(got, want))


def _gouraud(case):
    """the fallback restated: per texel the extrapolated blend of the vertex colours"""
    _, V, C, F, _, _, _, _, _, _, T, page = case
    S = T + 4
    out = []
    for own in R.owners(len(F), T, page):
        img = np.zeros(own.shape + (3,), np.uint8)
        for (y, x), f in np.ndenumerate(own):
            if f < 0:
                continue
            i, j = x % S, y % S
            if i + j <= T + 2:
                be, ga = (i + 0.5 - 1) / T, (j + 0.5 - 1) / T
            else:
                be, ga = (T + 3 - (i + 0.5)) / T, (T + 3 - (j + 0.5)) / T
            al = (1 - be) - ga
            for k in range(3):
                v = np.floor(((al * float(C[F[f, 0], k]) + be * float(C[F[f, 1], k])) + ga * float(C[F[f, 2], k])) + 0.5)
                img[y, x, k] = min(max(v, 0.0), 255.0)
        out.append(img)
    return out


def test_fill_cases_cover_the_rule(contract_fill):
    by = {c[0]: c for c in FILL}
    assert [p.shape for p in contract_fill["three-pages"]] == [(64, 64, 3), (64, 64, 3), (24, 64, 3)]
    odd = contract_fill["odd-nf-bgr"][0]
    own = R.owners(7, 5, 64)[0]
    assert (own == -1).any() and (odd[own == -1] == 0).all() and odd[own == 6].any()     # the last cell: half empty, black
    g = contract_fill["gray-67x33"]
    tex = np.concatenate([p.reshape(-1, 3) for p in g])
    assert ((tex[:, 0] == tex[:, 1]) & (tex[:, 1] == tex[:, 2])).mean() > 0.9          # gray frames fill the channels alike
    # below min_pixels (and best_view -1): exactly the Gouraud blend
    low = by["below-min-pixels"]
    assert (low[7] < low[9]).all()
    assert all(R.same_bits(a, b) for a, b in zip(contract_fill["below-min-pixels"], _gouraud(low)))
    # a NaN, an infinity, an overflow and denormals in P: the first three fall back for every texel of their faces
    nf_case = by["non-finite-P"]
    gour = _gouraud(nf_case)[0]
    own = R.owners(8, 2, 64)[0]
    got = contract_fill["non-finite-P"][0]
    for f in range(8):
        if nf_case[8][f] in (0, 1, 2):
            assert (got[own == f] == gour[own == f]).all(), f
    # behind the camera falls back; outside the image clamps to a border pixel
    b = by["behind-and-outside"]
    V, F, P, frame = b[1], b[3], b[6][0], b[4][0]
    pts, own = R.texel_points(V, F, 5, 64)[0], R.owners(12, 5, 64)[0]
    hh = pts @ P[:, :3].T + P[:, 3]
    gour, got = _gouraud(b)[0], contract_fill["behind-and-outside"][0]
    behind = (own >= 0) & (hh[..., 2] < -1e-9)
    assert behind.sum() > 20 and (got[behind] == gour[behind]).all()
    with np.errstate(all="ignore"):
        u, v = hh[..., 0] / hh[..., 2], hh[..., 1] / hh[..., 2]
    corner = (own >= 0) & (hh[..., 2] > 1e-9) & (u > 64) & (v > 48)
    edge = (own >= 0) & (hh[..., 2] > 1e-9) & (u < -1) & (v < -1)
    assert corner.sum() + edge.sum() > 5
    assert (got[corner] == frame[47, 63]).all() and (got[edge] == frame[0, 0]).all()


def _check_known_answer(case, atlas, faces, params):
    """every texel of `faces` whose centre lies inside its UV triangle equals the texture at its 3-D point
    within 2 levels: 0.5 frame rounding + 0.5 output rounding + 0.125 bilinear (second derivative <= 0.5 per
    axis: 2 x 0.5 / 8) + 0.02 weight quantisation (gradient 4 x 1/512 per axis, twice), rounded up"""
    T, page = params.texel, params.page
    nf = len(case["F"])
    checked = 0
    for pg, own, inside, pts in zip(atlas, R.owners(nf, T, page), R.interior(nf, T, page), R.texel_points(case["V"], case["F"], T, page)):
        m = inside & np.isin(own, faces)
        want = case["texture"](pts[m][:, 0], pts[m][:, 1])
        err = np.abs(pg[m].astype(np.float64) - want)
        assert err.max() <= 2.0, err.max()
        checked += int(m.sum())
    return checked


@pytest.fixture(scope="module")
def plane():
    case = R.plane_case()
    prm = surface.TextureParams(texel=12, page=128, min_pixels=4)
    case["params"] = prm
    case["ids"] = R.render_ids(case["V"], case["C"], case["F"], case["K"], case["rotations"], case["positions"], [0, 1, 2], case["size"])
    case["want"] = R.texture(case["V"], case["C"], case["F"], case["frames"], case["K"], case["rotations"], case["positions"], prm,
                             ids=case["ids"])
    return case


def test_known_answer_plane(plane):
    uv, fp, atlas, bv, bc = plane["want"]
    nf = len(plane["F"])
    assert nf == 48 and (bc >= 4).all() and (bv >= 0).all()            # every face is textured
    assert len(set(bv.tolist())) >= 2                                   # and not all from one view
    n = _check_known_answer(plane, atlas, np.arange(nf), plane["params"])
    assert n >= nf * 12 * 11 // 2


@pytest.fixture(scope="module")
def occlusion():
    case = R.occlusion_case()
    prm = surface.TextureParams(texel=6, page=128, min_pixels=2)
    case["params"] = prm
    case["want"] = R.texture(case["V"], case["C"], case["F"], case["frames"], case["K"], case["rotations"], case["positions"], prm,
                             ids=case["ids"])
    return case


def test_known_answer_occlusion(occlusion):
    uv, fp, atlas, bv, bc = occlusion["want"]
    hidden, nwall = occlusion["hidden"], occlusion["nwall"]
    assert len(hidden) >= 4 and (bv[hidden] == 1).all() and (bc[hidden] >= 2).all()
    assert _check_known_answer(occlusion, atlas, hidden, occlusion["params"]) >= len(hidden) * 10
    cnt = R.count(occlusion["ids"], len(occlusion["F"]))
    both = np.flatnonzero((cnt[0] > 0) & (cnt[1] > 0))
    assert len(both) > 10
    assert (bv[both] == np.where(cnt[1, both] > cnt[0, both], 1, 0)).all() and (bc[both] == cnt[:, both].max(0)).all()
    # the quad itself is textured with its own constant colour
    own = R.owners(len(occlusion["F"]), 6, 128)
    inside = R.interior(len(occlusion["F"]), 6, 128)
    for f in (nwall, nwall + 1):
        m = inside[fp[f]] & (own[fp[f]] == f)
        assert m.any() and (atlas[fp[f]][m] == R.OCCLUDER).all(-1).mean() > 0.5      # but for its silhouette's pixels


def test_whole_pipeline_on_the_host(plane, occlusion):
    for case in (plane, occlusion):
        ids = case["ids"]
        got = surface.texture(case["V"], case["C"], case["F"], case["frames"], case["K"], case["rotations"], case["positions"],
                              case["params"], host=True, ids=ids if case is plane else (lambda a, b: ids[a:b]), chunk=2)
        uv, fp, atlas, bv, bc = case["want"]
        assert R.same_bits(got.uv, uv) and R.same_bits(got.page, fp) and R.same_bits(got.best_view, bv)
        assert R.same_bits(got.best_count, bc) and len(got.atlas) == len(atlas)
        assert all(R.same_bits(a, b) for a, b in zip(got.atlas, atlas))
        assert got.textured.all() or case is occlusion
    # without ids the host path refuses: the library has no host rasteriser
    with pytest.raises(ValueError):
        surface.texture(plane["V"], plane["C"], plane["F"], plane["frames"], plane["K"], plane["rotations"], plane["positions"],
                        plane["params"], host=True)
    empty = surface.texture(np.zeros((0, 3)), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32), plane["frames"], plane["K"],
                            plane["rotations"], plane["positions"], plane["params"], host=True, ids=np.zeros((3, 48, 64), np.int32))
    assert empty.atlas == [] and empty.uv.shape == (0, 3, 2)


def test_view_camera_and_params():
    K = np.array([[50.0, 0, 31.5], [0, 40.0, 23.5], [0, 0, 1.0]])
    V = np.array([[0, 0, 2.0], [1, 0, 8.0], [0, 1, -3.0], [np.nan, 0, 50.0]])
    Rz = np.array([[0.0, -1.0, 0], [1.0, 0, 0], [0, 0, 1.0]])
    (Rc, tc), cam = surface.view_camera(K, Rz, [1.0, 2.0, 0.0], V, (64, 48))
    assert np.array_equal(Rc, Rz.T) and np.array_equal(tc, -(Rz.T @ np.array([1.0, 2.0, 0.0])))
    assert cam == (50.0, 40.0, 32.0, 24.0, 1.0, 16.0)                   # z in {2, 8}: far = 16, near = max(1, 16 / 16384)
    assert surface.view_camera(K, np.eye(3), np.zeros(3), -V[:1], (64, 48))[1][4:] == (0.01, 1000.01)
    skew = K.copy()
    skew[0, 1] = 0.1
    with pytest.raises(ValueError):
        surface.view_camera(skew, np.eye(3), np.zeros(3), V, (64, 48))
    assert surface.texture_views(5) == [0, 1, 2, 3, 4] and surface.texture_views(5, 9) == [0, 1, 2, 3, 4]
    assert surface.texture_views(10, 3) == [1, 5, 8] and surface.texture_views(7, 1) == [3]
    p = surface.TextureParams()
    assert (p.texel, p.page, p.min_pixels, p.max_views) == (12, 4096, 4, None)
    for bad in (dict(texel=0), dict(texel=65), dict(page=15), dict(page=8193), dict(min_pixels=0), dict(max_views=0)):
        with pytest.raises(ValueError):
            surface.TextureParams(**bad)
    assert surface.SurfaceParams().texture is None and surface.SurfaceParams(texture=p).texture is p
    with pytest.raises(ValueError):
        surface.SurfaceParams(texture=12)


# ---- files -------------------------------------------------------------------------------------------

def test_textured_mesh_round_trip(tmp_path, contract_fill):
    case = FILL[1]
    V, F = case[1], case[3]
    atlas = contract_fill["three-pages"]
    _, _, uv, fp = R.layout(len(F), 4, 64)
    path = str(tmp_path / "surface.obj")
    files = scene.write_textured_mesh(path, V, F, uv, fp, atlas)
    assert [os.path.basename(f) for f in files] == ["surface.obj", "surface.mtl", "surface_atlas_0.png", "surface_atlas_1.png",
                                                    "surface_atlas_2.png"]
    assert all(os.path.exists(f) for f in files)
    lv, lf, luv, lp, la = scene.load_textured_mesh(path)
    assert np.array_equal(lv, V.astype(np.float32).astype(np.float64)) and R.same_bits(lf, F)
    assert R.same_bits(luv, uv) and R.same_bits(lp, fp)                 # repr floats: exact
    assert len(la) == 3 and all(R.same_bits(a, b) for a, b in zip(la, atlas))
    ppm = str(tmp_path / "p" / "m.obj")
    os.makedirs(os.path.dirname(ppm))
    scene.write_textured_mesh(ppm, V, F, uv, fp, atlas, atlas_ext=".ppm")
    assert all(R.same_bits(a, b) for a, b in zip(scene.load_textured_mesh(ppm)[4], atlas))
    scene.write_textured_mesh(path, np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros((0, 3, 2)), np.zeros(0, np.int32), [])
    lv, lf, luv, lp, la = scene.load_textured_mesh(path)
    assert lv.shape == (0, 3) and lf.shape == (0, 3) and luv.shape == (0, 3, 2) and la == []
    with pytest.raises(ValueError):
        scene.write_textured_mesh(path, V, F, uv[:-1], fp, atlas)
    with pytest.raises(ValueError):
        scene.write_textured_mesh(path, V, F, uv, fp, atlas[:2])


# ---- argument errors ---------------------------------------------------------------------------------

def test_argument_errors():
    name, V, C, F, frames, fidx, P, bc, bv, mp, T, page = FILL[0]

    def fill(**kw):
        a = dict(V=V, C=C, F=F, frames=frames, P=P, bc=bc, bv=bv, mp=mp, T=T, page=page, fidx=fidx)
        a.update(kw)
        return slamhip.texFill(a["V"], a["C"], a["F"], a["frames"], a["P"], a["bc"], a["bv"], a["mp"], a["T"], a["page"],
                               frame_idx=a["fidx"], host=True)

    fill()
    badF, negF = F.copy(), F.copy()
    badF[3, 1] = len(V)
    negF[0, 0] = -1
    bigv, lowv = bv.copy(), bv.copy()
    bigv[2] = 3
    lowv[2] = -2
    for kw in (dict(T=0), dict(T=65), dict(page=T + 3), dict(page=8193), dict(mp=0), dict(mp=(1 << 30) + 1), dict(F=badF),
               dict(F=negF), dict(bv=bigv), dict(bv=lowv), dict(fidx=[0, 1, 3]), dict(fidx=[-1, 0, 1])):
        with pytest.raises(L.SlamError) as e:
            fill(**kw)
        assert e.value.code == L.SLAM_E_INVALID_ARG, kw
    lib = slamhip.lib()
    n1, n2 = ctypes.c_int(0), ctypes.c_int(0)
    one = np.zeros(8, np.int32)
    # null pointers with non-zero counts; more than 2^30 faces; the checks come before any access
    assert lib.slam_tex_fill_host(None, L.ptr(C), L.ptr(F), len(V), 7, None, 0, 4, 4, 3, None, None, 0, L.ptr(bc), L.ptr(bv), 4, 5,
                                  64, L.ptr(np.zeros(64 * 64 * 3, np.uint8))) == L.SLAM_E_INVALID_ARG
    assert lib.slam_tex_fill_host(L.ptr(V), L.ptr(C), L.ptr(F), len(V), 7, None, 0, 4, 4, 3, None, None, 0, L.ptr(bc), L.ptr(bv), 4,
                                  5, 64, None) == L.SLAM_E_INVALID_ARG
    assert lib.slam_tex_fill_host(L.ptr(V), L.ptr(C), L.ptr(F), len(V), 7, None, 1, 4, 4, 3, None, L.ptr(np.stack(P)), 1,
                                  L.ptr(bc), L.ptr(bv), 4, 5, 64, L.ptr(one)) == L.SLAM_E_INVALID_ARG
    assert lib.slam_tex_fill_host(None, None, None, 0, (1 << 30) + 1, None, 0, 4, 4, 3, None, None, 0, None, None, 4, 5, 64,
                                  None) == L.SLAM_E_UNSUPPORTED
    assert lib.slam_tex_fill_host(None, None, None, 0, 0, None, 0, 4, 4, 3, None, None, 0, None, None, 4, 5, 64, None) == L.SLAM_OK
    assert lib.slam_tex_select_host(None, 1, 4, 4, 0, 8, L.ptr(one), L.ptr(one)) == L.SLAM_E_INVALID_ARG
    assert lib.slam_tex_select_host(L.ptr(one), 1, 2, 4, 0, 8, None, L.ptr(one)) == L.SLAM_E_INVALID_ARG
    assert lib.slam_tex_select_host(L.ptr(one), 1, 2, 4, -1, 8, L.ptr(one), L.ptr(one)) == L.SLAM_E_INVALID_ARG
    assert lib.slam_tex_select_host(L.ptr(one), 1, 0, 4, 0, 8, L.ptr(one), L.ptr(one)) == L.SLAM_E_INVALID_ARG
    assert lib.slam_tex_select_host(L.ptr(one), 1, 2, 4, 0, (1 << 30) + 1, L.ptr(one), L.ptr(one)) == L.SLAM_E_UNSUPPORTED
    assert lib.slam_tex_select_host(None, 0, 2, 4, 0, 0, None, None) == L.SLAM_OK
    for args, rc in (((3, 0, 64), L.SLAM_E_INVALID_ARG), ((3, 65, 8192), L.SLAM_E_INVALID_ARG), ((3, 5, 8), L.SLAM_E_INVALID_ARG),
                     ((3, 5, 8193), L.SLAM_E_INVALID_ARG), ((-1, 5, 64), L.SLAM_E_INVALID_ARG),
                     (((1 << 30) + 1, 5, 64), L.SLAM_E_UNSUPPORTED), ((0, 5, 64), L.SLAM_OK)):
        assert lib.slam_tex_layout(*args, ctypes.byref(n1), ctypes.byref(n2), None, 0, None, None) == rc, args
    assert (n1.value, n2.value) == (0, 63)
    ph = np.zeros(2, np.int32)
    assert lib.slam_tex_layout(300, 4, 64, ctypes.byref(n1), ctypes.byref(n2), L.ptr(ph), 2, None, None) == L.SLAM_E_CAPACITY
    assert n1.value == 3 and (ph == 0).all()


# ---- the host twins under ASan + UBSan, as a stand-alone program ---------------------------------------

def _dump(path, arrays):
    """the vectors of tests/cpp/tex_host_test.cpp: per array a line `name dtype count` and its raw bytes"""
    with open(path, "wb") as f:
        for name, a in arrays:
            a = np.ascontiguousarray(a)
            f.write(f"{name} {a.dtype.name} {a.size}\n".encode())
            f.write(a.tobytes())


def test_host_twins_under_sanitizers(tmp_path, contract_fill):
    vec = str(tmp_path / "tex_vectors.bin")
    arrays = [("ncases", np.array([len(FILL), len(SELECT)], np.int32))]
    for name, V, C, F, frames, fidx, P, bc, bv, mp, T, page in FILL:
        fr = np.stack(frames)
        arrays += [("dims", np.array([len(V), len(F), fr.shape[0], fr.shape[1], fr.shape[2], 1 if fr.ndim == 3 else 3, len(P), mp, T,
                                      page], np.int32)),
                   ("V", V.astype(np.float64)), ("C", C), ("F", F), ("frames", fr), ("fidx", np.array(fidx, np.int32)),
                   ("P", np.stack(P).astype(np.float64)), ("bc", bc), ("bv", bv),
                   ("atlas", np.concatenate([p.ravel() for p in contract_fill[name]]))]
    for name, ids, nf in SELECT:
        bc, bv = R.select(R.empty_state(nf), ids, 5, nf)
        arrays += [("sdims", np.array([ids.shape[0], ids.shape[1], ids.shape[2], 5, nf], np.int32)), ("ids", ids), ("bc", bc),
                   ("bv", bv)]
    _dump(vec, arrays)
    exe = str(tmp_path / "tex_host_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread",
           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-static-libasan",
           os.path.join(ROOT, "tests", "cpp", "tex_host_test.cpp"), os.path.join(CSRC, "tex_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe, vec], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines()[-1].startswith("OK: ")

"""The reference's scene post-processing, up to the mesh of every plane
segment: what runs after slamMain, or after an onlyViz reload of the result
files (src/main.cpp:55-71).

  load_global_data   getGlobalDataFromLogFiles        src/misc/IOmisc.cpp:133-177
  segment            vizualizePointsAndCameras:72-104 src/vizualization/vizualizationModule.cpp
                     (clusterizePoints, getBestFittingPlaneByPoints, the
                     TriangleMinimumPoints filter and makeMesh's projection,
                     bestFittingPlane.cpp:51-63)
  make_mesh / mesh   makeMesh:67-114 (builtInTriangulation, bowyerWatson.cpp:86-105,
                     the corner lookup and the max_size filter) and the
                     try / catch around it, vizualizePointsAndCameras:105-115
  write_mesh         the cloud and every face as an ASCII PLY, in place of the
                     cv::viz::WMesh widgets
  trajectory_lines   viz::WTrajectory(path, BOTH, 0.1, green), vizualizeCameras:50-54
  reference_view     the viewer pose of vizualizeCameras:56-57
  fly                rotationMatrixToEulerAngles + KeyboardViz3d, :149-250
  render             the window's picture: cloud, trajectory and meshes through
                     api.renderViews, seen with viz::Camera(Vec2d(1, 1), Size(1000, 1000))
  write_ppm / write_png   the frames on disk
  write_textured_mesh / load_textured_mesh   the textured surface (surface.texture, DESIGN.md
                     section 29) as Wavefront OBJ + MTL + one image per atlas page
  main               the onlyViz branch of main()

The numeric steps are slamhip.api's clusterizePoints / getBestFittingPlaneByPoints
/ projectToPlane / delaunay2d (HIP kernels behind the C ABI), delaunay2dHost for
components of a few dozen points, meshFilter, and renderViews (a z-buffer
rasteriser in HIP: the cv::viz window is VTK over OpenGL and cannot run on a
headless server, so the picture is the project's own, defined by
tests/render_ref.py; the window itself and its event loop are not built).
"""
import math
import os
import struct
import sys
import zlib
from collections import namedtuple

import numpy as np

from . import api
from .config import INTEGER, ConfigService
from .cycle import GlobalData

# one kept component: indices into the cloud (ascending), its Point3f points,
# Vec3b colours and the projected Point2f (x, z) coordinates makeMesh triangulates
Segment = namedtuple("Segment", "indices points colors xy")
# one component's mesh: triangles (T, 3) index the segment, faces = the same
# rows as indices into the cloud; both after makeMesh's max_size filter
Mesh = namedtuple("Mesh", "triangles faces")

SUBDIV_RANGE = 100000.0      # builtInTriangulation's Subdiv2D rectangle: x, y in [-SUBDIV_RANGE, SUBDIV_RANGE)


def _numbers(path):
    with open(path) as f:
        return np.array(f.read().split(), np.float64)


def _rows(path, width):
    v = _numbers(path)
    # operator>> stops at the last complete record; a trailing partial one is dropped at eof
    return v[:len(v) // width * width].reshape(-1, width)


def load_global_data(out_dir, cloud="sparse"):
    """IOmisc.cpp:133-177: GlobalData from points.txt, colors.txt, poses.txt and
    rotations.txt of `out_dir` as cycle.Logs writes them (rawOutput rows).
    Colours are cast with (uchar), i.e. truncated.  Raises ValueError where the
    reference throws: rotation / pose counts or point / colour counts differ.
    cloud="dense" reads dense_points.txt / dense_colors.txt (slam_main(dense=...))
    in place of the sparse cloud's files; cloud="closed" reads the four *_closed.txt
    files of slam_main(loops=LoopParams(close=True)): corrected cameras and the
    merged cloud; cloud="refined" reads the four *_refined.txt files that
    global_ba=True adds: the closed map after global bundle adjustment."""
    if cloud not in ("sparse", "dense", "closed", "refined"):
        raise ValueError('cloud: "sparse" or "dense" (or "closed", "refined")')
    prefix = "dense_" if cloud == "dense" else ""
    suffix = "_" + cloud if cloud in ("closed", "refined") else ""
    poses = _rows(os.path.join(out_dir, "poses" + suffix + ".txt"), 3)
    rotations = _rows(os.path.join(out_dir, "rotations" + suffix + ".txt"), 9)
    if len(rotations) != len(poses):
        raise ValueError("Count of rotations and translations must be equal: "
                         f"{len(rotations)} rotations, {len(poses)} translations")
    points = _rows(os.path.join(out_dir, prefix + "points" + suffix + ".txt"), 3)
    colors = _rows(os.path.join(out_dir, prefix + "colors" + suffix + ".txt"), 3)
    if len(points) != len(colors):
        raise ValueError("Count of points and their colors must be equal: "
                         f"{len(points)} points, {len(colors)} colors")
    gd = GlobalData()
    gd.spatialCameraPositions = [p.reshape(3, 1).copy() for p in poses]
    gd.cameraRotations = [r.reshape(3, 3).copy() for r in rotations]
    gd.push_points(points, colors.astype(np.int64).astype(np.uint8))
    return gd


def segment(global_data, config, ctx=None):
    """vizualizePointsAndCameras:72-104 without the window: narrow the points
    to Point3f (main.cpp:61-64), cluster them, fit the plane on ALL points,
    drop components with fewer than TriangleMinimumPoints members and project
    each kept component onto the plane.  Returns a list of Segment in the
    reference's component order (by smallest member)."""
    pts = np.ascontiguousarray(global_data.spatialPoints, np.float64).astype(np.float32).reshape(-1, 3)
    cols = np.ascontiguousarray(global_data.spatialPointsColors, np.uint8).reshape(-1, 3)
    comps = api.clusterizePoints(pts, cols, config, ctx=ctx)
    if len(pts) == 0:
        return []
    centroid, normal = api.getBestFittingPlaneByPoints(pts, ctx=ctx)
    min_points = int(config.getValue("TriangleMinimumPoints", INTEGER))
    out = []
    for comp in comps:
        if len(comp) < min_points:
            continue
        idx = np.asarray(comp, np.int32)
        p = pts[idx]
        out.append(Segment(idx, p, cols[idx], api.projectToPlane(p, centroid, normal, ctx=ctx)))
    return out


def write_clusters(segments, path):
    """one line of point indices per kept component"""
    with open(path, "w") as f:
        for s in segments:
            f.write(" ".join(str(int(i)) for i in s.indices) + "\n")


def make_mesh(segment, ctx=None):
    """makeMesh:67-114 for one Segment: triangulate its projected points
    (api.delaunay2d on the device; below api.DELAUNAY_HOST_BELOW points
    api.delaunay2dHost, the same contract on the host, where a launch would
    cost more than the work), then drop every triangle with a 3-D edge longer
    than 10000 (api.meshFilter).  Returns a Mesh, or None where the reference's Subdiv2D
    throws and vizualizePointsAndCameras:105-115 catches, so that the component
    gets no mesh: a projected coordinate that is not finite or outside
    [-100000, 100000).  Fewer than 3 points: an empty Mesh, no launch."""
    xy = np.ascontiguousarray(segment.xy, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        if not bool(((xy >= -SUBDIV_RANGE) & (xy < SUBDIV_RANGE)).all()):      # NaN and inf fail both
            return None
    idx = np.asarray(segment.indices, np.int32)
    if len(xy) < 3:
        tris = np.zeros((0, 3), np.int32)
    elif len(xy) < api.DELAUNAY_HOST_BELOW:
        tris = api.meshFilter(segment.points, api.delaunay2dHost(xy))
    else:
        tris = api.meshFilter(segment.points, api.delaunay2d(xy, ctx=ctx))
    return Mesh(tris, idx[tris].astype(np.int32).reshape(-1, 3))


def mesh(segments, ctx=None):
    """make_mesh of every segment, in order (None for a skipped component)"""
    return [make_mesh(s, ctx=ctx) for s in segments]


def write_mesh(global_points, colors, meshes, path):
    """the cloud (n x 3, written as float32: the Point3f the mesh was built on),
    its colours (n x 3 Vec3b, stored blue-green-red as OpenCV does; the file
    names them red green blue) and the faces of every Mesh as an ASCII PLY, the
    format the reference's python_utility viewer library loads."""
    pts = np.ascontiguousarray(global_points, np.float64).astype(np.float32).reshape(-1, 3)
    cols = np.ascontiguousarray(colors, np.uint8).reshape(-1, 3)
    if len(pts) != len(cols):
        raise ValueError("points and colors differ in length")
    faces = [m.faces for m in meshes if m is not None and len(m.faces)]
    faces = np.concatenate(faces) if faces else np.zeros((0, 3), np.int32)
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment slamhip scene mesh\n")
        f.write(f"element vertex {len(pts)}\nproperty float x\nproperty float y\nproperty float z\n")
        f.write("property uchar red\nproperty uchar green\nproperty uchar blue\n")
        f.write(f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
        for p, c in zip(pts, cols):
            f.write(f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {int(c[2])} {int(c[1])} {int(c[0])}\n")
        for t in faces:
            f.write(f"3 {int(t[0])} {int(t[1])} {int(t[2])}\n")


def load_surface(path):
    """write_mesh's own ASCII PLY back: (vertices (n, 3) float64 holding the float32 values of the file,
    colors (n, 3) uint8 blue-green-red, faces (m, 3) int32).  slam_main(surface=...) writes surface.ply
    in this form.  Anything but write_mesh's header raises ValueError."""
    with open(path) as f:
        lines = f.read().split("\n")
    try:
        end = lines.index("end_header")
    except ValueError:
        raise ValueError(f"{path}: no PLY header")
    head = lines[:end]
    if head[:2] != ["ply", "format ascii 1.0"]:
        raise ValueError(f"{path}: not an ASCII PLY")
    counts = {h.split()[1]: int(h.split()[2]) for h in head if h.startswith("element ")}
    props = [h for h in head if h.startswith("property ")]
    if sorted(counts) != ["face", "vertex"] or props != [
            "property float x", "property float y", "property float z", "property uchar red", "property uchar green",
            "property uchar blue", "property list uchar int vertex_indices"]:
        raise ValueError(f"{path}: not a mesh written by write_mesh")
    nv, nf = counts["vertex"], counts["face"]
    body = lines[end + 1:]
    if len(body) < nv + nf:
        raise ValueError(f"{path}: truncated")
    vt = np.array([r.split() for r in body[:nv]], np.float64).reshape(nv, 6)
    fc = np.array([r.split() for r in body[nv:nv + nf]], np.int64).reshape(nf, 4)
    if nf and not (fc[:, 0] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    return (np.ascontiguousarray(vt[:, :3]), np.ascontiguousarray(vt[:, 5:2:-1]).astype(np.uint8),
            np.ascontiguousarray(fc[:, 1:]).astype(np.int32))


GREEN, RED, BLUE = (0, 255, 0), (0, 0, 255), (255, 0, 0)     # viz::Color, blue-green-red
# Point3f centroid(-0.368855, 0.538447, 7.92543), vizualizeCameras:56: narrowed to float, then an Affine3d
REFERENCE_VIEWER_POSITION = np.array([-0.368855, 0.538447, 7.92543], np.float32).astype(np.float64)
SPEED_MIN, SPEED_MAX, SPEED_STEP = 0.25, 2.5, 0.25


def trajectory_lines(rotations, positions, scale=0.1, color=GREEN):
    """viz::WTrajectory(path, WTrajectory::BOTH, scale, color) of the poses
    Affine3d(rotations[i], positions[i]) as (lines (k, 6) float32, colours (k, 3)
    uint8 BGR): first the polyline between consecutive positions in `color`,
    then per pose its three axes of length `scale` from the position along the
    columns of the rotation, x red, y green, z blue."""
    R = [np.asarray(r, np.float64).reshape(3, 3) for r in rotations]
    t = [np.asarray(p, np.float64).reshape(3) for p in positions]
    if len(R) != len(t):
        raise ValueError("Count of rotations and translations must be equal")
    lines, cols = [], []
    for a, b in zip(t[:-1], t[1:]):
        lines.append(np.concatenate([a, b]))
        cols.append(color)
    for r, p in zip(R, t):
        for axis, c in enumerate((RED, GREEN, BLUE)):
            lines.append(np.concatenate([p, p + r[:, axis] * scale]))
            cols.append(c)
    return (np.array(lines, np.float64).astype(np.float32).reshape(-1, 6), np.array(cols, np.uint8).reshape(-1, 3))


def reference_view(global_data):
    """window.setViewerPose(Affine3d(rotations[0], Mat(centroid))), vizualizeCameras:56-57"""
    if not global_data.cameraRotations:
        raise ValueError("reference_view needs at least one camera rotation")
    return (np.asarray(global_data.cameraRotations[0], np.float64).reshape(3, 3).copy(), REFERENCE_VIEWER_POSITION.copy())


def rotation_to_euler(R):
    """rotationMatrixToEulerAngles:149-185: (bank, attitude, heading), narrowed to
    float as its Vec3f result is"""
    m = np.asarray(R, np.float64).reshape(3, 3)
    if m[1, 0] > 0.998:
        e = (0.0, math.pi / 2, math.atan2(m[0, 2], m[2, 2]))
    elif m[1, 0] < -0.998:
        e = (0.0, -math.pi / 2, math.atan2(m[0, 2], m[2, 2]))
    else:
        e = (math.atan2(-m[1, 2], m[1, 1]), math.asin(m[1, 0]), math.atan2(-m[2, 0], m[0, 0]))
    return tuple(float(np.float32(v)) for v in e)


def fly(view, keys, speed=0.5):
    """KeyboardViz3d:187-250 for each character of `keys`, starting from view
    (R, t) and the reference's global `speed`: w / s move along the heading, a / d
    along the heading -/+ 3.14 / 2.0 (the reference's constant, not pi / 2), c and
    space move y by +/- speed * speed, + (or =, the key code 61 the reference
    tests) and - change the speed by 0.25 within 0.25 .. 2.5.  The translation is
    added to the pose's (Affine3d::translate); the rotation never changes.
    Returns the list of views after each key stroke."""
    R = np.asarray(view[0], np.float64).reshape(3, 3).copy()
    t = np.asarray(view[1], np.float64).reshape(3).copy()
    out = []
    for key in keys:
        heading = rotation_to_euler(R)[2]
        d = np.zeros(3)
        if key == "w":
            d[2], d[0] = math.cos(heading) * speed, math.sin(heading) * speed
        elif key == "s":
            d[2], d[0] = -math.cos(heading) * speed, -math.sin(heading) * speed
        elif key == "a":
            d[2], d[0] = math.cos(heading - 3.14 / 2.0) * speed, math.sin(heading - 3.14 / 2.0) * speed
        elif key == "d":
            d[2], d[0] = math.cos(heading + 3.14 / 2.0) * speed, math.sin(heading + 3.14 / 2.0) * speed
        elif key == "c":
            d[1] = speed * speed
        elif key == " ":
            d[1] = -speed * speed
        elif key in "+=":
            if speed < SPEED_MAX:
                speed += SPEED_STEP
        elif key == "-":
            if speed > SPEED_MIN:
                speed -= SPEED_STEP
        else:
            raise ValueError(f"fly: unknown key {key!r} (w s a d c space + -)")
        t = t + d
        out.append((R.copy(), t.copy()))
    return out


def scene_primitives(global_data, meshes):
    """what the window shows: (points float32, colours, faces, lines, line colours).
    If the colour count differs from the point count the cloud is green
    (getPointCloudFromPoints:28-33)."""
    pts = np.ascontiguousarray(global_data.spatialPoints, np.float64).astype(np.float32).reshape(-1, 3)
    cols = np.ascontiguousarray(global_data.spatialPointsColors, np.uint8).reshape(-1, 3)
    if len(cols) != len(pts):
        cols = np.tile(np.array(GREEN, np.uint8), (len(pts), 1))
    faces = [m.faces for m in meshes if m is not None and len(m.faces)]
    faces = np.concatenate(faces).astype(np.int32) if faces else np.zeros((0, 3), np.int32)
    lines, line_cols = trajectory_lines(global_data.cameraRotations, global_data.spatialCameraPositions)
    return pts, cols, faces, lines, line_cols


def render(global_data, meshes, views=None, camera=None, size=(1000, 1000), point_size=1, ids=False, depth=False,
           ctx=None):
    """The picture of vizualizePointsAndCameras' window from each of `views`
    (default: the reference view): api.renderViews of scene_primitives."""
    if views is None:
        views = [reference_view(global_data)]
    return api.renderViews(*scene_primitives(global_data, meshes), views, camera=camera, size=size,
                           point_size=point_size, ids=ids, depth=depth, ctx=ctx)


render_scene = render      # main's `render` argument hides the function there


def _rgb(frame):
    a = np.asarray(frame)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("a frame is (h, w, 3) uint8, blue-green-red")
    return np.ascontiguousarray(a[:, :, ::-1])


def write_ppm(path, frame):
    """a BGR frame as a binary PPM (P6, red-green-blue)"""
    rgb = _rgb(frame)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())


def write_png(path, frame):
    """a BGR frame as an 8-bit RGB PNG: one zlib stream, filter 0 on every row"""
    rgb = _rgb(frame)
    h, w = rgb.shape[:2]

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    rows = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, w * 3)], axis=1)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        f.write(chunk(b"IEND", b""))


def write_image(path, frame, ctx=None):
    """a BGR frame by its name: .jpg / .jpeg through api.imwrite (the device encoder,
    quality 95, 4:2:0), .ppm as a PPM, anything else as a PNG"""
    name = path.lower()
    if name.endswith((".jpg", ".jpeg")):
        if not api.imwrite(path, np.ascontiguousarray(frame), ctx=ctx):
            raise OSError(f"cannot write {path}")
    else:
        (write_ppm if name.endswith(".ppm") else write_png)(path, frame)


def read_image(path, ctx=None):
    """write_image's own files back as (h, w, 3) uint8 blue-green-red: a PNG as write_png writes it
    (8-bit RGB, filter 0 on every row), a binary PPM, or a JPEG through api.imread"""
    name = path.lower()
    if name.endswith((".jpg", ".jpeg")):
        return np.asarray(api.imread(path, ctx=ctx))
    with open(path, "rb") as f:
        data = f.read()
    if name.endswith(".ppm"):
        head = data.split(b"\n", 3)
        if len(head) != 4 or head[0] != b"P6" or head[2] != b"255":
            raise ValueError(f"{path}: not a PPM written by write_ppm")
        w, h = (int(v) for v in head[1].split())
        return np.ascontiguousarray(np.frombuffer(head[3], np.uint8, h * w * 3).reshape(h, w, 3)[:, :, ::-1])
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG")
    o, idat, w, h = 8, b"", 0, 0
    while o + 8 <= len(data):
        n, kind = struct.unpack(">I", data[o:o + 4])[0], data[o + 4:o + 8]
        body = data[o + 8:o + 8 + n]
        if kind == b"IHDR":
            w, h, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", body)
            if (depth, colour, interlace) != (8, 2, 0):
                raise ValueError(f"{path}: not a PNG written by write_png")
        elif kind == b"IDAT":
            idat += body
        o += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    if rows[:, 0].any():
        raise ValueError(f"{path}: a filtered row; not a PNG written by write_png")
    return np.ascontiguousarray(rows[:, 1:].reshape(h, w, 3)[:, :, ::-1])


def write_textured_mesh(path, vertices, faces, uv, page, atlases, atlas_ext=".png", ctx=None):
    """A textured mesh as Wavefront OBJ + MTL + one image per atlas page: `path` (x.obj), x.mtl and
    x_atlas_<p><atlas_ext> beside it, the images through write_image.  vertices (n, 3) are written as
    float32 (as write_mesh does), uv (nf, 3, 2) as exact `repr` floats, three `vt` per face in face
    order; faces (nf, 3) index the vertices, page (nf,) names each face's atlas page (material
    page_<p>).  PNG is the default: a 4:2:0 JPEG would bleed chroma across the atlas cells.
    Returns the files written."""
    pts = np.ascontiguousarray(vertices, np.float64).astype(np.float32).reshape(-1, 3)
    fcs = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 3, 2)
    page = np.ascontiguousarray(page, np.int32).reshape(-1)
    if len(uv) != len(fcs) or len(page) != len(fcs):
        raise ValueError("one uv triple and one page per face")
    if len(fcs) and (page.min() < 0 or page.max() >= len(atlases)):
        raise ValueError("a face on a page without an atlas")
    if not atlas_ext.startswith(".") or any(c.isspace() for c in os.path.basename(path)):
        raise ValueError("atlas_ext starts with a dot; the file name holds no white space")
    stem = os.path.splitext(path)[0]
    base = os.path.basename(stem)
    files = [path, stem + ".mtl"]
    with open(path, "w") as f:
        f.write(f"# slamhip textured mesh\nmtllib {base}.mtl\n")
        for p in pts:
            f.write(f"v {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n")
        for t in uv.reshape(-1, 2):
            f.write(f"vt {float(t[0])!r} {float(t[1])!r}\n")
        current = -1
        for i, t in enumerate(fcs):
            if page[i] != current:
                current = int(page[i])
                f.write(f"usemtl page_{current}\n")
            f.write(f"f {int(t[0]) + 1}/{3 * i + 1} {int(t[1]) + 1}/{3 * i + 2} {int(t[2]) + 1}/{3 * i + 3}\n")
    with open(stem + ".mtl", "w") as f:
        f.write("# slamhip textured mesh\n")
        for p in range(len(atlases)):
            f.write(f"newmtl page_{p}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd {base}_atlas_{p}{atlas_ext}\n")
    for p, a in enumerate(atlases):
        files.append(f"{stem}_atlas_{p}{atlas_ext}")
        write_image(files[-1], a, ctx=ctx)
    return files


def load_textured_mesh(path, ctx=None):
    """write_textured_mesh's own files back: (vertices (n, 3) float64 holding the float32 values of
    the file, faces (m, 3) int32, uv (m, 3, 2) float64, page (m,) int32, atlases: a list of (h, w, 3)
    uint8 blue-green-red).  Anything but write_textured_mesh's form raises ValueError."""
    with open(path) as f:
        lines = f.read().split("\n")
    v, vt, fc, pg, mtl, current = [], [], [], [], None, -1
    for ln in lines:
        k = ln.split()
        if not k or k[0] == "#":
            continue
        if k[0] == "mtllib" and len(k) == 2:
            mtl = k[1]
        elif k[0] == "v" and len(k) == 4:
            v.append([float(x) for x in k[1:]])
        elif k[0] == "vt" and len(k) == 3:
            vt.append([float(x) for x in k[1:]])
        elif k[0] == "usemtl" and len(k) == 2 and k[1].startswith("page_"):
            current = int(k[1][5:])
        elif k[0] == "f" and len(k) == 4:
            c = [x.split("/") for x in k[1:]]
            if any(len(x) != 2 for x in c) or [int(x[1]) for x in c] != [3 * len(fc) + 1, 3 * len(fc) + 2, 3 * len(fc) + 3]:
                raise ValueError(f"{path}: not a mesh written by write_textured_mesh")
            fc.append([int(x[0]) - 1 for x in c])
            pg.append(current)
        else:
            raise ValueError(f"{path}: not a mesh written by write_textured_mesh")
    if mtl is None or len(vt) != 3 * len(fc) or (pg and min(pg) < 0):
        raise ValueError(f"{path}: not a mesh written by write_textured_mesh")
    maps = {}
    with open(os.path.join(os.path.dirname(path), mtl)) as f:
        name = None
        for ln in f.read().split("\n"):
            k = ln.split()
            if k[:1] == ["newmtl"] and len(k) == 2 and k[1].startswith("page_"):
                name = int(k[1][5:])
            elif k[:1] == ["map_Kd"] and len(k) == 2 and name is not None:
                maps[name] = k[1]
    if sorted(maps) != list(range(len(maps))) or (pg and max(pg) >= len(maps)):
        raise ValueError(f"{path}: its materials are not write_textured_mesh's")
    atlases = [read_image(os.path.join(os.path.dirname(path), maps[p]), ctx=ctx) for p in range(len(maps))]
    return (np.array(v, np.float64).reshape(-1, 3), np.array(fc, np.int32).reshape(-1, 3), np.array(vt, np.float64).reshape(-1, 3, 2),
            np.array(pg, np.int32).reshape(-1), atlases)



def write_video(path, global_data, meshes, views, fps=30.0, ctx=None, **render_args):
    """the views rendered with resident primitives and encoded from the resident frames into one
    Motion-JPEG AVI (video.VideoWriter); returns the bytes written"""
    import torch
    from . import video
    ctx = ctx or api.default_context()
    dev = torch.device("cuda", ctx.device)
    pts, cols, faces, lines, line_cols = scene_primitives(global_data, meshes)
    prim = [torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1, k)).to(dev)
            for a, dt, k in ((pts, np.float32, 3), (cols, np.uint8, 3), (faces, np.int32, 3), (lines, np.float32, 6),
                             (line_cols, np.uint8, 3))]
    frames = api.renderViews(*prim, views, ctx=ctx, **render_args)
    wr = video.VideoWriter(path, "MJPG", fps, (int(frames.shape[2]), int(frames.shape[1])), ctx=ctx)
    wr.write_batch(frames)
    return wr.release()


def main(config_path, render=None, cloud="sparse"):
    """the onlyViz branch of the reference's main(): reload outputDataDir's
    result files, segment the cloud and write clusters.txt and mesh.ply next to
    them.  render = "view.png" also writes the reference view there (a .ppm name
    gives a PPM, a .jpg name a JPEG from the device encoder); render =
    ("fly_%04d.png", "wwwwaadd") writes one frame per key stroke of scene.fly from the
    reference view, and render = ("fly.avi", keys) encodes those frames where they
    were rendered and writes one Motion-JPEG AVI.  The default writes nothing more.
    cloud="dense" works on the dense cloud of slam_main(dense=...) instead, cloud="closed"
    on the corrected cameras and merged cloud of slam_main(loops=LoopParams(close=True)),
    cloud="refined" on that map after global bundle adjustment (global_ba=True).
    cloud="surface" draws the surface of slam_main(surface=...): the cameras come from the
    sparse files, surface.ply's vertices are the cloud and its faces one Mesh; nothing is
    segmented and neither clusters.txt nor mesh.ply is written (returns no segments)."""
    cfg = ConfigService()
    cfg.setConfigFile(config_path)
    if not cfg.getValue("onlyViz"):
        raise ValueError("scene.main handles onlyViz = true; run cycle.slam_main first, then scene.segment")
    out_dir = cfg.getValue("outputDataDir")
    if cloud == "surface":
        gd = load_global_data(out_dir)
        verts, cols, faces = load_surface(os.path.join(out_dir, "surface.ply"))
        cams = gd
        gd = GlobalData()
        gd.spatialCameraPositions, gd.cameraRotations = cams.spatialCameraPositions, cams.cameraRotations
        gd.push_points(verts, cols)
        segments, meshes = [], [Mesh(faces, faces)]
    else:
        gd = load_global_data(out_dir, cloud)
        segments = segment(gd, cfg)
        write_clusters(segments, os.path.join(out_dir, "clusters.txt"))
        meshes = mesh(segments)
        write_mesh(gd.spatialPoints, gd.spatialPointsColors, meshes, os.path.join(out_dir, "mesh.ply"))
    if render is not None:
        draw = render_scene
        if isinstance(render, str):
            write_image(os.path.join(out_dir, render), draw(gd, meshes)[0])
        else:
            pattern, keys = render
            views = fly(reference_view(gd), keys)
            if views and pattern.lower().endswith(".avi"):
                write_video(os.path.join(out_dir, pattern), gd, meshes, views)
            elif views:
                for i, frame in enumerate(draw(gd, meshes, views=views)):
                    write_image(os.path.join(out_dir, pattern % i), frame)
    return segments


if __name__ == "__main__":
    main(sys.argv[1], *sys.argv[2:3])

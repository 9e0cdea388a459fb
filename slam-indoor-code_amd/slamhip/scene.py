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
  main               the onlyViz branch of main()

The numeric steps are slamhip.api's clusterizePoints / getBestFittingPlaneByPoints
/ projectToPlane / delaunay2d (HIP kernels behind the C ABI), delaunay2dHost for
components of a few dozen points, and meshFilter.
The cv::viz window is out of scope.
"""
import os
import sys
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


def load_global_data(out_dir):
    """IOmisc.cpp:133-177: GlobalData from points.txt, colors.txt, poses.txt and
    rotations.txt of `out_dir` as cycle.Logs writes them (rawOutput rows).
    Colours are cast with (uchar), i.e. truncated.  Raises ValueError where the
    reference throws: rotation / pose counts or point / colour counts differ."""
    poses = _rows(os.path.join(out_dir, "poses.txt"), 3)
    rotations = _rows(os.path.join(out_dir, "rotations.txt"), 9)
    if len(rotations) != len(poses):
        raise ValueError("Count of rotations and translations must be equal: "
                         f"{len(rotations)} rotations, {len(poses)} translations")
    points = _rows(os.path.join(out_dir, "points.txt"), 3)
    colors = _rows(os.path.join(out_dir, "colors.txt"), 3)
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


def main(config_path):
    """the onlyViz branch of the reference's main(): reload outputDataDir's
    result files, segment the cloud and write clusters.txt and mesh.ply next to
    them."""
    cfg = ConfigService()
    cfg.setConfigFile(config_path)
    if not cfg.getValue("onlyViz"):
        raise ValueError("scene.main handles onlyViz = true; run cycle.slam_main first, then scene.segment")
    out_dir = cfg.getValue("outputDataDir")
    gd = load_global_data(out_dir)
    segments = segment(gd, cfg)
    write_clusters(segments, os.path.join(out_dir, "clusters.txt"))
    write_mesh(gd.spatialPoints, gd.spatialPointsColors, mesh(segments), os.path.join(out_dir, "mesh.ply"))
    return segments


if __name__ == "__main__":
    main(sys.argv[1])

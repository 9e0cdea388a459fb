"""The reference's scene post-processing, up to the 2-D points its Delaunay step
consumes: what runs after slamMain, or after an onlyViz reload of the result
files (src/main.cpp:55-71).

  load_global_data   getGlobalDataFromLogFiles        src/misc/IOmisc.cpp:133-177
  segment            vizualizePointsAndCameras:72-104 src/vizualization/vizualizationModule.cpp
                     (clusterizePoints, getBestFittingPlaneByPoints, the
                     TriangleMinimumPoints filter and makeMesh's projection,
                     bestFittingPlane.cpp:51-63)
  main               the onlyViz branch of main()

The numeric steps are slamhip.api's clusterizePoints / getBestFittingPlaneByPoints
/ projectToPlane (HIP kernels behind the C ABI).  The triangulation itself
(cv::Subdiv2D) and the cv::viz window are out of scope.
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


def main(config_path):
    """the onlyViz branch of the reference's main(): reload outputDataDir's
    result files, segment the cloud and write clusters.txt next to them."""
    cfg = ConfigService()
    cfg.setConfigFile(config_path)
    if not cfg.getValue("onlyViz"):
        raise ValueError("scene.main handles onlyViz = true; run cycle.slam_main first, then scene.segment")
    out_dir = cfg.getValue("outputDataDir")
    segments = segment(load_global_data(out_dir), cfg)
    write_clusters(segments, os.path.join(out_dir, "clusters.txt"))
    return segments


if __name__ == "__main__":
    main(sys.argv[1])

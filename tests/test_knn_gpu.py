"""The matcher's kernels (csrc/knn.hip) against the exact reference on the
adversarial cases of tests/knn_cases.py: every key mode, every shipped kernel
variant, the split and tile seams, ties, the extremes of the key arithmetic,
the ratio test at equality and the multi-frame launch on near-empty frames.
Bit-exact: indices and distances are compared with assert_array_equal.

Every test asserts through slam_last_knn_launch the key mode and the kernel
instance it was written for, so a fixture that drifts to another kernel fails
instead of passing vacuously.  tests/test_knn_cases.py proves the fixtures on
the CPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_cases as K
import slamhip
from slamhip import _lib as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

_REF = {}          # case name -> (idx, dist): computed once, shared by the in-process and the variant tests


def reference(case):
    if case.name not in _REF:
        idx, dist = K.knn2_exact(case.q, case.t, case.norm)
        idx.setflags(write=False)
        dist.setflags(write=False)
        _REF[case.name] = (idx, dist)
    return _REF[case.name]


def _env_int(name):
    try:
        return int(os.environ.get(name, "0") or 0)
    except ValueError:
        return 0


def _env_xcd():
    return 1 if os.environ.get("SLAMHIP_KNN_XCD", "")[:1] == "1" else 0


def check_case(case, idx, dist, launch, matches, pipe, xcd):
    """what the library returned for a case against the exact reference, and the launch it reports"""
    ri, rd = reference(case)
    mode, tsplit, variant = (int(x) for x in launch)
    assert mode == case.mode, f"{case.name}: key mode {mode}, built for {case.mode}"
    assert variant == K.expected_variant(case.mode, pipe, xcd), f"{case.name}: variant {variant:#x}"
    if case.tsplit is not None:
        assert tsplit == case.tsplit, f"{case.name}: tsplit {tsplit}, built for {case.tsplit}"
    np.testing.assert_array_equal(idx, ri, err_msg=case.name)
    np.testing.assert_array_equal(dist, rd, err_msg=case.name)
    if case.expect is not None:
        n = len(case.expect[0])
        np.testing.assert_array_equal(idx[:n], case.expect[0], err_msg=case.name)
        np.testing.assert_array_equal(dist[:n], case.expect[1], err_msg=case.name)
    for r in case.ratios:
        np.testing.assert_array_equal(matches[r], K.ratio_exact(ri, rd, r), err_msg=f"{case.name} ratio {r!r}")


# ---- 1. every case in this process (the default kernels) --------------------------

def test_last_knn_launch_getter():
    ctx = slamhip.Context(0)
    try:
        with pytest.raises(slamhip.SlamError):
            slamhip.lastKnnLaunch(ctx)            # nothing launched yet
        c = K.get("size_sweep-pk-1x1")
        slamhip.knnMatch2(c.q, c.t, c.matcher, ctx=ctx)
        assert slamhip.lastKnnLaunch(ctx) == (K.MODE_L2P, 1, K.expected_variant(K.MODE_L2P, _env_int("SLAMHIP_KNN_PIPE"),
                                                                               _env_xcd()))
        assert slamhip.lib().slam_last_knn_launch(ctx.handle, None, None, None) == L.SLAM_OK
        assert slamhip.lib().slam_last_knn_launch(None, None, None, None) == L.SLAM_E_INVALID_ARG
    finally:
        ctx.close()


@pytest.mark.parametrize("name", K.NAMES)
def test_case(gpu_ctx, name):
    case = K.get(name)
    idx, dist, launch, matches = K.run_case(slamhip, gpu_ctx, case)
    pipe = _env_int("SLAMHIP_KNN_PIPE")
    check_case(case, idx, dist, launch, matches, pipe, _env_xcd())


def test_ratio_edge_match_order(gpu_ctx):
    """slam_match on 700 queries of which every third survives at the equality
    edge: knn_finish's strict double comparison and knn_compact's order over a
    partial last block of 256"""
    for fam in ("pk", "l1", "ham"):
        case = K.get(f"ratio_edge_700-{fam}")
        m = slamhip.matchFeatures(case.q, case.t, case.matcher, K.RATIO_EQ, norm=case.norm, ctx=gpu_ctx)
        assert slamhip.lastKnnLaunch(gpu_ctx)[0] == case.mode
        assert m["queryIdx"].tolist() == list(range(0, 700, 3))
        np.testing.assert_array_equal(m, K.ratio_exact(*reference(case), K.RATIO_EQ))
        case = K.get(f"ratio_edge-{fam}")
        assert len(slamhip.matchFeatures(case.q, case.t, case.matcher, K.RATIO_EQ, norm=case.norm, ctx=gpu_ctx)) == 0
        assert len(slamhip.matchFeatures(case.q, case.t, case.matcher, K.RATIO_ABOVE, norm=case.norm,
                                         ctx=gpu_ctx)) == 1


# ---- 2. the multi-frame launch on frames with 0, 1 and 2 descriptors --------------

def sparse_frames():
    """6 frames of 160 x 120: constant (no keypoint), black with one bright pixel
    at (80, 60) (one keypoint), with two at (50, 40) and (110, 80) (two keypoints
    with identical descriptors: a tie), and three synthetic scenes.  The planted
    points are far enough from the border for ORB's border filter to keep them."""
    fr = np.zeros((6, 120, 160, 3), np.uint8)
    fr[0] = 77
    fr[1, 60, 80] = 255
    fr[2, 40, 50] = 255
    fr[2, 80, 110] = 255
    fr[3:] = slamhip.synth_frames(160, 120, 0, 3, seed=1234)
    return fr


@pytest.mark.parametrize("matcher,norm,mode", [(L.SIFT_BF, L.NORM_L2, K.MODE_L2P), (L.SIFT_BF, L.NORM_L1, K.MODE_L1P),
                                               (L.ORB_BF, L.NORM_HAMMING, K.MODE_HAMP)])
def test_batch_match_sparse_frames(gpu_ctx, matcher, norm, mode):
    import torch
    from slamhip.batch import DeviceBatch
    db = DeviceBatch(gpu_ctx)
    dev = torch.from_numpy(sparse_frames()).cuda()
    db.extract(dev, 12, matcher)
    desc = [db.descriptors(i).copy() for i in range(6)]
    assert [len(d) for d in desc[:3]] == [0, 1, 2]
    assert all(len(d) >= 10 for d in desc[3:])
    for qf in (3, 1, 0):                       # query sets of a full frame, of one descriptor and of none
        q, nq = db.export_desc(qf)
        assert nq == len(desc[qf])
        counts = db.match(q, nq, 0.8, norm=norm)
        if nq:
            assert slamhip.lastKnnLaunch(gpu_ctx)[0] == mode
        for i in range(6):
            ref = K.ratio_exact(*K.knn2_exact(desc[qf], desc[i], norm), 0.8)
            if len(desc[i]) < 2 or nq == 0:
                assert len(ref) == 0
            assert counts[i] == len(ref)
            np.testing.assert_array_equal(db.matches(i, nq), ref)
        if qf == 3:
            assert counts[3] > 0 and counts[4:].sum() > 0         # real matches are being compared


# ---- 3. every shipped kernel variant, each in a process of its own ----------------
# The library reads SLAMHIP_KNN_PIPE / SLAMHIP_KNN_XCD once per process.  A child
# that ends on a signal, a time limit or an abort may have faulted the device:
# nothing more is started on it.
VARIANTS = [("pipe1", {"SLAMHIP_KNN_PIPE": "1"}, 1, 0), ("pipe2", {"SLAMHIP_KNN_PIPE": "2"}, 2, 0),
            ("pipe3", {"SLAMHIP_KNN_PIPE": "3"}, 3, 0), ("xcd", {"SLAMHIP_KNN_XCD": "1"}, 0, 1)]
CHILD_TIMEOUT_S = 60      # a child takes 2.6 - 2.9 s on an MI355X (import, its cases, the .npz): a factor of 20
_device_suspect = []


@pytest.mark.parametrize("tag,env,pipe,xcd", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_variant_child(tmp_path, tag, env, pipe, xcd):
    if _device_suspect:
        pytest.skip(f"an earlier variant child ended abnormally ({_device_suspect[0]}): nothing more is started")
    out = tmp_path / f"{tag}.npz"
    e = {k: v for k, v in os.environ.items() if k not in ("SLAMHIP_KNN_PIPE", "SLAMHIP_KNN_XCD")}
    e.update(env)
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "knn_cases.py"), str(out)], env=e, timeout=CHILD_TIMEOUT_S,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired:
        _device_suspect.append(f"{tag}: time limit")
        pytest.fail(f"{tag}: the child ran into its {CHILD_TIMEOUT_S} s time limit")
    if p.returncode < 0 or p.returncode in (134, 139):
        _device_suspect.append(f"{tag}: exit {p.returncode}")
    assert p.returncode == 0, f"{tag}: exit {p.returncode}\n{p.stdout[-2000:]}"
    with np.load(out) as z:
        names = [str(n) for n in z["names"]]
        assert names == list(K.VARIANT_NAMES)
        seen = set()
        for k, name in enumerate(names):
            case = K.get(name)
            matches = {r: z[f"{k}.m{j}"] for j, r in enumerate(case.ratios)}
            check_case(case, z[f"{k}.idx"], z[f"{k}.dist"], z[f"{k}.launch"], matches, pipe, xcd)
            seen.add((case.mode, int(z[f"{k}.launch"][2])))
    # the variant under test really ran, for L2 and (pipe1, xcd) for Hamming
    want = {("pipe1", K.MODE_L2P): K.V_PIPE_QT2, ("pipe1", K.MODE_HAMP): K.V_PIPE_QT2,
            ("pipe2", K.MODE_L2P): K.V_PIPE_QT1, ("pipe3", K.MODE_L2P): K.V_PK_QT1,
            ("xcd", K.MODE_L2P): K.V_PK_QT2 | K.V_XCD, ("xcd", K.MODE_HAMP): K.V_PK_QT2 | K.V_XCD}
    for (t, mode), v in want.items():
        if t == tag:
            assert (mode, v) in seen

"""One environment-selected form of the full SIFT detector in a process of its
own: a plain program, not a test (tests/test_siftdet_gpu.py starts it).

The library reads the SLAMHIP_SD_* variables once per process, so a form needs
a fresh process with the variable in its environment.  The program runs the
host entry on the dense blocky image and on the 137 x 77 sweep image and the
batch entry on three 144 x 77 frames, compares every keypoint field and every
descriptor with the oracle itself, and checks through
slam_last_sift_detect_forms that the form named on the command line is the one
that ran: a mistyped variable cannot pass as the default form.

usage: siftdet_variant_child.py <forms bitmask> <refine blocks>
exit status 0: all equal and the form ran; 1: not.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "slam-indoor-code_amd"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402


def equal(tag, got, ref):
    (gk, gd), (rk, rd) = got, ref
    bad = []
    if len(gk) != len(rk):
        bad.append(f"count {len(gk)} != {len(rk)}")
    else:
        bad += [f for f in ("x", "y", "size", "angle", "response", "octave", "class_id") if not np.array_equal(gk[f], rk[f])]
        if not np.array_equal(gd, rd):
            bad.append("descriptors")
    print(f"{tag}: {len(rk)} keypoints, " + ("equal" if not bad else "DIFFERENT: " + ", ".join(bad)), flush=True)
    return not bad


def main(argv):
    want = (int(argv[1], 0), int(argv[2], 0))
    import torch
    import siftdet_cases as S
    import slamhip
    if want != S.expected_forms(os.environ):
        print(f"the environment gives forms {S.expected_forms(os.environ)}, asked for {want}")
        return 1
    ctx = slamhip.Context(0)
    ok = True
    for name in ("blocky4", "sweep_w137"):
        ok &= equal(name, slamhip.siftDetectAndCompute(S.image(name), ctx=ctx), S.reference(name))
        got = slamhip.lastSiftDetectForms(ctx)
        print(f"forms {got[0]:#x} refine_blocks {got[1]}", flush=True)
        ok &= got == want
    names = [S.frame(77, 144, 4, 200 + i) for i in range(3)]
    out = slamhip.siftDetectAndComputeBatch(torch.from_numpy(np.stack([S.image(n) for n in names])).cuda(), ctx=ctx)
    for f, n in enumerate(names):
        ok &= equal(f"batch[{f}]", out.host(f), S.reference(n))
    got = slamhip.lastSiftDetectForms(ctx)
    print(f"forms {got[0]:#x} refine_blocks {got[1]}", flush=True)
    ok &= got == want
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))

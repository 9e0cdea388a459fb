"""Co-residency guard (CPU: compiles, no GPU): what the pipelined step runs
beside sift_desc_band must fit on a CU that holds a descriptor workgroup.

The descriptor kernel is persistent, one 8-wave workgroup per CU, two waves per
SIMD, for ~10 ms of a 210-frame step.  With overlap "desc_start" the other
context's FAST (fast_detect, fast_finalize) and the tail of its previous match
(knn_finish, knn_compact) are queued while it runs; whatever does not fit
beside it waits for its tail and is serial again.  A CU
has 160 KB of LDS and each SIMD 512 VGPRs, allocated in steps of 8.

No kNN instance is listed: knn_mfma_pk (107 / 128 VGPRs) does not fit beside two
descriptor waves (204 VGPRs each) and the step does not co-run it; it runs
between two descriptor launches.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-indoor-code_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD = 512

DESCRIPTORS = ["sift_desc_bandILb1ELi1EE", "sift_desc_bandILb1ELi2EE"]
# (source, mangled-name fragment, workgroup waves per SIMD) of the kernels the step queues beside the descriptor
CO_RUN = [
    ("fast.hip", "fast_detectILi1ELi16EE", 1),
    ("fast.hip", "fast_finalize", 1),
    ("knn.hip", "knn_finish", 1),
    ("knn.hip", "knn_compact", 1),
]


def _usage(src):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics",
           "-I" + os.path.join(ROOT, "include"), "-x", "hip", "--cuda-device-only", "-c",
           os.path.join(CSRC, src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return kernels


def _one(kernels, frag):
    hits = [v for k, v in kernels.items() if frag in k]
    assert len(hits) == 1, (frag, len(hits))
    return hits[0]


def _ceil8(n):
    return (n + 7) // 8 * 8


@pytest.fixture(scope="module")
def usage():
    return {src: _usage(src) for src in sorted({"sift_band.hip"} | {c[0] for c in CO_RUN})}


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc absent")
@pytest.mark.parametrize("desc", DESCRIPTORS)
def test_kernels_fit_beside_the_descriptor(usage, desc):
    d = _one(usage["sift_band.hip"], desc)
    assert d["VGPRs Spill"] == 0 and d["ScratchSize [bytes/lane]"] == 0, d
    assert d.get("AGPRs", 0) == 0, d
    co = [(frag, waves, _one(usage[src], frag)) for src, frag, waves in CO_RUN]
    for frag, _, k in co:
        assert k["VGPRs Spill"] == 0 and k["ScratchSize [bytes/lane]"] == 0, (frag, k)
    lds = d["LDS Size [bytes/block]"]
    worst = max(k["LDS Size [bytes/block]"] for _, _, k in co)
    print(f"{desc}: LDS {lds} + {worst} of {LDS_PER_CU}, VGPRs {d['VGPRs']}")
    assert lds + worst <= LDS_PER_CU, (lds, worst)
    for frag, waves, k in co:
        need = 2 * _ceil8(d["VGPRs"]) + waves * _ceil8(k["VGPRs"] + k.get("AGPRs", 0))
        print(f"  {frag}: LDS {k['LDS Size [bytes/block]']}, VGPRs {k['VGPRs']}, per SIMD {need} of {VGPRS_PER_SIMD}")
        assert need <= VGPRS_PER_SIMD, (frag, need)

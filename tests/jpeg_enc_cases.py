"""The committed cases of the JPEG encoder's tests (tests/golden/jpeg_enc, written by
tests/golden/make_jpeg_enc_fixtures.py), shared by tests/test_jpeg_enc.py and
tests/test_jpeg_enc_gpu.py: the sources, the case list, and the contract's stream of a
case, computed once."""
import glob
import json
import os

import numpy as np

import jpeg_enc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "golden", "jpeg_enc")
SAMPLINGS = {"444": R.S444, "422": R.S422, "420": R.S420, "gray": R.GRAY}

with open(os.path.join(DIR, "cases.json")) as _f:
    CASES = json.load(_f)["cases"]
SOURCES = {os.path.basename(p)[:-4]: np.load(p) for p in glob.glob(os.path.join(DIR, "*.npy"))}
_REF = {}


def source(case):
    """the image a case encodes: the gray cases take the green channel of a colour source"""
    img = SOURCES[case["source"]]
    return np.ascontiguousarray(img[..., 1]) if case["sampling"] == "gray" and img.ndim == 3 else img


def ref_stream(k):
    """the contract's stream of case k: computed once, shared by the tests"""
    if k not in _REF:
        c = CASES[k]
        _REF[k] = R.encode(source(c), c["quality"], SAMPLINGS[c["sampling"]], c["restart"])
    return _REF[k]

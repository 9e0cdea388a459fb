"""Where tests/golden/fisheye/ comes from: the reference repository's fisheye
calibration set, docs/artifact/calibration/for_calib_2/Fisheye2_1.jpg ..
Fisheye2_16.jpg (748 x 480 baseline JPEG photos of a board with 6 x 8 inner
corners), copied byte for byte.  Fisheye2_16.jpg is byte-identical to
Fisheye2_1.jpg and is left out: 15 distinct photos.

    python tests/golden/make_fisheye_fixtures.py <reference checkout>
"""
import hashlib
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main(reference):
    src = os.path.join(reference, "docs", "artifact", "calibration", "for_calib_2")
    dst = os.path.join(HERE, "fisheye")
    os.makedirs(dst, exist_ok=True)
    digest = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()
    assert digest(os.path.join(src, "Fisheye2_1.jpg")) == digest(os.path.join(src, "Fisheye2_16.jpg"))
    for i in range(1, 16):
        name = "Fisheye2_%d.jpg" % i
        shutil.copyfile(os.path.join(src, name), os.path.join(dst, name))
        print(name, digest(os.path.join(dst, name))[:16])


if __name__ == "__main__":
    main(sys.argv[1])

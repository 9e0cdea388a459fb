"""Regenerate oracle/orb_pattern.h from scikit-image's ORB position table (data only).

The table equals OpenCV's bit_pattern_31_ used by cv::ORB (reference call site
src/mainModule/featureMatching/featureMatchingCPU.cpp:60).  Its 256 x 4 rows are
kept as tests/golden/orb_bit_pattern_31.npy, which this script checks the header
against: python oracle/gen_orb_pattern.py [positions.txt | table.npy]
"""
import os
import sys

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                   "orb_bit_pattern_31.npy")

def main():
    src = sys.argv[1] if len(sys.argv) > 1 else SRC
    p = (np.load(src) if src.endswith(".npy") else np.loadtxt(src)).astype(int)
    assert p.shape == (256, 4)
    body = "\n".join("    %d,%d, %d,%d," % tuple(r) for r in p)
    with open(__file__.replace("gen_orb_pattern.py", "orb_pattern.h")) as f:
        cur = f.read()
    assert body in cur, "orb_pattern.h is stale"
    print("orb_pattern.h matches", src)

if __name__ == "__main__":
    main()

"""DevLayout (csrc/dev_layout.h), the planner of every staged device buffer, under
AddressSanitizer + UBSan as a stand-alone program (tests/cpp/dev_layout_test.cpp): the 256-byte
carve rule, alignment for every slot type, no overlap, zero-count slots, saturation on overflow
and the strided byte slot.  Plain C++17 with no HIP include: g++ alone builds it.  No GPU.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dev_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "dev_layout_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", os.path.join(ROOT, "tests", "cpp", "dev_layout_test.cpp"),
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().splitlines()[-1].startswith("OK: ")

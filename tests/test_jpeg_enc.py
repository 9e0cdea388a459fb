"""CPU tests of JPEG encoding: the numpy contract
tests/jpeg_enc_ref.py against PIL's committed streams (tests/golden/jpeg_enc, written
by tests/golden/make_jpeg_enc_fixtures.py), the host encoder slam_jpeg_encode_host
against the contract, decoding what was encoded, the capacity rules, the AVI writer,
and the sanitizer-built program over the code the kernels share
(tests/cpp/jpeg_enc_test.cpp).  The device encoder is tested in
tests/test_jpeg_enc_gpu.py."""
import ctypes
import glob
import hashlib
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_enc_ref as R
import jpeg_ref
import slamhip
from slamhip import _lib as L
from slamhip import api

from jpeg_enc_cases import CASES, DIR, ROOT, SAMPLINGS, SOURCES, ref_stream, source


def host_encode(img, quality, sampling, restart=0, cap=None):
    return api.jpegEncode(img, quality, sampling, restart, host=True, cap=cap)


def test_fixture_set_is_complete():
    assert len(CASES) >= 850 and len(SOURCES) >= 18
    names = {c["source"] for c in CASES}
    for h, w in [(1, 1), (2, 2), (3, 5), (7, 8), (8, 8), (16, 9), (9, 17), (12, 16), (20, 16), (8, 40), (17, 33), (29, 37),
                 (40, 25), (48, 50), (256, 256)]:
        assert f"n{h}x{w}" in names
    assert {"checker32x32", "flat24x24", "smooth40x48"} <= names
    assert len(glob.glob(os.path.join(DIR, "pil", "*.jpg"))) >= 18
    assert sum(os.path.getsize(p) for p in glob.glob(os.path.join(DIR, "**", "*"), recursive=True) if os.path.isfile(p)) < 512 * 1024


def test_ref_equals_every_pil_stream():
    """the contract equals PIL / libjpeg-turbo whole-file on all cases: the committed sums, and byte
    for byte where the stream itself is committed"""
    for k, c in enumerate(CASES):
        data = ref_stream(k)
        assert len(data) == c["size"] and hashlib.sha256(data).hexdigest() == c["sha256"], c
        name = os.path.join(DIR, "pil", f"{c['source']}_{c['sampling']}_q{c['quality']}_r{c['restart']}.jpg")
        if os.path.exists(name):
            with open(name, "rb") as f:
                assert f.read() == data, c


def test_fixtures_exercise_the_coder():
    seen = {"zrl": 0, "no_eob": 0, "cat": 0, "wrap": 0, "pair": 0, "last": 0}
    for k, c in enumerate(CASES):
        data = ref_stream(k)
        sos = data.index(b"\xff\xda")
        scan = data[sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big"):-2]
        seen["wrap"] += b"\xff\xd7" in scan and scan.count(b"\xff\xd0") > 1
        seen["pair"] += b"\xff\x00\xff\x00" in scan
        seen["last"] += scan.endswith(b"\xff\x00")
        if c["source"] not in ("checker32x32", "smooth40x48", "n48x50"):
            continue
        st = {}
        assert R.encode(source(c), c["quality"], SAMPLINGS[c["sampling"]], c["restart"], st) == data
        seen["zrl"] += st.get("zrl", 0)
        seen["no_eob"] += st.get("no_eob", 0)
        seen["cat"] = max(seen["cat"], st["max_dc_cat"])
    assert seen["cat"] == 11 and all(seen[k] > 0 for k in ("zrl", "no_eob", "wrap", "pair", "last")), seen
    flat = {}
    R.encode(SOURCES["flat24x24"], 75, R.S420, 0, flat)
    assert len(flat["scan"]) < 32 and not flat.get("zrl") and not flat.get("no_eob")


def test_host_equals_ref_on_all_fixtures():
    for k, c in enumerate(CASES):
        data, size, st = host_encode(source(c), c["quality"], SAMPLINGS[c["sampling"]], c["restart"])
        assert st == 0 and size == len(data) and data == ref_stream(k), c


def test_decode_of_encode():
    """jpeg_ref.decode of an encoded stream equals the host decoder's frame"""
    for c in CASES:
        if c["quality"] not in (50, 100) or c["source"] == "n256x256":
            continue
        k = CASES.index(c)
        want = jpeg_ref.decode(ref_stream(k), 3)
        got, st = api.imdecode_host(ref_stream(k))
        assert st == 0
        np.testing.assert_array_equal(got, want)


def test_fresh_random_encodes_equal_pil():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(20261020)
    sub = {R.S444: 0, R.S422: 1, R.S420: 2}
    for k in range(24):
        h, w = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        sampling = (R.S444, R.S422, R.S420, R.GRAY)[k % 4]
        q = int(rng.integers(1, 101))
        img = rng.integers(0, 256, (h, w) if sampling == R.GRAY else (h, w, 3), dtype=np.uint8)
        if k % 3 == 0:
            img = (img // 32 * 32).astype(np.uint8)
        b = io.BytesIO()
        if sampling == R.GRAY:
            Image.fromarray(img).save(b, format="JPEG", quality=q)
        else:
            Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(b, format="JPEG", quality=q, subsampling=sub[sampling])
        assert R.encode(img, q, sampling) == b.getvalue(), (h, w, sampling, q)
        assert host_encode(img, q, sampling)[0] == b.getvalue()


def test_quality_clamps():
    img = SOURCES["n17x33"]
    assert host_encode(img, 0, R.S420)[0] == host_encode(img, 1, R.S420)[0] == R.encode(img, 1, R.S420)
    assert host_encode(img, 101, R.S420)[0] == host_encode(img, 100, R.S420)[0] == R.encode(img, 101, R.S420)
    assert R.encode(img, 0, R.S420) == R.encode(img, 1, R.S420)


def test_capacity_one_byte_short():
    img = SOURCES["n29x37"]
    full, size, st = host_encode(img, 90, R.S420, 2)
    assert st == 0 and size == len(full)
    buf = np.full(size + 64, 0xA5, np.uint8)
    n = ctypes.c_size_t(0)
    status = ctypes.c_int(0)
    a = np.ascontiguousarray(img)
    rc = L.lib().slam_jpeg_encode_host(L.ptr(a), 29, 37, 3, a.strides[0], 90, R.S420, 2, L.ptr(buf), size - 1, ctypes.byref(n),
                                       ctypes.byref(status))
    assert rc == L.SLAM_OK and n.value == size and status.value == L.JPEG_ENC_OVERFLOW
    assert buf[:size - 1].tobytes() == full[:size - 1] and (buf[size - 1:] == 0xA5).all()
    assert api.jpegEncodeBound(29, 37, R.S420, 2) >= size
    for h, w, s in ((1, 1, R.S444), (29, 37, R.S420), (256, 256, R.GRAY)):      # the bound: headers and markers are in it
        assert api.jpegEncodeBound(h, w, s, 1) > 640 + (h + 7) // 8 * ((w + 7) // 8) * 2 * 207


def test_refusals():
    img = SOURCES["n8x8"]
    for kw in (dict(sampling=0x12), dict(restart_interval=65536), dict(restart_interval=-1)):
        with pytest.raises(L.SlamError):
            api.jpegEncode(img, 90, **{"sampling": R.S420, **kw}, host=True)
    with pytest.raises(TypeError):
        api.jpegEncode(img.astype(np.uint16), host=True)
    assert api.jpegEncodeBound(0, 8) == 0
    assert api.imencode(".png", img, host=True) == (False, b"")


def test_abi_exports():
    lib = L.lib()
    for name in ("slam_jpeg_encode_batch_dev", "slam_jpeg_encode", "slam_jpeg_encode_host", "slam_jpeg_encode_bound",
                 "slam_jpeg_enc_last_timing", "slam_jpeg_enc_last_error"):
        assert name in L.SIGNATURES and getattr(lib, name)
    assert lib.slam_abi_version() == 3
    assert callable(slamhip.imencode) and callable(slamhip.imwrite) and callable(slamhip.imencode_batch)


def test_imencode_params_and_imwrite(tmp_path):
    img = SOURCES["n40x25"]
    ok, data = slamhip.imencode(".jpg", img, host=True)
    assert ok and data == R.encode(img, 95, R.S420)
    ok, data = slamhip.imencode(".JPEG", img, (slamhip.IMWRITE_JPEG_QUALITY, 60, slamhip.IMWRITE_JPEG_RST_INTERVAL, 2,
                                               slamhip.IMWRITE_JPEG_SAMPLING_FACTOR, slamhip.IMWRITE_JPEG_SAMPLING_FACTOR_422), host=True)
    assert ok and data == R.encode(img, 60, R.S422, 2)
    path = str(tmp_path / "x.jpg")
    assert slamhip.imwrite(path, img[..., 0], host=True)
    with open(path, "rb") as f:
        assert f.read() == R.encode(img[..., 0], 95, R.GRAY)
    assert not slamhip.imwrite(str(tmp_path / "x.bmp"), img, host=True)


def test_video_writer_index(tmp_path):
    """what VideoWriter writes, slam_avi_index finds: the same offsets and sizes, and the same frames"""
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (4, 24, 40, 3), dtype=np.uint8)
    frames[2] //= 16
    path = str(tmp_path / "v.avi")
    wr = slamhip.VideoWriter(path, "MJPG", 25, (40, 24), quality=80, restart_rows=1, host=True)
    assert wr.isOpened()
    wr.write(frames[0])
    wr.write_batch(frames[1:])
    streams = list(wr.streams)
    assert streams == [R.encode(f, 80, R.S420, 3) for f in frames]
    assert wr.release() == os.path.getsize(path) and not wr.isOpened()
    with open(path, "rb") as f:
        data = f.read()
    info, off, size = api.aviIndex(data)
    assert info["frames"] == 4 and (info["width"], info["height"]) == (40, 24) and info["fps"] == 25
    pos = data.index(b"movi") + 4
    for i, s in enumerate(streams):
        assert int(off[i]) == pos + 8 and int(size[i]) == len(s) and data[int(off[i]):int(off[i]) + len(s)] == s
        pos += 8 + len(s) + (len(s) & 1)
    cap = slamhip.VideoCapture(path)
    ok, frame = cap.read()
    assert ok
    np.testing.assert_array_equal(frame, jpeg_ref.decode(streams[0], 3))
    assert not slamhip.VideoWriter(str(tmp_path / "w.avi"), "XVID", 25, (40, 24)).isOpened()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_encoder_program_under_sanitizers(tmp_path):
    """every fixture source and fixed-seed random images through the host encoder the kernels share
    their arithmetic with, into buffers of exactly the reported size and one byte short, built with
    the address and undefined-behaviour sanitizers: it must exit clean"""
    exe = str(tmp_path / "jpeg_enc_test")
    csrc = os.path.join(ROOT, "slam-indoor-code_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "jpeg_enc_test.cpp"), os.path.join(csrc, "jpeg_enc_host.cpp"),
                    os.path.join(csrc, "jpeg_parse.cpp")], check=True)
    raw = []
    for name in sorted(SOURCES):
        a = SOURCES[name]
        if a.ndim != 3:
            continue
        p = str(tmp_path / f"{name}.raw")
        with open(p, "wb") as f:
            f.write(np.array([a.shape[0], a.shape[1]], "<i4").tobytes() + a.tobytes())
        raw.append(p)
    r = subprocess.run([exe, "40", *raw], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "encodes" in r.stdout

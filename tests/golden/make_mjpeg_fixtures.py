"""Writes tests/golden/mjpeg: the streams the chunk-parallel entropy decoder and the
Motion-JPEG reader are tested on, encoded by PIL from fixed-seed arrays, each with
PIL's own decode (BGR, .npy) as its expectation, and two corrupt streams derived from
the clean set.  Run once; the output is committed.  tests/golden/jpeg is not touched.

    python tests/golden/make_mjpeg_fixtures.py
"""
import io
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mjpeg")
W, H = 96, 80


def noise(seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def smooth(seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([x * 2 + y, 255 - x - y, (x * y) // 40], -1).astype(np.float64)
    return np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)


def encode(img, **kw):
    bio = io.BytesIO()
    Image.fromarray(img).save(bio, "JPEG", **kw)
    return bio.getvalue()


def scan_range(data):
    pos = 2
    while data[pos + 1] != 0xDA:
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
    start = pos + 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
    return start, len(data) - 2


def main():
    os.makedirs(OUT, exist_ok=True)
    clean = {
        "m96x80_noise_444_q95": encode(noise(1), quality=95, subsampling=0),          # ~19 KB: 1200 chunks of 16 bytes
        "m96x80_smooth_420_q75": encode(smooth(2), quality=75, subsampling=2),        # long zero runs
        "m96x80_mixed_422_q90": encode((noise(3) // 4 + smooth(4) // 4 * 3).astype(np.uint8), quality=90, subsampling=1),
        "m96x80_gray_q85": encode(smooth(5)[..., 0], quality=85),
        "m96x80_noise_420_q75_opt": encode(noise(6), quality=75, subsampling=2, optimize=True),
        "m96x80_noise_444_q100": encode(noise(7), quality=100, subsampling=0),        # 16-bit codes, many FF 00
    }
    for name, data in clean.items():
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        bgr = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]
        np.save(os.path.join(OUT, name + ".npy"), np.ascontiguousarray(bgr))
    big = bytearray(clean["m96x80_noise_444_q95"])
    a, b = scan_range(big)
    mid = (a + b) // 2
    while big[mid] in (0x00, 0xFF) or big[mid - 1] == 0xFF:      # keep the flip a data byte: no marker appears or goes
        mid += 1
    big[mid] ^= 0xA5      # a run past coefficient 63 follows (status 4)
    if big[mid] == 0xFF:
        big[mid] = 0x7F
    with open(os.path.join(OUT, "bad_mid_flip.jpg"), "wb") as f:
        f.write(bytes(big))
    cut = clean["m96x80_mixed_422_q90"]
    a, b = scan_range(cut)
    with open(os.path.join(OUT, "bad_cut.jpg"), "wb") as f:
        f.write(cut[:a + (b - a) * 3 // 5])


if __name__ == "__main__":
    main()

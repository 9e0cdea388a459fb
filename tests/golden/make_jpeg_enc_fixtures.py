"""Writes tests/golden/jpeg_enc/: the sources, PIL's streams and their SHA-256 sums for the
JPEG encoder's tests.  Needs PIL (libjpeg-turbo behind it) and runs where the fixtures
are made only; the tests read what it wrote.

    sources   <name>.npy, fixed seeds: colour noise of every shape (its green channel
              is the gray source), and the special images named below
    pil/      PIL's whole stream for one case of every source and for the special cases
    cases.json  every case (source, sampling, quality, restart interval): the length and
              the SHA-256 of PIL's stream

Restart intervals come from PIL's restart_marker_blocks (MCUs per interval), which the
installed version has; the script stops if it has not.  The script asserts that the set
holds what it is meant to exercise and prints what it found.
"""
import hashlib
import io
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_enc_ref as R  # noqa: E402

OUT = os.path.join(HERE, "jpeg_enc")
SHAPES = [(1, 1), (2, 2), (3, 5), (7, 8), (8, 8), (16, 9), (9, 17), (12, 16), (20, 16), (8, 40), (17, 33), (29, 37),
          (40, 25), (48, 50)]
SAMPLINGS = {"444": R.S444, "422": R.S422, "420": R.S420, "gray": R.GRAY}
QUALITIES = (5, 50, 75, 95, 100)
SUB = {R.S444: 0, R.S422: 1, R.S420: 2}
LIMIT = 512 * 1024
SEARCH = 4000       # seeds tried for the two FF cases


def pil_encode(img, quality, sampling, restart):
    b = io.BytesIO()
    kw = {"restart_marker_blocks": restart} if restart else {}
    if img.ndim == 2:
        Image.fromarray(img).save(b, format="JPEG", quality=quality, **kw)
    else:
        Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(b, format="JPEG", quality=quality,
                                                                   subsampling=SUB[sampling], **kw)
    return b.getvalue()


def source_for(img, sampling):
    return np.ascontiguousarray(img[..., 1]) if sampling == R.GRAY and img.ndim == 3 else img


def mcus_per_row(w, sampling):
    hs = 2 if sampling in (R.S422, R.S420) else 1
    return -(-w // (8 * hs))


def main():
    probe = io.BytesIO()
    Image.new("L", (8, 8)).save(probe, format="JPEG", restart_marker_blocks=1)     # raises where PIL has no restart option
    os.makedirs(os.path.join(OUT, "pil"), exist_ok=True)
    sources = {}
    for k, (h, w) in enumerate(SHAPES):
        sources[f"n{h}x{w}"] = np.random.default_rng(1000 + k).integers(0, 256, (h, w, 3), dtype=np.uint8)
    sources["n256x256"] = np.random.default_rng(7).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:32, 0:32]
    sources["checker32x32"] = np.repeat((((yy // 8 + xx // 8) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    sources["flat24x24"] = np.full((24, 24, 3), 93, np.uint8)
    yy, xx = np.mgrid[0:40, 0:48]
    smooth = np.stack([(3 * xx + yy) % 256, (2 * yy + xx // 2) % 256, (xx * yy // 8) % 256], axis=2).astype(np.uint8)
    smooth[::13, ::11] = 255      # sparse spikes: isolated high-frequency terms, so runs of zeros past 15
    sources["smooth40x48"] = smooth

    # the two FF cases: a bounded search over seeds of 8 x 8 gray noise at quality 100
    found = {}
    for seed in range(SEARCH):
        g = np.random.default_rng(50000 + seed).integers(0, 256, (8, 8), dtype=np.uint8)
        st = {}
        R.encode(g, 100, R.GRAY, 0, st)
        if "ff_last" not in found and st["scan"].endswith(b"\xff\x00"):
            found["ff_last"] = g
        if "ff_pair" not in found and b"\xff\x00\xff\x00" in st["scan"]:
            found["ff_pair"] = g
        if len(found) == 2:
            break
    for k, g in found.items():
        sources[f"{k}8x8"] = g
    # what the search did not find gets no source of its own: the asserts below then rest on the ordinary cases
    print("FF search:", {k: k in found for k in ("ff_last", "ff_pair")}, f"within {SEARCH} seeds")

    cases, whole, seen = [], {}, {"zrl": 0, "no_eob": 0, "max_dc_cat": 0, "ff_pair": 0, "ff_last": 0, "eob_only": 0, "rst_wrap": 0}

    def add(name, sname, quality, restart, keep):
        sampling = SAMPLINGS[sname]
        img = source_for(sources[name], sampling)
        data = pil_encode(img, quality, sampling, restart)
        st = {}
        ref = R.encode(img, quality, sampling, restart, st)
        assert ref == data, (name, sname, quality, restart)
        seen["zrl"] += st.get("zrl", 0)
        seen["no_eob"] += st.get("no_eob", 0)
        seen["max_dc_cat"] = max(seen["max_dc_cat"], st.get("max_dc_cat", 0))
        scan = st["scan"]
        seen["ff_pair"] += b"\xff\x00\xff\x00" in scan
        seen["ff_last"] += scan.endswith(b"\xff\x00")
        seen["rst_wrap"] += b"\xff\xd7" in scan and scan.count(b"\xff\xd0") > 1
        cases.append({"source": name, "sampling": sname, "quality": quality, "restart": restart, "size": len(data),
                      "sha256": hashlib.sha256(data).hexdigest()})
        if keep:
            whole[f"{name}_{sname}_q{quality}_r{restart}.jpg"] = data
        return data

    for (h, w) in SHAPES:
        name = f"n{h}x{w}"
        for sname, sampling in SAMPLINGS.items():
            for q in QUALITIES:
                for restart in (0, 1, mcus_per_row(w, sampling)):
                    add(name, sname, q, restart, keep=(sname == "420" and q == 75 and restart == 0))
    for sname, sampling in SAMPLINGS.items():
        for restart in (0, 1, mcus_per_row(256, sampling)):
            add("n256x256", sname, 100, restart, keep=False)
    add("checker32x32", "gray", 100, 0, True)
    add("checker32x32", "444", 100, 1, True)
    flat = add("flat24x24", "420", 75, 0, True)
    add("flat24x24", "gray", 50, 1, True)
    for q in (5, 50, 95):
        add("smooth40x48", "420", q, 0, q == 50)
        add("smooth40x48", "444", q, 3, False)
    for k in found:
        add(f"{k}8x8", "gray", 100, 0, True)

    # a flat image: after the first block of each component every block is a zero difference and EOB
    st = {}
    R.encode(sources["flat24x24"], 75, R.S420, 0, st)
    seen["eob_only"] = int(st.get("zrl", 0) == 0 and st.get("no_eob", 0) == 0 and len(st["scan"]) < 32)
    assert flat
    print("exercised:", seen)
    assert seen["zrl"] > 0, "no stream with ZRL"
    assert seen["no_eob"] > 0, "no block without EOB"
    assert seen["max_dc_cat"] == 11, "no category-11 DC difference"
    assert seen["eob_only"], "the flat image is not EOB-only"
    assert seen["rst_wrap"] > 0, "no stream whose RSTn wraps"
    assert seen["ff_pair"] > 0, "no FF 00 FF 00 pair"
    if not seen["ff_last"]:
        print(f"no stream whose last scan byte is FF was found within {SEARCH} seeds")

    total = 0
    for name, a in sources.items():
        np.save(os.path.join(OUT, name + ".npy"), a)
        total += os.path.getsize(os.path.join(OUT, name + ".npy"))
    for name, data in whole.items():
        with open(os.path.join(OUT, "pil", name), "wb") as f:
            f.write(data)
        total += len(data)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump({"pil": Image.__version__ if hasattr(Image, "__version__") else "", "cases": cases}, f, separators=(",", ":"))
    total += os.path.getsize(os.path.join(OUT, "cases.json"))
    print(f"{len(sources)} sources, {len(cases)} cases, {len(whole)} whole streams, {total} bytes")
    assert total < LIMIT, total


if __name__ == "__main__":
    main()

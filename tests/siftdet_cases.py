"""Adversarial inputs for the full SIFT detector (csrc/siftdet.hip against
oracle/siftdet.c): fixture builders, numpy only.

The detector's older tests feed it one kind of picture, the synthetic scene's
texture.  These are the pictures it does not see there:

  blocky     random b x b blocks: dense corners at one scale, thousands of
             keypoints over several octaves, many with more than one
             orientation peak, descriptor windows up to the 38-pixel limit and
             windows that leave the octave image
  two-level  0 / 255 only: the largest DoG values the u8 input can give
  bars/ramp  exact periodicity: whole columns of tied DoG values pass the >=
             test of sd_extrema and every one must fall in refinement (singular
             Hessians in solve33); the oracle finds no keypoint
  blobs      Gaussian blobs a few pixels from the borders and corners
  squares    one large structure: sizes up to 44
  strips     frames 11 - 20 pixels across: every window clipped on two sides
  sweep      octave 1 has the input's own size, so the sizes at which sd_blur
             and sd_extrema change from their float4 interior path to the
             per-pixel edge path are reachable one pixel at a time

tests/test_siftdet_cases.py proves on the CPU, with the oracle alone, that the
fixtures reach what they were built for; tests/test_siftdet_gpu.py runs them
through the library.  All images are gray (h, w) uint8.
"""
import numpy as np


def blocky(h, w, b, seed):
    """h x w image of random b x b blocks"""
    r = np.random.default_rng(seed).integers(0, 256, (-(-h // b), -(-w // b)), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(r, np.ones((b, b), np.uint8))[:h, :w])


def bars(h, w, period, vertical):
    """0 / 255 bars, half a period each"""
    n = w if vertical else h
    line = (((np.arange(n) // (period // 2)) & 1) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.tile(line, (h, 1)) if vertical else np.tile(line[:, None], (1, w)))


def blobs():
    """seven Gaussian blobs of sigma 2 - 4, centred 3 - 6 pixels from the borders
    and corners of a 128 x 128 image (x, y, sigma)"""
    spots = [(3, 3, 2.0), (124, 4, 2.5), (5, 122, 3.0), (121, 121, 4.0), (64, 3, 2.0), (6, 64, 3.5), (123, 60, 3.0)]
    yy, xx = np.mgrid[0:128, 0:128].astype(np.float64)
    img = np.full((128, 128), 20.0)
    for x, y, s in spots:
        img += 220.0 * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def square(n, side):
    img = np.full((n, n), 30, np.uint8)
    a = (n - side) // 2
    img[a:a + side, a:a + side] = 220
    return img


def _named():
    c = {}
    c["blocky4"] = lambda: blocky(240, 320, 4, 3)
    c["blocky8"] = lambda: blocky(240, 320, 8, 4)
    c["blocky16"] = lambda: blocky(240, 320, 16, 5)
    c["mix3"] = lambda: ((blocky(240, 320, 4, 1).astype(np.uint16) + blocky(240, 320, 16, 2) + blocky(240, 320, 48, 3))
                         // 3).astype(np.uint8)
    c["two_level"] = lambda: ((blocky(120, 160, 2, 9) > 127) * 255).astype(np.uint8)
    c["mirrored"] = lambda: np.ascontiguousarray(blocky(150, 200, 4, 6)[:, ::-1])
    for p in (4, 8, 16):
        c[f"vbars{p}"] = lambda p=p: bars(96, 128, p, True)
        c[f"hbars{p}"] = lambda p=p: bars(96, 128, p, False)
    c["ramp"] = lambda: np.ascontiguousarray(np.tile((np.arange(256) % 256).astype(np.uint8), (64, 1)))
    c["blobs"] = blobs
    c["square64"] = lambda: square(128, 64)
    c["square65"] = lambda: square(129, 65)
    c["strip20x300"] = lambda: blocky(20, 300, 4, 11)
    c["strip12x400"] = lambda: blocky(12, 400, 4, 12)
    c["strip300x11"] = lambda: blocky(300, 11, 4, 13)
    c["low_contrast"] = lambda: (blocky(120, 160, 4, 7) // 32 + 100).astype(np.uint8)
    return c


_BUILD = _named()
NAMED = tuple(_BUILD)
ZERO = tuple(n for n in NAMED if n.startswith(("vbars", "hbars"))) + ("ramp", "low_contrast")   # the oracle finds none
STRIPS = ("strip20x300", "strip12x400", "strip300x11")

# the size sweep: (name, w, h).  Octave 1 is w x h, octave 0 is 2w x 2h.
# sd_blur<R> takes its float4 path for a tile at (x0, y0) when x0 + 64 + R + 3 <= W
# and y0 + 32 + R <= H (R in 5, 6, 8, 10, 13; the first tile column and row
# never do, x0 - R < 0).  For the second tile column (x0 = 64) the edge is W =
# 128 + R + 3, so the widths 128 + R + {2, 3} = 135 .. 144 sit on both sides of
# it for every R; for the second tile row (y0 = 32) it is H = 64 + R, heights
# 64 + R - {1, 0} = 68 .. 77.  sd_extrema's float4 path needs x0 - 1 + 68 <= W
# and y0 - 1 + 18 <= H with x0 = 5 + 64 bx, y0 = 5 + 16 by: its second tile
# column changes at W = 136 (widths 135 / 136), its fourth tile row at H = 70
# (heights 69 / 70).  Octave 0 puts the doubled sizes on other tiles' edges.
# sd_blur's width condition has slack: the results of its float4 rows are right
# as long as the tile's 64 + 2R columns are real pixels, W >= 128 + R (its
# 16-byte loads stay inside the row from 128 + R + 2 for R = 5, 13 and from
# 128 + R for R = 6, 8, 10; what they read beyond lands in the staged row's pad).
# So the widths 132 .. 134 are swept too: 128 + R - 1 = 132 .. 140 is the widest
# frame at which a float4 row of sd_blur<R> would take the next row's pixels for
# reflected ones.  Its height condition has no slack.  sd_extrema's conditions
# guard reads only, never values: the 5-pixel border keeps every neighbour of a
# tested pixel inside the image, so the columns and rows its edge path clamps
# are read by no test (both paths run here; no result can tell them apart).
SWEEP_W = tuple((f"sweep_w{w}", w, 77) for w in range(132, 145))
SWEEP_H = tuple((f"sweep_h{h}", 144, h) for h in range(68, 78))
SWEEP = SWEEP_W + SWEEP_H
SWEEP_NAMES = tuple(s[0] for s in SWEEP)

# hosts frames with no interior pixel in some or every octave, and frames with an empty pyramid
NO_INTERIOR = ((5, 5), (10, 40), (11, 11), (12, 400))      # (h, w)
EMPTY_PYRAMID = ((1, 50), (50, 1), (2, 50), (50, 2))       # (h, w): 1 x N, N x 1 have no octave, 2 x N one of 4 x 2N

_IMG = {}


def frame(h, w, b, seed):
    """the name of a blocky batch frame, for image() and reference()"""
    return f"blk:{h}:{w}:{b}:{seed}"


def flat(h, w, value=90):
    return f"flat:{h}:{w}:{value}"


def image(name):
    """the named case's, the sweep size's or the batch frame's image (built once, read-only)"""
    if name not in _IMG:
        if name in _BUILD:
            img = _BUILD[name]()
        elif name.startswith("blk:"):
            img = blocky(*(int(v) for v in name.split(":")[1:]))
        elif name.startswith("flat:"):
            h, w, v = (int(v) for v in name.split(":")[1:])
            img = np.full((h, w), v, np.uint8)
        else:
            _, w, h = SWEEP[SWEEP_NAMES.index(name)]
            img = blocky(h, w, 4, seed=w if name.startswith("sweep_w") else h)
        img = np.ascontiguousarray(img, np.uint8)
        img.setflags(write=False)
        _IMG[name] = img
    return _IMG[name]


def small(h, w, seed=21):
    return blocky(h, w, 2, seed)


_REF = {}


def reference(name):
    """the oracle's (keypoints, descriptors) of a named image: computed once,
    shared by the tests that need it, read-only"""
    if name not in _REF:
        import oracle_ffi as O
        k, d = O.sift_detect(image(name))
        k.setflags(write=False)
        d.setflags(write=False)
        _REF[name] = (k, d)
    return _REF[name]


def kp_stats(kps, h, w):
    """per keypoint of a detection of an h x w image: the pyramid octave (0 = the
    doubled image), the descriptor radius rint(3 * scl * sqrt(2) * 2.5), the
    orientation radius rint(4.5 * scl), and whether the descriptor window leaves
    the octave image (some sample of the (2 radius + 1)^2 square is not an
    interior pixel of it).  float32 arithmetic, as calcSIFTDescriptor's."""
    oct_ = (kps["octave"] & 255).astype(np.int32)
    oct_ = np.where(oct_ < 128, oct_, oct_ - 256)
    pyr = oct_ + 1
    scale = np.where(oct_ >= 0, 1.0 / (1 << np.maximum(oct_, 0)), 2.0).astype(np.float32)
    scl = (kps["size"] * scale) * np.float32(0.5)
    cols, rows = (2 * w) >> pyr, (2 * h) >> pyr
    hist_width = np.float32(3.0) * scl
    drad = np.rint(hist_width * np.float32(1.4142135623730951) * np.float32(5) * np.float32(0.5)).astype(np.int32)
    drad = np.minimum(drad, np.sqrt(cols.astype(np.float64) ** 2 + rows.astype(np.float64) ** 2).astype(np.int32))
    orad = np.rint(np.float32(4.5) * scl).astype(np.int32)
    px = np.rint(kps["x"] * scale).astype(np.int32)
    py = np.rint(kps["y"] * scale).astype(np.int32)
    clipped = (px - drad <= 0) | (px + drad >= cols - 1) | (py - drad <= 0) | (py + drad >= rows - 1)
    return {"octave": pyr, "desc_radius": drad, "ori_radius": orad, "clipped": clipped}


def extra_orientations(kps):
    """keypoints that share x, y and size with their predecessor in the sorted
    list and differ in angle: the second and later orientation peaks"""
    if len(kps) < 2:
        return 0
    same = (kps["x"][1:] == kps["x"][:-1]) & (kps["y"][1:] == kps["y"][:-1]) & (kps["size"][1:] == kps["size"][:-1])
    return int(np.count_nonzero(same & (kps["angle"][1:] != kps["angle"][:-1])))


# ---- the detector's environment-selected forms (slam_last_sift_detect_forms) ------
SD_DOG_PLANES, SD_XCD, SD_DESC_STAGED, SD_DESC_CPL2, SD_DESC_XCD = 1, 2, 4, 8, 16
SD_ENV = ("SLAMHIP_SD_DOG", "SLAMHIP_SD_XCD", "SLAMHIP_SD_DESC", "SLAMHIP_SD_CPL", "SLAMHIP_SD_DESC_XCD",
          "SLAMHIP_SD_REFINE_BLOCKS")
# (tag, the child's environment, the bits it must report after a call with descriptors, sd_refine's grid)
FORMS = (("dog", {"SLAMHIP_SD_DOG": "1"}, SD_DOG_PLANES | SD_XCD | SD_DESC_STAGED | SD_DESC_XCD, 4096),
         ("noxcd", {"SLAMHIP_SD_XCD": "0", "SLAMHIP_SD_DESC_XCD": "0"}, SD_DESC_STAGED, 4096),
         ("direct", {"SLAMHIP_SD_DESC": "0"}, SD_XCD, 4096),
         ("cpl2", {"SLAMHIP_SD_CPL": "2"}, SD_XCD | SD_DESC_STAGED | SD_DESC_CPL2 | SD_DESC_XCD, 4096),
         ("refine3", {"SLAMHIP_SD_REFINE_BLOCKS": "3"}, SD_XCD | SD_DESC_STAGED | SD_DESC_XCD, 3))


def _atoi(s):
    try:
        return int(s)
    except (TypeError, ValueError):
        return 0


def expected_forms(env):
    """(bits after a call with descriptors, refine grid) the library reports
    under the SLAMHIP_SD_* variables of env, as csrc/siftdet.hip reads them"""
    staged = _atoi(env["SLAMHIP_SD_DESC"]) != 0 if "SLAMHIP_SD_DESC" in env else True
    cpl2 = staged and "SLAMHIP_SD_CPL" in env and _atoi(env["SLAMHIP_SD_CPL"]) != 1
    bits = (SD_DOG_PLANES if env.get("SLAMHIP_SD_DOG", "")[:1] == "1" else 0) | \
           (SD_XCD if env.get("SLAMHIP_SD_XCD", "")[:1] != "0" else 0) | (SD_DESC_STAGED if staged else 0) | \
           (SD_DESC_CPL2 if cpl2 else 0) | (SD_DESC_XCD if staged and env.get("SLAMHIP_SD_DESC_XCD", "")[:1] != "0" else 0)
    blocks = _atoi(env.get("SLAMHIP_SD_REFINE_BLOCKS"))
    return bits, blocks if blocks > 0 else 4096

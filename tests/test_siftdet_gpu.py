"""The full SIFT detector (csrc/siftdet.hip) against oracle/siftdet.c on the
adversarial inputs of tests/siftdet_cases.py: the float4 fast-path edges of
sd_blur and sd_extrema one pixel at a time, saturated, periodic, tiny and
strip-shaped frames, batches whose tile counts are no multiple of 8, the
outputs without descriptors, short capacities, a caller's stream, the argument
edges, and every environment-selected form in a process of its own.

Every comparison is exact: all seven keypoint fields and every descriptor
element with assert_array_equal.  There is no tolerance in this file.
tests/test_siftdet_cases.py proves on the CPU that the fixtures reach what
they were built for.

Not here, on purpose: sd_desc_staged's fallback for a window wider than kSdW
(78 = 2 * 38 + 1, rounded up).  A detected keypoint's descriptor radius is at
most 38 at three octave layers (scl < 1.6 * 2^(3.5 / 3) = 3.6), so no input
reaches it through the detector; the fixtures reach 38 itself.  Nor a keypoint
with angle exactly 0.0 (the |angle - 360| < FLT_EPSILON fold): the oracle
produced none in 65 588 blocky keypoints, mirrored images included.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import siftdet_cases as S
import slamhip
from slamhip import _lib as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KP = L.KEYPOINT_DTYPE
FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
SENT = 0xA5                       # sentinel byte of output rows the library must not write


def kp_equal(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for f in FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)


def check(got, name):
    rk, rd = S.reference(name)
    kp_equal(got[0], rk)
    if got[1] is not None:
        np.testing.assert_array_equal(got[1], rd, err_msg=name)


def host_raw(ctx, img, cap, rows, with_desc=True):
    """slam_sift_detect itself: (rc, n, kps, desc) with `rows` sentinel-filled output rows"""
    img = np.ascontiguousarray(img)
    h, w = img.shape
    kps = np.full(rows * KP.itemsize, SENT, np.uint8).view(KP) if rows else None
    desc = np.full((rows, 128), -7.0, np.float32) if rows and with_desc else None
    n = ctypes.c_int(-1)
    rc = slamhip.lib().slam_sift_detect(ctx.handle, L.ptr(img), w, h, img.strides[0], 1, L.ptr(kps), cap,
                                        ctypes.byref(n), L.ptr(desc))
    return rc, n.value, kps, desc


def batch_raw(ctx, names, cap, rows=None, with_desc=True, stream=None, nframes=None, w=None):
    """slam_sift_detect_batch itself on the named frames: (rc, counts, kps, desc),
    `rows` (default cap) sentinel-filled rows per frame plus one spare frame's worth"""
    import torch
    frames = torch.from_numpy(np.stack([S.image(n) for n in names])).cuda()
    nf, h, fw = frames.shape
    rows = cap if rows is None else rows
    kps = torch.full(((nf + 1) * rows * KP.itemsize,), SENT, dtype=torch.uint8, device="cuda") if rows else None
    desc = torch.full(((nf + 1) * rows, 128), -7.0, dtype=torch.float32, device="cuda") if rows and with_desc else None
    cnt = np.full(nframes or nf, -1, np.int32)
    torch.cuda.synchronize()
    rc = slamhip.lib().slam_sift_detect_batch(
        ctx.handle, ctypes.c_void_p(stream.cuda_stream) if stream is not None else None,
        ctypes.c_void_p(frames.data_ptr()), nframes or nf, w or fw, h, 1,
        ctypes.c_void_p(kps.data_ptr()) if kps is not None else None, cap, L.ptr(cnt),
        ctypes.c_void_p(desc.data_ptr()) if desc is not None else None)
    torch.cuda.synchronize()
    k = kps.cpu().numpy().view(KP).reshape(nf + 1, rows) if kps is not None else None
    d = desc.cpu().numpy().reshape(nf + 1, rows, 128) if desc is not None else None
    return rc, cnt, k, d


def untouched(kps, desc=None):
    assert (kps.view(np.uint8) == SENT).all()
    if desc is not None:
        assert (desc == -7.0).all()


def check_batch(names, cnt, k, d, cap):
    """every frame's first min(count, cap) rows are the oracle's, the rest untouched"""
    for f, name in enumerate(names):
        rk, rd = S.reference(name)
        assert cnt[f] == len(rk), (name, cnt[f], len(rk))
        m = min(len(rk), cap)
        kp_equal(k[f, :m], rk[:m])
        if d is not None:
            np.testing.assert_array_equal(d[f, :m], rd[:m], err_msg=name)
        untouched(k[f, m:], d[f, m:] if d is not None else None)
    untouched(k[len(names)], d[len(names)] if d is not None else None)


# ---- 1. the host entry: every named case, every sweep size ------------------------

@pytest.mark.parametrize("name", S.NAMED)
def test_named_case(gpu_ctx, name):
    check(slamhip.siftDetectAndCompute(S.image(name), ctx=gpu_ctx), name)


@pytest.mark.parametrize("name", S.SWEEP_NAMES)
def test_sweep_size(gpu_ctx, name):
    """octave 1 on both sides of each float4 interior-path edge of sd_blur
    (every R) and sd_extrema, octave 0 at the doubled sizes"""
    check(slamhip.siftDetectAndCompute(S.image(name), ctx=gpu_ctx), name)


def test_bgr_of_a_case_equals_its_gray(gpu_ctx):
    g = S.image("sweep_h69")
    check(slamhip.siftDetectAndCompute(np.repeat(g[..., None], 3, 2), ctx=gpu_ctx), "sweep_h69")


# ---- 2. the batch entry ---------------------------------------------------------------

@pytest.mark.parametrize("hw", [(40, 40), (77, 144)], ids=["40x40", "144x77"])
@pytest.mark.parametrize("nf", [1, 2, 3, 5, 9])
def test_batch_sizes(gpu_ctx, hw, nf):
    """40 x 40 frames: octave 0 has 2 x 3 blur tiles, so nf frames give 6 nf
    tiles, no multiple of 8 for nf in 1, 2, 3, 5, 9 (xcd_tile's tail)"""
    names = [S.frame(hw[0], hw[1], 4, 200 + i) for i in range(nf)]
    cap = 512
    rc, cnt, k, d = batch_raw(gpu_ctx, names, cap)
    assert rc == L.SLAM_OK
    assert min(len(S.reference(n)[0]) for n in names) >= (20 if hw == (40, 40) else 200)
    check_batch(names, cnt, k, d, cap)


def test_batch_flat_first_and_last_dense_among_sparse(gpu_ctx):
    names = [S.flat(77, 144), S.frame(77, 144, 16, 300), S.frame(77, 144, 4, 200), S.frame(77, 144, 16, 301),
             S.flat(77, 144, 0)]
    rc, cnt, k, d = batch_raw(gpu_ctx, names, 512)
    assert rc == L.SLAM_OK and cnt[0] == 0 and cnt[4] == 0
    assert cnt[2] > 4 * max(cnt[1], cnt[3]) > 0
    check_batch(names, cnt, k, d, 512)


# ---- 3. with_descriptors = False ------------------------------------------------------

@pytest.mark.parametrize("name", ["blocky4", "sweep_w139", "strip300x11", "vbars8"])
def test_host_without_descriptors(gpu_ctx, name):
    k0, d0 = slamhip.siftDetectAndCompute(S.image(name), ctx=gpu_ctx, with_descriptors=False)
    assert d0 is None
    kp_equal(k0, S.reference(name)[0])
    k1, _ = slamhip.siftDetectAndCompute(S.image(name), ctx=gpu_ctx)
    np.testing.assert_array_equal(k0.view(np.uint8), k1.view(np.uint8))


def test_batch_without_descriptors(gpu_ctx):
    """the batch entry's own device-to-device keypoint copies"""
    names = [S.frame(77, 144, 4, 200), S.flat(77, 144), S.frame(77, 144, 4, 201), S.frame(77, 144, 16, 300)]
    rc, cnt, k0, d0 = batch_raw(gpu_ctx, names, 512, with_desc=False)
    assert rc == L.SLAM_OK and d0 is None
    check_batch(names, cnt, k0, None, 512)
    rc, cnt1, k1, _ = batch_raw(gpu_ctx, names, 512)
    assert rc == L.SLAM_OK
    np.testing.assert_array_equal(cnt, cnt1)
    np.testing.assert_array_equal(k0.view(np.uint8), k1.view(np.uint8))
    # a short capacity through the same copies
    rc, cnt, k, _ = batch_raw(gpu_ctx, names, 16, with_desc=False)
    assert rc == L.SLAM_E_CAPACITY
    check_batch(names, cnt, k, None, 16)


# ---- 4. capacity ------------------------------------------------------------------------

@pytest.mark.parametrize("with_desc", [True, False])
def test_host_capacity(gpu_ctx, with_desc):
    rk, rd = S.reference("blocky4")
    rc, n, k, d = host_raw(gpu_ctx, S.image("blocky4"), 16, 32, with_desc)
    assert rc == L.SLAM_E_CAPACITY and n == len(rk)
    kp_equal(k[:16], rk[:16])
    untouched(k[16:])
    if with_desc:
        np.testing.assert_array_equal(d[:16], rd[:16])
        untouched(k[16:], d[16:])
    # a capacity of exactly the count, and one below it
    rc, n, k, d = host_raw(gpu_ctx, S.image("blobs"), len(S.reference("blobs")[0]), 32)
    assert rc == L.SLAM_OK
    check((k[:n], d[:n]), "blobs")
    untouched(k[n:], d[n:])
    rc, n, k, d = host_raw(gpu_ctx, S.image("blobs"), len(S.reference("blobs")[0]) - 1, 32)
    assert rc == L.SLAM_E_CAPACITY and n == len(S.reference("blobs")[0])
    untouched(k[n - 1:], d[n - 1:])


def test_batch_capacity(gpu_ctx):
    names = [S.frame(77, 144, 4, 200), S.flat(77, 144), S.frame(77, 144, 4, 201), S.frame(77, 144, 16, 300)]
    rc, cnt, k, d = batch_raw(gpu_ctx, names, 16, rows=24)
    assert rc == L.SLAM_E_CAPACITY and cnt.max() > 200
    # 24 rows per frame were allocated; the library's frame stride is cap = 16
    flatk = k.reshape(-1)
    flatd = d.reshape(-1, 128)
    for f, name in enumerate(names):
        rk, rd = S.reference(name)
        assert cnt[f] == len(rk)
        m = min(len(rk), 16)
        kp_equal(flatk[f * 16:f * 16 + m], rk[:m])
        np.testing.assert_array_equal(flatd[f * 16:f * 16 + m], rd[:m])
        untouched(flatk[f * 16 + m:(f + 1) * 16], flatd[f * 16 + m:(f + 1) * 16])
    untouched(flatk[len(names) * 16:], flatd[len(names) * 16:])


def test_counts_only(gpu_ctx):
    """cap = 0 with null outputs: the counts, and SLAM_E_CAPACITY where there are keypoints"""
    rc, n, _, _ = host_raw(gpu_ctx, S.image("blocky8"), 0, 0)
    assert rc == L.SLAM_E_CAPACITY and n == len(S.reference("blocky8")[0])
    rc, n, _, _ = host_raw(gpu_ctx, S.image("vbars4"), 0, 0)
    assert rc == L.SLAM_OK and n == 0
    names = [S.frame(77, 144, 4, 200), S.flat(77, 144), S.frame(77, 144, 16, 300)]
    rc, cnt, _, _ = batch_raw(gpu_ctx, names, 0)
    assert rc == L.SLAM_E_CAPACITY
    assert cnt.tolist() == [len(S.reference(n)[0]) for n in names]
    rc, cnt, _, _ = batch_raw(gpu_ctx, [S.flat(77, 144)] * 2, 0)
    assert rc == L.SLAM_OK and cnt.tolist() == [0, 0]


# ---- 5. a caller's stream ---------------------------------------------------------------

def test_batch_on_caller_stream(gpu_ctx):
    """the batch entry on a non-default stream directly after a call on the
    context's own stream: the caller's stream waits for the earlier call's
    readers of the shared scratch (ev_order)"""
    import torch
    a = [S.frame(77, 144, 4, 200 + i) for i in range(3)]
    b = [S.frame(77, 144, 4, 203 + i) for i in range(2)] + [S.frame(77, 144, 16, 300)]
    s = torch.cuda.Stream()
    rc, cnt, k, d = batch_raw(gpu_ctx, a, 512)
    assert rc == L.SLAM_OK
    rc2, cnt2, k2, d2 = batch_raw(gpu_ctx, b, 512, stream=s)
    assert rc2 == L.SLAM_OK
    check_batch(a, cnt, k, d, 512)
    check_batch(b, cnt2, k2, d2, 512)
    rc, cnt, k, d = batch_raw(gpu_ctx, a, 512, with_desc=False, stream=s)      # the stream's second call, no descriptors
    assert rc == L.SLAM_OK
    check_batch(a, cnt, k, None, 512)


# ---- 6. argument edges ------------------------------------------------------------------

def test_batch_argument_edges(gpu_ctx):
    # 257 frames: refused before anything is allocated (the buffer holds 2 frames; it is never read)
    names = [S.frame(16, 16, 4, 1), S.frame(16, 16, 4, 2)]
    rc, cnt, k, d = batch_raw(gpu_ctx, names, 4, nframes=257)
    assert rc == L.SLAM_E_INVALID_ARG and (cnt == 0).all()
    untouched(k, d)
    rc, cnt, k, d = batch_raw(gpu_ctx, names, 4, w=2)
    assert rc == L.SLAM_E_INVALID_ARG and (cnt == 0).all()
    untouched(k, d)
    rc, cnt, k, d = batch_raw(gpu_ctx, names, 4)             # and the same frames as they are: 16 x 16
    assert rc in (L.SLAM_OK, L.SLAM_E_CAPACITY)
    check_batch(names, cnt, k, d, 4)


@pytest.mark.parametrize("hw", S.EMPTY_PYRAMID + ((1, 1), (1, 4096)), ids=lambda hw: f"{hw[1]}x{hw[0]}")
def test_host_empty_pyramid(gpu_ctx, hw):
    """a frame 1 pixel wide or tall has no octave (cvRound(log2(2) - 2) + 1 = 0):
    SLAM_OK and no keypoint, as the oracle, and nothing launched; 2 x N has one
    octave of 4 x 2N without an interior pixel"""
    img = S.small(*hw)
    rc, n, k, d = host_raw(gpu_ctx, img, 8, 8)
    assert rc == L.SLAM_OK and n == 0
    untouched(k, d)
    k, d = slamhip.siftDetectAndCompute(img, ctx=gpu_ctx)
    assert len(k) == 0 and d.shape == (0, 128)


@pytest.mark.parametrize("hw", S.NO_INTERIOR, ids=lambda hw: f"{hw[1]}x{hw[0]}")
def test_host_no_interior(gpu_ctx, hw):
    """frames whose octaves (some or all) are at most 10 pixels across: no pixel
    inside the 5-pixel border, blur halos that reflect more than once"""
    import oracle_ffi as O
    img = S.small(*hw)
    rk, rd = O.sift_detect(img)
    gk, gd = slamhip.siftDetectAndCompute(img, ctx=gpu_ctx)
    kp_equal(gk, rk)
    np.testing.assert_array_equal(gd, rd)


# ---- 7. the forms ---------------------------------------------------------------------

def test_forms_getter():
    ctx = slamhip.Context(0)
    try:
        with pytest.raises(slamhip.SlamError):
            slamhip.lastSiftDetectForms(ctx)            # no detector call yet
        slamhip.siftDetectAndCompute(S.small(1, 50), ctx=ctx)
        with pytest.raises(slamhip.SlamError):
            slamhip.lastSiftDetectForms(ctx)            # an empty pyramid launches nothing
        bits, blocks = S.expected_forms(os.environ)
        slamhip.siftDetectAndCompute(S.image("blobs"), ctx=ctx, with_descriptors=False)
        assert slamhip.lastSiftDetectForms(ctx) == (bits & (S.SD_DOG_PLANES | S.SD_XCD), blocks)
        slamhip.siftDetectAndCompute(S.image("blobs"), ctx=ctx)
        assert slamhip.lastSiftDetectForms(ctx) == (bits, blocks)
        assert slamhip.lib().slam_last_sift_detect_forms(ctx.handle, None, None) == L.SLAM_OK
        assert slamhip.lib().slam_last_sift_detect_forms(None, None, None) == L.SLAM_E_INVALID_ARG
    finally:
        ctx.close()


# The library reads the SLAMHIP_SD_* variables once per process: one fresh child
# per form, one at a time.  A child that ends on a signal or its time limit may
# have faulted the device: the session ends there, nothing further starts on it.
CHILD_TIMEOUT_S = 120


@pytest.mark.parametrize("tag,env,bits,blocks", S.FORMS, ids=[f[0] for f in S.FORMS])
def test_form_child(tag, env, bits, blocks):
    assert S.expected_forms(env) == (bits, blocks)
    e = {k: v for k, v in os.environ.items() if k not in S.SD_ENV}
    e.update(env)
    try:
        p = subprocess.run([sys.executable, os.path.join(HERE, "siftdet_variant_child.py"), str(bits), str(blocks)], env=e,
                           timeout=CHILD_TIMEOUT_S, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired:
        pytest.exit(f"detector form {tag}: the child ran into its {CHILD_TIMEOUT_S} s time limit", returncode=3)
    if p.returncode < 0 or p.returncode in (134, 139):
        pytest.exit(f"detector form {tag}: the child ended on a signal (exit {p.returncode})\n{p.stdout[-2000:]}",
                    returncode=3)
    print(p.stdout)
    assert p.returncode == 0, f"{tag}: exit {p.returncode}\n{p.stdout[-2000:]}"
    assert f"forms {bits:#x} refine_blocks {blocks}" in p.stdout

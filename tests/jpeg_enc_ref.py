"""numpy restatement of libjpeg's baseline encoder: the contract of slam_jpeg_encode.

What cv::imwrite / cv::imencode(".jpg") and PIL's save(format="JPEG") run with
libjpeg's defaults (jpeg_set_defaults, jpeg_set_quality(q, TRUE)): jccolor.c
(SCALEBITS 16), jcprepct.c / jcsample.c (edge replication and the h2v1 / h2v2
box filters), jccoefct.c (dummy blocks), jfdctint.c jpeg_fdct_islow, jcdctmgr.c
(quantisation), jchuff.c with the Annex K tables, jcmarker.c.  No optimisation, no
smoothing.  Scalar integer arithmetic throughout; slam_jpeg_encode_host and the
kernels of jpeg_enc.hip must equal encode() byte for byte.
"""
import numpy as np

GRAY, S444, S422, S420 = 0, 0x11, 0x21, 0x22

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                   41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.1, natural order
QLUM = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
QCHR = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

# Annex K.3: counts per code length 1 .. 16, then the values
DC_COUNTS = [[0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]]
DC_VALS = [list(range(12)), list(range(12))]
AC_COUNTS = [[0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]]
AC_VALS = [
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
]


def FIX(x):
    return int(x * 65536 + 0.5)


def quant_table(base, quality):
    """jpeg_set_quality(q, TRUE): the scaled table, natural order."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base.astype(np.int64) * scale + 50) // 100, 1, 255)


def huff_codes(counts, vals):
    """symbol -> (code, length), Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def bgr_to_ycc(img):
    b, g, r = (img[..., i].astype(np.int64) for i in range(3))
    y = (FIX(.299) * r + FIX(.587) * g + FIX(.114) * b + 32768) >> 16
    cb = (-FIX(.16874) * r - FIX(.33126) * g + FIX(.5) * b + (128 << 16) + 32767) >> 16
    cr = (FIX(.5) * r - FIX(.41869) * g - FIX(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def geometry(h, w, sampling):
    """(ncomp, [(hc, vc)], hmax, vmax, mcux, mcuy, [(blocks wide, blocks high)])"""
    if sampling == GRAY:
        fac = [(1, 1)]
    else:
        fac = [(sampling >> 4, sampling & 15), (1, 1), (1, 1)]
    hmax, vmax = fac[0]
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    grid = [(-(-(-(-w * hc // hmax)) // 8), -(-(-(-h * vc // vmax)) // 8)) for hc, vc in fac]
    return len(fac), fac, hmax, vmax, mcux, mcuy, grid


def _pad_to(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def component_planes(img, sampling):
    """The component planes as the FDCT sees them: padded to the MCU grid by jcprepct.c's order."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    n, fac, hmax, vmax, mcux, mcuy, _ = geometry(h, w, sampling)
    if img.ndim == 2 or img.shape[2] == 1:
        planes = [img.reshape(h, w).astype(np.int64)]
    else:
        planes = list(bgr_to_ycc(img))[:n]
    W, H = mcux * 8 * hmax, mcuy * 8 * vmax
    h_in = -(-h // vmax) * vmax                      # the bottom row only up to a multiple of the vertical factor
    out = []
    for c, p in enumerate(planes):
        p = _pad_to(p, h_in, W)
        hc, vc = fac[c]
        if hmax // hc == 2 and vmax // vc == 1:
            bias = np.arange(W // 2) & 1
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        elif hmax // hc == 2 and vmax // vc == 2:
            bias = 1 + (np.arange(W // 2) & 1)
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        out.append(_pad_to(p, H * vc // vmax, W * hc // hmax))
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_islow(block):
    """jfdctint.c jpeg_fdct_islow on an 8 x 8 block of samples - 128 (any leading dimensions)."""
    C = {k: int(v * 8192 + 0.5) for k, v in dict(a=0.298631336, b=0.390180644, c=0.541196100, d=0.765366865,
                                                 e=0.899976223, f=1.175875602, g=1.501321110, h=1.847759065,
                                                 i=1.961570560, j=2.053119869, k=2.562915447, l=3.072711026).items()}
    d = np.asarray(block, dtype=np.int64)
    for p in range(2):
        x = [d[..., i] for i in range(8)]
        t0, t7 = x[0] + x[7], x[0] - x[7]
        t1, t6 = x[1] + x[6], x[1] - x[6]
        t2, t5 = x[2] + x[5], x[2] - x[5]
        t3, t4 = x[3] + x[4], x[3] - x[4]
        t10, t13 = t0 + t3, t0 - t3
        t11, t12 = t1 + t2, t1 - t2
        o = [None] * 8
        if p == 0:
            o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
            sh = 11
        else:
            o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
            sh = 15
        z1 = (t12 + t13) * C["c"]
        o[2] = _descale(z1 + t13 * C["d"], sh)
        o[6] = _descale(z1 - t12 * C["h"], sh)
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * C["f"]
        t4, t5, t6, t7 = t4 * C["a"], t5 * C["j"], t6 * C["l"], t7 * C["g"]
        z1, z2, z3, z4 = -z1 * C["e"], -z2 * C["k"], -z3 * C["i"] + z5, -z4 * C["b"] + z5
        o[7] = _descale(t4 + z1 + z3, sh)
        o[5] = _descale(t5 + z2 + z4, sh)
        o[3] = _descale(t6 + z2 + z3, sh)
        o[1] = _descale(t7 + z1 + z4, sh)
        d = np.stack(o, axis=-1)
        d = np.swapaxes(d, -1, -2)      # rows first, then columns
    return d


def quantise(t, q):
    qq = 8 * q.reshape(8, 8).astype(np.int64)
    v = (np.abs(t) + (qq >> 1)) // qq
    return np.where(t < 0, -v, v)


def scan_blocks(img, quality=95, sampling=S420):
    """The quantised blocks in scan order: a list of (component, 64 coefficients in zigzag order, dummy)."""
    img = np.asarray(img)
    if img.ndim == 2 or img.shape[2] == 1:
        sampling = GRAY
    h, w = img.shape[:2]
    n, fac, hmax, vmax, mcux, mcuy, grid = geometry(h, w, sampling)
    planes = component_planes(img, sampling)
    coefs = []
    for c, p in enumerate(planes):
        q = quant_table(QLUM if c == 0 else QCHR, quality)
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        blocks = p.reshape(bh, 8, bw, 8).swapaxes(1, 2) - 128
        coefs.append(quantise(fdct_islow(blocks), q).reshape(bh, bw, 64)[..., ZIGZAG])
    out = []
    for my in range(mcuy):
        for mx in range(mcux):
            for c in range(n):
                hc, vc = fac[c]
                for by in range(vc):
                    for bx in range(hc):
                        col, row = mx * hc + bx, my * vc + by
                        if col < grid[c][0] and row < grid[c][1]:
                            out.append((c, coefs[c][row, col], False))
                        else:                       # jccoefct.c: not transformed; DC of the block before it
                            z = np.zeros(64, dtype=np.int64)
                            z[0] = out[-1][1][0]
                            out.append((c, z, True))
    return out, mcux * mcuy, len(out) // (mcux * mcuy)


class _Bits:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _nbits(v):
    return int(abs(int(v))).bit_length()


def encode_block(bits, zz, pred, dc, ac, stats=None):
    diff = int(zz[0]) - pred
    t = _nbits(diff)
    assert t <= 11, "DC category past the table"
    bits.put(*dc[t])
    if t:
        bits.put((diff if diff >= 0 else diff - 1) & ((1 << t) - 1), t)
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac[0xF0])
            run -= 16
            if stats is not None:
                stats["zrl"] = stats.get("zrl", 0) + 1
        t = _nbits(v)
        assert t <= 10, "AC category past the table"
        bits.put(*ac[(run << 4) | t])
        bits.put((v if v >= 0 else v - 1) & ((1 << t) - 1), t)
        run = 0
    if run:
        bits.put(*ac[0])
    elif stats is not None:
        stats["no_eob"] = stats.get("no_eob", 0) + 1
    if stats is not None:
        stats["max_dc_cat"] = max(stats.get("max_dc_cat", 0), _nbits(diff))
    return int(zz[0])


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def header(h, w, quality, sampling, restart_interval):
    n, fac = geometry(h, w, sampling)[:2]
    out = bytearray(b"\xff\xd8")
    out += _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2 if n == 3 else 1):
        q = quant_table(QLUM if t == 0 else QCHR, quality)
        out += _seg(0xDB, bytes([t]) + bytes(int(v) for v in q[ZIGZAG]))
    sof = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([n])
    for c in range(n):
        sof += bytes([c + 1, fac[c][0] << 4 | fac[c][1], 0 if c == 0 else 1])
    out += _seg(0xC0, sof)
    for t in range(2 if n == 3 else 1):
        out += _seg(0xC4, bytes([t]) + bytes(DC_COUNTS[t]) + bytes(DC_VALS[t]))
        out += _seg(0xC4, bytes([0x10 | t]) + bytes(AC_COUNTS[t]) + bytes(AC_VALS[t]))
    if restart_interval:
        out += _seg(0xDD, restart_interval.to_bytes(2, "big"))
    sos = bytes([n])
    for c in range(n):
        sos += bytes([c + 1, 0 if c == 0 else 0x11])
    out += _seg(0xDA, sos + bytes([0, 63, 0]))
    return bytes(out)


def encode(img, quality=95, sampling=S420, restart_interval=0, stats=None):
    """The JPEG stream of an h x w (gray) or h x w x 3 (BGR) uint8 image."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2 or img.shape[2] == 1:
        sampling = GRAY
    h, w = img.shape[:2]
    blocks, nmcu, bpm = scan_blocks(img, quality, sampling)
    dc = [huff_codes(DC_COUNTS[t], DC_VALS[t]) for t in range(2)]
    ac = [huff_codes(AC_COUNTS[t], AC_VALS[t]) for t in range(2)]
    out = bytearray(header(h, w, quality, sampling, restart_interval))
    bits = _Bits()
    pred = [0, 0, 0]
    nrst = 0
    for m in range(nmcu):
        if restart_interval and m and m % restart_interval == 0:
            bits.flush()
            bits.out += bytes([0xFF, 0xD0 + (nrst & 7)])
            nrst += 1
            pred = [0, 0, 0]
        for c, zz, _ in blocks[m * bpm:(m + 1) * bpm]:
            t = 0 if c == 0 else 1
            pred[c] = encode_block(bits, zz, pred[c], dc[t], ac[t], stats)
    bits.flush()
    if stats is not None:
        stats["scan"] = bytes(bits.out)
    return bytes(out + bits.out + b"\xff\xd9")

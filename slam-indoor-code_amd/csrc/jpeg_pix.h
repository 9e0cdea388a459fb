// Baseline JPEG sample reconstruction, host and device, header only: libjpeg's
// jidctint.c (jpeg_idct_islow), its range-limit table, jdsample.c (fancy
// upsampling) and jdcolor.c restated in 32-bit integers.  jpeg.hip's jpeg_idct and
// jpeg_upcolor kernels and the host decoder (jpeg_parse.cpp) call the same
// functions.
//
// All sums and products are taken on uint32_t and read back as int32_t only for
// the arithmetic right shifts: a hostile stream (coefficients of +-32767 under
// quantisers of 255) wraps modulo 2^32 instead of overflowing a signed type.
// Streams an encoder makes stay far inside int32 (the largest intermediate at
// tables scaled x4 is 2^27.1), where this is libjpeg's scalar arithmetic exactly.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JPEG_HD __host__ __device__
#else
#define JPEG_HD
#endif

namespace jpeg {

constexpr int kConstBits = 13, kPass1Bits = 2;
// FIX(x) = round(x * 8192)
constexpr uint32_t kFix0_298631336 = 2446, kFix0_390180644 = 3196, kFix0_541196100 = 4433, kFix0_765366865 = 6270,
                   kFix0_899976223 = 7373, kFix1_175875602 = 9633, kFix1_501321110 = 12299, kFix1_847759065 = 15137,
                   kFix1_961570560 = 16069, kFix2_053119869 = 16819, kFix2_562915447 = 20995,
                   kFix3_072711026 = 25172;

// (x + 2^(s-1)) >> s, arithmetic
JPEG_HD inline uint32_t descale(uint32_t x, int s) { return (uint32_t)((int32_t)(x + (1u << (s - 1))) >> s); }

// One 1-D pass of the islow butterfly over in[0 .. 7] (dequantised coefficients
// of a column, or a row of the first pass's results, as two's complement),
// descaled by `shift`: 11 (CONST_BITS - PASS1_BITS) for the column pass, 18
// (CONST_BITS + PASS1_BITS + 3) for the row pass.
JPEG_HD inline void idct_pass(const uint32_t* in, uint32_t* out, int shift)
{
    uint32_t z2 = in[2], z3 = in[6];
    uint32_t z1 = (z2 + z3) * kFix0_541196100;
    uint32_t tmp2 = z1 - z3 * kFix1_847759065;
    uint32_t tmp3 = z1 + z2 * kFix0_765366865;
    z2 = in[0];
    z3 = in[4];
    uint32_t tmp0 = (z2 + z3) << kConstBits;
    uint32_t tmp1 = (z2 - z3) << kConstBits;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;

    tmp0 = in[7];
    tmp1 = in[5];
    tmp2 = in[3];
    tmp3 = in[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * kFix1_175875602;
    tmp0 *= kFix0_298631336;
    tmp1 *= kFix2_053119869;
    tmp2 *= kFix3_072711026;
    tmp3 *= kFix1_501321110;
    z1 = 0u - z1 * kFix0_899976223;
    z2 = 0u - z2 * kFix2_562915447;
    z3 = 0u - z3 * kFix1_961570560;
    z4 = 0u - z4 * kFix0_390180644;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;

    out[0] = descale(tmp10 + tmp3, shift);
    out[7] = descale(tmp10 - tmp3, shift);
    out[1] = descale(tmp11 + tmp2, shift);
    out[6] = descale(tmp11 - tmp2, shift);
    out[2] = descale(tmp12 + tmp1, shift);
    out[5] = descale(tmp12 - tmp1, shift);
    out[3] = descale(tmp13 + tmp0, shift);
    out[4] = descale(tmp13 - tmp0, shift);
}

// column c of a block: dequantise (coef * q in 32 bits) and run the column pass
JPEG_HD inline void idct_column(const int16_t* coef, const uint16_t* q, int c, uint32_t* out)
{
    uint32_t in[8];
    for (int r = 0; r < 8; r++) in[r] = (uint32_t)((int32_t)coef[r * 8 + c] * (int32_t)q[r * 8 + c]);
    idct_pass(in, out, kConstBits - kPass1Bits);
}

// libjpeg's range_limit table behind "& RANGE_MASK": a lookup with wrap, not a clamp
JPEG_HD inline uint8_t range_limit(uint32_t v)
{
    const uint32_t x = v & 0x3FFu;
    return (uint8_t)(x < 128u ? x + 128u : x < 512u ? 255u : x < 896u ? 0u : x - 896u);
}

// a row of the first pass's results to 8 samples
JPEG_HD inline void idct_row(const uint32_t* ws, uint8_t* out)
{
    uint32_t o[8];
    idct_pass(ws, o, kConstBits + kPass1Bits + 3);
    for (int i = 0; i < 8; i++) out[i] = range_limit(o[i]);
}

// SLAM_JPEG_* sampling codes (include/slamhip.h): (luma h << 4) | luma v
constexpr int kGray = 0, k444 = 0x11, k422 = 0x21, k420 = 0x22;

// The chroma sample of output pixel (x, y), from a plane of pitch `pitch` cropped
// to cw x ch.  jdsample.c picks the triangle filters only for planes wider than
// two samples and replicates otherwise.
JPEG_HD inline int chroma_sample(const uint8_t* plane, int pitch, int cw, int ch, int sampling, int x, int y)
{
    if (sampling == k444) return plane[(size_t)y * pitch + x];
    const int i = x >> 1;
    if (sampling == k422) {
        const uint8_t* p = plane + (size_t)y * pitch;
        if (cw <= 2) return p[i];
        if (x & 1) return i == cw - 1 ? p[i] : (3 * p[i] + p[i + 1] + 2) >> 2;
        return i == 0 ? p[i] : (3 * p[i] + p[i - 1] + 1) >> 2;
    }
    const int near = y >> 1;
    if (cw <= 2) return plane[(size_t)near * pitch + i];
    int far = (y & 1) ? near + 1 : near - 1;
    far = far < 0 ? 0 : far > ch - 1 ? ch - 1 : far;
    const uint8_t* pn = plane + (size_t)near * pitch;
    const uint8_t* pf = plane + (size_t)far * pitch;
    const int s = 3 * pn[i] + pf[i];
    if (x & 1) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * pn[i + 1] + pf[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * pn[i - 1] + pf[i - 1] + 8) >> 4;
}

JPEG_HD inline uint8_t clamp_u8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// jdcolor.c's YCbCr -> RGB with FIX(x) = int(x * 65536 + 0.5), written as B, G, R
JPEG_HD inline void ycc_to_bgr(int y, int cb, int cr, uint8_t* bgr)
{
    cb -= 128;
    cr -= 128;
    bgr[0] = clamp_u8(y + ((116130 * cb + 32768) >> 16));
    bgr[1] = clamp_u8(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    bgr[2] = clamp_u8(y + ((91881 * cr + 32768) >> 16));
}

}  // namespace jpeg

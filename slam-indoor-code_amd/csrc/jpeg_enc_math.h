// Baseline JPEG encoding (libjpeg's encoder restated), host
// and device, header only: colour conversion and the edge / downsampling rules on
// the load (jccolor.c, jcprepct.c, jcsample.c), jpeg_fdct_islow (jfdctint.c),
// quantisation (jcdctmgr.c), the dummy-block rule (jccoefct.c) and the Huffman
// coding of one block (jchuff.c) into a sink.  jpeg_enc.hip's kernels and the host
// encoder (jpeg_enc_host.cpp) call the same functions; tests/jpeg_enc_ref.py is the
// contract and tests/cpp/jpeg_enc_test.cpp runs the host side under the sanitizers.
//
// Bounds.  Every sample address is clamped into the frame, every table index is
// masked (a category past the tables sets kEncCategory and is clamped), every loop
// has a fixed trip count.
#pragma once

#include <stdint.h>

#include "jpeg_huff.h"

namespace jpeg {

constexpr int kEncOverflow = 1;      // SLAM_JPEG_ENC_OVERFLOW: the stream is longer than the caller's capacity
constexpr int kEncCategory = 2;      // SLAM_JPEG_ENC_CATEGORY: a coefficient past the Huffman tables (never from 8-bit input)
constexpr int kEncHeaderMax = 640;   // SOI .. SOS of a colour stream with DRI is 629 bytes
// The longest block: an 11-bit DC code + 11 bits, and 63 AC terms of a 16-bit code + 10 bits.
constexpr int kEncMaxBlockBits = 22 + 63 * 26;

struct EncTables {
    uint16_t quant[2][64];       // natural order
    uint16_t dc_code[2][16];     // by category; 12 used
    uint8_t dc_len[2][16];
    uint16_t ac_code[2][256];    // by run << 4 | category
    uint8_t ac_len[2][256];
};

struct EncGeom {
    int32_t w, h, channels;      // of the frames: 1 or 3
    int32_t ncomp, hs, vs;       // components written; luma sampling factors (chroma is 1 x 1)
    int32_t mcux, mcuy, bpm;     // the MCU grid and the blocks of one MCU
    int32_t bw[3], bh[3];        // each component's own block grid: what lies beyond is a dummy block
    uint32_t nmcu, ri, nint;     // MCUs; MCUs per restart interval (nmcu when there is none); intervals
    uint64_t row_step, frame_step;
};

// FIX(x) = int(x 65536 + 0.5) of jccolor.c, written out
JPEG_HD inline int enc_y(const uint8_t* p)
{
    return (19595 * p[2] + 38470 * p[1] + 7471 * p[0] + 32768) >> 16;
}
JPEG_HD inline int enc_cb(const uint8_t* p)
{
    return (-11059 * p[2] - 21709 * p[1] + 32768 * p[0] + (128 << 16) + 32767) >> 16;
}
JPEG_HD inline int enc_cr(const uint8_t* p)
{
    return (32768 * p[2] - 27439 * p[1] - 5329 * p[0] + (128 << 16) + 32767) >> 16;
}

JPEG_HD inline int enc_chroma(const uint8_t* frame, const EncGeom& g, int c, int x, int y)
{
    const uint8_t* p = frame + (uint64_t)y * g.row_step + (uint64_t)x * 3u;
    return c == 1 ? enc_cb(p) : enc_cr(p);
}

// Sample (sx, sy) of component c as the FDCT sees it, any position of the MCU grid:
// the right edge is replicated in the input, the bottom row up to a multiple of the
// vertical factor, then the box filter runs, then the last filtered row is replicated.
JPEG_HD inline int enc_sample(const uint8_t* frame, const EncGeom& g, int c, int sx, int sy)
{
    const int xm = g.w - 1, ym = g.h - 1;
    if (c == 0) {
        const int x = sx < xm ? sx : xm, y = sy < ym ? sy : ym;
        if (g.channels == 1) return frame[(uint64_t)y * g.row_step + (uint64_t)x];
        return enc_y(frame + (uint64_t)y * g.row_step + (uint64_t)x * 3u);
    }
    if (g.hs == 1) {      // 4:4:4
        return enc_chroma(frame, g, c, sx < xm ? sx : xm, sy < ym ? sy : ym);
    }
    const int x0 = 2 * sx < xm ? 2 * sx : xm, x1 = 2 * sx + 1 < xm ? 2 * sx + 1 : xm;
    if (g.vs == 1) {      // h2v1: bias 0, 1, 0, 1 ...
        const int y = sy < ym ? sy : ym;
        return (enc_chroma(frame, g, c, x0, y) + enc_chroma(frame, g, c, x1, y) + (sx & 1)) >> 1;
    }
    const int rows = (g.h + 1) >> 1;      // h2v2: bias 1, 2, 1, 2 ...
    const int r = sy < rows - 1 ? sy : rows - 1;
    const int y0 = 2 * r, y1 = 2 * r + 1 < ym ? 2 * r + 1 : ym;
    return (enc_chroma(frame, g, c, x0, y0) + enc_chroma(frame, g, c, x1, y0) + enc_chroma(frame, g, c, x0, y1) +
            enc_chroma(frame, g, c, x1, y1) + 1 + (sx & 1)) >> 2;
}

// jpeg_fdct_islow, one pass over eight values in place.  last = false: the row pass
// (results scaled up by 2^PASS1_BITS); true: the column pass.
JPEG_HD inline int enc_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

JPEG_HD inline void enc_fdct_pass(int* d, bool last)
{
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int sh = last ? 15 : 11;
    if (last) {
        d[0] = enc_descale(t10 + t11, 2);
        d[4] = enc_descale(t10 - t11, 2);
    } else {
        d[0] = (t10 + t11) * 4;
        d[4] = (t10 - t11) * 4;
    }
    int z1 = (t12 + t13) * 4433;
    d[2] = enc_descale(z1 + t13 * 6270, sh);
    d[6] = enc_descale(z1 - t12 * 15137, sh);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 = -z1 * 7373;
    z2 = -z2 * 20995;
    z3 = -z3 * 16069 + z5;
    z4 = -z4 * 3196 + z5;
    d[7] = enc_descale(a4 + z1 + z3, sh);
    d[5] = enc_descale(a5 + z2 + z4, sh);
    d[3] = enc_descale(a6 + z2 + z3, sh);
    d[1] = enc_descale(a7 + z1 + z4, sh);
}

// jcdctmgr.c: divide by 8 q, rounding half away from zero
JPEG_HD inline int enc_quant(int t, int q)
{
    const int qq = 8 * q, a = t < 0 ? -t : t;
    const int v = (a + (qq >> 1)) / qq;
    return t < 0 ? -v : v;
}

// Block k of MCU (mx, my): its component, its block column and row, and whether the
// component's own grid holds it (else it is a dummy block).
JPEG_HD inline bool enc_block_pos(const EncGeom& g, int k, int mx, int my, int& c, int& col, int& row)
{
    const int nl = g.hs * g.vs;
    if (k < nl) {
        c = 0;
        col = mx * g.hs + k % g.hs;
        row = my * g.vs + k / g.hs;
    } else {
        c = k - nl + 1;
        col = mx;
        row = my;
    }
    if (c > 2) c = 2;      // k < bpm keeps it there
    return col < g.bw[c] && row < g.bh[c];
}

// Row j of block (col, row) of component c: samples - 128, after the row pass.
JPEG_HD inline void enc_block_row(const uint8_t* frame, const EncGeom& g, int c, int col, int row, int j, int* d)
{
    for (int i = 0; i < 8; i++) d[i] = enc_sample(frame, g, c, col * 8 + i, row * 8 + j) - 128;
    enc_fdct_pass(d, false);
}

// The whole block on one thread (the host encoder): 64 quantised coefficients in zigzag order.
JPEG_HD inline void enc_block_coef(const uint8_t* frame, const EncGeom& g, const EncTables& T, int c, int col, int row,
                                   int16_t* zz)
{
    int ws[64];
    for (int j = 0; j < 8; j++) enc_block_row(frame, g, c, col, row, j, ws + j * 8);
    const uint16_t* q = T.quant[c ? 1 : 0];
    int nat[64];
    for (int i = 0; i < 8; i++) {
        int d[8];
        for (int j = 0; j < 8; j++) d[j] = ws[j * 8 + i];
        enc_fdct_pass(d, true);
        for (int j = 0; j < 8; j++) nat[j * 8 + i] = enc_quant(d[j], q[j * 8 + i]);
    }
    for (int k = 0; k < 64; k++) zz[k] = (int16_t)nat[zigzag_natural(k)];
}

JPEG_HD inline int enc_nbits(int v)
{
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// One block through the Huffman coder: sink.put(code, length), length 1 .. 16.  t: table
// slot (0 luminance, 1 chrominance).  Returns the fault bits.
template <class Sink>
JPEG_HD inline int enc_block(Sink& s, const int16_t* zz, int pred, const EncTables& T, int t)
{
    int st = 0;
    const int diff = (int)zz[0] - pred;
    int nb = enc_nbits(diff);
    if (nb > 11) {
        nb = 11;
        st |= kEncCategory;
    }
    s.put(T.dc_code[t][nb], T.dc_len[t][nb]);
    if (nb) s.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u), nb);
    int run = 0;
    for (int k = 1; k < 64; k++) {
        const int v = zz[k];
        if (v == 0) {
            run++;
            continue;
        }
        if (run > 15) {      // at most three ZRL: run <= 62
            for (int z = 0; z < 3 && run > 15; z++, run -= 16) s.put(T.ac_code[t][0xF0], T.ac_len[t][0xF0]);
        }
        nb = enc_nbits(v);
        if (nb > 10) {
            nb = 10;
            st |= kEncCategory;
        }
        const int sym = ((run << 4) | nb) & 255;
        s.put(T.ac_code[t][sym], T.ac_len[t][sym]);
        s.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u), nb);
        run = 0;
    }
    if (run) s.put(T.ac_code[t][0], T.ac_len[t][0]);
    return st;
}

// A dummy block: the DC of the block before it (difference 0), no AC terms.
template <class Sink>
JPEG_HD inline void enc_dummy_block(Sink& s, const EncTables& T, int t)
{
    s.put(T.dc_code[t][0], T.dc_len[t][0]);
    s.put(T.ac_code[t][0], T.ac_len[t][0]);
}

struct EncCountSink {
    uint32_t bits = 0;
    JPEG_HD void put(uint32_t, int len) { bits += (uint32_t)len; }
};

// The blocks of MCU m, whose quantised coefficients are at coef (bpm blocks of 64, zigzag order; a
// dummy block's are not read), through the coder.  pred: the DC predictors on entry (zero at the
// start of a restart interval), updated.  Returns the fault bits.
template <class Sink>
JPEG_HD inline int enc_mcu(Sink& s, const EncGeom& g, const EncTables& T, uint32_t m, const int16_t* coef, int* pred)
{
    const int mx = (int)(m % (uint32_t)g.mcux), my = (int)(m / (uint32_t)g.mcux);
    int st = 0;
    for (int k = 0; k < g.bpm && k < 6; k++) {
        int c, col, row;
        const bool real = enc_block_pos(g, k, mx, my, c, col, row);
        const int t = c ? 1 : 0;
        if (!real) {
            enc_dummy_block(s, T, t);
            continue;
        }
        const int16_t* zz = coef + (size_t)k * 64;
        st |= enc_block(s, zz, pred[c], T, t);
        pred[c] = zz[0];
    }
    return st;
}

// The DC predictors with which MCU m starts: zero at the start of its restart interval, else the
// DC of each component's last real block of MCU m - 1 (block 0 of an MCU is always real).
JPEG_HD inline void enc_mcu_pred(const EncGeom& g, uint32_t m, const int16_t* coef_image, int* pred)
{
    pred[0] = pred[1] = pred[2] = 0;
    if (m % g.ri == 0) return;
    const uint32_t p = m - 1;
    const int mx = (int)(p % (uint32_t)g.mcux), my = (int)(p / (uint32_t)g.mcux);
    const int16_t* cf = coef_image + (uint64_t)p * (uint64_t)g.bpm * 64u;
    for (int k = 0; k < g.bpm && k < 6; k++) {
        int c, col, row;
        if (enc_block_pos(g, k, mx, my, c, col, row)) pred[c] = cf[(size_t)k * 64];
    }
}

}  // namespace jpeg

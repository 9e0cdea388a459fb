// Baseline JPEG entropy decoding (libjpeg's jdhuff.c restated), host and device,
// header only: the bit reader, the Huffman table build and lookup, and the
// decoding of one block and of one segment (a restart interval, or the whole scan
// of a stream without DRI).  jpeg.hip's jpeg_huff kernel and the host decoder
// (jpeg_parse.cpp) call the same functions; tests/cpp/jpeg_fuzz_test.cpp runs them
// under the address and undefined-behaviour sanitizers.
//
// Bounds.  The reader never touches a byte at or past the segment's end: past it
// it supplies zero bits and counts them.  Every table index is masked or checked
// (a lookahead index is 9 bits, a value index is tested against the 256 values,
// a coefficient index against 63), every loop has a fixed trip bound, and a
// segment decodes at most its own MCU count.  A stream of any content therefore
// reads only [off, end) of the byte buffer and writes only its own blocks.
//
// Faults (the per-image status bits): a segment that meets one stops; its
// remaining blocks keep the zeros the coefficient buffer was cleared to.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JPEG_HD __host__ __device__
#else
#define JPEG_HD
#endif

namespace jpeg {

constexpr int kStatusEof = 1;       // ran out of bytes: bits past the segment's end were consumed
constexpr int kStatusCode = 2;      // no such Huffman code
constexpr int kStatusRun = 4;       // a run went past coefficient 63
constexpr int kStatusRestart = 8;   // restart marker missing or out of sequence (set by the parser)

constexpr int kLookBits = 9;

// jpeg_natural_order: zigzag position -> natural (row-major) position
#define JPEG_ZIGZAG_INIT                                                                                 \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,              \
     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,              \
     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

JPEG_HD inline int zigzag_natural(int k)
{
    constexpr uint8_t t[64] = JPEG_ZIGZAG_INIT;
    return t[k & 63];
}

// One canonical Huffman table in the form both sides read (1424 bytes).
//   look[i]      for the 9 bits i: (length << 8) | symbol of the code that starts them, 0 when it is longer than 9
//   maxcode[l]   the largest code of length l (1 .. 16), -1 when there is none
//   valoff[l]    index of the first value of length l minus its first code
struct HuffTable {
    uint16_t look[1 << kLookBits];
    int32_t maxcode[17];
    int32_t valoff[17];
    uint8_t vals[256];
    int32_t defined;
};

// counts[0 .. 15]: codes of length 1 .. 16; vals: nvals symbols.  Returns false (table left
// undefined) when the counts exceed 256 symbols, differ from nvals or oversubscribe the code space.
inline bool huff_build(HuffTable& t, const uint8_t* counts, const uint8_t* vals, int nvals)
{
    t.defined = 0;
    int total = 0;
    for (int l = 0; l < 16; l++) total += counts[l];
    if (total > 256 || total != nvals) return false;
    for (int i = 0; i < (1 << kLookBits); i++) t.look[i] = 0;
    for (int i = 0; i < 256; i++) t.vals[i] = i < nvals ? vals[i] : 0;
    unsigned code = 0;
    int k = 0;
    t.maxcode[0] = -1;
    t.valoff[0] = 0;
    for (int l = 1; l <= 16; l++) {
        const int n = counts[l - 1];
        if (code + (unsigned)n > (1u << l)) return false;       // more codes than l bits hold
        t.valoff[l] = k - (int)code;
        for (int i = 0; i < n; i++, k++, code++) {
            if (l <= kLookBits) {
                const unsigned first = code << (kLookBits - l);
                for (unsigned j = 0; j < (1u << (kLookBits - l)); j++)
                    t.look[first + j] = (uint16_t)((l << 8) | t.vals[k]);
            }
        }
        t.maxcode[l] = n ? (int)code - 1 : -1;
        code <<= 1;
    }
    t.defined = 1;
    return true;
}

// MSB-first reader over [pos, end) of p.  FF 00 un-stuffs to FF; any other FF is
// taken as it stands (the parser cuts segments at the markers, so none is left
// inside one).  Past the end: zero bits, counted in pad.
struct BitReader {
    const uint8_t* p;
    uint32_t pos, end;
    uint32_t acc;      // the low n bits are unread
    int n;
    uint32_t pad;      // zero bits appended so far

    JPEG_HD void init(const uint8_t* base, uint32_t off, uint32_t stop)
    {
        p = base;
        pos = off;
        end = stop < off ? off : stop;
        acc = 0;
        n = 0;
        pad = 0;
    }
    JPEG_HD void fill()
    {
        while (n <= 24) {
            uint32_t b = 0;
            if (pos < end) {
                b = p[pos++];
                if (b == 0xFF && pos < end && p[pos] == 0) pos++;
            } else {
                pad += 8;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    // k in 0 .. 16; fill() first
    JPEG_HD uint32_t peek(int k) const { return (acc >> (n - k)) & ((1u << k) - 1u); }
    JPEG_HD void skip(int k) { n -= k; }
    // true once a bit that was never in the stream has been consumed
    JPEG_HD bool overrun() const { return pad > (uint32_t)n; }
};

// the next symbol, or -1 when the 16 bits ahead start no code
JPEG_HD inline int huff_decode(BitReader& br, const HuffTable& t)
{
    br.fill();
    const uint32_t b16 = br.peek(16);
    const uint32_t e = t.look[(b16 >> (16 - kLookBits)) & ((1u << kLookBits) - 1u)];
    if (e) {
        br.skip((int)(e >> 8));
        return (int)(e & 0xFF);
    }
    for (int l = kLookBits + 1; l <= 16; l++) {
        const int code = (int)(b16 >> (16 - l));
        if (code <= t.maxcode[l]) {
            const int idx = code + t.valoff[l];
            if (idx < 0 || idx > 255) return -1;
            br.skip(l);
            return t.vals[idx];
        }
    }
    return -1;
}

// jdhuff.c's HUFF_EXTEND
JPEG_HD inline int extend(int v, int t) { return v >= (1 << (t - 1)) ? v : v - (1 << t) + 1; }

// One block into out[64] (natural order; cleared by the caller, only non-zero
// coefficients are written).  pred: the component's DC predictor, kept modulo
// 2^32 so that a hostile stream overflows nothing.  zz: zigzag_natural's 64
// values (a copy in the caller's fastest memory: the lookup precedes every
// store).  Returns 0 or the fault bits.
JPEG_HD inline int decode_block(BitReader& br, const HuffTable& dc, const HuffTable& ac, const uint8_t* zz, uint32_t& pred,
                                int16_t* out)
{
    int t = huff_decode(br, dc);
    if (t < 0 || t > 16) return kStatusCode;
    if (t) {
        br.fill();
        const int v = (int)br.peek(t);
        br.skip(t);
        pred += (uint32_t)extend(v, t);
    }
    const int16_t d = (int16_t)(uint16_t)pred;
    if (d) out[0] = d;
    for (int k = 1; k < 64;) {
        const int rs = huff_decode(br, ac);
        if (rs < 0) return kStatusCode;
        const int r = rs >> 4, s = rs & 15;
        if (s == 0) {
            if (r != 15) break;      // EOB
            k += 16;                 // ZRL
            continue;
        }
        k += r;
        if (k > 63) return kStatusRun;
        br.fill();
        const int v = (int)br.peek(s);
        br.skip(s);
        out[zz[k & 63]] = (int16_t)extend(v, s);
        k++;
    }
    return br.overrun() ? kStatusEof : 0;
}

// What the entropy decoder needs of one scan component.
struct ScanComp {
    int32_t h, v;          // blocks per MCU across and down (1 x 1 for a one-component scan)
    int32_t bw, bh;        // the component's padded block grid
    int32_t dc, ac;        // Huffman table slots: tables[dc], tables[4 + ac]
    uint32_t coef_block;   // the component's first block in the image's coefficient area
};

// One image as the decoder sees it: 8 Huffman tables (DC 0 .. 3, AC 0 .. 3),
// the quantisation tables in natural order and the geometry.
struct ImageDesc {
    HuffTable tables[8];
    uint16_t quant[3][64];        // per component, natural order
    ScanComp comp[3];
    int32_t ncomp;
    int32_t width, height;
    int32_t mcus_x, mcus_y;
    int32_t sampling;             // SLAM_JPEG_* of include/slamhip.h
    int32_t out_channels;         // 1 or 3
    int32_t valid;                // 0: the frame is cleared instead of decoded
    uint32_t data_off;            // the stream's first byte in the batch's byte buffer
    uint32_t total_blocks;        // blocks of all components
    uint64_t coef_off;            // first coefficient (int16 index) in the batch's coefficient buffer
    uint64_t plane_off;           // first byte in the batch's component planes
    uint32_t plane_comp[3];       // ... and each component's plane after it
};

// One restart interval: bytes [off, end) of the image's stream, MCUs [mcu0, mcu0 + nmcu).
struct Segment {
    uint32_t image;
    uint32_t off, end;
    uint32_t mcu0, nmcu;
};

// Decodes one segment into coef (the image's coefficient area, cleared).  tables: the
// image's eight Huffman tables (im.tables, or a copy of them in faster memory);
// zz: zigzag_natural's 64 values.  The geometry is read once, ahead of the loop:
// nothing in it is fetched again per block.  Returns the fault bits.
JPEG_HD inline int decode_segment(const ImageDesc& im, const HuffTable* tables, const uint8_t* zz, const uint8_t* bytes,
                                  const Segment& sg, int16_t* coef)
{
    BitReader br;
    br.init(bytes, sg.off, sg.end);
    uint32_t pred[3] = {0, 0, 0};
    const int ncomp = im.ncomp, mcus_x = im.mcus_x;
    if (mcus_x < 1) return 0;
    const uint32_t total = (uint32_t)mcus_x * (uint32_t)im.mcus_y;
    const ScanComp sc0 = im.comp[0], sc1 = im.comp[1], sc2 = im.comp[2];
    int mx = (int)(sg.mcu0 % (uint32_t)mcus_x), my = (int)(sg.mcu0 / (uint32_t)mcus_x);
    for (uint32_t m = sg.mcu0, e = sg.mcu0 + sg.nmcu; m < e && m < total; m++) {
        for (int c = 0; c < ncomp && c < 3; c++) {
            const ScanComp sc = c == 0 ? sc0 : c == 1 ? sc1 : sc2;      // selects, not an indexed array
            const HuffTable& dc = tables[sc.dc & 3];
            const HuffTable& ac = tables[4 + (sc.ac & 3)];
            for (int by = 0; by < sc.v; by++)
                for (int bx = 0; bx < sc.h; bx++) {
                    const int row = my * sc.v + by, col = mx * sc.h + bx;
                    if (row >= sc.bh || col >= sc.bw) return kStatusRun;      // never: the grid is built from the MCUs
                    const uint32_t blk = sc.coef_block + (uint32_t)row * (uint32_t)sc.bw + (uint32_t)col;
                    const int st = decode_block(br, dc, ac, zz, pred[c], coef + (uint64_t)blk * 64u);
                    if (st) return st;
                }
        }
        if (++mx == mcus_x) {
            mx = 0;
            my++;
        }
    }
    return 0;
}

}  // namespace jpeg

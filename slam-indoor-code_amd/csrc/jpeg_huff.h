// Baseline JPEG entropy decoding (libjpeg's jdhuff.c restated), host and device,
// header only: the bit reader, the Huffman table build and lookup, and the
// decoding of one block and of one segment (a restart interval, or the whole scan
// of a stream without DRI), and the per-chunk steps of the chunk-parallel decoding
// of one segment (below).  jpeg.hip's kernels and the host decoders
// (jpeg_parse.cpp) call the same functions; tests/cpp/jpeg_fuzz_test.cpp and
// tests/cpp/mjpeg_fuzz_test.cpp run them under the address and undefined-behaviour
// sanitizers.
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

// the next symbol, or -1 when the 16 bits ahead start no code (Reader: BitReader or PosReader)
template <class Reader>
JPEG_HD inline int huff_decode(Reader& br, const HuffTable& t)
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

// ---- chunk-parallel decoding of one segment ---------------
//
// A faster way to decode_segment's bytes, after Weissenberger & Schmidt's
// self-synchronising decoder; never a second definition: a segment is accepted only
// when the chain of states below is proven from the segment's true start and every
// block was decoded by decode_block without a fault, and is otherwise decoded by
// decode_segment itself.
//
// The segment's bytes [off, end) are cut into chunks of C bytes; one lane owns one
// chunk and the symbols that START in it.  A state is a symbol boundary: (byte, bit)
// of the next unread bit in the raw stream, the block index inside the MCU and the
// zigzag position k (0: a DC symbol comes next).  sync_walk decodes from an entry
// state to the first boundary at or past the chunk's limit and returns that exit
// state; a lane's entry is its predecessor's exit, or the cold state (chunk start,
// block 0, k 0) while that is unknown.  The rounds that repeat this until nothing
// changes are the callers' (jpeg.hip's jpeg_sync kernel and jpeg_parse.cpp's host
// driver, the same structure); sync_walk with a ChunkCount then verifies the chain
// (entry = the stored exit of the predecessor, recomputed exit = the stored one) and
// counts the blocks started and their DC differences per component, modulo 2^32; an
// exclusive scan gives each chunk its first block index and predictors, and
// sync_write decodes the chunk's blocks with decode_block into decode_segment's layout.
//
// Bounds: every walk is limited to max_steps symbols (a symbol is at least one bit),
// the readers never touch a byte at or past the segment's end, and sync_write
// writes only blocks below the segment's block count, at addresses checked against
// the component's grid.
constexpr int kSyncLanes = 256;          // chunks of one workgroup (and of the host driver's)
constexpr int kSyncLaunches = 4;         // rounds between workgroups: one cold launch and three that pass states on
constexpr int kSyncChunkMin = 16, kSyncChunkMax = 1024;
constexpr uint64_t kStateUnknown = ~0ull;          // a fault met while speculating: the successor starts cold
constexpr uint64_t kStateEnd = ~0ull - 1;          // the segment's bytes are used up: the successors have nothing to do
constexpr uint32_t kChunkFault = 1;      // a fault of the stream itself (met in the verified chain or by decode_block)
constexpr uint32_t kChunkMismatch = 2;   // the recomputed exit state is not the stored one

JPEG_HD inline uint64_t state_pack(uint32_t byte, int bit, int blk, int k)
{
    return ((uint64_t)byte << 32) | ((uint64_t)(bit & 7) << 16) | ((uint64_t)(blk & 255) << 8) | (uint64_t)(k & 255);
}

// BitReader that also knows where in the raw stream its next unread bit lies.
// stuff: bit i set when the i-th most recently loaded byte was followed by a skipped 00.
struct PosReader {
    const uint8_t* p;
    uint32_t pos, end;
    uint32_t acc;
    int n;
    uint32_t pad;
    uint32_t stuff;

    JPEG_HD void init(const uint8_t* base, uint32_t off, uint32_t stop)
    {
        p = base;
        pos = off;
        end = stop < off ? off : stop;
        acc = 0;
        n = 0;
        pad = 0;
        stuff = 0;
    }
    JPEG_HD void fill()
    {
        while (n <= 24) {
            uint32_t b = 0, st = 0;
            if (pos < end) {
                b = p[pos++];
                if (b == 0xFF && pos < end && p[pos] == 0) {
                    pos++;
                    st = 1;
                }
            } else {
                pad += 8;
            }
            acc = (acc << 8) | b;
            stuff = (stuff << 1) | st;
            n += 8;
        }
    }
    JPEG_HD uint32_t peek(int k) const { return (acc >> (n - k)) & ((1u << k) - 1u); }
    JPEG_HD void skip(int k) { n -= k; }
    JPEG_HD bool overrun() const { return pad > (uint32_t)n; }
    // fewer than 16 bits of the stream are left unread
    JPEG_HD bool near_end() const { return pos >= end && n - (int)pad < 16; }
    // the raw byte that holds the next unread bit, and the bit's index in it (0 = the top bit); not after an overrun
    JPEG_HD void position(uint32_t& byte, int& bit) const
    {
        const int real = n - (int)pad;                 // unread bits that came from the stream
        const int nb = (real + 7) >> 3;                // the loaded bytes they lie in (at most 4)
        const uint32_t m = (stuff >> (pad >> 3)) & ((1u << nb) - 1u);
        int skipped = 0;
        for (int i = 0; i < 4; i++) skipped += (int)((m >> i) & 1u);
        byte = pos - (uint32_t)nb - (uint32_t)skipped;
        bit = (8 - (real & 7)) & 7;
    }
};

// One segment that takes the parallel path, as both sides read it.
struct SyncSeg {
    uint32_t image;
    uint32_t off, end;       // its bytes in the byte buffer
    uint32_t mcu0;
    uint32_t nblocks;        // the blocks decode_segment decodes
    uint32_t nchunks;
    uint32_t chunk0;         // its first chunk slot: a multiple of kSyncLanes
    uint32_t bpm;            // blocks per MCU (at most 10)
    uint64_t blkinfo;        // 6 bits per block of an MCU: component | DC slot << 2 | AC slot << 4
};

// What the verified walk of one chunk found.
struct ChunkCount {
    uint32_t nstart;         // blocks whose DC symbol starts in the chunk
    uint32_t dc0, dc1, dc2;  // the sum of their DC differences per component, modulo 2^32
    uint64_t first;          // the state at the first of them
    uint32_t flags;          // kChunk*
};

JPEG_HD inline uint32_t seg_blocks_per_mcu(const ImageDesc& im)
{
    uint32_t n = 0;
    for (int c = 0; c < im.ncomp && c < 3; c++) n += (uint32_t)(im.comp[c].h * im.comp[c].v);
    return n;
}

// fills everything but chunk0; false when the segment cannot take the parallel path
inline bool sync_seg_init(SyncSeg& s, const ImageDesc& im, const Segment& sg, uint32_t chunk_bytes)
{
    const uint32_t bpm = seg_blocks_per_mcu(im);
    if (im.mcus_x < 1 || bpm < 1 || bpm > 10 || sg.end <= sg.off) return false;
    const uint64_t total = (uint64_t)im.mcus_x * (uint64_t)im.mcus_y;
    if (sg.mcu0 >= total) return false;
    const uint64_t nm = total - sg.mcu0 < sg.nmcu ? total - sg.mcu0 : sg.nmcu;
    if (nm * bpm > 0x7FFFFFFFull) return false;
    s.image = sg.image;
    s.off = sg.off;
    s.end = sg.end;
    s.mcu0 = sg.mcu0;
    s.nblocks = (uint32_t)(nm * bpm);
    s.nchunks = (sg.end - sg.off + chunk_bytes - 1) / chunk_bytes;
    s.chunk0 = 0;
    s.bpm = bpm;
    s.blkinfo = 0;
    int b = 0;
    for (int c = 0; c < im.ncomp && c < 3; c++)
        for (int i = 0; i < im.comp[c].h * im.comp[c].v; i++, b++)
            s.blkinfo |= (uint64_t)((uint32_t)c | ((uint32_t)(im.comp[c].dc & 3) << 2) | ((uint32_t)(im.comp[c].ac & 3) << 4)) << (6 * b);
    return true;
}

// the cold state of chunk ci: its first byte, or the byte after it when that is the 00 of an FF 00 pair
JPEG_HD inline uint64_t sync_cold(const uint8_t* bytes, const SyncSeg& sg, uint32_t ci, uint32_t chunk_bytes)
{
    uint32_t b = sg.off + ci * chunk_bytes;
    if (ci && bytes[b] == 0 && bytes[b - 1] == 0xFF) b++;
    return state_pack(b, 0, 0, 0);
}

// the entry state of a chunk whose predecessor left `prev`
JPEG_HD inline uint64_t sync_entry(uint64_t prev, uint64_t cold) { return prev == kStateUnknown ? cold : prev; }

// Decodes, without writing, the symbols that start at or after `entry` and before byte `limit`.
// Returns the exit state.  cc (nullable): counts the blocks started; a fault sets kChunkFault there
// unless fewer than 16 bits of the segment are left (the padding after the last block, which
// decode_segment never reads; what it does read is decoded again by sync_write).
JPEG_HD inline uint64_t sync_walk(const HuffTable* tables, const uint8_t* bytes, const SyncSeg& sg, uint64_t entry,
                                  uint32_t limit, uint32_t max_steps, ChunkCount* cc)
{
    if (cc) {
        cc->nstart = cc->dc0 = cc->dc1 = cc->dc2 = 0;
        cc->first = 0;
        cc->flags = 0;
    }
    if (entry == kStateEnd || entry == kStateUnknown) return entry;
    uint32_t byte = (uint32_t)(entry >> 32);
    int bit = (int)(entry >> 16) & 7, blk = (int)(entry >> 8) & 255, k = (int)entry & 255;
    if (byte >= limit) return entry;
    if (byte < sg.off || blk >= (int)sg.bpm || k > 63) return kStateUnknown;      // never: states are made here
    PosReader br;
    br.init(bytes, byte, sg.end);
    br.fill();
    br.skip(bit);
    for (uint32_t step = 0; step < max_steps; step++) {
        br.fill();
        br.position(byte, bit);
        if (byte >= limit) return state_pack(byte, bit, blk, k);
        const uint32_t info = (uint32_t)(sg.blkinfo >> (6 * blk)) & 63u;
        bool fault = false;
        if (k == 0) {
            const int t = huff_decode(br, tables[(info >> 2) & 3]);
            int diff = 0;
            if (t < 0 || t > 16) {
                fault = true;
            } else if (t) {
                br.fill();
                diff = extend((int)br.peek(t), t);
                br.skip(t);
            }
            if (!fault) {
                if (br.overrun()) return kStateEnd;
                if (cc) {
                    if (!cc->nstart) cc->first = state_pack(byte, bit, blk, 0);
                    cc->nstart++;
                    const uint32_t c = info & 3u;
                    cc->dc0 += c == 0 ? (uint32_t)diff : 0u;
                    cc->dc1 += c == 1 ? (uint32_t)diff : 0u;
                    cc->dc2 += c == 2 ? (uint32_t)diff : 0u;
                }
                k = 1;
            }
        } else {
            const int rs = huff_decode(br, tables[4 + ((info >> 4) & 3)]);
            if (rs < 0) {
                fault = true;
            } else {
                const int r = rs >> 4, s = rs & 15;
                if (s == 0) {
                    k = r != 15 ? 64 : k + 16;
                } else {
                    k += r;
                    if (k > 63) {
                        fault = true;
                    } else {
                        br.fill();
                        br.skip(s);
                        k++;
                    }
                }
            }
            if (!fault && br.overrun()) return kStateEnd;
        }
        if (fault) {
            if (br.overrun() || br.near_end()) return kStateEnd;
            if (cc) cc->flags |= kChunkFault;
            return kStateUnknown;
        }
        if (k >= 64) {
            k = 0;
            blk = blk + 1 == (int)sg.bpm ? 0 : blk + 1;
        }
    }
    return kStateUnknown;      // never: max_steps covers the chunk's bits
}

// symbols a walk of one chunk can take: a symbol is at least one bit, and an entry lies less than 16 bytes past the start
JPEG_HD inline uint32_t sync_max_steps(uint32_t chunk_bytes) { return chunk_bytes * 8u + 160u; }

// the coefficient block of block j of a segment that starts at MCU mcu0 (decode_segment's arithmetic); false: outside the grid
JPEG_HD inline bool seg_block_addr(const ImageDesc& im, uint32_t mcu0, uint32_t bpm, uint32_t j, uint32_t& blk, int& comp)
{
    const uint32_t m = mcu0 + j / bpm;
    uint32_t i = j % bpm;
    const uint32_t mx = m % (uint32_t)im.mcus_x, my = m / (uint32_t)im.mcus_x;
    for (int c = 0; c < im.ncomp && c < 3; c++) {
        const ScanComp sc = c == 0 ? im.comp[0] : c == 1 ? im.comp[1] : im.comp[2];
        const uint32_t n = (uint32_t)(sc.h * sc.v);
        if (i < n) {
            const uint32_t row = my * (uint32_t)sc.v + i / (uint32_t)sc.h, col = mx * (uint32_t)sc.h + i % (uint32_t)sc.h;
            if (row >= (uint32_t)sc.bh || col >= (uint32_t)sc.bw) return false;
            blk = sc.coef_block + row * (uint32_t)sc.bw + col;
            comp = c;
            return true;
        }
        i -= n;
    }
    return false;
}

// Decodes the cc.nstart blocks that start in a chunk with decode_block, from the state cc.first,
// block index j0 of the segment and the three predictors, into coef (the image's coefficient
// area).  Blocks at or past sg.nblocks are not decoded.  Returns the fault bits (kStatus*).
JPEG_HD inline int sync_write(const ImageDesc& im, const HuffTable* tables, const uint8_t* zz, const uint8_t* bytes,
                              const SyncSeg& sg, const ChunkCount& cc, uint32_t j0, uint32_t p0, uint32_t p1, uint32_t p2,
                              int16_t* coef)
{
    if (!cc.nstart || j0 >= sg.nblocks) return 0;
    BitReader br;
    br.init(bytes, (uint32_t)(cc.first >> 32), sg.end);
    br.fill();
    br.skip((int)(cc.first >> 16) & 7);
    for (uint32_t i = 0, j = j0; i < cc.nstart && j < sg.nblocks; i++, j++) {
        uint32_t blk = 0;
        int c = 0;
        if (!seg_block_addr(im, sg.mcu0, sg.bpm, j, blk, c)) return kStatusRun;      // never: the grid is built from the MCUs
        const uint32_t info = (uint32_t)(sg.blkinfo >> (6 * (j % sg.bpm))) & 63u;
        uint32_t pred = c == 0 ? p0 : c == 1 ? p1 : p2;
        const int st = decode_block(br, tables[(info >> 2) & 3], tables[4 + ((info >> 4) & 3)], zz, pred, coef + (uint64_t)blk * 64u);
        if (st) return st;
        if (c == 0) p0 = pred;
        else if (c == 1) p1 = pred;
        else p2 = pred;
    }
    return 0;
}

}  // namespace jpeg

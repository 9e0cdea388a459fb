// The JPEG decoder's host side (jpeg_parse.cpp): marker parsing and validation,
// the segment table, and the whole decoder on the host over jpeg_huff.h /
// jpeg_pix.h.  No HIP: tests/cpp/jpeg_fuzz_test.cpp links jpeg_parse.cpp alone.
#pragma once

#include <string>
#include <vector>

#include "jpeg_huff.h"
#include "jpeg_pix.h"

namespace jpeg {

constexpr int kMaxDim = 16384;

// One output pixel from the component planes (`planes`: the image's plane area):
// out_channels bytes at dst.
JPEG_HD inline void emit_pixel(const ImageDesc& im, const uint8_t* planes, int x, int y, uint8_t* dst)
{
    const int yp = im.comp[0].bw * 8;
    const int lum = planes[im.plane_comp[0] + (size_t)y * yp + x];
    if (im.out_channels == 1) {
        dst[0] = (uint8_t)lum;
        return;
    }
    if (im.ncomp == 1) {
        dst[0] = dst[1] = dst[2] = (uint8_t)lum;
        return;
    }
    const int hmax = im.comp[0].h, vmax = im.comp[0].v;
    const int cw = (im.width + hmax - 1) / hmax, ch = (im.height + vmax - 1) / vmax;
    const int cp = im.comp[1].bw * 8;
    const int cb = chroma_sample(planes + im.plane_comp[1], cp, cw, ch, im.sampling, x, y);
    const int cr = chroma_sample(planes + im.plane_comp[2], cp, cw, ch, im.sampling, x, y);
    ycc_to_bgr(lum, cb, cr, dst);
}

struct Parsed {
    ImageDesc d;                  // data_off 0, coef_off 0, plane_off 0: one image on its own
    std::vector<Segment> segs;    // offsets relative to the stream's first byte; image 0
    int restart = 0;
    int orientation = 1;
    int status0 = 0;              // kStatusRestart when the markers found are not the ones expected
    size_t plane_bytes = 0;       // all component planes
};

// Parses and validates a stream.  channels: 1 or 3 (the output wanted).  flags:
// SLAM_JPEG_MJPEG = the two rules of Motion-JPEG frames (the Annex K tables for the
// undefined Huffman slots 0 and 1; an AVI1 APP0 that marks one field of an interlaced
// pair is refused).  Returns a SLAM_* code; msg names the cause of a failure.
int parse(const uint8_t* buf, size_t len, int channels, Parsed& P, std::string& msg, int flags = 0);

// The Annex K Huffman table of a class (0 DC, 1 AC) and slot (0 luminance, 1 chrominance):
// counts[16], the values and their number.
void std_huff_table(int klass, int slot, const uint8_t** counts, const uint8_t** vals, int* nvals);

// What the chunk-parallel path did (slam_jpeg_sync_stats without the timings).
struct SyncTotals {
    int32_t parallel = 0, fallback = 0;
    int64_t chunks = 0;
    int32_t wg_rounds_max = 0, launch_rounds_max = 0;
    int64_t wg_rounds_total = 0, launch_rounds_total = 0;
};

// chunk bytes for an option value: 0 = the default; a power of two in 16 .. 1024, else 0
uint32_t sync_chunk_bytes(int value);
constexpr uint32_t kSyncChunkDefault = 256;
constexpr uint32_t kSyncAutoBytes = 16384;       // SLAM_OPT_JPEG_SYNC = 1: segments of at least this many bytes

// Decodes the parallel segments `segs` of one image on the host in the kernels' round structure
// (kSyncLanes chunks per workgroup, kSyncLaunches rounds between workgroups) into coef, which is
// cleared where those segments write; a segment that is not accepted is cleared again and decoded
// by decode_segment.  Returns the fault bits of the segments that fell back.
int sync_decode_host(const ImageDesc& d, const uint8_t* bytes, const std::vector<SyncSeg>& segs, uint32_t chunk_bytes,
                     int16_t* coef, SyncTotals& T);

}  // namespace jpeg

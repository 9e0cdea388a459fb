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

// Parses and validates a stream.  channels: 1 or 3 (the output wanted).  Returns a
// SLAM_* code; msg names the cause of a failure.
int parse(const uint8_t* buf, size_t len, int channels, Parsed& P, std::string& msg);

}  // namespace jpeg

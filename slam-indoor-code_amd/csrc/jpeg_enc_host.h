// The JPEG encoder's host side (jpeg_enc_host.cpp): argument checks, geometry,
// tables and markers, and the whole encoder on the host over jpeg_enc_math.h.  No
// HIP: tests/cpp/jpeg_enc_test.cpp links jpeg_enc_host.cpp and jpeg_parse.cpp alone.
#pragma once

#include <stddef.h>

#include <string>

#include "jpeg_enc_math.h"

namespace jpeg {

// Checks the arguments of an encode and fills the geometry and the tables.  A one-channel
// frame is written as a gray stream whatever the sampling.  Returns a SLAM_* code.
int enc_setup(int h, int w, int channels, size_t row_step, size_t frame_step, int quality, int sampling,
              int restart_interval, EncGeom& g, EncTables& T, std::string& msg);

// SOI .. SOS into out (kEncHeaderMax bytes of room); returns the length.
size_t enc_header(const EncGeom& g, const EncTables& T, int restart_interval, uint8_t* out);

// What no stream of this geometry can exceed (slam_jpeg_encode_bound).
size_t enc_bound(const EncGeom& g);

}  // namespace jpeg

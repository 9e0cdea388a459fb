// The Motion-JPEG AVI container (avi_parse.cpp): a bounds-checked walk over the RIFF
// chunks of a file held in memory.  Plain C++, no HIP: tests/cpp/mjpeg_fuzz_test.cpp
// links it under the sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/slamhip.h"

namespace avi {

constexpr int kMaxDepth = 8;      // LIST rec inside LIST movi: deeper nesting is refused

struct Frame {
    uint64_t off, size;
};

// Walks buf; frames: the video chunks in file order.  Returns a SLAM_* code; msg names the cause of a failure.
int index(const uint8_t* buf, size_t len, slam_avi_info& info, std::vector<Frame>& frames, std::string& msg);

}  // namespace avi

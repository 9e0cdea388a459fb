// The host JPEG encoder (jpeg_enc_host.cpp over jpeg_enc_math.h, the arithmetic the
// kernels of jpeg_enc.hip share) under the sanitizers: a stand-alone program, linked
// with jpeg_enc_host.cpp and jpeg_parse.cpp alone.
//
//   jpeg_enc_test <random images> <file.raw> ...
//
// A raw file is two little-endian int32 (height, width) and the h x w x 3 BGR bytes.
// Every image, and <random images> fixed-seed ones of 1 .. 40 pixels a side, is
// encoded in every sampling (and as gray), at qualities 5, 75 and 100 and restart
// intervals 0, 1 and 3: once to learn the size, once into a heap buffer of exactly
// that size, once into one that is a byte short.  The buffers are exact heap
// allocations, so a byte written past a capacity is an AddressSanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/slamhip.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}

static long g_encodes = 0;

static int fail(const char* what, int h, int w, int sampling, int q, int ri)
{
    std::fprintf(stderr, "FAIL %s: %d x %d sampling %#x quality %d restart %d\n", what, h, w, sampling, q, ri);
    return 1;
}

static int run(const uint8_t* img, int h, int w, int channels)
{
    const int samplings[4] = {SLAM_JPEG_444, SLAM_JPEG_422, SLAM_JPEG_420, SLAM_JPEG_GRAY};
    const int quals[3] = {5, 75, 100}, rst[3] = {0, 1, 3};
    const size_t step = (size_t)w * channels;
    for (int s = 0; s < (channels == 1 ? 1 : 4); s++)
        for (int q : quals)
            for (int ri : rst) {
                const int smp = channels == 1 ? SLAM_JPEG_GRAY : samplings[s];
                size_t need = 0, got = 0;
                int st = 0;
                if (slam_jpeg_encode_host(img, h, w, channels, step, q, smp, ri, nullptr, 0, &need, &st) != SLAM_OK)
                    return fail("size query", h, w, smp, q, ri);
                if (need < 100 || !(st & SLAM_JPEG_ENC_OVERFLOW) || (st & SLAM_JPEG_ENC_CATEGORY)) return fail("size query status", h, w, smp, q, ri);
                if (need > slam_jpeg_encode_bound(h, w, smp, ri)) return fail("bound", h, w, smp, q, ri);
                uint8_t* exact = static_cast<uint8_t*>(std::malloc(need));
                uint8_t* shorter = static_cast<uint8_t*>(std::malloc(need - 1));
                if (!exact || !shorter) return fail("malloc", h, w, smp, q, ri);
                if (slam_jpeg_encode_host(img, h, w, channels, step, q, smp, ri, exact, need, &got, &st) != SLAM_OK || got != need || st)
                    return fail("exact buffer", h, w, smp, q, ri);
                if (exact[0] != 0xFF || exact[1] != 0xD8 || exact[need - 2] != 0xFF || exact[need - 1] != 0xD9)
                    return fail("SOI / EOI", h, w, smp, q, ri);
                if (slam_jpeg_encode_host(img, h, w, channels, step, q, smp, ri, shorter, need - 1, &got, &st) != SLAM_OK ||
                    got != need || st != SLAM_JPEG_ENC_OVERFLOW)
                    return fail("short buffer", h, w, smp, q, ri);
                if (std::memcmp(exact, shorter, need - 1) != 0) return fail("short buffer prefix", h, w, smp, q, ri);
                std::free(exact);
                std::free(shorter);
                g_encodes += 3;
            }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: jpeg_enc_test <random images> [file.raw ...]\n");
        return 2;
    }
    const int nrand = std::atoi(argv[1]);
    for (int a = 2; a < argc; a++) {
        FILE* f = std::fopen(argv[a], "rb");
        int32_t hw[2];
        if (!f || std::fread(hw, 4, 2, f) != 2 || hw[0] < 1 || hw[1] < 1 || hw[0] > 4096 || hw[1] > 4096) {
            std::fprintf(stderr, "cannot read %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> px((size_t)hw[0] * hw[1] * 3);
        if (std::fread(px.data(), 1, px.size(), f) != px.size()) {
            std::fprintf(stderr, "short file %s\n", argv[a]);
            return 2;
        }
        std::fclose(f);
        if (hw[0] > 64) {      // the large source: one sampling's worth is enough under the sanitizers
            std::vector<uint8_t> g((size_t)hw[0] * hw[1]);
            for (size_t i = 0; i < g.size(); i++) g[i] = px[i * 3 + 1];
            if (run(g.data(), hw[0], hw[1], 1)) return 1;
            continue;
        }
        if (run(px.data(), hw[0], hw[1], 3)) return 1;
    }
    for (int k = 0; k < nrand; k++) {
        const int h = 1 + (int)(rnd() % 40), w = 1 + (int)(rnd() % 40), channels = (k & 3) == 3 ? 1 : 3;
        // exact allocation: a read past the frame is a report too
        uint8_t* px = static_cast<uint8_t*>(std::malloc((size_t)h * w * channels));
        const uint32_t mode = rnd() % 3;
        for (size_t i = 0; i < (size_t)h * w * channels; i++) px[i] = mode == 0 ? (uint8_t)rnd() : mode == 1 ? (uint8_t)((rnd() & 1) * 255) : (uint8_t)(i * 3);
        const int rc = run(px, h, w, channels);
        std::free(px);
        if (rc) return 1;
    }
    // refused arguments leave the outputs alone
    size_t n = 7;
    uint8_t one[3] = {1, 2, 3};
    if (slam_jpeg_encode_host(one, 0, 1, 3, 3, 90, SLAM_JPEG_420, 0, nullptr, 0, &n, nullptr) == SLAM_OK) return fail("h = 0 accepted", 0, 1, 0, 0, 0);
    if (slam_jpeg_encode_host(one, 1, 1, 2, 3, 90, SLAM_JPEG_420, 0, nullptr, 0, &n, nullptr) == SLAM_OK) return fail("2 channels accepted", 1, 1, 0, 0, 0);
    if (slam_jpeg_encode_host(one, 1, 1, 3, 2, 90, SLAM_JPEG_420, 0, nullptr, 0, &n, nullptr) == SLAM_OK) return fail("short step accepted", 1, 1, 0, 0, 0);
    std::printf("%ld encodes clean\n", g_encodes);
    return 0;
}

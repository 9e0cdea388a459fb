// The JPEG decoder's shared code (slam-indoor-code_amd/csrc/jpeg_huff.h, jpeg_pix.h,
// jpeg_parse.cpp: the functions the kernels of jpeg.hip call) over the committed
// fixtures and a fixed-seed set of mutated copies of them.  tests/test_jpeg.py
// builds this with -fsanitize=address,undefined -fno-sanitize-recover=all: a read or
// write out of bounds, or undefined arithmetic, on any of these streams ends the
// program.  The output buffer is allocated at exactly the size slam_jpeg_info
// reports, so a write past a frame is a heap overflow the sanitizer sees.
//
//   jpeg_fuzz_test <mutations per stream> <file.jpg> ...
//
// prints one line per file (return code, status) and a summary of the mutated runs.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/slamhip.h"

namespace {

struct Rng {      // xorshift64*
    uint64_t s;
    uint64_t next()
    {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 2685821237402637421ull;
    }
    size_t below(size_t n) { return n ? (size_t)(next() % n) : 0; }
};

constexpr int64_t kMaxPixels = 1 << 22;      // mutated headers may claim 16384 x 16384: those are parsed, not decoded

// returns the decode's return code; *status as the decoder leaves it
int decode(const std::vector<uint8_t>& d, int channels, int* status, uint64_t* sum, bool limit)
{
    struct slam_jpeg_info info;
    *status = 0;
    const int rc = slam_jpeg_info(d.data(), d.size(), &info);
    if (rc != SLAM_OK) {
        if (rc != SLAM_E_INVALID_ARG && rc != SLAM_E_UNSUPPORTED) std::abort();
        if (!slam_jpeg_last_error()[0]) std::abort();      // every refusal names its cause
        return rc;
    }
    if (limit && (int64_t)info.width * info.height > kMaxPixels) return 1;
    std::vector<uint8_t> out((size_t)info.width * info.height * channels);
    const int rc2 = slam_jpeg_decode_host(d.data(), d.size(), out.data(), (size_t)info.width * channels, channels, status);
    if (rc2 != SLAM_OK) std::abort();      // what slam_jpeg_info takes, the decoder takes
    if (*status < 0 || *status > 15) std::abort();
    for (uint8_t v : out) *sum = *sum * 1099511628211ull + v;
    return rc2;
}

std::vector<uint8_t> mutate(const std::vector<uint8_t>& src, Rng& r)
{
    std::vector<uint8_t> d = src;
    static const uint8_t markers[] = {0xD0, 0xD3, 0xD7, 0xD9, 0xDA, 0xC4, 0xDB, 0xDD, 0xC0, 0xC2, 0x00, 0xFF};
    const int kind = (int)r.below(6);
    const int reps = 1 + (int)r.below(4);
    for (int k = 0; k < reps && !d.empty(); k++) {
        switch (kind) {
        case 0:      // byte flips anywhere
            d[r.below(d.size())] ^= (uint8_t)(1u << r.below(8));
            break;
        case 1:      // random bytes in the second half (mostly the scan)
            d[d.size() / 2 + r.below(d.size() - d.size() / 2)] = (uint8_t)r.next();
            break;
        case 2:      // truncation
            d.resize(r.below(d.size()) + 1);
            break;
        case 3: {    // a marker spliced over two bytes
            if (d.size() < 4) break;
            const size_t p = 2 + r.below(d.size() - 3);
            d[p] = 0xFF;
            d[p + 1] = markers[r.below(sizeof(markers))];
            break;
        }
        case 4: {    // a run of bytes removed
            if (d.size() < 16) break;
            const size_t p = r.below(d.size() - 8), n = 1 + r.below(8);
            d.erase(d.begin() + (long)p, d.begin() + (long)(p + n));
            break;
        }
        default: {   // a header byte rewritten (the first 700 bytes hold the tables and the frame)
            const size_t lim = d.size() < 700 ? d.size() : 700;
            d[r.below(lim)] = (uint8_t)r.next();
            break;
        }
        }
    }
    return d;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const int per = std::atoi(argv[1]);
    Rng rng{0x9E3779B97F4A7C15ull};
    long runs = 0, refused = 0, flagged = 0, clean = 0, skipped = 0;
    uint64_t sum = 14695981039346656037ull;
    for (int a = 2; a < argc; a++) {
        FILE* f = std::fopen(argv[a], "rb");
        if (!f) return 3;
        std::vector<uint8_t> d;
        uint8_t buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) d.insert(d.end(), buf, buf + n);
        std::fclose(f);
        int st = 0;
        const char* name = std::strrchr(argv[a], '/');
        const int rc = decode(d, 3, &st, &sum, false);
        int st1 = 0;
        decode(d, 1, &st1, &sum, false);
        std::printf("%s %d %d\n", name ? name + 1 : argv[a], rc, st);
        // large streams get fewer mutations: the run is meant to take seconds
        const int m = d.size() > 20000 ? per / 50 : per;
        for (int k = 0; k < m; k++) {
            const std::vector<uint8_t> x = mutate(d, rng);
            const int r = decode(x, (k & 1) ? 1 : 3, &st, &sum, true);
            runs++;
            if (r < 0) refused++;
            else if (r == 1) skipped++;
            else if (st) flagged++;
            else clean++;
        }
    }
    std::printf("mutated %ld refused %ld flagged %ld clean %ld skipped %ld sum %016llx\n", runs, refused, flagged, clean,
                skipped, (unsigned long long)sum);
    return 0;
}

// The host driver of the chunk-parallel entropy decoder (slam_jpeg_decode_host_sync: the
// functions of jpeg_huff.h that the kernels of jpeg.hip call, in their round structure) and
// the AVI walker (slam_avi_index) over fixtures and fixed-seed mutated copies of them.
// tests/test_mjpeg.py builds this with -fsanitize=address,undefined
// -fno-sanitize-recover=all: a read or write out of bounds, or undefined arithmetic, ends
// the program.  Streams and containers are handed over in buffers of exactly their size,
// and frames are decoded into buffers of exactly the size slam_jpeg_info_ex reports.
// Wherever the serial decoder decodes, the parallel path must give its pixels and status:
// the program aborts otherwise.
//
//   mjpeg_fuzz_test <mutations per stream> <file.avi | file.jpg> ...
//
// prints a summary line.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

long g_parallel = 0, g_fellback = 0, g_refused = 0, g_decoded = 0;

void die(const char* what)
{
    std::fprintf(stderr, "mjpeg_fuzz_test: %s\n", what);
    std::abort();
}

// one stream through the serial decoder and the parallel path at one chunk size; limit: skip huge claimed frames
void both(const std::vector<uint8_t>& src, int flags, int chunk, bool limit)
{
    std::vector<uint8_t> d(src);      // exactly the stream's size on the heap
    struct slam_jpeg_info info;
    const int rc = slam_jpeg_info_ex(d.data(), d.size(), &info, flags);
    if (rc != SLAM_OK) {
        if (rc != SLAM_E_INVALID_ARG && rc != SLAM_E_UNSUPPORTED) die("unknown refusal code");
        if (!slam_jpeg_last_error()[0]) die("a refusal without a message");
        g_refused++;
        return;
    }
    if (limit && (int64_t)info.width * info.height > kMaxPixels) return;
    const size_t row = (size_t)info.width * 3;
    std::vector<uint8_t> a(row * info.height, 0x11), b(row * info.height, 0x22);
    int sa = 0, sb = 0;
    struct slam_jpeg_sync_stats st;
    if (slam_jpeg_decode_host_ex(d.data(), d.size(), a.data(), row, 3, flags, &sa) != SLAM_OK) die("serial decoder refused what info took");
    if (slam_jpeg_decode_host_sync(d.data(), d.size(), b.data(), row, 3, chunk, flags, &sb, &st) != SLAM_OK)
        die("parallel path refused what info took");
    if (sa != sb) die("status differs between the serial decoder and the parallel path");
    if (a != b) die("pixels differ between the serial decoder and the parallel path");
    if (st.fallback_segments < 0 || st.fallback_segments > st.parallel_segments || st.chunk_bytes != chunk) die("statistics out of range");
    if (st.launch_rounds_max > 4 || st.wg_rounds_max > st.lanes + 1) die("a round bound was passed");
    if ((sa & 7) && st.parallel_segments && !st.fallback_segments && info.segments == 1) die("a faulted segment was accepted");
    g_parallel += st.parallel_segments;
    g_fellback += st.fallback_segments;
    g_decoded++;
}

std::vector<uint8_t> mutate(const std::vector<uint8_t>& src, Rng& r, bool container)
{
    std::vector<uint8_t> d = src;
    static const uint8_t markers[] = {0xD0, 0xD3, 0xD7, 0xD9, 0xDA, 0xC4, 0xDB, 0xDD, 0xC0, 0xC2, 0x00, 0xFF};
    const int kind = (int)r.below(container ? 7 : 6);
    const int reps = 1 + (int)r.below(4);
    for (int k = 0; k < reps && !d.empty(); k++) {
        switch (kind) {
        case 0:      // bit flips anywhere
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
        case 5: {    // a header byte rewritten
            const size_t lim = d.size() < 700 ? d.size() : 700;
            d[r.below(lim)] = (uint8_t)r.next();
            break;
        }
        default: {   // containers: a 32-bit size field rewritten (chunk headers sit on even offsets)
            if (d.size() < 16) break;
            const size_t p = (r.below(d.size() - 8) & ~(size_t)1) + 4;
            const uint32_t v = r.below(3) == 0 ? 0xFFFFFFF0u + (uint32_t)r.below(16) : (uint32_t)r.below(d.size() * 2);
            std::memcpy(&d[p], &v, 4 <= d.size() - p ? 4 : d.size() - p);
            break;
        }
        }
    }
    return d;
}

std::vector<uint8_t> read_file(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) die("cannot open a file");
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) d.insert(d.end(), buf, buf + n);
    std::fclose(f);
    return d;
}

// returns true when the walker took the container; every frame it reports must lie inside the buffer
bool walk(const std::vector<uint8_t>& src)
{
    std::vector<uint8_t> d(src);
    struct slam_avi_info info;
    const int rc = slam_avi_index(d.data(), d.size(), &info, nullptr, nullptr, 0);
    if (rc != SLAM_OK) {
        if (rc != SLAM_E_INVALID_ARG && rc != SLAM_E_UNSUPPORTED) die("unknown refusal code of the walker");
        if (!slam_avi_last_error()[0]) die("a refusal of the walker without a message");
        return false;
    }
    if (info.frames < 0 || (uint64_t)info.frames > d.size()) die("more frames than bytes");
    std::vector<uint64_t> off((size_t)info.frames), size((size_t)info.frames);
    if (slam_avi_index(d.data(), d.size(), &info, off.data(), size.data(), off.size()) != SLAM_OK) die("the second walk failed");
    for (size_t i = 0; i < off.size(); i++)
        if (off[i] > d.size() || size[i] > d.size() - off[i]) die("a frame outside the buffer");
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const int per = std::atoi(argv[1]);
    Rng rng{0xD1B54A32D192ED03ull};
    long streams = 0, mutated = 0, avi_runs = 0, avi_ok = 0;
    for (int a = 2; a < argc; a++) {
        const std::vector<uint8_t> d = read_file(argv[a]);
        const size_t n = std::strlen(argv[a]);
        if (n > 4 && std::strcmp(argv[a] + n - 4, ".avi") == 0) {
            if (!walk(d)) die("a well-formed container was refused");
            for (int k = 0; k < 30 * per; k++) {
                avi_runs++;
                avi_ok += walk(mutate(d, rng, true)) ? 1 : 0;
            }
            continue;
        }
        streams++;
        both(d, 0, 16, false);
        both(d, 0, 64, false);
        both(d, SLAM_JPEG_MJPEG, 64, false);
        // large streams get fewer mutations: the run is meant to take seconds
        const int m = d.size() > 100000 ? per / 20 : d.size() > 20000 ? per / 4 : per;
        for (int k = 0; k < m; k++) {
            const std::vector<uint8_t> x = mutate(d, rng, false);
            both(x, (k & 2) ? SLAM_JPEG_MJPEG : 0, (k & 1) ? 64 : 16, true);
            mutated++;
        }
    }
    std::printf("streams %ld mutated %ld decoded %ld refused %ld parallel %ld fellback %ld accepted %ld avi_runs %ld avi_ok %ld avi_refused %ld\n",
                streams, mutated, g_decoded, g_refused, g_parallel, g_fellback, g_parallel - g_fellback, avi_runs, avi_ok,
                avi_runs - avi_ok);
    return 0;
}

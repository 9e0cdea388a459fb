// Stand-alone check of the texture atlas host twins (csrc/tex_host.cpp), built with
// -fsanitize=address,undefined,float-cast-overflow by tests/test_tex.py.  The twins are
// compared with vectors dumped by the contract (tests/tex_ref.py): argv[1] is a file of
// arrays, each a line `name dtype count` followed by its raw bytes.  Every buffer has
// exactly the stated size, so an access out of bounds is an ASan report; the selection is
// also run split over calls in both orders, and the fill on 500 fixed-seed random
// projections of ordinary, 1e300, 1e150 and denormal magnitude with NaNs and infinities mixed in.
#include "../../include/slamhip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int g_fail = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            g_fail++;                                              \
        }                                                          \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
static double sym() { return 2.0 * ((double)(rnd() >> 11) / 9007199254740992.0) - 1.0; }

static FILE* g_in = nullptr;

// the next array of the file: its name must be `name`
template <class T> static std::vector<T> next(const char* name)
{
    char got[64], dtype[64];
    long long count = 0;
    if (fscanf(g_in, "%63s %63s %lld", got, dtype, &count) != 3 || fgetc(g_in) != '\n' || strcmp(got, name) != 0 || count < 0) {
        printf("FAIL: expected array %s\n", name);
        exit(2);
    }
    std::vector<T> v((size_t)count);
    if (count && fread(v.data(), sizeof(T), (size_t)count, g_in) != (size_t)count) {
        printf("FAIL: array %s is short\n", name);
        exit(2);
    }
    return v;
}

int main(int argc, char** argv)
{
    if (argc < 2 || !(g_in = fopen(argv[1], "rb"))) {
        printf("usage: tex_host_test vectors.bin\n");
        return 2;
    }
    int cases = 0;
    const std::vector<int32_t> n = next<int32_t>("ncases");
    for (int k = 0; k < n[0]; k++) {
        const auto d = next<int32_t>("dims");      // nv nf n h w channels nviews min_pixels T page
        const auto V = next<double>("V");
        const auto C = next<uint8_t>("C");
        const auto F = next<int32_t>("F");
        const auto frames = next<uint8_t>("frames");
        const auto fidx = next<int32_t>("fidx");
        auto P = next<double>("P");
        const auto bc = next<int32_t>("bc");
        const auto bv = next<int32_t>("bv");
        const auto want = next<uint8_t>("atlas");
        CHECK(frames.size() == (size_t)d[2] * d[3] * d[4] * d[5]);
        // the layout's sizes give the atlas exactly
        int npages = 0, pw = 0;
        CHECK(slam_tex_layout(d[1], d[8], d[9], &npages, &pw, nullptr, 0, nullptr, nullptr) == SLAM_OK);
        std::vector<int32_t> ph((size_t)npages), page((size_t)d[1]);
        std::vector<double> uv((size_t)d[1] * 6);
        CHECK(slam_tex_layout(d[1], d[8], d[9], &npages, &pw, ph.data(), npages, uv.data(), page.data()) == SLAM_OK);
        size_t bytes = 0;
        for (int32_t hgt : ph) bytes += (size_t)hgt * pw * 3;
        CHECK(bytes == want.size());
        for (double u : uv) CHECK(u >= 0.0 && u <= 1.0);
        std::vector<uint8_t> got(bytes, 0xAB);
        int rc = slam_tex_fill_host(V.data(), C.data(), F.data(), d[0], d[1], frames.data(), d[2], d[3], d[4], d[5], fidx.data(),
                                    P.data(), d[6], bc.data(), bv.data(), d[7], d[8], d[9], got.data());
        CHECK(rc == SLAM_OK);
        CHECK(got == want);
        cases++;
        // random projections: no NaN, infinity or huge value reaches an integer conversion or an index
        if (k == 0) {
            const double mags[4] = {1.0, 1e300, 1e150, 4.9406564584124654e-324 * 1000.0};
            for (int t = 0; t < 500; t++) {
                for (size_t i = 0; i < P.size(); i++) {
                    P[i] = sym() * 30.0 * mags[(t + (rnd() % 3 == 0 ? (int)(rnd() % 4) : 0)) % 4];
                    if (rnd() % 41 == 0) P[i] = rnd() % 2 ? NAN : (rnd() % 2 ? INFINITY : -INFINITY);
                }
                rc = slam_tex_fill_host(V.data(), C.data(), F.data(), d[0], d[1], frames.data(), d[2], d[3], d[4], d[5], fidx.data(),
                                        P.data(), d[6], bc.data(), bv.data(), d[7], d[8], d[9], got.data());
                CHECK(rc == SLAM_OK);
            }
            cases += 500;
        }
    }
    for (int k = 0; k < n[1]; k++) {
        const auto d = next<int32_t>("sdims");     // nv h w view0 nf
        const auto ids = next<int32_t>("ids");
        const auto wc = next<int32_t>("bc");
        const auto wv = next<int32_t>("bv");
        const size_t npx = (size_t)d[1] * d[2];
        CHECK(ids.size() == npx * d[0] && wc.size() == (size_t)d[4]);
        std::vector<int32_t> bc((size_t)d[4], 0), bv((size_t)d[4], -1);
        CHECK(slam_tex_select_host(ids.data(), d[0], d[1], d[2], d[3], d[4], bc.data(), bv.data()) == SLAM_OK);
        CHECK(bc == wc && bv == wv);
        // one view per call, last view first
        std::fill(bc.begin(), bc.end(), 0);
        std::fill(bv.begin(), bv.end(), -1);
        for (int m = d[0] - 1; m >= 0; m--) {
            const std::vector<int32_t> one(ids.begin() + (size_t)m * npx, ids.begin() + (size_t)(m + 1) * npx);
            CHECK(slam_tex_select_host(one.data(), 1, d[1], d[2], d[3] + m, d[4], bc.data(), bv.data()) == SLAM_OK);
        }
        CHECK(bc == wc && bv == wv);
        cases++;
    }
    // argument errors come before any access
    {
        int32_t one[4] = {0, 0, 0, 0};
        int np = 0, pw = 0;
        CHECK(slam_tex_select_host(nullptr, 1, 2, 2, 0, 4, one, one) == SLAM_E_INVALID_ARG);
        CHECK(slam_tex_select_host(one, 1, 2, 2, 0, (1 << 30) + 1, one, one) == SLAM_E_UNSUPPORTED);
        CHECK(slam_tex_select_host(nullptr, 0, 2, 2, 0, 0, nullptr, nullptr) == SLAM_OK);
        CHECK(slam_tex_layout(2, 0, 64, &np, &pw, nullptr, 0, nullptr, nullptr) == SLAM_E_INVALID_ARG);
        CHECK(slam_tex_layout(2, 5, 8, &np, &pw, nullptr, 0, nullptr, nullptr) == SLAM_E_INVALID_ARG);
        CHECK(slam_tex_layout(0, 5, 9, &np, &pw, nullptr, 0, nullptr, nullptr) == SLAM_OK && np == 0 && pw == 9);
        CHECK(slam_tex_fill_host(nullptr, nullptr, nullptr, 0, 0, nullptr, 0, 4, 4, 3, nullptr, nullptr, 0, nullptr, nullptr, 4, 5, 64,
                                 nullptr) == SLAM_OK);
        CHECK(slam_tex_fill_host(nullptr, nullptr, nullptr, 0, 2, nullptr, 0, 4, 4, 3, nullptr, nullptr, 0, nullptr, nullptr, 4, 5, 64,
                                 nullptr) == SLAM_E_INVALID_ARG);
        CHECK(slam_tex_fill_host(nullptr, nullptr, nullptr, 0, 0, nullptr, 0, 4, 4, 2, nullptr, nullptr, 0, nullptr, nullptr, 4, 5, 64,
                                 nullptr) == SLAM_E_INVALID_ARG);
    }
    fclose(g_in);
    if (g_fail) {
        printf("%d failures\n", g_fail);
        return 1;
    }
    printf("OK: %d cases\n", cases);
    return 0;
}

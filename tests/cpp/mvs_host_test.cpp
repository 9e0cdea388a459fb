// Stand-alone driver of the plane-sweep host twin (csrc/mvs_host.cpp + csrc/mvs_math.h),
// built by tests/test_mvs.py with -fsanitize=address,undefined and run as a plain
// program.  Every output lives in a heap buffer of exactly the stated size, so a write
// past an image, a tile or a plane table is reported; every float -> int conversion of a
// projection is checked by UBSan.  The values are checked against a direct restatement of
// the rule on the full cost volume (no streaming), and the planted plane against its
// known answer.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/slamhip.h"
#include "../../slam-indoor-code_amd/csrc/mvs_math.h"

using namespace slamhip;

namespace slamhip {
void mvs_census_host(const uint8_t* img, int w, int h, size_t step, int channels, uint64_t* out);
}

static int failures = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            failures++;                                                 \
        }                                                               \
    } while (0)

struct Rng {
    uint64_t s;
    uint32_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    double uni(double a, double b) { return a + (b - a) * (next() / 2147483648.0); }
};

struct Out {
    int16_t* plane;
    int32_t* cost;
    float* inv;
    Out(size_t n) : plane((int16_t*)malloc(n * 2)), cost((int32_t*)malloc(n * 4)), inv((float*)malloc(n * 4)) {}
    ~Out()
    {
        free(plane);
        free(cost);
        free(inv);
    }
};

// the rule on the materialised cost volume
static void direct(const uint8_t* ref, const std::vector<const uint8_t*>& srcs, int w, int h, int ch, const double* M,
                   const double* v, const double* pl, int D, int r, int uniq, int min_views, Out& o)
{
    const int S = (int)srcs.size();
    const size_t npx = (size_t)w * h;
    std::vector<uint64_t> cen((S + 1) * npx);
    mvs_census_host(ref, w, h, (size_t)w * ch, ch, cen.data());
    for (int s = 0; s < S; s++) mvs_census_host(srcs[s], w, h, (size_t)w * ch, ch, cen.data() + (s + 1) * npx);
    std::vector<int32_t> raw((size_t)D * npx), nv((size_t)D * npx), C((size_t)D * npx);
    for (int d = 0; d < D; d++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                int sum = 0, n = 0;
                for (int s = 0; s < S; s++) {
                    double q[3], h2;
                    int ix, iy;
                    mvs_q(M + 9 * s, x, y, q);
                    if (mvs_project(q, v + 3 * s, pl[d], w, h, &ix, &iy, &h2)) {
                        CHECK(ix >= 0 && ix < w && iy >= 0 && iy < h);
                        sum += mvs_popc64(cen[(size_t)y * w + x] ^ cen[(s + 1) * npx + (size_t)iy * w + ix]);
                        n++;
                    } else
                        sum += 64;
                }
                raw[d * npx + (size_t)y * w + x] = sum;
                nv[d * npx + (size_t)y * w + x] = n;
            }
    for (int d = 0; d < D; d++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                int sum = 0;
                for (int dy = -r; dy <= r; dy++)
                    for (int dx = -r; dx <= r; dx++)
                        sum += raw[d * npx + (size_t)mvs_clamp(y + dy, 0, h - 1) * w + mvs_clamp(x + dx, 0, w - 1)];
                C[d * npx + (size_t)y * w + x] = sum;
            }
    for (size_t i = 0; i < npx; i++) {
        int best = 0;
        for (int d = 1; d < D; d++)
            if (C[d * npx + i] < C[best * npx + i]) best = d;
        int64_t second = std::numeric_limits<int64_t>::max();
        for (int d = 0; d < D; d++)
            if (std::abs(d - best) > 1 && C[d * npx + i] < second) second = C[d * npx + i];
        const int32_t b = C[best * npx + i];
        o.plane[i] = (int16_t)best;
        o.cost[i] = b;
        float inv = 0.f;
        if ((int64_t)b * 100 < uniq * second && nv[best * npx + i] >= min_views) {
            double wq = pl[best];
            if (best > 0 && best < D - 1) {
                const int32_t a = C[(best - 1) * npx + i], c = C[(best + 1) * npx + i], den = a - 2 * b + c;
                const double off = den > 0 ? (double)(a - c) / (double)(2 * den) : 0.0;
                wq = off >= 0 ? pl[best] + off * (pl[best + 1] - pl[best]) : pl[best] + off * (pl[best] - pl[best - 1]);
            }
            inv = (float)wq;
        }
        o.inv[i] = inv;
    }
}

static bool run_case(const char* name, int w, int h, int ch, int S, int D, int r, int uniq, int min_views, const double* M,
                     const double* v, const double* pl, Rng& g, bool same_frames, int shift, bool planted = false)
{
    const size_t fb = (size_t)w * h * ch, npx = (size_t)w * h;
    // frames in buffers of exactly w * h * ch bytes
    std::vector<uint8_t*> fr(S + 1);
    for (int f = 0; f <= S; f++) {
        fr[f] = (uint8_t*)malloc(fb);
        for (size_t i = 0; i < fb; i++) fr[f][i] = (uint8_t)(g.next() >> 8);
    }
    if (same_frames)
        for (int f = 1; f <= S; f++)
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++)
                    for (int k = 0; k < ch; k++) fr[f][((size_t)y * w + (x + shift) % w) * ch + k] = fr[0][((size_t)y * w + x) * ch + k];
    std::vector<const uint8_t*> srcs(fr.begin() + 1, fr.end());
    // the arguments too, so a read past S x 9, S x 3 or D doubles is seen
    double* Mh = (double*)malloc(sizeof(double) * 9 * S);
    double* vh = (double*)malloc(sizeof(double) * 3 * S);
    double* ph = (double*)malloc(sizeof(double) * D);
    memcpy(Mh, M, sizeof(double) * 9 * S);
    memcpy(vh, v, sizeof(double) * 3 * S);
    memcpy(ph, pl, sizeof(double) * D);
    Out got(npx), want(npx);
    const int rc = slam_mvs_depth_host(fr[0], srcs.data(), S, w, h, (size_t)w * ch, ch, Mh, vh, ph, D, r, uniq, min_views,
                                       got.plane, got.cost, got.inv);
    bool ok = rc == SLAM_OK;
    if (ok) {
        direct(fr[0], srcs, w, h, ch, Mh, vh, ph, D, r, uniq, min_views, want);
        ok = !memcmp(got.plane, want.plane, npx * 2) && !memcmp(got.cost, want.cost, npx * 4) &&
             !memcmp(got.inv, want.inv, npx * 4);
        for (size_t i = 0; i < npx; i++) ok = ok && got.plane[i] >= 0 && got.plane[i] < D;
    }
    if (!ok) {
        printf("FAIL case %s (rc %d)\n", name, rc);
        failures++;
    }
    if (planted && ok) {      // the planted plane: the known answer
        for (int y = 5; y < h - 5; y++)
            for (int x = 6; x < w - 6 - shift; x++) {
                const size_t i = (size_t)y * w + x;
                CHECK(got.plane[i] == shift && got.cost[i] == 0 && got.inv[i] > 0.f);
            }
    }
    free(Mh);
    free(vh);
    free(ph);
    for (auto p : fr) free(p);
    return ok;
}

int main()
{
    Rng g{12345};
    const double I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double vx[3] = {1, 0, 0};
    double pl12[12];
    for (int d = 0; d < 12; d++) pl12[d] = d;
    // planted plane and its relatives
    run_case("planted", 52, 40, 1, 1, 12, 2, 80, 1, I9, vx, pl12, g, true, 5, true);
    run_case("planted_bgr", 52, 40, 3, 1, 12, 2, 80, 1, I9, vx, pl12, g, true, 5, true);
    {
        const double eq[6] = {0, 1, 2, 2, 3, 4};
        run_case("equal_w", 24, 20, 1, 1, 6, 2, 80, 1, I9, vx, eq, g, true, 2, true);
        double neg[9];
        for (int i = 0; i < 9; i++) neg[i] = -I9[i];
        const double v0[3] = {0, 0, 0};
        run_case("behind", 24, 20, 1, 1, 6, 2, 80, 1, neg, v0, pl12, g, false, 0);
        double far_[9];
        memcpy(far_, I9, sizeof(I9));
        far_[2] = 1e4;
        run_case("out_of_view", 24, 20, 1, 1, 6, 3, 80, 1, far_, vx, pl12, g, false, 0);
        const double hugeM[9] = {1e300, -1e300, 1e300, -1e300, 1e300, 1e300, 1e300, 1e300, -1e300};
        const double hugev[3] = {1e300, -1e300, 1e300};
        const double hugep[6] = {0.0, 1.0, 1e300, -1e300, 5e-324, 3.0};
        run_case("huge", 24, 20, 1, 1, 6, 2, 80, 1, hugeM, hugev, hugep, g, false, 0);
    }
    // fixed-seed random M, v, w: ordinary, huge and denormal magnitudes, S, radius and sizes mixed
    const int sizes[4][2] = {{8, 8}, {13, 9}, {33, 7}, {17, 21}};
    const double mags[6] = {1.0, 1e-3, 1e3, 1e300, 1e-310, 1e150};
    int ran = 0;
    for (int it = 0; it < 3000; it++) {
        const int* sz = sizes[it % 4];
        const int S = 1 + (int)(g.next() % 4), D = 4 + (int)(g.next() % 6), r = (int)(g.next() % 4), ch = (g.next() & 1) ? 3 : 1;
        double M[36], v[12], pl[16];
        const int kind = (int)(g.next() % 3);      // 0: near the identity, 1: free, 2: wild magnitudes
        for (int s = 0; s < S; s++)
            for (int i = 0; i < 9; i++) {
                if (kind == 0)
                    M[9 * s + i] = I9[i] + g.uni(-0.05, 0.05) * (i % 3 == 2 ? 20 : 1);
                else if (kind == 1)
                    M[9 * s + i] = g.uni(-2, 2) * (i % 3 == 2 ? 10 : 1);
                else
                    M[9 * s + i] = g.uni(-1, 1) * mags[g.next() % 6];
            }
        for (int i = 0; i < 3 * S; i++) v[i] = kind == 2 ? g.uni(-1, 1) * mags[g.next() % 6] : g.uni(-3, 3);
        for (int d = 0; d < D; d++) pl[d] = kind == 2 ? g.uni(-1, 1) * mags[g.next() % 6] : g.uni(0, 2);
        const int mv = 1 + (int)(g.next() % S), uq = 1 + (int)(g.next() % 100);
        char name[64];
        snprintf(name, sizeof(name), "random %d (kind %d)", it, kind);
        ran += run_case(name, sz[0], sz[1], ch, S, D, r, uq, mv, M, v, pl, g, kind == 0 && (it & 8), 1) ? 1 : 0;
    }
    // argument errors
    {
        uint8_t img[64] = {0};
        const uint8_t* srcs[4] = {img, img, img, img};
        Out o(64);
        auto call = [&](int S, int w, int D, int r, const double* M, const double* v, const double* pl, int uq, int mv) {
            return slam_mvs_depth_host(img, srcs, S, w, 8, (size_t)w, 1, M, v, pl, D, r, uq, mv, o.plane, o.cost, o.inv);
        };
        double M4[36], v4[12];
        for (int s = 0; s < 4; s++) {
            memcpy(M4 + 9 * s, I9, sizeof(I9));
            memcpy(v4 + 3 * s, vx, sizeof(vx));
        }
        CHECK(call(1, 8, 12, 2, M4, v4, pl12, 80, 1) == SLAM_OK);
        CHECK(call(0, 8, 12, 2, M4, v4, pl12, 80, 1) == SLAM_E_INVALID_ARG);
        CHECK(call(5, 8, 12, 2, M4, v4, pl12, 80, 1) == SLAM_E_INVALID_ARG);
        CHECK(call(1, 8, 3, 2, M4, v4, pl12, 80, 1) == SLAM_E_INVALID_ARG);
        CHECK(call(1, 8, 257, 2, M4, v4, pl12, 80, 1) == SLAM_E_INVALID_ARG);
        CHECK(call(1, 8, 12, 4, M4, v4, pl12, 80, 1) == SLAM_E_INVALID_ARG);
        CHECK(call(1, 8, 12, 2, M4, v4, pl12, 0, 1) == SLAM_E_INVALID_ARG);
        CHECK(call(1, 8, 12, 2, M4, v4, pl12, 101, 1) == SLAM_E_INVALID_ARG);
        CHECK(call(2, 8, 12, 2, M4, v4, pl12, 80, 3) == SLAM_E_INVALID_ARG);
        CHECK(call(1, 4097, 12, 2, M4, v4, pl12, 80, 1) == SLAM_E_UNSUPPORTED);
        double bad[12];
        memcpy(bad, pl12, sizeof(bad));
        bad[3] = std::numeric_limits<double>::quiet_NaN();
        CHECK(call(1, 8, 12, 2, M4, v4, bad, 80, 1) == SLAM_E_INVALID_ARG);
        double Mb[9];
        memcpy(Mb, I9, sizeof(I9));
        Mb[4] = std::numeric_limits<double>::infinity();
        CHECK(call(1, 8, 12, 2, Mb, v4, pl12, 80, 1) == SLAM_E_INVALID_ARG);
        double vb[3] = {0, -std::numeric_limits<double>::infinity(), 0};
        CHECK(call(1, 8, 12, 2, M4, vb, pl12, 80, 1) == SLAM_E_INVALID_ARG);
    }
    printf("%s: %d random cases equal the direct rule, %d failures\n", failures ? "FAILED" : "OK", ran, failures);
    return failures ? 1 : 0;
}

// Stand-alone driver of the semi-global host twins (csrc/mvs_sgm_host.cpp over
// csrc/mvs_host.cpp), built by tests/test_mvs_sgm.py with -fsanitize=address,undefined
// and run as a plain program.  Every buffer is a heap block of exactly the stated size,
// so a read or write past a scan line, a plane or a volume is reported.  The values are
// checked against a direct, unoptimised restatement of the recurrence (pixel by pixel
// over the whole image, no scan lines) and of the winner rule on the full volume.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/slamhip.h"

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
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

template <class T> struct Exact {      // a heap block of exactly n elements
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p((T*)malloc(n_ * sizeof(T) ? n_ * sizeof(T) : 1)), n(n_) {}
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

static const int kMaxCost = 12544, kMaxP2 = 65535 - 12544;
static const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1}, DY[8] = {0, 0, 1, -1, 1, -1, -1, 1};

// S = sum over the paths of L_r, every L_r from its definition: pixels visited so that p - r is done before p
static void direct_aggregate(const uint16_t* C, int w, int h, int D, long long P1, long long P2, int paths, int32_t* S)
{
    const size_t vol = (size_t)w * h * D;
    std::vector<long long> L(vol), sum(vol, 0);
    for (int r = 0; r < paths; r++) {
        const int dx = DX[r], dy = DY[r];
        for (int yi = 0; yi < h; yi++)
            for (int xi = 0; xi < w; xi++) {
                const int y = dy < 0 ? h - 1 - yi : yi, x = dx < 0 ? w - 1 - xi : xi;
                const int qx = x - dx, qy = y - dy;
                long long* Lp = &L[((size_t)y * w + x) * D];
                const uint16_t* Cp = C + ((size_t)y * w + x) * D;
                if (qx < 0 || qx >= w || qy < 0 || qy >= h) {
                    for (int d = 0; d < D; d++) Lp[d] = Cp[d];
                } else {
                    const long long* Lq = &L[((size_t)qy * w + qx) * D];
                    long long m = Lq[0];
                    for (int d = 1; d < D; d++) m = Lq[d] < m ? Lq[d] : m;
                    for (int d = 0; d < D; d++) {
                        long long best = Lq[d];
                        if (d > 0 && Lq[d - 1] + P1 < best) best = Lq[d - 1] + P1;
                        if (d + 1 < D && Lq[d + 1] + P1 < best) best = Lq[d + 1] + P1;
                        if (m + P2 < best) best = m + P2;
                        Lp[d] = Cp[d] + best - m;
                        CHECK(Lp[d] >= Cp[d] && Lp[d] <= Cp[d] + P2 && Lp[d] <= 65535);
                    }
                }
                for (int d = 0; d < D; d++) sum[((size_t)y * w + x) * D + d] += Lp[d];
            }
    }
    for (size_t i = 0; i < vol; i++) S[i] = (int32_t)sum[i];
}

// the winner rule on a full volume of one pixel
static void direct_winner(const int32_t* S, const uint8_t* nv, const double* pl, int D, int uniq, int min_views,
                          int16_t* plane, int32_t* cost, float* inv)
{
    int best = 0;
    for (int d = 1; d < D; d++)
        if (S[d] < S[best]) best = d;
    bool have = false;
    long long second = 0;
    for (int d = 0; d < D; d++)
        if (abs(d - best) > 1 && (!have || S[d] < second)) {
            second = S[d];
            have = true;
        }
    *plane = (int16_t)best;
    *cost = S[best];
    float out = 0.f;
    if (have && (long long)S[best] * 100 < (long long)uniq * second && nv[best] >= min_views) {
        double wq = pl[best];
        if (best > 0 && best < D - 1) {
            const long long a = S[best - 1], b = S[best], c = S[best + 1], den = a - 2 * b + c;
            const double off = den > 0 ? (double)(a - c) / (double)(2 * den) : 0.0;
            wq = off >= 0.0 ? pl[best] + off * (pl[best + 1] - pl[best]) : pl[best] + off * (pl[best] - pl[best - 1]);
        }
        out = (float)wq;
    }
    *inv = out;
}

static void random_volumes(int count, uint64_t seed)
{
    Rng rng{seed};
    for (int it = 0; it < count; it++) {
        const bool big = it % 200 == 0;
        const int w = big ? 9 : 1 + rng.below(9), h = big ? 7 : 1 + rng.below(7);
        const int Ds[] = {4, 5, 12, 63, 64, 65, 128, 129, 256};
        const int D = big ? 256 : (it % 7 == 0 ? Ds[rng.below(9)] : 4 + rng.below(29));
        const int paths = rng.below(2) ? 8 : 4, n = 1 + (it % 3 == 0);
        int P2 = it % 4 == 0 ? kMaxP2 : rng.below(kMaxP2 + 1);
        int P1 = it % 5 == 0 ? P2 : rng.below(P2 + 1);
        const size_t vol = (size_t)w * h * D;
        Exact<uint16_t> C(n * vol);
        Exact<int32_t> got(n * vol), want(n * vol);
        const int mode = rng.below(3);       // the values at their maxima, two-valued, or anything
        for (size_t i = 0; i < n * vol; i++) {
            const int t = rng.below(10);
            C.p[i] = (uint16_t)(mode == 0 ? (t < 6 ? kMaxCost : (t < 8 ? 0 : kMaxCost - 1))
                                          : (mode == 1 ? (t < 5 ? 0 : kMaxCost) : rng.below(kMaxCost + 1)));
        }
        memset(got.p, 0x5a, n * vol * 4);
        CHECK(slam_mvs_sgm_aggregate_host(C.p, n, w, h, D, P1, P2, paths, got.p) == SLAM_OK);
        for (int i = 0; i < n; i++) direct_aggregate(C.p + i * vol, w, h, D, P1, P2, paths, want.p + i * vol);
        const bool same = memcmp(got.p, want.p, n * vol * 4) == 0;
        if (!same) printf("volume %d: %d x %d x %d, n %d, P %d %d, paths %d\n", it, w, h, D, n, P1, P2, paths);
        CHECK(same);
    }
}

// a textured frame with a constant box (none when the frame is too small) and a source shifted by k pixels
static void scene(int w, int h, int ch, int k, uint64_t seed, uint8_t* ref, uint8_t* src)
{
    Rng rng{seed};
    for (size_t i = 0; i < (size_t)w * h * ch; i++) ref[i] = (uint8_t)rng.below(256);
    for (int y = h / 3; y < 2 * h / 3; y++)
        for (int x = w / 3; x < 2 * w / 3; x++)
            for (int c = 0; c < ch; c++) ref[((size_t)y * w + x) * ch + c] = 128;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            memcpy(src + ((size_t)y * w + (x + k) % w) * ch, ref + ((size_t)y * w + x) * ch, ch);
}

static void depth_case(int w, int h, int ch, int S, int D, int r, int uniq, int p1, int p2, int paths, uint64_t seed)
{
    const size_t fb = (size_t)w * h * ch, npx = (size_t)w * h, vol = npx * D;
    Exact<uint8_t> ref(fb), s0(fb), s1(fb);
    scene(w, h, ch, 5, seed, ref.p, s0.p);
    scene(w, h, ch, 3, seed, ref.p, s1.p);
    const uint8_t* srcs[2] = {s0.p, s1.p};
    // a shift along x, the second source a little rotated and scaled
    const double M[18] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.999, 0.012, 0.1, -0.012, 0.999, -0.2, 1e-5, -2e-5, 1.0};
    const double v[6] = {1, 0, 0, 0.6, 0.05, 0.001};
    Exact<double> pl(D);
    for (int d = 0; d < D; d++) pl.p[d] = D <= 16 ? d : 12.0 * d / (D - 1);
    Exact<uint16_t> C(vol);
    Exact<uint8_t> nv(vol);
    Exact<int32_t> agg(vol), cost(npx), wcost(npx);
    Exact<int16_t> plane(npx), wplane(npx);
    Exact<float> inv(npx), winv(npx);
    CHECK(slam_mvs_cost_volume_host(ref.p, srcs, S, w, h, (size_t)w * ch, ch, M, v, pl.p, D, r, C.p, nv.p) == SLAM_OK);
    const int win = (2 * r + 1) * (2 * r + 1);
    for (size_t i = 0; i < vol; i++) CHECK(C.p[i] <= 64 * win * S && nv.p[i] <= S);
    CHECK(slam_mvs_depth_sgm_host(ref.p, srcs, S, w, h, (size_t)w * ch, ch, M, v, pl.p, D, r, uniq, 1, p1, p2, paths,
                                  plane.p, cost.p, inv.p) == SLAM_OK);
    direct_aggregate(C.p, w, h, D, (long long)p1 * win * S, (long long)p2 * win * S, paths, agg.p);
    for (size_t i = 0; i < npx; i++)
        direct_winner(agg.p + i * D, nv.p + i * D, pl.p, D, uniq, 1, &wplane.p[i], &wcost.p[i], &winv.p[i]);
    const bool same = !memcmp(plane.p, wplane.p, npx * 2) && !memcmp(cost.p, wcost.p, npx * 4) && !memcmp(inv.p, winv.p, npx * 4);
    if (!same) printf("depth %d x %d x %d, S %d, D %d, r %d, p %d %d, paths %d\n", w, h, ch, S, D, r, p1, p2, paths);
    CHECK(same);
    if (p1 == 0 && p2 == 0) {      // the identity: every L_r is C
        CHECK(slam_mvs_depth_host(ref.p, srcs, S, w, h, (size_t)w * ch, ch, M, v, pl.p, D, r, uniq, 1, wplane.p, wcost.p,
                                  winv.p) == SLAM_OK);
        CHECK(!memcmp(plane.p, wplane.p, npx * 2) && !memcmp(inv.p, winv.p, npx * 4));
        for (size_t i = 0; i < npx; i++) CHECK(cost.p[i] == paths * wcost.p[i]);
    }
}

static void argument_errors()
{
    Exact<uint16_t> C(2 * 3 * 4);
    Exact<int32_t> S(2 * 3 * 4);
    memset(C.p, 0, 2 * 3 * 4 * 2);
    CHECK(slam_mvs_sgm_aggregate_host(C.p, 1, 3, 2, 4, 1, 2, 8, S.p) == SLAM_OK);
    CHECK(slam_mvs_sgm_aggregate_host(C.p, 1, 3, 2, 4, 3, 2, 8, S.p) == SLAM_E_INVALID_ARG);
    CHECK(slam_mvs_sgm_aggregate_host(C.p, 1, 3, 2, 4, 1, kMaxP2 + 1, 8, S.p) == SLAM_E_INVALID_ARG);
    CHECK(slam_mvs_sgm_aggregate_host(C.p, 1, 3, 2, 4, -1, 2, 8, S.p) == SLAM_E_INVALID_ARG);
    CHECK(slam_mvs_sgm_aggregate_host(C.p, 1, 3, 2, 4, 1, 2, 6, S.p) == SLAM_E_INVALID_ARG);
    CHECK(slam_mvs_sgm_aggregate_host(C.p, 1, 3, 2, 3, 1, 2, 8, S.p) == SLAM_E_INVALID_ARG);
    CHECK(slam_mvs_sgm_aggregate_host(nullptr, 1, 3, 2, 4, 1, 2, 8, S.p) == SLAM_E_INVALID_ARG);
    CHECK(slam_mvs_sgm_aggregate_host(C.p, 1, 4097, 2, 4, 1, 2, 8, S.p) == SLAM_E_UNSUPPORTED);
    CHECK(slam_mvs_sgm_aggregate_host(nullptr, 0, 3, 2, 4, 1, 2, 8, nullptr) == SLAM_OK);
}

int main()
{
    argument_errors();
    random_volumes(3000, 2024);
    const int shapes[][2] = {{1, 1}, {9, 1}, {1, 9}, {8, 8}, {33, 67}, {67, 33}};      // w, h
    const int settings[][3] = {{10, 120, 8}, {2, 12, 4}, {0, 255, 8}, {255, 255, 4}, {0, 0, 8}, {0, 0, 4}};
    int k = 0;
    for (auto& sh : shapes)
        for (auto& st : settings) depth_case(sh[0], sh[1], 1 + 2 * (k % 2), 1 + k % 2, 12, k % 4, 80, st[0], st[1], st[2], 100 + k), k++;
    const int Ds[] = {4, 63, 64, 65, 128, 129, 256};
    for (int D : Ds)
        for (int s = 0; s < 4; s += 3) depth_case(24, 20, 1, 2, D, 2, 80, settings[s][0], settings[s][1], settings[s][2], 200 + D);
    depth_case(64, 48, 1, 1, 12, 2, 80, 10, 120, 8, 7);      // the wall scene's shape
    depth_case(64, 48, 1, 1, 12, 2, 80, 0, 0, 8, 7);
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("OK: mvs_sgm_host_test\n");
    return 0;
}

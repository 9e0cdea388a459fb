// Stand-alone check of the TSDF host twins (csrc/tsdf_host.cpp), built with
// -fsanitize=address,undefined,float-cast-overflow by tests/test_tsdf.py.  The
// integration is compared with a direct restatement of the rule of DESIGN.md section
// 26, written here without the shared header, on small volumes and on 2000 fixed-seed
// random projections of ordinary, 1e300, 1e150 and denormal magnitude; the extraction is
// checked for its invariants.  Every buffer has exactly the stated size, so an access
// out of bounds is an ASan report.
#include "../../include/slamhip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}
static double unit() { return (double)(rnd() >> 11) / 9007199254740992.0; }          // [0, 1)
static double sym() { return 2.0 * unit() - 1.0; }

static int g_fail = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            g_fail++;                                              \
        }                                                          \
    } while (0)

struct Scene {
    int nx, ny, nz, w, h, ch, nframes, nmaps;
    double origin[3], voxel, trunc;
    std::vector<uint8_t> frames;
    std::vector<float> inv;
    std::vector<double> P;
    std::vector<int32_t> idx;
};

// the rule, node by node, map by map
static void restate(const Scene& s, std::vector<int32_t>& vol)
{
    const size_t nn = (size_t)s.nx * s.ny * s.nz, npx = (size_t)s.w * s.h;
    for (int k = 0; k < s.nz; k++)
        for (int j = 0; j < s.ny; j++)
            for (int i = 0; i < s.nx; i++) {
                const size_t o = ((size_t)k * s.ny + j) * s.nx + i;
                const double X = s.origin[0] + (double)i * s.voxel, Y = s.origin[1] + (double)j * s.voxel,
                             Z = s.origin[2] + (double)k * s.voxel;
                for (int m = 0; m < s.nmaps; m++) {
                    const double* P = &s.P[(size_t)m * 12];
                    double hh[3];
                    for (int r = 0; r < 3; r++) hh[r] = ((P[4 * r] * X + P[4 * r + 1] * Y) + P[4 * r + 2] * Z) + P[4 * r + 3];
                    if (!(hh[2] > 0.0)) continue;
                    const double u = hh[0] / hh[2], v = hh[1] / hh[2];
                    if (!(u >= -0.5) || !(u < (double)s.w - 0.5) || !(v >= -0.5) || !(v < (double)s.h - 0.5)) continue;
                    const int ix = (int)std::floor(u + 0.5), iy = (int)std::floor(v + 0.5);
                    const float wv = s.inv[(size_t)m * npx + (size_t)iy * s.w + ix];
                    if (wv <= 0.f) continue;
                    double r = (1.0 / (double)wv - hh[2]) / s.trunc;
                    if (r < -1.0) continue;
                    if (r > 1.0) r = 1.0;
                    vol[o] += (int32_t)std::floor(r * 1024.0 + 0.5);
                    vol[nn + o] += 1;
                    if (r < 1.0) {
                        const uint8_t* px = &s.frames[((size_t)s.idx[m] * npx + (size_t)iy * s.w + ix) * s.ch];
                        vol[2 * nn + o] += 1;
                        for (int c = 0; c < 3; c++) vol[(3 + c) * nn + o] += px[s.ch == 3 ? c : 0];
                    }
                }
            }
}

static Scene make_scene(int nx, int ny, int nz, int nmaps, int ch)
{
    Scene s;
    s.nx = nx, s.ny = ny, s.nz = nz, s.w = 20, s.h = 24, s.ch = ch, s.nframes = nmaps + 1, s.nmaps = nmaps;
    s.origin[0] = -0.6, s.origin[1] = -0.5, s.origin[2] = 1.6;
    s.voxel = 1.2 / (nx > ny ? nx : ny), s.trunc = 0.45;
    const size_t npx = (size_t)s.w * s.h;
    s.frames.resize((size_t)s.nframes * npx * ch);
    for (auto& b : s.frames) b = (uint8_t)rnd();
    s.inv.resize((size_t)nmaps * npx);
    for (auto& v : s.inv) v = unit() < 0.1 ? 0.f : (float)(1.0 / (2.0 + 0.3 * sym()));
    s.P.resize((size_t)nmaps * 12);
    s.idx.resize(nmaps);
    for (int m = 0; m < nmaps; m++) {
        const double P[12] = {20, 0, 9.5, 0.5 * sym(), 0, 20, 11.5, 0.5 * sym(), 0, 0, 1, 0.05 * sym()};
        memcpy(&s.P[(size_t)m * 12], P, sizeof(P));
        s.idx[m] = nmaps - m;                      // not the identity
    }
    return s;
}

static void check_integrate(const Scene& s, const char* what)
{
    const size_t nn = (size_t)s.nx * s.ny * s.nz;
    std::vector<int32_t> want(6 * nn, 0), got(6 * nn, 0);
    restate(s, want);
    const int rc = slam_tsdf_integrate_host(got.data(), s.nx, s.ny, s.nz, s.origin, s.voxel, s.trunc, s.frames.data(),
                                            s.nframes, s.w, s.h, s.ch, s.idx.data(), s.inv.data(), s.P.data(), s.nmaps);
    CHECK(rc == SLAM_OK);
    if (memcmp(want.data(), got.data(), 6 * nn * sizeof(int32_t)) != 0) {
        printf("FAIL: %s differs from the rule\n", what);
        g_fail++;
    }
}

// counts, then buffers of exactly that size; every index in range, every capacity error clean
static void check_mesh(const std::vector<int32_t>& vol, int nx, int ny, int nz, int min_weight, int* nv_out, int* nf_out)
{
    const double origin[3] = {0.25, -1.0, 2.0};
    int nv = -1, nf = -1;
    int rc = slam_tsdf_mesh_host(vol.data(), nx, ny, nz, origin, 0.5, min_weight, nullptr, nullptr, nullptr, 0, 0, &nv, &nf);
    CHECK(rc == (nv == 0 ? SLAM_OK : SLAM_E_CAPACITY) && nv >= 0 && nf >= 0);
    *nv_out = nv, *nf_out = nf;
    if (nv == 0) {
        CHECK(nf == 0);
        return;
    }
    std::vector<double> v((size_t)nv * 3);
    std::vector<uint8_t> c((size_t)nv * 3);
    std::vector<int32_t> f((size_t)nf * 3);
    int nv2 = 0, nf2 = 0;
    if (nf > 0) {
        std::vector<int32_t> shortf((size_t)(nf - 1) * 3, -9);
        rc = slam_tsdf_mesh_host(vol.data(), nx, ny, nz, origin, 0.5, min_weight, v.data(), c.data(), shortf.data(), nv, nf - 1,
                                 &nv2, &nf2);
        CHECK(rc == SLAM_E_CAPACITY && nv2 == nv && nf2 == nf);
        for (int32_t x : shortf) CHECK(x == -9);
    }
    rc = slam_tsdf_mesh_host(vol.data(), nx, ny, nz, origin, 0.5, min_weight, v.data(), c.data(), f.data(), nv, nf, &nv2, &nf2);
    CHECK(rc == SLAM_OK && nv2 == nv && nf2 == nf);
    std::vector<int> used(nv, 0);
    for (int32_t x : f) {
        CHECK(x >= 0 && x < nv);
        if (x >= 0 && x < nv) used[x] = 1;
    }
    for (int u : used) CHECK(u == 1);                 // the vertex set is exactly the set that faces reference
    for (int i = 0; i < nv; i++)
        for (int k = 0; k < 3; k++) {
            const double lo = origin[k], hi = origin[k] + 0.5 * ((k == 0 ? nx : k == 1 ? ny : nz) - 1);
            CHECK(v[3 * i + k] >= lo && v[3 * i + k] <= hi);
        }
}

int main()
{
    int cases = 0;
    const int dims[4][3] = {{2, 2, 2}, {3, 2, 2}, {9, 7, 5}, {17, 17, 17}};
    for (const auto& d : dims)
        for (int nmaps = 1; nmaps <= 3; nmaps++)
            for (int ch = 1; ch <= 3; ch += 2) {
                const Scene s = make_scene(d[0], d[1], d[2], nmaps, ch);
                check_integrate(s, "scene");
                cases++;
            }
    // r exactly -1 and 1, and just beyond: depth 2, nodes at Z = 1.5 .. 3.5, trunc 0.5 and its neighbours
    for (double tr : {0.5, std::nextafter(0.5, 0.0), std::nextafter(0.5, 1.0)}) {
        Scene s = make_scene(2, 2, 5, 1, 3);
        s.w = s.h = 4;
        s.frames.assign((size_t)2 * 16 * 3, 77);
        s.inv.assign(16, 0.5f);
        const double P[12] = {1, 0, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0};
        memcpy(s.P.data(), P, sizeof(P));
        s.origin[0] = s.origin[1] = 0.0, s.origin[2] = 1.5, s.voxel = 0.5, s.trunc = tr;
        check_integrate(s, "exact r");
        cases++;
    }
    // 2000 random projections: ordinary, 1e300, 1e150 and denormal magnitudes, mixed signs
    {
        Scene s = make_scene(5, 4, 3, 1, 3);
        const double mags[4] = {1.0, 1e300, 1e150, 4.9406564584124654e-324 * 1000.0};
        for (int t = 0; t < 2000; t++) {
            for (int k = 0; k < 12; k++) {
                const double mag = mags[(t + (rnd() % 3 == 0 ? (int)(rnd() % 4) : 0)) % 4];
                s.P[k] = sym() * 30.0 * mag;
            }
            check_integrate(s, "random P");
        }
        cases += 2000;
    }
    // extraction: integrated volumes, random signs with unknown nodes, D == 0, empty, all inside
    {
        const Scene s = make_scene(9, 7, 5, 3, 3);
        std::vector<int32_t> vol(6 * (size_t)9 * 7 * 5, 0);
        restate(s, vol);
        int nv, nf, total = 0;
        for (int mw = 1; mw <= 2; mw++) {
            check_mesh(vol, 9, 7, 5, mw, &nv, &nf);
            total += nf;
        }
        CHECK(total > 0);
        const int n = 11;
        std::vector<int32_t> rv(6 * (size_t)n * n * n, 0);
        for (int t = 0; t < 4; t++) {
            for (size_t o = 0; o < (size_t)n * n * n; o++) {
                rv[o] = (int32_t)(rnd() % 7) - 3;
                rv[(size_t)n * n * n + o] = t == 0 ? 1 : (int32_t)(rnd() % 3);
                rv[2 * (size_t)n * n * n + o] = (int32_t)(rnd() % 2);
                for (int c = 0; c < 3; c++) rv[(3 + c) * (size_t)n * n * n + o] = rv[2 * (size_t)n * n * n + o] * (int32_t)(rnd() % 256);
            }
            check_mesh(rv, n, n, n, 1 + t % 2, &nv, &nf);
            cases++;
        }
        std::vector<int32_t> empty(6 * 8, 0), inside(6 * 8, 0);
        for (int o = 0; o < 8; o++) inside[o] = -5, inside[8 + o] = 2;
        check_mesh(empty, 2, 2, 2, 1, &nv, &nf);
        CHECK(nv == 0 && nf == 0);
        check_mesh(inside, 2, 2, 2, 2, &nv, &nf);
        CHECK(nv == 0 && nf == 0);
        cases += 4;
    }
    // argument errors come before any access
    {
        const double o[3] = {0, 0, 0}, bad[3] = {0, NAN, 0};
        int32_t v8[48] = {0};
        int nv, nf;
        CHECK(slam_tsdf_mesh_host(v8, 1, 2, 2, o, 1.0, 1, nullptr, nullptr, nullptr, 0, 0, &nv, &nf) == SLAM_E_UNSUPPORTED);
        CHECK(slam_tsdf_mesh_host(v8, 2, 2, 2049, o, 1.0, 1, nullptr, nullptr, nullptr, 0, 0, &nv, &nf) == SLAM_E_UNSUPPORTED);
        CHECK(slam_tsdf_mesh_host(v8, 2048, 2048, 512, o, 1.0, 1, nullptr, nullptr, nullptr, 0, 0, &nv, &nf) == SLAM_E_UNSUPPORTED);
        CHECK(slam_tsdf_mesh_host(v8, 2, 2, 2, bad, 1.0, 1, nullptr, nullptr, nullptr, 0, 0, &nv, &nf) == SLAM_E_INVALID_ARG);
        CHECK(slam_tsdf_mesh_host(v8, 2, 2, 2, o, 0.0, 1, nullptr, nullptr, nullptr, 0, 0, &nv, &nf) == SLAM_E_INVALID_ARG);
        CHECK(slam_tsdf_mesh_host(v8, 2, 2, 2, o, 1.0, 0, nullptr, nullptr, nullptr, 0, 0, &nv, &nf) == SLAM_E_INVALID_ARG);
        Scene s = make_scene(2, 2, 2, 1, 1);
        s.P[5] = INFINITY;
        CHECK(slam_tsdf_integrate_host(v8, 2, 2, 2, o, 1.0, 1.0, s.frames.data(), 2, s.w, s.h, 1, s.idx.data(), s.inv.data(),
                                       s.P.data(), 1) == SLAM_E_INVALID_ARG);
        s.P[5] = 1.0;
        CHECK(slam_tsdf_integrate_host(v8, 2, 2, 2, o, 1.0, -1.0, s.frames.data(), 2, s.w, s.h, 1, s.idx.data(), s.inv.data(),
                                       s.P.data(), 1) == SLAM_E_INVALID_ARG);
        s.idx[0] = 2;
        CHECK(slam_tsdf_integrate_host(v8, 2, 2, 2, o, 1.0, 1.0, s.frames.data(), 2, s.w, s.h, 1, s.idx.data(), s.inv.data(),
                                       s.P.data(), 1) == SLAM_E_INVALID_ARG);
        CHECK(slam_tsdf_integrate_host(v8, 2, 2, 2, o, 1.0, 1.0, nullptr, 1, 4, 4, 1, nullptr, nullptr, nullptr, 0) == SLAM_OK);
    }
    if (g_fail) {
        printf("%d failures\n", g_fail);
        return 1;
    }
    printf("OK: %d cases\n", cases);
    return 0;
}

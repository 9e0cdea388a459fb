// Plane-sweep stereo on the host: slam_mvs_depth_host, the twin of mvs_census +
// mvs_sweep (mvs.hip) for one reference frame.  It needs no context and no device;
// the arithmetic is mvs_math.h's, so the results equal the device's bit for bit.
// Rows are dealt to up to 16 threads; a thread sweeps the planes over its band.
#include "../../include/slamhip.h"
#include "mvs_math.h"

#include <algorithm>
#include <thread>
#include <vector>

namespace slamhip {

// 9 x 7 census of one frame, coordinates clamped to the image
void mvs_census_host(const uint8_t* img, int w, int h, size_t step, int channels, uint64_t* out)
{
    std::vector<uint8_t> g((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) g[(size_t)y * w + x] = (uint8_t)mvs_gray(img + (size_t)y * step + (size_t)x * channels, channels);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const uint8_t c = g[(size_t)y * w + x];
            uint64_t bits = 0;
            int b = 0;
            for (int dy = -kMvsCensusRy; dy <= kMvsCensusRy; dy++)
                for (int dx = -kMvsCensusRx; dx <= kMvsCensusRx; dx++) {
                    if (dx == 0 && dy == 0) continue;
                    const uint8_t v = g[(size_t)mvs_clamp(y + dy, 0, h - 1) * w + mvs_clamp(x + dx, 0, w - 1)];
                    if (v < c) bits |= 1ull << b;
                    b++;
                }
            out[(size_t)y * w + x] = bits;
        }
}

int mvs_check_args(int S, int w, int h, int channels, const double* M, const double* v, const double* planes, int D,
                   int radius, int uniq, int min_views)
{
    if (S < 1 || S > kMvsMaxSources || D < kMvsMinPlanes || D > kMvsMaxPlanes || radius < 0 || radius > kMvsMaxRadius ||
        uniq < 1 || uniq > 100 || min_views < 1 || min_views > S || w < 1 || h < 1 || (channels != 1 && channels != 3) ||
        !M || !v || !planes)
        return SLAM_E_INVALID_ARG;
    if (w > kMvsMaxWidth) return SLAM_E_UNSUPPORTED;
    for (int i = 0; i < 9 * S; i++)
        if (!mvs_finite(M[i])) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < 3 * S; i++)
        if (!mvs_finite(v[i])) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < D; i++)
        if (!mvs_finite(planes[i])) return SLAM_E_INVALID_ARG;
    return SLAM_OK;
}

// The plane loop of one reference over census maps cen ((S + 1) x h x w, the reference first): rows are
// dealt to up to 16 threads, a thread sweeps the planes over its band and hands sink(x, y, d, C, nvalid)
// every pixel of every plane, planes in order.  Shared by slam_mvs_depth_host and mvs_cost_volume_host.
template <class Sink>
static void sweep_bands(const uint64_t* cen, int S, int w, int h, const double* M, const double* v, const double* planes,
                        int D, int radius, Sink sink)
{
    const size_t npx = (size_t)w * h;
    const int r = radius;
    // bands of at least 16 rows: a band repeats the `radius` rows above and below it
    const int nthreads = std::max(1, std::min({16, (int)std::thread::hardware_concurrency(), (h + 15) / 16}));
    auto band = [&](int t) {
        const int y0 = (int)((long long)h * t / nthreads), y1 = (int)((long long)h * (t + 1) / nthreads);
        if (y1 <= y0) return;
        // raw rows lo .. hi (the band and the rows its windows clamp to)
        const int lo = std::max(0, y0 - r), hi = std::min(h - 1, y1 - 1 + r);
        const int nr = hi - lo + 1;
        std::vector<double> q((size_t)nr * w * S * 3);
        for (int y = lo; y <= hi; y++)
            for (int x = 0; x < w; x++)
                for (int s = 0; s < S; s++) mvs_q(M + 9 * s, x, y, &q[(((size_t)(y - lo) * w + x) * S + s) * 3]);
        std::vector<int32_t> raw((size_t)nr * w), hs((size_t)nr * w);
        std::vector<uint8_t> nval((size_t)nr * w);
        for (int d = 0; d < D; d++) {
            for (int y = lo; y <= hi; y++)
                for (int x = 0; x < w; x++) {
                    const uint64_t cr = cen[(size_t)y * w + x];
                    int32_t sum = 0;
                    int nv = 0;
                    for (int s = 0; s < S; s++) {
                        int ix, iy;
                        double h2;
                        if (mvs_project(&q[(((size_t)(y - lo) * w + x) * S + s) * 3], v + 3 * s, planes[d], w, h, &ix, &iy, &h2)) {
                            sum += mvs_popc64(cr ^ cen[(size_t)(s + 1) * npx + (size_t)iy * w + ix]);
                            nv++;
                        } else {
                            sum += kMvsInvalidCost;
                        }
                    }
                    raw[(size_t)(y - lo) * w + x] = sum;
                    nval[(size_t)(y - lo) * w + x] = (uint8_t)nv;
                }
            for (int y = 0; y < nr; y++)
                for (int x = 0; x < w; x++) {
                    int32_t a = 0;
                    for (int dx = -r; dx <= r; dx++) a += raw[(size_t)y * w + mvs_clamp(x + dx, 0, w - 1)];
                    hs[(size_t)y * w + x] = a;
                }
            for (int y = y0; y < y1; y++)
                for (int x = 0; x < w; x++) {
                    int32_t C = 0;
                    for (int dy = -r; dy <= r; dy++) C += hs[(size_t)(mvs_clamp(y + dy, 0, h - 1) - lo) * w + x];
                    sink(x, y, d, C, (int32_t)nval[(size_t)(y - lo) * w + x]);
                }
        }
    };
    if (nthreads == 1) {
        band(0);
    } else {
        std::vector<std::thread> pool;
        for (int t = 1; t < nthreads; t++) pool.emplace_back(band, t);
        band(0);
        for (auto& th : pool) th.join();
    }
}

static std::vector<uint64_t> census_all(const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h, size_t step,
                                        int channels)
{
    const size_t npx = (size_t)w * h;
    std::vector<uint64_t> cen((size_t)(S + 1) * npx);
    mvs_census_host(ref, w, h, step, channels, cen.data());
    for (int s = 0; s < S; s++) mvs_census_host(srcs[s], w, h, step, channels, cen.data() + (size_t)(s + 1) * npx);
    return cen;
}

// C and nvalid of one reference in the public layout (h x w x D, the plane innermost); arguments checked by the caller
void mvs_cost_volume_host(const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h, size_t step, int channels,
                          const double* M, const double* v, const double* planes, int D, int radius, uint16_t* C,
                          uint8_t* nvalid)
{
    std::vector<uint64_t> cen = census_all(ref, srcs, S, w, h, step, channels);
    sweep_bands(cen.data(), S, w, h, M, v, planes, D, radius, [&](int x, int y, int d, int32_t c, int32_t nv) {
        const size_t o = ((size_t)y * w + x) * D + d;
        C[o] = (uint16_t)c;
        nvalid[o] = (uint8_t)nv;
    });
}

}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_mvs_depth_host(const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h, size_t step,
                                   int channels, const double* M, const double* v, const double* planes, int D,
                                   int radius, int uniq, int min_views, int16_t* plane, int32_t* cost, float* inv_depth)
{
    if (!ref || !srcs || !plane || !cost || !inv_depth) return SLAM_E_INVALID_ARG;
    if (int rc = mvs_check_args(S, w, h, channels, M, v, planes, D, radius, uniq, min_views)) return rc;
    if (step < (size_t)w * channels) return SLAM_E_INVALID_ARG;
    for (int s = 0; s < S; s++)
        if (!srcs[s]) return SLAM_E_INVALID_ARG;

    const size_t npx = (size_t)w * h;
    std::vector<uint64_t> cen = census_all(ref, srcs, S, w, h, step, channels);
    std::vector<MvsPixel> st(npx);
    for (auto& p : st) mvs_pixel_init(p);
    sweep_bands(cen.data(), S, w, h, M, v, planes, D, radius,
                [&](int x, int y, int d, int32_t C, int32_t nv) { mvs_pixel_update(st[(size_t)y * w + x], d, C, nv); });
    for (size_t i = 0; i < npx; i++) mvs_pixel_finish(st[i], planes, D, uniq, min_views, &plane[i], &cost[i], &inv_depth[i]);
    return SLAM_OK;
}


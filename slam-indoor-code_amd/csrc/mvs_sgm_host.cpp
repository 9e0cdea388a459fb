// Semi-global aggregation on the host: slam_mvs_sgm_aggregate_host and
// slam_mvs_depth_sgm_host, the twins of sgm_path + sgm_winner (mvs_sgm.hip) over
// the volume of mvs_host.cpp.  No context, no device; the arithmetic is
// mvs_sgm_math.h's, so the results equal the device's bit for bit.  The directions
// run one after the other; the scan lines of a direction touch disjoint pixels and
// are dealt to up to 16 threads.
#include "../../include/slamhip.h"
#include "mvs_sgm_math.h"

#include <algorithm>
#include <thread>
#include <vector>

namespace slamhip {

int mvs_check_args(int S, int w, int h, int channels, const double* M, const double* v, const double* planes, int D,
                   int radius, int uniq, int min_views);   // mvs_host.cpp
void mvs_cost_volume_host(const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h, size_t step, int channels,
                          const double* M, const double* v, const double* planes, int D, int radius, uint16_t* C,
                          uint8_t* nvalid);                 // mvs_host.cpp

namespace {

// one scan line: L_r along it, added into S
void sgm_walk(const uint16_t* C, int32_t* S, int w, int h, int D, int dx, int dy, int line, uint32_t P1, uint32_t P2,
              uint32_t* prev, uint32_t* cur)
{
    int x, y, len;
    sgm_line(dx, dy, w, h, line, &x, &y, &len);
    uint32_t m = 0;
    for (int i = 0; i < len; i++, x += dx, y += dy) {
        const size_t o = ((size_t)y * w + x) * D;
        uint32_t mn = kSgmAbsent;
        for (int d = 0; d < D; d++) {
            const uint32_t c = C[o + d];
            const uint32_t L = i == 0 ? c
                                      : sgm_step(c, prev[d], d > 0 ? prev[d - 1] : kSgmAbsent,
                                                 d + 1 < D ? prev[d + 1] : kSgmAbsent, m, P1, P2);
            cur[d] = L;
            mn = L < mn ? L : mn;
            S[o + d] += (int32_t)L;
        }
        m = mn;
        std::swap(prev, cur);
    }
}

void sgm_aggregate_one(const uint16_t* C, int w, int h, int D, int P1, int P2, int paths, int32_t* S)
{
    std::fill(S, S + (size_t)w * h * D, 0);
    for (int r = 0; r < paths; r++) {
        int dx, dy;
        sgm_dir(r, &dx, &dy);
        const int lines = sgm_line_count(dx, dy, w, h);
        const int nthreads = std::max(1, std::min({16, (int)std::thread::hardware_concurrency(), lines / 8}));
        auto work = [&](int t) {
            std::vector<uint32_t> buf(2 * (size_t)D);
            for (int i = t; i < lines; i += nthreads)
                sgm_walk(C, S, w, h, D, dx, dy, i, (uint32_t)P1, (uint32_t)P2, buf.data(), buf.data() + D);
        };
        if (nthreads == 1) {
            work(0);
        } else {
            std::vector<std::thread> pool;
            for (int t = 1; t < nthreads; t++) pool.emplace_back(work, t);
            work(0);
            for (auto& th : pool) th.join();
        }
    }
}

}  // namespace
}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_mvs_sgm_aggregate_host(const uint16_t* C, int n, int w, int h, int D, int P1, int P2, int paths,
                                           int32_t* S)
{
    if (!sgm_aggregate_args_ok(n, w, h, D, P1, P2, paths)) return SLAM_E_INVALID_ARG;
    if (w > kMvsMaxWidth) return SLAM_E_UNSUPPORTED;
    if (n == 0) return SLAM_OK;
    if (!C || !S) return SLAM_E_INVALID_ARG;
    const size_t vol = (size_t)w * h * D;
    for (int i = 0; i < n; i++) sgm_aggregate_one(C + i * vol, w, h, D, P1, P2, paths, S + i * vol);
    return SLAM_OK;
}

extern "C" int slam_mvs_cost_volume_host(const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h, size_t step,
                                         int channels, const double* M, const double* v, const double* planes, int D,
                                         int radius, uint16_t* C, uint8_t* nvalid)
{
    if (!ref || !srcs || !C || !nvalid) return SLAM_E_INVALID_ARG;
    if (int rc = mvs_check_args(S, w, h, channels, M, v, planes, D, radius, 1, 1)) return rc;
    if (step < (size_t)w * channels) return SLAM_E_INVALID_ARG;
    for (int s = 0; s < S; s++)
        if (!srcs[s]) return SLAM_E_INVALID_ARG;
    mvs_cost_volume_host(ref, srcs, S, w, h, step, channels, M, v, planes, D, radius, C, nvalid);
    return SLAM_OK;
}

extern "C" int slam_mvs_depth_sgm_host(const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h, size_t step,
                                       int channels, const double* M, const double* v, const double* planes, int D,
                                       int radius, int uniq, int min_views, int p1, int p2, int paths, int16_t* plane,
                                       int32_t* cost, float* inv_depth)
{
    if (!ref || !srcs || !plane || !cost || !inv_depth) return SLAM_E_INVALID_ARG;
    if (int rc = mvs_check_args(S, w, h, channels, M, v, planes, D, radius, uniq, min_views)) return rc;
    if (!sgm_penalties_ok(p1, p2, paths) || step < (size_t)w * channels) return SLAM_E_INVALID_ARG;
    for (int s = 0; s < S; s++)
        if (!srcs[s]) return SLAM_E_INVALID_ARG;
    const size_t npx = (size_t)w * h;
    std::vector<uint16_t> C(npx * D);
    std::vector<uint8_t> nv(npx * D);
    std::vector<int32_t> agg(npx * D);
    mvs_cost_volume_host(ref, srcs, S, w, h, step, channels, M, v, planes, D, radius, C.data(), nv.data());
    sgm_aggregate_one(C.data(), w, h, D, sgm_effective(p1, radius, S), sgm_effective(p2, radius, S), paths, agg.data());
    const int nthreads = std::max(1, std::min({16, (int)std::thread::hardware_concurrency(), (h + 15) / 16}));
    auto band = [&](int t) {
        const size_t i0 = npx * t / nthreads, i1 = npx * (t + 1) / nthreads;
        for (size_t i = i0; i < i1; i++) {
            MvsPixel st;
            mvs_pixel_init(st);
            for (int d = 0; d < D; d++) mvs_pixel_update(st, d, agg[i * D + d], nv[i * D + d]);
            mvs_pixel_finish(st, planes, D, uniq, min_views, &plane[i], &cost[i], &inv_depth[i]);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; t++) pool.emplace_back(band, t);
    band(0);
    for (auto& th : pool) th.join();
    return SLAM_OK;
}

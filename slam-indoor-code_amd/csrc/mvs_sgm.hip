// Semi-global aggregation of the plane-sweep cost volume on the device (DESIGN.md
// section 28; tests/mvs_sgm_ref.py is the definition, mvs_sgm_math.h the shared
// arithmetic).  The volume comes from mvs_volume (mvs.hip: mvs_sweep's plane loop
// with another sink).
//
//   sgm_path    one wave64 per scan line of a direction, every direction and every
//               reference of a group in one launch.  Lane l holds the planes l, l + 64,
//               ... (K = ceil(D / 64) registers), so a pixel's costs arrive as K
//               contiguous 128-byte reads and L_r leaves as K contiguous 256-byte
//               integer atomic adds into S.  The neighbours d - 1 and d + 1 are lane
//               rotations, the minimum a butterfly over the wave: no LDS, no barrier.
//               Integer adds commute, so the directions need no order among them.
//   sgm_winner  a thread per pixel streams S (and nvalid) in plane order through the
//               winner rule of mvs_sweep (MvsPixel).
#include "slamhip_internal.h"
#include "mvs_sgm_math.h"

#include <algorithm>
#include <cstring>

namespace slamhip {

int mvs_check_args(int S, int w, int h, int channels, const double* M, const double* v, const double* planes, int D,
                   int radius, int uniq, int min_views);   // mvs_host.cpp

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr size_t kSgmDefaultBudget = (size_t)8 << 30;      // bytes of volume + counts + S a group of references may take

struct SgmLines {
    int first[9];        // first[r]: the lines before direction r; first[paths]: all of them
};

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)v, o);
        v = t < v ? t : v;
    }
    return v;
}

template <int K>
__global__ __launch_bounds__(kThreads) void sgm_path(const uint16_t* __restrict__ C, int32_t* __restrict__ S, int w, int h,
                                                     int D, uint32_t P1, uint32_t P2, const uint32_t* __restrict__ pen,
                                                     int paths, SgmLines ln)
{
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * kWaves + (threadIdx.x >> 6);       // uniform in the wave
    if (g >= ln.first[paths]) return;
    int r = 0;
    while (g >= ln.first[r + 1]) r++;
    const int n = blockIdx.y;
    if (pen) {
        P1 = pen[2 * n];
        P2 = pen[2 * n + 1];
    }
    int dx, dy, x, y, len;
    sgm_dir(r, &dx, &dy);
    sgm_line(dx, dy, w, h, g - ln.first[r], &x, &y, &len);
    const size_t vol = (size_t)w * h * D;
    const uint16_t* Cn = C + (size_t)n * vol;
    int32_t* Sn = S + (size_t)n * vol;
    const ptrdiff_t stride = ((ptrdiff_t)dy * w + dx) * D;

    bool ok[K];
#pragma unroll
    for (int j = 0; j < K; j++) ok[j] = j * 64 + lane < D;
    const int up = (lane + 63) & 63, down = (lane + 1) & 63;

    size_t o = ((size_t)y * w + x) * D + lane;
    uint32_t prev[K], cur[K];
    uint32_t mn = kSgmAbsent;
#pragma unroll
    for (int j = 0; j < K; j++) {
        prev[j] = ok[j] ? (uint32_t)Cn[o + j * 64] : kSgmAbsent;
        mn = prev[j] < mn ? prev[j] : mn;
        if (ok[j]) atomicAdd(&Sn[o + j * 64], (int32_t)prev[j]);
    }
    uint32_t m = wave_min(mn);
    if (len > 1) {
#pragma unroll
        for (int j = 0; j < K; j++) cur[j] = ok[j] ? (uint32_t)Cn[o + stride + j * 64] : 0u;
    }
    for (int i = 1; i < len; i++) {
        o += stride;
        uint32_t c[K];
#pragma unroll
        for (int j = 0; j < K; j++) c[j] = cur[j];
        if (i + 1 < len) {                     // the next pixel's costs are on their way while this one is computed
#pragma unroll
            for (int j = 0; j < K; j++) cur[j] = ok[j] ? (uint32_t)Cn[o + stride + j * 64] : 0u;
        }
        uint32_t lo[K], hi[K];
#pragma unroll
        for (int j = 0; j < K; j++) {
            lo[j] = (uint32_t)__shfl((int)prev[j], up);
            hi[j] = (uint32_t)__shfl((int)prev[j], down);
        }
        mn = kSgmAbsent;
        uint32_t L[K];
#pragma unroll
        for (int j = 0; j < K; j++) {
            // plane d - 1 lives one lane down, or for lane 0 in lane 63's register j - 1; d + 1 likewise
            const uint32_t below = lane > 0 ? lo[j] : (j > 0 ? lo[j > 0 ? j - 1 : 0] : kSgmAbsent);
            const uint32_t above = lane < 63 ? hi[j] : (j < K - 1 ? hi[j < K - 1 ? j + 1 : 0] : kSgmAbsent);
            L[j] = ok[j] ? sgm_step(c[j], prev[j], below, above, m, P1, P2) : kSgmAbsent;
            mn = L[j] < mn ? L[j] : mn;
        }
#pragma unroll
        for (int j = 0; j < K; j++) {
            if (ok[j]) atomicAdd(&Sn[o + j * 64], (int32_t)L[j]);
            prev[j] = L[j];
        }
        m = wave_min(mn);
    }
}

template <bool Vec>
__global__ __launch_bounds__(kThreads) void sgm_winner(const int32_t* __restrict__ S, const uint8_t* __restrict__ nvalid,
                                                       const double* __restrict__ planes, size_t npx, int D, int uniq,
                                                       int min_views, int16_t* __restrict__ plane,
                                                       int32_t* __restrict__ cost, float* __restrict__ inv)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= npx) return;
    const size_t px = (size_t)blockIdx.y * npx + i;
    const int32_t* s = S + px * D;
    const uint8_t* nv = nvalid + px * D;
    MvsPixel st;
    mvs_pixel_init(st);
    if (Vec) {                                 // D a multiple of 4: 16 bytes of S and 4 valid counts per load
        for (int d = 0; d < D; d += 4) {
            const int4 a = *reinterpret_cast<const int4*>(s + d);
            const uint32_t b = *reinterpret_cast<const uint32_t*>(nv + d);
            mvs_pixel_update(st, d, a.x, (int32_t)(b & 255u));
            mvs_pixel_update(st, d + 1, a.y, (int32_t)((b >> 8) & 255u));
            mvs_pixel_update(st, d + 2, a.z, (int32_t)((b >> 16) & 255u));
            mvs_pixel_update(st, d + 3, a.w, (int32_t)(b >> 24));
        }
    } else {
        for (int d = 0; d < D; d++) mvs_pixel_update(st, d, s[d], (int32_t)nv[d]);
    }
    mvs_pixel_finish(st, planes + (size_t)blockIdx.y * D, D, uniq, min_views, &plane[px], &cost[px], &inv[px]);
}

hipError_t launch_paths(hipStream_t s, const uint16_t* C, int n, int w, int h, int D, int P1, int P2, const uint32_t* pen,
                        int paths, int32_t* S)
{
    hipError_t rc = hipMemsetAsync(S, 0, sizeof(int32_t) * (size_t)n * w * h * D, s);
    if (rc != hipSuccess) return rc;
    SgmLines ln;
    ln.first[0] = 0;
    for (int r = 0; r < 8; r++) {
        int dx, dy;
        sgm_dir(r, &dx, &dy);
        ln.first[r + 1] = ln.first[r] + (r < paths ? sgm_line_count(dx, dy, w, h) : 0);
    }
    const dim3 grid((ln.first[paths] + kWaves - 1) / kWaves, n);
    switch ((D + 63) / 64) {
    case 1: hipLaunchKernelGGL(sgm_path<1>, grid, dim3(kThreads), 0, s, C, S, w, h, D, (uint32_t)P1, (uint32_t)P2, pen, paths, ln); break;
    case 2: hipLaunchKernelGGL(sgm_path<2>, grid, dim3(kThreads), 0, s, C, S, w, h, D, (uint32_t)P1, (uint32_t)P2, pen, paths, ln); break;
    case 3: hipLaunchKernelGGL(sgm_path<3>, grid, dim3(kThreads), 0, s, C, S, w, h, D, (uint32_t)P1, (uint32_t)P2, pen, paths, ln); break;
    default: hipLaunchKernelGGL(sgm_path<4>, grid, dim3(kThreads), 0, s, C, S, w, h, D, (uint32_t)P1, (uint32_t)P2, pen, paths, ln); break;
    }
    return hipGetLastError();
}

hipError_t sgm_events(slam_ctx* c)
{
    for (auto& e : c->sgm_ev)
        if (!e) {
            const hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return rc;
        }
    return hipSuccess;
}

double elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (double)ms : 0.0;
}

}  // namespace
}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_mvs_sgm_last_timing(slam_ctx* c, double* ms)
{
    if (!c || !ms) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < 3; i++) ms[i] = c->sgm_ms[i];
    return SLAM_OK;
}

extern "C" int slam_mvs_sgm_set_budget(slam_ctx* c, size_t bytes)
{
    if (!c) return SLAM_E_INVALID_ARG;
    c->sgm_budget = bytes;
    return SLAM_OK;
}

extern "C" int slam_mvs_cost_volume_dev(slam_ctx* c, void* stream, const uint8_t* d_frames, int nframes, int w, int h,
                                        int channels, int nref, const int32_t* ref_idx, const int32_t* nsrc,
                                        const int32_t* src_idx, const double* M, const double* v, const double* planes,
                                        int D, int radius, uint16_t* d_C, uint8_t* d_nvalid)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (nref > 0 && (!d_C || !d_nvalid)) return set_err(c, SLAM_E_INVALID_ARG, "mvs volume: null output");
    MvsBatchOut out;
    out.C = d_C;
    out.nvalid = d_nvalid;
    double ms[2] = {0, 0};
    const int rc = mvs_batch_run(c, stream, d_frames, nframes, w, h, channels, nref, ref_idx, nsrc, src_idx, M, v, planes, D,
                                 radius, 1, 1, out, false, ms);
    if (rc == SLAM_OK) c->sgm_ms[0] = ms[1];
    return rc;
}

extern "C" int slam_mvs_sgm_aggregate_dev(slam_ctx* c, void* stream, const uint16_t* d_C, int n, int w, int h, int D, int P1,
                                          int P2, int paths, int32_t* d_S)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!sgm_aggregate_args_ok(n, w, h, D, P1, P2, paths))
        return set_err(c, SLAM_E_INVALID_ARG, "sgm aggregate: n 0..65535, D 4..256, 0 <= P1 <= P2 <= 65535 - 12544, paths 4 or 8");
    if (w > kMvsMaxWidth) return set_err(c, SLAM_E_UNSUPPORTED, "sgm aggregate: volumes wider than 4096 pixels");
    if (n == 0) return SLAM_OK;
    if (!d_C || !d_S) return set_err(c, SLAM_E_INVALID_ARG, "sgm aggregate: null argument");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    SLAM_HIP(c, sgm_events(c));
    SLAM_HIP(c, hipEventRecord(c->sgm_ev[0], s));
    SLAM_HIP(c, launch_paths(s, d_C, n, w, h, D, P1, P2, nullptr, paths, d_S));
    SLAM_HIP(c, hipEventRecord(c->sgm_ev[1], s));
    if (int rc = stream_sync(c, s)) return rc;
    c->sgm_ms[1] = elapsed(c->sgm_ev[0], c->sgm_ev[1]);
    return SLAM_OK;
}

extern "C" int slam_mvs_depth_sgm_batch_dev(slam_ctx* c, void* stream, const uint8_t* d_frames, int nframes, int w, int h,
                                            int channels, int nref, const int32_t* ref_idx, const int32_t* nsrc,
                                            const int32_t* src_idx, const double* M, const double* v,
                                            const double* planes, int D, int radius, int uniq, int min_views, int p1, int p2,
                                            int paths, int16_t* d_plane, int32_t* d_cost, float* d_inv_depth)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!sgm_penalties_ok(p1, p2, paths)) return set_err(c, SLAM_E_INVALID_ARG, "mvs sgm: 0 <= p1 <= p2 <= 255, paths 4 or 8");
    MvsBatchOut win;
    win.plane = d_plane;
    win.cost = d_cost;
    win.inv = d_inv_depth;
    double ms[2] = {0, 0};
    if (int rc = mvs_batch_run(c, stream, d_frames, nframes, w, h, channels, nref, ref_idx, nsrc, src_idx, M, v, planes, D,
                               radius, uniq, min_views, win, true, ms))
        return rc;
    if (nref == 0) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    SLAM_HIP(c, sgm_events(c));
    const size_t npx = (size_t)w * h, vol = npx * D;
    // references per group: as many as the budget holds, one at the least
    const size_t budget = c->sgm_budget ? c->sgm_budget : kSgmDefaultBudget;
    auto plan = [&](size_t g, Slot<uint16_t>* sC, Slot<uint8_t>* sN, Slot<int32_t>* sS, Slot<double>* sW, Slot<uint32_t>* sP) {
        DevLayout lay;
        *sC = lay.add<uint16_t>(g * vol);
        *sN = lay.add<uint8_t>(g * vol);
        *sS = lay.add<int32_t>(g * vol);
        *sW = lay.add<double>(g * D);
        *sP = lay.add<uint32_t>(g * 2);
        return lay;
    };
    Slot<uint16_t> sC;
    Slot<uint8_t> sN;
    Slot<int32_t> sS;
    Slot<double> sW;
    Slot<uint32_t> sP;
    size_t group = std::min<size_t>((size_t)nref, std::max<size_t>(1, budget / (7 * vol)));
    while (group > 1 && plan(group, &sC, &sN, &sS, &sW, &sP).bytes() > budget) group--;
    DevMem m;
    SLAM_HIP(c, m.bind(c->mvs_sgm, plan(group, &sC, &sN, &sS, &sW, &sP)));
    double t_vol = 0, t_path = 0, t_win = 0;
    std::vector<uint32_t> pen(2 * group);
    const bool vec = D % 4 == 0;
    for (size_t g0 = 0; g0 < (size_t)nref; g0 += group) {
        const int g = (int)std::min(group, (size_t)nref - g0);
        MvsBatchOut out;
        out.C = m.ptr(sC);
        out.nvalid = m.ptr(sN);
        if (int rc = mvs_batch_run(c, s, d_frames, nframes, w, h, channels, g, ref_idx + g0, nsrc + g0, src_idx + 4 * g0,
                                   M + 36 * g0, v + 12 * g0, planes + g0 * D, D, radius, uniq, min_views, out, false, ms))
            return rc;
        t_vol += ms[1];
        for (int i = 0; i < g; i++) {
            pen[2 * i] = (uint32_t)sgm_effective(p1, radius, nsrc[g0 + i]);
            pen[2 * i + 1] = (uint32_t)sgm_effective(p2, radius, nsrc[g0 + i]);
        }
        SLAM_HIP(c, m.upload(sW, planes + g0 * D, (size_t)g * D, s));
        SLAM_HIP(c, m.upload(sP, pen.data(), (size_t)g * 2, s));
        SLAM_HIP(c, hipEventRecord(c->sgm_ev[0], s));
        SLAM_HIP(c, launch_paths(s, m.ptr(sC), g, w, h, D, 0, 0, m.ptr(sP), paths, m.ptr(sS)));
        SLAM_HIP(c, hipEventRecord(c->sgm_ev[1], s));
        const dim3 grid((unsigned)((npx + kThreads - 1) / kThreads), g);
        if (vec)
            hipLaunchKernelGGL(sgm_winner<true>, grid, dim3(kThreads), 0, s, m.ptr(sS), m.ptr(sN), m.ptr(sW), npx, D, uniq,
                               min_views, d_plane + g0 * npx, d_cost + g0 * npx, d_inv_depth + g0 * npx);
        else
            hipLaunchKernelGGL(sgm_winner<false>, grid, dim3(kThreads), 0, s, m.ptr(sS), m.ptr(sN), m.ptr(sW), npx, D, uniq,
                               min_views, d_plane + g0 * npx, d_cost + g0 * npx, d_inv_depth + g0 * npx);
        SLAM_HIP(c, hipGetLastError());
        SLAM_HIP(c, hipEventRecord(c->sgm_ev[2], s));
        if (int rc = stream_sync(c, s)) return rc;      // the scratch and the host blocks are reused by the next group
        t_path += elapsed(c->sgm_ev[0], c->sgm_ev[1]);
        t_win += elapsed(c->sgm_ev[1], c->sgm_ev[2]);
    }
    c->sgm_ms[0] = t_vol;
    c->sgm_ms[1] = t_path;
    c->sgm_ms[2] = t_win;
    return SLAM_OK;
}

extern "C" int slam_mvs_depth_sgm(slam_ctx* c, const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h,
                                  size_t step, int channels, const double* M, const double* v, const double* planes, int D,
                                  int radius, int uniq, int min_views, int p1, int p2, int paths, int16_t* plane,
                                  int32_t* cost, float* inv_depth)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!ref || !srcs || !plane || !cost || !inv_depth) return set_err(c, SLAM_E_INVALID_ARG, "mvs sgm: null argument");
    if (int rc = mvs_check_args(S, w, h, channels, M, v, planes, D, radius, uniq, min_views))
        return set_err(c, rc, "mvs sgm: bad arguments");
    if (!sgm_penalties_ok(p1, p2, paths)) return set_err(c, SLAM_E_INVALID_ARG, "mvs sgm: 0 <= p1 <= p2 <= 255, paths 4 or 8");
    if (step < (size_t)w * channels) return set_err(c, SLAM_E_INVALID_ARG, "mvs sgm: short row stride");
    for (int s = 0; s < S; s++)
        if (!srcs[s]) return set_err(c, SLAM_E_INVALID_ARG, "mvs sgm: null source");
    SLAM_HIP(c, hipSetDevice(c->device));
    const size_t row = (size_t)w * channels, fb = row * h, npx = (size_t)w * h;
    DevLayout lay;
    const auto s_frames = lay.add<uint8_t>((size_t)(S + 1) * fb);
    const auto s_cost = lay.add<int32_t>(npx);
    const auto s_inv = lay.add<float>(npx);
    const auto s_plane = lay.add<int16_t>(npx);
    DevMem m;
    SLAM_HIP(c, m.bind(c->mvs_in, lay));
    uint8_t* d = m.ptr(s_frames);
    for (int f = 0; f <= S; f++)
        SLAM_HIP(c, hipMemcpy2DAsync(d + f * fb, row, f == 0 ? ref : srcs[f - 1], step, row, h, hipMemcpyHostToDevice,
                                     c->stream));
    const int32_t ref_idx = 0, nsrc = S, src_idx[4] = {1, 2, 3, 4};
    double M4[36] = {0}, v4[12] = {0};
    memcpy(M4, M, sizeof(double) * 9 * S);
    memcpy(v4, v, sizeof(double) * 3 * S);
    if (int rc = slam_mvs_depth_sgm_batch_dev(c, c->stream, d, S + 1, w, h, channels, 1, &ref_idx, &nsrc, src_idx, M4, v4,
                                              planes, D, radius, uniq, min_views, p1, p2, paths, m.ptr(s_plane),
                                              m.ptr(s_cost), m.ptr(s_inv)))
        return rc;
    SLAM_HIP(c, m.download(cost, s_cost, c->stream));
    SLAM_HIP(c, m.download(inv_depth, s_inv, c->stream));
    SLAM_HIP(c, m.download(plane, s_plane, c->stream));
    return stream_sync(c, c->stream);
}

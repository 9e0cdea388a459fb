// Plane-sweep stereo on the device (tests/mvs_ref.py is the
// definition of every value computed here, mvs_math.h the shared arithmetic):
//
//   mvs_census  BGR / gray frame -> gray tile (+ 4 x 3 halo, clamped) in LDS -> the
//               62-bit 9 x 7 census of every pixel, one 8-byte store per pixel.  One
//               launch covers every distinct frame of a call.
//   mvs_sweep   a workgroup owns 32 x 16 reference pixels and loops over the planes.
//               Per plane every thread projects its share of the tile + radius halo
//               into each source, gathers the source census through L2 and writes
//               the Hamming sum (and the valid count) to LDS; the box sum is
//               separable (rows, then columns); the winner rule streams in
//               registers (MvsPixel), so the cost volume never exists.  The part of
//               the projection no plane changes (q) is computed once per position.
//   mvs_volume  the same plane loop (mvs_plane_loop) with another sink: C and nvalid
//               of every plane are stored, the plane index innermost, for the
//               semi-global aggregation of mvs_sgm.hip.
//   mvs_filter  the pairwise consistency test, one thread per pixel, one 64-bit
//               ballot per row segment.
//   mvs_count / mvs_emit
//               popcounts per row, an exclusive scan, points written in mask order
//               (raster order, map after map).  No atomics: the idea of fast_emit.
#include "slamhip_internal.h"
#include "mvs_math.h"

#include <algorithm>
#include <cstring>

namespace slamhip {

int mvs_check_args(int S, int w, int h, int channels, const double* M, const double* v, const double* planes, int D,
                   int radius, int uniq, int min_views);   // mvs_host.cpp

namespace {

constexpr int kThreads = 256;

// ---- census ------------------------------------------------------------------------

constexpr int kCenTW = 64, kCenTH = 16;
constexpr int kCenLW = kCenTW + 2 * kMvsCensusRx, kCenLH = kCenTH + 2 * kMvsCensusRy;   // 72 x 22
static_assert(kCenTW * kCenTH == 4 * kThreads, "four pixels per thread");

__global__ __launch_bounds__(kThreads) void mvs_census(const uint8_t* __restrict__ frames, size_t frame_stride,
                                                       int channels, int w, int h, const int32_t* __restrict__ list,
                                                       uint64_t* __restrict__ out)
{
    __shared__ uint8_t g[kCenLH][kCenLW + 4];
    const int tid = threadIdx.x;
    const int slot = blockIdx.z;
    const int f = list ? list[slot] : slot;
    const uint8_t* img = frames + (size_t)f * frame_stride;
    const int X0 = blockIdx.x * kCenTW, Y0 = blockIdx.y * kCenTH;
    for (int i = tid; i < kCenLH * kCenLW; i += kThreads) {
        const int ly = i / kCenLW, lx = i - ly * kCenLW;
        const int X = mvs_clamp(X0 - kMvsCensusRx + lx, 0, w - 1), Y = mvs_clamp(Y0 - kMvsCensusRy + ly, 0, h - 1);
        g[ly][lx] = (uint8_t)mvs_gray(img + ((size_t)Y * w + X) * channels, channels);
    }
    __syncthreads();
    for (int k = 0; k < 4; k++) {
        const int p = tid + k * kThreads;
        const int ly = p / kCenTW, lx = p % kCenTW;
        const int X = X0 + lx, Y = Y0 + ly;
        if (X >= w || Y >= h) continue;
        const uint32_t c = g[ly + kMvsCensusRy][lx + kMvsCensusRx];
        uint64_t bits = 0;
        int b = 0;
#pragma unroll
        for (int dy = 0; dy <= 2 * kMvsCensusRy; dy++)
#pragma unroll
            for (int dx = 0; dx <= 2 * kMvsCensusRx; dx++) {
                if (dx == kMvsCensusRx && dy == kMvsCensusRy) continue;
                bits |= (uint64_t)(g[ly + dy][lx + dx] < c ? 1u : 0u) << b;
                b++;
            }
        out[((size_t)slot * h + Y) * w + X] = bits;
    }
}

// ---- sweep -------------------------------------------------------------------------

constexpr int kSwTW = 32, kSwTH = 16;                       // reference pixels per workgroup: two rows per thread
constexpr int kSwLW = kSwTW + 2 * kMvsMaxRadius, kSwLH = kSwTH + 2 * kMvsMaxRadius;   // 38 x 22 at radius 3
constexpr int kSwPitch = kSwLW + 1;
constexpr int kSwPos = (kSwLW * kSwLH + kThreads - 1) / kThreads;                       // 4 positions per thread
static_assert(kSwTW * kSwTH == 2 * kThreads, "two pixels per thread");

// one reference of a call: census slots of the frames, the sources' M and v
struct MvsRefDesc {
    int32_t ref_slot, S;
    int32_t src_slot[kMvsMaxSources];
    int32_t pad[2];
    double M[kMvsMaxSources][9];
    double v[kMvsMaxSources][3];
};

struct SweepParams {
    const uint64_t* census;      // slots x h x w
    const MvsRefDesc* refs;
    const int32_t* list;         // the references this launch sweeps (all of one S)
    const double* planes;        // nref x D
    int w, h, D, radius, uniq, min_views;
    int16_t* plane;              // nref x h x w each (mvs_sweep)
    int32_t* cost;
    float* inv;
    uint16_t* vol_C;             // nref x h x w x D each (mvs_volume)
    uint8_t* vol_nv;
};

// The plane loop shared by mvs_sweep and mvs_volume: the sink is told its two pixels (begin), then
// every plane's box-summed cost and valid count of each in plane order (plane), then the end (finish).
template <int S, class Sink>
__device__ __forceinline__ void mvs_plane_loop(const SweepParams& p, Sink& sink)
{
    __shared__ int32_t raw[2][kSwLH][kSwPitch];     // cost | nvalid << 16 of the tile + halo, two planes
    __shared__ int32_t hs[kSwLH][kSwTW + 1];        // row sums
    __shared__ double wpl[kMvsMaxPlanes];
    const int tid = threadIdx.x;
    const int ri = p.list[blockIdx.z];
    const MvsRefDesc& R = p.refs[ri];
    const int w = p.w, h = p.h, D = p.D, r = p.radius;
    const int LW = kSwTW + 2 * r, LH = kSwTH + 2 * r, npos = LW * LH;
    const int X0 = blockIdx.x * kSwTW, Y0 = blockIdx.y * kSwTH;
    const size_t npx = (size_t)w * h;
    for (int d = tid; d < D; d += kThreads) wpl[d] = p.planes[(size_t)ri * D + d];

    const uint64_t* cref = p.census + (size_t)R.ref_slot * npx;
    const uint64_t* csrc[S];
    double sv[S][3];
#pragma unroll
    for (int s = 0; s < S; s++) {
        csrc[s] = p.census + (size_t)R.src_slot[s] * npx;
        sv[s][0] = R.v[s][0];
        sv[s][1] = R.v[s][1];
        sv[s][2] = R.v[s][2];
    }

    // this thread's positions of the tile + halo: the pixel each clamps to, its census, its q per source
    double q[kSwPos][S][3];
    uint64_t cr[kSwPos];
    int lofs[kSwPos];
#pragma unroll
    for (int k = 0; k < kSwPos; k++) {
        const int pos = tid + k * kThreads;
        lofs[k] = -1;
        cr[k] = 0;
#pragma unroll
        for (int s = 0; s < S; s++) q[k][s][0] = q[k][s][1] = q[k][s][2] = 0.0;
        if (pos < npos) {
            const int ly = pos / LW, lx = pos - ly * LW;
            const int X = mvs_clamp(X0 - r + lx, 0, w - 1), Y = mvs_clamp(Y0 - r + ly, 0, h - 1);
            lofs[k] = ly * kSwPitch + lx;
            cr[k] = cref[(size_t)Y * w + X];
#pragma unroll
            for (int s = 0; s < S; s++) mvs_q(R.M[s], X, Y, q[k][s]);
        }
    }
    const int tx = tid & (kSwTW - 1), ty = tid / kSwTW;     // pixel rows ty and ty + 8
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int X = X0 + tx, Y = Y0 + ty + 8 * j;
        sink.begin(j, X < w && Y < h, (size_t)ri * npx + (size_t)Y * w + X);
    }
    __syncthreads();

    for (int d = 0; d < D; d++) {
        const double wd = wpl[d];
        int32_t* rw = &raw[d & 1][0][0];
#pragma unroll
        for (int k = 0; k < kSwPos; k++) {
            if (lofs[k] < 0) continue;
            int32_t sum = 0, nv = 0;
#pragma unroll
            for (int s = 0; s < S; s++) {
                int ix, iy;
                double h2;
                if (mvs_project(q[k][s], sv[s], wd, w, h, &ix, &iy, &h2)) {
                    sum += mvs_popc64(cr[k] ^ csrc[s][(size_t)iy * w + ix]);
                    nv++;
                } else {
                    sum += kMvsInvalidCost;
                }
            }
            rw[lofs[k]] = sum | (nv << 16);
        }
        __syncthreads();
        for (int i = tid; i < LH * kSwTW; i += kThreads) {
            const int ly = i / kSwTW, x = i % kSwTW;
            const int32_t* row = rw + ly * kSwPitch + x;
            int32_t a = 0;
            for (int dx = 0; dx <= 2 * r; dx++) a += row[dx] & 0xffff;
            hs[ly][x] = a;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int y = ty + 8 * j;
            int32_t C = 0;
            for (int dy = 0; dy <= 2 * r; dy++) C += hs[y + dy][tx];
            sink.plane(j, d, C, rw[(y + r) * kSwPitch + tx + r] >> 16, p);
        }
        // the next plane writes the other half of raw; its first barrier orders hs
    }

#pragma unroll
    for (int j = 0; j < 2; j++) sink.finish(j, p, wpl);
}

// the winner rule streamed in registers: the cost volume never exists
struct WinnerSink {
    MvsPixel st[2];
    size_t o[2];
    bool in[2];
    __device__ __forceinline__ void begin(int j, bool inside, size_t pixel)
    {
        mvs_pixel_init(st[j]);
        in[j] = inside;
        o[j] = pixel;
    }
    __device__ __forceinline__ void plane(int j, int d, int32_t C, int32_t nv, const SweepParams&)
    {
        mvs_pixel_update(st[j], d, C, nv);
    }
    __device__ __forceinline__ void finish(int j, const SweepParams& p, const double* wpl)
    {
        if (in[j]) mvs_pixel_finish(st[j], wpl, p.D, p.uniq, p.min_views, &p.plane[o[j]], &p.cost[o[j]], &p.inv[o[j]]);
    }
};

template <int S>
__global__ __launch_bounds__(kThreads) void mvs_sweep(SweepParams p)
{
    WinnerSink sink;
    mvs_plane_loop<S>(p, sink);
}

// The volume itself, the plane index innermost.  With D a multiple of 8 (Vec) a pixel's costs are staged
// eight planes at a time in a 128-bit shift register and leave as one 16-byte store (the valid counts as
// one 8-byte store); any other D stores plane by plane.
template <bool Vec>
struct VolumeSink {
    uint32_t cw[2][4], nw[2][2];
    size_t o[2];
    bool in[2];
    __device__ __forceinline__ void begin(int j, bool inside, size_t pixel)
    {
        in[j] = inside;
        o[j] = pixel;
        cw[j][0] = cw[j][1] = cw[j][2] = cw[j][3] = nw[j][0] = nw[j][1] = 0;
    }
    __device__ __forceinline__ void plane(int j, int d, int32_t C, int32_t nv, const SweepParams& p)
    {
        if (!in[j]) return;
        if (Vec) {
            cw[j][0] = (cw[j][0] >> 16) | (cw[j][1] << 16);
            cw[j][1] = (cw[j][1] >> 16) | (cw[j][2] << 16);
            cw[j][2] = (cw[j][2] >> 16) | (cw[j][3] << 16);
            cw[j][3] = (cw[j][3] >> 16) | ((uint32_t)C << 16);
            nw[j][0] = (nw[j][0] >> 8) | (nw[j][1] << 24);
            nw[j][1] = (nw[j][1] >> 8) | ((uint32_t)nv << 24);
            if ((d & 7) == 7) {
                const size_t e = o[j] * p.D + (d - 7);       // a multiple of 8 elements: 16- and 8-byte aligned
                *reinterpret_cast<uint4*>(p.vol_C + e) = make_uint4(cw[j][0], cw[j][1], cw[j][2], cw[j][3]);
                *reinterpret_cast<uint2*>(p.vol_nv + e) = make_uint2(nw[j][0], nw[j][1]);
            }
        } else {
            const size_t e = o[j] * p.D + d;
            p.vol_C[e] = (uint16_t)C;
            p.vol_nv[e] = (uint8_t)nv;
        }
    }
    __device__ __forceinline__ void finish(int, const SweepParams&, const double*) {}
};

template <int S, bool Vec>
__global__ __launch_bounds__(kThreads) void mvs_volume(SweepParams p)
{
    VolumeSink<Vec> sink;
    mvs_plane_loop<S>(p, sink);
}

// ---- filter and emit ---------------------------------------------------------------

// one depth map of a fuse call: its frame (colours), its neighbours' maps with M and v, B and c
struct MvsMapDesc {
    int32_t frame, nnbr;
    int32_t nbr[kMvsMaxSources];
    int32_t pad[2];
    double M[kMvsMaxSources][9];
    double v[kMvsMaxSources][3];
    double B[9];
    double c[3];
};

__global__ __launch_bounds__(kThreads) void mvs_filter(const float* __restrict__ inv, const MvsMapDesc* __restrict__ maps,
                                                       int w, int h, int ntx, double eps, int min_consistent, int step,
                                                       int border, uint64_t* __restrict__ masks)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = blockIdx.z, Y = blockIdx.y * 4 + wave, X = blockIdx.x * 64 + lane;
    if (Y >= h) return;                                   // uniform in the wave
    const MvsMapDesc& mp = maps[m];
    const size_t npx = (size_t)w * h;
    bool keep = false;
    if (X < w && X % step == 0 && Y % step == 0 && X >= border && X < w - border && Y >= border && Y < h - border) {
        const float wi = inv[(size_t)m * npx + (size_t)Y * w + X];
        if (wi > 0.f) {
            int count = 0;
            for (int n = 0; n < mp.nnbr; n++) {
                double q[3], h2;
                int ix, iy;
                mvs_q(mp.M[n], X, Y, q);
                if (mvs_project(q, mp.v[n], (double)wi, w, h, &ix, &iy, &h2)) {
                    const float wj = inv[(size_t)mp.nbr[n] * npx + (size_t)iy * w + ix];
                    if (mvs_consistent(h2, wj, wi, eps)) count++;
                }
            }
            keep = count >= min_consistent;
        }
    }
    const uint64_t bal = __ballot(keep);
    if (lane == 0) masks[((size_t)m * h + Y) * ntx + blockIdx.x] = bal;
}

__global__ __launch_bounds__(kThreads) void mvs_count(const uint64_t* __restrict__ masks, int words, int32_t* __restrict__ counts)
{
    __shared__ int part[kThreads];
    const uint64_t* mk = masks + (size_t)blockIdx.x * words;
    int c = 0;
    for (int i = threadIdx.x; i < words; i += kThreads) c += __popcll(mk[i]);
    part[threadIdx.x] = c;
    __syncthreads();
    for (int d = kThreads / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = part[0];
}

constexpr int kEmitThreads = 1024;

// one workgroup per map; thread t owns rows t * rpt .. (t + 1) * rpt - 1
__global__ __launch_bounds__(kEmitThreads) void mvs_emit(const uint64_t* __restrict__ masks, const float* __restrict__ inv,
                                                         const MvsMapDesc* __restrict__ maps,
                                                         const uint8_t* __restrict__ frames, int channels, int w, int h,
                                                         int ntx, int rpt, const int64_t* __restrict__ bases,
                                                         double* __restrict__ pts, uint8_t* __restrict__ cols)
{
    __shared__ int sc[2][kEmitThreads];
    const int t = threadIdx.x, m = blockIdx.x;
    const MvsMapDesc& mp = maps[m];
    const int r0 = min(h, t * rpt), r1 = min(h, (t + 1) * rpt);
    const uint64_t* mk = masks + (size_t)m * h * ntx;
    int cnt = 0;
    for (int y = r0; y < r1; y++)
        for (int j = 0; j < ntx; j++) cnt += __popcll(mk[(size_t)y * ntx + j]);
    sc[0][t] = cnt;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kEmitThreads; d <<= 1, cur ^= 1) {
        sc[cur ^ 1][t] = sc[cur][t] + (t >= d ? sc[cur][t - d] : 0);
        __syncthreads();
    }
    int64_t base = bases[m] + (sc[cur][t] - cnt);
    const size_t npx = (size_t)w * h;
    const uint8_t* img = frames + (size_t)mp.frame * npx * channels;
    for (int y = r0; y < r1; y++)
        for (int j = 0; j < ntx; j++) {
            uint64_t bits = mk[(size_t)y * ntx + j];
            while (bits) {
                const int x = j * 64 + __builtin_ctzll(bits);
                bits &= bits - 1;
                double X[3];
                mvs_backproject(mp.B, mp.c, x, y, inv[(size_t)m * npx + (size_t)y * w + x], X);
                pts[3 * base] = X[0];
                pts[3 * base + 1] = X[1];
                pts[3 * base + 2] = X[2];
                const uint8_t* px = img + ((size_t)y * w + x) * channels;
                cols[3 * base] = px[0];
                cols[3 * base + 1] = channels == 3 ? px[1] : px[0];
                cols[3 * base + 2] = channels == 3 ? px[2] : px[0];
                base++;
            }
        }
}

hipError_t launch_census(hipStream_t s, const uint8_t* frames, int channels, int w, int h, const int32_t* d_list,
                         int count, uint64_t* out)
{
    const dim3 grid((w + kCenTW - 1) / kCenTW, (h + kCenTH - 1) / kCenTH, count);
    hipLaunchKernelGGL(mvs_census, grid, dim3(kThreads), 0, s, frames, (size_t)w * h * channels, channels, w, h, d_list,
                       out);
    return hipGetLastError();
}

// the context's timing events, created on first use
hipError_t mvs_events(slam_ctx* c)
{
    for (auto& e : c->mvs_ev)
        if (!e) {
            const hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return rc;
        }
    return hipSuccess;
}

double mvs_elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (double)ms : 0.0;
}

bool frame_args_ok(int nframes, int w, int h, int channels)
{
    return nframes >= 1 && w >= 1 && h >= 1 && (channels == 1 || channels == 3) && (long long)h <= (1 << 20);
}

}  // namespace

void mvs_release(slam_ctx* c)
{
    for (auto& e : c->mvs_ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    for (auto& e : c->sgm_ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_mvs_last_timing(slam_ctx* c, double* ms)
{
    if (!c || !ms) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < 4; i++) ms[i] = c->mvs_ms[i];
    return SLAM_OK;
}

extern "C" int slam_mvs_census_dev(slam_ctx* c, void* stream, const uint8_t* d_frames, int nframes, int w, int h,
                                   int channels, uint64_t* d_out)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!frame_args_ok(nframes, w, h, channels) || !d_frames || !d_out || nframes > 65535)
        return set_err(c, SLAM_E_INVALID_ARG, "mvs census: bad frame arguments");
    if (w > kMvsMaxWidth) return set_err(c, SLAM_E_UNSUPPORTED, "mvs census: frames wider than 4096 pixels");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    SLAM_HIP(c, launch_census(s, d_frames, channels, w, h, nullptr, nframes, d_out));
    return stream_sync(c, s);
}

// slam_mvs_depth_batch_dev (out.C null: mvs_sweep into plane, cost, inv) and the volume of the same
// references (out.C set: mvs_volume into C, nvalid); check_only stops after the argument checks.
// ms[0] census, ms[1] the sweep or volume launches.
int slamhip::mvs_batch_run(slam_ctx* c, void* stream, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                           int nref, const int32_t* ref_idx, const int32_t* nsrc, const int32_t* src_idx, const double* M,
                           const double* v, const double* planes, int D, int radius, int uniq, int min_views,
                           const MvsBatchOut& out, bool check_only, double* ms)
{
    int16_t* d_plane = out.plane;
    int32_t* d_cost = out.cost;
    float* d_inv_depth = out.inv;
    const bool volume = out.C != nullptr;
    if (!frame_args_ok(nframes, w, h, channels) || !d_frames || nref < 0 || nref > 65535)
        return set_err(c, SLAM_E_INVALID_ARG, "mvs depth: bad frame arguments");
    if (nref == 0) return SLAM_OK;
    if (!ref_idx || !nsrc || !src_idx || !M || !v || !planes ||
        (volume ? !out.nvalid : (!d_plane || !d_cost || !d_inv_depth)))
        return set_err(c, SLAM_E_INVALID_ARG, "mvs depth: null argument");
    std::vector<MvsRefDesc> refs((size_t)nref);
    std::vector<int32_t> slot_of((size_t)nframes, -1), frames_used;
    auto slot = [&](int f) {
        if (slot_of[f] < 0) {
            slot_of[f] = (int32_t)frames_used.size();
            frames_used.push_back(f);
        }
        return slot_of[f];
    };
    for (int i = 0; i < nref; i++) {
        const int S = nsrc[i];
        const int rc = mvs_check_args(S, w, h, channels, M + (size_t)i * 36, v + (size_t)i * 12, planes + (size_t)i * D, D,
                                      radius, uniq, min_views);
        if (rc) return set_err(c, rc, rc == SLAM_E_UNSUPPORTED ? "mvs depth: frames wider than 4096 pixels"
                                                               : "mvs depth: S 1..4, D 4..256, radius 0..3, uniq 1..100, "
                                                                 "min_views 1..S and finite M, v, w");
        if (ref_idx[i] < 0 || ref_idx[i] >= nframes) return set_err(c, SLAM_E_INVALID_ARG, "mvs depth: reference index");
        MvsRefDesc& R = refs[i];
        memset(&R, 0, sizeof(R));
        R.S = S;
        for (int s = 0; s < S; s++) {
            const int f = src_idx[4 * i + s];
            if (f < 0 || f >= nframes) return set_err(c, SLAM_E_INVALID_ARG, "mvs depth: source index");
        }
        R.ref_slot = slot(ref_idx[i]);
        for (int s = 0; s < S; s++) {
            R.src_slot[s] = slot(src_idx[4 * i + s]);
            memcpy(R.M[s], M + (size_t)i * 36 + 9 * s, 9 * sizeof(double));
            memcpy(R.v[s], v + (size_t)i * 12 + 3 * s, 3 * sizeof(double));
        }
    }
    if (check_only) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    const size_t npx = (size_t)w * h;
    const int nslots = (int)frames_used.size();
    // parameter block: descriptors, planes, the frame list, the per-S reference lists
    const size_t o_refs = 0, o_planes = o_refs + sizeof(MvsRefDesc) * nref;
    const size_t o_frames = o_planes + sizeof(double) * (size_t)nref * D;
    const size_t o_list = o_frames + sizeof(int32_t) * nslots;
    const size_t total = o_list + sizeof(int32_t) * nref;
    std::vector<uint8_t> blk(total);
    memcpy(blk.data() + o_refs, refs.data(), sizeof(MvsRefDesc) * nref);
    memcpy(blk.data() + o_planes, planes, sizeof(double) * (size_t)nref * D);
    memcpy(blk.data() + o_frames, frames_used.data(), sizeof(int32_t) * nslots);
    int32_t* lists = reinterpret_cast<int32_t*>(blk.data() + o_list);
    int first[kMvsMaxSources + 2] = {0};
    {
        int n = 0;
        for (int S = 1; S <= kMvsMaxSources; S++) {
            first[S] = n;
            for (int i = 0; i < nref; i++)
                if (refs[i].S == S) lists[n++] = i;
        }
        first[kMvsMaxSources + 1] = n;
    }
    SLAM_HIP(c, c->mvs_par.ensure(total));
    SLAM_HIP(c, c->mvs_census.ensure(sizeof(uint64_t) * npx * nslots));
    uint8_t* dpar = c->mvs_par.as<uint8_t>();
    SLAM_HIP(c, hipMemcpyAsync(dpar, blk.data(), total, hipMemcpyHostToDevice, s));
    SLAM_HIP(c, mvs_events(c));
    SLAM_HIP(c, hipEventRecord(c->mvs_ev[0], s));
    SLAM_HIP(c, launch_census(s, d_frames, channels, w, h, reinterpret_cast<const int32_t*>(dpar + o_frames), nslots,
                              c->mvs_census.as<uint64_t>()));
    SLAM_HIP(c, hipEventRecord(c->mvs_ev[1], s));
    SweepParams p;
    p.census = c->mvs_census.as<uint64_t>();
    p.refs = reinterpret_cast<const MvsRefDesc*>(dpar + o_refs);
    p.planes = reinterpret_cast<const double*>(dpar + o_planes);
    p.w = w;
    p.h = h;
    p.D = D;
    p.radius = radius;
    p.uniq = uniq;
    p.min_views = min_views;
    p.plane = d_plane;
    p.cost = d_cost;
    p.inv = d_inv_depth;
    p.vol_C = out.C;
    p.vol_nv = out.nvalid;
    // the staged stores need whole, aligned groups of eight planes
    const bool vec = D % 8 == 0 && reinterpret_cast<uintptr_t>(out.C) % 16 == 0 && reinterpret_cast<uintptr_t>(out.nvalid) % 8 == 0;
    const int gx = (w + kSwTW - 1) / kSwTW, gy = (h + kSwTH - 1) / kSwTH;
    for (int S = 1; S <= kMvsMaxSources; S++) {
        const int n = first[S + 1] - first[S];
        if (n == 0) continue;
        p.list = reinterpret_cast<const int32_t*>(dpar + o_list) + first[S];
        const dim3 grid(gx, gy, n);
        if (volume) {
            switch (S * 2 + (vec ? 1 : 0)) {
            case 2: hipLaunchKernelGGL((mvs_volume<1, false>), grid, dim3(kThreads), 0, s, p); break;
            case 3: hipLaunchKernelGGL((mvs_volume<1, true>), grid, dim3(kThreads), 0, s, p); break;
            case 4: hipLaunchKernelGGL((mvs_volume<2, false>), grid, dim3(kThreads), 0, s, p); break;
            case 5: hipLaunchKernelGGL((mvs_volume<2, true>), grid, dim3(kThreads), 0, s, p); break;
            case 6: hipLaunchKernelGGL((mvs_volume<3, false>), grid, dim3(kThreads), 0, s, p); break;
            case 7: hipLaunchKernelGGL((mvs_volume<3, true>), grid, dim3(kThreads), 0, s, p); break;
            case 8: hipLaunchKernelGGL((mvs_volume<4, false>), grid, dim3(kThreads), 0, s, p); break;
            default: hipLaunchKernelGGL((mvs_volume<4, true>), grid, dim3(kThreads), 0, s, p); break;
            }
        } else {
            switch (S) {
            case 1: hipLaunchKernelGGL(mvs_sweep<1>, grid, dim3(kThreads), 0, s, p); break;
            case 2: hipLaunchKernelGGL(mvs_sweep<2>, grid, dim3(kThreads), 0, s, p); break;
            case 3: hipLaunchKernelGGL(mvs_sweep<3>, grid, dim3(kThreads), 0, s, p); break;
            default: hipLaunchKernelGGL(mvs_sweep<4>, grid, dim3(kThreads), 0, s, p); break;
            }
        }
        SLAM_HIP(c, hipGetLastError());
    }
    SLAM_HIP(c, hipEventRecord(c->mvs_ev[2], s));
    if (int rc = stream_sync(c, s)) return rc;      // the parameter block is reused by the next call
    ms[0] = mvs_elapsed(c->mvs_ev[0], c->mvs_ev[1]);
    ms[1] = mvs_elapsed(c->mvs_ev[1], c->mvs_ev[2]);
    return SLAM_OK;
}

extern "C" int slam_mvs_depth_batch_dev(slam_ctx* c, void* stream, const uint8_t* d_frames, int nframes, int w, int h,
                                        int channels, int nref, const int32_t* ref_idx, const int32_t* nsrc,
                                        const int32_t* src_idx, const double* M, const double* v, const double* planes,
                                        int D, int radius, int uniq, int min_views, int16_t* d_plane, int32_t* d_cost,
                                        float* d_inv_depth)
{
    if (!c) return SLAM_E_INVALID_ARG;
    MvsBatchOut out;
    out.plane = d_plane;
    out.cost = d_cost;
    out.inv = d_inv_depth;
    return mvs_batch_run(c, stream, d_frames, nframes, w, h, channels, nref, ref_idx, nsrc, src_idx, M, v, planes, D, radius,
                         uniq, min_views, out, false, c->mvs_ms);
}

extern "C" int slam_mvs_fuse_dev(slam_ctx* c, void* stream, const uint8_t* d_frames, int nframes, int w, int h,
                                 int channels, int nmaps, const int32_t* frame_idx, const float* d_inv_depth,
                                 const int32_t* nnbr, const int32_t* nbr_idx, const double* M, const double* v,
                                 const double* B, const double* cvec, double eps, int min_consistent, int step,
                                 int radius, double* points, uint8_t* colors, int cap, int* n_out)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!n_out || cap < 0 || (cap > 0 && (!points || !colors))) return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: null output");
    *n_out = 0;
    if (!frame_args_ok(nframes, w, h, channels) || !d_frames || nmaps < 0 || nmaps > 65535)
        return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: bad frame arguments");
    if (w > kMvsMaxWidth) return set_err(c, SLAM_E_UNSUPPORTED, "mvs fuse: frames wider than 4096 pixels");
    if (nmaps == 0) return SLAM_OK;
    if (!frame_idx || !d_inv_depth || !nnbr || !nbr_idx || !M || !v || !B || !cvec || !(eps >= 0) || !mvs_finite(eps) ||
        min_consistent < 0 || min_consistent > kMvsMaxSources || step < 1 || radius < 0 || radius > kMvsMaxRadius)
        return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: eps >= 0, min_consistent 0..4, step >= 1, radius 0..3");
    std::vector<MvsMapDesc> maps((size_t)nmaps);
    for (int i = 0; i < nmaps; i++) {
        MvsMapDesc& m = maps[i];
        memset(&m, 0, sizeof(m));
        if (frame_idx[i] < 0 || frame_idx[i] >= nframes || nnbr[i] < 0 || nnbr[i] > kMvsMaxSources)
            return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: frame index or neighbour count");
        m.frame = frame_idx[i];
        m.nnbr = nnbr[i];
        for (int n = 0; n < m.nnbr; n++) {
            const int j = nbr_idx[4 * i + n];
            if (j < 0 || j >= nmaps) return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: neighbour index");
            m.nbr[n] = j;
            memcpy(m.M[n], M + (size_t)i * 36 + 9 * n, 9 * sizeof(double));
            memcpy(m.v[n], v + (size_t)i * 12 + 3 * n, 3 * sizeof(double));
            for (int k = 0; k < 9; k++)
                if (!mvs_finite(m.M[n][k])) return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: non-finite M");
            for (int k = 0; k < 3; k++)
                if (!mvs_finite(m.v[n][k])) return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: non-finite v");
        }
        memcpy(m.B, B + (size_t)i * 9, 9 * sizeof(double));
        memcpy(m.c, cvec + (size_t)i * 3, 3 * sizeof(double));
        for (int k = 0; k < 9; k++)
            if (!mvs_finite(m.B[k])) return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: non-finite B");
        for (int k = 0; k < 3; k++)
            if (!mvs_finite(m.c[k])) return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: non-finite c");
    }
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    const int ntx = (w + 63) / 64;
    const size_t words = (size_t)h * ntx;
    const size_t o_maps = 0, o_cnt = sizeof(MvsMapDesc) * nmaps, o_base = o_cnt + ((sizeof(int32_t) * nmaps + 7) & ~(size_t)7);
    const size_t total = o_base + sizeof(int64_t) * nmaps;
    SLAM_HIP(c, c->mvs_par.ensure(total));
    SLAM_HIP(c, c->mvs_mask.ensure(sizeof(uint64_t) * words * nmaps));
    uint8_t* dpar = c->mvs_par.as<uint8_t>();
    const MvsMapDesc* dmaps = reinterpret_cast<const MvsMapDesc*>(dpar + o_maps);
    int32_t* dcnt = reinterpret_cast<int32_t*>(dpar + o_cnt);
    int64_t* dbase = reinterpret_cast<int64_t*>(dpar + o_base);
    SLAM_HIP(c, hipMemcpyAsync(dpar, maps.data(), sizeof(MvsMapDesc) * nmaps, hipMemcpyHostToDevice, s));
    SLAM_HIP(c, mvs_events(c));
    SLAM_HIP(c, hipEventRecord(c->mvs_ev[3], s));
    hipLaunchKernelGGL(mvs_filter, dim3(ntx, (h + 3) / 4, nmaps), dim3(kThreads), 0, s, d_inv_depth, dmaps, w, h, ntx, eps,
                       min_consistent, step, radius + kMvsFilterBorder, c->mvs_mask.as<uint64_t>());
    SLAM_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(mvs_count, dim3(nmaps), dim3(kThreads), 0, s, c->mvs_mask.as<uint64_t>(), (int)words, dcnt);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(c->mvs_ev[4], s));
    std::vector<int32_t> cnt((size_t)nmaps);
    SLAM_HIP(c, hipMemcpyAsync(cnt.data(), dcnt, sizeof(int32_t) * nmaps, hipMemcpyDeviceToHost, s));
    if (int rc = stream_sync(c, s)) return rc;
    c->mvs_ms[2] = mvs_elapsed(c->mvs_ev[3], c->mvs_ev[4]);
    c->mvs_ms[3] = 0.0;
    std::vector<int64_t> base((size_t)nmaps);
    int64_t n = 0;
    for (int i = 0; i < nmaps; i++) {
        base[i] = n;
        n += cnt[i];
    }
    if (n > 0x7fffffff) return set_err(c, SLAM_E_UNSUPPORTED, "mvs fuse: more than 2^31 - 1 points");
    *n_out = (int)n;
    if (n > cap) return set_err(c, SLAM_E_CAPACITY, "mvs fuse: output buffers too small (n_out holds the needed count)");
    if (n == 0) return SLAM_OK;
    SLAM_HIP(c, c->mvs_out.ensure((size_t)n * 27));
    double* dpts = c->mvs_out.as<double>();
    uint8_t* dcol = c->mvs_out.as<uint8_t>() + (size_t)n * 24;
    SLAM_HIP(c, hipMemcpyAsync(dbase, base.data(), sizeof(int64_t) * nmaps, hipMemcpyHostToDevice, s));
    SLAM_HIP(c, hipEventRecord(c->mvs_ev[5], s));
    hipLaunchKernelGGL(mvs_emit, dim3(nmaps), dim3(kEmitThreads), 0, s, c->mvs_mask.as<uint64_t>(), d_inv_depth, dmaps,
                       d_frames, channels, w, h, ntx, (h + kEmitThreads - 1) / kEmitThreads, dbase, dpts, dcol);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(c->mvs_ev[6], s));
    SLAM_HIP(c, hipMemcpyAsync(points, dpts, (size_t)n * 24, hipMemcpyDeviceToHost, s));
    SLAM_HIP(c, hipMemcpyAsync(colors, dcol, (size_t)n * 3, hipMemcpyDeviceToHost, s));
    if (int rc = stream_sync(c, s)) return rc;
    c->mvs_ms[3] = mvs_elapsed(c->mvs_ev[5], c->mvs_ev[6]);
    return SLAM_OK;
}

extern "C" int slam_mvs_depth(slam_ctx* c, const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h,
                              size_t step, int channels, const double* M, const double* v, const double* planes, int D,
                              int radius, int uniq, int min_views, int16_t* plane, int32_t* cost, float* inv_depth)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!ref || !srcs || !plane || !cost || !inv_depth) return set_err(c, SLAM_E_INVALID_ARG, "mvs depth: null argument");
    if (int rc = mvs_check_args(S, w, h, channels, M, v, planes, D, radius, uniq, min_views))
        return set_err(c, rc, "mvs depth: bad arguments");
    if (step < (size_t)w * channels) return set_err(c, SLAM_E_INVALID_ARG, "mvs depth: short row stride");
    for (int s = 0; s < S; s++)
        if (!srcs[s]) return set_err(c, SLAM_E_INVALID_ARG, "mvs depth: null source");
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
    if (int rc = slam_mvs_depth_batch_dev(c, c->stream, d, S + 1, w, h, channels, 1, &ref_idx, &nsrc, src_idx, M4, v4,
                                          planes, D, radius, uniq, min_views, m.ptr(s_plane), m.ptr(s_cost), m.ptr(s_inv)))
        return rc;
    SLAM_HIP(c, m.download(cost, s_cost, c->stream));
    SLAM_HIP(c, m.download(inv_depth, s_inv, c->stream));
    SLAM_HIP(c, m.download(plane, s_plane, c->stream));
    return stream_sync(c, c->stream);
}

extern "C" int slam_mvs_fuse(slam_ctx* c, const uint8_t* const* frames, int w, int h, size_t step, int channels,
                             int nmaps, const float* inv_depth, const int32_t* nnbr, const int32_t* nbr_idx,
                             const double* M, const double* v, const double* B, const double* cvec, double eps,
                             int min_consistent, int step_px, int radius, double* points, uint8_t* colors, int cap,
                             int* n_out)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!n_out) return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: null output");
    *n_out = 0;
    if (nmaps < 0 || nmaps > 65535 || !frame_args_ok(1, w, h, channels) || step < (size_t)w * channels)
        return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: bad frame arguments");
    if (nmaps == 0) return SLAM_OK;
    if (!frames || !inv_depth) return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: null argument");
    for (int i = 0; i < nmaps; i++)
        if (!frames[i]) return set_err(c, SLAM_E_INVALID_ARG, "mvs fuse: null frame");
    SLAM_HIP(c, hipSetDevice(c->device));
    const size_t row = (size_t)w * channels, fb = row * h, npx = (size_t)w * h;
    DevLayout lay;
    const auto s_frames = lay.add<uint8_t>((size_t)nmaps * fb);
    const auto s_inv = lay.add<float>(npx * nmaps);
    DevMem m;
    SLAM_HIP(c, m.bind(c->mvs_in, lay));
    uint8_t* d = m.ptr(s_frames);
    std::vector<int32_t> idx((size_t)nmaps);
    for (int i = 0; i < nmaps; i++) {
        idx[i] = i;
        SLAM_HIP(c, hipMemcpy2DAsync(d + i * fb, row, frames[i], step, row, h, hipMemcpyHostToDevice, c->stream));
    }
    SLAM_HIP(c, m.upload(s_inv, inv_depth, c->stream));
    return slam_mvs_fuse_dev(c, c->stream, d, nmaps, w, h, channels, nmaps, idx.data(), m.ptr(s_inv),
                             nnbr, nbr_idx, M, v, B, cvec, eps, min_consistent, step_px, radius, points, colors, cap, n_out);
}

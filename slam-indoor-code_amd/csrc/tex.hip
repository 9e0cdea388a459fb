// Per-face texture atlas on the device (tests/tex_ref.py is the
// definition of every value computed here, tex_math.h the shared arithmetic):
//
//   tex_count   one thread per pixel of a chunk of id images (x: pixels, y: view).  A lane is
//               the head of a run when its face differs from the lane before it; the heads'
//               ballot gives each head its run length, and only heads add: one integer
//               atomicAdd of the run length into counts[view][face].  Integer adds commute, so
//               the counts do not depend on the order of the waves.
//   tex_best    one thread per face: folds the chunk's counts, views ascending, into the
//               caller's (best_count, best_view) by tex_best_step.
//   tex_check   one thread per face: a vertex index outside the cloud or a best view outside
//               the call's views raises a bit of a flag word that the host reads before
//               anything is filled.
//   tex_fill    one thread per atlas texel, 256 consecutive texels of the atlas raster per
//               workgroup.  The texels' bytes go through 768 bytes of LDS and leave as dwords:
//               consecutive lanes store consecutive dwords.  A view's 12 entries of P and its
//               frame index sit in a parameter block; frames are gathered read-only.
#include "slamhip_internal.h"
#include "tex_math.h"

#include <algorithm>
#include <vector>

namespace slamhip {
namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr size_t kCountBudget = (size_t)1 << 24;        // int32 counts of one chunk of views (64 MiB)
constexpr int kMaxChunkViews = 64;

__global__ __launch_bounds__(kThreads) void tex_count(const int32_t* __restrict__ ids, int npx, int nf,
                                                      int32_t* __restrict__ counts)
{
    const int p = blockIdx.x * kThreads + threadIdx.x;       // whole waves stay: the ballot needs every lane
    const int m = blockIdx.y;
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t f = p < npx ? tex_id_face(ids[(size_t)m * npx + p], nf) : -1;
    const int32_t prev = __shfl_up(f, 1, kWave);
    const bool head = lane == 0 || prev != f;
    const unsigned long long heads = __ballot(head);
    if (!head || f < 0) return;
    const unsigned long long above = lane == kWave - 1 ? 0ull : heads >> (lane + 1);
    const int len = above ? __ffsll(above) : kWave - lane;   // to the next head, or to the wave's end
    atomicAdd(&counts[(size_t)m * nf + f], len);
}

__global__ __launch_bounds__(kThreads) void tex_best(const int32_t* __restrict__ counts, int nviews, int nf, int view0,
                                                     int32_t* __restrict__ best_count, int32_t* __restrict__ best_view)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= nf) return;
    int32_t bc = best_count[f], bv = best_view[f];
    for (int m = 0; m < nviews; m++) tex_best_step(bc, bv, counts[(size_t)m * nf + f], view0 + m);
    best_count[f] = bc;
    best_view[f] = bv;
}

__global__ __launch_bounds__(kThreads) void tex_check(const int32_t* __restrict__ F, const int32_t* __restrict__ best_view,
                                                      int nv, int nf, int nviews, int32_t* __restrict__ flag)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= nf) return;
    int bad = 0;
    for (int k = 0; k < 3; k++) {
        const int32_t v = F[3 * (size_t)f + k];
        if (v < 0 || v >= nv) bad |= 1;
    }
    const int32_t bv = best_view[f];
    if (bv < -1 || bv >= nviews) bad |= 2;
    if (bad) atomicOr(flag, bad);
}

__global__ __launch_bounds__(kThreads) void tex_fill(TexLayout l, int nf, unsigned long long ntexels,
                                                     const double* __restrict__ V, const uint8_t* __restrict__ C,
                                                     const int32_t* __restrict__ F, const uint8_t* __restrict__ frames,
                                                     int w, int h, int channels, const TexView* __restrict__ views,
                                                     const int32_t* __restrict__ best_count,
                                                     const int32_t* __restrict__ best_view, int min_pixels,
                                                     uint8_t* __restrict__ atlas)
{
    __shared__ __attribute__((aligned(4))) uint8_t stage[kThreads * 3];
    const unsigned long long t0 = (unsigned long long)blockIdx.x * kThreads;     // the block's first texel
    const unsigned long long y0 = t0 / (unsigned)l.page_w;
    const unsigned xx = (unsigned)(t0 - y0 * (unsigned)l.page_w) + threadIdx.x;  // < page_w + 256
    const unsigned dy = xx / (unsigned)l.page_w;
    const bool live = t0 + threadIdx.x < ntexels;
    if (live)
        tex_texel(l, nf, (int)(xx - dy * (unsigned)l.page_w), (long long)(y0 + dy), V, C, F, frames, w, h, channels, views,
                  best_count, best_view, min_pixels, stage + 3 * threadIdx.x);
    __syncthreads();
    const unsigned long long left = ntexels - t0;                                // > 0: the grid covers no empty block
    const unsigned nbytes = left < kThreads ? (unsigned)left * 3u : kThreads * 3u;
    uint8_t* dst = atlas + t0 * 3;                                               // t0 * 3 is a multiple of 4
    if (((uintptr_t)atlas & 3u) == 0) {
        const unsigned nwords = nbytes >> 2;
        if (threadIdx.x < nwords) reinterpret_cast<uint32_t*>(dst)[threadIdx.x] = reinterpret_cast<const uint32_t*>(stage)[threadIdx.x];
        const unsigned tail = nwords << 2;
        if (threadIdx.x < nbytes - tail) dst[tail + threadIdx.x] = stage[tail + threadIdx.x];
    } else {
        for (unsigned b = threadIdx.x; b < nbytes; b += kThreads) dst[b] = stage[b];
    }
}

hipError_t tex_events(slam_ctx* c)
{
    for (auto& e : c->tex_ev)
        if (!e) {
            const hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return rc;
        }
    return hipSuccess;
}

double tex_elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (double)ms : 0.0;
}

const char* const kSelectMsg = "tex select: nv >= 0, h, w >= 1 with h w <= 2^30, view0 >= 0, 0 <= nf <= 2^30 (beyond: "
                               "unsupported), no null pointer with a non-zero count";
const char* const kFillMsg = "tex fill: T 1..64, T + 4 <= page <= 8192, min_pixels 1..2^30, frames of 1 or 3 channels, 0 <= "
                             "nviews <= 2^20, frame indices inside the batch, nf <= 2^30 (beyond: unsupported), no null "
                             "pointer with a non-zero count";

}  // namespace

void tex_release(slam_ctx* c)
{
    for (auto& e : c->tex_ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_tex_last_timing(slam_ctx* c, double* ms)
{
    if (!c || !ms) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < 2; i++) ms[i] = c->tex_ms[i];
    return SLAM_OK;
}

extern "C" int slam_tex_select_dev(slam_ctx* c, void* stream, const int32_t* d_ids, int nv, int h, int w, int view0, int nf,
                                   int32_t* d_best_count, int32_t* d_best_view)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (int rc = tex_check_select(d_ids, nv, h, w, view0, nf, d_best_count, d_best_view)) return set_err(c, rc, kSelectMsg);
    c->tex_ms[0] = 0.0;
    if (nv == 0 || nf == 0) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    const int npx = h * w;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)kMaxChunkViews, (size_t)nv, kCountBudget / (size_t)nf}));
    DevLayout lay;
    const auto s_cnt = lay.add<int32_t>((size_t)chunk * nf);
    DevMem mem;
    SLAM_HIP(c, mem.bind(c->tex_ws, lay));
    SLAM_HIP(c, tex_events(c));
    SLAM_HIP(c, hipEventRecord(c->tex_ev[0], s));
    const unsigned fblocks = (unsigned)((nf + kThreads - 1) / kThreads);
    for (int m0 = 0; m0 < nv; m0 += chunk) {
        const int n = std::min(chunk, nv - m0);
        SLAM_HIP(c, hipMemsetAsync(mem.ptr(s_cnt), 0, (size_t)n * nf * sizeof(int32_t), s));
        hipLaunchKernelGGL(tex_count, dim3((unsigned)((npx + kThreads - 1) / kThreads), (unsigned)n), dim3(kThreads), 0, s,
                           d_ids + (size_t)m0 * npx, npx, nf, mem.ptr(s_cnt));
        SLAM_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(tex_best, dim3(fblocks), dim3(kThreads), 0, s, mem.ptr(s_cnt), n, nf, view0 + m0, d_best_count,
                           d_best_view);
        SLAM_HIP(c, hipGetLastError());
    }
    SLAM_HIP(c, hipEventRecord(c->tex_ev[1], s));
    if (int rc = stream_sync(c, s)) return rc;
    c->tex_ms[0] = tex_elapsed(c->tex_ev[0], c->tex_ev[1]);
    return SLAM_OK;
}

extern "C" int slam_tex_fill_dev(slam_ctx* c, void* stream, const double* d_V, const uint8_t* d_C, const int32_t* d_F, int nv,
                                 int nf, const uint8_t* d_frames, int n, int h, int w, int channels, const int32_t* frame_idx,
                                 const double* P, int nviews, const int32_t* d_best_count, const int32_t* d_best_view,
                                 int min_pixels, int T, int page, uint8_t* d_atlas)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (int rc = tex_check_fill(d_V, d_C, d_F, nv, nf, d_frames, n, h, w, channels, frame_idx, P, nviews, d_best_count,
                                d_best_view, min_pixels, T, page, d_atlas))
        return set_err(c, rc, kFillMsg);
    c->tex_ms[1] = 0.0;
    if (nf == 0) return SLAM_OK;
    const TexLayout l = tex_layout(nf, T, page);
    const unsigned long long ntexels = (unsigned long long)l.cell_rows * l.S * l.page_w;
    const unsigned long long blocks = (ntexels + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffull) return set_err(c, SLAM_E_UNSUPPORTED, "tex fill: more than 2^39 atlas texels");
    std::vector<TexView> views((size_t)std::max(nviews, 1));
    tex_make_views(P, frame_idx, nviews, views.data());
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    DevLayout lay;
    const auto s_views = lay.add<TexView>(views.size());
    const auto s_flag = lay.add<int32_t>(1);
    DevMem mem;
    SLAM_HIP(c, mem.bind(c->tex_par, lay));
    SLAM_HIP(c, mem.upload(s_views, views.data(), s));
    SLAM_HIP(c, hipMemsetAsync(mem.ptr(s_flag), 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(tex_check, dim3((unsigned)((nf + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, d_F, d_best_view, nv, nf,
                       nviews, mem.ptr(s_flag));
    SLAM_HIP(c, hipGetLastError());
    int32_t* flag = static_cast<int32_t*>(readback(c, sizeof(int32_t)));
    if (!flag) return set_err(c, SLAM_E_HIP, "tex fill: no pinned readback space");
    SLAM_HIP(c, hipMemcpyAsync(flag, mem.ptr(s_flag), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (int rc = stream_sync(c, s)) return rc;
    if (*flag & 1) return set_err(c, SLAM_E_INVALID_ARG, "tex fill: a face index outside the vertices");
    if (*flag & 2) return set_err(c, SLAM_E_INVALID_ARG, "tex fill: a best view outside -1 .. nviews - 1");
    SLAM_HIP(c, tex_events(c));
    SLAM_HIP(c, hipEventRecord(c->tex_ev[2], s));
    hipLaunchKernelGGL(tex_fill, dim3((unsigned)blocks), dim3(kThreads), 0, s, l, nf, ntexels, d_V, d_C, d_F, d_frames, w, h,
                       channels, mem.ptr(s_views), d_best_count, d_best_view, min_pixels, d_atlas);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(c->tex_ev[3], s));
    if (int rc = stream_sync(c, s)) return rc;          // the parameter block is host memory of this call
    c->tex_ms[1] = tex_elapsed(c->tex_ev[2], c->tex_ev[3]);
    return SLAM_OK;
}

extern "C" int slam_tex_select(slam_ctx* c, const int32_t* ids, int nv, int h, int w, int view0, int nf, int32_t* best_count,
                               int32_t* best_view)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (int rc = tex_check_select(ids, nv, h, w, view0, nf, best_count, best_view)) return set_err(c, rc, kSelectMsg);
    if (nv == 0 || nf == 0) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    DevLayout lay;
    const auto s_ids = lay.add<int32_t>((size_t)nv * h * w);
    const auto s_bc = lay.add<int32_t>((size_t)nf);
    const auto s_bv = lay.add<int32_t>((size_t)nf);
    DevMem mem;
    SLAM_HIP(c, mem.bind(c->tex_in, lay));
    SLAM_HIP(c, mem.upload(s_ids, ids, c->stream));
    SLAM_HIP(c, mem.upload(s_bc, best_count, c->stream));
    SLAM_HIP(c, mem.upload(s_bv, best_view, c->stream));
    if (int rc = slam_tex_select_dev(c, c->stream, mem.ptr(s_ids), nv, h, w, view0, nf, mem.ptr(s_bc), mem.ptr(s_bv))) return rc;
    SLAM_HIP(c, mem.download(best_count, s_bc, c->stream));
    SLAM_HIP(c, mem.download(best_view, s_bv, c->stream));
    return stream_sync(c, c->stream);
}

extern "C" int slam_tex_fill(slam_ctx* c, const double* V, const uint8_t* C, const int32_t* F, int nv, int nf,
                             const uint8_t* frames, int n, int h, int w, int channels, const int32_t* frame_idx, const double* P,
                             int nviews, const int32_t* best_count, const int32_t* best_view, int min_pixels, int T, int page,
                             uint8_t* atlas)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (int rc = tex_check_fill(V, C, F, nv, nf, frames, n, h, w, channels, frame_idx, P, nviews, best_count, best_view,
                                min_pixels, T, page, atlas))
        return set_err(c, rc, kFillMsg);
    if (nf == 0) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    const TexLayout l = tex_layout(nf, T, page);
    DevLayout lay;
    const auto s_V = lay.add<double>(3 * (size_t)nv);
    const auto s_C = lay.add<uint8_t>(3 * (size_t)nv);
    const auto s_F = lay.add<int32_t>(3 * (size_t)nf);
    const auto s_fr = lay.add<uint8_t>((size_t)n * h * w * channels);
    const auto s_bc = lay.add<int32_t>((size_t)nf);
    const auto s_bv = lay.add<int32_t>((size_t)nf);
    const auto s_at = lay.add<uint8_t>((size_t)l.cell_rows * l.S * l.page_w * 3);
    DevMem mem;
    SLAM_HIP(c, mem.bind(c->tex_in, lay));
    SLAM_HIP(c, mem.upload(s_V, V, c->stream));
    SLAM_HIP(c, mem.upload(s_C, C, c->stream));
    SLAM_HIP(c, mem.upload(s_F, F, c->stream));
    if (s_fr.count && frames) SLAM_HIP(c, mem.upload(s_fr, frames, c->stream));
    SLAM_HIP(c, mem.upload(s_bc, best_count, c->stream));
    SLAM_HIP(c, mem.upload(s_bv, best_view, c->stream));
    if (int rc = slam_tex_fill_dev(c, c->stream, mem.ptr(s_V), mem.ptr(s_C), mem.ptr(s_F), nv, nf, mem.ptr(s_fr), n, h, w, channels,
                                   frame_idx, P, nviews, mem.ptr(s_bc), mem.ptr(s_bv), min_pixels, T, page, mem.ptr(s_at)))
        return rc;
    SLAM_HIP(c, mem.download(atlas, s_at, c->stream));
    return stream_sync(c, c->stream);
}

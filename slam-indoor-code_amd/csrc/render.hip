// Headless rendering of the onlyViz scene (the cv::viz window of
// vizualizePointsAndCameras, src/vizualization/vizualizationModule.cpp:61-134):
// a deterministic z-buffer rasteriser for the coloured cloud (WCloud), the
// trajectory (WTrajectory) and the vertex-coloured meshes (WMesh).
// tests/render_ref.py is the definition; render_setup.h holds everything
// between a world-space primitive and the integers the loops below walk.
//
// Per chunk of views that fits the key buffer, four passes on one stream:
//   clear          every pixel's 64-bit key to all ones (hipMemsetAsync)
//   points, lines  render_points: a thread per (view, point) puts its square;
//                  render_lines: a wave per (view, segment), lanes stride the walk
//   triangles      render_tris: a thread per (view, face) does the set-up (sort
//                  the indices, transform, clip, fan, snap).  A piece whose
//                  bounding box holds at most kSmallArea pixels is walked by
//                  that thread with incremental int64 edge functions; a larger
//                  one is cut into tiles of 32 x 32 pixels (doubled until a piece
//                  has at most kMaxTiles) that go to the chunk's list through one
//                  atomic counter, and render_large gives every tile a wave.
//                  The list is one pool of kLargePool tiles shared by the views of
//                  a chunk; tiles that do not fit it are walked by the appending
//                  thread (slow, never wrong).  List order has no effect: every fragment is one
//                  64-bit atomicMin on the pixel's key
//                  (~bits(f32 1/Z) << 32 | kind << 30 | index).
//   resolve        render_resolve: a thread per pixel turns the winning key into
//                  colour, id and depth; a triangle's colour is recomputed from
//                  the face by the same set-up, so no colour is stored per fragment.
// Nothing depends on launch order: keys are totally ordered and atomicMin commutes.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "render_setup.h"
#include "slamhip_internal.h"

namespace slamhip {

namespace rs = render_setup;

namespace {

constexpr int kSmallArea = 128;          // pixels of a bounding box one thread walks
constexpr int kTile = 32, kMaxTiles = 1024;
constexpr int kLargePool = 1 << 19;      // list entries per chunk of views (48 MiB), shared by its views
constexpr int kTinyPool = 64;            // the list of raster_mode 3: the tests' way into the overflow branch
constexpr int kLargeBlocks = 8192;       // waves that drain the list
constexpr size_t kKeyBudget = (size_t)256 << 20;
constexpr int kMaxChunk = 1024;

struct LargeItem {
    rs::ScreenTri t;                     // bx0 .. by1: the tile
    uint32_t id;
    uint32_t view;                       // within the chunk
};

// skipped, clipped away, rasterised, fragments tested
constexpr int kStats = 4;

struct RenderHdr {
    unsigned long long stats[kStats];
};

__device__ __forceinline__ void put_key(uint64_t* keys, size_t pix, float depth, uint32_t id)
{
    const uint64_t key = ((uint64_t)(~rs::float_bits(depth)) << 32) | id;
    unsigned long long* p = reinterpret_cast<unsigned long long*>(keys + pix);
    // keys only fall: a stale read is never below the current value, so skipping on it is safe
    if (*reinterpret_cast<volatile unsigned long long*>(p) > key) atomicMin(p, (unsigned long long)key);
}

__device__ void block_stats(unsigned long long* s_stat, const unsigned long long* mine, unsigned long long* g_stats)
{
    for (int i = 0; i < kStats; i++)
        if (mine[i]) atomicAdd(&s_stat[i], mine[i]);
    __syncthreads();
    if (threadIdx.x < kStats && s_stat[threadIdx.x]) atomicAdd(&g_stats[threadIdx.x], s_stat[threadIdx.x]);
}

// the pixels x0 .. x1, y0 .. y1 (inside the viewport) of one prepared triangle
__device__ void raster_box(const rs::ScreenTri& t, int x0, int y0, int x1, int y1, uint32_t id, uint64_t* keys, int w)
{
    int64_t A[3], B[3], bias[3], row[3];
    for (int i = 0; i < 3; i++) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        A[i] = -(int64_t)(t.y[b] - t.y[a]) * 16;
        B[i] = (int64_t)(t.x[b] - t.x[a]) * 16;
        bias[i] = rs::edge_bias(t.x[a], t.y[a], t.x[b], t.y[b]);
        row[i] = rs::edge_fn(t.x[a], t.y[a], t.x[b], t.y[b], x0 * 16 + 8, y0 * 16 + 8) + bias[i];
    }
    for (int y = y0; y <= y1; y++) {
        int64_t e0 = row[0], e1 = row[1], e2 = row[2];
        for (int x = x0; x <= x1; x++) {
            if ((e0 | e1 | e2) >= 0) {
                const int64_t wt[3] = {e0 - bias[0], e1 - bias[1], e2 - bias[2]};
                put_key(keys, (size_t)y * w + x, rs::tri_depth(t, wt), id);
            }
            e0 += A[0]; e1 += A[1]; e2 += A[2];
        }
        row[0] += B[0]; row[1] += B[1]; row[2] += B[2];
    }
}

__global__ __launch_bounds__(256) void render_points(const float* __restrict__ pts, int n, const double* __restrict__ views,
                                                     rs::Camera cam, int radius, uint64_t* keys, unsigned long long* g_stats)
{
    __shared__ unsigned long long s_stat[kStats];
    if (threadIdx.x < kStats) s_stat[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long mine[kStats] = {0, 0, 0, 0};
    const int i = blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (i < n) {
        const float p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
        int32_t px, py;
        float depth;
        if (!rs::finite3(p)) mine[0] = 1;
        else if (!rs::setup_point(cam, views + 12 * v, p, &px, &py, &depth)) mine[1] = 1;
        else {
            const int x0 = max(px - radius, 0), x1 = min(px + radius, cam.w - 1);
            const int y0 = max(py - radius, 0), y1 = min(py + radius, cam.h - 1);
            uint64_t* kv = keys + (size_t)v * cam.w * cam.h;
            for (int y = y0; y <= y1; y++)
                for (int x = x0; x <= x1; x++) put_key(kv, (size_t)y * cam.w + x, depth, ((uint32_t)rs::kPoint << 30) | (uint32_t)i);
            mine[2] = 1;
            mine[3] = (unsigned long long)(x1 - x0 + 1) * (y1 - y0 + 1);
        }
    }
    block_stats(s_stat, mine, g_stats);
}

__global__ __launch_bounds__(64) void render_lines(const float* __restrict__ lines, const double* __restrict__ views, rs::Camera cam,
                                                   uint64_t* keys, unsigned long long* g_stats)
{
    const int l = blockIdx.x, v = blockIdx.y, lane = threadIdx.x;
    float a[3], b[3];
    for (int k = 0; k < 3; k++) {
        a[k] = lines[6 * (size_t)l + k];
        b[k] = lines[6 * (size_t)l + 3 + k];
    }
    int stat = 2;
    rs::ScreenLine sl;
    if (!rs::finite3(a) || !rs::finite3(b)) stat = 0;
    else {
        const int rc = rs::setup_line(cam, views + 12 * v, a, b, &sl);
        if (rc < 0) stat = 0;
        else if (rc == 0 || sl.k0 > sl.k1) stat = 1;
    }
    if (stat == 2) {
        uint64_t* kv = keys + (size_t)v * cam.w * cam.h;
        for (int32_t k = sl.k0 + lane; k <= sl.k1; k += 64) {
            int32_t x, y;
            float depth;
            rs::line_pixel(sl, k, &x, &y, &depth);
            if (x >= 0 && x < cam.w && y >= 0 && y < cam.h)
                put_key(kv, (size_t)y * cam.w + x, depth, ((uint32_t)rs::kLine << 30) | (uint32_t)l);
        }
    }
    if (lane == 0) {
        atomicAdd(&g_stats[stat], 1ull);
        if (stat == 2) atomicAdd(&g_stats[3], (unsigned long long)(sl.k1 - sl.k0 + 1));
    }
}

// the face's vertex indices in ascending order (the result does not depend on how a face lists them);
// false: an index is out of range or a coordinate is not finite
__device__ __forceinline__ bool face_vertices(const int32_t* __restrict__ faces, int f, int n_pts, const float* __restrict__ pts,
                                              int32_t* idx, float p[3][3])
{
    int32_t i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    if ((uint32_t)i0 >= (uint32_t)n_pts || (uint32_t)i1 >= (uint32_t)n_pts || (uint32_t)i2 >= (uint32_t)n_pts) return false;
    int32_t t;
    if (i1 < i0) { t = i0; i0 = i1; i1 = t; }
    if (i2 < i1) { t = i1; i1 = i2; i2 = t; }
    if (i1 < i0) { t = i0; i0 = i1; i1 = t; }
    idx[0] = i0; idx[1] = i1; idx[2] = i2;
    for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) p[j][k] = pts[3 * (size_t)idx[j] + k];
    return rs::finite3(p[0]) && rs::finite3(p[1]) && rs::finite3(p[2]);
}

__global__ __launch_bounds__(256) void render_tris(const float* __restrict__ pts, const uint8_t* __restrict__ cols, int n_pts,
                                                   const int32_t* __restrict__ faces, int n_faces,
                                                   const double* __restrict__ views, rs::Camera cam, int mode, uint64_t* keys,
                                                   LargeItem* items, unsigned long long* count, int cap,
                                                   unsigned long long* g_stats)
{
    __shared__ unsigned long long s_stat[kStats];
    if (threadIdx.x < kStats) s_stat[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long mine[kStats] = {0, 0, 0, 0};
    const int f = blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (f < n_faces) {
        int32_t idx[3];
        float p[3][3];
        rs::ScreenPoly poly;
        int n = -1;
        if (face_vertices(faces, f, n_pts, pts, idx, p))
            n = rs::setup_triangle(cam, views + 12 * v, p[0], p[1], p[2], cols + 3 * (size_t)idx[0], cols + 3 * (size_t)idx[1],
                                   cols + 3 * (size_t)idx[2], &poly);
        if (n < 0) mine[0] = 1;
        else {
            const uint32_t id = ((uint32_t)rs::kTriangle << 30) | (uint32_t)f;
            uint64_t* kv = keys + (size_t)v * cam.w * cam.h;
            for (int piece = 0; piece < rs::fan_count(n); piece++) {
                rs::ScreenTri t;
                if (!rs::tri_prepare(cam, poly, piece, &t)) continue;
                const int bw = t.bx1 - t.bx0 + 1, bh = t.by1 - t.by0 + 1;
                const long long area = (long long)bw * bh;
                mine[2]++;
                mine[3] += (unsigned long long)area;
                if (mode == 1 || (mode == 0 && area <= kSmallArea)) {
                    raster_box(t, t.bx0, t.by0, t.bx1, t.by1, id, kv, cam.w);
                    continue;
                }
                int T = kTile;
                while ((long long)((bw + T - 1) / T) * ((bh + T - 1) / T) > kMaxTiles) T <<= 1;
                const int tx = (bw + T - 1) / T, ty = (bh + T - 1) / T;
                const unsigned long long base = atomicAdd(count, (unsigned long long)(tx * ty));
                const int x0 = t.bx0, y0 = t.by0, x1 = t.bx1, y1 = t.by1;
                for (int j = 0; j < ty; j++)
                    for (int i = 0; i < tx; i++) {
                        const int ax = x0 + i * T, ay = y0 + j * T;
                        const int bx = min(ax + T - 1, x1), by = min(ay + T - 1, y1);
                        const unsigned long long slot = base + (unsigned long long)(j * tx + i);
                        if (slot < (unsigned long long)cap) {
                            LargeItem it;
                            it.t = t;
                            it.t.bx0 = ax; it.t.by0 = ay; it.t.bx1 = bx; it.t.by1 = by;
                            it.id = id;
                            it.view = (uint32_t)v;
                            items[slot] = it;
                        } else {
                            raster_box(t, ax, ay, bx, by, id, kv, cam.w);
                        }
                    }
            }
            if (mine[2] == 0) mine[1] = 1;
        }
    }
    block_stats(s_stat, mine, g_stats);
}

__global__ __launch_bounds__(64) void render_large(const LargeItem* __restrict__ items, const unsigned long long* __restrict__ count,
                                                   int cap, uint64_t* keys, int w, int h)
{
    const int lane = threadIdx.x;
    const unsigned long long total = *count;
    const int n = (int)(total < (unsigned long long)cap ? total : (unsigned long long)cap);
    for (int e = blockIdx.x; e < n; e += gridDim.x) {
        const LargeItem it = items[e];
        uint64_t* kv = keys + (size_t)it.view * w * h;
        const int tw = it.t.bx1 - it.t.bx0 + 1, th = it.t.by1 - it.t.by0 + 1;
        const int npx = tw * th;
        for (int i = lane; i < npx; i += 64) {
            const int px = it.t.bx0 + i % tw, py = it.t.by0 + i / tw;
            int64_t wt[3];
            if (rs::tri_cover(it.t, px, py, wt)) put_key(kv, (size_t)py * w + px, rs::tri_depth(it.t, wt), it.id);
        }
    }
}

__global__ __launch_bounds__(256) void render_resolve(const uint64_t* __restrict__ keys, const float* __restrict__ pts,
                                                      const uint8_t* __restrict__ cols, int n_pts, const int32_t* __restrict__ faces,
                                                      const uint8_t* __restrict__ line_cols, const double* __restrict__ views,
                                                      rs::Camera cam, uint8_t* out, int32_t* ids, float* depth)
{
    const size_t wh = (size_t)cam.w * cam.h;
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int v = blockIdx.y;
    if (pix >= wh) return;
    const uint64_t key = keys[(size_t)v * wh + pix];
    uint8_t bgr[3] = {255, 255, 255};
    int32_t id = -1;
    float d = 0.f;
    if (key != rs::kEmptyKey) {
        const uint32_t lo = (uint32_t)key, kind = lo >> 30, index = lo & ((1u << 30) - 1);
        id = (int32_t)lo;
        d = rs::bits_float(~(uint32_t)(key >> 32));
        if (kind == rs::kPoint) {
            for (int k = 0; k < 3; k++) bgr[k] = cols[3 * (size_t)index + k];
        } else if (kind == rs::kLine) {
            for (int k = 0; k < 3; k++) bgr[k] = line_cols[3 * (size_t)index + k];
        } else {
            const int px = (int)(pix % cam.w), py = (int)(pix / cam.w);
            int32_t idx[3];
            float p[3][3];
            rs::ScreenPoly poly;
            int n = 0;
            if (face_vertices(faces, (int)index, n_pts, pts, idx, p))
                n = rs::setup_triangle(cam, views + 12 * v, p[0], p[1], p[2], cols + 3 * (size_t)idx[0],
                                       cols + 3 * (size_t)idx[1], cols + 3 * (size_t)idx[2], &poly);
            for (int piece = 0; piece < rs::fan_count(n); piece++) {
                rs::ScreenTri t;
                int64_t wt[3];
                if (!rs::tri_prepare(cam, poly, piece, &t)) continue;
                if (px < t.bx0 || px > t.bx1 || py < t.by0 || py > t.by1 || !rs::tri_cover(t, px, py, wt)) continue;
                rs::tri_color(t, wt, bgr);
                break;
            }
        }
    }
    uint8_t* o = out + ((size_t)v * wh + pix) * 3;
    o[0] = bgr[0]; o[1] = bgr[1]; o[2] = bgr[2];
    if (ids) ids[(size_t)v * wh + pix] = id;
    if (depth) depth[(size_t)v * wh + pix] = d;
}

bool render_args_ok(int n_pts, int n_faces, int n_lines, const void* pts, const void* colors, const void* faces, const void* lines,
                    const void* line_colors, const double* views, int nv, const double* cam, int w, int h, int point_size)
{
    constexpr int kMaxPrims = 1 << rs::kIndexBits;
    if (n_pts < 0 || n_faces < 0 || n_lines < 0 || nv < 0 || n_pts > kMaxPrims || n_faces > kMaxPrims || n_lines > kMaxPrims)
        return false;
    if ((n_pts > 0 && (!pts || !colors)) || (n_faces > 0 && !faces) || (n_lines > 0 && (!lines || !line_colors))) return false;
    if (!cam || !rs::camera_valid(cam, w, h)) return false;
    if (point_size < 1 || point_size > rs::kMaxPointSize || !(point_size & 1)) return false;
    if (nv > 0 && !views) return false;
    for (int i = 0; i < nv * 12; i++)
        if (!std::isfinite(views[i])) return false;
    return true;
}

int render_run(slam_ctx* c, hipStream_t s, const float* d_pts, const uint8_t* d_colors, int n_pts, const int32_t* d_faces,
               int n_faces, const float* d_lines, const uint8_t* d_line_colors, int n_lines, const double* views, int nv,
               const double* camv, int w, int h, int point_size, uint8_t* d_out, int32_t* d_ids, float* d_depth,
               int chunk_views, int raster_mode)
{
    const rs::Camera cam = rs::make_camera(camv, w, h);
    const size_t wh = (size_t)w * h;
    int chunk = (int)std::max<size_t>(1, kKeyBudget / (wh * 8));
    chunk = std::min(std::min(chunk, kMaxChunk), nv);
    if (chunk_views > 0) chunk = std::min(chunk, chunk_views);
    const int nchunks = (nv + chunk - 1) / chunk;
    const int mode = raster_mode == 3 ? 2 : raster_mode;
    const int cap = raster_mode == 3 ? kTinyPool : kLargePool;
    DevLayout lay;
    const auto s_hdr = lay.add<RenderHdr>(1);     // first: slam_render_last_stats reads it at the buffer's start
    const auto s_count = lay.add<unsigned long long>(1);
    const auto s_views = lay.add<double>((size_t)nv * 12);
    const auto s_items = lay.add<LargeItem>((size_t)kLargePool);
    const auto s_keys = lay.add<uint64_t>((size_t)chunk * wh);
    DevMem ws;
    SLAM_HIP(c, ws.bind(c->render_ws, lay));
    RenderHdr* hdr = ws.ptr(s_hdr);
    unsigned long long* count = ws.ptr(s_count);
    double* d_views = ws.ptr(s_views);
    LargeItem* items = ws.ptr(s_items);
    uint64_t* keys = ws.ptr(s_keys);
    // five events per chunk: the passes are timed without a host wait between chunks
    while (c->render_evs.size() < (size_t)nchunks * 5) {
        hipEvent_t e = nullptr;
        SLAM_HIP(c, hipEventCreate(&e));
        c->render_evs.push_back(e);
    }
    SLAM_HIP(c, ws.upload(s_views, views, s));

    SLAM_HIP(c, hipMemsetAsync(hdr, 0, sizeof(RenderHdr), s));
    for (double& m : c->render_ms) m = 0;
    c->render_in_count = (unsigned long long)nv * ((unsigned long long)n_pts + n_faces + n_lines);
    c->render_ran = true;
    c->render_stream = s;
    for (int v0 = 0, k = 0; v0 < nv; v0 += chunk, k++) {
        const int cv = std::min(chunk, nv - v0);
        hipEvent_t* ev = c->render_evs.data() + 5 * k;
        const double* cviews = d_views + 12 * (size_t)v0;
        SLAM_HIP(c, hipEventRecord(ev[0], s));
        SLAM_HIP(c, hipMemsetAsync(keys, 0xff, (size_t)cv * wh * 8, s));
        SLAM_HIP(c, hipMemsetAsync(count, 0, sizeof(unsigned long long), s));
        SLAM_HIP(c, hipEventRecord(ev[1], s));
        if (n_pts > 0)
            hipLaunchKernelGGL(render_points, dim3((n_pts + 255) / 256, cv), dim3(256), 0, s, d_pts, n_pts, cviews, cam,
                               (point_size - 1) / 2, keys, hdr->stats);
        if (n_lines > 0)
            hipLaunchKernelGGL(render_lines, dim3(n_lines, cv), dim3(64), 0, s, d_lines, cviews, cam, keys, hdr->stats);
        SLAM_HIP(c, hipEventRecord(ev[2], s));
        if (n_faces > 0) {
            hipLaunchKernelGGL(render_tris, dim3((n_faces + 255) / 256, cv), dim3(256), 0, s, d_pts, d_colors, n_pts, d_faces,
                               n_faces, cviews, cam, mode, keys, items, count, cap, hdr->stats);
            if (mode != 1)
                hipLaunchKernelGGL(render_large, dim3(kLargeBlocks), dim3(64), 0, s, items, count, cap, keys, w, h);
        }
        SLAM_HIP(c, hipEventRecord(ev[3], s));
        hipLaunchKernelGGL(render_resolve, dim3((unsigned)((wh + 255) / 256), cv), dim3(256), 0, s, keys, d_pts, d_colors, n_pts,
                           d_faces, d_line_colors, cviews, cam, d_out + (size_t)v0 * wh * 3, d_ids ? d_ids + (size_t)v0 * wh : nullptr,
                           d_depth ? d_depth + (size_t)v0 * wh : nullptr);
        SLAM_HIP(c, hipEventRecord(ev[4], s));
        SLAM_HIP(c, hipGetLastError());
        // the list and the key buffer are reused by the next chunk: stream order keeps them apart
    }
    // the call returns when the frames are there (views is the caller's host memory)
    SLAM_HIP(c, hipStreamSynchronize(s));
    for (int k = 0; k < nchunks; k++)
        for (int i = 0; i < 4; i++) {
            float ms = 0.f;
            SLAM_HIP(c, hipEventElapsedTime(&ms, c->render_evs[5 * k + i], c->render_evs[5 * k + i + 1]));
            c->render_ms[i] += ms;
        }
    return SLAM_OK;
}

}  // namespace

void render_release(slam_ctx* c)
{
    for (hipEvent_t e : c->render_evs) (void)hipEventDestroy(e);
    c->render_evs.clear();
}

}  // namespace slamhip

using namespace slamhip;

extern "C" {

int slam_render_views_dev(slam_ctx* c, void* stream, const float* d_pts, const uint8_t* d_colors, int n_pts,
                          const int32_t* d_faces, int n_faces, const float* d_lines, const uint8_t* d_line_colors, int n_lines,
                          const double* views, int nv, const double* cam, int w, int h, int point_size, uint8_t* d_out,
                          int32_t* d_ids, float* d_depth, int chunk_views, int raster_mode)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!render_args_ok(n_pts, n_faces, n_lines, d_pts, d_colors, d_faces, d_lines, d_line_colors, views, nv, cam, w, h,
                        point_size) ||
        (nv > 0 && !d_out) || chunk_views < 0 || raster_mode < 0 || raster_mode > 3)
        return set_err(c, SLAM_E_INVALID_ARG, "slam_render_views_dev: bad size, point_size, camera or view");
    if (nv == 0) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    return render_run(c, s, d_pts, d_colors, n_pts, d_faces, n_faces, d_lines, d_line_colors, n_lines, views, nv, cam, w, h,
                      point_size, d_out, d_ids, d_depth, chunk_views, raster_mode);
}

int slam_render(slam_ctx* c, const float* pts, const uint8_t* colors, int n_pts, const int32_t* faces, int n_faces,
                const float* lines, const uint8_t* line_colors, int n_lines, const double* view, const double* cam, int w,
                int h, int point_size, uint8_t* out, int32_t* ids, float* depth)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!view || !out ||
        !render_args_ok(n_pts, n_faces, n_lines, pts, colors, faces, lines, line_colors, view, 1, cam, w, h, point_size))
        return set_err(c, SLAM_E_INVALID_ARG, "slam_render: bad size, point_size, camera or view");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t wh = (size_t)w * h;
    DevLayout lin, lout;
    const auto s_pts = lin.add<float>((size_t)n_pts * 3);
    const auto s_col = lin.add<uint8_t>((size_t)n_pts * 3);
    const auto s_faces = lin.add<int32_t>((size_t)n_faces * 3);
    const auto s_lines = lin.add<float>((size_t)n_lines * 6);
    const auto s_lcol = lin.add<uint8_t>((size_t)n_lines * 3);
    const auto s_out = lout.add<uint8_t>(wh * 3);
    const auto s_ids = lout.add<int32_t>(wh);
    const auto s_depth = lout.add<float>(wh);
    DevMem in, res;
    SLAM_HIP(c, in.bind(c->render_in, lin));
    SLAM_HIP(c, res.bind(c->render_out, lout));
    if (n_pts) {
        SLAM_HIP(c, in.upload(s_pts, pts, s));
        SLAM_HIP(c, in.upload(s_col, colors, s));
    }
    if (n_faces) SLAM_HIP(c, in.upload(s_faces, faces, s));
    if (n_lines) {
        SLAM_HIP(c, in.upload(s_lines, lines, s));
        SLAM_HIP(c, in.upload(s_lcol, line_colors, s));
    }
    const int rc = render_run(c, s, in.ptr(s_pts), in.ptr(s_col), n_pts, in.ptr(s_faces), n_faces, in.ptr(s_lines), in.ptr(s_lcol),
                              n_lines, view, 1, cam, w, h, point_size, res.ptr(s_out), ids ? res.ptr(s_ids) : nullptr,
                              depth ? res.ptr(s_depth) : nullptr, 0, 0);
    if (rc != SLAM_OK) return rc;
    SLAM_HIP(c, res.download(out, s_out, s));
    if (ids) SLAM_HIP(c, res.download(ids, s_ids, s));
    if (depth) SLAM_HIP(c, res.download(depth, s_depth, s));
    SLAM_HIP(c, hipStreamSynchronize(s));
    return SLAM_OK;
}

int slam_render_last_stats(slam_ctx* c, uint64_t* stats, double* ms)
{
    if (!c || !stats) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < 5; i++) stats[i] = 0;
    if (ms)
        for (int i = 0; i < 4; i++) ms[i] = 0;
    if (!c->render_ws.p || !c->render_ran) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    RenderHdr h;
    SLAM_HIP(c, hipMemcpyAsync(&h, c->render_ws.p, sizeof(h), hipMemcpyDeviceToHost, c->render_stream));
    SLAM_HIP(c, hipStreamSynchronize(c->render_stream));
    stats[0] = c->render_in_count;
    for (int i = 0; i < kStats; i++) stats[1 + i] = h.stats[i];
    if (ms)
        for (int i = 0; i < 4; i++) ms[i] = c->render_ms[i];
    return SLAM_OK;
}

}  // extern "C"

// TSDF fusion and marching cubes on the device (tests/tsdf_ref.py is
// the definition of every value computed here, tsdf_math.h the shared arithmetic,
// tsdf_table.h the generated 256-case table):
//
//   tsdf_integrate       one thread per node, x along the lane.  The loop over the call's maps
//                        runs inside the thread with the six sums in registers: the volume is
//                        read once and written once per call.  A map's 12 entries of P and its
//                        frame index are read from the parameter block at a wave-uniform
//                        address (scalar loads).  No atomics, no culling.
//   tsdf_classify        a workgroup owns 32 x 4 x 4 nodes; the known / inside flags of the
//                        block plus a one-node halo go through LDS.  Per node one byte: the
//                        3-bit edge mask, the triangle count of the node's cell, the two flags.
//   tsdf_count           one wave per x row: the row's vertex and triangle counts.
//   tsdf_scan            one workgroup: the exclusive scan of the row counts (rows are in
//                        raster order, so the scan numbers vertices and faces in raster order)
//                        and the two totals, which the host reads before anything is emitted.
//   tsdf_emit_vertices   one wave per row: the in-row prefix by lane shuffles, the node's
//                        vertex base index to scratch, positions and colours to the output.
//   tsdf_emit_faces      one wave per row: a face's vertex index is base[owner] +
//                        popcount(mask[owner] & ((1 << axis) - 1)).
//
// count -> scan -> emit: no atomics, order-preserving (the idea of fast_emit and mvs_emit).
#include "slamhip_internal.h"
#include "tsdf_math.h"
#define TSDF_TABLE_ATTR __device__
#include "tsdf_table.h"

#include <cstring>

namespace slamhip {
namespace {

constexpr int kWave = 64;

// ---- integration -------------------------------------------------------------------

constexpr int kIntThreads = 256, kIntRows = kIntThreads / kWave;

struct TsdfMapDesc {
    double P[12];
    int32_t frame, pad;
};

struct TsdfGrid {
    int nx, ny, nz;
    double ox, oy, oz, voxel;
};

__global__ __launch_bounds__(kIntThreads) void tsdf_integrate(int32_t* __restrict__ vol, TsdfGrid g, double trunc,
                                                              const TsdfMapDesc* __restrict__ maps, int nmaps,
                                                              const uint8_t* __restrict__ frames,
                                                              const float* __restrict__ inv, int w, int h, int channels)
{
    const int i = blockIdx.x * kWave + (threadIdx.x & (kWave - 1));
    const int j = blockIdx.y * kIntRows + (threadIdx.x / kWave);
    const int k = blockIdx.z;
    if (i >= g.nx || j >= g.ny) return;
    const size_t nn = (size_t)g.nx * g.ny * g.nz, npx = (size_t)w * h;
    const size_t o = ((size_t)k * g.ny + j) * g.nx + i;
    const double X = tsdf_coord(g.ox, i, g.voxel), Y = tsdf_coord(g.oy, j, g.voxel), Z = tsdf_coord(g.oz, k, g.voxel);
    TsdfNode n = {vol[o], vol[nn + o], vol[2 * nn + o], vol[3 * nn + o], vol[4 * nn + o], vol[5 * nn + o]};
    for (int m = 0; m < nmaps; m++) {
        const TsdfMapDesc& d = maps[m];
        tsdf_integrate_node(n, d.P, X, Y, Z, inv + (size_t)m * npx, frames + (size_t)d.frame * npx * channels, w, h,
                            channels, trunc);
    }
    vol[o] = n.D;
    vol[nn + o] = n.W;
    vol[2 * nn + o] = n.CW;
    vol[3 * nn + o] = n.B;
    vol[4 * nn + o] = n.G;
    vol[5 * nn + o] = n.R;
}

// ---- classification ----------------------------------------------------------------

constexpr int kClsX = 32, kClsY = 4, kClsZ = 4, kClsThreads = kClsX * kClsY * kClsZ;     // 512
constexpr int kClsLX = kClsX + 2, kClsLY = kClsY + 2, kClsLZ = kClsZ + 2;

// the eight corners of the cell whose low corner is the (-1, -1, -1) neighbour, as bits of the
// 27-bit neighbourhood word (bit x + 3 y + 9 z, offsets 0 .. 2)
constexpr uint32_t kCell0 = 0x1Bu | (0x1Bu << 9);

__global__ __launch_bounds__(kClsThreads) void tsdf_classify(const int32_t* __restrict__ vol, int nx, int ny, int nz,
                                                             int min_weight, uint8_t* __restrict__ info)
{
    __shared__ uint8_t fl[kClsLZ][kClsLY][kClsLX + 2];
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * kClsX, Y0 = blockIdx.y * kClsY, Z0 = blockIdx.z * kClsZ;
    const size_t nn = (size_t)nx * ny * nz;
    for (int p = tid; p < kClsLZ * kClsLY * kClsLX; p += kClsThreads) {
        const int lz = p / (kClsLY * kClsLX), r = p - lz * (kClsLY * kClsLX), ly = r / kClsLX, lx = r - ly * kClsLX;
        const int x = X0 - 1 + lx, y = Y0 - 1 + ly, z = Z0 - 1 + lz;
        uint8_t f = 0;
        if (x >= 0 && y >= 0 && z >= 0 && x < nx && y < ny && z < nz) {
            const size_t o = ((size_t)z * ny + y) * nx + x;
            f = tsdf_node_flags(vol[o], vol[nn + o], min_weight);
        }
        fl[lz][ly][lx] = f;
    }
    __syncthreads();
    const int lx = tid % kClsX, ly = (tid / kClsX) % kClsY, lz = tid / (kClsX * kClsY);
    const int x = X0 + lx, y = Y0 + ly, z = Z0 + lz;
    if (x >= nx || y >= ny || z >= nz) return;
    uint32_t kn = 0, in = 0;
#pragma unroll
    for (int dz = 0; dz < 3; dz++)
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
            for (int dx = 0; dx < 3; dx++) {
                const uint32_t f = fl[lz + dz][ly + dy][lx + dx];
                kn |= ((f >> 6) & 1u) << (dx + 3 * dy + 9 * dz);
                in |= ((f >> 7) & 1u) << (dx + 3 * dy + 9 * dz);
            }
    // the cell whose low corner is the neighbour at offset (cx, cy, cz) in {-1, 0}
    auto active = [&](int cx, int cy, int cz) {
        const uint32_t m = kCell0 << ((cx + 1) + 3 * (cy + 1) + 9 * (cz + 1));
        return (kn & m) == m;
    };
    constexpr int kCentre = 13, kStep[3] = {1, 3, 9};
    int mask = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int far = kCentre + kStep[a];
        const bool cross = ((kn >> kCentre) & (kn >> far) & 1u) && (((in >> kCentre) ^ (in >> far)) & 1u);
        bool any = false;
#pragma unroll
        for (int db = 0; db < 2; db++)
#pragma unroll
            for (int dc = 0; dc < 2; dc++) {
                int c[3] = {0, 0, 0};
                c[(a + 1) % 3] = -db;
                c[(a + 2) % 3] = -dc;
                any = any || active(c[0], c[1], c[2]);
            }
        if (cross && any) mask |= 1 << a;
    }
    int nf = 0;
    if (active(0, 0, 0)) {
        int cs = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) cs |= (int)((in >> (kCentre + (c & 1) + 3 * ((c >> 1) & 1) + 9 * (c >> 2))) & 1u) << c;
        nf = kTsdfTriCount[cs];
    }
    const uint32_t f0 = fl[lz + 1][ly + 1][lx + 1];
    info[((size_t)z * ny + y) * nx + x] = (uint8_t)(f0 | mask | (nf << kTsdfFaceShift));
}

// ---- count, scan, emit ---------------------------------------------------------------

constexpr int kRowThreads = 256, kRowsPerBlock = kRowThreads / kWave;

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

// inclusive prefix over the wave's lanes
__device__ __forceinline__ int wave_scan(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int t = __shfl_up(v, d, kWave);
        if (lane >= d) v += t;
    }
    return v;
}

__global__ __launch_bounds__(kRowThreads) void tsdf_count(const uint8_t* __restrict__ info, int nx, long long nrows,
                                                          int32_t* __restrict__ rowcnt)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long r = (long long)blockIdx.x * kRowsPerBlock + threadIdx.x / kWave;
    if (r >= nrows) return;                                  // uniform in the wave
    const uint8_t* row = info + (size_t)r * nx;
    int v = 0, f = 0;
    for (int i = lane; i < nx; i += kWave) {
        const int b = row[i];
        v += tsdf_popc3(b & kTsdfMaskBits);
        f += (b >> kTsdfFaceShift) & 7;
    }
    v = wave_sum(v);
    f = wave_sum(f);
    if (lane == 0) {
        rowcnt[2 * r] = v;
        rowcnt[2 * r + 1] = f;
    }
}

constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(kScanThreads) void tsdf_scan(const int32_t* __restrict__ rowcnt, long long nrows,
                                                          int32_t* __restrict__ rowbase, int64_t* __restrict__ totals)
{
    __shared__ int64_t sc[2][2][kScanThreads];
    const int t = threadIdx.x;
    const long long per = (nrows + kScanThreads - 1) / kScanThreads;
    const long long r0 = min(nrows, t * per), r1 = min(nrows, (t + 1) * per);
    int64_t v = 0, f = 0;
    for (long long r = r0; r < r1; r++) {
        v += rowcnt[2 * r];
        f += rowcnt[2 * r + 1];
    }
    sc[0][0][t] = v;
    sc[0][1][t] = f;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kScanThreads; d <<= 1, cur ^= 1) {
        sc[cur ^ 1][0][t] = sc[cur][0][t] + (t >= d ? sc[cur][0][t - d] : 0);
        sc[cur ^ 1][1][t] = sc[cur][1][t] + (t >= d ? sc[cur][1][t - d] : 0);
        __syncthreads();
    }
    int64_t bv = sc[cur][0][t] - v, bf = sc[cur][1][t] - f;
    for (long long r = r0; r < r1; r++) {
        rowbase[2 * r] = (int32_t)bv;          // past 2^31 - 1 the host refuses the totals and nothing reads these
        rowbase[2 * r + 1] = (int32_t)bf;
        bv += rowcnt[2 * r];
        bf += rowcnt[2 * r + 1];
    }
    if (t == kScanThreads - 1) {
        totals[0] = sc[cur][0][t];
        totals[1] = sc[cur][1][t];
    }
}

__global__ __launch_bounds__(kRowThreads) void tsdf_emit_vertices(const int32_t* __restrict__ vol,
                                                                  const uint8_t* __restrict__ info, TsdfGrid g,
                                                                  long long nrows, const int32_t* __restrict__ rowbase,
                                                                  int32_t* __restrict__ vbase, double* __restrict__ verts,
                                                                  uint8_t* __restrict__ cols)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long r = (long long)blockIdx.x * kRowsPerBlock + threadIdx.x / kWave;
    if (r >= nrows) return;                                  // uniform in the wave
    const int j = (int)(r % g.ny), k = (int)(r / g.ny);
    const size_t nn = (size_t)g.nx * g.ny * g.nz;
    const size_t step[3] = {1, (size_t)g.nx, (size_t)g.nx * g.ny};
    int carry = rowbase[2 * r];
    for (int c0 = 0; c0 < g.nx; c0 += kWave) {
        const int i = c0 + lane;
        const size_t o = (size_t)r * g.nx + i;
        const int mask = i < g.nx ? (info[o] & kTsdfMaskBits) : 0;
        const int cnt = tsdf_popc3(mask);
        const int incl = wave_scan(cnt, lane);
        int base = carry + incl - cnt;
        carry += __shfl(incl, kWave - 1, kWave);
        if (!mask) continue;
        vbase[o] = base;
        const int idx[3] = {i, j, k};
        const double org[3] = {g.ox, g.oy, g.oz};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (!((mask >> a) & 1)) continue;
            const size_t o2 = o + step[a];
            const double t = tsdf_edge_t(vol[o], vol[nn + o], vol[o2], vol[nn + o2]);
            double X[3] = {tsdf_coord(g.ox, i, g.voxel), tsdf_coord(g.oy, j, g.voxel), tsdf_coord(g.oz, k, g.voxel)};
            X[a] = org[a] + ((double)idx[a] + t) * g.voxel;
            const int32_t cwa = vol[2 * nn + o], cwb = vol[2 * nn + o2];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                verts[(size_t)base * 3 + c] = X[c];
                cols[(size_t)base * 3 + c] = tsdf_mix_color(tsdf_node_color(vol[(3 + c) * nn + o], cwa),
                                                            tsdf_node_color(vol[(3 + c) * nn + o2], cwb), t);
            }
            base++;
        }
    }
}

__global__ __launch_bounds__(kRowThreads) void tsdf_emit_faces(const uint8_t* __restrict__ info, int nx, int ny,
                                                               long long nrows, const int32_t* __restrict__ rowbase,
                                                               const int32_t* __restrict__ vbase,
                                                               int32_t* __restrict__ faces)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long r = (long long)blockIdx.x * kRowsPerBlock + threadIdx.x / kWave;
    if (r >= nrows) return;                                  // uniform in the wave
    const size_t step[3] = {1, (size_t)nx, (size_t)nx * ny};
    int carry = rowbase[2 * r + 1];
    for (int c0 = 0; c0 < nx; c0 += kWave) {
        const int i = c0 + lane;
        const size_t o = (size_t)r * nx + i;
        const int nf = i < nx ? ((info[o] >> kTsdfFaceShift) & 7) : 0;
        const int incl = wave_scan(nf, lane);
        const int base = carry + incl - nf;
        carry += __shfl(incl, kWave - 1, kWave);
        if (!nf) continue;                     // nf > 0: the cell is active, its eight corners are nodes of the grid
        int cs = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const size_t oc = o + (c & 1) * step[0] + ((c >> 1) & 1) * step[1] + (c >> 2) * step[2];
            cs |= (int)((info[oc] >> 7) & 1) << c;
        }
        for (int e3 = 0; e3 < 3 * nf; e3++) {
            const int e = kTsdfTriEdges[cs][e3], c = tsdf_edge_owner(e), a = e >> 2;
            const size_t oc = o + (c & 1) * step[0] + ((c >> 1) & 1) * step[1] + (c >> 2) * step[2];
            faces[(size_t)base * 3 + e3] = vbase[oc] + tsdf_popc3(info[oc] & ((1 << a) - 1));
        }
    }
}

hipError_t tsdf_events(slam_ctx* c)
{
    for (auto& e : c->tsdf_ev)
        if (!e) {
            const hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return rc;
        }
    return hipSuccess;
}

double tsdf_elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (double)ms : 0.0;
}

TsdfGrid make_grid(int nx, int ny, int nz, const double* origin, double voxel)
{
    return TsdfGrid{nx, ny, nz, origin[0], origin[1], origin[2], voxel};
}

}  // namespace

void tsdf_release(slam_ctx* c)
{
    for (auto& e : c->tsdf_ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_tsdf_last_timing(slam_ctx* c, double* ms)
{
    if (!c || !ms) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < 4; i++) ms[i] = c->tsdf_ms[i];
    return SLAM_OK;
}

extern "C" int slam_tsdf_integrate_dev(slam_ctx* c, void* stream, int32_t* d_volume, int nx, int ny, int nz,
                                       const double* origin, double voxel, double trunc, const uint8_t* d_frames,
                                       int nframes, int w, int h, int channels, const int32_t* frame_idx,
                                       const float* d_inv_depth, const double* P, int nmaps)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (int rc = tsdf_check_volume(d_volume, nx, ny, nz, origin, voxel))
        return set_err(c, rc, rc == SLAM_E_UNSUPPORTED ? "tsdf: each dimension 2..2048 and at most 2^30 nodes"
                                                       : "tsdf: null volume or origin, or a non-finite origin or voxel, or voxel <= 0");
    if (int rc = tsdf_check_maps(trunc, d_frames, nframes, w, h, channels, frame_idx, d_inv_depth, P, nmaps))
        return set_err(c, rc, "tsdf integrate: trunc > 0 finite, nmaps 0..2^20, frames of 1 or 3 channels, frame indices "
                              "inside the batch, finite P");
    if (nmaps == 0) return SLAM_OK;
    std::vector<TsdfMapDesc> maps((size_t)nmaps);
    for (int m = 0; m < nmaps; m++) {
        memcpy(maps[m].P, P + (size_t)m * 12, sizeof(double) * 12);
        maps[m].frame = frame_idx ? frame_idx[m] : m;
        maps[m].pad = 0;
    }
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    DevLayout lay;
    const auto s_maps = lay.add<TsdfMapDesc>((size_t)nmaps);
    DevMem mem;
    SLAM_HIP(c, mem.bind(c->tsdf_par, lay));
    SLAM_HIP(c, mem.upload(s_maps, maps.data(), s));
    SLAM_HIP(c, tsdf_events(c));
    SLAM_HIP(c, hipEventRecord(c->tsdf_ev[0], s));
    const dim3 grid((nx + kWave - 1) / kWave, (ny + kIntRows - 1) / kIntRows, nz);
    hipLaunchKernelGGL(tsdf_integrate, grid, dim3(kIntThreads), 0, s, d_volume, make_grid(nx, ny, nz, origin, voxel), trunc,
                       mem.ptr(s_maps), nmaps, d_frames, d_inv_depth, w, h, channels);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(c->tsdf_ev[1], s));
    if (int rc = stream_sync(c, s)) return rc;          // the parameter block is host memory of this call
    c->tsdf_ms[0] = tsdf_elapsed(c->tsdf_ev[0], c->tsdf_ev[1]);
    return SLAM_OK;
}

extern "C" int slam_tsdf_mesh_dev(slam_ctx* c, void* stream, const int32_t* d_volume, int nx, int ny, int nz,
                                  const double* origin, double voxel, int min_weight, double* d_vertices,
                                  uint8_t* d_colors, int32_t* d_faces, int cap_vertices, int cap_faces, int* nv_out,
                                  int* nf_out)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!nv_out || !nf_out) return set_err(c, SLAM_E_INVALID_ARG, "tsdf mesh: null count");
    *nv_out = *nf_out = 0;
    if (int rc = tsdf_check_volume(d_volume, nx, ny, nz, origin, voxel))
        return set_err(c, rc, rc == SLAM_E_UNSUPPORTED ? "tsdf: each dimension 2..2048 and at most 2^30 nodes"
                                                       : "tsdf: null volume or origin, or a non-finite origin or voxel, or voxel <= 0");
    if (min_weight < 1 || cap_vertices < 0 || cap_faces < 0 || (cap_vertices > 0 && (!d_vertices || !d_colors)) ||
        (cap_faces > 0 && !d_faces))
        return set_err(c, SLAM_E_INVALID_ARG, "tsdf mesh: min_weight >= 1, capacities >= 0 with their buffers");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    const size_t nn = (size_t)nx * ny * nz;
    const long long nrows = (long long)ny * nz;
    DevLayout lay;
    const auto s_info = lay.add<uint8_t>(nn);
    const auto s_vbase = lay.add<int32_t>(nn);
    const auto s_cnt = lay.add<int32_t>(2 * (size_t)nrows);
    const auto s_base = lay.add<int32_t>(2 * (size_t)nrows);
    const auto s_tot = lay.add<int64_t>(2);
    DevMem mem;
    SLAM_HIP(c, mem.bind(c->tsdf_ws, lay));
    SLAM_HIP(c, tsdf_events(c));
    c->tsdf_ms[1] = c->tsdf_ms[2] = c->tsdf_ms[3] = 0.0;
    SLAM_HIP(c, hipEventRecord(c->tsdf_ev[2], s));
    const dim3 cgrid((nx + kClsX - 1) / kClsX, (ny + kClsY - 1) / kClsY, (nz + kClsZ - 1) / kClsZ);
    hipLaunchKernelGGL(tsdf_classify, cgrid, dim3(kClsThreads), 0, s, d_volume, nx, ny, nz, min_weight, mem.ptr(s_info));
    SLAM_HIP(c, hipGetLastError());
    const unsigned rblocks = (unsigned)((nrows + kRowsPerBlock - 1) / kRowsPerBlock);
    hipLaunchKernelGGL(tsdf_count, dim3(rblocks), dim3(kRowThreads), 0, s, mem.ptr(s_info), nx, nrows, mem.ptr(s_cnt));
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(c->tsdf_ev[3], s));
    hipLaunchKernelGGL(tsdf_scan, dim3(1), dim3(kScanThreads), 0, s, mem.ptr(s_cnt), nrows, mem.ptr(s_base), mem.ptr(s_tot));
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(c->tsdf_ev[4], s));
    int64_t* tot = static_cast<int64_t*>(readback(c, 2 * sizeof(int64_t)));
    if (!tot) return set_err(c, SLAM_E_HIP, "tsdf mesh: no pinned readback space");
    SLAM_HIP(c, hipMemcpyAsync(tot, mem.ptr(s_tot), 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (int rc = stream_sync(c, s)) return rc;
    c->tsdf_ms[1] = tsdf_elapsed(c->tsdf_ev[2], c->tsdf_ev[3]);
    c->tsdf_ms[2] = tsdf_elapsed(c->tsdf_ev[3], c->tsdf_ev[4]);
    const int64_t tv = tot[0], tf = tot[1];
    if (tv > 0x7fffffff || tf > 0x7fffffff) return set_err(c, SLAM_E_UNSUPPORTED, "tsdf mesh: more than 2^31 - 1 vertices or faces");
    *nv_out = (int)tv;
    *nf_out = (int)tf;
    if (tv > cap_vertices || tf > cap_faces)
        return set_err(c, SLAM_E_CAPACITY, "tsdf mesh: output buffers too small (nv and nf hold the needed counts)");
    if (tv == 0) return SLAM_OK;
    const TsdfGrid g = make_grid(nx, ny, nz, origin, voxel);
    SLAM_HIP(c, hipEventRecord(c->tsdf_ev[5], s));
    hipLaunchKernelGGL(tsdf_emit_vertices, dim3(rblocks), dim3(kRowThreads), 0, s, d_volume, mem.ptr(s_info), g, nrows,
                       mem.ptr(s_base), mem.ptr(s_vbase), d_vertices, d_colors);
    SLAM_HIP(c, hipGetLastError());
    if (tf > 0) {
        hipLaunchKernelGGL(tsdf_emit_faces, dim3(rblocks), dim3(kRowThreads), 0, s, mem.ptr(s_info), nx, ny, nrows,
                           mem.ptr(s_base), mem.ptr(s_vbase), d_faces);
        SLAM_HIP(c, hipGetLastError());
    }
    SLAM_HIP(c, hipEventRecord(c->tsdf_ev[6], s));
    if (int rc = stream_sync(c, s)) return rc;
    c->tsdf_ms[3] = tsdf_elapsed(c->tsdf_ev[5], c->tsdf_ev[6]);
    return SLAM_OK;
}

extern "C" int slam_tsdf_integrate(slam_ctx* c, int32_t* volume, int nx, int ny, int nz, const double* origin, double voxel,
                                   double trunc, const uint8_t* frames, int nframes, int w, int h, int channels,
                                   const int32_t* frame_idx, const float* inv_depth, const double* P, int nmaps)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (int rc = tsdf_check_volume(volume, nx, ny, nz, origin, voxel)) return set_err(c, rc, "tsdf: bad volume arguments");
    if (int rc = tsdf_check_maps(trunc, frames, nframes, w, h, channels, frame_idx, inv_depth, P, nmaps))
        return set_err(c, rc, "tsdf integrate: bad map arguments");
    if (nmaps == 0) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    const size_t nn = (size_t)nx * ny * nz, npx = (size_t)w * h;
    DevLayout lay;
    const auto s_vol = lay.add<int32_t>(kTsdfPlanes * nn);
    const auto s_frames = lay.add<uint8_t>((size_t)nframes * npx * channels);
    const auto s_inv = lay.add<float>((size_t)nmaps * npx);
    DevMem mem;
    SLAM_HIP(c, mem.bind(c->tsdf_in, lay));
    SLAM_HIP(c, mem.upload(s_vol, volume, c->stream));
    SLAM_HIP(c, mem.upload(s_frames, frames, c->stream));
    SLAM_HIP(c, mem.upload(s_inv, inv_depth, c->stream));
    if (int rc = slam_tsdf_integrate_dev(c, c->stream, mem.ptr(s_vol), nx, ny, nz, origin, voxel, trunc, mem.ptr(s_frames),
                                         nframes, w, h, channels, frame_idx, mem.ptr(s_inv), P, nmaps))
        return rc;
    SLAM_HIP(c, mem.download(volume, s_vol, c->stream));
    return stream_sync(c, c->stream);
}

extern "C" int slam_tsdf_mesh(slam_ctx* c, const int32_t* volume, int nx, int ny, int nz, const double* origin, double voxel,
                              int min_weight, double* vertices, uint8_t* colors, int32_t* faces, int cap_vertices,
                              int cap_faces, int* nv_out, int* nf_out)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!nv_out || !nf_out) return set_err(c, SLAM_E_INVALID_ARG, "tsdf mesh: null count");
    *nv_out = *nf_out = 0;
    if (int rc = tsdf_check_volume(volume, nx, ny, nz, origin, voxel)) return set_err(c, rc, "tsdf: bad volume arguments");
    if (cap_vertices < 0 || cap_faces < 0 || (cap_vertices > 0 && (!vertices || !colors)) || (cap_faces > 0 && !faces))
        return set_err(c, SLAM_E_INVALID_ARG, "tsdf mesh: capacities >= 0 with their buffers");
    SLAM_HIP(c, hipSetDevice(c->device));
    const size_t nn = (size_t)nx * ny * nz;
    DevLayout lay;
    const auto s_vol = lay.add<int32_t>(kTsdfPlanes * nn);
    const auto s_v = lay.add<double>(3 * (size_t)cap_vertices);
    const auto s_c = lay.add<uint8_t>(3 * (size_t)cap_vertices);
    const auto s_f = lay.add<int32_t>(3 * (size_t)cap_faces);
    DevMem mem;
    SLAM_HIP(c, mem.bind(c->tsdf_in, lay));
    SLAM_HIP(c, mem.upload(s_vol, volume, c->stream));
    if (int rc = slam_tsdf_mesh_dev(c, c->stream, mem.ptr(s_vol), nx, ny, nz, origin, voxel, min_weight,
                                    cap_vertices ? mem.ptr(s_v) : nullptr, cap_vertices ? mem.ptr(s_c) : nullptr,
                                    cap_faces ? mem.ptr(s_f) : nullptr, cap_vertices, cap_faces, nv_out, nf_out))
        return rc;
    if (*nv_out > 0) {
        SLAM_HIP(c, mem.download(vertices, s_v, 3 * (size_t)*nv_out, c->stream));
        SLAM_HIP(c, mem.download(colors, s_c, 3 * (size_t)*nv_out, c->stream));
    }
    if (*nf_out > 0) SLAM_HIP(c, mem.download(faces, s_f, 3 * (size_t)*nf_out, c->stream));
    return stream_sync(c, c->stream);
}

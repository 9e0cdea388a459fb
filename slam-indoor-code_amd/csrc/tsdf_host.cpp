// TSDF fusion and marching cubes on the host: slam_tsdf_integrate_host and
// slam_tsdf_mesh_host, the twins of tsdf.hip's kernels.  They need no context and no
// device; the arithmetic is tsdf_math.h's and the table tsdf_table.h's, so the results
// equal the device's bit for bit.  z slices are dealt to up to 16 threads.
#include "../../include/slamhip.h"
#include "tsdf_math.h"
#include "tsdf_table.h"

#include <algorithm>
#include <functional>
#include <thread>
#include <vector>

namespace slamhip {

int tsdf_check_volume(const void* volume, int nx, int ny, int nz, const double* origin, double voxel)
{
    if (!volume || !origin) return SLAM_E_INVALID_ARG;
    if (nx < kTsdfMinDim || ny < kTsdfMinDim || nz < kTsdfMinDim || nx > kTsdfMaxDim || ny > kTsdfMaxDim || nz > kTsdfMaxDim ||
        (long long)nx * ny * nz > kTsdfMaxNodes)
        return SLAM_E_UNSUPPORTED;
    for (int i = 0; i < 3; i++)
        if (!tsdf_finite(origin[i])) return SLAM_E_INVALID_ARG;
    if (!tsdf_finite(voxel) || !(voxel > 0.0)) return SLAM_E_INVALID_ARG;
    return SLAM_OK;
}

// everything of an integrate call but the volume; nmaps == 0 is legal (the caller returns early)
int tsdf_check_maps(double trunc, const void* frames, int nframes, int w, int h, int channels, const int32_t* frame_idx,
                    const void* inv_depth, const double* P, int nmaps)
{
    if (!tsdf_finite(trunc) || !(trunc > 0.0) || nmaps < 0 || nmaps > kTsdfMaxMaps) return SLAM_E_INVALID_ARG;
    if (nframes < 1 || w < 1 || h < 1 || (channels != 1 && channels != 3) || (long long)w * h > (1ll << 30))
        return SLAM_E_INVALID_ARG;
    if (nmaps == 0) return SLAM_OK;
    if (!frames || !inv_depth || !P) return SLAM_E_INVALID_ARG;
    for (int m = 0; m < nmaps; m++) {
        const int f = frame_idx ? frame_idx[m] : m;
        if (f < 0 || f >= nframes) return SLAM_E_INVALID_ARG;
        for (int k = 0; k < 12; k++)
            if (!tsdf_finite(P[(size_t)m * 12 + k])) return SLAM_E_INVALID_ARG;
    }
    return SLAM_OK;
}

namespace {

void parallel_slices(int n, const std::function<void(int, int)>& fn)
{
    const int nthreads = std::max(1, std::min({16, (int)std::thread::hardware_concurrency(), n}));
    auto part = [&](int t) {
        const int a = (int)((long long)n * t / nthreads), b = (int)((long long)n * (t + 1) / nthreads);
        if (b > a) fn(a, b);
    };
    if (nthreads == 1) {
        part(0);
        return;
    }
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; t++) pool.emplace_back(part, t);
    part(0);
    for (auto& th : pool) th.join();
}

}  // namespace
}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_tsdf_integrate_host(int32_t* volume, int nx, int ny, int nz, const double* origin, double voxel,
                                        double trunc, const uint8_t* frames, int nframes, int w, int h, int channels,
                                        const int32_t* frame_idx, const float* inv_depth, const double* P, int nmaps)
{
    if (int rc = tsdf_check_volume(volume, nx, ny, nz, origin, voxel)) return rc;
    if (int rc = tsdf_check_maps(trunc, frames, nframes, w, h, channels, frame_idx, inv_depth, P, nmaps)) return rc;
    if (nmaps == 0) return SLAM_OK;
    const size_t nn = (size_t)nx * ny * nz, npx = (size_t)w * h;
    parallel_slices(nz, [&](int k0, int k1) {
        for (int k = k0; k < k1; k++) {
            const double Z = tsdf_coord(origin[2], k, voxel);
            for (int j = 0; j < ny; j++) {
                const double Y = tsdf_coord(origin[1], j, voxel);
                for (int i = 0; i < nx; i++) {
                    const double X = tsdf_coord(origin[0], i, voxel);
                    const size_t o = ((size_t)k * ny + j) * nx + i;
                    TsdfNode n = {volume[o], volume[nn + o], volume[2 * nn + o], volume[3 * nn + o], volume[4 * nn + o],
                                  volume[5 * nn + o]};
                    for (int m = 0; m < nmaps; m++) {
                        const int f = frame_idx ? frame_idx[m] : m;
                        tsdf_integrate_node(n, P + (size_t)m * 12, X, Y, Z, inv_depth + (size_t)m * npx,
                                            frames + (size_t)f * npx * channels, w, h, channels, trunc);
                    }
                    volume[o] = n.D;
                    volume[nn + o] = n.W;
                    volume[2 * nn + o] = n.CW;
                    volume[3 * nn + o] = n.B;
                    volume[4 * nn + o] = n.G;
                    volume[5 * nn + o] = n.R;
                }
            }
        }
    });
    return SLAM_OK;
}

extern "C" int slam_tsdf_mesh_host(const int32_t* volume, int nx, int ny, int nz, const double* origin, double voxel,
                                   int min_weight, double* vertices, uint8_t* colors, int32_t* faces, int cap_vertices,
                                   int cap_faces, int* nv_out, int* nf_out)
{
    if (!nv_out || !nf_out) return SLAM_E_INVALID_ARG;
    *nv_out = *nf_out = 0;
    if (int rc = tsdf_check_volume(volume, nx, ny, nz, origin, voxel)) return rc;
    if (min_weight < 1 || cap_vertices < 0 || cap_faces < 0 || (cap_vertices > 0 && (!vertices || !colors)) ||
        (cap_faces > 0 && !faces))
        return SLAM_E_INVALID_ARG;
    const size_t nn = (size_t)nx * ny * nz;
    const int32_t *D = volume, *W = volume + nn, *CW = volume + 2 * nn;
    auto at = [&](int i, int j, int k) { return ((size_t)k * ny + j) * nx + i; };
    std::vector<uint8_t> flag(nn);
    parallel_slices(nz, [&](int k0, int k1) {
        for (size_t o = at(0, 0, k0); o < at(0, 0, k1); o++) flag[o] = tsdf_node_flags(D[o], W[o], min_weight);
    });
    // known / inside of a node, 0 outside the grid
    auto fl = [&](int i, int j, int k) -> uint8_t {
        return (i < 0 || j < 0 || k < 0 || i >= nx || j >= ny || k >= nz) ? (uint8_t)0 : (uint8_t)(flag[at(i, j, k)] & (kTsdfKnown | kTsdfInside));
    };
    auto active = [&](int i, int j, int k) {     // the cell whose low corner is (i, j, k)
        for (int c = 0; c < 8; c++)
            if (!(fl(i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)) & kTsdfKnown)) return false;
        return true;
    };
    // masks and face counts into a second array: the flags of neighbours are read while they are written
    std::vector<uint8_t> info(nn);
    const size_t nrows = (size_t)ny * nz;
    std::vector<int64_t> row_v(nrows + 1), row_f(nrows + 1);
    parallel_slices(nz, [&](int k0, int k1) {
        for (int k = k0; k < k1; k++)
            for (int j = 0; j < ny; j++) {
                int64_t rv = 0, rf = 0;
                for (int i = 0; i < nx; i++) {
                    const uint8_t f0 = fl(i, j, k);
                    int mask = 0, nf = 0;
                    const int p[3] = {i, j, k};
                    for (int a = 0; a < 3; a++) {
                        int q[3] = {i, j, k};
                        q[a]++;
                        const uint8_t f1 = fl(q[0], q[1], q[2]);
                        if (!(f0 & f1 & kTsdfKnown) || !((f0 ^ f1) & kTsdfInside)) continue;
                        const int b = (a + 1) % 3, c = (a + 2) % 3;
                        bool any = false;
                        for (int db = 0; db < 2; db++)
                            for (int dc = 0; dc < 2; dc++) {
                                int cell[3] = {p[0], p[1], p[2]};
                                cell[b] -= db;
                                cell[c] -= dc;
                                any = any || active(cell[0], cell[1], cell[2]);
                            }
                        if (any) mask |= 1 << a;
                    }
                    if (active(i, j, k)) {
                        int cs = 0;
                        for (int c = 0; c < 8; c++)
                            if (fl(i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2)) & kTsdfInside) cs |= 1 << c;
                        nf = kTsdfTriCount[cs];
                    }
                    info[at(i, j, k)] = (uint8_t)(f0 | mask | (nf << kTsdfFaceShift));
                    rv += tsdf_popc3(mask);
                    rf += nf;
                }
                row_v[(size_t)k * ny + j] = rv;
                row_f[(size_t)k * ny + j] = rf;
            }
    });
    int64_t tv = 0, tf = 0;
    for (size_t r = 0; r < nrows; r++) {
        const int64_t v = row_v[r], f = row_f[r];
        row_v[r] = tv;
        row_f[r] = tf;
        tv += v;
        tf += f;
    }
    if (tv > 0x7fffffff || tf > 0x7fffffff) return SLAM_E_UNSUPPORTED;
    *nv_out = (int)tv;
    *nf_out = (int)tf;
    if (tv > cap_vertices || tf > cap_faces) return SLAM_E_CAPACITY;
    if (tv == 0) return SLAM_OK;
    std::vector<int32_t> vbase(nn);
    parallel_slices(nz, [&](int k0, int k1) {
        for (int k = k0; k < k1; k++)
            for (int j = 0; j < ny; j++) {
                int32_t base = (int32_t)row_v[(size_t)k * ny + j];
                for (int i = 0; i < nx; i++) {
                    const size_t o = at(i, j, k);
                    vbase[o] = base;
                    const int mask = info[o] & kTsdfMaskBits;
                    for (int a = 0; a < 3; a++) {
                        if (!((mask >> a) & 1)) continue;
                        int q[3] = {i, j, k};
                        q[a]++;
                        const size_t o2 = at(q[0], q[1], q[2]);
                        const double t = tsdf_edge_t(D[o], W[o], D[o2], W[o2]);
                        double X[3] = {tsdf_coord(origin[0], i, voxel), tsdf_coord(origin[1], j, voxel),
                                       tsdf_coord(origin[2], k, voxel)};
                        const int ia = a == 0 ? i : (a == 1 ? j : k);
                        X[a] = origin[a] + ((double)ia + t) * voxel;
                        for (int c = 0; c < 3; c++) {
                            vertices[(size_t)base * 3 + c] = X[c];
                            const int32_t* S = volume + (3 + c) * nn;
                            colors[(size_t)base * 3 + c] =
                                tsdf_mix_color(tsdf_node_color(S[o], CW[o]), tsdf_node_color(S[o2], CW[o2]), t);
                        }
                        base++;
                    }
                }
            }
    });
    parallel_slices(nz - 1, [&](int k0, int k1) {
        for (int k = k0; k < k1; k++)
            for (int j = 0; j < ny - 1; j++) {
                int64_t fb = row_f[(size_t)k * ny + j];
                for (int i = 0; i < nx - 1; i++) {
                    const int nf = (info[at(i, j, k)] >> kTsdfFaceShift) & 7;
                    if (!nf) continue;
                    int cs = 0;
                    for (int c = 0; c < 8; c++)
                        if (info[at(i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2))] & kTsdfInside) cs |= 1 << c;
                    for (int e3 = 0; e3 < 3 * nf; e3++) {
                        const int e = kTsdfTriEdges[cs][e3], c = tsdf_edge_owner(e), a = e >> 2;
                        const size_t oo = at(i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2));
                        faces[(size_t)fb * 3 + e3] = vbase[oo] + tsdf_popc3(info[oo] & ((1 << a) - 1));
                    }
                    fb += nf;
                }
            }
    });
    return SLAM_OK;
}

// Scene post-processing on gfx950: the reference's clusterizePoints
// (src/vizualization/delauney-triangulation/geomAdditionalFunc.cpp:105-163),
// getBestFittingPlaneByPoints (bestFittingPlane.cpp:11-40) and the per-point
// projection of makeMesh (bestFittingPlane.cpp:51-63 with projectPointOnPlane,
// geomAdditionalFunc.cpp:20-32).
//
// Clustering.  The reference fills a dense N x N float matrix with the edge
// predicate and recurses a DFS through it.  Here the predicate is evaluated
// once per unordered pair over upper-triangle pairs of 256-point tiles and the
// components come from a lock-free union-find, so device memory is O(N).
//
//   predicate (bit for bit the reference's, :16-18 and :119-128):
//     d    = p_i - p_j               per component in f32 (Point3f operator-)
//     s    = dx*dx + dy*dy + dz*dz   in f64, left to right, no FMA
//     real = sqrt(s) * dw            correctly rounded f64 sqrt
//     ci   = sum (c_i[k] - c_j[k])^2 exact integer (cv::norm(Vec3b, Vec3b), NORM_L2)
//     col  = sqrt((double)ci) * cw
//     edge iff real + col < max
//   d only changes sign when i and j swap, so the predicate is symmetric and
//   the pair is evaluated once.  NaN compares false: a NaN point is a singleton.
//
//   union-find over parent[N] (int32; the label array itself) with the
//   invariant parent[x] <= x, kept by every write:
//     - init           parent[x] = x;
//     - path halving   atomicMin(parent[x], grandparent): only lowers it;
//     - hook           atomicCAS(parent[a], a, b) with a a root and b < a.
//   A parent therefore only ever decreases.  Every find walks strictly
//   downwards in index, so it ends; a failed CAS retries from a strictly smaller
//   root, so a union ends; and a cycle would need an upward link, which no
//   write creates.  Each stored parent is a member of x's component (it is or
//   was an ancestor), so a stale read still names the right component, and the
//   hook always puts the larger root under the smaller: the root of a tree is
//   its smallest index.  The flatten pass (a launch of its own, after every
//   union is visible) writes label[i] = root(i) = the smallest index of i's
//   component, whatever the scheduling was.  Every access to parent[] inside
//   the pair kernel is an agent-scope atomic (workgroups on other XCDs update
//   it concurrently); no float atomics anywhere.
//
// Plane.  One reduction kernel (plane_reduce) run twice -- sums about zero for
// the centroid, then about the f64 centroid for the six second moments --
// with per-workgroup f64 slots added in index order by plane_sum_slots: no
// atomics, so two runs agree bit for bit.  The 3 x 3 eigenproblem is solved on
// the host (jacobi.h).
#include <cfloat>
#include <cmath>
#include <cstring>

#include "jacobi.h"
#include "slamhip_internal.h"

namespace slamhip {

namespace {

constexpr int kTile = 256;            // points per tile = threads per workgroup (tests/test_scene_gpu.py: T)
constexpr int kPlaneBlocks = 512;     // upper bound of plane_reduce's grid (a fixed function of n)
constexpr int kPlaneSums = 9;         // sum(d) x 3, then xx xy xz yy yz zz of d = p - centre

struct ClusterParams {
    double max, dw, cw;
    // Conservative rejects (cluster_rejects): s >= s_cut, or the f32 sum
    // s32 > t32, proves "no edge".  NaN / +inf disable them.
    double s_cut;
    float t32;
};

// ---- union-find ----------------------------------------------------------------
__device__ __forceinline__ int uf_load(int* parent, int x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int uf_find(int* parent, int x)
{
    for (;;) {
        const int p = uf_load(parent, x);
        if (p == x) return x;
        const int g = uf_load(parent, p);
        if (g == p) return p;
        atomicMin(parent + x, g);     // path halving; g <= p < x
        x = g;
    }
}

// a, b: roots as last seen.  Returns the root of the merged tree.
__device__ __forceinline__ int uf_union(int* parent, int a, int b)
{
    for (;;) {
        if (a == b) return a;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(parent + a, a, b);   // hook the larger root under the smaller
        if (old == a) return b;
        a = uf_find(parent, old);                      // a was hooked meanwhile: old < a
        b = uf_find(parent, b);
    }
}

__global__ __launch_bounds__(256) void cluster_init(int* parent, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = i;
}

// One workgroup per tile pair (ti <= tj): thread t holds point ti * 256 + t in
// registers, the j-tile sits in LDS as SoA (x, y, z, packed colour) and every
// lane of a wave reads the same j (an LDS broadcast).
__global__ __launch_bounds__(kTile) void cluster_pairs(const float* __restrict__ pts,
                                                       const uint8_t* __restrict__ colors, int n, ClusterParams p,
                                                       int* parent, unsigned long long* stats)
{
    __shared__ float sx[kTile], sy[kTile], sz[kTile];
    __shared__ uint32_t sc[kTile];
    __shared__ int shint[kTile];      // a member of j's component (its parent when staged, later a root)
    __shared__ unsigned s_exact;

    // blockIdx.x = tj (tj + 1) / 2 + ti with ti <= tj
    const long long b = blockIdx.x;
    long long tj = (long long)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while (tj * (tj + 1) / 2 > b) tj--;
    while ((tj + 1) * (tj + 2) / 2 <= b) tj++;
    const int ti = (int)(b - tj * (tj + 1) / 2);
    const int tid = threadIdx.x;
    const int i = ti * kTile + tid;
    const int j0 = (int)tj * kTile;
    const int jn = min(kTile, n - j0);
    const bool vi = i < n;

    float xi = 0.f, yi = 0.f, zi = 0.f;
    int bi = 0, gi = 0, ri_c = 0;
    if (vi) {
        xi = pts[3 * (size_t)i]; yi = pts[3 * (size_t)i + 1]; zi = pts[3 * (size_t)i + 2];
        bi = colors[3 * (size_t)i]; gi = colors[3 * (size_t)i + 1]; ri_c = colors[3 * (size_t)i + 2];
    }
    if (tid < jn) {
        const size_t j = (size_t)j0 + tid;
        sx[tid] = pts[3 * j]; sy[tid] = pts[3 * j + 1]; sz[tid] = pts[3 * j + 2];
        sc[tid] = (uint32_t)colors[3 * j] | ((uint32_t)colors[3 * j + 1] << 8) | ((uint32_t)colors[3 * j + 2] << 16);
        shint[tid] = uf_load(parent, (int)j);
    }
    if (tid == 0) s_exact = 0;
    __syncthreads();

    int root = vi ? uf_find(parent, i) : -1;
    unsigned nexact = 0;
    // the diagonal tile pair takes j > i only (j == i is no union)
    const int kbeg = (ti == (int)tj) ? tid + 1 : 0;
    for (int k = 0; k < jn; k++) {
        const float dx = xi - sx[k], dy = yi - sy[k], dz = zi - sz[k];
        const float s32 = dx * dx + dy * dy + dz * dz;
        if (!vi || k < kbeg || s32 > p.t32) continue;      // reject 2 (cluster_rejects)
        nexact++;
        const double ex = (double)dx, ey = (double)dy, ez = (double)dz;
        const double s = ex * ex + ey * ey + ez * ez;
        if (s >= p.s_cut) continue;                        // reject 1 (cluster_rejects)
        const double real = sqrt(s) * p.dw;
        const uint32_t cj = sc[k];
        const int db = bi - (int)(cj & 255u), dg = gi - (int)((cj >> 8) & 255u), dr = ri_c - (int)(cj >> 16);
        const int ci = db * db + dg * dg + dr * dr;
        const double col = sqrt((double)ci) * p.cw;
        if (!(real + col < p.max)) continue;
        // an edge: skip the union when both ends are already known to share a component
        if (shint[k] == root) continue;
        const int rj = uf_find(parent, j0 + k);
        root = uf_find(parent, root);
        if (rj != root) root = uf_union(parent, root, rj);
        shint[k] = root;                                   // a hint only: any member of the component serves
    }
    if (nexact) atomicAdd(&s_exact, nexact);
    __syncthreads();
    if (tid == 0 && s_exact) atomicAdd(stats, (unsigned long long)s_exact);
}

__global__ __launch_bounds__(256) void cluster_flatten(int* parent, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int x = i;
    for (;;) {
        const int q = uf_load(parent, x);
        if (q == x) break;
        x = q;
    }
    // the root's own slot never changes here, and any value written is the
    // reader's root as well, so concurrent walks through slot i stay correct
    __hip_atomic_store(parent + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// real(s) = fl(fl(sqrt(s)) * dw), the reference's realDistance as a function of s
double real_of(double s, double dw) { return sqrt(s) * dw; }

// The two rejects, valid when dw >= 0 and cw >= 0 (otherwise both are disabled).
//
// Reject 1 (exact on the f64 s).  col = fl(fl(sqrt(ci)) * cw) >= 0, and
// rounding is monotone, so fl(real + col) >= real: an edge needs real < max.
// sqrt is correctly rounded, hence monotone, and so is the product with
// dw >= 0, so real(s) is non-decreasing in s and { s : real(s) < max } is a
// down-set.  s_cut is the smallest f64 >= 0 with !(real(s_cut) < max), found by
// bisection over the bit patterns with the host's correctly rounded sqrt (the
// same function the kernel evaluates): s >= s_cut implies no edge, and a NaN s
// fails the comparison and goes on to the exact predicate (which it fails).
//
// Reject 2 (f32, ahead of any f64 work).  The squares of f32 values are exact
// in f64, so s = S (1 + e1)(1 + e2), |e| <= 2^-53, with S the exact sum.  The
// f32 sum s32 carries three roundings: s32 <= S (1 + 2^-24)^3 plus at most
// 2^-147 from products that fall in the subnormal range.  With
// t32 >= max(s_cut (1 + 2^-21), 2^-100), s32 > t32 gives
//   S >= (s32 - 2^-147) (1 + 2^-24)^-3 > s32 (1 - 2^-22),
//   s >= S (1 - 2^-53)^2 > s_cut (1 + 2^-21)(1 - 2^-22)(1 - 2^-52) > s_cut,
// which is reject 1.  An s32 that overflowed to +inf means S (1 + 2^-24)^3 >=
// FLT_MAX >= t32, the same chain.  t32 is rounded up to f32; if it does not
// fit, it is +inf and rejects nothing.  A NaN s32 fails the comparison.
void cluster_rejects(ClusterParams& p)
{
    p.s_cut = NAN;
    p.t32 = INFINITY;
    if (!(p.dw >= 0.0) || !(p.cw >= 0.0)) return;
    uint64_t lo = 0, hi = 0x7FF0000000000000ull;   // +0 .. +inf; !(real(+inf) < max) always holds
    auto no_edge = [&](uint64_t bits) {
        double s;
        memcpy(&s, &bits, 8);
        return !(real_of(s, p.dw) < p.max);
    };
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (no_edge(mid)) hi = mid; else lo = mid + 1;
    }
    memcpy(&p.s_cut, &lo, 8);
    double t = p.s_cut * (1.0 + ldexp(1.0, -21));
    if (t < ldexp(1.0, -100)) t = ldexp(1.0, -100);
    if (t <= (double)FLT_MAX) {
        float f = (float)t;
        if ((double)f < t) f = nextafterf(f, INFINITY);
        p.t32 = f;
    }
}

// ---- plane ---------------------------------------------------------------------
// slot[blockIdx.x][0..8] = sums over this workgroup's points of d = p - centre
// (f32 point widened to f64 first) and of d's six products.  The grid, the
// strided assignment and the LDS tree are fixed functions of n.
__global__ __launch_bounds__(256) void plane_reduce(const float* __restrict__ pts, int n,
                                                    const double* __restrict__ centre, double* slots)
{
    __shared__ double red[256];
    double c0 = 0, c1 = 0, c2 = 0;
    if (centre) { c0 = centre[0]; c1 = centre[1]; c2 = centre[2]; }
    double acc[kPlaneSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) {
        const double x = (double)pts[3 * i] - c0, y = (double)pts[3 * i + 1] - c1, z = (double)pts[3 * i + 2] - c2;
        acc[0] += x; acc[1] += y; acc[2] += z;
        acc[3] += x * x; acc[4] += x * y; acc[5] += x * z;
        acc[6] += y * y; acc[7] += y * z; acc[8] += z * z;
    }
    for (int q = 0; q < kPlaneSums; q++) {
        red[threadIdx.x] = acc[q];
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) slots[(size_t)blockIdx.x * kPlaneSums + q] = red[0];
        __syncthreads();
    }
}

// out[q] = slots added in index order; mean (nullable) = out[0..2] / n
__global__ void plane_sum_slots(const double* slots, int nslots, int n, double* out, double* mean)
{
    const int q = threadIdx.x;
    if (q >= kPlaneSums) return;
    double s = 0;
    for (int b = 0; b < nslots; b++) s += slots[(size_t)b * kPlaneSums + q];
    out[q] = s;
    if (mean && q < 3) mean[q] = s / (double)n;
}

struct ProjectParams {
    float cx, cy, cz;
    double n0, n1, n2;
};

// projectPointOnPlane + makeMesh:56-63 for one point, the reference's mix of
// f32 fields and f64 arithmetic (no contraction)
__global__ __launch_bounds__(256) void plane_project(const float* __restrict__ pts, int n, ProjectParams p,
                                                     float* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n) return;
    const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    const double num = (double)(px - p.cx) * p.n0 + (double)(py - p.cy) * p.n1 + (double)(pz - p.cz) * p.n2;
    const double den = p.n0 * p.n0 + p.n1 * p.n1 + p.n2 * p.n2;
    const double x = num / den;
    float qx = (float)((double)px - p.n0 * x);      // projectedPoint.x = point.x - normal[0] * x
    float qy = (float)((double)py - p.n1 * x);
    float qz = (float)((double)pz - p.n2 * x);
    qx = qx - p.cx; qy = qy - p.cy; qz = qz - p.cz;   // projectedPoint - centroid (Point3f)
    const double ax = (double)qx, ay = (double)qy, az = (double)qz;
    const double coef = sqrt(ay * ay / (ax * ax + az * az) + 1.0);
    out[2 * i] = (float)(ax * coef);                // Point3f * double: saturate_cast<float>
    out[2 * i + 1] = (float)(az * coef);
}

// cluster workspace: the pair counters {exact-path pairs} first (slam_cluster_last_stats reads them at the
// buffer's start), then the plane fit's block slots and its results (sum 9, moments 9, mean 3)
struct ClusterWs {
    DevLayout lay;
    Slot<unsigned long long> stats = lay.add<unsigned long long>(2);
    Slot<double> slots = lay.add<double>((size_t)kPlaneBlocks * kPlaneSums);
    Slot<double> res = lay.add<double>(2 * kPlaneSums + 3);
};

int cluster_dev(slam_ctx* c, hipStream_t s, const float* d_pts, const uint8_t* d_colors, int n, float max_distance,
                float euclid_weight, float color_weight, int32_t* d_labels)
{
    const long long nt = ((long long)n + kTile - 1) / kTile;
    const long long npairs = nt * (nt + 1) / 2;
    if (npairs > 0x7FFFFFFFll)
        return set_err(c, SLAM_E_UNSUPPORTED, "slam_cluster_points: more tile pairs than one grid holds (n > ~16.7M)");
    ClusterParams p;
    p.max = (double)max_distance;       // getValue<float> assigned to double
    p.dw = (double)euclid_weight;
    p.cw = (double)color_weight;
    cluster_rejects(p);
    const ClusterWs L;
    DevMem ws;
    SLAM_HIP(c, ws.bind(c->cluster, L.lay));
    unsigned long long* stats = ws.ptr(L.stats);
    SLAM_HIP(c, hipMemsetAsync(stats, 0, L.stats.bytes(), s));
    const int nb = (n + 255) / 256;
    hipLaunchKernelGGL(cluster_init, dim3(nb), dim3(256), 0, s, d_labels, n);
    hipLaunchKernelGGL(cluster_pairs, dim3((unsigned)npairs), dim3(kTile), 0, s, d_pts, d_colors, n, p, d_labels, stats);
    hipLaunchKernelGGL(cluster_flatten, dim3(nb), dim3(256), 0, s, d_labels, n);
    SLAM_HIP(c, hipGetLastError());
    c->cluster_pairs_total = (unsigned long long)n * (unsigned long long)(n - 1) / 2;
    c->cluster_stats_stream = s;
    return SLAM_OK;
}

// device part of the plane fit: sum[3] (about zero) and mom[6] about the f64 mean
int plane_moments(slam_ctx* c, const float* pts, int n, double* sum, double* mean, double* mom)
{
    hipStream_t s = c->stream;
    const ClusterWs L;
    DevLayout lin;
    const auto s_pts = lin.add<float>((size_t)n * 3);
    DevMem ws, in;
    SLAM_HIP(c, ws.bind(c->cluster, L.lay));
    SLAM_HIP(c, in.bind(c->geom, lin));
    float* d_pts = in.ptr(s_pts);
    double *slots = ws.ptr(L.slots), *d_sum = ws.ptr(L.res), *d_mom = d_sum + kPlaneSums, *d_mean = d_mom + kPlaneSums;
    SLAM_HIP(c, in.upload(s_pts, pts, s));
    const int nb = std::min(kPlaneBlocks, (n + 255) / 256);
    hipLaunchKernelGGL(plane_reduce, dim3(nb), dim3(256), 0, s, d_pts, n, (const double*)nullptr, slots);
    hipLaunchKernelGGL(plane_sum_slots, dim3(1), dim3(64), 0, s, slots, nb, n, d_sum, d_mean);
    hipLaunchKernelGGL(plane_reduce, dim3(nb), dim3(256), 0, s, d_pts, n, (const double*)d_mean, slots);
    hipLaunchKernelGGL(plane_sum_slots, dim3(1), dim3(64), 0, s, slots, nb, n, d_mom, (double*)nullptr);
    SLAM_HIP(c, hipGetLastError());
    double h[2 * kPlaneSums + 3];
    SLAM_HIP(c, ws.download(h, L.res, s));
    SLAM_HIP(c, hipStreamSynchronize(s));
    for (int k = 0; k < 3; k++) { sum[k] = h[k]; mean[k] = h[2 * kPlaneSums + k]; }
    for (int k = 0; k < 6; k++) mom[k] = h[kPlaneSums + 3 + k];
    return SLAM_OK;
}

}  // namespace

}  // namespace slamhip

using namespace slamhip;

extern "C" {

int slam_cluster_points_dev(slam_ctx* c, void* stream, const float* d_pts, const uint8_t* d_colors, int n,
                            float max_distance, float euclid_weight, float color_weight, int32_t* d_labels)
{
    if (!c || n < 0 || (n > 0 && (!d_pts || !d_colors || !d_labels))) return SLAM_E_INVALID_ARG;
    if (n == 0) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    return cluster_dev(c, s, d_pts, d_colors, n, max_distance, euclid_weight, color_weight, d_labels);
}

int slam_cluster_points(slam_ctx* c, const float* pts, const uint8_t* colors, int n, float max_distance,
                        float euclid_weight, float color_weight, int32_t* labels, int* n_components)
{
    if (!c || n < 0 || !n_components || (n > 0 && (!pts || !colors || !labels))) return SLAM_E_INVALID_ARG;
    *n_components = 0;
    if (n == 0) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevLayout lay;
    const auto s_pts = lay.add<float>((size_t)n * 3);
    const auto s_col = lay.add<uint8_t>((size_t)n * 3);
    const auto s_lab = lay.add<int32_t>((size_t)n);
    DevMem d;
    SLAM_HIP(c, d.bind(c->geom, lay));
    SLAM_HIP(c, d.upload(s_pts, pts, s));
    SLAM_HIP(c, d.upload(s_col, colors, s));
    const int rc = cluster_dev(c, s, d.ptr(s_pts), d.ptr(s_col), n, max_distance, euclid_weight, color_weight, d.ptr(s_lab));
    if (rc != SLAM_OK) return rc;
    SLAM_HIP(c, d.download(labels, s_lab, s));
    SLAM_HIP(c, hipStreamSynchronize(s));
    int comps = 0;
    for (int i = 0; i < n; i++) comps += labels[i] == i;
    *n_components = comps;
    return SLAM_OK;
}

int slam_cluster_last_stats(slam_ctx* c, uint64_t* pairs, uint64_t* exact_pairs)
{
    if (!c || !pairs || !exact_pairs) return SLAM_E_INVALID_ARG;
    *pairs = *exact_pairs = 0;
    if (!c->cluster.p || !c->cluster_pairs_total) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    unsigned long long h = 0;
    SLAM_HIP(c, hipMemcpyAsync(&h, c->cluster.p, sizeof(h), hipMemcpyDeviceToHost, c->cluster_stats_stream));
    SLAM_HIP(c, hipStreamSynchronize(c->cluster_stats_stream));
    *pairs = c->cluster_pairs_total;
    *exact_pairs = h;
    return SLAM_OK;
}

int slam_plane_moments(slam_ctx* c, const float* pts, int n, double* sum, double* mean, double* moments)
{
    if (!c || !pts || n < 1 || !sum || !mean || !moments) return SLAM_E_INVALID_ARG;
    SLAM_HIP(c, hipSetDevice(c->device));
    return plane_moments(c, pts, n, sum, mean, moments);
}

int slam_fit_plane(slam_ctx* c, const float* pts, int n, float* centroid, double* normal)
{
    if (!c || !pts || n < 1 || !centroid || !normal) return SLAM_E_INVALID_ARG;
    SLAM_HIP(c, hipSetDevice(c->device));
    double sum[3], mean[3], m[6];
    const int rc = plane_moments(c, pts, n, sum, mean, m);
    if (rc != SLAM_OK) return rc;
    for (int k = 0; k < 3; k++) centroid[k] = (float)mean[k];   // Point3f(mean(row)[0], ...)
    // symmetric positive semi-definite: its SVD is its eigen-decomposition, and
    // jsvd sorts descending, so row 2 of Vt belongs to the smallest eigenvalue
    double At[9] = {m[0], m[1], m[2], m[1], m[3], m[4], m[2], m[4], m[5]}, W[3], Vt[9];
    jsvd<3, 3>(At, W, Vt);
    double v[3] = {Vt[6], Vt[7], Vt[8]};
    const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    int big = 0;
    for (int k = 1; k < 3; k++)
        if (fabs(v[k]) > fabs(v[big])) big = k;
    const double sgn = v[big] < 0 ? -1.0 : 1.0;
    for (int k = 0; k < 3; k++) normal[k] = sgn * v[k] / len;
    return SLAM_OK;
}

int slam_project_to_plane(slam_ctx* c, const float* pts, int n, const float* centroid, const double* normal,
                          float* out_xy)
{
    if (!c || n < 0 || !centroid || !normal || (n > 0 && (!pts || !out_xy))) return SLAM_E_INVALID_ARG;
    if (n == 0) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevLayout lay;
    const auto s_pts = lay.add<float>((size_t)n * 3), s_out = lay.add<float>((size_t)n * 2);
    DevMem d;
    SLAM_HIP(c, d.bind(c->geom, lay));
    SLAM_HIP(c, d.upload(s_pts, pts, s));
    ProjectParams p{centroid[0], centroid[1], centroid[2], normal[0], normal[1], normal[2]};
    hipLaunchKernelGGL(plane_project, dim3((n + 255) / 256), dim3(256), 0, s, d.ptr(s_pts), n, p, d.ptr(s_out));
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, d.download(out_xy, s_out, s));
    SLAM_HIP(c, hipStreamSynchronize(s));
    return SLAM_OK;
}

}  // extern "C"

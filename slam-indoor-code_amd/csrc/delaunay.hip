// The Delaunay step of the meshing stage on gfx950: the reference's
// builtInTriangulation (src/vizualization/delauney-triangulation/bowyerWatson.cpp:86-105,
// cv::Subdiv2D insert + getTriangleList) and makeMesh's corner lookup
// (bestFittingPlane.cpp:67-95), as the exact, deterministic triangulation of
// DESIGN.md section 11.
//
// Contract.  Point i is a vertex iff no j < i has the same coordinates (float
// ==).  The triangles are the Delaunay triangulation of the vertices, complete
// up to the convex hull, decided by the exact signs of exact_pred.h.  A maximal
// set of >= 4 cocircular vertices on an empty circle is fanned from its
// lowest-indexed vertex.  Each triangle is (i, j, k), i its smallest index,
// counter-clockwise; the list is sorted lexicographically.
//
// Algorithm.  No shared frontier, no edge hash, no rounds: one wave64 per
// vertex a builds a's own star.
//   seed   b0 = the nearest other vertex (exact comparison, ties to the lower
//          index).  The closed disc on the diameter a b0 holds no other vertex,
//          so the edge is in every Delaunay triangulation.
//   walk   b_(i+1) = apex(a, b_i) counter-clockwise until it returns to b0 or
//          finds nothing (the hull); then clockwise from b0 with apex(c_i, a).
//   apex(a, b)  candidates are the vertices strictly left of a -> b.  Each
//          lane strides over the points and keeps its best c, replaced by p when
//          incircle(a, b, c, p) > 0; "p strictly inside the circle of c" is a
//          strict weak order on the candidates (circles through a and b are
//          ordered by how far they reach to the left), so the running best and
//          the cross-lane butterfly with the same comparator find a minimal
//          class whatever the order.  A flag records any exact zero met on the
//          way.  A member of the minimal class T never loses a comparison, so
//          the result of any part of the reduction that saw one is a member of
//          T; two members therefore meet, in a lane or in the butterfly, as a
//          zero: the flag is set whenever T has more than one member.  It can
//          also be set by a zero between two points that both lost, which
//          costs a pass and changes nothing: the second scan collects T itself
//          (possibly just the winner) and applies the tie rule:
//            m = min(T + {a, b});  m in T: the apex is m;
//            m == a: the t in T with every other member strictly left of b -> t;
//            m == b: the t in T with every other member strictly left of t -> a.
//          (T lies on one arc from b to a, so both are total orders.)
//   emit   triangle (a, b_i, b_(i+1)) only by the wave whose a is its smallest
//          index: each triangle is written once, through one atomic counter,
//          and a bitonic sort brings the list to the canonical order.
// Every walk loop is bounded by n, there is no workgroup barrier in the star
// kernel (waves take different numbers of steps), and every index that reaches
// memory is below n (points) or below the scratch capacity (triangles).
//
// The coordinates are read as float2 straight from global memory: 8 B per
// point, lane-strided loads coalesce and a component sits in L2.
#include <climits>
#include <cstring>

#include "exact_pred.h"
#include "slamhip_internal.h"

namespace slamhip {

namespace {

constexpr float kSubdivRange = 100000.f;      // Subdiv2D(Rect(-100000, -100000, 200000, 200000))
constexpr int kWavesPerBlock = 4;
struct DelaunayHdr {
    unsigned long long pred, exact, ties;     // predicates evaluated, of those on the exact path, tie passes
    int bad;                                  // a non-finite or out-of-range coordinate was seen
    int count;                                // triangles emitted
};

struct Tri { int32_t i, j, k; };

struct Ctr { unsigned long long pred = 0, exact = 0; };

// the exact paths stay out of line: they are rare and carry a private array
__device__ __noinline__ int orient_slow(float2 a, float2 b, float2 c)
{
    return exact_pred::orient2d_exact(a.x, a.y, b.x, b.y, c.x, c.y);
}
__device__ __noinline__ int incircle_slow(float2 a, float2 b, float2 c, float2 d)
{
    return exact_pred::incircle_exact(a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y);
}
__device__ __noinline__ int closer_slow(float2 a, float2 p, float2 q)
{
    return exact_pred::closer_exact(a.x, a.y, p.x, p.y, q.x, q.y);
}

__device__ __forceinline__ int orient(float2 a, float2 b, float2 c, Ctr& k)
{
    k.pred++;
    int s = exact_pred::orient2d_filter(a.x, a.y, b.x, b.y, c.x, c.y);
    if (s == exact_pred::kPredUndecided) { k.exact++; s = orient_slow(a, b, c); }
    return s;
}
__device__ __forceinline__ int incircle(float2 a, float2 b, float2 c, float2 d, Ctr& k)
{
    k.pred++;
    int s = exact_pred::incircle_filter(a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y);
    if (s == exact_pred::kPredUndecided) { k.exact++; s = incircle_slow(a, b, c, d); }
    return s;
}
__device__ __forceinline__ int closer(float2 a, float2 p, float2 q, Ctr& k)
{
    k.pred++;
    int s = exact_pred::closer_filter(a.x, a.y, p.x, p.y, q.x, q.y);
    if (s == exact_pred::kPredUndecided) { k.exact++; s = closer_slow(a, p, q); }
    return s;
}

__device__ __forceinline__ float2 shfl_xor2(float2 v, int off)
{
    return make_float2(__shfl_xor(v.x, off, 64), __shfl_xor(v.y, off, 64));
}

// dup[i] = some j < i has the same coordinates; hdr->bad on a coordinate that is
// not finite or outside [-range, range).  Tiled like cluster_pairs: workgroup b
// holds points b * 256 + t in registers and walks the tiles 0 .. b through LDS
// (the trip count depends on blockIdx only, so the barriers match).
__global__ __launch_bounds__(256) void delaunay_prepass(const float2* __restrict__ xy, int n, uint8_t* __restrict__ dup,
                                                        DelaunayHdr* hdr)
{
    __shared__ float2 tile[256];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * 256 + tid;
    float2 p = make_float2(0.f, 0.f);
    if (i < n) {
        p = xy[i];
        const bool ok = p.x >= -kSubdivRange && p.x < kSubdivRange && p.y >= -kSubdivRange && p.y < kSubdivRange;
        if (!ok) atomicOr(&hdr->bad, 1);
    }
    bool d = false;
    for (int t = 0; t <= (int)blockIdx.x; t++) {
        const int j = t * 256 + tid;
        __syncthreads();
        if (j < n) tile[tid] = xy[j];
        __syncthreads();
        const int jn = min(256, min(n, i) - t * 256);      // only j < i
        for (int q = 0; q < jn; q++) d |= (tile[q].x == p.x) & (tile[q].y == p.y);
    }
    if (i < n) dup[i] = d ? 1 : 0;
}

// apex of the directed edge (a, b) over the vertices, or -1.  Wave-uniform result.
__device__ int apex(const float2* __restrict__ xy, const uint8_t* __restrict__ dup, int n, int a, float2 pa, int b,
                    float2 pb, int lane, Ctr& k, unsigned long long& ties)
{
    int best = -1, flag = 0;
    float2 pbest = make_float2(0.f, 0.f);
    for (int p = lane; p < n; p += 64) {
        if (dup[p]) continue;
        const float2 pp = xy[p];
        if (orient(pa, pb, pp, k) <= 0) continue;           // a, b and everything not strictly left
        if (best < 0) { best = p; pbest = pp; continue; }
        const int s = incircle(pa, pb, pbest, pp, k);
        if (s > 0) { best = p; pbest = pp; }
        else if (s == 0) flag = 1;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int ob = __shfl_xor(best, off, 64);
        const float2 po = shfl_xor2(pbest, off);
        flag |= __shfl_xor(flag, off, 64);
        if (ob < 0) continue;
        if (best < 0) { best = ob; pbest = po; continue; }
        const int s = incircle(pa, pb, pbest, po, k);
        if (s > 0) { best = ob; pbest = po; }
        else if (s == 0) flag = 1;
    }
    const int c = __shfl(best, 0, 64);
    if (c < 0 || !__shfl(flag, 0, 64)) return c;

    // the tie rule over T = { p strictly left : incircle(a, b, c, p) == 0 } (c included; T = {c}: c again)
    if (lane == 0) ties++;
    const float2 pc = xy[c];
    int tmin = INT_MAX, t1 = -1, t2 = -1;                   // min index; first after b; last before a
    float2 p1 = make_float2(0.f, 0.f), p2 = p1;
    for (int p = lane; p < n; p += 64) {
        if (dup[p]) continue;
        const float2 pp = xy[p];
        if (orient(pa, pb, pp, k) <= 0) continue;
        if (p != c && incircle(pa, pb, pc, pp, k) != 0) continue;
        tmin = min(tmin, p);
        if (t1 < 0 || orient(pb, p1, pp, k) < 0) { t1 = p; p1 = pp; }
        if (t2 < 0 || orient(p2, pa, pp, k) < 0) { t2 = p; p2 = pp; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        tmin = min(tmin, __shfl_xor(tmin, off, 64));
        const int o1 = __shfl_xor(t1, off, 64), o2 = __shfl_xor(t2, off, 64);
        const float2 q1 = shfl_xor2(p1, off), q2 = shfl_xor2(p2, off);
        if (o1 >= 0 && (t1 < 0 || orient(pb, p1, q1, k) < 0)) { t1 = o1; p1 = q1; }
        if (o2 >= 0 && (t2 < 0 || orient(p2, pa, q2, k) < 0)) { t2 = o2; p2 = q2; }
    }
    tmin = __shfl(tmin, 0, 64);
    if (tmin < a && tmin < b) return tmin;
    return a < b ? __shfl(t1, 0, 64) : __shfl(t2, 0, 64);
}

__device__ __forceinline__ void emit(Tri* tris, int tri_cap, DelaunayHdr* hdr, int lane, int a, int b, int c)
{
    if (lane != 0 || a > b || a > c) return;
    const int at = atomicAdd(&hdr->count, 1);
    if (at < tri_cap) tris[at] = Tri{a, b, c};
}

// one wave per point a: a's star, walked from its nearest neighbour
__global__ __launch_bounds__(64 * kWavesPerBlock) void delaunay_star(const float2* __restrict__ xy,
                                                                      const uint8_t* __restrict__ dup, int n, Tri* tris,
                                                                      int tri_cap, DelaunayHdr* hdr)
{
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (wave >= n || hdr->bad) return;
    const int a = (int)wave;
    if (dup[a]) return;
    const float2 pa = xy[a];
    Ctr k;
    unsigned long long ties = 0;

    // seed: the nearest other vertex, ties to the lower index
    int b0 = -1;
    float2 p0 = make_float2(0.f, 0.f);
    for (int p = lane; p < n; p += 64) {
        if (p == a || dup[p]) continue;
        const float2 pp = xy[p];
        if (b0 < 0 || closer(pa, pp, p0, k) < 0) { b0 = p; p0 = pp; }      // p ascends: a tie keeps the lower index
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int ob = __shfl_xor(b0, off, 64);
        const float2 po = shfl_xor2(p0, off);
        if (ob < 0) continue;
        if (b0 < 0) { b0 = ob; p0 = po; continue; }
        const int s = closer(pa, po, p0, k);
        if (s < 0 || (s == 0 && ob < b0)) { b0 = ob; p0 = po; }
    }
    b0 = __shfl(b0, 0, 64);

    if (b0 >= 0) {
        p0 = xy[b0];
        int b = b0;
        float2 pb = p0;
        bool closed = false;
        for (int step = 0; step < n; step++) {               // counter-clockwise
            const int c = apex(xy, dup, n, a, pa, b, pb, lane, k, ties);
            if (c < 0) break;
            emit(tris, tri_cap, hdr, lane, a, b, c);
            if (c == b0) { closed = true; break; }
            b = c;
            pb = xy[c];
        }
        if (!closed) {
            b = b0;
            pb = p0;
            for (int step = 0; step < n; step++) {           // clockwise from b0, up to the hull
                const int c = apex(xy, dup, n, b, pb, a, pa, lane, k, ties);
                if (c < 0) break;
                emit(tris, tri_cap, hdr, lane, a, c, b);
                b = c;
                pb = xy[c];
            }
        }
    }

    for (int off = 32; off > 0; off >>= 1) {
        k.pred += __shfl_down(k.pred, off, 64);
        k.exact += __shfl_down(k.exact, off, 64);
    }
    if (lane == 0) {
        atomicAdd(&hdr->pred, k.pred);
        if (k.exact) atomicAdd(&hdr->exact, k.exact);
        if (ties) atomicAdd(&hdr->ties, ties);
    }
}

// ---- canonical order: bitonic sort of the triples, padded to a power of two -------
__device__ __forceinline__ bool tri_less(const Tri& x, const Tri& y)
{
    if (x.i != y.i) return x.i < y.i;
    if (x.j != y.j) return x.j < y.j;
    return x.k < y.k;
}

__global__ __launch_bounds__(256) void tri_pad(Tri* t, int count, int padded)
{
    const int i = blockIdx.x * 256 + threadIdx.x + count;
    if (i < padded) t[i] = Tri{INT_MAX, INT_MAX, INT_MAX};
}

// one compare-exchange step: partner = i ^ j, ascending where (i & k) == 0
__global__ __launch_bounds__(256) void tri_bitonic_step(Tri* t, int padded, int k, int j)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int l = i ^ j;
    if (i >= padded || l <= i) return;
    const Tri x = t[i], y = t[l];
    const bool up = (i & k) == 0;
    if (tri_less(y, x) == up) { t[i] = y; t[l] = x; }
}

// all steps with j < 256 of one k inside a 256-triple tile held in LDS
__global__ __launch_bounds__(256) void tri_bitonic_tile(Tri* t, int padded, int k, int jstart)
{
    __shared__ Tri tile[256];
    const int i = blockIdx.x * 256 + threadIdx.x;        // padded is a multiple of 256 here
    tile[threadIdx.x] = t[i];
    __syncthreads();
    for (int j = jstart; j > 0; j >>= 1) {
        const int l = (int)threadIdx.x ^ j;
        if (l > (int)threadIdx.x) {
            const Tri x = tile[threadIdx.x], y = tile[l];
            const bool up = (i & k) == 0;
            if (tri_less(y, x) == up) { tile[threadIdx.x] = y; tile[l] = x; }
        }
        __syncthreads();
    }
    t[i] = tile[threadIdx.x];
}

// one predicate per thread through the wrappers apex uses (slam_delaunay_predicates):
// kind 'o' orient(v0..5), 'i' incircle(v0..7), 'c' closer(v0..5)
__global__ __launch_bounds__(64) void predicate_cases(const uint8_t* __restrict__ kind, const float* __restrict__ vals,
                                                      int n, int8_t* __restrict__ filter_sign, int8_t* __restrict__ sign)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* v = vals + (size_t)i * 8;
    const float2 a = make_float2(v[0], v[1]), b = make_float2(v[2], v[3]), p = make_float2(v[4], v[5]);
    Ctr k;
    int fs, s;
    if (kind[i] == 'o') {
        fs = exact_pred::orient2d_filter(a.x, a.y, b.x, b.y, p.x, p.y);
        s = orient(a, b, p, k);
    } else if (kind[i] == 'i') {
        const float2 d = make_float2(v[6], v[7]);
        fs = exact_pred::incircle_filter(a.x, a.y, b.x, b.y, p.x, p.y, d.x, d.y);
        s = incircle(a, b, p, d, k);
    } else {
        fs = exact_pred::closer_filter(a.x, a.y, b.x, b.y, p.x, p.y);
        s = closer(a, b, p, k);
    }
    filter_sign[i] = (int8_t)fs;
    sign[i] = (int8_t)s;
}

int next_pow2(long long v)
{
    long long p = 1;
    while (p < v) p <<= 1;
    return (int)p;
}

// Runs the whole step on stream s and waits for it.  *count = the number of
// triangles (also when it exceeds cap); d_n_tris (nullable) receives it too.
int delaunay_run(slam_ctx* c, hipStream_t s, const float* d_xy, int n, int32_t* d_tris, int cap, int32_t* d_n_tris,
                 int* count)
{
    *count = 0;
    if (n > (1 << 29)) return set_err(c, SLAM_E_UNSUPPORTED, "slam_delaunay_2d: n > 2^29");
    const int tri_cap = std::max(256, next_pow2(2ll * n));      // >= 2n - 5, and a whole number of sort tiles
    DevLayout lay;
    const auto s_hdr = lay.add<DelaunayHdr>(1);       // first: slam_delaunay_last_stats reads it at the buffer's start
    const auto s_dup = lay.add<uint8_t>((size_t)n);
    const auto s_tris = lay.add<Tri>((size_t)tri_cap);
    DevMem ws;
    SLAM_HIP(c, ws.bind(c->delaunay, lay));
    DelaunayHdr* hdr = ws.ptr(s_hdr);
    uint8_t* dup = ws.ptr(s_dup);
    Tri* tris = ws.ptr(s_tris);
    const float2* xy = reinterpret_cast<const float2*>(d_xy);

    SLAM_HIP(c, hipMemsetAsync(hdr, 0, sizeof(DelaunayHdr), s));
    hipLaunchKernelGGL(delaunay_prepass, dim3((n + 255) / 256), dim3(256), 0, s, xy, n, dup, hdr);
    hipLaunchKernelGGL(delaunay_star, dim3((n + kWavesPerBlock - 1) / kWavesPerBlock), dim3(64 * kWavesPerBlock), 0, s,
                       xy, dup, n, tris, tri_cap, hdr);
    SLAM_HIP(c, hipGetLastError());
    c->delaunay_ran = true;
    c->delaunay_stats_stream = s;
    DelaunayHdr* h = static_cast<DelaunayHdr*>(readback(c, sizeof(DelaunayHdr)));
    if (!h) return set_err(c, SLAM_E_HIP, "slam_delaunay_2d: no pinned readback space");
    SLAM_HIP(c, hipMemcpyAsync(h, hdr, sizeof(DelaunayHdr), hipMemcpyDeviceToHost, s));
    SLAM_HIP(c, hipStreamSynchronize(s));
    const bool bad = h->bad != 0;
    const int nt = bad ? 0 : h->count;
    if (nt > tri_cap) return set_err(c, SLAM_E_HIP, "slam_delaunay_2d: more triangles than 2n (internal error)");
    if (d_n_tris) {
        if (bad) SLAM_HIP(c, hipMemsetAsync(d_n_tris, 0, sizeof(int32_t), s));
        else SLAM_HIP(c, hipMemcpyAsync(d_n_tris, &hdr->count, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        SLAM_HIP(c, hipStreamSynchronize(s));
    }
    if (bad)
        return set_err(c, SLAM_E_INVALID_ARG,
                       "slam_delaunay_2d: a coordinate is not finite or outside [-100000, 100000): no mesh");
    *count = nt;
    if (nt > cap) return set_err(c, SLAM_E_CAPACITY, "slam_delaunay_2d: tris holds fewer triangles than there are");
    if (nt == 0) return SLAM_OK;

    const int padded = std::max(256, next_pow2(nt));
    if (padded > nt) hipLaunchKernelGGL(tri_pad, dim3((padded - nt + 255) / 256), dim3(256), 0, s, tris, nt, padded);
    const int nb = padded / 256;
    for (int k = 2; k <= padded; k <<= 1) {
        int j = k >> 1;
        for (; j >= 256; j >>= 1) hipLaunchKernelGGL(tri_bitonic_step, dim3(nb), dim3(256), 0, s, tris, padded, k, j);
        hipLaunchKernelGGL(tri_bitonic_tile, dim3(nb), dim3(256), 0, s, tris, padded, k, j);
    }
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipMemcpyAsync(d_tris, tris, (size_t)nt * sizeof(Tri), hipMemcpyDeviceToDevice, s));
    SLAM_HIP(c, hipStreamSynchronize(s));
    return SLAM_OK;
}

}  // namespace

}  // namespace slamhip

using namespace slamhip;

extern "C" {

int slam_delaunay_2d_dev(slam_ctx* c, void* stream, const float* d_xy, int n, int32_t* d_tris, int cap,
                         int32_t* d_n_tris)
{
    if (!c || n < 0 || cap < 0 || !d_n_tris || (n > 0 && !d_xy) || (cap > 0 && !d_tris) ||
        (reinterpret_cast<uintptr_t>(d_xy) & 7))
        return SLAM_E_INVALID_ARG;
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if (n == 0) {
        SLAM_HIP(c, hipMemsetAsync(d_n_tris, 0, sizeof(int32_t), s));
        return SLAM_OK;
    }
    int count = 0;
    return delaunay_run(c, s, d_xy, n, d_tris, cap, d_n_tris, &count);
}

int slam_delaunay_2d(slam_ctx* c, const float* xy, int n, int32_t* tris, int cap, int* n_tris)
{
    if (!c || n < 0 || cap < 0 || !n_tris || (n > 0 && !xy) || (cap > 0 && !tris)) return SLAM_E_INVALID_ARG;
    *n_tris = 0;
    if (n == 0) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t keep = (size_t)std::min<long long>(cap, std::max(256ll, 4ll * n));   // >= the scratch capacity of delaunay_run
    DevLayout lay;
    const auto s_xy = lay.add<float>((size_t)n * 2);
    const auto s_tris = lay.add<int32_t>(keep * 3);
    DevMem d;
    SLAM_HIP(c, d.bind(c->geom, lay));
    SLAM_HIP(c, d.upload(s_xy, xy, s));
    int count = 0;
    const int rc = delaunay_run(c, s, d.ptr(s_xy), n, d.ptr(s_tris), cap, nullptr, &count);
    *n_tris = count;
    if (rc != SLAM_OK) return rc;
    if (count) {
        SLAM_HIP(c, d.download(tris, s_tris, (size_t)count * 3, s));
        SLAM_HIP(c, hipStreamSynchronize(s));
    }
    return SLAM_OK;
}

int slam_delaunay_last_stats(slam_ctx* c, uint64_t* predicates, uint64_t* exact_predicates, uint64_t* tie_passes)
{
    if (!c || !predicates || !exact_predicates || !tie_passes) return SLAM_E_INVALID_ARG;
    *predicates = *exact_predicates = *tie_passes = 0;
    if (!c->delaunay.p || !c->delaunay_ran) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    DelaunayHdr h;
    SLAM_HIP(c, hipMemcpyAsync(&h, c->delaunay.p, sizeof(h), hipMemcpyDeviceToHost, c->delaunay_stats_stream));
    SLAM_HIP(c, hipStreamSynchronize(c->delaunay_stats_stream));
    *predicates = h.pred;
    *exact_predicates = h.exact;
    *tie_passes = h.ties;
    return SLAM_OK;
}

int slam_delaunay_predicates(slam_ctx* c, const uint8_t* kind, const float* vals, int n, int8_t* filter_sign,
                             int8_t* sign)
{
    if (!c || n < 0 || !kind || !vals || !filter_sign || !sign) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < n; i++)
        if (kind[i] != 'o' && kind[i] != 'i' && kind[i] != 'c') return SLAM_E_INVALID_ARG;
    if (n == 0) return SLAM_OK;
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevLayout lay;
    const auto s_vals = lay.add<float>((size_t)n * 8);
    const auto s_kind = lay.add<uint8_t>((size_t)n);
    const auto s_fs = lay.add<int8_t>((size_t)n), s_sign = lay.add<int8_t>((size_t)n);
    DevMem d;
    SLAM_HIP(c, d.bind(c->geom, lay));
    SLAM_HIP(c, d.upload(s_vals, vals, s));
    SLAM_HIP(c, d.upload(s_kind, kind, s));
    hipLaunchKernelGGL(predicate_cases, dim3((n + 63) / 64), dim3(64), 0, s, d.ptr(s_kind), d.ptr(s_vals), n, d.ptr(s_fs),
                       d.ptr(s_sign));
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, d.download(filter_sign, s_fs, s));
    SLAM_HIP(c, d.download(sign, s_sign, s));
    SLAM_HIP(c, hipStreamSynchronize(s));
    return SLAM_OK;
}

}  // extern "C"

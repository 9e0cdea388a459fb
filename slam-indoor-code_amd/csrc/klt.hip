// Pyramidal Lucas-Kanade tracking on the device (DESIGN.md section 15;
// tests/klt_ref.py is the definition of every value computed here):
//
//   klt_gray_pyr   one pyrDown step for a batch of frames (blockIdx.z = frame): the
//                  source tile + 2 px halo (BORDER_REFLECT_101) in LDS, the separable
//                  1 4 6 4 1 as a row pass into LDS and a column pass, (sum + 128) >> 8.
//                  The first step reads the BGR / gray frame itself: BGR -> gray is
//                  fused into the tile load and the tile's interior is level 0.
//   klt_scharr     calcScharrDeriv of every level of one frame's pyramid (blockIdx.z
//                  = level): int16 {Ix, Iy} interleaved.  Only the previous frame has
//                  derivative planes; candidates carry gray pyramids only.
//   klt_track      LKTrackerInvoker, one wave64 per (candidate frame, point), the whole
//                  level loop inside.  Per level the wave stages the point's {I, Ix,
//                  Iy} patch as int16 in LDS (lane l owns window pixels l, l + 64, ...),
//                  then every iteration its lanes sample J for their pixels and the
//                  int64 partial sums meet in an xor butterfly, so every lane holds
//                  the same exact sums and takes the same branches.  A lane reads
//                  back only the patch entries it wrote: no barrier anywhere, and
//                  waves of different iteration counts never wait for each other.
//                  J is read through L2 (a candidate's pyramid is 2.8 MB at 1080p and
//                  its points run together); a lane issues the loads of four of its
//                  pixels before it uses the first, and a window that lies inside the
//                  level, which the wave tests once per position, skips the index
//                  reflection (measurements: DESIGN.md section 15).
//
// The five window sums are exact (int64, one conversion to f32): the deviation
// from OpenCV's f32 accumulators that makes the result independent of the
// summation order (include/slamhip.h).  Everything downstream is f32 in the
// source's order; the Makefile's -ffp-contract=off keeps it unfused.
#include "slamhip_internal.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace slamhip {

namespace {

constexpr int kPyrTW = 32, kPyrTH = 16;                       // destination tile of klt_gray_pyr
constexpr int kPyrSW = 2 * kPyrTW + 3, kPyrSH = 2 * kPyrTH + 3;   // source tile: 67 x 35
constexpr int kPyrThreads = 256;
constexpr int W_BITS = 14;

__device__ __forceinline__ uint32_t gray_at(const uint8_t* p, int channels)
{
    if (channels == 1) return p[0];
    return ((uint32_t)p[0] * 1868u + (uint32_t)p[1] * 9617u + (uint32_t)p[2] * 4899u + (1u << 13)) >> 14;
}

// BORDER_REFLECT_101 of any i into 0 .. n - 1 (period 2 (n - 1))
__device__ __forceinline__ int reflect101(int i, int n)
{
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

struct PyrParams {
    const uint8_t* img;        // first step: the frames (frame f at img + f * frame_stride)
    size_t frame_stride, row_stride;
    int channels, first;
    uint8_t* pyr;              // frame f's levels at pyr + f * pyr_stride
    size_t pyr_stride;
    uint32_t src_off, dst_off; // level offsets in a frame's pyramid
    int sw, sh, dw, dh;        // dw == 0: no destination level (a one-level pyramid's first step)
};

__global__ __launch_bounds__(kPyrThreads) void klt_gray_pyr(PyrParams p)
{
    __shared__ uint8_t src[kPyrSH][kPyrSW + 1];
    __shared__ uint16_t hrow[kPyrSH][kPyrTW];
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * kPyrTW, Y0 = blockIdx.y * kPyrTH;
    uint8_t* pyr = p.pyr + blockIdx.z * p.pyr_stride;
    const uint8_t* img = p.first ? p.img + blockIdx.z * p.frame_stride : pyr + p.src_off;
    for (int i = tid; i < kPyrSH * kPyrSW; i += kPyrThreads) {
        const int ly = i / kPyrSW, lx = i - ly * kPyrSW;
        const int gx = 2 * X0 - 2 + lx, gy = 2 * Y0 - 2 + ly;
        const int x = reflect101(gx, p.sw), y = reflect101(gy, p.sh);
        uint32_t v;
        if (p.first) {
            v = gray_at(img + (size_t)y * p.row_stride + (size_t)x * p.channels, p.channels);
            // the tile's interior is level 0 (each source pixel belongs to one tile's interior)
            if (lx >= 2 && lx < 2 + 2 * kPyrTW && ly >= 2 && ly < 2 + 2 * kPyrTH && gx < p.sw && gy < p.sh)
                pyr[p.src_off + (size_t)gy * p.sw + gx] = (uint8_t)v;
        } else {
            v = img[(size_t)y * p.sw + x];
        }
        src[ly][lx] = (uint8_t)v;
    }
    if (p.dw == 0) return;
    __syncthreads();
    for (int i = tid; i < kPyrSH * kPyrTW; i += kPyrThreads) {
        const int ly = i / kPyrTW, dx = i - ly * kPyrTW;
        const uint8_t* s = &src[ly][2 * dx];
        hrow[ly][dx] = (uint16_t)(s[0] + 4 * s[1] + 6 * s[2] + 4 * s[3] + s[4]);
    }
    __syncthreads();
    for (int i = tid; i < kPyrTH * kPyrTW; i += kPyrThreads) {
        const int dy = i / kPyrTW, dx = i - dy * kPyrTW;
        const int X = X0 + dx, Y = Y0 + dy;
        if (X >= p.dw || Y >= p.dh) continue;
        const int r = 2 * dy;
        const int sum = hrow[r][dx] + 4 * hrow[r + 1][dx] + 6 * hrow[r + 2][dx] + 4 * hrow[r + 3][dx] + hrow[r + 4][dx];
        pyr[p.dst_off + (size_t)Y * p.dw + X] = (uint8_t)((sum + 128) >> 8);
    }
}

__global__ __launch_bounds__(256) void klt_scharr(const uint8_t* pyr, KltLayout L, short2* deriv)
{
    const int level = blockIdx.z;
    const int w = L.w[level], h = L.h[level];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const uint8_t* g = pyr + L.off[level];
    const uint8_t* r0 = g + (size_t)reflect101(y - 1, h) * w;
    const uint8_t* r1 = g + (size_t)y * w;
    const uint8_t* r2 = g + (size_t)reflect101(y + 1, h) * w;
    const int xl = reflect101(x - 1, w), xr = reflect101(x + 1, w);
    const int t0l = (r0[xl] + r2[xl]) * 3 + r1[xl] * 10, t0r = (r0[xr] + r2[xr]) * 3 + r1[xr] * 10;
    const int t1l = r2[xl] - r0[xl], t1c = r2[x] - r0[x], t1r = r2[xr] - r0[xr];
    deriv[L.off[level] + (size_t)y * w + x] = make_short2((short)(t0r - t0l), (short)((t1r + t1l) * 3 + t1c * 10));
}

struct TrackParams {
    const uint8_t* prev_pyr;   // the previous frame's gray levels
    const short2* deriv;       // ... and derivative planes
    const uint8_t* next_pyr;   // candidate f's gray levels at next_pyr + f * next_stride
    size_t next_stride;
    KltLayout L;
    const float* prev_pts;     // n x 2
    float* next_pts;           // nframes x n x 2 (read with USE_INITIAL_FLOW)
    uint8_t* status;           // nframes x n
    float* err;                // nframes x n
    int32_t* counts;           // nframes, zero at launch: status == 1 per candidate
    int n, win_w, win_h, max_count, flags;
    float min_eig;
    double eps2;
};

__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// exact integer sum -> f32 once: int64 -> f64 is exact below 2^53, f64 -> f32 rounds to nearest even
__device__ __forceinline__ float sum_f32(long long v) { return (float)(double)v; }

struct Weights { int w00, w01, w10, w11; };
__device__ __forceinline__ Weights lk_weights(float a, float b)
{
    Weights w;
    w.w00 = __float2int_rn((1.f - a) * (1.f - b) * (float)(1 << W_BITS));
    w.w01 = __float2int_rn(a * (1.f - b) * (float)(1 << W_BITS));
    w.w10 = __float2int_rn((1.f - a) * b * (float)(1 << W_BITS));
    w.w11 = (1 << W_BITS) - w.w00 - w.w01 - w.w10;
    return w;
}

__device__ __forceinline__ int descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

// the 2 x 2 neighbours of (x, y), intensities reflected; lk_mix: sum iw * src.  Split so that a
// lane's loads of several window pixels are all in flight before the first is used (kUnroll):
// an iteration is a chain of dependent L2 round trips otherwise.
struct Quad { int v00, v01, v10, v11; };
// INNER: the whole window and its right / lower neighbours lie inside the level (the wave
// tests it once per position), so no index is reflected
template <bool INNER>
__device__ __forceinline__ Quad lk_load(const uint8_t* g, int cols, int rows, int x, int y)
{
    Quad q;
    if (INNER) {
        const uint8_t* r = g + (y * cols + x);
        q.v00 = r[0];
        q.v01 = r[1];
        q.v10 = r[cols];
        q.v11 = r[cols + 1];
    } else {
        const int x0 = reflect101(x, cols), x1 = reflect101(x + 1, cols);
        const uint8_t* r0 = g + reflect101(y, rows) * cols;
        const uint8_t* r1 = g + reflect101(y + 1, rows) * cols;
        q.v00 = r0[x0];
        q.v01 = r0[x1];
        q.v10 = r1[x0];
        q.v11 = r1[x1];
    }
    return q;
}
__device__ __forceinline__ int lk_mix(const Quad& q, const Weights& w)
{
    return q.v00 * w.w00 + q.v01 * w.w01 + q.v10 * w.w10 + q.v11 * w.w11;
}
constexpr int kUnroll = 4;      // window pixels per lane whose loads are issued together

template <bool INNER>
__device__ __forceinline__ short2 lk_deriv_at(const short2* d, int cols, int rows, int x, int y)
{
    if (!INNER && ((unsigned)x >= (unsigned)cols || (unsigned)y >= (unsigned)rows)) return make_short2(0, 0);
    return d[y * cols + x];
}

__device__ __forceinline__ bool lk_inner(int ix, int iy, int ww, int wh, int cols, int rows)
{
    return ix >= 0 && iy >= 0 && ix + ww < cols && iy + wh < rows;
}

// One lane's part of a level's patch: {I, Ix, Iy} of its window pixels into LDS and its partial
// sums of Ix^2, Ix Iy, Iy^2 (at most 16 terms below 2^26 each: int32 holds them)
template <bool INNER>
__device__ __forceinline__ void lk_stage(const uint8_t* I, const short2* dI, int cols, int rows, int ix, int iy,
                                         const Weights& wp, int lane, int area, const uint16_t* pxy, short* pI,
                                         short* pIx, short* pIy, int& s11, int& s12, int& s22)
{
    for (int i = lane; i < area; i += 64) {
        const int x = ix + (pxy[i] & 255), y = iy + (pxy[i] >> 8);
        const Quad q = lk_load<INNER>(I, cols, rows, x, y);
        const short2 d00 = lk_deriv_at<INNER>(dI, cols, rows, x, y), d01 = lk_deriv_at<INNER>(dI, cols, rows, x + 1, y);
        const short2 d10 = lk_deriv_at<INNER>(dI, cols, rows, x, y + 1),
                     d11 = lk_deriv_at<INNER>(dI, cols, rows, x + 1, y + 1);
        const int iv = descale(lk_mix(q, wp), W_BITS - 5);
        const int gx = descale(d00.x * wp.w00 + d01.x * wp.w01 + d10.x * wp.w10 + d11.x * wp.w11, W_BITS);
        const int gy = descale(d00.y * wp.w00 + d01.y * wp.w01 + d10.y * wp.w10 + d11.y * wp.w11, W_BITS);
        pI[i] = (short)iv;
        pIx[i] = (short)gx;
        pIy[i] = (short)gy;
        s11 += gx * gx;
        s12 += gx * gy;
        s22 += gy * gy;
    }
}

// One lane's partial sums of diff Ix, diff Iy (ABS: of |diff| in b1) at the window position (jx, jy) of J
template <bool INNER, bool ABS>
__device__ __forceinline__ void lk_mismatch(const uint8_t* J, int cols, int rows, int jx, int jy, const Weights& wn,
                                            int lane, int area, const uint16_t* pxy, const short* pI, const short* pIx,
                                            const short* pIy, int& b1, int& b2)
{
    for (int c = lane; c < area; c += 64 * kUnroll) {
        Quad q[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int i = min(c + 64 * u, area - 1);       // past the window: a pixel of it, not used
            q[u] = lk_load<INNER>(J, cols, rows, jx + (pxy[i] & 255), jy + (pxy[i] >> 8));
        }
#pragma unroll
        for (int u = 0; u < kUnroll; u++) {
            const int i = c + 64 * u;
            if (i < area) {
                const int diff = descale(lk_mix(q[u], wn), W_BITS - 5) - pI[i];
                if (ABS) {
                    b1 += abs(diff);
                } else {
                    b1 += diff * pIx[i];
                    b2 += diff * pIy[i];
                }
            }
        }
    }
}

// the window position's integer corner and the bounds test on the floored floats:
// NaN, infinite and out-of-int-range positions are outside
__device__ __forceinline__ bool lk_corner(float x, float y, int ww, int wh, int cols, int rows, int& ix, int& iy)
{
    const float fx = floorf(x), fy = floorf(y);
    if (!(fx >= (float)-ww && fx < (float)cols && fy >= (float)-wh && fy < (float)rows)) return false;
    ix = (int)fx;
    iy = (int)fy;
    return true;
}

__global__ __launch_bounds__(64) void klt_track(TrackParams p)
{
    // 4 x area int16: the patch {I, Ix, Iy} and (y << 8) | x of window pixel i (sized by the launch:
    // 3.5 KB at 21 x 21, 7.7 KB at 31 x 31, so the usual window does not cap the occupancy)
    extern __shared__ short klt_smem[];
    const int lane = threadIdx.x;
    const int pt = blockIdx.x, f = blockIdx.y;
    const size_t o = (size_t)f * p.n + pt;
    const int ww = p.win_w, wh = p.win_h, area = ww * wh;
    short* pI = klt_smem;
    short* pIx = pI + area;
    short* pIy = pIx + area;
    uint16_t* pxy = reinterpret_cast<uint16_t*>(pIy + area);
    const float hx = (float)(ww - 1) * 0.5f, hy = (float)(wh - 1) * 0.5f;
    const float px = p.prev_pts[2 * (size_t)pt], py = p.prev_pts[2 * (size_t)pt + 1];
    const uint8_t* next_pyr = p.next_pyr + f * p.next_stride;
    const int top = p.L.nlevels - 1;
    // every lane carries the same point and takes the same branches
    float ox = 0.f, oy = 0.f;                // nextPts[ptidx]
    if (p.flags & SLAM_KLT_USE_INITIAL_FLOW) {
        ox = p.next_pts[2 * o];
        oy = p.next_pts[2 * o + 1];
    }
    bool st = true;
    float er = 0.f;
    for (int i = lane; i < area; i += 64) {
        const int y = i / ww;
        pxy[i] = (uint16_t)((y << 8) | (i - y * ww));
    }
    for (int level = top; level >= 0; level--) {
        const int cols = p.L.w[level], rows = p.L.h[level];
        const uint8_t* I = p.prev_pyr + p.L.off[level];
        const short2* dI = p.deriv + p.L.off[level];
        const uint8_t* J = next_pyr + p.L.off[level];
        const float sc = 1.f / (float)(1 << level);            // a power of two: exact
        float ppx = px * sc, ppy = py * sc;
        if (level == top) {
            if (p.flags & SLAM_KLT_USE_INITIAL_FLOW) {
                ox = ox * sc;
                oy = oy * sc;
            } else {
                ox = ppx;
                oy = ppy;
            }
        } else {
            ox = ox * 2.f;
            oy = oy * 2.f;
        }
        ppx -= hx;
        ppy -= hy;
        int ix, iy;
        if (!lk_corner(ppx, ppy, ww, wh, cols, rows, ix, iy)) {
            if (level == 0) {
                st = false;
                er = 0.f;
            }
            continue;
        }
        const Weights wp = lk_weights(ppx - (float)ix, ppy - (float)iy);
        int s11 = 0, s12 = 0, s22 = 0;
        if (lk_inner(ix, iy, ww, wh, cols, rows))
            lk_stage<true>(I, dI, cols, rows, ix, iy, wp, lane, area, pxy, pI, pIx, pIy, s11, s12, s22);
        else
            lk_stage<false>(I, dI, cols, rows, ix, iy, wp, lane, area, pxy, pI, pIx, pIy, s11, s12, s22);
        const float scale = 1.f / (float)(1 << 20);
        const float A11 = sum_f32(wave_sum(s11)) * scale, A12 = sum_f32(wave_sum(s12)) * scale,
                    A22 = sum_f32(wave_sum(s22)) * scale;
        const float D = A11 * A22 - A12 * A12;
        const float min_eig = cr_divf(A22 + A11 - cr_sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12),
                                      (float)(2 * ww * wh));
        if (p.flags & SLAM_KLT_GET_MIN_EIGENVALS) er = min_eig;
        if (min_eig < p.min_eig || D < FLT_EPSILON) {
            if (level == 0) st = false;
            continue;
        }
        const float Dinv = cr_divf(1.f, D);
        float nx = ox - hx, ny = oy - hy;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < p.max_count; j++) {
            int jx, jy;
            if (!lk_corner(nx, ny, ww, wh, cols, rows, jx, jy)) {
                if (level == 0) st = false;
                break;
            }
            const Weights wn = lk_weights(nx - (float)jx, ny - (float)jy);
            int sb1 = 0, sb2 = 0;
            if (lk_inner(jx, jy, ww, wh, cols, rows))
                lk_mismatch<true, false>(J, cols, rows, jx, jy, wn, lane, area, pxy, pI, pIx, pIy, sb1, sb2);
            else
                lk_mismatch<false, false>(J, cols, rows, jx, jy, wn, lane, area, pxy, pI, pIx, pIy, sb1, sb2);
            const float b1 = sum_f32(wave_sum(sb1)) * scale, b2 = sum_f32(wave_sum(sb2)) * scale;
            const float dx = (A12 * b2 - A22 * b1) * Dinv, dy = (A12 * b1 - A11 * b2) * Dinv;
            nx = nx + dx;
            ny = ny + dy;
            ox = nx + hx;
            oy = ny + hy;
            if ((double)dx * (double)dx + (double)dy * (double)dy <= p.eps2) break;
            if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {
                ox = ox - dx * 0.5f;
                oy = oy - dy * 0.5f;
                break;
            }
            pdx = dx;
            pdy = dy;
        }
        if (st && level == 0 && !(p.flags & SLAM_KLT_GET_MIN_EIGENVALS)) {
            const float qx = ox - hx, qy = oy - hy;
            int jx, jy;
            if (!lk_corner(qx, qy, ww, wh, cols, rows, jx, jy)) {
                st = false;
                continue;
            }
            const Weights wn = lk_weights(qx - (float)jx, qy - (float)jy);
            int se = 0, unused = 0;
            if (lk_inner(jx, jy, ww, wh, cols, rows))
                lk_mismatch<true, true>(J, cols, rows, jx, jy, wn, lane, area, pxy, pI, pIx, pIy, se, unused);
            else
                lk_mismatch<false, true>(J, cols, rows, jx, jy, wn, lane, area, pxy, pI, pIx, pIy, se, unused);
            er = cr_divf(sum_f32(wave_sum(se)), (float)(32 * ww * wh));
        }
    }
    if (lane == 0) {
        p.next_pts[2 * o] = ox;
        p.next_pts[2 * o + 1] = oy;
        p.status[o] = st ? 1 : 0;
        p.err[o] = er;
        if (st) atomicAdd(&p.counts[f], 1);
    }
}

}  // namespace

KltLayout klt_layout(int w, int h, int win_w, int win_h, int max_level)
{
    KltLayout L = {};
    uint32_t off = 0;
    for (int l = 0; l <= max_level; l++) {
        L.w[l] = w;
        L.h[l] = h;
        L.off[l] = off;
        off += (uint32_t)w * (uint32_t)h;
        L.nlevels = l + 1;
        w = (w + 1) / 2;
        h = (h + 1) / 2;
        if (w <= win_w || h <= win_h) break;    // buildOpticalFlowPyramid's early return
    }
    L.frame_px = (off + 15u) & ~15u;
    return L;
}

hipError_t launch_klt_pyramid(hipStream_t s, const uint8_t* img, size_t frame_stride, size_t row_stride, int channels,
                              int nframes, const KltLayout& L, uint8_t* pyr)
{
    for (int l = 0; l < std::max(L.nlevels - 1, 1); l++) {
        PyrParams p;
        p.img = img;
        p.frame_stride = frame_stride;
        p.row_stride = row_stride;
        p.channels = channels;
        p.first = l == 0;
        p.pyr = pyr;
        p.pyr_stride = L.frame_px;
        p.src_off = L.off[l];
        p.sw = L.w[l];
        p.sh = L.h[l];
        const bool dst = l + 1 < L.nlevels;
        p.dst_off = dst ? L.off[l + 1] : 0;
        p.dw = dst ? L.w[l + 1] : 0;
        p.dh = dst ? L.h[l + 1] : 0;
        // the grid covers the half-size level whether or not it is built: its tiles' interiors cover the source
        const int gw = (p.sw + 1) / 2, gh = (p.sh + 1) / 2;
        const dim3 grid((gw + kPyrTW - 1) / kPyrTW, (gh + kPyrTH - 1) / kPyrTH, nframes);
        hipLaunchKernelGGL(klt_gray_pyr, grid, dim3(kPyrThreads), 0, s, p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_klt_scharr(hipStream_t s, const uint8_t* pyr, const KltLayout& L, int16_t* deriv)
{
    const dim3 grid((L.w[0] + 63) / 64, (L.h[0] + 3) / 4, L.nlevels);
    hipLaunchKernelGGL(klt_scharr, grid, dim3(256), 0, s, pyr, L, reinterpret_cast<short2*>(deriv));
    return hipGetLastError();
}

hipError_t launch_klt_track(hipStream_t s, const KltLayout& L, const uint8_t* prev_pyr, const int16_t* deriv,
                            const uint8_t* next_pyr, int nframes, const float* prev_pts, int n, float* next_pts,
                            uint8_t* status, float* err, int32_t* counts, int win_w, int win_h, int max_count,
                            double eps2, int flags, float min_eig)
{
    TrackParams p;
    p.prev_pyr = prev_pyr;
    p.deriv = reinterpret_cast<const short2*>(deriv);
    p.next_pyr = next_pyr;
    p.next_stride = L.frame_px;
    p.L = L;
    p.prev_pts = prev_pts;
    p.next_pts = next_pts;
    p.status = status;
    p.err = err;
    p.counts = counts;
    p.n = n;
    p.win_w = win_w;
    p.win_h = win_h;
    p.max_count = max_count;
    p.flags = flags;
    p.min_eig = min_eig;
    p.eps2 = eps2;
    hipLaunchKernelGGL(klt_track, dim3(n, nframes), dim3(64), (size_t)win_w * win_h * 4 * sizeof(short), s, p);
    return hipGetLastError();
}

}  // namespace slamhip

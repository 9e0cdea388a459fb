// Chessboard calibration on the device (tests/calib_ref.py is
// the definition of every value computed here):
//
//   chess_response  BGR / gray photo -> s x s area-mean level tile (+ 5 px halo)
//                   in LDS -> 80 x the ChESS response of every level pixel, int32.
//                   The photo is read once; the level image never reaches HBM.
//                   A thread scores 4 horizontally adjacent pixels: every ring
//                   row is one byte-aligned dword cut from two LDS dwords
//                   (v_alignbyte), as fast_detect's prefilter takes its circle.
//   chess_nms       15 x 15 window maximum with the raster tie rule on a response
//                   tile (+ 7 px halo) in LDS; one 64-bit ballot per (row, tile).
//   chess_emit      one workgroup per frame: popcounts per row, an exclusive scan
//                   over the rows, candidates written in raster order.  No atomics:
//                   the order is that of the masks (the idea of fast_emit).
//   calib_subpix    cv::cornerSubPix, one wave per corner: the 64 lanes sample the
//                   window (getRectSubPix 8u -> 32f) and form the f64 products of
//                   the five sums in LDS; five lanes add them in raster order (a
//                   tree would change the result).
#include "slamhip_internal.h"

#include <cfloat>
#include <cmath>

namespace slamhip {

namespace {

constexpr int TW = kChessTileW, TH = kChessTileH;
constexpr int kRing = 5;                       // ring radius = response border
constexpr int kNms = 7;                        // 15 x 15 window
constexpr int kThreads = 256;
constexpr int LW = TW + 2 * kRing;             // 74 level columns per tile
constexpr int LPITCH = 80;                     // dword rows; row4 reads up to byte 75
constexpr int NW = TW + 2 * kNms;              // 78
static_assert(TW == 64 && TH * (TW / 4) == kThreads, "one wave per tile row, one 4-pixel task per thread");
static_assert((LW + 3) / 4 * 4 + 4 <= LPITCH, "row4's second dword stays in the row");

struct ChessParams {
    const uint8_t* img;
    size_t frame_stride, row_stride;
    int channels, s, W, H;      // level size W x H = floor(w / s) x floor(h / s)
    int32_t* resp;              // nframes x H x W
};

__device__ __forceinline__ uint32_t gray_at(const uint8_t* p, int channels)
{
    if (channels == 1) return p[0];
    return ((uint32_t)p[0] * 1868u + (uint32_t)p[1] * 9617u + (uint32_t)p[2] * 4899u + (1u << 13)) >> 14;
}

// the 16-sample radius-5 ring, (dx, dy) in the contract's order
__device__ constexpr int kRingDx[16] = {0, 2, 3, 5, 5, 5, 3, 2, 0, -2, -3, -5, -5, -5, -3, -2};
__device__ constexpr int kRingDy[16] = {-5, -5, -3, -2, 0, 2, 3, 5, 5, 5, 3, 2, 0, -2, -3, -5};

__global__ __launch_bounds__(kThreads) void chess_response(ChessParams p)
{
    __shared__ __attribute__((aligned(16))) uint8_t g[TH + 2 * kRing][LPITCH];
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * TW, Y0 = blockIdx.y * TH;
    const uint8_t* img = p.img + blockIdx.z * p.frame_stride;
    const int s = p.s, ss = s * s;

    // level tile + halo: the s x s area mean, round half up.  Level pixels outside
    // the level image are 0; they only reach responses the border rule zeroes.
    for (int i = tid; i < (TH + 2 * kRing) * LW; i += kThreads) {
        const int ly = i / LW, lx = i - ly * LW;
        const int X = X0 - kRing + lx, Y = Y0 - kRing + ly;
        uint32_t v = 0;
        if (X >= 0 && X < p.W && Y >= 0 && Y < p.H) {
            const uint8_t* q = img + (size_t)Y * s * p.row_stride + (size_t)X * s * p.channels;
            if (s == 1) {
                v = gray_at(q, p.channels);
            } else {
                uint32_t sum = 0;
                for (int dy = 0; dy < s; dy++, q += p.row_stride)
                    for (int dx = 0; dx < s; dx++) sum += gray_at(q + dx * p.channels, p.channels);
                v = (sum + ss / 2) / ss;
            }
        }
        g[ly][lx] = (uint8_t)v;
    }
    __syncthreads();

    const int ly = tid / (TW / 4), lx0 = 4 * (tid % (TW / 4));
    const int Y = Y0 + ly;
    if (Y >= p.H || X0 + lx0 >= p.W) return;
    const int cy = ly + kRing, cx = lx0 + kRing;
    // bytes g[r][b .. b + 3], b >= 0, from the two dwords that hold them
    auto row4 = [&](int r, int b) __attribute__((always_inline)) -> uint32_t {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(&g[r][b & ~3]);
        return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(b & 3));
    };
    uint32_t ring[16];
#pragma unroll
    for (int n = 0; n < 16; n++) ring[n] = row4(cy + kRingDy[n], cx + kRingDx[n]);
    const uint32_t c0 = row4(cy, cx), cl = row4(cy, cx - 1), cr = row4(cy, cx + 1), cu = row4(cy - 1, cx),
                   cd = row4(cy + 1, cx);
    int32_t out[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        auto px = [k](uint32_t v) { return (int)((v >> (8 * k)) & 255u); };
        int I[16];
#pragma unroll
        for (int n = 0; n < 16; n++) I[n] = px(ring[n]);
        const int L = px(c0) + px(cl) + px(cr) + px(cu) + px(cd);
        int SR = 0, DR = 0, sum = 0;
#pragma unroll
        for (int n = 0; n < 4; n++) SR += abs(I[n] + I[n + 8] - I[n + 4] - I[n + 12]);
#pragma unroll
        for (int n = 0; n < 8; n++) DR += abs(I[n] - I[n + 8]);
#pragma unroll
        for (int n = 0; n < 16; n++) sum += I[n];
        const int MR = abs(5 * sum - 16 * L);
        const int X = X0 + lx0 + k;
        const bool scored = X >= kRing && X < p.W - kRing && Y >= kRing && Y < p.H - kRing;
        out[k] = scored ? 80 * (SR - DR) - 16 * MR : 0;
    }
    int32_t* dst = p.resp + ((size_t)blockIdx.z * p.H + Y) * p.W + X0 + lx0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (X0 + lx0 + k < p.W) dst[k] = out[k];
}

__global__ __launch_bounds__(kThreads) void chess_nms(const int32_t* __restrict__ resp, int W, int H, int ntx,
                                                      uint64_t* __restrict__ masks)
{
    __shared__ int32_t t[TH + 2 * kNms][NW];
    const int tid = threadIdx.x;
    const int X0 = blockIdx.x * TW, Y0 = blockIdx.y * TH;
    const int32_t* R = resp + (size_t)blockIdx.z * W * H;
    for (int i = tid; i < (TH + 2 * kNms) * NW; i += kThreads) {
        const int ly = i / NW, lx = i - ly * NW;
        const int X = X0 - kNms + lx, Y = Y0 - kNms + ly;
        t[ly][lx] = (X >= 0 && X < W && Y >= 0 && Y < H) ? R[(size_t)Y * W + X] : 0;   // outside counts as 0
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int rr = 0; rr < TH / 4; rr++) {
        const int ly = wave * (TH / 4) + rr;
        const int Y = Y0 + ly, X = X0 + lane;
        if (Y >= H) break;                                  // uniform in the wave
        const int v = t[ly + kNms][lane + kNms];
        bool keep = v > 0 && X < W;
        if (keep) {
            // strictly above everything earlier in raster order, at least everything later
            for (int dy = -kNms; dy <= kNms && keep; dy++) {
                const int32_t* row = &t[ly + kNms + dy][lane];
                for (int dx = 0; dx <= 2 * kNms; dx++) {
                    const int u = row[dx];
                    const bool earlier = dy < 0 || (dy == 0 && dx < kNms);
                    if (earlier ? u >= v : (u > v)) keep = false;
                }
            }
        }
        const uint64_t m = __ballot(keep);
        if (lane == 0) masks[((size_t)blockIdx.z * H + Y) * ntx + blockIdx.x] = m;
    }
}

constexpr int kEmitThreads = 1024;   // one thread per level row: H <= 1024 by the level rule

__global__ __launch_bounds__(kEmitThreads) void chess_emit(const int32_t* __restrict__ resp,
                                                           const uint64_t* __restrict__ masks, int W, int H, int ntx,
                                                           int cap, int32_t* __restrict__ out, int32_t* __restrict__ counts)
{
    __shared__ int sc[2][kEmitThreads];
    const int r = threadIdx.x, f = blockIdx.x;
    const uint64_t* mrow = masks + ((size_t)f * H + r) * ntx;
    int cnt = 0;
    if (r < H)
        for (int j = 0; j < ntx; j++) cnt += __popcll(mrow[j]);
    sc[0][r] = cnt;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kEmitThreads; d <<= 1, cur ^= 1) {
        sc[cur ^ 1][r] = sc[cur][r] + (r >= d ? sc[cur][r - d] : 0);
        __syncthreads();
    }
    int base = sc[cur][r] - cnt;     // rows before this one
    if (r == kEmitThreads - 1) counts[f] = sc[cur][r];
    if (r >= H) return;
    const int32_t* R = resp + (size_t)f * W * H + (size_t)r * W;
    int32_t* o = out + (size_t)f * cap * 3;
    for (int j = 0; j < ntx; j++) {
        uint64_t m = mrow[j];
        while (m) {
            const int x = j * 64 + __builtin_ctzll(m);
            m &= m - 1;
            if (base < cap) {
                o[3 * (size_t)base] = x;
                o[3 * (size_t)base + 1] = r;
                o[3 * (size_t)base + 2] = R[x];
            }
            base++;
        }
    }
}

// ---- cornerSubPix ------------------------------------------------------------------

constexpr int kSubMaxWin = 2 * kSubpixMaxWin + 1;        // 31
constexpr int kSubMaxBuf = kSubMaxWin + 2;               // 33

struct SubpixParams {
    const uint8_t* img;
    size_t row_stride;
    int channels, w, h;
    int win_w, win_h, max_iter;
    double eps2;
    const float* vx;     // 2 win_w + 1
    const float* vy;     // 2 win_h + 1
    float* corners;      // n x 2, in and out
};

__device__ __forceinline__ float subpix_px(const SubpixParams& p, int y, int x)
{
    return (float)gray_at(p.img + (size_t)y * p.row_stride + (size_t)x * p.channels, p.channels);
}

__global__ __launch_bounds__(64) void calib_subpix(SubpixParams p)
{
    __shared__ float sub[kSubMaxBuf * kSubMaxBuf];
    __shared__ double prod[5][kSubMaxWin * kSubMaxWin];
    __shared__ double sums[5];
    const int lane = threadIdx.x;
    const int ww = 2 * p.win_w + 1, wh = 2 * p.win_h + 1, sw = ww + 2, sh = wh + 2;
    const float cTx = p.corners[2 * (size_t)blockIdx.x], cTy = p.corners[2 * (size_t)blockIdx.x + 1];
    float cIx = cTx, cIy = cTy;
    int iter = 0;
    double err = 0;
    // every lane carries the same corner and takes the same branches
    do {
        // getRectSubPix(src, (sw, sh), cI) 8u -> 32f
        const float cx = cIx - (float)(sw - 1) * 0.5f, cy = cIy - (float)(sh - 1) * 0.5f;
        const int ipx = (int)floorf(cx), ipy = (int)floorf(cy);
        float a = cx - (float)ipx;
        const float b = cy - (float)ipy;
        if (0 <= ipx && ipx + sw < p.w && 0 <= ipy && ipy + sh < p.h) {
            // getRectSubPix_8u32f: the window and its right / lower neighbours are inside
            a = fmaxf(a, 0.0001f);
            const float a12 = a * (1.f - b), a22 = a * b, b1 = 1.f - b, b2 = b;
            const double s = (1. - (double)a) / (double)a;
            for (int i = lane; i < sw * sh; i += 64) {
                const int r = i / sw, j = i - r * sw;
                const int y = ipy + r, x = ipx + j;
                const float t = a12 * subpix_px(p, y, x + 1) + a22 * subpix_px(p, y + 1, x + 1);
                float prev;
                if (j == 0) {
                    prev = (1.f - a) * (b1 * subpix_px(p, y, x) + b2 * subpix_px(p, y + 1, x));
                } else {
                    const float tp = a12 * subpix_px(p, y, x) + a22 * subpix_px(p, y + 1, x);
                    prev = (float)((double)tp * s);
                }
                sub[i] = prev + t;
            }
        } else {
            // getRectSubPix_Cn_ with adjustRect: replicated border; indices clamped to the image
            const float a11 = (1.f - a) * (1.f - b), a12 = a * (1.f - b), a21 = (1.f - a) * b, a22 = a * b;
            const float b1 = 1.f - b, b2 = b;
            const int rx = max(-ipx, 0), rw = ipx < p.w - sw ? sw : p.w - ipx - 1;
            const int xl = min(max(ipx + rx, 0), p.w - 1), xr = min(max(ipx + rw, 0), p.w - 1);
            for (int i = lane; i < sw * sh; i += 64) {
                const int r = i / sw, j = i - r * sw;
                const int ya = min(max(ipy + r, 0), p.h - 1), yb = min(max(ipy + r + 1, 0), p.h - 1);
                float v;
                if (j < rx) {
                    v = subpix_px(p, ya, xl) * b1 + subpix_px(p, yb, xl) * b2;
                } else if (j >= rw) {
                    v = subpix_px(p, ya, xr) * b1 + subpix_px(p, yb, xr) * b2;
                } else {
                    const int x0 = min(max(ipx + j, 0), p.w - 1), x1 = min(max(ipx + j + 1, 0), p.w - 1);
                    v = subpix_px(p, ya, x0) * a11 + subpix_px(p, ya, x1) * a12 + subpix_px(p, yb, x0) * a21 +
                        subpix_px(p, yb, x1) * a22;
                }
                sub[i] = v;
            }
        }
        __syncthreads();
        for (int i = lane; i < ww * wh; i += 64) {
            const int r = i / ww, j = i - r * ww;
            const float* c = &sub[(r + 1) * sw + j + 1];
            const double m = (double)(p.vy[r] * p.vx[j]);
            const double tgx = (double)(c[1] - c[-1]);
            const double tgy = (double)(c[sw] - c[-sw]);
            const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
            const double px = (double)(j - p.win_w), py = (double)(r - p.win_h);
            prod[0][i] = gxx;
            prod[1][i] = gxy;
            prod[2][i] = gyy;
            prod[3][i] = gxx * px + gxy * py;
            prod[4][i] = gxy * px + gyy * py;
        }
        __syncthreads();
        if (lane < 5) {
            // the source's raster-order sums
            const double* q = prod[lane];
            double acc = 0;
            for (int i = 0; i < ww * wh; i++) acc += q[i];
            sums[lane] = acc;
        }
        __syncthreads();
        const double A = sums[0], B = sums[1], C = sums[2], bb1 = sums[3], bb2 = sums[4];
        __syncthreads();               // sums are rewritten by the next iteration
        const double det = A * C - B * B;
        if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) break;
        const double scale = 1.0 / det;
        const float nx = (float)((double)cIx + C * scale * bb1 - B * scale * bb2);
        const float ny = (float)((double)cIy - B * scale * bb1 + A * scale * bb2);
        const float dx = nx - cIx, dy = ny - cIy;
        err = (double)(dx * dx + dy * dy);
        cIx = nx;
        cIy = ny;
        if (cIx < 0 || cIx >= (float)p.w || cIy < 0 || cIy >= (float)p.h) break;
    } while (++iter < p.max_iter && err > p.eps2);
    // too far from the start: poor convergence, the start stays
    if (fabsf(cIx - cTx) > (float)p.win_w || fabsf(cIy - cTy) > (float)p.win_h) {
        cIx = cTx;
        cIy = cTy;
    }
    if (lane == 0) {
        p.corners[2 * (size_t)blockIdx.x] = cIx;
        p.corners[2 * (size_t)blockIdx.x + 1] = cIy;
    }
}

}  // namespace

int chess_scale(int w, int h) { return std::max(1, (std::max(w, h) + 1023) / 1024); }

int chess_cap(int w, int h)
{
    const int s = chess_scale(w, h);
    return ((w / s + 7) / 8) * ((h / s + 7) / 8);
}

// candidates of nframes frames (frame f at img + f * frame_stride) into
// c->calib_out: nframes x chess_cap x 3 int32, then nframes counts
hipError_t launch_chess_candidates(slam_ctx* c, hipStream_t s, const uint8_t* img, size_t frame_stride,
                                   size_t row_stride, int channels, int nframes, int w, int h)
{
    const int sc = chess_scale(w, h);
    const int W = w / sc, H = h / sc;
    const int ntx = (W + TW - 1) / TW, nty = (H + TH - 1) / TH;
    const int cap = chess_cap(w, h);
    hipError_t e;
    if ((e = c->calib_resp.ensure((size_t)nframes * W * H * sizeof(int32_t))) != hipSuccess) return e;
    if ((e = c->calib_mask.ensure((size_t)nframes * H * ntx * sizeof(uint64_t))) != hipSuccess) return e;
    if ((e = c->calib_out.ensure(((size_t)nframes * cap * 3 + nframes) * sizeof(int32_t))) != hipSuccess) return e;
    ChessParams p;
    p.img = img;
    p.frame_stride = frame_stride;
    p.row_stride = row_stride;
    p.channels = channels;
    p.s = sc;
    p.W = W;
    p.H = H;
    p.resp = c->calib_resp.as<int32_t>();
    const dim3 grid(ntx, nty, nframes);
    hipLaunchKernelGGL(chess_response, grid, dim3(kThreads), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(chess_nms, grid, dim3(kThreads), 0, s, p.resp, W, H, ntx, c->calib_mask.as<uint64_t>());
    if ((e = hipGetLastError()) != hipSuccess) return e;
    int32_t* out = c->calib_out.as<int32_t>();
    hipLaunchKernelGGL(chess_emit, dim3(nframes), dim3(kEmitThreads), 0, s, p.resp, c->calib_mask.as<uint64_t>(), W, H,
                       ntx, cap, out, out + (size_t)nframes * cap * 3);
    return hipGetLastError();
}

// d_corners: n x 2 f32 on the device, refined in place; d_vx / d_vy: the mask's factors
hipError_t launch_calib_subpix(hipStream_t s, const uint8_t* img, size_t row_stride, int channels, int w, int h,
                               float* d_corners, int n, int win_w, int win_h, int max_iter, double eps,
                               const float* d_vx, const float* d_vy)
{
    SubpixParams p;
    p.img = img;
    p.row_stride = row_stride;
    p.channels = channels;
    p.w = w;
    p.h = h;
    p.win_w = win_w;
    p.win_h = win_h;
    p.max_iter = max_iter;
    p.eps2 = eps * eps;
    p.vx = d_vx;
    p.vy = d_vy;
    p.corners = d_corners;
    hipLaunchKernelGGL(calib_subpix, dim3(n), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace slamhip

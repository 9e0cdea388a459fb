// Full ORB detector, gfx950: cv::ORB::create(nfeatures, scaleFactor, nlevels, 31, 0, 2,
// scoreType, 31, fastThreshold)->detectAndCompute(img, noArray(), kps, desc) over a batch
// of frames resident in device memory.
//
// Restated from OpenCV 4.8 features2d/src/orb.cpp from upstream knowledge (no OpenCV
// build is at hand: fidelity to one is NOT verified); the kernels are held byte for
// byte to tests/orb_detect_ref.py.  One stated deviation: inside
// a level the keypoints come in raster (y, x) order, where OpenCV leaves what
// std::nth_element produced.
//
// Every launch covers one pyramid level of the whole batch:
//   orbdet_gray          cvtColor(BGR2GRAY) of the packed frames into level 0
//   orbdet_down          resize(INTER_LINEAR_EXACT) level l-1 -> l: one workgroup per
//                        64 x 64 destination tile, its source tile staged in LDS,
//                        offsets and weights from tables built on the host (doubles
//                        in OpenCV's order), pure integer arithmetic on the device
//   fast_detect / _emit  fast.hip on the level planes (1 channel, border 31)
//   orbdet_select        KeyPointsFilter::retainBest per (frame, level) segment: the n-th
//                        largest response from a 256-bin LDS histogram (FAST scores) or
//                        a 4-pass 8-bit radix select on the order-preserving u32 image
//                        of the float (Harris), then an order-preserving ballot +
//                        prefix-sum compaction (ties all kept)
//   orbdet_harris        HarrisResponses, one wave per keypoint (lane = block pixel)
//   orbdet_pack          the segments' survivors -> one contiguous list
//   orbdet_angle         IC_Angle, one wave per keypoint, hal::fastAtan2 on lane 0
//   orb_blur / orb_desc  orb.hip on the level planes, {cos, sin} per keypoint from
//                        the host (glibc cosf / sinf, as the oracle's)
//   orbdet_emit          level coordinates -> cv::KeyPoint, rows to the frame's output
#include <algorithm>
#include <cmath>
#include <cstring>

#include "sift_dev.h"
#include "slamhip_internal.h"

namespace slamhip {

namespace {

constexpr int kHalfPatch = 15;          // ORB patchSize 31
constexpr int kHarrisBlock = 7;
// od_cnt (int32): per-frame counts after the first / second selection, the level's
// offsets in the packed list, each frame's output row of the level's first keypoint,
// the keypoints emitted so far, then the packed list's length
constexpr int kCnt1 = 0, kCnt2 = kOrbDetectMaxFrames, kLvlOff = 2 * kOrbDetectMaxFrames,
              kBase = 3 * kOrbDetectMaxFrames, kAcc = 4 * kOrbDetectMaxFrames, kTotal = 5 * kOrbDetectMaxFrames,
              kCntInts = 5 * kOrbDetectMaxFrames + 16;

// ORB_Impl's umax for half patch 15 (tests/orb_detect_ref.py derives it)
__constant__ int8_t c_umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};

__global__ __launch_bounds__(256) void orbdet_gray(const uint8_t* img, int channels, int w, int h, uint8_t* gray)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const uint8_t* s = img + ((size_t)blockIdx.z * h + y) * ((size_t)w * channels) + (size_t)x * channels;
    uint32_t v;
    if (channels == 1) v = s[0];
    else v = ((uint32_t)s[0] * 1868u + (uint32_t)s[1] * 9617u + (uint32_t)s[2] * 4899u + (1u << 13)) >> 14;
    gray[(size_t)blockIdx.z * w * h + (size_t)y * w + x] = (uint8_t)v;
}

// table entry of one destination index: first source index (low 16 bits), weight of
// the next source index out of 256 (high bits); the next index is clamped to the
// last one, where the weight is 0 by construction
struct DownParams {
    const uint8_t* src;
    uint8_t* dst;
    int sw, sh, dw, dh;
    const uint32_t* tabx;
    const uint32_t* taby;
};

constexpr int kDT = 64;      // destination tile (square)
constexpr int kDS = 80;      // source tile rows / columns held in LDS (ratio <= ~1.22)

__global__ __launch_bounds__(256) void orbdet_down(DownParams p)
{
    __shared__ uint8_t t[kDS * kDS];
    __shared__ uint32_t ex[kDT], ey[kDT];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kDT, y0 = blockIdx.y * kDT;
    const int nx = min(kDT, p.dw - x0), ny = min(kDT, p.dh - y0);
    const uint8_t* src = p.src + (size_t)blockIdx.z * p.sw * p.sh;
    uint8_t* dst = p.dst + (size_t)blockIdx.z * p.dw * p.dh;
    if (tid < kDT) ex[tid] = p.tabx[x0 + min(tid, nx - 1)];
    else if (tid < 2 * kDT) ey[tid - kDT] = p.taby[y0 + min(tid - kDT, ny - 1)];
    __syncthreads();
    // the tile's source rectangle (the tables are non-decreasing)
    const int sx0 = (int)(ex[0] & 0xffffu), sx1 = min((int)(ex[nx - 1] & 0xffffu) + 1, p.sw - 1);
    const int sy0 = (int)(ey[0] & 0xffffu), sy1 = min((int)(ey[ny - 1] & 0xffffu) + 1, p.sh - 1);
    const int tw = sx1 - sx0 + 1, th = sy1 - sy0 + 1;
    const bool staged = tw <= kDS && th <= kDS;      // uniform; larger ratios read the source directly
    if (staged) {
        for (int i = tid; i < tw * th; i += 256) {
            const int r = i / tw, c = i - r * tw;
            t[r * kDS + c] = src[(size_t)(sy0 + r) * p.sw + sx0 + c];
        }
    }
    __syncthreads();
    // four adjacent destination pixels per thread, 16 rows per pass
    const int c4 = 4 * (tid & 15);
    for (int r = tid >> 4; r < ny; r += 16) {
        const uint32_t wy = ey[r];
        const int ya = (int)(wy & 0xffffu), yb = min(ya + 1, p.sh - 1);
        const uint32_t cy1 = wy >> 16, cy0 = 256u - cy1;
        uint32_t out = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = min(c4 + q, nx - 1);
            const uint32_t wx = ex[c];
            const int xa = (int)(wx & 0xffffu), xb = min(xa + 1, p.sw - 1);
            const uint32_t cx1 = wx >> 16, cx0 = 256u - cx1;
            uint32_t s00, s01, s10, s11;
            if (staged) {
                const uint8_t* ra = t + (ya - sy0) * kDS - sx0;
                const uint8_t* rb = t + (yb - sy0) * kDS - sx0;
                s00 = ra[xa]; s01 = ra[xb]; s10 = rb[xa]; s11 = rb[xb];
            } else {
                const uint8_t* ra = src + (size_t)ya * p.sw;
                const uint8_t* rb = src + (size_t)yb * p.sw;
                s00 = ra[xa]; s01 = ra[xb]; s10 = rb[xa]; s11 = rb[xb];
            }
            const uint32_t h0 = s00 * cx0 + s01 * cx1;       // the u16 horizontal pass, exact
            const uint32_t h1 = s10 * cx0 + s11 * cx1;
            const uint32_t v = h0 * cy0 + h1 * cy1;          // the u32 vertical pass, exact
            out |= ((v + 32768u) >> 16) << (8 * q);
        }
        uint8_t* d = dst + (size_t)(y0 + r) * p.dw + x0 + c4;
        if ((p.dw & 3) == 0 && c4 + 3 < nx) {
            *reinterpret_cast<uint32_t*>(d) = out;
        } else {
            for (int q = 0; q < 4 && c4 + q < nx; q++) d[q] = (uint8_t)(out >> (8 * q));
        }
    }
}

// order-preserving u32 image of a float (-0 taken as +0)
__device__ __forceinline__ uint32_t resp_key(float x)
{
    const uint32_t u = __float_as_uint(__fadd_rn(x, 0.f));
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct SelectParams {
    const slam_keypoint* in;
    slam_keypoint* out;
    const int4* frame_info;   // .x: the frame's segment offset (both lists), .y: FAST's count
    const int* in_cnt;        // the segment's length; null: frame_info[f].y
    int* out_cnt;
    int keep;                 // retainBest's n
    int int_scores;           // the responses are FAST scores: integers 0 .. 255
};

constexpr int kSelThreads = 1024, kSelWaves = kSelThreads / 64;

// KeyPointsFilter::retainBest on one frame's segment: one workgroup.  The cut (the
// n-th largest response) comes from one 256-bin histogram for FAST scores, from a
// 4-pass 8-bit radix select on the float's order-preserving image otherwise
__global__ __launch_bounds__(kSelThreads) void orbdet_select(SelectParams p)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_k;
    __shared__ int wsum[kSelWaves];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int off = p.frame_info[f].x;
    const int n = p.in_cnt ? p.in_cnt[f] : p.frame_info[f].y;
    if (p.keep <= 0 || n <= 0) {
        if (tid == 0) p.out_cnt[f] = 0;
        return;
    }
    const slam_keypoint* in = p.in + off;
    slam_keypoint* out = p.out + off;
    const bool ints = p.int_scores != 0;
    auto key_of = [&](float r) { return ints ? (uint32_t)r : resp_key(r); };
    uint32_t cut = 0;        // keep every key >= cut
    if (n > p.keep) {
        uint32_t prefix = 0, mask = 0, k = (uint32_t)p.keep;
        for (int shift = ints ? 0 : 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < n; i += kSelThreads) {
                const uint32_t key = key_of(in[i].response);
                if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                // the digit of the k-th largest among the keys that share the prefix
                uint32_t kk = k;
                int b = 255;
                for (; b > 0; b--) {
                    if (hist[b] >= kk) break;
                    kk -= hist[b];
                }
                s_prefix = prefix | ((uint32_t)b << shift);
                s_k = kk;
            }
            __syncthreads();
            prefix = s_prefix;
            k = s_k;
            mask |= 0xffu << shift;
            __syncthreads();
        }
        cut = prefix;
    }
    int run = 0;
    for (int base = 0; base < n; base += kSelThreads) {
        const int i = base + tid;
        slam_keypoint kp;
        bool keep = false;
        if (i < n) {
            kp = in[i];
            keep = key_of(kp.response) >= cut;
        }
        const uint64_t m = __ballot(keep);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int pos = run + __popcll(m & ((1ull << lane) - 1ull));
        int all = 0;
#pragma unroll
        for (int q = 0; q < kSelWaves; q++) {
            if (q < wave) pos += wsum[q];
            all += wsum[q];
        }
        if (keep) out[pos] = kp;
        run += all;
        __syncthreads();
    }
    if (tid == 0) p.out_cnt[f] = run;
}

struct PointParams {
    slam_keypoint* kps;
    const uint8_t* img;       // the level planes, frame f at f * w * h
    int w, h;
    const int4* frame_info;   // harris: segment offsets
    const int* cnt;           // harris: segment lengths
    const int* kp_frame;      // angle: the packed list's frames
    int total;                // angle: the packed list's length
    float* ang;               // angle: the angles alone (the host's {cos, sin} input)
    float scale_sq_sq;
};

// HarrisResponses(blockSize 7, k 0.04): grid (x, frame), one wave per keypoint of
// the frame's segment; lane < 49 owns one block pixel, the integer sums are order-free
__global__ __launch_bounds__(256) void orbdet_harris(PointParams p)
{
    const int f = blockIdx.y, lane = threadIdx.x & 63;
    const int n = p.cnt[f];
    slam_keypoint* kps = p.kps + p.frame_info[f].x;
    const uint8_t* img = p.img + (size_t)f * p.w * p.h;
    const int by = lane / kHarrisBlock - kHarrisBlock / 2, bx = lane % kHarrisBlock - kHarrisBlock / 2;
    for (int j = blockIdx.x * 4 + (threadIdx.x >> 6); j < n; j += gridDim.x * 4) {
        const int x = (int)kps[j].x, y = (int)kps[j].y;
        int a = 0, b = 0, c = 0;
        if (lane < kHarrisBlock * kHarrisBlock) {
            const uint8_t* q = img + (size_t)(y + by) * p.w + (x + bx);
            const int s = p.w;
            const int Ix = ((int)q[1] - (int)q[-1]) * 2 + ((int)q[-s + 1] - (int)q[-s - 1]) +
                           ((int)q[s + 1] - (int)q[s - 1]);
            const int Iy = ((int)q[s] - (int)q[-s]) * 2 + ((int)q[s - 1] - (int)q[-s - 1]) +
                           ((int)q[s + 1] - (int)q[-s + 1]);
            a = Ix * Ix; b = Iy * Iy; c = Ix * Iy;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o, 64);
            b += __shfl_xor(b, o, 64);
            c += __shfl_xor(c, o, 64);
        }
        if (lane == 0) {
            const float fa = (float)a, fb = (float)b, fc = (float)c;
            const float s = __fadd_rn(fa, fb);
            const float det = __fsub_rn(__fmul_rn(fa, fb), __fmul_rn(fc, fc));
            const float r = __fsub_rn(det, __fmul_rn(__fmul_rn(0.04f, s), s));
            kps[j].response = __fmul_rn(r, p.scale_sq_sq);
        }
    }
}

struct PackParams {
    const slam_keypoint* in;
    const int4* frame_info;
    const int* cnt;
    int nframes;
    slam_keypoint* out;
    int* kp_frame;
    int* counters;            // od_cnt
};

// the segments' survivors -> one contiguous list in frame order; workgroup = frame
__global__ __launch_bounds__(256) void orbdet_pack(PackParams p)
{
    __shared__ int s_before[4], s_all[4];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mine = tid < p.nframes ? p.cnt[tid] : 0;     // nframes <= 256
    int before = tid < f ? mine : 0, all = mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        before += __shfl_xor(before, o, 64);
        all += __shfl_xor(all, o, 64);
    }
    if (lane == 0) { s_before[wave] = before; s_all[wave] = all; }
    __syncthreads();
    const int off = s_before[0] + s_before[1] + s_before[2] + s_before[3];
    const int n = p.cnt[f];
    if (tid == 0) {
        p.counters[kLvlOff + f] = off;
        const int acc = p.counters[kAcc + f];
        p.counters[kBase + f] = acc;
        p.counters[kAcc + f] = acc + n;
        if (f == 0) p.counters[kTotal] = s_all[0] + s_all[1] + s_all[2] + s_all[3];
    }
    const slam_keypoint* in = p.in + p.frame_info[f].x;
    for (int j = tid; j < n; j += 256) {
        p.out[off + j] = in[j];
        p.kp_frame[off + j] = f;
    }
}

// IC_Angle(half patch 15): one wave per keypoint of the packed list; the disc's rows
// are walked 2 per step (lane = row parity x column), the integer moments are order-free
__global__ __launch_bounds__(256) void orbdet_angle(PointParams p)
{
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= p.total) return;
    const slam_keypoint kp = p.kps[g];
    const int x = (int)kp.x, y = (int)kp.y;
    const uint8_t* center = p.img + (size_t)p.kp_frame[g] * p.w * p.h + (size_t)y * p.w + x;
    int m01 = 0, m10 = 0;
    const int u = (lane & 31) - kHalfPatch;
    for (int r = lane >> 5; r < 2 * kHalfPatch + 1; r += 2) {
        const int v = r - kHalfPatch;
        const int av = v < 0 ? -v : v, au = u < 0 ? -u : u;
        if (au <= (int)c_umax[av]) {       // u = 16 (lane 31 of a half) is outside every row
            const int val = center[v * p.w + u];
            m10 += u * val;
            m01 += v * val;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m01 += __shfl_xor(m01, o, 64);
        m10 += __shfl_xor(m10, o, 64);
    }
    if (lane == 0) {
        const float a = sd::fast_atan2_deg((float)m01, (float)m10);
        p.kps[g].angle = a;
        p.ang[g] = a;
    }
}

struct EmitParams {
    const slam_keypoint* kps;
    const int* kp_frame;
    const uint32_t* desc;     // total x 8 dwords
    const int* counters;
    int total, cap, level;
    float scale;
    slam_keypoint* out;
    uint32_t* out_desc;       // nullable
};

// eight threads per keypoint: a descriptor dword each, the first also the cv::KeyPoint
__global__ __launch_bounds__(256) void orbdet_emit(EmitParams p)
{
    const int i = blockIdx.x * 256 + threadIdx.x, g = i >> 3, q = i & 7;
    if (g >= p.total) return;
    const int f = p.kp_frame[g];
    const int row = p.counters[kBase + f] + (g - p.counters[kLvlOff + f]);
    if (row >= p.cap) return;
    const size_t dst = (size_t)f * p.cap + row;
    if (p.out_desc) p.out_desc[dst * 8 + q] = p.desc[(size_t)g * 8 + q];
    if (q == 0) {
        slam_keypoint k = p.kps[g];
        k.x = __fmul_rn(k.x, p.scale);
        k.y = __fmul_rn(k.y, p.scale);
        k.size = __fmul_rn(31.f, p.scale);
        k.octave = p.level;
        k.class_id = -1;
        p.out[dst] = k;
    }
}

inline int cv_round_f(float x) { return (int)lrintf(x); }
inline int cv_round_d(double x) { return (int)lrint(x); }

// resize(INTER_LINEAR_EXACT)'s coefficients of one axis, doubles in OpenCV's order
void resize_table(int src, int dst, uint32_t* out)
{
    const double scale = 1.0 / ((double)dst / src);
    for (int d = 0; d < dst; d++) {
        const double fx = scale * (d + 0.5) - 0.5;
        const int i = (int)std::floor(fx);
        uint32_t i0, c1;
        if (i < 0 || src == 1) { i0 = 0; c1 = 0; }
        else if (i >= src - 1) { i0 = (uint32_t)(src - 1); c1 = 0; }
        else { i0 = (uint32_t)i; c1 = (uint32_t)cv_round_d((fx - i) * 256.0); }
        out[d] = i0 | (c1 << 16);
    }
}

}  // namespace

void orb_detect_geometry(int w, int h, int nfeatures, double scale_factor, int nlevels, OrbDetLevel* lv)
{
    const float factor = (float)(1.0 / scale_factor);
    float nd = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels; l++) {
        lv[l].scale = (float)std::pow(scale_factor, (double)l);
        lv[l].w = cv_round_f((float)w / lv[l].scale);
        lv[l].h = cv_round_f((float)h / lv[l].scale);
        if (l < nlevels - 1) {
            lv[l].nfeatures = cv_round_f(nd);
            sum += lv[l].nfeatures;
            nd *= factor;
        } else {
            lv[l].nfeatures = std::max(nfeatures - sum, 0);
        }
    }
}

int orb_detect_batch(slam_ctx* c, hipStream_t s, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                     int nfeatures, double scale_factor, int nlevels, int fast_threshold, int score_type,
                     slam_keypoint* d_kps, int cap, int32_t* n_out, uint8_t* d_desc)
{
    OrbDetLevel lv[kOrbDetectMaxLevels];
    orb_detect_geometry(w, h, nfeatures, scale_factor, nlevels, lv);
    // the levels that can hold a keypoint (a level's size never grows); the pyramid
    // is built no further
    int used = 0;
    while (used < nlevels && lv[used].w > 2 * kOrbEdge && lv[used].h > 2 * kOrbEdge) used++;
    if (used == 0) return SLAM_OK;

    // level planes: level l's frames are contiguous, its base 256-byte aligned
    size_t base[kOrbDetectMaxLevels], bytes = 0;
    for (int l = 0; l < used; l++) {
        base[l] = bytes;
        bytes += ((size_t)nframes * lv[l].w * lv[l].h + 255) & ~(size_t)255;
    }
    SLAM_HIP(c, c->od_pyr.ensure(bytes));
    SLAM_HIP(c, c->od_cnt.ensure(kCntInts * sizeof(int)));
    uint8_t* pyr = c->od_pyr.as<uint8_t>();
    int* counters = c->od_cnt.as<int>();

    // the resize tables of (w, h, scaleFactor, nlevels), cached as the undistortion map is
    size_t tab_off[kOrbDetectMaxLevels][2] = {};
    {
        size_t n = 0;
        for (int l = 1; l < used; l++) {
            tab_off[l][0] = n; n += lv[l].w;
            tab_off[l][1] = n; n += lv[l].h;
        }
        const bool same = c->od_tab_valid && c->od_tab_w == w && c->od_tab_h == h && c->od_tab_levels == used &&
                          c->od_tab_scale == scale_factor;
        if (!same && n > 0) {
            c->od_tab_valid = false;
            std::vector<uint32_t> tab(n);
            for (int l = 1; l < used; l++) {
                resize_table(lv[l - 1].w, lv[l].w, tab.data() + tab_off[l][0]);
                resize_table(lv[l - 1].h, lv[l].h, tab.data() + tab_off[l][1]);
            }
            SLAM_HIP(c, c->od_tab.ensure(n * sizeof(uint32_t)));
            // the previous table's readers are on streams this call has been ordered after, or drained
            SLAM_HIP(c, hipMemcpyAsync(c->od_tab.p, tab.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
            if (int rc = stream_sync(c, s)) return rc;
            c->od_tab_w = w; c->od_tab_h = h; c->od_tab_levels = used; c->od_tab_scale = scale_factor;
            c->od_tab_valid = true;
        }
    }

    SLAM_HIP(c, hipMemsetAsync(counters, 0, kCntInts * sizeof(int), s));
    prof_begin(c, 8, s);
    hipLaunchKernelGGL(orbdet_gray, dim3((w + 255) / 256, h, nframes), dim3(256), 0, s, d_frames, channels, w, h, pyr);
    for (int l = 1; l < used; l++) {
        DownParams dp;
        dp.src = pyr + base[l - 1]; dp.dst = pyr + base[l];
        dp.sw = lv[l - 1].w; dp.sh = lv[l - 1].h; dp.dw = lv[l].w; dp.dh = lv[l].h;
        dp.tabx = c->od_tab.as<uint32_t>() + tab_off[l][0];
        dp.taby = c->od_tab.as<uint32_t>() + tab_off[l][1];
        hipLaunchKernelGGL(orbdet_down, dim3((dp.dw + kDT - 1) / kDT, (dp.dh + kDT - 1) / kDT, nframes), dim3(256), 0, s,
                           dp);
    }
    prof_end(c, 8, s);
    SLAM_HIP(c, hipGetLastError());

    const float hs = 1.f / (4 * kHarrisBlock * 255.f);
    const float scale_sq_sq = hs * hs * hs * hs;
    const bool harris = score_type == SLAM_ORB_HARRIS_SCORE;
    for (int l = 0; l < used; l++) {
        const int wl = lv[l].w, hl = lv[l].h, nl = lv[l].nfeatures;
        if (nl <= 0) continue;      // retainBest(0) clears the level
        const uint8_t* plane = pyr + base[l];
        // 3 x 3 non-max suppression leaves at most one corner per 2 x 2 pixels
        const size_t lcap = (size_t)nframes * ((wl + 1) / 2) * ((hl + 1) / 2);
        SLAM_HIP(c, launch_fast_detect(c, s, plane, (size_t)wl * hl, (size_t)wl, 1, nframes, wl, hl, fast_threshold, 1,
                                       kOrbEdge, SLAM_FAST_TYPE_9_16));
        SLAM_HIP(c, launch_fast_emit(c, s, nframes, wl, hl, (int)lcap));
        SLAM_HIP(c, c->od_kps.ensure(lcap * sizeof(slam_keypoint)));
        SLAM_HIP(c, c->od_list.ensure(lcap * sizeof(slam_keypoint)));
        SLAM_HIP(c, c->od_frame.ensure(lcap * sizeof(int)));
        slam_keypoint* A = c->kps.as<slam_keypoint>();
        slam_keypoint* B = c->od_kps.as<slam_keypoint>();
        slam_keypoint* P = c->od_list.as<slam_keypoint>();
        const int4* info = c->frame_info.as<int4>();

        SelectParams sp;
        sp.in = A; sp.out = B; sp.frame_info = info; sp.in_cnt = nullptr; sp.out_cnt = counters + kCnt1;
        sp.keep = harris ? 2 * nl : nl;
        sp.int_scores = 1;
        prof_begin(c, 9, s);
        hipLaunchKernelGGL(orbdet_select, dim3(nframes), dim3(kSelThreads), 0, s, sp);
        prof_end(c, 9, s);
        const slam_keypoint* fin = B;
        const int* fin_cnt = counters + kCnt1;
        PointParams pp;
        pp.img = plane; pp.w = wl; pp.h = hl; pp.frame_info = info; pp.scale_sq_sq = scale_sq_sq;
        pp.kp_frame = nullptr; pp.total = 0; pp.ang = nullptr;
        if (harris) {
            pp.kps = B; pp.cnt = counters + kCnt1;
            prof_begin(c, 10, s);
            hipLaunchKernelGGL(orbdet_harris, dim3(128, nframes), dim3(256), 0, s, pp);
            prof_end(c, 10, s);
            sp.in = B; sp.out = A; sp.in_cnt = counters + kCnt1; sp.out_cnt = counters + kCnt2; sp.keep = nl;
            sp.int_scores = 0;
            prof_begin(c, 9, s);
            hipLaunchKernelGGL(orbdet_select, dim3(nframes), dim3(kSelThreads), 0, s, sp);
            prof_end(c, 9, s);
            fin = A;
            fin_cnt = counters + kCnt2;
        }
        PackParams kp;
        kp.in = fin; kp.frame_info = info; kp.cnt = fin_cnt; kp.nframes = nframes; kp.out = P;
        kp.kp_frame = c->od_frame.as<int>(); kp.counters = counters;
        prof_begin(c, 9, s);
        hipLaunchKernelGGL(orbdet_pack, dim3(nframes), dim3(256), 0, s, kp);
        prof_end(c, 9, s);
        SLAM_HIP(c, hipGetLastError());
        // the blurred level is queued ahead of the count's read-back
        SLAM_HIP(c, c->orbblur.ensure((size_t)nframes * wl * hl));
        SLAM_HIP(c, launch_orb_blur_planes(c, s, plane, c->orbblur.as<uint8_t>(), nframes, wl, hl));
        int* h_total = static_cast<int*>(readback(c, 64));
        if (!h_total) return set_err(c, SLAM_E_HIP, "pinned readback buffer");
        SLAM_HIP(c, hipMemcpyAsync(h_total, counters + kTotal, sizeof(int), hipMemcpyDeviceToHost, s));
        if (int rc = stream_sync(c, s)) return rc;
        const int total = *h_total;
        if (total <= 0) continue;

        SLAM_HIP(c, c->od_ang.ensure((size_t)total * 3 * sizeof(float)));
        float* d_ang = c->od_ang.as<float>();
        float* d_ab = d_ang + total;
        pp.kps = P; pp.cnt = nullptr; pp.kp_frame = c->od_frame.as<int>(); pp.total = total; pp.ang = d_ang;
        prof_begin(c, 10, s);
        hipLaunchKernelGGL(orbdet_angle, dim3((total + 3) / 4), dim3(256), 0, s, pp);
        prof_end(c, 10, s);
        SLAM_HIP(c, hipGetLastError());
        // {cos, sin} on the host (glibc's, as the oracle's; the device's differ in the last place)
        float* h_ang = static_cast<float*>(readback(c, (size_t)total * 3 * sizeof(float)));
        if (!h_ang) return set_err(c, SLAM_E_HIP, "pinned readback buffer");
        SLAM_HIP(c, hipMemcpyAsync(h_ang, d_ang, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, s));
        if (int rc = stream_sync(c, s)) return rc;
        float* h_ab = h_ang + total;
        for (int i = 0; i < total; i++) {
            const float angle = h_ang[i] * (float)(M_PI / 180.f);
            h_ab[2 * i] = cosf(angle);
            h_ab[2 * i + 1] = sinf(angle);
        }
        SLAM_HIP(c, hipMemcpyAsync(d_ab, h_ab, (size_t)total * 2 * sizeof(float), hipMemcpyHostToDevice, s));
        SLAM_HIP(c, c->desc_u8.ensure((size_t)total * kOrbDescBytes));
        SLAM_HIP(c, c->desc_exp.ensure((size_t)total * kOrbExpBytes));
        SLAM_HIP(c, launch_orb_desc_on(c, s, c->orbblur.as<uint8_t>(), wl, hl, P, c->od_frame.as<int>(),
                                       counters + kTotal, d_ab, total, c->desc_u8.as<uint8_t>(),
                                       c->desc_exp.as<uint32_t>()));
        EmitParams ep;
        ep.kps = P; ep.kp_frame = c->od_frame.as<int>(); ep.desc = c->desc_u8.as<uint32_t>(); ep.counters = counters;
        ep.total = total; ep.cap = cap; ep.level = l; ep.scale = lv[l].scale;
        ep.out = d_kps; ep.out_desc = reinterpret_cast<uint32_t*>(d_desc);
        prof_begin(c, 11, s);
        hipLaunchKernelGGL(orbdet_emit, dim3((unsigned)(((size_t)total * 8 + 255) / 256)), dim3(256), 0, s, ep);
        prof_end(c, 11, s);
        SLAM_HIP(c, hipGetLastError());
    }
    int32_t* h_cnt = static_cast<int32_t*>(readback(c, (size_t)nframes * sizeof(int32_t)));
    if (!h_cnt) return set_err(c, SLAM_E_HIP, "pinned readback buffer");
    SLAM_HIP(c, hipMemcpyAsync(h_cnt, counters + kAcc, (size_t)nframes * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (int rc = stream_sync(c, s)) return rc;
    std::memcpy(n_out, h_cnt, (size_t)nframes * sizeof(int32_t));
    return SLAM_OK;
}

}  // namespace slamhip

// Place recognition: a flat visual vocabulary and bag-of-words retrieval, gfx950.
//
// The contract is tests/place_ref.py; the arithmetic shared with the host twin
// (place_host.cpp) is place_math.h.  Everything is integer except the one IEEE
// division of a score, so every result equals the reference bit for bit.
//
//   voc_assign_sift  nearest centroid of u8[128] descriptors by squared L2: knn.hip's
//                    int8 GEMM (x' = x ^ 0x80, d^2 = |x'|^2 + |c'|^2 - 2<x', c'>,
//                    v_mfma_i32_32x32x32_i8) with the descriptors on the lane columns
//                    and 32-centroid tiles streamed through LDS in ascending index
//                    order; the top-1 is kept with strict <, so a tie keeps the lower
//                    centroid.  No packed keys: the whole u8 range is legal.
//   voc_assign_orb   the same walk for 32-byte descriptors by Hamming distance,
//                    popcount on the VALU (one descriptor per lane, the centroid
//                    tile broadcast from LDS).
//   voc_assign_finish merges the partial winners of the K splits by (dist, index)
//                    and, for training, counts the words.
//   voc_scan / voc_scatter / voc_update_*: the Lloyd update as a counting sort by
//                    word and one workgroup per centroid (no float, no order
//                    dependence: the sums are integers).  Measured against u32
//                    atomics at the bench size: 0.3 ms against
//                    2.8 ms per iteration.
//   bow_hist_*       per-image word counts times the idf weights, and their total.
//   bow_score        histogram intersection of L1-normalised vectors, int64 sums.
//   bow_topk         one wave per query: k rounds of (score desc, index asc) selection.
#include <climits>
#include <cstring>

#include <vector>

#include "place_math.h"
#include "slamhip_internal.h"

namespace slamhip {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

struct AssignParams {
    const uint8_t* desc;
    int n;
    const uint8_t* cent;
    const int* cnorm;     // SIFT: |c'|^2 per centroid
    int K;
    int split;
    int2* part;           // [split][n] = {dist, word}
};

// centroids [lo, hi) of split z: 32-row tiles, the last split may be short or empty
__device__ __forceinline__ void voc_split_range(int K, int split, int z, int& lo, int& hi)
{
    int chunk = (K + split - 1) / split;
    chunk = (chunk + 31) & ~31;
    lo = z * chunk;
    hi = min(K, lo + chunk);
}

__device__ __forceinline__ int sumsq_i8x4(int w)
{
    const int a = (int)(int8_t)w, b = (int)(int8_t)(w >> 8), c = (int)(int8_t)(w >> 16), d = w >> 24;
    return a * a + b * b + c * c + d * d;
}

__global__ __launch_bounds__(256) void voc_cent_norm(const uint8_t* cent, int K, int* norm)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= K) return;
    const uint4* p = reinterpret_cast<const uint4*>(cent + (size_t)c * 128);
    int s = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint4 u = p[i];
        s += sumsq_i8x4((int)(u.x ^ 0x80808080u)) + sumsq_i8x4((int)(u.y ^ 0x80808080u)) +
             sumsq_i8x4((int)(u.z ^ 0x80808080u)) + sumsq_i8x4((int)(u.w ^ 0x80808080u));
    }
    norm[c] = s;
}

// Grid: x = 256-descriptor block (4 waves x 64 descriptors), y = split of the centroids.
// A = centroid tile (rows), B = descriptors (columns): the 32 x 32 accumulator puts one
// descriptor per lane column and 16 centroid rows in the lane's registers, row
// (j & 3) + 8 (j >> 2) + 4 (lane >> 5) at register j -- ascending in j, so strict <
// keeps the lowest index per lane; lanes l and l ^ 32 hold the two halves of a column.
__global__ __launch_bounds__(256) void voc_assign_sift(AssignParams p)
{
    constexpr int KB = 128, KS = 4;
    __shared__ __attribute__((aligned(16))) uint8_t tile[32 * KB];
    __shared__ __attribute__((aligned(16))) int tn_s[32];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const int qbase = blockIdx.x * 256 + wave * 64;
    const uint32_t xm = 0x80808080u;

    v4i bq[2][KS];
    int qn[2];
#pragma unroll
    for (int qt = 0; qt < 2; qt++) {
        const int q = qbase + qt * 32 + (lane & 31);
        int s = 0;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            v4i v = {0, 0, 0, 0};
            if (q < p.n) {
                const uint4 u = *reinterpret_cast<const uint4*>(p.desc + (size_t)q * KB + ks * 32 + h * 16);
                v = v4i{(int)(u.x ^ xm), (int)(u.y ^ xm), (int)(u.z ^ xm), (int)(u.w ^ xm)};
                s += sumsq_i8x4(v[0]) + sumsq_i8x4(v[1]) + sumsq_i8x4(v[2]) + sumsq_i8x4(v[3]);
            }
            bq[qt][ks] = v;
        }
        qn[qt] = s + __shfl_xor(s, 32, 64);     // |x'|^2: the lane's half plus lane ^ 32's
    }

    int lo, hi;
    voc_split_range(p.K, p.split, blockIdx.y, lo, hi);

    // one 16-byte chunk of a 32-centroid tile per thread (32 rows x 8 chunks = 256 threads) and the norm
    // of one row per thread of the first half-wave; the next tile's loads are in flight under the MFMAs
    const int srow = tid >> 3, sch = tid & 7;
    auto fetch = [&](int tb, uint4& u, int& tnv) {
        u = make_uint4(0, 0, 0, 0);
        if (tb + srow < hi) {
            u = *reinterpret_cast<const uint4*>(p.cent + (size_t)(tb + srow) * KB + sch * 16);
            u.x ^= xm; u.y ^= xm; u.z ^= xm; u.w ^= xm;
        }
        // the norm with the row's accumulator register j = (row & 3) + 4 (row >> 3) in its low 4 bits;
        // a padding row is all zero, so its key stays INT_MAX
        tnv = tid < 32 && tb + tid < hi ? (p.cnorm[tb + tid] << 4) | ((tid & 3) + 4 * (tid >> 3)) : INT_MAX;
    };
    uint4 pre = make_uint4(0, 0, 0, 0);
    int pre_tn = INT_MAX;
    if (lo < hi) fetch(lo, pre, pre_tn);

    // Per lane the 16 candidates of a tile are keys 16 (|c'|^2 - 2<x', c'>) + j (|.| < 2^27): their
    // minimum is the least distance and then the least register j, which is the least row.  A tile
    // replaces the lane's best only with a strictly smaller distance, so an earlier tile keeps a tie.
    int b1[2] = {INT_MAX, INT_MAX}, t1[2] = {0, 0};
    for (int tb = lo; tb < hi; tb += 32) {
        // stage the tile (16-byte chunks swizzled by the row) and its norms
        *reinterpret_cast<uint4*>(tile + srow * KB + ((sch ^ (srow & 7)) * 16)) = pre;
        if (tid < 32) tn_s[tid] = pre_tn;
        __syncthreads();
        if (tb + 32 < hi) fetch(tb + 32, pre, pre_tn);

        v16i acc[2];
#pragma unroll
        for (int qt = 0; qt < 2; qt++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[qt][r] = 0;
        const int arow = lane & 31;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            const int ch = 2 * ks + h;
            const v4i a = *reinterpret_cast<const v4i*>(tile + arow * KB + ((ch ^ (arow & 7)) * 16));
#pragma unroll
            for (int qt = 0; qt < 2; qt++) acc[qt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, bq[qt][ks], acc[qt], 0, 0, 0);
        }
        int tn[16];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int4 v = *reinterpret_cast<const int4*>(tn_s + 8 * g + 4 * h);
            tn[4 * g + 0] = v.x; tn[4 * g + 1] = v.y; tn[4 * g + 2] = v.z; tn[4 * g + 3] = v.w;
        }
#pragma unroll
        for (int qt = 0; qt < 2; qt++) {
            int m = INT_MAX;
#pragma unroll
            for (int j = 0; j < 16; j++) m = min(m, tn[j] - 32 * acc[qt][j]);     // 16 (d^2 - |x'|^2) + j
            const bool better = (m >> 4) < (b1[qt] >> 4);
            b1[qt] = better ? m : b1[qt];
            t1[qt] = better ? tb : t1[qt];
        }
        __syncthreads();
    }

#pragma unroll
    for (int qt = 0; qt < 2; qt++) {
        const int j = b1[qt] & 15;
        const int mine = b1[qt] == INT_MAX ? -1 : t1[qt] + (j & 3) + 8 * (j >> 2) + 4 * h;
        int e = b1[qt] >> 4, x = mine;
        const int ob = __shfl_xor(e, 32, 64), oi = __shfl_xor(x, 32, 64);
        if (voc_key_lt(ob, oi, e, x)) { e = ob; x = oi; }
        const int q = qbase + qt * 32 + (lane & 31);
        if (h == 0 && q < p.n) p.part[(size_t)blockIdx.y * p.n + q] = make_int2(x >= 0 ? e + qn[qt] : kVocNoDist, x);
    }
}

__device__ __forceinline__ int ham128(const uint4& a, const uint4& b)
{
    return __popc(a.x ^ b.x) + __popc(a.y ^ b.y) + __popc(a.z ^ b.z) + __popc(a.w ^ b.w);
}

// Grid as voc_assign_sift; one descriptor per lane, 64-centroid tiles read as LDS broadcasts.
__global__ __launch_bounds__(256) void voc_assign_orb(AssignParams p)
{
    __shared__ uint4 tile[64 * 2];
    const int tid = threadIdx.x;
    const int q = blockIdx.x * 256 + tid;
    uint4 x0 = make_uint4(0, 0, 0, 0), x1 = x0;
    if (q < p.n) {
        const uint4* d = reinterpret_cast<const uint4*>(p.desc + (size_t)q * 32);
        x0 = d[0];
        x1 = d[1];
    }
    int lo, hi;
    voc_split_range(p.K, p.split, blockIdx.y, lo, hi);
    int b1 = INT_MAX, i1 = -1;
    for (int tb = lo; tb < hi; tb += 64) {
        if (tid < 128) {
            const int row = tid >> 1;
            uint4 u = make_uint4(0, 0, 0, 0);
            if (tb + row < hi) u = reinterpret_cast<const uint4*>(p.cent + (size_t)(tb + row) * 32)[tid & 1];
            tile[tid] = u;
        }
        __syncthreads();
        const int nr = min(64, hi - tb);
        for (int r = 0; r < nr; r++) {
            const int d = ham128(x0, tile[2 * r]) + ham128(x1, tile[2 * r + 1]);
            if (d < b1) {
                b1 = d;
                i1 = tb + r;
            }
        }
        __syncthreads();
    }
    if (q < p.n) p.part[(size_t)blockIdx.y * p.n + q] = make_int2(i1 >= 0 ? b1 : kVocNoDist, i1);
}

// the winner over the splits by the full (dist, index) compare; count: the words' histogram (training)
__global__ __launch_bounds__(256) void voc_assign_finish(const int2* part, int n, int split, int32_t* word, int32_t* dist,
                                                         uint32_t* count)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int bd = kVocNoDist, bi = -1;
    for (int z = 0; z < split; z++) {
        const int2 v = part[(size_t)z * n + i];
        if (v.y >= 0 && voc_key_lt(v.x, v.y, bd, bi)) {
            bd = v.x;
            bi = v.y;
        }
    }
    word[i] = bi;
    dist[i] = bd;
    if (count && bi >= 0) atomicAdd(&count[bi], 1u);
}

// cent[c] = desc[floor(c N / K)], one thread per 4 bytes
__global__ __launch_bounds__(256) void voc_init(const uint8_t* desc, int n, int K, int words, uint32_t* cent)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K * words) return;
    const int c = i / words, w = i - c * words;
    const size_t row = (size_t)((long long)c * n / K);
    cent[i] = reinterpret_cast<const uint32_t*>(desc)[row * words + w];
}

// exclusive scan of the K <= 65536 counts by one workgroup: start and the scatter's cursors
__global__ __launch_bounds__(1024) void voc_scan(const uint32_t* count, int K, uint32_t* start, uint32_t* cursor)
{
    __shared__ uint32_t s[1024];
    const int tid = threadIdx.x;
    const int per = (K + 1023) / 1024;
    const int lo = min(K, tid * per), hi = min(K, lo + per);
    uint32_t sum = 0;
    for (int c = lo; c < hi; c++) sum += count[c];
    s[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const uint32_t v = tid >= off ? s[tid - off] : 0u;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    uint32_t run = s[tid] - sum;
    for (int c = lo; c < hi; c++) {
        start[c] = run;
        cursor[c] = run;
        run += count[c];
    }
}

__global__ __launch_bounds__(256) void voc_scatter(const int32_t* word, int n, int K, uint32_t* cursor, uint32_t* order)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int w = word[i];
    if ((unsigned)w >= (unsigned)K) return;
    const uint32_t pos = atomicAdd(&cursor[w], 1u);
    if (pos < (uint32_t)n) order[pos] = (uint32_t)i;
}

// One workgroup per centroid: 8 row groups x 32 lanes of 4 dimensions, reduced in LDS.
__global__ __launch_bounds__(256) void voc_update_sift(const uint8_t* desc, int n, const uint32_t* count,
                                                       const uint32_t* start, const uint32_t* order, uint8_t* cent,
                                                       int* changed)
{
    __shared__ uint32_t red[8][128];
    const int c = blockIdx.x, tid = threadIdx.x, g = tid >> 5, l = tid & 31;
    const uint32_t cnt = count[c];
    if (cnt == 0) return;       // an empty cluster keeps its centroid
    const uint32_t st = start[c];
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (uint32_t r = g; r < cnt; r += 8) {
        const uint32_t row = order[st + r];
        if (row >= (uint32_t)n) continue;
        const uint32_t w = reinterpret_cast<const uint32_t*>(desc + (size_t)row * 128)[l];
        s0 += w & 255u;
        s1 += (w >> 8) & 255u;
        s2 += (w >> 16) & 255u;
        s3 += w >> 24;
    }
    red[g][4 * l + 0] = s0;
    red[g][4 * l + 1] = s1;
    red[g][4 * l + 2] = s2;
    red[g][4 * l + 3] = s3;
    __syncthreads();
    int ch = 0;
    if (tid < 128) {
        uint32_t S = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) S += red[k][tid];
        const uint8_t nc = (uint8_t)voc_sift_mean(S, cnt);
        uint8_t* dst = cent + (size_t)c * 128 + tid;
        if (*dst != nc) {
            *dst = nc;
            ch = 1;
        }
    }
    if (__syncthreads_or(ch) && tid == 0) atomicOr(changed, 1);
}

// One workgroup per centroid, one thread per bit.
__global__ __launch_bounds__(256) void voc_update_orb(const uint8_t* desc, int n, const uint32_t* count,
                                                      const uint32_t* start, const uint32_t* order, uint8_t* cent,
                                                      int* changed)
{
    __shared__ uint32_t bits[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const uint32_t cnt = count[c];
    if (cnt == 0) return;
    const uint32_t st = start[c];
    uint32_t ones = 0;
    for (uint32_t r = 0; r < cnt; r++) {
        const uint32_t row = order[st + r];
        if (row >= (uint32_t)n) continue;
        ones += (desc[(size_t)row * 32 + (tid >> 3)] >> (tid & 7)) & 1u;
    }
    bits[tid] = voc_orb_bit(ones, cnt);
    __syncthreads();
    int ch = 0;
    if (tid < 32) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 8; b++) v |= bits[8 * tid + b] << b;
        uint8_t* dst = cent + (size_t)c * 32 + tid;
        if (*dst != (uint8_t)v) {
            *dst = (uint8_t)v;
            ch = 1;
        }
    }
    if (__syncthreads_or(ch) && tid == 0) atomicOr(changed, 1);
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// v = h w and A = sum v of one image from its counts `h` (LDS or the row of vec itself);
// scratch: 4 u64 of LDS that nothing else uses after the barrier
__device__ __forceinline__ void bow_weight_row(const uint32_t* h, const int32_t* weights, int K, uint32_t* vrow, u64* total,
                                               u64* scratch)
{
    const int tid = threadIdx.x;
    u64 a = 0;
    for (int k = tid; k < K; k += 256) {
        const uint32_t v = h[k] * (uint32_t)weights[k];
        vrow[k] = v;
        a += v;
    }
    a = wave_sum_u64(a);
    __syncthreads();        // every read of h is done: its space may hold the wave sums
    if ((tid & 63) == 0) scratch[tid >> 6] = a;
    __syncthreads();
    if (tid == 0) *total = scratch[0] + scratch[1] + scratch[2] + scratch[3];
}

// One workgroup per image, the histogram in 4 K bytes of LDS (K <= 16384).
__global__ __launch_bounds__(256) void bow_hist_lds(const int32_t* word, const int32_t* offsets, const int32_t* weights,
                                                    int K, uint32_t* vec, u64* total)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t hs[];     // max(K, 8) words
    const int r = blockIdx.x, tid = threadIdx.x;
    const int lo = offsets[r], hi = offsets[r + 1];
    for (int k = tid; k < K; k += 256) hs[k] = 0;
    __syncthreads();
    for (int i = lo + tid; i < hi; i += 256) {
        const int w = word[i];
        if ((unsigned)w < (unsigned)K) atomicAdd(&hs[w], 1u);
    }
    __syncthreads();
    bow_weight_row(hs, weights, K, vec + (size_t)r * K, total + r, reinterpret_cast<u64*>(hs));
}

// K > 16384: counts by global atomics into the zeroed rows of vec, then the weights in place.
__global__ __launch_bounds__(256) void bow_count_global(const int32_t* word, const int32_t* offsets, int K, uint32_t* vec)
{
    const int r = blockIdx.x;
    const int lo = offsets[r], hi = offsets[r + 1];
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        const int w = word[i];
        if ((unsigned)w < (unsigned)K) atomicAdd(&vec[(size_t)r * K + w], 1u);
    }
}

__global__ __launch_bounds__(256) void bow_weight_global(const int32_t* weights, int K, uint32_t* vec, u64* total)
{
    __shared__ u64 scratch[4];
    const int r = blockIdx.x;
    bow_weight_row(vec + (size_t)r * K, weights, K, vec + (size_t)r * K, total + r, scratch);
}

constexpr int kScoreRows = 8;       // database rows per workgroup, two per wave
constexpr int kScoreQT = 8;         // queries scored per pass over a row

// Grid: x = 8 database rows, y = a tile of QT <= NQ queries.  LDSQ: the tile's vectors sit in
// LDS (QT K words <= 64 KB); otherwise (K > 16384) they are read through the caches.  A wave
// streams one row at a time, int64 sums, one division.  vec (K % 4 == 0 and 16-byte aligned
// bases): lanes load 16 bytes, four loads in flight each; otherwise dword loads.
template <bool LDSQ, int NQ>
__global__ __launch_bounds__(256) void bow_score_k(const uint32_t* q, const u64* qtot, int nq, const uint32_t* db,
                                                   const u64* dbtot, int m, int K, int QT, int vec, double* scores)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t qs[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.y * QT;
    const int nqt = min(QT, nq - q0);
    const uint32_t* qg = q + (size_t)q0 * K;
    if (LDSQ) {
        if (vec)
            for (int i = tid; i < nqt * (K >> 2); i += 256)
                reinterpret_cast<uint4*>(qs)[i] = reinterpret_cast<const uint4*>(qg)[i];
        else
            for (int i = tid; i < nqt * K; i += 256) qs[i] = qg[i];
        __syncthreads();
    }
    u64 At[NQ];
#pragma unroll
    for (int qi = 0; qi < NQ; qi++) At[qi] = qi < nqt ? qtot[q0 + qi] : 0;

    for (int rr = wave; rr < kScoreRows; rr += 4) {
        const int r = blockIdx.x * kScoreRows + rr;
        if (r >= m) break;
        const u64 Bt = dbtot[r];
        const uint32_t* brow = db + (size_t)r * K;
        u64 num[NQ];
#pragma unroll
        for (int qi = 0; qi < NQ; qi++) num[qi] = 0;
        if (vec) {
            const uint4* b4 = reinterpret_cast<const uint4*>(brow);
            const int K4 = K >> 2;
            for (int k0 = lane; k0 < K4; k0 += 256) {
                uint4 bv[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int kk = k0 + 64 * u;
                    bv[u] = kk < K4 ? b4[kk] : make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int kk = min(k0 + 64 * u, K4 - 1);     // past the row: b = 0 adds nothing
#pragma unroll
                    for (int qi = 0; qi < NQ; qi++)
                        if (NQ == 1 || qi < nqt) {
                            const uint4 a = LDSQ ? reinterpret_cast<const uint4*>(qs + qi * K)[kk]
                                                 : reinterpret_cast<const uint4*>(qg + (size_t)qi * K)[kk];
                            num[qi] += (u64)bow_term(a.x, At[qi], bv[u].x, Bt) + (u64)bow_term(a.y, At[qi], bv[u].y, Bt) +
                                       (u64)bow_term(a.z, At[qi], bv[u].z, Bt) + (u64)bow_term(a.w, At[qi], bv[u].w, Bt);
                        }
                }
            }
        } else {
            for (int k = lane; k < K; k += 64) {
                const uint32_t b = brow[k];
#pragma unroll
                for (int qi = 0; qi < NQ; qi++)
                    if (NQ == 1 || qi < nqt) {
                        const uint32_t a = LDSQ ? qs[qi * K + k] : qg[(size_t)qi * K + k];
                        num[qi] += (u64)bow_term(a, At[qi], b, Bt);
                    }
            }
        }
#pragma unroll
        for (int qi = 0; qi < NQ; qi++)
            if (NQ == 1 || qi < nqt) {
                const u64 s = wave_sum_u64(num[qi]);
                if (lane == 0) scores[(size_t)(q0 + qi) * m + r] = bow_score_div((int64_t)s, At[qi], Bt);
            }
    }
}

// One wave per query: round t picks the best row of [first, last) that ranks after round t - 1's.
__global__ __launch_bounds__(64) void bow_topk_k(const double* scores, int m, int first, int last, int k, int32_t* idx,
                                                 double* out)
{
    const int qi = blockIdx.x, lane = threadIdx.x;
    const double* s = scores + (size_t)qi * m;
    double ps = 0.0;
    int pi = -1;
    bool have = false;      // a previous pick exists
    for (int t = 0; t < k; t++) {
        double bs = 0.0;
        int bi = -1;
        for (int i0 = first + lane; i0 < last; i0 += 256) {
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = i0 + 64 * u < last ? s[i0 + 64 * u] : 0.0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int i = i0 + 64 * u;
                const bool ok = i < last && (!have || bow_rank_before(ps, pi, v[u], i)) &&
                                (bi < 0 || bow_rank_before(v[u], i, bs, bi));
                bs = ok ? v[u] : bs;
                bi = ok ? i : bi;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double os = __shfl_xor(bs, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (oi >= 0 && (bi < 0 || bow_rank_before(os, oi, bs, bi))) {
                bs = os;
                bi = oi;
            }
        }
        if (lane == 0) {
            idx[(size_t)qi * k + t] = bi;
            out[(size_t)qi * k + t] = bi >= 0 ? bs : 0.0;
        }
        if (bi >= 0) {
            ps = bs;
            pi = bi;
            have = true;
        } else {
            // the window is used up: nothing ranks after the last pick in later rounds either
            ps = -1.0;
            pi = INT_MAX;
            have = true;
        }
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int assign_split(const slam_ctx* c, int n, int K)
{
    const int nblk = (n + 255) / 256;
    const int want = (2 * c->cu_count + nblk - 1) / nblk;
    return std::max(1, std::min({want, (K + 31) / 32, 64}));
}

// word / dist of n descriptors; count (optional, zeroed here): the histogram of the words
int launch_assign(slam_ctx* c, hipStream_t s, const uint8_t* d_desc, int n, const uint8_t* d_cent, int K, int kind,
                  int32_t* d_word, int32_t* d_dist, uint32_t* d_count)
{
    const int split = assign_split(c, n, K);
    SLAM_HIP(c, c->place_part.ensure(sizeof(int2) * (size_t)split * n));
    AssignParams p;
    p.desc = d_desc;
    p.n = n;
    p.cent = d_cent;
    p.cnorm = nullptr;
    p.K = K;
    p.split = split;
    p.part = c->place_part.as<int2>();
    const dim3 grid((n + 255) / 256, split);
    if (kind == kVocSift) {
        SLAM_HIP(c, c->place_norm.ensure(sizeof(int) * (size_t)K));
        p.cnorm = c->place_norm.as<int>();
        hipLaunchKernelGGL(voc_cent_norm, dim3((K + 255) / 256), dim3(256), 0, s, d_cent, K, c->place_norm.as<int>());
        hipLaunchKernelGGL(voc_assign_sift, grid, dim3(256), 0, s, p);
    } else {
        hipLaunchKernelGGL(voc_assign_orb, grid, dim3(256), 0, s, p);
    }
    if (d_count) SLAM_HIP(c, hipMemsetAsync(d_count, 0, sizeof(uint32_t) * (size_t)K, s));
    hipLaunchKernelGGL(voc_assign_finish, dim3((n + 255) / 256), dim3(256), 0, s, p.part, n, split, d_word, d_dist, d_count);
    SLAM_HIP(c, hipGetLastError());
    return SLAM_OK;
}

}  // namespace

}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_voc_assign_dev(slam_ctx* c, void* stream, const uint8_t* d_desc, int n, const uint8_t* d_cent, int K,
                                   int kind, int32_t* d_word, int32_t* d_dist)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (place_check_assign(d_desc, n, d_cent, K, kind) || !aligned16(d_desc) || !aligned16(d_cent))
        return set_err(c, SLAM_E_INVALID_ARG, "voc assign: kind 0 / 1, 0 <= n <= 2^24, 1 <= K <= 65536, 16-byte aligned rows");
    if (n == 0) return SLAM_OK;
    if (!d_word || !d_dist) return set_err(c, SLAM_E_INVALID_ARG, "voc assign: null output");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if (int rc = launch_assign(c, s, d_desc, n, d_cent, K, kind, d_word, d_dist, nullptr)) return rc;
    return stream_sync(c, s);
}

extern "C" int slam_voc_train_dev(slam_ctx* c, void* stream, const uint8_t* d_desc, int n, int K, int iters, int kind,
                                  uint8_t* d_cent, int32_t* iters_run)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (place_check_train(d_desc, n, K, iters, kind, d_cent, iters_run) || !aligned16(d_desc) || !aligned16(d_cent))
        return set_err(c, SLAM_E_INVALID_ARG, "voc train: kind 0 / 1, 1 <= n <= 2^24, 1 <= K <= 65536, iters >= 0, "
                                              "16-byte aligned rows");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    const int B = voc_desc_bytes(kind);
    // words + distances + the sorted order; counts, starts, cursors and the changed flag
    SLAM_HIP(c, c->place_word.ensure(sizeof(int32_t) * 3 * (size_t)n));
    SLAM_HIP(c, c->place_cnt.ensure(sizeof(uint32_t) * (3 * (size_t)K + 1)));
    int32_t* word = c->place_word.as<int32_t>();
    int32_t* dist = word + n;
    uint32_t* order = reinterpret_cast<uint32_t*>(word + 2 * (size_t)n);
    uint32_t* count = c->place_cnt.as<uint32_t>();
    uint32_t *start = count + K, *cursor = count + 2 * (size_t)K;
    int* flag = reinterpret_cast<int*>(count + 3 * (size_t)K);
    int* h_flag = static_cast<int*>(readback(c, sizeof(int)));
    if (!h_flag) return set_err(c, SLAM_E_HIP, "voc train: no pinned readback space");

    hipLaunchKernelGGL(voc_init, dim3((K * (B / 4) + 255) / 256), dim3(256), 0, s, d_desc, n, K, B / 4,
                       reinterpret_cast<uint32_t*>(d_cent));
    SLAM_HIP(c, hipGetLastError());
    int it = 0;
    while (it < iters) {
        if (int rc = launch_assign(c, s, d_desc, n, d_cent, K, kind, word, dist, count)) return rc;
        SLAM_HIP(c, hipMemsetAsync(flag, 0, sizeof(int), s));
        hipLaunchKernelGGL(voc_scan, dim3(1), dim3(1024), 0, s, count, K, start, cursor);
        hipLaunchKernelGGL(voc_scatter, dim3((n + 255) / 256), dim3(256), 0, s, word, n, K, cursor, order);
        if (kind == kVocSift)
            hipLaunchKernelGGL(voc_update_sift, dim3(K), dim3(256), 0, s, d_desc, n, count, start, order, d_cent, flag);
        else
            hipLaunchKernelGGL(voc_update_orb, dim3(K), dim3(256), 0, s, d_desc, n, count, start, order, d_cent, flag);
        SLAM_HIP(c, hipGetLastError());
        SLAM_HIP(c, hipMemcpyAsync(h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s));
        if (int rc = stream_sync(c, s)) return rc;
        it++;
        if (!*h_flag) break;
    }
    *iters_run = it;
    return stream_sync(c, s);
}

extern "C" int slam_bow_vectors_dev(slam_ctx* c, void* stream, const int32_t* d_word, const int32_t* offsets, int m,
                                    const int32_t* weights, int K, uint32_t* d_vec, uint64_t* d_total)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (place_check_vectors(offsets, m, weights, K))
        return set_err(c, SLAM_E_INVALID_ARG, "bow vectors: 1 <= K <= 65536, offsets ascending with at most 65535 "
                                              "descriptors per image, weights in [0, 1023]");
    if (m == 0) return SLAM_OK;
    if (!d_vec || !d_total || (offsets[m] > offsets[0] && !d_word))
        return set_err(c, SLAM_E_INVALID_ARG, "bow vectors: null argument");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    SLAM_HIP(c, c->place_par.ensure(sizeof(int32_t) * ((size_t)m + 1 + K)));
    int32_t* d_off = c->place_par.as<int32_t>();
    int32_t* d_w = d_off + m + 1;
    SLAM_HIP(c, hipMemcpyAsync(d_off, offsets, sizeof(int32_t) * ((size_t)m + 1), hipMemcpyHostToDevice, s));
    SLAM_HIP(c, hipMemcpyAsync(d_w, weights, sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, s));
    u64* tot = reinterpret_cast<u64*>(d_total);
    if (K <= 16384) {
        hipLaunchKernelGGL(bow_hist_lds, dim3(m), dim3(256), sizeof(uint32_t) * (size_t)std::max(K, 8), s, d_word, d_off, d_w,
                           K, d_vec, tot);
    } else {
        SLAM_HIP(c, hipMemsetAsync(d_vec, 0, sizeof(uint32_t) * (size_t)m * K, s));
        hipLaunchKernelGGL(bow_count_global, dim3(m), dim3(256), 0, s, d_word, d_off, K, d_vec);
        hipLaunchKernelGGL(bow_weight_global, dim3(m), dim3(256), 0, s, d_w, K, d_vec, tot);
    }
    SLAM_HIP(c, hipGetLastError());
    return stream_sync(c, s);
}

extern "C" int slam_bow_score_dev(slam_ctx* c, void* stream, const uint32_t* d_q, const uint64_t* d_qtotal, int nq,
                                  const uint32_t* d_db, const uint64_t* d_dbtotal, int m, int K, double* d_scores)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (place_check_score(nq, m, K)) return set_err(c, SLAM_E_INVALID_ARG, "bow score: nq, m >= 0 and 1 <= K <= 65536");
    if (nq == 0 || m == 0) return SLAM_OK;
    if (!d_q || !d_qtotal || !d_db || !d_dbtotal || !d_scores) return set_err(c, SLAM_E_INVALID_ARG, "bow score: null argument");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    const u64* qt = reinterpret_cast<const u64*>(d_qtotal);
    const u64* bt = reinterpret_cast<const u64*>(d_dbtotal);
    const int gx = (m + kScoreRows - 1) / kScoreRows;
    const int vec = (K & 3) == 0 && aligned16(d_q) && aligned16(d_db);
    const bool lds = K <= 16384;
    const int QT = nq == 1 ? 1 : lds ? std::min(kScoreQT, 16384 / K) : kScoreQT;
    const dim3 grid(gx, (nq + QT - 1) / QT);
    const size_t shm = lds ? sizeof(uint32_t) * (size_t)QT * K : 0;
    if (lds && QT == 1)
        hipLaunchKernelGGL((bow_score_k<true, 1>), grid, dim3(256), shm, s, d_q, qt, nq, d_db, bt, m, K, QT, vec, d_scores);
    else if (lds)
        hipLaunchKernelGGL((bow_score_k<true, kScoreQT>), grid, dim3(256), shm, s, d_q, qt, nq, d_db, bt, m, K, QT, vec, d_scores);
    else if (QT == 1)
        hipLaunchKernelGGL((bow_score_k<false, 1>), grid, dim3(256), shm, s, d_q, qt, nq, d_db, bt, m, K, QT, vec, d_scores);
    else
        hipLaunchKernelGGL((bow_score_k<false, kScoreQT>), grid, dim3(256), shm, s, d_q, qt, nq, d_db, bt, m, K, QT, vec, d_scores);
    SLAM_HIP(c, hipGetLastError());
    return stream_sync(c, s);
}

extern "C" int slam_bow_topk_dev(slam_ctx* c, void* stream, const double* d_scores, int nq, int m, int first, int last,
                                 int k, int32_t* d_idx, double* d_score)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (place_check_topk(nq, m, first, last, k))
        return set_err(c, SLAM_E_INVALID_ARG, "bow topk: 0 <= first <= last <= m and 1 <= k <= 32");
    if (nq == 0) return SLAM_OK;
    if (!d_idx || !d_score || (last > first && !d_scores)) return set_err(c, SLAM_E_INVALID_ARG, "bow topk: null argument");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    hipLaunchKernelGGL(bow_topk_k, dim3(nq), dim3(64), 0, s, d_scores, m, first, last, k, d_idx, d_score);
    SLAM_HIP(c, hipGetLastError());
    return stream_sync(c, s);
}

// ---- host-buffer wrappers: stage, run the device entry points, copy back ----

extern "C" int slam_voc_assign(slam_ctx* c, const uint8_t* desc, int n, const uint8_t* cent, int K, int kind,
                               int32_t* word, int32_t* dist)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (place_check_assign(desc, n, cent, K, kind)) return set_err(c, SLAM_E_INVALID_ARG, "voc assign: bad arguments");
    if (n == 0) return SLAM_OK;
    if (!word || !dist) return set_err(c, SLAM_E_INVALID_ARG, "voc assign: null output");
    SLAM_HIP(c, hipSetDevice(c->device));
    const size_t B = voc_desc_bytes(kind);
    DevLayout lay;
    const auto s_desc = lay.add<uint8_t>(n * B), s_cent = lay.add<uint8_t>(K * B);
    const auto s_word = lay.add<int32_t>((size_t)n), s_dist = lay.add<int32_t>((size_t)n);
    DevMem d;
    SLAM_HIP(c, d.bind(c->place_in, lay));
    SLAM_HIP(c, d.upload(s_desc, desc, c->stream));
    SLAM_HIP(c, d.upload(s_cent, cent, c->stream));
    if (int rc = slam_voc_assign_dev(c, c->stream, d.ptr(s_desc), n, d.ptr(s_cent), K, kind, d.ptr(s_word), d.ptr(s_dist)))
        return rc;
    SLAM_HIP(c, d.download(word, s_word, c->stream));
    SLAM_HIP(c, d.download(dist, s_dist, c->stream));
    return stream_sync(c, c->stream);
}

extern "C" int slam_voc_train(slam_ctx* c, const uint8_t* desc, int n, int K, int iters, int kind, uint8_t* cent,
                              int32_t* iters_run)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (place_check_train(desc, n, K, iters, kind, cent, iters_run)) return set_err(c, SLAM_E_INVALID_ARG, "voc train: bad arguments");
    SLAM_HIP(c, hipSetDevice(c->device));
    const size_t B = voc_desc_bytes(kind);
    DevLayout lay;
    const auto s_desc = lay.add<uint8_t>(n * B), s_cent = lay.add<uint8_t>(K * B);
    DevMem d;
    SLAM_HIP(c, d.bind(c->place_in, lay));
    SLAM_HIP(c, d.upload(s_desc, desc, c->stream));
    if (int rc = slam_voc_train_dev(c, c->stream, d.ptr(s_desc), n, K, iters, kind, d.ptr(s_cent), iters_run)) return rc;
    SLAM_HIP(c, d.download(cent, s_cent, c->stream));
    return stream_sync(c, c->stream);
}

extern "C" int slam_bow_vectors(slam_ctx* c, const int32_t* word, const int32_t* offsets, int m, const int32_t* weights,
                                int K, uint32_t* vec, uint64_t* total)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (place_check_vectors(offsets, m, weights, K)) return set_err(c, SLAM_E_INVALID_ARG, "bow vectors: bad arguments");
    if (m == 0) return SLAM_OK;
    const int32_t w0 = offsets[0], nw = offsets[m] - offsets[0];
    if (!vec || !total || (nw > 0 && !word)) return set_err(c, SLAM_E_INVALID_ARG, "bow vectors: null argument");
    for (int i = 0; i < nw; i++)
        if (word[w0 + i] < 0 || word[w0 + i] >= K) return set_err(c, SLAM_E_INVALID_ARG, "bow vectors: word outside [0, K)");
    SLAM_HIP(c, hipSetDevice(c->device));
    std::vector<int32_t> off((size_t)m + 1);
    for (int i = 0; i <= m; i++) off[i] = offsets[i] - w0;
    DevLayout lay;
    const auto s_word = lay.add<int32_t>((size_t)nw);
    const auto s_vec = lay.add<uint32_t>((size_t)m * K);
    const auto s_tot = lay.add<uint64_t>((size_t)m);
    DevMem d;
    SLAM_HIP(c, d.bind(c->place_in, lay));
    if (nw > 0) SLAM_HIP(c, d.upload(s_word, word + w0, c->stream));
    if (int rc = slam_bow_vectors_dev(c, c->stream, d.ptr(s_word), off.data(), m, weights, K, d.ptr(s_vec), d.ptr(s_tot)))
        return rc;
    SLAM_HIP(c, d.download(vec, s_vec, c->stream));
    SLAM_HIP(c, d.download(total, s_tot, c->stream));
    return stream_sync(c, c->stream);
}

extern "C" int slam_bow_query(slam_ctx* c, const uint32_t* q, const uint64_t* qtotal, int nq, const uint32_t* db,
                              const uint64_t* dbtotal, int m, int K, int first, int last, int k, int32_t* idx,
                              double* score)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (place_check_score(nq, m, K) || place_check_topk(nq, m, first, last, k))
        return set_err(c, SLAM_E_INVALID_ARG, "bow query: bad arguments");
    if (nq == 0) return SLAM_OK;
    if (!q || !qtotal || !idx || !score || (m > 0 && (!db || !dbtotal))) return set_err(c, SLAM_E_INVALID_ARG, "bow query: null argument");
    SLAM_HIP(c, hipSetDevice(c->device));
    const size_t Q = (size_t)nq, M = (size_t)m;
    DevLayout lay;
    const auto s_qt = lay.add<uint64_t>(Q), s_bt = lay.add<uint64_t>(M);
    const auto s_sc = lay.add<double>(Q * M), s_out = lay.add<double>(Q * k);
    const auto s_q = lay.add<uint32_t>(Q * K), s_db = lay.add<uint32_t>(M * K);
    const auto s_idx = lay.add<int32_t>(Q * k);
    DevMem d;
    SLAM_HIP(c, d.bind(c->place_in, lay));
    hipStream_t s = c->stream;
    SLAM_HIP(c, d.upload(s_qt, qtotal, s));
    SLAM_HIP(c, d.upload(s_q, q, s));
    if (m > 0) {
        SLAM_HIP(c, d.upload(s_bt, dbtotal, s));
        SLAM_HIP(c, d.upload(s_db, db, s));
    }
    if (int rc = slam_bow_score_dev(c, s, d.ptr(s_q), d.ptr(s_qt), nq, d.ptr(s_db), d.ptr(s_bt), m, K, d.ptr(s_sc))) return rc;
    if (int rc = slam_bow_topk_dev(c, s, d.ptr(s_sc), nq, m, first, last, k, d.ptr(s_idx), d.ptr(s_out))) return rc;
    SLAM_HIP(c, d.download(idx, s_idx, s));
    SLAM_HIP(c, d.download(score, s_out, s));
    return stream_sync(c, s);
}

// Baseline JPEG encoding on gfx950 (cv::imencode / cv::imwrite).
//
// A batch of resident frames of one size becomes n streams in one set of launches.
// Huffman encoding has no serial dependency once every quantised DC is known: the
// stream is lengths, then prefix sums, then a pack.
//
//   jpeg_enc_dct        eight lanes per block: colour conversion, the edge rules and
//                       the downsampling happen on the load (jpeg_enc_math.h), each
//                       lane transforms one row, the block is transposed through
//                       LDS, each lane transforms and quantises one column, and the
//                       int16 coefficients go out in zigzag order, blocks in scan
//                       order (MCU-interleaved); dummy blocks are not written
//   jpeg_enc_count      one lane per MCU: its bit length (dummy-block rule, restart
//                       reset), scanned over the workgroup's 256 MCUs
//   jpeg_enc_scan_tiles one workgroup per image: the exclusive scan of the tile sums
//   jpeg_enc_intervals  one lane per restart interval: its bytes (intervals are
//                       byte-aligned), scanned the same way
//   jpeg_enc_pack       one lane per MCU writes its bits into the zeroed, unstuffed
//                       stream: whole words are plain stores, the boundary words
//                       atomicOr (commutative: the bytes do not depend on scheduling)
//   jpeg_enc_ffcount    one lane per 256-byte chunk counts its FF bytes, scanned
//   jpeg_enc_write      one lane per chunk writes the final bytes: header, stuffed
//                       scan, RSTn between intervals, EOI, the size and the status
//
// The host reads back the unstuffed length of every image once, between the
// interval scan and the pack (the buffer and the grids of the last three kernels
// are sized by it).  No workgroup waits on another inside a kernel; every loop is
// bounded by a constant or by a uniform kernel argument.  Nothing is written at or
// past an image's capacity.
#include <cstring>

#include "jpeg_enc_host.h"
#include "slamhip_internal.h"

namespace slamhip {

namespace {

using jpeg::EncGeom;
using jpeg::EncTables;

constexpr int kDctBlocks = 32;      // blocks per workgroup of jpeg_enc_dct (8 lanes each)
constexpr int kDctRow = 9;          // LDS words per row of a block: 8 + 1
constexpr int kDctPitch = 72;       // LDS words per block: lane (slot, j) of a wave touches bank 8 slot + 9 j + i (row pass)
                                    // or 8 slot + j + 9 r (column pass), distinct over the wave's 64 lanes
constexpr int kTile = 256;          // lanes of the scanning kernels: a tile of MCUs, intervals or chunks
constexpr uint32_t kChunk = 256;    // bytes of the unstuffed stream per lane of the stuffing pass

struct EncParams {
    EncGeom g;
    EncTables T;
    uint32_t hdr_len;
    uint8_t hdr[jpeg::kEncHeaderMax];
};
static_assert(sizeof(EncTables) % 4 == 0, "tables are copied as words");

__global__ void __launch_bounds__(kDctBlocks * 8) jpeg_enc_dct(const EncParams* __restrict__ P,
                                                               const uint8_t* __restrict__ frames,
                                                               int16_t* __restrict__ coef)
{
    __shared__ int ws[kDctBlocks * kDctPitch];
    __shared__ alignas(16) int16_t zs[kDctBlocks * 64];
    __shared__ uint8_t inv[64];      // natural position -> zigzag position
    const EncGeom& g = P->g;
    const uint32_t nblk = g.nmcu * (uint32_t)g.bpm;
    const int slot = (int)threadIdx.x >> 3, j = (int)threadIdx.x & 7;
    const uint32_t blk = (uint32_t)blockIdx.x * kDctBlocks + (uint32_t)slot;
    if (threadIdx.x < 64) inv[jpeg::zigzag_natural((int)threadIdx.x)] = (uint8_t)threadIdx.x;
    bool real = false;
    int c = 0;
    if (blk < nblk) {
        const uint32_t m = blk / (uint32_t)g.bpm;
        const int k = (int)(blk % (uint32_t)g.bpm);
        int col, row;
        real = jpeg::enc_block_pos(g, k, (int)(m % (uint32_t)g.mcux), (int)(m / (uint32_t)g.mcux), c, col, row);
        if (real) {
            int d[8];
            jpeg::enc_block_row(frames + (uint64_t)blockIdx.y * g.frame_step, g, c, col, row, j, d);
#pragma unroll
            for (int i = 0; i < 8; i++) ws[slot * kDctPitch + j * kDctRow + i] = d[i];
        }
    }
    __syncthreads();
    if (real) {
        int d[8];
#pragma unroll
        for (int r = 0; r < 8; r++) d[r] = ws[slot * kDctPitch + r * kDctRow + j];
        jpeg::enc_fdct_pass(d, true);
        const uint16_t* q = P->T.quant[c ? 1 : 0];
#pragma unroll
        for (int r = 0; r < 8; r++) zs[slot * 64 + inv[r * 8 + j]] = (int16_t)jpeg::enc_quant(d[r], q[r * 8 + j]);
    }
    __syncthreads();
    if (real) {      // 16 bytes per lane: blocks are 128 bytes, the buffer is 256-byte aligned
        int16_t* dst = coef + ((uint64_t)blockIdx.y * nblk + blk) * 64u + (uint32_t)j * 8u;
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(zs + slot * 64 + j * 8);
    }
}

// exclusive scan of v over the workgroup's kTile lanes; total: the sum.  Every lane calls it.
__device__ inline uint64_t tile_scan(uint64_t v, uint64_t* sh, uint64_t& total)
{
    const int lane = (int)threadIdx.x;
    __syncthreads();      // the scan before is read
    sh[lane] = v;
    __syncthreads();
    for (int d = 1; d < kTile; d <<= 1) {
        const uint64_t add = lane >= d ? sh[lane - d] : 0;
        __syncthreads();
        sh[lane] += add;
        __syncthreads();
    }
    total = sh[kTile - 1];
    return sh[lane] - v;
}

__device__ inline void stage_tables(EncTables* dst, const EncParams* P)
{
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&P->T);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (int i = (int)threadIdx.x; i < (int)(sizeof(EncTables) / 4); i += kTile) d[i] = src[i];
    __syncthreads();
}

// what the kernels after the scans read: bit offsets of MCUs and byte offsets of intervals
struct EncScans {
    const uint32_t* mcu_pre;      // n x nmcu: bits of the tile's MCUs before this one
    const uint64_t* tile_a;       // n x nta: bits of the image's tiles before this one
    const uint64_t* total_a;      // n
    const uint64_t* int_pre;      // n x nint, bytes
    const uint64_t* tile_b;       // n x ntb
    const uint64_t* total_b;      // n: the unstuffed bytes of the image
    uint32_t nta, ntb;
};

__device__ inline uint64_t mcu_bit(const EncScans& S, const EncGeom& g, uint32_t img, uint32_t m)
{
    if (m >= g.nmcu) return S.total_a[img];
    return S.tile_a[(uint64_t)img * S.nta + m / kTile] + S.mcu_pre[(uint64_t)img * g.nmcu + m];
}

__device__ inline uint64_t interval_byte(const EncScans& S, const EncGeom& g, uint32_t img, uint32_t i)
{
    if (i >= g.nint) return S.total_b[img];
    return S.tile_b[(uint64_t)img * S.ntb + i / kTile] + S.int_pre[(uint64_t)img * g.nint + i];
}

// One lane per MCU walks its blocks serially and neighbouring lanes are bpm x 128 bytes apart: the loads do
// not coalesce.  Measured: this kernel and jpeg_enc_pack, which reads the same way,
// are 45 % and 36 % of a 210 x 1080p call (10.4 and 8.2 of 23 ms).
__global__ void __launch_bounds__(kTile) jpeg_enc_count(const EncParams* __restrict__ P, const int16_t* __restrict__ coef,
                                                        uint32_t* __restrict__ mcu_pre, uint64_t* __restrict__ tile_a,
                                                        int32_t* __restrict__ status)
{
    __shared__ EncTables T;
    __shared__ uint64_t sh[kTile];
    const EncGeom& g = P->g;
    stage_tables(&T, P);
    const uint32_t m = (uint32_t)blockIdx.x * kTile + threadIdx.x, img = blockIdx.y;
    uint64_t bits = 0;
    if (m < g.nmcu) {
        const int16_t* ci = coef + (uint64_t)img * g.nmcu * (uint64_t)g.bpm * 64u;
        int pred[3];
        jpeg::enc_mcu_pred(g, m, ci, pred);
        jpeg::EncCountSink s;
        const int st = jpeg::enc_mcu(s, g, T, m, ci + (uint64_t)m * (uint64_t)g.bpm * 64u, pred);
        if (st) atomicOr(&status[img], st);
        bits = s.bits;
    }
    uint64_t total;
    const uint64_t ex = tile_scan(bits, sh, total);
    if (m < g.nmcu) mcu_pre[(uint64_t)img * g.nmcu + m] = (uint32_t)ex;      // 256 MCUs of 6 blocks of 1660 bits at the most
    if (threadIdx.x == 0) tile_a[(uint64_t)img * gridDim.x + blockIdx.x] = total;
}

// tiles: n x ntiles sums, replaced by their exclusive scan per image; totals: n
__global__ void __launch_bounds__(kTile) jpeg_enc_scan_tiles(uint64_t* __restrict__ tiles, uint32_t ntiles,
                                                             uint64_t* __restrict__ totals)
{
    __shared__ uint64_t sh[kTile];
    uint64_t* t = tiles + (uint64_t)blockIdx.x * ntiles;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < ntiles; base += kTile) {
        const uint32_t k = base + threadIdx.x;
        const uint64_t v = k < ntiles ? t[k] : 0;
        uint64_t total;
        const uint64_t ex = tile_scan(v, sh, total);
        if (k < ntiles) t[k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kTile) jpeg_enc_intervals(const EncParams* __restrict__ P, EncScans S,
                                                            uint64_t* __restrict__ int_pre, uint64_t* __restrict__ tile_b)
{
    __shared__ uint64_t sh[kTile];
    const EncGeom& g = P->g;
    const uint32_t i = (uint32_t)blockIdx.x * kTile + threadIdx.x, img = blockIdx.y;
    uint64_t bytes = 0;
    if (i < g.nint) {
        const uint64_t m0 = (uint64_t)i * g.ri, m1 = m0 + g.ri < g.nmcu ? m0 + g.ri : g.nmcu;
        bytes = (mcu_bit(S, g, img, (uint32_t)m1) - mcu_bit(S, g, img, (uint32_t)m0) + 7u) >> 3;
    }
    uint64_t total;
    const uint64_t ex = tile_scan(bytes, sh, total);
    if (i < g.nint) int_pre[(uint64_t)img * g.nint + i] = ex;
    if (threadIdx.x == 0) tile_b[(uint64_t)img * gridDim.x + blockIdx.x] = total;
}

// Bits, most significant first, into 32-bit words of a zeroed buffer.  The first and the last word
// of a lane may be shared with its neighbours: atomicOr; the words between are its own.
struct PackSink {
    uint32_t* words;
    uint64_t wi, wlimit;      // the next word; words of the image's region
    uint64_t acc = 0;
    int n;                    // bits of the next word that are decided (those before the lane's first are left zero)
    bool first = true;
    __device__ PackSink(uint32_t* w, uint64_t bit, uint64_t limit) : words(w), wi(bit >> 5), wlimit(limit), n((int)(bit & 31)) {}
    __device__ void word(uint32_t v, bool shared)
    {
        v = __builtin_bswap32(v);
        if (wi < wlimit) {
            if (shared) atomicOr(&words[wi], v);
            else words[wi] = v;
        }
        wi++;
        first = false;
    }
    __device__ void put(uint32_t code, int len)
    {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            word((uint32_t)(acc >> (n - 32)), first);
            n -= 32;
            acc &= (1ull << n) - 1ull;
        }
    }
    __device__ void finish()
    {
        if (n) word((uint32_t)(acc << (32 - n)), true);
        n = 0;
    }
};

__global__ void __launch_bounds__(kTile) jpeg_enc_pack(const EncParams* __restrict__ P, const int16_t* __restrict__ coef,
                                                       EncScans S, const uint64_t* __restrict__ off,
                                                       uint8_t* __restrict__ unst)
{
    __shared__ EncTables T;
    const EncGeom& g = P->g;
    stage_tables(&T, P);
    const uint32_t m = (uint32_t)blockIdx.x * kTile + threadIdx.x, img = blockIdx.y;
    if (m >= g.nmcu) return;
    const uint32_t i = m / g.ri, m0 = i * g.ri;
    const uint64_t bit = 8u * interval_byte(S, g, img, i) + (mcu_bit(S, g, img, m) - mcu_bit(S, g, img, m0));
    PackSink s(reinterpret_cast<uint32_t*>(unst + off[img]), bit, (S.total_b[img] + 3u) >> 2);
    const int16_t* ci = coef + (uint64_t)img * g.nmcu * (uint64_t)g.bpm * 64u;
    int pred[3];
    jpeg::enc_mcu_pred(g, m, ci, pred);
    (void)jpeg::enc_mcu(s, g, T, m, ci + (uint64_t)m * (uint64_t)g.bpm * 64u, pred);
    if (m == m0 + (g.ri - 1u) || m == g.nmcu - 1u) {      // the interval's last byte is padded with 1 bits
        const int r = s.n & 7;
        if (r) s.put((1u << (8 - r)) - 1u, 8 - r);
    }
    s.finish();
}

__device__ inline uint32_t count_ff(uint32_t w)
{
    w &= w >> 1;
    w &= w >> 2;
    w &= w >> 4;
    return (uint32_t)__builtin_popcount(w & 0x01010101u);
}

// every image's region of unst is zero up to a multiple of kChunk: whole chunks are read
__global__ void __launch_bounds__(kTile) jpeg_enc_ffcount(const uint64_t* __restrict__ total_b, const uint64_t* __restrict__ off,
                                                          const uint8_t* __restrict__ unst, uint32_t* __restrict__ ff_pre,
                                                          uint64_t* __restrict__ tile_c)
{
    __shared__ uint64_t sh[kTile];
    const uint32_t ch = (uint32_t)blockIdx.x * kTile + threadIdx.x, img = blockIdx.y;
    const uint64_t p0 = (uint64_t)ch * kChunk;
    uint64_t cnt = 0;
    if (p0 < total_b[img]) {
        const uint4* src = reinterpret_cast<const uint4*>(unst + off[img] + p0);
        for (int q = 0; q < (int)(kChunk / 16); q++) {
            const uint4 v = src[q];
            cnt += count_ff(v.x) + count_ff(v.y) + count_ff(v.z) + count_ff(v.w);
        }
    }
    uint64_t total;
    const uint64_t ex = tile_scan(cnt, sh, total);
    ff_pre[((uint64_t)img * gridDim.x + blockIdx.x) * kTile + threadIdx.x] = (uint32_t)ex;
    if (threadIdx.x == 0) tile_c[(uint64_t)img * gridDim.x + blockIdx.x] = total;
}

__global__ void __launch_bounds__(kTile) jpeg_enc_write(const EncParams* __restrict__ P, EncScans S,
                                                        const uint64_t* __restrict__ off, const uint8_t* __restrict__ unst,
                                                        const uint32_t* __restrict__ ff_pre, const uint64_t* __restrict__ tile_c,
                                                        const uint64_t* __restrict__ total_c, uint8_t* __restrict__ out,
                                                        uint64_t cap, uint64_t* __restrict__ sizes, int32_t* __restrict__ status)
{
    const EncGeom& g = P->g;
    const uint32_t img = blockIdx.y, ch = (uint32_t)blockIdx.x * kTile + threadIdx.x;
    const uint64_t U = S.total_b[img], hdr = P->hdr_len;
    uint8_t* dst = out + (uint64_t)img * cap;
    if (blockIdx.x == 0) {
        for (uint32_t k = threadIdx.x; k < P->hdr_len && k < (uint32_t)jpeg::kEncHeaderMax; k += kTile)
            if (k < cap) dst[k] = P->hdr[k];
        if (threadIdx.x == 0) {
            const uint64_t end = hdr + U + total_c[img] + 2u * (uint64_t)(g.nint - 1u);
            if (end < cap) dst[end] = 0xFF;
            if (end + 1 < cap) dst[end + 1] = 0xD9;
            sizes[img] = end + 2;
            if (end + 2 > cap) atomicOr(&status[img], jpeg::kEncOverflow);
        }
    }
    const uint64_t p0 = (uint64_t)ch * kChunk;
    if (p0 >= U) return;
    // the interval that holds byte p0: the last one that starts at or before it (intervals are not empty)
    uint32_t lo = 0, hi = g.nint - 1u;
    for (int it = 0; it < 32 && lo < hi; it++) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (interval_byte(S, g, img, mid) <= p0) lo = mid;
        else hi = mid - 1u;
    }
    // RSTn ahead of interval i is written by the lane that holds the interval's first byte
    uint32_t cur = lo;
    uint64_t next;
    if (lo > 0 && interval_byte(S, g, img, lo) == p0) {
        cur = lo - 1u;
        next = p0;
    } else {
        next = interval_byte(S, g, img, lo + 1u);      // U past the last interval: never met below
    }
    const uint64_t ff = tile_c[(uint64_t)img * gridDim.x + blockIdx.x] + ff_pre[((uint64_t)img * gridDim.x + blockIdx.x) * kTile + threadIdx.x];
    uint64_t pos = hdr + p0 + ff + 2u * (uint64_t)cur;
    const uint4* src = reinterpret_cast<const uint4*>(unst + off[img] + p0);
    for (int q = 0; q < (int)(kChunk / 16); q++) {
        const uint4 v = src[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int b = 0; b < 16; b++) {
            const uint64_t p = p0 + (uint64_t)(q * 16 + b);
            if (p >= U) return;
            if (p == next) {
                if (pos < cap) dst[pos] = 0xFF;
                if (pos + 1 < cap) dst[pos + 1] = (uint8_t)(0xD0 + (cur & 7u));
                pos += 2;
                cur++;
                next = interval_byte(S, g, img, cur + 1u);
            }
            const uint8_t by = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
            if (pos < cap) dst[pos] = by;
            pos++;
            if (by == 0xFF) {
                if (pos < cap) dst[pos] = 0;
                pos++;
            }
        }
    }
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int enc_events(slam_ctx* c)
{
    for (hipEvent_t& e : c->jenc_ev)
        if (!e) SLAM_HIP(c, hipEventCreate(&e));
    return SLAM_OK;
}

// n resident frames (geometry g) into n slots of cap bytes at d_out, sizes and status on the device.  Synchronous.
int encode_batch(slam_ctx* c, hipStream_t s, const uint8_t* d_frames, int n, const EncGeom& g, const EncTables& T,
                 int restart_interval, uint8_t* d_out, size_t cap, uint64_t* d_sizes, int32_t* d_status)
{
    const uint32_t nblk = g.nmcu * (uint32_t)g.bpm;
    const uint32_t nta = (g.nmcu + kTile - 1) / kTile, ntb = (g.nint + kTile - 1) / kTile;
    const size_t N = (size_t)n;
    // workspace: parameters | mcu_pre | tile_a | total_a | int_pre | tile_b | total_b | off | total_c
    const size_t o_mcu = align_up(sizeof(EncParams), 256), o_ta = o_mcu + align_up(N * g.nmcu * 4, 256);
    const size_t o_tota = o_ta + align_up(N * nta * 8, 256), o_int = o_tota + align_up(N * 8, 256);
    const size_t o_tb = o_int + align_up(N * g.nint * 8, 256), o_totb = o_tb + align_up(N * ntb * 8, 256);
    const size_t o_off = o_totb + align_up(N * 8, 256), o_totc = o_off + align_up(N * 8, 256);
    SLAM_HIP(c, c->jenc_ws.ensure(o_totc + align_up(N * 8, 256)));
    SLAM_HIP(c, c->jenc_coef.ensure((size_t)N * nblk * 64 * sizeof(int16_t) + 256));
    if (int rc = enc_events(c)) return rc;
    // pinned: the parameters on their way up, the unstuffed lengths on their way down, the offsets on their way up
    const size_t h_len = align_up(sizeof(EncParams), 256), h_bytes = h_len + 2 * N * 8;
    uint8_t* hp = static_cast<uint8_t*>(readback(c, h_bytes));
    if (!hp) return set_err(c, SLAM_E_HIP, "pinned readback allocation failed");
    EncParams* hP = reinterpret_cast<EncParams*>(hp);
    uint64_t* h_U = reinterpret_cast<uint64_t*>(hp + h_len);
    uint64_t* h_off = h_U + N;
    std::memset(hP, 0, sizeof(EncParams));
    hP->g = g;
    hP->T = T;
    hP->hdr_len = (uint32_t)jpeg::enc_header(g, T, restart_interval, hP->hdr);

    uint8_t* ws = c->jenc_ws.as<uint8_t>();
    const EncParams* dP = reinterpret_cast<const EncParams*>(ws);
    uint32_t* mcu_pre = reinterpret_cast<uint32_t*>(ws + o_mcu);
    uint64_t* tile_a = reinterpret_cast<uint64_t*>(ws + o_ta);
    uint64_t* total_a = reinterpret_cast<uint64_t*>(ws + o_tota);
    uint64_t* int_pre = reinterpret_cast<uint64_t*>(ws + o_int);
    uint64_t* tile_b = reinterpret_cast<uint64_t*>(ws + o_tb);
    uint64_t* total_b = reinterpret_cast<uint64_t*>(ws + o_totb);
    uint64_t* off = reinterpret_cast<uint64_t*>(ws + o_off);
    uint64_t* total_c = reinterpret_cast<uint64_t*>(ws + o_totc);
    int16_t* coef = c->jenc_coef.as<int16_t>();
    const EncScans S{mcu_pre, tile_a, total_a, int_pre, tile_b, total_b, nta, ntb};
    hipEvent_t* ev = c->jenc_ev;

    SLAM_HIP(c, hipMemcpyAsync(ws, hP, sizeof(EncParams), hipMemcpyHostToDevice, s));
    SLAM_HIP(c, hipMemsetAsync(d_status, 0, N * sizeof(int32_t), s));
    SLAM_HIP(c, hipEventRecord(ev[0], s));
    jpeg_enc_dct<<<dim3((nblk + kDctBlocks - 1) / kDctBlocks, n), kDctBlocks * 8, 0, s>>>(dP, d_frames, coef);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(ev[1], s));
    jpeg_enc_count<<<dim3(nta, n), kTile, 0, s>>>(dP, coef, mcu_pre, tile_a, d_status);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(ev[2], s));
    jpeg_enc_scan_tiles<<<n, kTile, 0, s>>>(tile_a, nta, total_a);
    SLAM_HIP(c, hipGetLastError());
    jpeg_enc_intervals<<<dim3(ntb, n), kTile, 0, s>>>(dP, S, int_pre, tile_b);
    SLAM_HIP(c, hipGetLastError());
    jpeg_enc_scan_tiles<<<n, kTile, 0, s>>>(tile_b, ntb, total_b);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(ev[3], s));
    SLAM_HIP(c, hipMemcpyAsync(h_U, total_b, N * 8, hipMemcpyDeviceToHost, s));
    if (int rc = stream_sync(c, s)) return rc;

    uint64_t total = 0, max_u = 0;
    for (int i = 0; i < n; i++) {
        h_off[i] = total;
        total += align_up((size_t)h_U[i], kChunk);
        if (h_U[i] > max_u) max_u = h_U[i];
    }
    const uint32_t nchunk = (uint32_t)((max_u + kChunk - 1) / kChunk), ntc = (nchunk + kTile - 1) / kTile;
    const size_t o_tc = align_up(N * ntc * kTile * 4, 256);
    SLAM_HIP(c, c->jenc_bits.ensure((size_t)total + 256));
    SLAM_HIP(c, c->jenc_ff.ensure(o_tc + N * ntc * 8));
    uint8_t* unst = c->jenc_bits.as<uint8_t>();
    uint32_t* ff_pre = c->jenc_ff.as<uint32_t>();
    uint64_t* tile_c = reinterpret_cast<uint64_t*>(c->jenc_ff.as<uint8_t>() + o_tc);
    SLAM_HIP(c, hipMemcpyAsync(off, h_off, N * 8, hipMemcpyHostToDevice, s));
    SLAM_HIP(c, hipEventRecord(ev[4], s));
    SLAM_HIP(c, hipMemsetAsync(unst, 0, (size_t)total, s));
    jpeg_enc_pack<<<dim3(nta, n), kTile, 0, s>>>(dP, coef, S, off, unst);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(ev[5], s));
    jpeg_enc_ffcount<<<dim3(ntc, n), kTile, 0, s>>>(total_b, off, unst, ff_pre, tile_c);
    SLAM_HIP(c, hipGetLastError());
    jpeg_enc_scan_tiles<<<n, kTile, 0, s>>>(tile_c, ntc, total_c);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(ev[6], s));
    jpeg_enc_write<<<dim3(ntc, n), kTile, 0, s>>>(dP, S, off, unst, ff_pre, tile_c, total_c, d_out, (uint64_t)cap, d_sizes,
                                                  d_status);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(ev[7], s));
    if (int rc = stream_sync(c, s)) return rc;
    float ms = 0.f;
    for (int k = 0; k < 7; k++) {
        SLAM_HIP(c, hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
        c->jenc_ms[k] = ms;
    }
    c->jenc_bytes[0] = (uint64_t)N * g.h * g.w * g.channels;
    c->jenc_bytes[1] = (uint64_t)N * nblk * 128u;
    c->jenc_bytes[2] = total;
    c->jenc_bytes[3] = (uint64_t)N * 8;      // read back mid-way
    c->jenc_timed = true;
    return SLAM_OK;
}

}  // namespace

void jpeg_enc_release(slam_ctx* c)
{
    for (hipEvent_t& e : c->jenc_ev)
        if (e) {
            (void)hipEventDestroy(e);
            e = nullptr;
        }
}

}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_jpeg_encode_batch_dev(slam_ctx* c, void* stream, const uint8_t* frames_dev, int n, int h, int w,
                                          int channels, size_t row_step, size_t frame_step, int quality, int sampling,
                                          int restart_interval, uint8_t* out_dev, size_t cap_per_image, uint64_t* sizes_dev,
                                          int32_t* status_dev)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!frames_dev || n <= 0 || !out_dev || !sizes_dev || !status_dev) return set_err(c, SLAM_E_INVALID_ARG, "null argument or empty batch");
    if (n > 65535) return set_err(c, SLAM_E_INVALID_ARG, "more than 65535 frames in a batch");
    EncGeom g;
    EncTables T;
    std::string msg;
    if (int rc = jpeg::enc_setup(h, w, channels, row_step, frame_step, quality, sampling, restart_interval, g, T, msg))
        return set_err(c, rc, msg);
    if (frame_step < row_step * (size_t)h && n > 1) return set_err(c, SLAM_E_INVALID_ARG, "frame step smaller than a frame");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    return encode_batch(c, s, frames_dev, n, g, T, restart_interval, out_dev, cap_per_image, sizes_dev, status_dev);
}

extern "C" int slam_jpeg_encode(slam_ctx* c, const uint8_t* img, int h, int w, int channels, size_t row_step, int quality,
                                int sampling, int restart_interval, uint8_t* out, size_t cap, size_t* size, int* status)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (size) *size = 0;
    if (status) *status = 0;
    if (!img || !size || (!out && cap)) return set_err(c, SLAM_E_INVALID_ARG, "null argument");
    EncGeom g;
    EncTables T;
    std::string msg;
    if (int rc = jpeg::enc_setup(h, w, channels, row_step, 0, quality, sampling, restart_interval, g, T, msg))
        return set_err(c, rc, msg);
    SLAM_HIP(c, hipSetDevice(c->device));
    const size_t row = (size_t)w * channels;
    DevLayout lay;
    const auto s_img = lay.add<uint8_t>(row * h), s_out = lay.add<uint8_t>(cap);
    const auto s_meta = lay.add<uint64_t>(2);       // the size, then the status in the second word's low half
    DevMem io;
    SLAM_HIP(c, io.bind(c->jenc_io, lay));
    SLAM_HIP(c, hipMemcpy2D(io.ptr(s_img), row, img, row_step, row, h, hipMemcpyHostToDevice));
    g.row_step = row;
    g.frame_step = row * h;
    uint64_t* d_size = io.ptr(s_meta);
    int32_t* d_stat = reinterpret_cast<int32_t*>(d_size + 1);
    if (int rc = encode_batch(c, c->stream, io.ptr(s_img), 1, g, T, restart_interval, io.ptr(s_out), cap, d_size, d_stat)) return rc;
    uint64_t meta[2] = {0, 0};
    SLAM_HIP(c, hipMemcpy(meta, d_size, s_meta.bytes(), hipMemcpyDeviceToHost));
    const size_t have = meta[0] < cap ? (size_t)meta[0] : cap;
    if (have) SLAM_HIP(c, hipMemcpy(out, io.ptr(s_out), have, hipMemcpyDeviceToHost));
    *size = (size_t)meta[0];
    if (status) *status = (int)(int32_t)(meta[1] & 0xFFFFFFFFu);
    return SLAM_OK;
}

extern "C" int slam_jpeg_enc_last_timing(slam_ctx* c, double* ms7, uint64_t* bytes4)
{
    if (!c || !ms7) return SLAM_E_INVALID_ARG;
    if (!c->jenc_timed) return set_err(c, SLAM_E_INVALID_ARG, "no slam_jpeg_encode_batch_dev call to report");
    for (int k = 0; k < 7; k++) ms7[k] = c->jenc_ms[k];
    if (bytes4)
        for (int k = 0; k < 4; k++) bytes4[k] = c->jenc_bytes[k];
    return SLAM_OK;
}

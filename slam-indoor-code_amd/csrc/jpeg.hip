// Baseline JPEG decoding on gfx950 (cv::imread / cv::imdecode).
//
// The host parses the headers of every stream of a batch on the thread pool
// (jpeg_parse.cpp) and uploads, in one copy from pinned memory, the image
// descriptors (tables, geometry), the segment table and the compressed bytes.
// Three kernels then run over the whole batch:
//
//   jpeg_huff     one lane per segment (a restart interval, or the whole scan of a
//                 stream without DRI): jpeg_huff.h's decode_segment writes the
//                 non-zero coefficients, int16, natural order, into the cleared
//                 coefficient buffer (blocks in raster order per component) and
//                 ors the fault bits into the image's status word
//   jpeg_idct     eight lanes per block: each dequantises and transforms one
//                 column, the block is transposed through LDS, each lane then
//                 transforms one row and stores its 8 range-limited samples
//   jpeg_upcolor  four pixels per lane: fancy upsampling and YCbCr -> BGR
//                 (jpeg_pix.h), written interleaved into the n x h x w x 3 frames
//
// With SLAM_OPT_JPEG_SYNC set, the segments it selects are decoded by one lane per
// chunk of their bytes instead (jpeg_sync, jpeg_sync_count, jpeg_sync_scan,
// jpeg_sync_write below) and reach jpeg_huff only when that
// path does not accept them.
//
// The arithmetic is in the two shared headers, which the host decoder
// (slam_jpeg_decode_host) runs too: device and host agree byte for byte, faulted
// streams included.
#include <chrono>
#include <cstring>

#include "jpeg_parse.h"
#include "slamhip_internal.h"

namespace slamhip {

namespace {

using jpeg::ImageDesc;
using jpeg::Segment;

constexpr int kIdctBlocks = 32;      // blocks per workgroup of jpeg_idct (8 lanes each)
constexpr int kIdctPitch = 72;       // LDS words per block: 64 + 8, so that blocks 0 .. 3 of a wave start in different banks

// lanes: active lanes per wave (the rest only help to stage the tables): with few
// segments every segment gets a wave of its own, so that segments do not wait on
// each other's branches.  The zigzag table lives in LDS (its lookup precedes every
// coefficient store).  When all segments of the workgroup belong to one image
// (always, unless images are a few blocks each) its eight Huffman tables are
// copied into LDS first: the table lookup is on the dependent chain of every
// symbol.  Measured on 210 x 1080p: 250 -> 222 ms without
// DRI, 11.5 -> 9.5 ms with a restart per MCU row; the kernel is bound by the
// instructions of that chain, not by memory (a reader that fetched eight bytes at
// a time, the next eight in flight, was slower: 311 ms).
__global__ void __launch_bounds__(64) jpeg_huff(const ImageDesc* __restrict__ desc, const Segment* __restrict__ segs,
                                                int nseg, int lanes, const uint8_t* __restrict__ bytes,
                                                int16_t* __restrict__ coef, int32_t* __restrict__ status)
{
    __shared__ jpeg::HuffTable tables[8];
    __shared__ uint8_t zz[64];
    constexpr int kTableWords = 8 * (int)sizeof(jpeg::HuffTable) / 4;      // copied as 32-bit words
    static_assert(sizeof(jpeg::HuffTable) % 4 == 0, "tables are whole words");
    const int first = (int)blockIdx.x * lanes;
    if (first >= nseg) return;
    const int last = first + lanes - 1 < nseg - 1 ? first + lanes - 1 : nseg - 1;
    const uint32_t image = segs[first].image;
    const bool one_image = segs[last].image == image;      // uniform over the workgroup
    zz[threadIdx.x] = (uint8_t)jpeg::zigzag_natural((int)threadIdx.x);
    if (one_image) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(desc[image].tables);
        uint32_t* dst = reinterpret_cast<uint32_t*>(tables);
        for (int i = (int)threadIdx.x; i < kTableWords; i += 64) dst[i] = src[i];
    }
    __syncthreads();
    const int s = first + (int)threadIdx.x;
    if ((int)threadIdx.x >= lanes || s >= nseg) return;
    const Segment sg = segs[s];
    const ImageDesc& im = desc[sg.image];
    const int st = one_image ? jpeg::decode_segment(im, tables, zz, bytes, sg, coef + im.coef_off)
                             : jpeg::decode_segment(im, im.tables, zz, bytes, sg, coef + im.coef_off);
    if (st) atomicOr(&status[sg.image], st);
}

__global__ void __launch_bounds__(kIdctBlocks * 8) jpeg_idct(const ImageDesc* __restrict__ desc,
                                                             const int16_t* __restrict__ coef,
                                                             uint8_t* __restrict__ planes)
{
    __shared__ uint32_t ws[kIdctBlocks * kIdctPitch];
    const ImageDesc& im = desc[blockIdx.y];
    const uint32_t total = im.total_blocks;
    if ((uint32_t)blockIdx.x * kIdctBlocks >= total) return;      // the whole workgroup: nothing waits at the barrier
    const int slot = (int)threadIdx.x >> 3, j = (int)threadIdx.x & 7;
    const uint32_t blk = (uint32_t)blockIdx.x * kIdctBlocks + (uint32_t)slot;
    const bool live = blk < total;
    int c = 0;
    if (live) {
        if (im.ncomp > 2 && blk >= im.comp[2].coef_block) c = 2;
        else if (im.ncomp > 1 && blk >= im.comp[1].coef_block) c = 1;
        uint32_t col[8];
        jpeg::idct_column(coef + im.coef_off + (uint64_t)blk * 64u, im.quant[c], j, col);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[slot * kIdctPitch + r * 8 + j] = col[r];
    }
    __syncthreads();
    if (!live) return;
    const jpeg::ScanComp& sc = im.comp[c];
    const uint32_t b = blk - sc.coef_block;
    const uint32_t brow = b / (uint32_t)sc.bw, bcol = b % (uint32_t)sc.bw;
    const size_t pitch = (size_t)sc.bw * 8;
    uint32_t row[8];
#pragma unroll
    for (int i = 0; i < 8; i++) row[i] = ws[slot * kIdctPitch + j * 8 + i];
    alignas(8) uint8_t px[8];
    jpeg::idct_row(row, px);
    uint8_t* dst = planes + im.plane_off + im.plane_comp[c] + ((size_t)brow * 8 + j) * pitch + (size_t)bcol * 8;
    *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(px);      // planes are 8-byte aligned by layout
}

// lane (x, y) of image z: pixels 4 x .. 4 x + 3 of row y
__global__ void __launch_bounds__(256) jpeg_upcolor(const ImageDesc* __restrict__ desc,
                                                    const uint8_t* __restrict__ planes, uint8_t* __restrict__ out, int w,
                                                    int h, int channels)
{
    const int x0 = 4 * ((int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x);
    const int y = (int)blockIdx.y * (int)blockDim.y + (int)threadIdx.y;
    if (x0 >= w || y >= h) return;
    const ImageDesc& im = desc[blockIdx.z];
    uint8_t* dst = out + (((size_t)blockIdx.z * h + y) * w + x0) * channels;
    alignas(4) uint8_t px[12];
    const int np = w - x0 < 4 ? w - x0 : 4;
    if (im.valid) {
        const uint8_t* pl = planes + im.plane_off;
        for (int i = 0; i < np; i++) jpeg::emit_pixel(im, pl, x0 + i, y, px + i * channels);
    } else {
        for (int i = 0; i < 12; i++) px[i] = 0;
    }
    if ((w & 3) == 0) {      // whole groups, and every row starts on a 4-byte boundary
        const uint32_t* v = reinterpret_cast<const uint32_t*>(px);
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
        for (int i = 0; i < channels; i++) d[i] = v[i];
    } else {
        for (int i = 0; i < np * channels; i++) dst[i] = px[i];
    }
}

// ---- chunk-parallel entropy decoding (jpeg_huff.h) ----------
//
// A workgroup is kSyncLanes consecutive chunks of one segment, one per lane, with the
// image's Huffman tables in LDS.  No workgroup waits on another inside a kernel: what
// passes between workgroups passes between launches, and every loop is bounded by the
// chunk size or the lane count.

using jpeg::ChunkCount;
using jpeg::SyncSeg;
constexpr int kSyncLanes = jpeg::kSyncLanes;
constexpr int kTableWords = 8 * (int)sizeof(jpeg::HuffTable) / 4;

struct ChunkBase {      // the exclusive scan of the counts: a chunk's first block and predictors
    uint32_t j0, p0, p1, p2;
};
struct SegState {       // per parallel segment, read back by the host
    uint32_t started, flags, launches, pad;
};

__device__ inline void sync_stage_tables(jpeg::HuffTable* tables, const ImageDesc* desc, uint32_t image)
{
    const uint32_t* src = reinterpret_cast<const uint32_t*>(desc[image].tables);
    uint32_t* dst = reinterpret_cast<uint32_t*>(tables);
    for (int i = (int)threadIdx.x; i < kTableWords; i += kSyncLanes) dst[i] = src[i];
}

__device__ inline uint32_t sync_limit(const SyncSeg& sg, uint32_t ci, uint32_t C)
{
    const uint64_t e = (uint64_t)sg.off + ((uint64_t)ci + 1) * C;
    return e < sg.end ? (uint32_t)e : sg.end;
}

// Launch r of jpeg::kSyncLaunches.  Lane 0 enters with the true state (the segment's first
// workgroup), cold (launch 0) or with what the workgroup before left in launch r - 1
// (wg_exit[r - 1]); a workgroup whose entry is the one it last ran with has nothing to do.
// Inside, a round recomputes the lanes whose entry changed; at most kSyncLanes + 1 rounds.
__global__ void __launch_bounds__(kSyncLanes) jpeg_sync(const ImageDesc* __restrict__ desc, const SyncSeg* __restrict__ psegs,
                                                        const uint32_t* __restrict__ wg_seg, const uint8_t* __restrict__ bytes,
                                                        uint32_t C, int r, int nwg, uint64_t* __restrict__ st_exit,
                                                        uint64_t* __restrict__ wg_entry, uint64_t* __restrict__ wg_exit,
                                                        uint32_t* __restrict__ wg_rmax, uint32_t* __restrict__ wg_rtot,
                                                        SegState* __restrict__ seg_state)
{
    __shared__ jpeg::HuffTable tables[8];
    __shared__ uint64_t ex[kSyncLanes];
    const int j = (int)blockIdx.x, lane = (int)threadIdx.x;
    const uint32_t ps = wg_seg[j];
    const SyncSeg sg = psegs[ps];
    const uint32_t ci0 = (uint32_t)j * kSyncLanes - sg.chunk0, ci = ci0 + (uint32_t)lane;
    const bool active = ci < sg.nchunks;
    uint64_t e0;
    if (ci0 == 0) e0 = jpeg::state_pack(sg.off, 0, 0, 0);
    else if (r == 0) e0 = jpeg::sync_cold(bytes, sg, ci0, C);
    else e0 = jpeg::sync_entry(wg_exit[(size_t)(r - 1) * nwg + j - 1], jpeg::sync_cold(bytes, sg, ci0, C));
    const uint64_t old0 = r > 0 ? wg_entry[j] : 0;
    if (r > 0 && old0 == e0) {      // the same in every lane
        if (lane == 0) wg_exit[(size_t)r * nwg + j] = wg_exit[(size_t)(r - 1) * nwg + j];
        return;
    }
    sync_stage_tables(tables, desc, sg.image);
    const size_t slot = (size_t)j * kSyncLanes + lane;
    ex[lane] = r == 0 ? jpeg::kStateUnknown : st_exit[slot];
    __syncthreads();
    const uint64_t cold = active && ci > 0 ? jpeg::sync_cold(bytes, sg, ci, C) : 0;
    const uint32_t limit = active ? sync_limit(sg, ci, C) : 0, max_steps = jpeg::sync_max_steps(C);
    uint64_t cur = lane == 0 ? old0 : jpeg::sync_entry(ex[lane - 1], cold);
    uint32_t rounds = 0;
    for (int round = 0; round < kSyncLanes + 1; round++) {
        const uint64_t ne = lane == 0 ? e0 : jpeg::sync_entry(ex[lane - 1], cold);
        const bool dirty = active && ((r == 0 && round == 0) || ne != cur);
        if (!__syncthreads_or(dirty)) break;      // also orders the reads of ex above before the writes below
        rounds++;
        if (dirty) {
            cur = ne;
            ex[lane] = jpeg::sync_walk(tables, bytes, sg, cur, limit, max_steps, nullptr);
        }
        __syncthreads();
    }
    st_exit[slot] = ex[lane];
    if (lane == 0) {
        wg_entry[j] = e0;
        wg_exit[(size_t)r * nwg + j] = ex[kSyncLanes - 1];
        if (rounds > wg_rmax[j]) wg_rmax[j] = rounds;
        wg_rtot[j] += rounds;
        atomicMax(&seg_state[ps].launches, (uint32_t)r + 1u);
    }
}

// Every chunk walks once more from its predecessor's stored exit state: the recomputed exit must
// be the stored one (else kChunkMismatch), and the walk counts the blocks started and their DC sums.
__global__ void __launch_bounds__(kSyncLanes) jpeg_sync_count(const ImageDesc* __restrict__ desc,
                                                              const SyncSeg* __restrict__ psegs,
                                                              const uint32_t* __restrict__ wg_seg,
                                                              const uint8_t* __restrict__ bytes, uint32_t C,
                                                              const uint64_t* __restrict__ st_exit, ChunkCount* __restrict__ counts)
{
    __shared__ jpeg::HuffTable tables[8];
    const int j = (int)blockIdx.x, lane = (int)threadIdx.x;
    const SyncSeg sg = psegs[wg_seg[j]];
    sync_stage_tables(tables, desc, sg.image);
    __syncthreads();
    const size_t slot = (size_t)j * kSyncLanes + lane;
    const uint32_t ci = (uint32_t)slot - sg.chunk0;
    ChunkCount cc = {0, 0, 0, 0, 0, 0};
    if (ci < sg.nchunks) {
        const uint64_t entry = ci == 0 ? jpeg::state_pack(sg.off, 0, 0, 0)
                                       : jpeg::sync_entry(st_exit[slot - 1], jpeg::sync_cold(bytes, sg, ci, C));
        const uint64_t x = jpeg::sync_walk(tables, bytes, sg, entry, sync_limit(sg, ci, C), jpeg::sync_max_steps(C), &cc);
        if (x != st_exit[slot]) cc.flags |= jpeg::kChunkMismatch;
    }
    counts[slot] = cc;
}

// One workgroup per parallel segment: the exclusive scan of its chunks' counts, tile by tile.
__global__ void __launch_bounds__(kSyncLanes) jpeg_sync_scan(const SyncSeg* __restrict__ psegs,
                                                             const ChunkCount* __restrict__ counts, ChunkBase* __restrict__ base,
                                                             SegState* __restrict__ seg_state)
{
    __shared__ uint32_t sc[4][kSyncLanes];
    __shared__ uint32_t flags_all;
    const int lane = (int)threadIdx.x;
    const SyncSeg sg = psegs[blockIdx.x];
    if (lane == 0) flags_all = 0;
    uint32_t carry[4] = {0, 0, 0, 0}, flags = 0;
    const uint32_t tiles = (sg.nchunks + kSyncLanes - 1) / kSyncLanes;
    for (uint32_t t = 0; t < tiles; t++) {
        const size_t slot = (size_t)sg.chunk0 + (size_t)t * kSyncLanes + lane;
        const ChunkCount cc = counts[slot];      // the slots past the segment's chunks hold zeros
        const uint32_t own[4] = {cc.nstart, cc.dc0, cc.dc1, cc.dc2};
        flags |= cc.flags;
        __syncthreads();      // the tile before is read
#pragma unroll
        for (int q = 0; q < 4; q++) sc[q][lane] = own[q];
        __syncthreads();
        for (int d = 1; d < kSyncLanes; d <<= 1) {
            uint32_t add[4] = {0, 0, 0, 0};
            if (lane >= d)
#pragma unroll
                for (int q = 0; q < 4; q++) add[q] = sc[q][lane - d];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; q++) sc[q][lane] += add[q];
            __syncthreads();
        }
        base[slot] = ChunkBase{carry[0] + sc[0][lane] - own[0], carry[1] + sc[1][lane] - own[1], carry[2] + sc[2][lane] - own[2],
                               carry[3] + sc[3][lane] - own[3]};
#pragma unroll
        for (int q = 0; q < 4; q++) carry[q] += sc[q][kSyncLanes - 1];
    }
    if (flags) atomicOr(&flags_all, flags);
    __syncthreads();
    if (lane == 0) {
        seg_state[blockIdx.x].started = carry[0];
        seg_state[blockIdx.x].flags = flags_all;
    }
}

// The blocks that start in a chunk, through decode_block, into decode_segment's layout.  A segment
// the count has already rejected is not written.
__global__ void __launch_bounds__(kSyncLanes) jpeg_sync_write(const ImageDesc* __restrict__ desc,
                                                              const SyncSeg* __restrict__ psegs,
                                                              const uint32_t* __restrict__ wg_seg,
                                                              const uint8_t* __restrict__ bytes,
                                                              const ChunkCount* __restrict__ counts,
                                                              const ChunkBase* __restrict__ base, int16_t* __restrict__ coef,
                                                              SegState* __restrict__ seg_state)
{
    __shared__ jpeg::HuffTable tables[8];
    __shared__ uint8_t zz[64];
    const int j = (int)blockIdx.x, lane = (int)threadIdx.x;
    const uint32_t ps = wg_seg[j];
    const SyncSeg sg = psegs[ps];
    if (lane < 64) zz[lane] = (uint8_t)jpeg::zigzag_natural(lane);
    sync_stage_tables(tables, desc, sg.image);
    __syncthreads();
    const SegState ss = seg_state[ps];
    if (ss.flags || ss.started != sg.nblocks) return;
    const size_t slot = (size_t)j * kSyncLanes + lane;
    if ((uint32_t)slot - sg.chunk0 >= sg.nchunks) return;
    const ChunkCount cc = counts[slot];
    const ChunkBase b = base[slot];
    const ImageDesc& im = desc[sg.image];
    if (jpeg::sync_write(im, tables, zz, bytes, sg, cc, b.j0, b.p0, b.p1, b.p2, coef + im.coef_off))
        atomicOr(&seg_state[ps].flags, jpeg::kChunkFault);
}

// the blocks of the segments that fall back, cleared again: grid (segments, slices)
__global__ void __launch_bounds__(256) jpeg_sync_clear(const ImageDesc* __restrict__ desc, const SyncSeg* __restrict__ psegs,
                                                       const uint32_t* __restrict__ list, int16_t* __restrict__ coef)
{
    const SyncSeg sg = psegs[list[blockIdx.x]];
    const ImageDesc& im = desc[sg.image];
    const uint32_t stride = gridDim.y * blockDim.x;
    for (uint32_t jb = blockIdx.y * blockDim.x + threadIdx.x; jb < sg.nblocks; jb += stride) {
        uint32_t blk;
        int c;
        if (!jpeg::seg_block_addr(im, sg.mcu0, sg.bpm, jb, blk, c)) continue;
        uint4* dst = reinterpret_cast<uint4*>(coef + im.coef_off + (uint64_t)blk * 64u);      // 128-byte blocks, 16-byte aligned
#pragma unroll
        for (int q = 0; q < 8; q++) dst[q] = make_uint4(0, 0, 0, 0);
    }
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct JpegHost {
    std::vector<jpeg::Parsed> parsed;
    std::vector<std::string> msgs;
    std::vector<int> codes;
    std::vector<size_t> byte_off;
    // SLAM_OPT_JPEG_SYNC: the segments on the parallel path (byte offsets of the batch), the
    // segments they were, their workgroups, and per image which of its segments they are
    std::vector<SyncSeg> psegs;
    std::vector<Segment> porig;
    std::vector<uint32_t> wg_seg;
    std::vector<std::vector<uint8_t>> is_par;
};

int jpeg_events(slam_ctx* c)
{
    for (hipEvent_t& e : c->jpeg_ev)
        if (!e) SLAM_HIP(c, hipEventCreate(&e));
    return SLAM_OK;
}

int jpeg_sync_events(slam_ctx* c)
{
    for (hipEvent_t& e : c->jpeg_sync_ev)
        if (!e) SLAM_HIP(c, hipEventCreate(&e));
    return SLAM_OK;
}

int jpeg_lanes(const slam_ctx* c, int nseg)
{
    if (c->opt_jpeg_lanes >= 1 && c->opt_jpeg_lanes <= 64) return c->opt_jpeg_lanes;      // SLAM_OPT_JPEG_LANES
    // fill the device's wave slots before a wave takes a second segment: a workgroup is one wave with
    // 11.4 KB of tables in LDS, so 14 of them fit the 160 KB of a CU
    const int slots = c->cu_count * 14;
    const int lanes = (nseg + slots - 1) / slots;
    return lanes < 1 ? 1 : lanes > 64 ? 64 : lanes;
}

// The parallel segments H.psegs of a batch whose tables and bytes are uploaded and whose
// coefficients are cleared: the sync launches, count, scan and write, then one small readback
// (the verdict per segment and the round counts), and for the segments that are not accepted
// the clearing of their blocks and the one-lane jpeg_huff over their compacted list.
int sync_segments(slam_ctx* c, hipStream_t s, JpegHost& H, uint32_t C, uint8_t* din, size_t o_bytes, size_t o_psegs,
                  size_t o_wgseg, size_t o_fb, const ImageDesc* d_desc, int32_t* d_stat)
{
    const size_t nps = H.psegs.size(), nwg = H.wg_seg.size(), nslots = nwg * kSyncLanes;
    constexpr int K = jpeg::kSyncLaunches;
    const size_t o_counts = nslots * sizeof(uint64_t), o_base = o_counts + nslots * sizeof(ChunkCount);
    const size_t o_wgentry = o_base + nslots * sizeof(ChunkBase), o_wgexit = o_wgentry + nwg * sizeof(uint64_t);
    const size_t o_state = o_wgexit + (size_t)K * nwg * sizeof(uint64_t);
    const size_t state_bytes = nps * sizeof(SegState) + 2 * nwg * sizeof(uint32_t);
    SLAM_HIP(c, c->jpeg_sync.ensure(o_state + state_bytes));
    if (int rc = jpeg_sync_events(c)) return rc;
    uint8_t* ws = c->jpeg_sync.as<uint8_t>();
    uint64_t* st_exit = reinterpret_cast<uint64_t*>(ws);
    ChunkCount* counts = reinterpret_cast<ChunkCount*>(ws + o_counts);
    ChunkBase* base = reinterpret_cast<ChunkBase*>(ws + o_base);
    uint64_t* wg_entry = reinterpret_cast<uint64_t*>(ws + o_wgentry);
    uint64_t* wg_exit = reinterpret_cast<uint64_t*>(ws + o_wgexit);
    SegState* seg_state = reinterpret_cast<SegState*>(ws + o_state);
    uint32_t* wg_rmax = reinterpret_cast<uint32_t*>(ws + o_state + nps * sizeof(SegState));
    uint32_t* wg_rtot = wg_rmax + nwg;
    const SyncSeg* d_psegs = reinterpret_cast<const SyncSeg*>(din + o_psegs);
    const uint32_t* d_wgseg = reinterpret_cast<const uint32_t*>(din + o_wgseg);
    const uint8_t* d_bytes = din + o_bytes;
    int16_t* coef = c->jpeg_coef.as<int16_t>();
    hipEvent_t* ev = c->jpeg_sync_ev;

    SLAM_HIP(c, hipMemsetAsync(seg_state, 0, state_bytes, s));
    SLAM_HIP(c, hipEventRecord(ev[0], s));
    for (int r = 0; r < K; r++) {
        jpeg_sync<<<(unsigned)nwg, kSyncLanes, 0, s>>>(d_desc, d_psegs, d_wgseg, d_bytes, C, r, (int)nwg, st_exit, wg_entry, wg_exit,
                                                       wg_rmax, wg_rtot, seg_state);
        SLAM_HIP(c, hipGetLastError());
    }
    SLAM_HIP(c, hipEventRecord(ev[1], s));
    jpeg_sync_count<<<(unsigned)nwg, kSyncLanes, 0, s>>>(d_desc, d_psegs, d_wgseg, d_bytes, C, st_exit, counts);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(ev[2], s));
    jpeg_sync_scan<<<(unsigned)nps, kSyncLanes, 0, s>>>(d_psegs, counts, base, seg_state);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(ev[3], s));
    jpeg_sync_write<<<(unsigned)nwg, kSyncLanes, 0, s>>>(d_desc, d_psegs, d_wgseg, d_bytes, counts, base, coef, seg_state);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(ev[4], s));
    uint8_t* rb = static_cast<uint8_t*>(readback(c, state_bytes));
    if (!rb) return set_err(c, SLAM_E_HIP, "pinned readback allocation failed");
    SLAM_HIP(c, hipMemcpyAsync(rb, seg_state, state_bytes, hipMemcpyDeviceToHost, s));
    if (int rc = stream_sync(c, s)) return rc;

    slam_jpeg_sync_stats& T = c->jpeg_sync_stats;
    T.parallel_segments = (int32_t)nps;
    T.chunk_bytes = (int32_t)C;
    T.lanes = kSyncLanes;
    const SegState* h_state = reinterpret_cast<const SegState*>(rb);
    const uint32_t* h_rmax = reinterpret_cast<const uint32_t*>(rb + nps * sizeof(SegState));
    const uint32_t* h_rtot = h_rmax + nwg;
    uint8_t* hs = static_cast<uint8_t*>(c->h_jpeg);
    Segment* fb_segs = reinterpret_cast<Segment*>(hs + o_fb);
    uint32_t* fb_list = reinterpret_cast<uint32_t*>(hs + o_fb + nps * sizeof(Segment));
    size_t nfb = 0;
    for (size_t k = 0; k < nps; k++) {
        T.chunks += H.psegs[k].nchunks;
        if ((int32_t)h_state[k].launches > T.launch_rounds_max) T.launch_rounds_max = (int32_t)h_state[k].launches;
        T.launch_rounds_total += h_state[k].launches;
        if (h_state[k].flags || h_state[k].started != H.psegs[k].nblocks) {
            fb_segs[nfb] = H.porig[k];
            fb_list[nfb] = (uint32_t)k;
            nfb++;
        }
    }
    for (size_t j = 0; j < nwg; j++) {
        if ((int32_t)h_rmax[j] > T.wg_rounds_max) T.wg_rounds_max = (int32_t)h_rmax[j];
        T.wg_rounds_total += h_rtot[j];
    }
    T.fallback_segments = (int32_t)nfb;
    float ms = 0.f;
    for (int k = 0; k < 4; k++) {
        SLAM_HIP(c, hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
        T.ms[k] = ms;
    }
    SLAM_HIP(c, hipEventRecord(ev[5], s));
    if (nfb) {
        // the list is compacted in place: the device copy keeps the layout (segments, then indices at nps segments)
        SLAM_HIP(c, hipMemcpyAsync(din + o_fb, hs + o_fb, nps * (sizeof(Segment) + sizeof(uint32_t)), hipMemcpyHostToDevice, s));
        const Segment* d_fb = reinterpret_cast<const Segment*>(din + o_fb);
        const uint32_t* d_list = reinterpret_cast<const uint32_t*>(din + o_fb + nps * sizeof(Segment));
        jpeg_sync_clear<<<dim3((unsigned)nfb, 16), 256, 0, s>>>(d_desc, d_psegs, d_list, coef);
        SLAM_HIP(c, hipGetLastError());
        const int lanes = jpeg_lanes(c, (int)nfb);
        jpeg_huff<<<((int)nfb + lanes - 1) / lanes, 64, 0, s>>>(d_desc, d_fb, (int)nfb, lanes, d_bytes, coef, d_stat);
        SLAM_HIP(c, hipGetLastError());
    }
    SLAM_HIP(c, hipEventRecord(ev[6], s));
    return SLAM_OK;
}

// n streams decoded into d_out (n x h x w x channels, device) on s; status: host, n.  w, h: the size
// every stream must have.  Synchronous.
int decode_batch(slam_ctx* c, hipStream_t s, const uint8_t* const* bufs, const size_t* lens, int n, int w, int h,
                 int channels, uint8_t* d_out, int* status, int flags = 0)
{
    if (flags & ~SLAM_JPEG_MJPEG) return set_err(c, SLAM_E_INVALID_ARG, "unknown parse flag");
    const int sync_mode = c->opt_jpeg_sync;
    const uint32_t C = jpeg::sync_chunk_bytes(c->opt_jpeg_chunk);
    c->jpeg_sync_stats = slam_jpeg_sync_stats{};
    if (sync_mode) {
        c->jpeg_sync_stats.chunk_bytes = (int32_t)C;
        c->jpeg_sync_stats.lanes = kSyncLanes;
    }
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    if (!c->jpeg_host) c->jpeg_host = new JpegHost;
    JpegHost& H = *static_cast<JpegHost*>(c->jpeg_host);
    if ((int)H.parsed.size() < n) H.parsed.resize(n);
    H.msgs.assign(n, std::string());
    H.codes.assign(n, 0);
    H.byte_off.assign(n + 1, 0);
    for (int i = 0; i < n; i++) {
        if (!bufs[i] && lens[i]) return set_err(c, SLAM_E_INVALID_ARG, "null stream");
        H.byte_off[i + 1] = H.byte_off[i] + align_up(lens[i], 16);
    }
    if (H.byte_off[n] >= 0xFFFFFFFFull) return set_err(c, SLAM_E_UNSUPPORTED, "a batch of 4 GiB or more of compressed bytes");

    host_parallel_run(n, [&](int i) {
        jpeg::Parsed& P = H.parsed[i];
        int rc = jpeg::parse(bufs[i], lens[i], channels, P, H.msgs[i], flags);
        if (rc == SLAM_OK && (P.d.width != w || P.d.height != h)) {
            rc = SLAM_E_INVALID_ARG;
            H.msgs[i] = "stream " + std::to_string(i) + " is " + std::to_string(P.d.width) + " x " + std::to_string(P.d.height) +
                        ", the batch " + std::to_string(w) + " x " + std::to_string(h);
        }
        H.codes[i] = rc;
    });

    // layout: descriptors | segments | status | bytes in one staging block; coefficients and planes per image
    size_t nseg = 0, coef_elems = 0, plane_bytes = 0;
    uint32_t max_blocks = 0;
    H.psegs.clear();
    H.porig.clear();
    H.wg_seg.clear();
    if (sync_mode) H.is_par.assign(n, std::vector<uint8_t>());
    std::vector<size_t> seg_first(n + 1, 0);
    for (int i = 0; i < n; i++) {
        jpeg::Parsed& P = H.parsed[i];
        ImageDesc& d = P.d;
        seg_first[i + 1] = seg_first[i];
        if (H.codes[i] != SLAM_OK) {
            std::memset(&d, 0, sizeof(d));
            P.segs.clear();
            continue;
        }
        d.data_off = (uint32_t)H.byte_off[i];
        d.coef_off = coef_elems;
        d.plane_off = plane_bytes;
        coef_elems += (size_t)d.total_blocks * 64;
        plane_bytes += align_up(P.plane_bytes, 256);
        size_t serial = P.segs.size();
        if (sync_mode) {      // which segments take the parallel path: by their bytes alone
            H.is_par[i].assign(P.segs.size(), 0);
            const uint32_t least = sync_mode == 2 ? C + 1 : (jpeg::kSyncAutoBytes > C ? jpeg::kSyncAutoBytes : C + 1);
            for (size_t k = 0; k < P.segs.size(); k++) {
                Segment sg = P.segs[k];
                SyncSeg ss;
                if (sg.end <= sg.off || sg.end - sg.off < least) continue;
                sg.image = (uint32_t)i;
                if (!jpeg::sync_seg_init(ss, d, sg, C)) continue;
                if ((H.wg_seg.size() + (ss.nchunks + kSyncLanes - 1) / kSyncLanes) * (size_t)kSyncLanes > 0x7FFFFFFFull) continue;
                sg.off += d.data_off;
                sg.end += d.data_off;
                ss.off = sg.off;
                ss.end = sg.end;
                ss.chunk0 = (uint32_t)(H.wg_seg.size() * kSyncLanes);
                for (uint32_t g = 0; g < (ss.nchunks + kSyncLanes - 1) / kSyncLanes; g++) H.wg_seg.push_back((uint32_t)H.psegs.size());
                H.psegs.push_back(ss);
                H.porig.push_back(sg);
                H.is_par[i][k] = 1;
                serial--;
            }
        }
        nseg += serial;
        seg_first[i + 1] = nseg;
        if (d.total_blocks > max_blocks) max_blocks = d.total_blocks;
    }
    if (nseg > 0x7FFFFFFFull) return set_err(c, SLAM_E_UNSUPPORTED, "too many restart intervals");
    const size_t nps = H.psegs.size(), nwg = H.wg_seg.size();
    const size_t o_desc = 0, o_segs = align_up((size_t)n * sizeof(ImageDesc), 256);
    const size_t o_stat = o_segs + align_up(nseg * sizeof(Segment), 256);
    const size_t o_bytes = o_stat + align_up((size_t)n * sizeof(int32_t), 256);
    // behind the bytes, only when segments take the parallel path: their table, their workgroups, and
    // room for the list of those that fall back (the segments they were, then their indices)
    const size_t o_psegs = o_bytes + (nps ? align_up(H.byte_off[n], 256) : H.byte_off[n]);
    const size_t o_wgseg = o_psegs + align_up(nps * sizeof(SyncSeg), 256);
    const size_t o_fb = o_wgseg + align_up(nwg * sizeof(uint32_t), 256);
    const size_t in_bytes = o_fb;
    const size_t all_bytes = o_fb + align_up(nps * (sizeof(Segment) + sizeof(uint32_t)), 256);
    if (c->h_jpeg_bytes < all_bytes) {
        if (c->h_jpeg) (void)hipHostFree(c->h_jpeg);
        c->h_jpeg = nullptr;
        c->h_jpeg_bytes = 0;
        const size_t want = align_up(all_bytes + all_bytes / 4, 1 << 20);
        SLAM_HIP(c, hipHostMalloc(&c->h_jpeg, want, hipHostMallocDefault));
        c->h_jpeg_bytes = want;
    }
    SLAM_HIP(c, c->jpeg_in.ensure(all_bytes));
    SLAM_HIP(c, c->jpeg_coef.ensure(coef_elems * sizeof(int16_t) + 16));
    SLAM_HIP(c, c->jpeg_planes.ensure(plane_bytes + 16));
    if (int rc = jpeg_events(c)) return rc;

    uint8_t* hs = static_cast<uint8_t*>(c->h_jpeg);
    ImageDesc* h_desc = reinterpret_cast<ImageDesc*>(hs + o_desc);
    Segment* h_segs = reinterpret_cast<Segment*>(hs + o_segs);
    int32_t* h_stat = reinterpret_cast<int32_t*>(hs + o_stat);
    const auto t1 = clk::now();
    host_parallel_run(n, [&](int i) {
        const jpeg::Parsed& P = H.parsed[i];
        h_desc[i] = P.d;
        h_stat[i] = H.codes[i] == SLAM_OK ? P.status0 : 0;
        Segment* sg = h_segs + seg_first[i];
        for (size_t k = 0; k < P.segs.size(); k++) {
            if (sync_mode && H.codes[i] == SLAM_OK && H.is_par[i][k]) continue;
            *sg = P.segs[k];
            sg->image = (uint32_t)i;
            sg->off += P.d.data_off;
            sg->end += P.d.data_off;
            sg++;
        }
        if (H.codes[i] == SLAM_OK) std::memcpy(hs + o_bytes + H.byte_off[i], bufs[i], lens[i]);
    });

    if (nps) {
        std::memcpy(hs + o_psegs, H.psegs.data(), nps * sizeof(SyncSeg));
        std::memcpy(hs + o_wgseg, H.wg_seg.data(), nwg * sizeof(uint32_t));
    }
    uint8_t* din = c->jpeg_in.as<uint8_t>();
    const ImageDesc* d_desc = reinterpret_cast<const ImageDesc*>(din + o_desc);
    const Segment* d_segs = reinterpret_cast<const Segment*>(din + o_segs);
    int32_t* d_stat = reinterpret_cast<int32_t*>(din + o_stat);
    SLAM_HIP(c, hipEventRecord(c->jpeg_ev[0], s));
    SLAM_HIP(c, hipMemcpyAsync(din, hs, in_bytes, hipMemcpyHostToDevice, s));
    SLAM_HIP(c, hipEventRecord(c->jpeg_ev[1], s));
    if (coef_elems) SLAM_HIP(c, hipMemsetAsync(c->jpeg_coef.p, 0, coef_elems * sizeof(int16_t), s));
    if (nseg) {
        const int lanes = jpeg_lanes(c, (int)nseg);
        const int grid = ((int)nseg + lanes - 1) / lanes;
        jpeg_huff<<<grid, 64, 0, s>>>(d_desc, d_segs, (int)nseg, lanes, din + o_bytes, c->jpeg_coef.as<int16_t>(), d_stat);
        SLAM_HIP(c, hipGetLastError());
    }
    if (nps) {
        if (int rc = sync_segments(c, s, H, C, din, o_bytes, o_psegs, o_wgseg, o_fb, d_desc, d_stat)) return rc;
    }
    SLAM_HIP(c, hipEventRecord(c->jpeg_ev[2], s));
    if (max_blocks) {
        jpeg_idct<<<dim3((max_blocks + kIdctBlocks - 1) / kIdctBlocks, n), kIdctBlocks * 8, 0, s>>>(
            d_desc, c->jpeg_coef.as<int16_t>(), c->jpeg_planes.as<uint8_t>());
        SLAM_HIP(c, hipGetLastError());
    }
    SLAM_HIP(c, hipEventRecord(c->jpeg_ev[3], s));
    jpeg_upcolor<<<dim3(((w + 3) / 4 + 63) / 64, (h + 3) / 4, n), dim3(64, 4), 0, s>>>(d_desc, c->jpeg_planes.as<uint8_t>(),
                                                                                      d_out, w, h, channels);
    SLAM_HIP(c, hipGetLastError());
    SLAM_HIP(c, hipEventRecord(c->jpeg_ev[4], s));
    int32_t* rb = static_cast<int32_t*>(readback(c, (size_t)n * sizeof(int32_t)));
    if (!rb) return set_err(c, SLAM_E_HIP, "pinned readback allocation failed");
    SLAM_HIP(c, hipMemcpyAsync(rb, d_stat, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (int rc = stream_sync(c, s)) return rc;
    c->err.clear();
    for (int i = 0; i < n; i++) {
        status[i] = H.codes[i] != SLAM_OK ? H.codes[i] : rb[i];
        if (H.codes[i] != SLAM_OK && c->err.empty()) c->err = H.msgs[i];
    }
    float ms = 0.f;
    c->jpeg_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    for (int k = 0; k < 4; k++) {
        SLAM_HIP(c, hipEventElapsedTime(&ms, c->jpeg_ev[k], c->jpeg_ev[k + 1]));
        c->jpeg_ms[k + 1] = ms;
    }
    if (nps) {
        SLAM_HIP(c, hipEventElapsedTime(&ms, c->jpeg_sync_ev[5], c->jpeg_sync_ev[6]));
        c->jpeg_sync_stats.ms[4] = ms;
    }
    c->jpeg_bytes[0] = H.byte_off[n];
    c->jpeg_bytes[1] = o_bytes;
    c->jpeg_bytes[2] = coef_elems * sizeof(int16_t);
    c->jpeg_bytes[3] = (uint64_t)n * h * w * channels;
    c->jpeg_timed = true;
    return SLAM_OK;
}

}  // namespace

void jpeg_release(slam_ctx* c)
{
    delete static_cast<JpegHost*>(c->jpeg_host);
    c->jpeg_host = nullptr;
    if (c->h_jpeg) (void)hipHostFree(c->h_jpeg);
    c->h_jpeg = nullptr;
    for (hipEvent_t& e : c->jpeg_ev)
        if (e) {
            (void)hipEventDestroy(e);
            e = nullptr;
        }
    for (hipEvent_t& e : c->jpeg_sync_ev)
        if (e) {
            (void)hipEventDestroy(e);
            e = nullptr;
        }
}

}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_jpeg_decode_batch_dev(slam_ctx* c, void* stream, const uint8_t* const* bufs, const size_t* lens, int n,
                                          int w, int h, uint8_t* d_frames, int* status)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!bufs || !lens || n <= 0 || !d_frames || !status) return set_err(c, SLAM_E_INVALID_ARG, "null argument or empty batch");
    if (w < 1 || h < 1 || w > jpeg::kMaxDim || h > jpeg::kMaxDim) return set_err(c, SLAM_E_INVALID_ARG, "frame size outside 1 .. 16384");
    if (n > 65535) return set_err(c, SLAM_E_INVALID_ARG, "more than 65535 streams in a batch");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    return decode_batch(c, s, bufs, lens, n, w, h, 3, d_frames, status);
}

extern "C" int slam_jpeg_decode_batch_dev_ex(slam_ctx* c, void* stream, const uint8_t* const* bufs, const size_t* lens, int n,
                                             int w, int h, uint8_t* d_frames, int* status, int flags)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!bufs || !lens || n <= 0 || !d_frames || !status) return set_err(c, SLAM_E_INVALID_ARG, "null argument or empty batch");
    if (w < 1 || h < 1 || w > jpeg::kMaxDim || h > jpeg::kMaxDim) return set_err(c, SLAM_E_INVALID_ARG, "frame size outside 1 .. 16384");
    if (n > 65535) return set_err(c, SLAM_E_INVALID_ARG, "more than 65535 streams in a batch");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    return decode_batch(c, s, bufs, lens, n, w, h, 3, d_frames, status, flags);
}

extern "C" int slam_jpeg_last_sync(slam_ctx* c, struct slam_jpeg_sync_stats* stats)
{
    if (!c || !stats) return SLAM_E_INVALID_ARG;
    if (!c->jpeg_timed) return set_err(c, SLAM_E_INVALID_ARG, "no slam_jpeg_decode_batch_dev call to report");
    *stats = c->jpeg_sync_stats;
    return SLAM_OK;
}

extern "C" int slam_jpeg_decode(slam_ctx* c, const uint8_t* buf, size_t len, uint8_t* out, size_t step, int channels,
                                int* status)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (status) *status = 0;
    if (!out) return set_err(c, SLAM_E_INVALID_ARG, "null output");
    struct slam_jpeg_info info;
    int rc = slam_jpeg_info(buf, len, &info);
    if (rc != SLAM_OK) return set_err(c, rc, slam_jpeg_last_error());
    if (channels != 1 && channels != 3) return set_err(c, SLAM_E_INVALID_ARG, "channels must be 1 or 3");
    const size_t row = (size_t)info.width * channels;
    if (step < row) return set_err(c, SLAM_E_INVALID_ARG, "step smaller than a row");
    SLAM_HIP(c, hipSetDevice(c->device));
    SLAM_HIP(c, c->jpeg_out.ensure(row * info.height + 16));
    int st = 0;
    rc = decode_batch(c, c->stream, &buf, &len, 1, info.width, info.height, channels, c->jpeg_out.as<uint8_t>(), &st);
    if (rc != SLAM_OK) return rc;
    if (st < 0) return st;      // the message is the context's
    SLAM_HIP(c, hipMemcpy2D(out, step, c->jpeg_out.p, row, row, info.height, hipMemcpyDeviceToHost));
    if (status) *status = st;
    return SLAM_OK;
}

extern "C" int slam_jpeg_last_orientations(slam_ctx* c, int32_t* out, int n)
{
    if (!c || !out || n < 0) return SLAM_E_INVALID_ARG;
    const JpegHost* H = static_cast<const JpegHost*>(c->jpeg_host);
    if (!H || (int)H->codes.size() != n) return set_err(c, SLAM_E_INVALID_ARG, "n is not the size of the context's last JPEG batch");
    for (int i = 0; i < n; i++) out[i] = H->codes[i] == SLAM_OK ? H->parsed[i].orientation : 1;
    return SLAM_OK;
}

extern "C" int slam_jpeg_last_timing(slam_ctx* c, double* ms5, uint64_t* bytes4)
{
    if (!c || !ms5) return SLAM_E_INVALID_ARG;
    if (!c->jpeg_timed) return set_err(c, SLAM_E_INVALID_ARG, "no slam_jpeg_decode_batch_dev call to report");
    for (int k = 0; k < 5; k++) ms5[k] = c->jpeg_ms[k];
    if (bytes4)
        for (int k = 0; k < 4; k++) bytes4[k] = c->jpeg_bytes[k];
    return SLAM_OK;
}

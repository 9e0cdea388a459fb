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

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct JpegHost {
    std::vector<jpeg::Parsed> parsed;
    std::vector<std::string> msgs;
    std::vector<int> codes;
    std::vector<size_t> byte_off;
};

int jpeg_events(slam_ctx* c)
{
    for (hipEvent_t& e : c->jpeg_ev)
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

// n streams decoded into d_out (n x h x w x channels, device) on s; status: host, n.  w, h: the size
// every stream must have.  Synchronous.
int decode_batch(slam_ctx* c, hipStream_t s, const uint8_t* const* bufs, const size_t* lens, int n, int w, int h,
                 int channels, uint8_t* d_out, int* status)
{
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
        int rc = jpeg::parse(bufs[i], lens[i], channels, P, H.msgs[i]);
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
    for (int i = 0; i < n; i++) {
        jpeg::Parsed& P = H.parsed[i];
        ImageDesc& d = P.d;
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
        nseg += P.segs.size();
        if (d.total_blocks > max_blocks) max_blocks = d.total_blocks;
    }
    if (nseg > 0x7FFFFFFFull) return set_err(c, SLAM_E_UNSUPPORTED, "too many restart intervals");
    const size_t o_desc = 0, o_segs = align_up((size_t)n * sizeof(ImageDesc), 256);
    const size_t o_stat = o_segs + align_up(nseg * sizeof(Segment), 256);
    const size_t o_bytes = o_stat + align_up((size_t)n * sizeof(int32_t), 256);
    const size_t in_bytes = o_bytes + H.byte_off[n];
    if (c->h_jpeg_bytes < in_bytes) {
        if (c->h_jpeg) (void)hipHostFree(c->h_jpeg);
        c->h_jpeg = nullptr;
        c->h_jpeg_bytes = 0;
        const size_t want = align_up(in_bytes + in_bytes / 4, 1 << 20);
        SLAM_HIP(c, hipHostMalloc(&c->h_jpeg, want, hipHostMallocDefault));
        c->h_jpeg_bytes = want;
    }
    SLAM_HIP(c, c->jpeg_in.ensure(in_bytes));
    SLAM_HIP(c, c->jpeg_coef.ensure(coef_elems * sizeof(int16_t) + 16));
    SLAM_HIP(c, c->jpeg_planes.ensure(plane_bytes + 16));
    if (int rc = jpeg_events(c)) return rc;

    uint8_t* hs = static_cast<uint8_t*>(c->h_jpeg);
    ImageDesc* h_desc = reinterpret_cast<ImageDesc*>(hs + o_desc);
    Segment* h_segs = reinterpret_cast<Segment*>(hs + o_segs);
    int32_t* h_stat = reinterpret_cast<int32_t*>(hs + o_stat);
    std::vector<size_t> seg_first(n + 1, 0);
    for (int i = 0; i < n; i++) seg_first[i + 1] = seg_first[i] + H.parsed[i].segs.size();
    const auto t1 = clk::now();
    host_parallel_run(n, [&](int i) {
        const jpeg::Parsed& P = H.parsed[i];
        h_desc[i] = P.d;
        h_stat[i] = H.codes[i] == SLAM_OK ? P.status0 : 0;
        Segment* sg = h_segs + seg_first[i];
        for (size_t k = 0; k < P.segs.size(); k++) {
            sg[k] = P.segs[k];
            sg[k].image = (uint32_t)i;
            sg[k].off += P.d.data_off;
            sg[k].end += P.d.data_off;
        }
        if (H.codes[i] == SLAM_OK) std::memcpy(hs + o_bytes + H.byte_off[i], bufs[i], lens[i]);
    });

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

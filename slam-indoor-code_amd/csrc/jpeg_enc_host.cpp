// Baseline JPEG encoding on the host: the setup the device
// path shares (geometry, quality-scaled tables, Huffman code tables, markers) and
// slam_jpeg_encode_host, the whole encoder over jpeg_enc_math.h.  No HIP.
#include "jpeg_enc_host.h"

#include <cstring>
#include <vector>

#include "../../include/slamhip.h"
#include "jpeg_parse.h"

namespace jpeg {

namespace {

// Annex K.1, natural order
const uint8_t kQuantLum[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                               14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                               18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kQuantChr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                               99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                               99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

void put16(uint8_t*& p, unsigned v)
{
    *p++ = (uint8_t)(v >> 8);
    *p++ = (uint8_t)v;
}

// bytes with FF 00 stuffing into a buffer of cap bytes: counts every byte, writes those that fit
struct HostSink {
    uint8_t* out;
    size_t cap, pos = 0;
    uint64_t acc = 0;
    int n = 0;
    void byte(uint8_t b)
    {
        if (pos < cap) out[pos] = b;
        pos++;
    }
    void put(uint32_t code, int len)
    {
        acc = (acc << len) | code;
        n += len;
        while (n >= 8) {
            const uint8_t b = (uint8_t)(acc >> (n - 8));
            byte(b);
            if (b == 0xFF) byte(0);
            n -= 8;
        }
        acc &= (1ull << n) - 1ull;
    }
    void flush()
    {
        if (n) put((1u << (8 - n)) - 1u, 8 - n);
    }
};

}  // namespace

int enc_setup(int h, int w, int channels, size_t row_step, size_t frame_step, int quality, int sampling,
              int restart_interval, EncGeom& g, EncTables& T, std::string& msg)
{
    if (w < 1 || h < 1 || w > kMaxDim || h > kMaxDim) return msg = "frame size outside 1 .. 16384", SLAM_E_INVALID_ARG;
    if (channels != 1 && channels != 3) return msg = "channels must be 1 or 3", SLAM_E_INVALID_ARG;
    if (row_step < (size_t)w * channels) return msg = "step smaller than a row", SLAM_E_INVALID_ARG;
    if (restart_interval < 0 || restart_interval > 65535) return msg = "restart interval outside 0 .. 65535", SLAM_E_INVALID_ARG;
    if (sampling != SLAM_JPEG_GRAY && sampling != SLAM_JPEG_444 && sampling != SLAM_JPEG_422 && sampling != SLAM_JPEG_420)
        return msg = "sampling is not one of SLAM_JPEG_GRAY, _444, _422, _420", SLAM_E_INVALID_ARG;
    if (channels == 1) sampling = SLAM_JPEG_GRAY;
    std::memset(&g, 0, sizeof(g));
    g.w = w;
    g.h = h;
    g.channels = channels;
    g.ncomp = sampling == SLAM_JPEG_GRAY ? 1 : 3;
    g.hs = g.ncomp == 1 ? 1 : sampling >> 4;
    g.vs = g.ncomp == 1 ? 1 : sampling & 15;
    g.mcux = (w + 8 * g.hs - 1) / (8 * g.hs);
    g.mcuy = (h + 8 * g.vs - 1) / (8 * g.vs);
    g.bpm = g.hs * g.vs + (g.ncomp == 3 ? 2 : 0);
    g.bw[0] = (w + 7) / 8;
    g.bh[0] = (h + 7) / 8;
    g.bw[1] = g.bw[2] = ((w + g.hs - 1) / g.hs + 7) / 8;
    g.bh[1] = g.bh[2] = ((h + g.vs - 1) / g.vs + 7) / 8;
    g.nmcu = (uint32_t)g.mcux * (uint32_t)g.mcuy;
    g.ri = restart_interval ? (uint32_t)restart_interval : g.nmcu;
    g.nint = (g.nmcu + g.ri - 1) / g.ri;
    g.row_step = row_step;
    g.frame_step = frame_step;

    const int q = quality < 1 ? 1 : quality > 100 ? 100 : quality;      // jpeg_quality_scaling
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int t = 0; t < 2; t++)
        for (int i = 0; i < 64; i++) {
            const int v = ((t ? kQuantChr : kQuantLum)[i] * scale + 50) / 100;
            T.quant[t][i] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);      // force_baseline
        }
    std::memset(T.dc_code, 0, sizeof(T.dc_code));
    std::memset(T.dc_len, 0, sizeof(T.dc_len));
    std::memset(T.ac_code, 0, sizeof(T.ac_code));
    std::memset(T.ac_len, 0, sizeof(T.ac_len));
    for (int klass = 0; klass < 2; klass++)
        for (int t = 0; t < 2; t++) {
            const uint8_t *counts, *vals;
            int nv;
            std_huff_table(klass, t, &counts, &vals, &nv);
            unsigned code = 0;
            int k = 0;
            for (int len = 1; len <= 16; len++) {      // Annex C
                for (int i = 0; i < counts[len - 1] && k < nv; i++, k++, code++) {
                    if (klass == 0) {
                        T.dc_code[t][vals[k] & 15] = (uint16_t)code;
                        T.dc_len[t][vals[k] & 15] = (uint8_t)len;
                    } else {
                        T.ac_code[t][vals[k]] = (uint16_t)code;
                        T.ac_len[t][vals[k]] = (uint8_t)len;
                    }
                }
                code <<= 1;
            }
        }
    return SLAM_OK;
}

size_t enc_header(const EncGeom& g, const EncTables& T, int restart_interval, uint8_t* out)
{
    uint8_t* p = out;
    put16(p, 0xFFD8);
    put16(p, 0xFFE0);
    put16(p, 16);
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    std::memcpy(p, jfif, 14);
    p += 14;
    const int ntab = g.ncomp == 3 ? 2 : 1;
    for (int t = 0; t < ntab; t++) {
        put16(p, 0xFFDB);
        put16(p, 67);
        *p++ = (uint8_t)t;
        for (int k = 0; k < 64; k++) *p++ = (uint8_t)T.quant[t][zigzag_natural(k)];
    }
    put16(p, 0xFFC0);
    put16(p, 8 + 3 * g.ncomp);
    *p++ = 8;
    put16(p, (unsigned)g.h);
    put16(p, (unsigned)g.w);
    *p++ = (uint8_t)g.ncomp;
    for (int c = 0; c < g.ncomp; c++) {
        *p++ = (uint8_t)(c + 1);
        *p++ = (uint8_t)(c == 0 ? (g.hs << 4 | g.vs) : 0x11);
        *p++ = (uint8_t)(c ? 1 : 0);
    }
    for (int t = 0; t < ntab; t++)
        for (int klass = 0; klass < 2; klass++) {
            const uint8_t *counts, *vals;
            int nv;
            std_huff_table(klass, t, &counts, &vals, &nv);
            put16(p, 0xFFC4);
            put16(p, (unsigned)(19 + nv));
            *p++ = (uint8_t)(klass << 4 | t);
            std::memcpy(p, counts, 16);
            p += 16;
            std::memcpy(p, vals, (size_t)nv);
            p += nv;
        }
    if (restart_interval) {
        put16(p, 0xFFDD);
        put16(p, 4);
        put16(p, (unsigned)restart_interval);
    }
    put16(p, 0xFFDA);
    put16(p, 6 + 2 * g.ncomp);
    *p++ = (uint8_t)g.ncomp;
    for (int c = 0; c < g.ncomp; c++) {
        *p++ = (uint8_t)(c + 1);
        *p++ = (uint8_t)(c ? 0x11 : 0);
    }
    *p++ = 0;
    *p++ = 63;
    *p++ = 0;
    return (size_t)(p - out);
}

size_t enc_bound(const EncGeom& g)
{
    const uint64_t blocks = (uint64_t)g.nmcu * (uint64_t)g.bpm;
    const uint64_t scan = (blocks * kEncMaxBlockBits + 7) / 8 + g.nint;      // a padding byte per interval at the most
    return (size_t)(kEncHeaderMax + 2 * scan + 2 * (uint64_t)g.nint + 2);
}

}  // namespace jpeg

namespace {
thread_local std::string g_enc_err;
}

extern "C" const char* slam_jpeg_enc_last_error(void) { return g_enc_err.c_str(); }

extern "C" size_t slam_jpeg_encode_bound(int h, int w, int sampling, int restart_interval)
{
    jpeg::EncGeom g;
    jpeg::EncTables T;
    if (jpeg::enc_setup(h, w, 3, (size_t)w * 3, 0, 95, sampling, restart_interval, g, T, g_enc_err) != SLAM_OK) return 0;
    return jpeg::enc_bound(g);
}

extern "C" int slam_jpeg_encode_host(const uint8_t* img, int h, int w, int channels, size_t row_step, int quality,
                                     int sampling, int restart_interval, uint8_t* out, size_t cap, size_t* size,
                                     int* status)
{
    if (size) *size = 0;
    if (status) *status = 0;
    if (!img || !size || (!out && cap)) return g_enc_err = "null argument", SLAM_E_INVALID_ARG;
    jpeg::EncGeom g;
    jpeg::EncTables T;
    if (int rc = jpeg::enc_setup(h, w, channels, row_step, 0, quality, sampling, restart_interval, g, T, g_enc_err)) return rc;
    uint8_t hdr[jpeg::kEncHeaderMax];
    const size_t nh = jpeg::enc_header(g, T, restart_interval, hdr);
    jpeg::HostSink s{out, cap};
    for (size_t i = 0; i < nh; i++) s.byte(hdr[i]);
    int st = 0, pred[3] = {0, 0, 0};
    std::vector<int16_t> coef((size_t)g.bpm * 64);
    for (uint32_t m = 0; m < g.nmcu; m++) {
        if (m && m % g.ri == 0) {
            s.flush();
            s.byte(0xFF);
            s.byte((uint8_t)(0xD0 + ((m / g.ri - 1) & 7)));
            pred[0] = pred[1] = pred[2] = 0;
        }
        const int mx = (int)(m % (uint32_t)g.mcux), my = (int)(m / (uint32_t)g.mcux);
        for (int k = 0; k < g.bpm; k++) {
            int c, col, row;
            if (jpeg::enc_block_pos(g, k, mx, my, c, col, row)) jpeg::enc_block_coef(img, g, T, c, col, row, coef.data() + (size_t)k * 64);
        }
        st |= jpeg::enc_mcu(s, g, T, m, coef.data(), pred);
    }
    s.flush();
    s.byte(0xFF);
    s.byte(0xD9);
    *size = s.pos;
    if (s.pos > cap) st |= jpeg::kEncOverflow;
    if (status) *status = st;
    return SLAM_OK;
}

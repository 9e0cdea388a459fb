// Baseline JPEG: marker parsing, validation and the segment table (host), and
// slam_jpeg_info / slam_jpeg_decode_host, the whole decoder on the host through
// the headers the kernels use (jpeg_huff.h, jpeg_pix.h).  Plain C++: no HIP.
#include "jpeg_parse.h"

#include <cstring>

#include "../../include/slamhip.h"

namespace jpeg {

namespace {

inline unsigned be16(const uint8_t* p) { return ((unsigned)p[0] << 8) | p[1]; }

// APP1 "Exif\0\0" + TIFF: IFD0's orientation (SHORT, tag 0x0112); 1 when absent or malformed
int exif_orientation(const uint8_t* p, size_t n)
{
    if (n < 14 || std::memcmp(p, "Exif\0\0", 6) != 0) return 0;
    const uint8_t* t = p + 6;
    const size_t tn = n - 6;
    bool le;
    if (t[0] == 'I' && t[1] == 'I') le = true;
    else if (t[0] == 'M' && t[1] == 'M') le = false;
    else return 0;
    auto r16 = [&](size_t o) -> unsigned { return le ? t[o] | (t[o + 1] << 8) : (t[o] << 8) | t[o + 1]; };
    auto r32 = [&](size_t o) -> uint32_t {
        return le ? (uint32_t)t[o] | ((uint32_t)t[o + 1] << 8) | ((uint32_t)t[o + 2] << 16) | ((uint32_t)t[o + 3] << 24)
                  : ((uint32_t)t[o] << 24) | ((uint32_t)t[o + 1] << 16) | ((uint32_t)t[o + 2] << 8) | (uint32_t)t[o + 3];
    };
    if (r16(2) != 42) return 0;
    const uint32_t ifd = r32(4);
    if (ifd > tn || tn - ifd < 2) return 0;
    const unsigned cnt = r16(ifd);
    for (unsigned i = 0; i < cnt; i++) {
        const size_t e = (size_t)ifd + 2 + (size_t)i * 12;
        if (e + 12 > tn) return 0;
        if (r16(e) == 0x0112) {
            if (r16(e + 2) != 3 || r32(e + 4) != 1) return 0;
            const unsigned v = r16(e + 8);
            return v >= 1 && v <= 8 ? (int)v : 0;
        }
    }
    return 0;
}

const char* sof_name(int m)
{
    switch (m) {
    case 0xC1: return "SOF1 (extended sequential)";
    case 0xC2: return "SOF2 (progressive)";
    case 0xC3: return "SOF3 (lossless)";
    case 0xC5: case 0xC6: case 0xC7: return "a differential frame (SOF5-7)";
    default: return "arithmetic coding (SOF9-15)";
    }
}

}  // namespace

int parse(const uint8_t* buf, size_t len, int channels, Parsed& P, std::string& msg)
{
    P.segs.clear();
    P.restart = 0;
    P.orientation = 1;
    P.status0 = 0;
    P.plane_bytes = 0;
    ImageDesc& d = P.d;
    std::memset(&d, 0, sizeof(d));      // valid = 0, no table defined
    if (channels != 1 && channels != 3) return msg = "channels must be 1 or 3", SLAM_E_INVALID_ARG;
    if (!buf || len < 4 || buf[0] != 0xFF || buf[1] != 0xD8) return msg = "no SOI: not a JPEG stream", SLAM_E_INVALID_ARG;
    if (len >= 0x7FFFFFFFu) return msg = "stream of 2 GiB or more", SLAM_E_UNSUPPORTED;

    uint16_t qt[4][64];
    bool qt_def[4] = {false, false, false, false};
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = -1;
    int ncomp = 0, cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
    int width = 0, height = 0;
    size_t pos = 2, scan_off = 0;

    for (;;) {
        // the next marker: FF, any number of fill FFs, a code
        while (pos < len && buf[pos] != 0xFF) pos++;
        while (pos < len && buf[pos] == 0xFF) pos++;
        if (pos >= len) return msg = "no scan (SOS) before the end of the stream", SLAM_E_INVALID_ARG;
        const int m = buf[pos++];
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;      // stand-alone markers
        if (m == 0xD9) return msg = "EOI before any scan", SLAM_E_INVALID_ARG;
        if (len - pos < 2) return msg = "segment length past the end of the stream", SLAM_E_INVALID_ARG;
        const size_t L = be16(buf + pos);
        if (L < 2 || L > len - pos) return msg = "segment length past the end of the stream", SLAM_E_INVALID_ARG;
        const uint8_t* s = buf + pos + 2;
        const size_t n = L - 2;
        pos += L;

        if (m == 0xC0) {
            if (have_sof) return msg = "two frame headers", SLAM_E_INVALID_ARG;
            if (n < 6) return msg = "short SOF0", SLAM_E_INVALID_ARG;
            if (s[0] != 8) return msg = "sample precision " + std::to_string(s[0]) + " (only 8-bit)", SLAM_E_UNSUPPORTED;
            height = (int)be16(s + 1);
            width = (int)be16(s + 3);
            ncomp = s[5];
            if (width == 0) return msg = "zero width", SLAM_E_INVALID_ARG;
            if (height == 0) return msg = "height left to a DNL marker", SLAM_E_UNSUPPORTED;
            if (width > kMaxDim || height > kMaxDim)
                return msg = "dimensions " + std::to_string(width) + " x " + std::to_string(height) + " above 16384", SLAM_E_UNSUPPORTED;
            if (ncomp != 1 && ncomp != 3)
                return msg = std::to_string(ncomp) + " components (only 1 or 3)", ncomp == 0 ? SLAM_E_INVALID_ARG : SLAM_E_UNSUPPORTED;
            if (n < 6 + (size_t)3 * ncomp) return msg = "short SOF0", SLAM_E_INVALID_ARG;
            for (int c = 0; c < ncomp; c++) {
                cid[c] = s[6 + 3 * c];
                ch[c] = s[7 + 3 * c] >> 4;
                cv[c] = s[7 + 3 * c] & 15;
                ctq[c] = s[8 + 3 * c];
                if (ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4) return msg = "sampling factor outside 1 .. 4", SLAM_E_INVALID_ARG;
                if (ctq[c] > 3) return msg = "quantisation table index above 3", SLAM_E_INVALID_ARG;
            }
            have_sof = true;
        } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return msg = std::string(sof_name(m)) + ": only baseline SOF0 is decoded", SLAM_E_UNSUPPORTED;
        } else if (m == 0xCC) {
            return msg = "arithmetic coding (DAC)", SLAM_E_UNSUPPORTED;
        } else if (m == 0xC4) {
            size_t o = 0;
            while (o < n) {
                if (n - o < 17) return msg = "short DHT", SLAM_E_INVALID_ARG;
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return msg = "DHT class or index out of range", SLAM_E_INVALID_ARG;
                int total = 0;
                for (int i = 0; i < 16; i++) total += s[o + 1 + i];
                if (total > 256) return msg = "DHT with more than 256 symbols", SLAM_E_INVALID_ARG;
                if (n - o - 17 < (size_t)total) return msg = "short DHT", SLAM_E_INVALID_ARG;
                if (!huff_build(d.tables[tc * 4 + th], s + o + 1, s + o + 17, total))
                    return msg = "DHT whose counts oversubscribe the code space", SLAM_E_INVALID_ARG;
                o += 17 + (size_t)total;
            }
        } else if (m == 0xDB) {
            size_t o = 0;
            while (o < n) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (tq > 3) return msg = "DQT index above 3", SLAM_E_INVALID_ARG;
                if (pq == 1) return msg = "16-bit quantisation table (Pq = 1)", SLAM_E_UNSUPPORTED;
                if (pq != 0) return msg = "DQT precision out of range", SLAM_E_INVALID_ARG;
                if (n - o < 65) return msg = "short DQT", SLAM_E_INVALID_ARG;
                for (int i = 0; i < 64; i++) qt[tq][zigzag_natural(i)] = s[o + 1 + i];
                qt_def[tq] = true;
                o += 65;
            }
        } else if (m == 0xDD) {
            if (n < 2) return msg = "short DRI", SLAM_E_INVALID_ARG;
            P.restart = (int)be16(s);
        } else if (m == 0xE0) {
            if (n >= 5 && std::memcmp(s, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xE1) {
            const int o = exif_orientation(s, n);
            if (o) P.orientation = o;
        } else if (m == 0xEE) {
            if (n >= 12 && std::memcmp(s, "Adobe", 5) == 0) {
                adobe = true;
                adobe_transform = s[11];
            }
        } else if (m == 0xDA) {
            if (!have_sof) return msg = "scan before the frame header", SLAM_E_INVALID_ARG;
            if (n < 1) return msg = "short SOS", SLAM_E_INVALID_ARG;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || n < (size_t)1 + 2 * ns + 3) return msg = "short SOS", SLAM_E_INVALID_ARG;
            if (ns != ncomp) return msg = "non-interleaved scan (a scan of " + std::to_string(ns) + " of " + std::to_string(ncomp) + " components)", SLAM_E_UNSUPPORTED;
            for (int c = 0; c < ns; c++) {
                if (s[1 + 2 * c] != cid[c]) return msg = "scan components not in the frame's order", SLAM_E_INVALID_ARG;
                const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 3 || ta > 3) return msg = "scan table index above 3", SLAM_E_INVALID_ARG;
                if (!d.tables[td].defined || !d.tables[4 + ta].defined)
                    return msg = "scan references a Huffman table that was never defined", SLAM_E_INVALID_ARG;
                if (!qt_def[ctq[c]]) return msg = "frame references a quantisation table that was never defined", SLAM_E_INVALID_ARG;
                d.comp[c].dc = td;
                d.comp[c].ac = ta;
            }
            const uint8_t* sp = s + 1 + 2 * ns;
            if (sp[0] != 0 || sp[1] != 63 || sp[2] != 0) return msg = "spectral selection or successive approximation in a baseline scan", SLAM_E_INVALID_ARG;
            scan_off = pos;
            break;
        }
        // every other segment (APPn, COM, ...) is skipped
    }

    // colour space: libjpeg's default_decompress_parms
    if (ncomp == 3) {
        bool rgb = false;
        if (jfif) rgb = false;
        else if (adobe) rgb = adobe_transform == 0;
        else rgb = cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B';
        if (rgb) return msg = "RGB-coded stream (no YCbCr transform)", SLAM_E_UNSUPPORTED;
        const bool ok = ch[1] == 1 && cv[1] == 1 && ch[2] == 1 && cv[2] == 1 &&
                        ((ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2));
        if (!ok) {
            msg = "sampling";
            for (int c = 0; c < 3; c++) msg += " " + std::to_string(ch[c]) + "x" + std::to_string(cv[c]);
            return msg += " (only 4:4:4, 4:2:2 and 4:2:0)", SLAM_E_UNSUPPORTED;
        }
    } else {
        ch[0] = cv[0] = 1;      // a one-component scan is never interleaved: one block per MCU
    }

    d.ncomp = ncomp;
    d.width = width;
    d.height = height;
    d.sampling = ncomp == 1 ? kGray : (ch[0] << 4) | cv[0];
    d.out_channels = channels;
    d.mcus_x = (width + 8 * ch[0] - 1) / (8 * ch[0]);
    d.mcus_y = (height + 8 * cv[0] - 1) / (8 * cv[0]);
    d.data_off = 0;
    d.coef_off = 0;
    d.plane_off = 0;
    uint32_t blocks = 0, plane = 0;
    for (int c = 0; c < 3; c++) {
        ScanComp& sc = d.comp[c];
        if (c >= ncomp) {
            sc = ScanComp{0, 0, 0, 0, 0, 0, 0};
            d.plane_comp[c] = 0;
            std::memset(d.quant[c], 0, sizeof(d.quant[c]));
            continue;
        }
        sc.h = ch[c];
        sc.v = cv[c];
        sc.bw = d.mcus_x * ch[c];
        sc.bh = d.mcus_y * cv[c];
        sc.coef_block = blocks;
        d.plane_comp[c] = plane;
        blocks += (uint32_t)sc.bw * (uint32_t)sc.bh;
        plane += (uint32_t)sc.bw * (uint32_t)sc.bh * 64u;
        std::memcpy(d.quant[c], qt[ctq[c]], sizeof(d.quant[c]));
    }
    d.total_blocks = blocks;
    P.plane_bytes = plane;

    // the segment table: the scan is cut at every RSTn and ends at the first other marker
    const uint32_t total = (uint32_t)d.mcus_x * (uint32_t)d.mcus_y;
    const uint32_t R = (uint32_t)P.restart;
    const uint32_t expected = R ? (total + R - 1) / R : 1;
    uint32_t start = (uint32_t)scan_off, k = 0;
    bool bad = false;
    auto close = [&](uint32_t end) {
        if (k < expected) {
            const uint32_t mcu0 = R ? k * R : 0;
            P.segs.push_back(Segment{0, start, end, mcu0, R ? (total - mcu0 < R ? total - mcu0 : R) : total});
        } else {
            bad = true;
        }
        k++;
    };
    size_t i = scan_off;
    while (i < len) {
        if (buf[i] != 0xFF) { i++; continue; }
        if (i + 1 >= len) { i = len; break; }
        const int nx = buf[i + 1];
        if (nx == 0) { i += 2; continue; }
        if (nx == 0xFF) { i++; continue; }
        if (nx >= 0xD0 && nx <= 0xD7) {
            if (R == 0 || nx != 0xD0 + (int)(k & 7)) bad = true;
            close((uint32_t)i);
            i += 2;
            start = (uint32_t)i;
            if (R == 0) break;      // no restart interval was declared: nothing decodes past the marker
            continue;
        }
        break;      // any other marker ends the scan
    }
    if (R != 0 || k == 0) {
        // the last interval (the whole scan without DRI); an interval of no bytes after a trailing RSTn is not one
        if (!(k >= expected && (uint32_t)i == start)) close((uint32_t)i);
    }
    if (k != expected) bad = true;
    if (bad) P.status0 |= kStatusRestart;

    // anything but EOI after the scan: another scan is unsupported
    size_t q = i;
    for (int guard = 0; guard < 64 && q + 1 < len; guard++) {
        if (buf[q] != 0xFF) break;
        const int mk = buf[q + 1];
        if (mk == 0xDA) return msg = "multiple scans", SLAM_E_UNSUPPORTED;
        if (mk == 0xD9 || mk == 0xFF || mk == 0 || (mk >= 0xD0 && mk <= 0xD7)) break;
        if (len - q < 4) break;
        const size_t L2 = be16(buf + q + 2);
        if (L2 < 2 || L2 > len - q - 2) break;
        q += 2 + L2;
    }
    d.valid = 1;
    msg.clear();
    return SLAM_OK;
}

}  // namespace jpeg

namespace {
thread_local std::string g_jpeg_err;
}

extern "C" const char* slam_jpeg_last_error(void) { return g_jpeg_err.c_str(); }

extern "C" int slam_jpeg_info(const uint8_t* buf, size_t len, struct slam_jpeg_info* out)
{
    if (!out) return g_jpeg_err = "null output", SLAM_E_INVALID_ARG;
    std::memset(out, 0, sizeof(*out));
    jpeg::Parsed P;
    const int rc = jpeg::parse(buf, len, 3, P, g_jpeg_err);
    if (rc != SLAM_OK) return rc;
    out->width = P.d.width;
    out->height = P.d.height;
    out->channels = P.d.ncomp == 1 ? 1 : 3;
    out->sampling = P.d.sampling;
    out->restart_interval = P.restart;
    out->segments = (int32_t)P.segs.size();
    out->orientation = P.orientation;
    return SLAM_OK;
}

extern "C" int slam_jpeg_decode_host(const uint8_t* buf, size_t len, uint8_t* out, size_t step, int channels,
                                     int* status)
{
    using namespace jpeg;
    if (status) *status = 0;
    if (!out) return g_jpeg_err = "null output", SLAM_E_INVALID_ARG;
    Parsed P;
    const int rc = parse(buf, len, channels, P, g_jpeg_err);
    if (rc != SLAM_OK) return rc;
    const ImageDesc& d = P.d;
    if (step < (size_t)d.width * (size_t)channels) return g_jpeg_err = "step smaller than a row", SLAM_E_INVALID_ARG;
    std::vector<int16_t> coef((size_t)d.total_blocks * 64, 0);
    std::vector<uint8_t> planes(P.plane_bytes);
    int st = P.status0;
    uint8_t zz[64];
    for (int i = 0; i < 64; i++) zz[i] = (uint8_t)zigzag_natural(i);
    for (const Segment& sg : P.segs) st |= decode_segment(d, d.tables, zz, buf, sg, coef.data());
    for (int c = 0; c < d.ncomp; c++) {
        const ScanComp& sc = d.comp[c];
        const int pitch = sc.bw * 8;
        for (int b = 0; b < sc.bw * sc.bh; b++) {
            const int16_t* blk = coef.data() + ((size_t)sc.coef_block + b) * 64;
            uint32_t ws[64], col[8];
            for (int x = 0; x < 8; x++) {
                idct_column(blk, d.quant[c], x, col);
                for (int r = 0; r < 8; r++) ws[r * 8 + x] = col[r];
            }
            uint8_t* dst = planes.data() + d.plane_comp[c] + (size_t)(b / sc.bw) * 8 * pitch + (size_t)(b % sc.bw) * 8;
            for (int r = 0; r < 8; r++) idct_row(ws + r * 8, dst + (size_t)r * pitch);
        }
    }
    for (int y = 0; y < d.height; y++)
        for (int x = 0; x < d.width; x++) emit_pixel(d, planes.data(), x, y, out + (size_t)y * step + (size_t)x * channels);
    if (status) *status = st;
    return SLAM_OK;
}

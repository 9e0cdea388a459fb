// Baseline JPEG: marker parsing, validation and the segment table (host), and
// slam_jpeg_info / slam_jpeg_decode_host, the whole decoder on the host through
// the headers the kernels use (jpeg_huff.h, jpeg_pix.h); the Motion-JPEG stream
// rules (SLAM_JPEG_MJPEG) and the host driver of the chunk-parallel entropy decoder
// (slam_jpeg_decode_host_sync).  Plain C++: no HIP.
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

int parse(const uint8_t* buf, size_t len, int channels, Parsed& P, std::string& msg, int flags)
{
    const bool mjpeg = (flags & SLAM_JPEG_MJPEG) != 0;
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
            // the AVI1 tag of Motion-JPEG frames: byte 4 is 0 for a progressive frame, 1 or 2 for the fields of a pair
            if (mjpeg && n >= 5 && std::memcmp(s, "AVI1", 4) == 0 && s[4] != 0)
                return msg = "interlaced Motion-JPEG (an AVI1 frame that is one field of a pair)", SLAM_E_UNSUPPORTED;
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
            if (mjpeg) {      // frames of an AVI usually carry no DHT: the Annex K tables stand in for slots 0 and 1
                for (int t = 0; t < 4; t++) {
                    HuffTable& ht = d.tables[(t >> 1) * 4 + (t & 1)];
                    if (ht.defined) continue;
                    const uint8_t *counts, *vals;
                    int nv;
                    std_huff_table(t >> 1, t & 1, &counts, &vals, &nv);
                    huff_build(ht, counts, vals, nv);
                }
            }
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

// ITU-T T.81 Annex K.3: the typical Huffman tables (tables K.3 .. K.6)
void std_huff_table(int klass, int slot, const uint8_t** counts, const uint8_t** vals, int* nvals)
{
    static const uint8_t dc_counts[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                             {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
    static const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    static const uint8_t ac_counts[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                             {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
    static const uint8_t ac_vals[2][162] = {
        {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
         0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
         0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
         0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
         0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
         0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
         0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
         0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
         0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
        {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
         0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
         0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
         0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
         0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
         0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
         0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
         0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
         0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
    const int s = slot & 1;
    if (klass == 0) {
        *counts = dc_counts[s];
        *vals = dc_vals;
        *nvals = 12;
    } else {
        *counts = ac_counts[s];
        *vals = ac_vals[s];
        *nvals = 162;
    }
}

uint32_t sync_chunk_bytes(int value)
{
    if (value == 0) return kSyncChunkDefault;
    if (value < kSyncChunkMin || value > kSyncChunkMax || (value & (value - 1))) return 0;
    return (uint32_t)value;
}

// The host driver of the chunk-parallel path: jpeg.hip's kernels restated as loops.  A workgroup
// is kSyncLanes consecutive chunks of one segment; a round recomputes the lanes whose entry state
// changed, from the exit states of the round before (two-phase, as the barriers make it); a launch
// runs every workgroup once, its first lane entering with what the workgroup before it left in
// the launch before.
int sync_decode_host(const ImageDesc& d, const uint8_t* bytes, const std::vector<SyncSeg>& segs, uint32_t C, int16_t* coef,
                     SyncTotals& T)
{
    constexpr uint32_t W = kSyncLanes;
    uint8_t zz[64];
    for (int i = 0; i < 64; i++) zz[i] = (uint8_t)zigzag_natural(i);
    const uint32_t max_steps = sync_max_steps(C);
    int status = 0;
    for (const SyncSeg& sg : segs) {
        const uint32_t nwg = (sg.nchunks + W - 1) / W;
        auto limit = [&](uint32_t ci) {
            const uint64_t e = (uint64_t)sg.off + ((uint64_t)ci + 1) * C;
            return e < sg.end ? (uint32_t)e : sg.end;
        };
        std::vector<uint64_t> ex((size_t)nwg * W, kStateUnknown), wg_entry(nwg, 0);
        std::vector<uint64_t> wg_exit[kSyncLaunches];
        for (auto& v : wg_exit) v.assign(nwg, kStateUnknown);
        std::vector<uint32_t> rmax(nwg, 0), rtot(nwg, 0);
        uint32_t seg_launch = 0;
        std::vector<uint64_t> lex(W), cur(W), cold(W), ne(W);
        std::vector<uint8_t> dirty(W);
        for (int r = 0; r < kSyncLaunches; r++) {
            for (uint32_t j = 0; j < nwg; j++) {
                const uint32_t ci0 = j * W;
                uint64_t e0;
                if (ci0 == 0) e0 = state_pack(sg.off, 0, 0, 0);
                else if (r == 0) e0 = sync_cold(bytes, sg, ci0, C);
                else e0 = sync_entry(wg_exit[r - 1][j - 1], sync_cold(bytes, sg, ci0, C));
                if (r > 0 && wg_entry[j] == e0) {
                    wg_exit[r][j] = wg_exit[r - 1][j];
                    continue;
                }
                for (uint32_t l = 0; l < W; l++) {
                    const uint32_t ci = ci0 + l;
                    lex[l] = r == 0 ? kStateUnknown : ex[(size_t)j * W + l];
                    cold[l] = ci < sg.nchunks && ci > 0 ? sync_cold(bytes, sg, ci, C) : 0;
                }
                for (uint32_t l = 0; l < W; l++) cur[l] = l == 0 ? wg_entry[j] : sync_entry(lex[l - 1], cold[l]);
                uint32_t rounds = 0;
                for (uint32_t round = 0; round < W + 1; round++) {
                    bool any = false;
                    for (uint32_t l = 0; l < W; l++) {
                        ne[l] = l == 0 ? e0 : sync_entry(lex[l - 1], cold[l]);
                        dirty[l] = ci0 + l < sg.nchunks && ((r == 0 && round == 0) || ne[l] != cur[l]);
                        any = any || dirty[l];
                    }
                    if (!any) break;
                    rounds++;
                    for (uint32_t l = 0; l < W; l++)
                        if (dirty[l]) {
                            cur[l] = ne[l];
                            lex[l] = sync_walk(d.tables, bytes, sg, cur[l], limit(ci0 + l), max_steps, nullptr);
                        }
                }
                for (uint32_t l = 0; l < W; l++) ex[(size_t)j * W + l] = lex[l];
                wg_entry[j] = e0;
                wg_exit[r][j] = lex[W - 1];
                if (rounds > rmax[j]) rmax[j] = rounds;
                rtot[j] += rounds;
                seg_launch = (uint32_t)r + 1;
            }
        }
        // count (and verify) under the settled states, scan, write
        std::vector<ChunkCount> cc(sg.nchunks);
        uint32_t flags = 0, started = 0;
        for (uint32_t ci = 0; ci < sg.nchunks; ci++) {
            const uint64_t entry = ci == 0 ? state_pack(sg.off, 0, 0, 0) : sync_entry(ex[ci - 1], sync_cold(bytes, sg, ci, C));
            const uint64_t x = sync_walk(d.tables, bytes, sg, entry, limit(ci), max_steps, &cc[ci]);
            if (x != ex[ci]) cc[ci].flags |= kChunkMismatch;
            flags |= cc[ci].flags;
            started += cc[ci].nstart;      // modulo 2^32, as the device's scan
        }
        if (!flags && started == sg.nblocks) {
            uint32_t j0 = 0, p0 = 0, p1 = 0, p2 = 0;
            for (uint32_t ci = 0; ci < sg.nchunks; ci++) {
                if (sync_write(d, d.tables, zz, bytes, sg, cc[ci], j0, p0, p1, p2, coef)) flags |= kChunkFault;
                j0 += cc[ci].nstart;
                p0 += cc[ci].dc0;
                p1 += cc[ci].dc1;
                p2 += cc[ci].dc2;
            }
        }
        const bool accepted = !flags && started == sg.nblocks;
        if (!accepted) {
            for (uint32_t j = 0; j < sg.nblocks; j++) {
                uint32_t blk;
                int c;
                if (seg_block_addr(d, sg.mcu0, sg.bpm, j, blk, c)) std::memset(coef + (size_t)blk * 64, 0, 64 * sizeof(int16_t));
            }
            const Segment s1{sg.image, sg.off, sg.end, sg.mcu0, sg.nblocks / sg.bpm};
            status |= decode_segment(d, d.tables, zz, bytes, s1, coef);
        }
        T.parallel++;
        T.fallback += accepted ? 0 : 1;
        T.chunks += sg.nchunks;
        for (uint32_t j = 0; j < nwg; j++) {
            if ((int32_t)rmax[j] > T.wg_rounds_max) T.wg_rounds_max = (int32_t)rmax[j];
            T.wg_rounds_total += rtot[j];
        }
        if ((int32_t)seg_launch > T.launch_rounds_max) T.launch_rounds_max = (int32_t)seg_launch;
        T.launch_rounds_total += seg_launch;
    }
    return status;
}

}  // namespace jpeg

namespace {
thread_local std::string g_jpeg_err;
}

extern "C" const char* slam_jpeg_last_error(void) { return g_jpeg_err.c_str(); }

namespace {

int info_impl(const uint8_t* buf, size_t len, struct slam_jpeg_info* out, int flags)
{
    if (!out) return g_jpeg_err = "null output", SLAM_E_INVALID_ARG;
    std::memset(out, 0, sizeof(*out));
    if (flags & ~SLAM_JPEG_MJPEG) return g_jpeg_err = "unknown parse flag", SLAM_E_INVALID_ARG;
    jpeg::Parsed P;
    const int rc = jpeg::parse(buf, len, 3, P, g_jpeg_err, flags);
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

// sync: the segments of more than one chunk take the chunk-parallel path (SLAM_OPT_JPEG_SYNC = 2)
int decode_host_impl(const uint8_t* buf, size_t len, uint8_t* out, size_t step, int channels, int* status, int flags, bool sync,
                     uint32_t chunk_bytes, jpeg::SyncTotals* T)
{
    using namespace jpeg;
    if (status) *status = 0;
    if (!out) return g_jpeg_err = "null output", SLAM_E_INVALID_ARG;
    if (flags & ~SLAM_JPEG_MJPEG) return g_jpeg_err = "unknown parse flag", SLAM_E_INVALID_ARG;
    Parsed P;
    const int rc = parse(buf, len, channels, P, g_jpeg_err, flags);
    if (rc != SLAM_OK) return rc;
    const ImageDesc& d = P.d;
    if (step < (size_t)d.width * (size_t)channels) return g_jpeg_err = "step smaller than a row", SLAM_E_INVALID_ARG;
    std::vector<int16_t> coef((size_t)d.total_blocks * 64, 0);
    std::vector<uint8_t> planes(P.plane_bytes);
    int st = P.status0;
    uint8_t zz[64];
    for (int i = 0; i < 64; i++) zz[i] = (uint8_t)zigzag_natural(i);
    std::vector<SyncSeg> par;
    for (const Segment& sg : P.segs) {
        SyncSeg ss;
        if (sync && sg.end - sg.off > chunk_bytes && sg.end > sg.off && sync_seg_init(ss, d, sg, chunk_bytes)) par.push_back(ss);
        else st |= decode_segment(d, d.tables, zz, buf, sg, coef.data());
    }
    if (!par.empty()) st |= sync_decode_host(d, buf, par, chunk_bytes, coef.data(), *T);
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

}  // namespace

extern "C" int slam_jpeg_info(const uint8_t* buf, size_t len, struct slam_jpeg_info* out) { return info_impl(buf, len, out, 0); }

extern "C" int slam_jpeg_info_ex(const uint8_t* buf, size_t len, struct slam_jpeg_info* out, int flags)
{
    return info_impl(buf, len, out, flags);
}

extern "C" int slam_jpeg_decode_host(const uint8_t* buf, size_t len, uint8_t* out, size_t step, int channels,
                                     int* status)
{
    return decode_host_impl(buf, len, out, step, channels, status, 0, false, 0, nullptr);
}

extern "C" int slam_jpeg_decode_host_ex(const uint8_t* buf, size_t len, uint8_t* out, size_t step, int channels, int flags,
                                        int* status)
{
    return decode_host_impl(buf, len, out, step, channels, status, flags, false, 0, nullptr);
}

extern "C" int slam_jpeg_decode_host_sync(const uint8_t* buf, size_t len, uint8_t* out, size_t step, int channels,
                                          int chunk_bytes, int flags, int* status, struct slam_jpeg_sync_stats* stats)
{
    if (stats) std::memset(stats, 0, sizeof(*stats));
    const uint32_t C = jpeg::sync_chunk_bytes(chunk_bytes);
    if (!C) return g_jpeg_err = "chunk bytes: 0 or a power of two from 16 to 1024", SLAM_E_INVALID_ARG;
    jpeg::SyncTotals T;
    const int rc = decode_host_impl(buf, len, out, step, channels, status, flags, true, C, &T);
    if (rc == SLAM_OK && stats) {
        stats->parallel_segments = T.parallel;
        stats->fallback_segments = T.fallback;
        stats->chunk_bytes = (int32_t)C;
        stats->lanes = jpeg::kSyncLanes;
        stats->chunks = T.chunks;
        stats->wg_rounds_max = T.wg_rounds_max;
        stats->launch_rounds_max = T.launch_rounds_max;
        stats->wg_rounds_total = T.wg_rounds_total;
        stats->launch_rounds_total = T.launch_rounds_total;
    }
    return rc;
}

extern "C" int slam_jpeg_std_table(int klass, int slot, uint8_t* counts16, uint8_t* vals256, int* nvals)
{
    if (klass < 0 || klass > 1 || slot < 0 || slot > 1 || !counts16 || !vals256 || !nvals)
        return g_jpeg_err = "class and slot are 0 or 1", SLAM_E_INVALID_ARG;
    const uint8_t *c, *v;
    jpeg::std_huff_table(klass, slot, &c, &v, nvals);
    std::memcpy(counts16, c, 16);
    std::memcpy(vals256, v, (size_t)*nvals);
    return SLAM_OK;
}

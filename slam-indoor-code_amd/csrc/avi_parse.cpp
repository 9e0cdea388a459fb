// Motion-JPEG AVI: the chunk walk behind slam_avi_index (include/slamhip.h states the
// contract).  No size field is trusted: every chunk must end inside its parent and the
// buffer, odd sizes are padded to even, and LIST nesting is bounded.  Plain C++: no HIP.
#include "avi_parse.h"

#include <cstring>

namespace avi {

namespace {

inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
constexpr uint32_t cc(char a, char b, char c, char d)
{
    return (uint32_t)(uint8_t)a | ((uint32_t)(uint8_t)b << 8) | ((uint32_t)(uint8_t)c << 16) | ((uint32_t)(uint8_t)d << 24);
}
inline uint32_t upper(uint32_t f)
{
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) {
        uint32_t ch = (f >> (8 * i)) & 255u;
        if (ch >= 'a' && ch <= 'z') ch -= 32;
        r |= ch << (8 * i);
    }
    return r;
}

struct Walk {
    const uint8_t* b;
    size_t n;
    slam_avi_info* info;
    std::vector<Frame>* frames;
    std::string* msg;
    bool have_hdrl = false, have_video = false;
    int streams = 0;
};

// One chunk header at p inside [p, end): its id, size and the range of its data.  false: it runs past its parent.
bool chunk_at(const Walk& w, size_t p, size_t end, uint32_t& id, size_t& data, size_t& size)
{
    if (end - p < 8) return false;
    id = le32(w.b + p);
    size = le32(w.b + p + 4);
    data = p + 8;
    return size <= end - data;
}

int fail(Walk& w, int code, const char* what)
{
    *w.msg = what;
    return code;
}

int walk_strl(Walk& w, size_t p, size_t end)
{
    const int number = w.streams++;
    bool vids = false;
    while (end - p >= 8) {
        uint32_t id;
        size_t data, size;
        if (!chunk_at(w, p, end, id, data, size)) return fail(w, SLAM_E_INVALID_ARG, "a chunk of strl runs past its list");
        if (id == cc('s', 't', 'r', 'h')) {
            if (size < 36) return fail(w, SLAM_E_INVALID_ARG, "short strh");
            vids = le32(w.b + data) == cc('v', 'i', 'd', 's') && !w.have_video;
            if (vids) {
                w.have_video = true;
                w.info->stream = number;
                w.info->handler = le32(w.b + data + 4);
                w.info->scale = le32(w.b + data + 20);
                w.info->rate = le32(w.b + data + 24);
            }
        } else if (id == cc('s', 't', 'r', 'f') && vids) {
            if (size < 20) return fail(w, SLAM_E_INVALID_ARG, "short strf");
            const int32_t bw = (int32_t)le32(w.b + data + 4), bh = (int32_t)le32(w.b + data + 8);
            w.info->width = bw;
            w.info->height = bh < 0 ? (bh == INT32_MIN ? 0 : -bh) : bh;
            w.info->compression = le32(w.b + data + 16);
        }
        p = data + size + (size & 1);
        if (p > end) break;
    }
    return SLAM_OK;
}

int walk_hdrl(Walk& w, size_t p, size_t end)
{
    w.have_hdrl = true;
    while (end - p >= 8) {
        uint32_t id;
        size_t data, size;
        if (!chunk_at(w, p, end, id, data, size)) return fail(w, SLAM_E_INVALID_ARG, "a chunk of hdrl runs past its list");
        if (id == cc('a', 'v', 'i', 'h')) {
            if (size < 40) return fail(w, SLAM_E_INVALID_ARG, "short avih");
            if (!w.info->width) w.info->width = (int32_t)le32(w.b + data + 32);
            if (!w.info->height) w.info->height = (int32_t)le32(w.b + data + 36);
        } else if (id == cc('L', 'I', 'S', 'T')) {
            if (size < 4) return fail(w, SLAM_E_INVALID_ARG, "a LIST of fewer than 4 bytes");
            if (le32(w.b + data) == cc('s', 't', 'r', 'l'))
                if (int rc = walk_strl(w, data + 4, data + size)) return rc;
        }
        p = data + size + (size & 1);
        if (p > end) break;
    }
    return SLAM_OK;
}

int walk_movi(Walk& w, size_t p, size_t end, int depth)
{
    if (depth > kMaxDepth) return fail(w, SLAM_E_INVALID_ARG, "LIST nesting deeper than 8");
    if (!w.have_hdrl) return fail(w, SLAM_E_INVALID_ARG, "movi before hdrl: hdrl missing");
    const int s = w.info->stream;
    const uint8_t d0 = (uint8_t)('0' + (s / 10) % 10), d1 = (uint8_t)('0' + s % 10);
    while (end - p >= 8) {
        uint32_t id;
        size_t data, size;
        if (!chunk_at(w, p, end, id, data, size)) return fail(w, SLAM_E_INVALID_ARG, "a chunk of movi runs past its list");
        if (id == cc('L', 'I', 'S', 'T')) {
            if (size < 4) return fail(w, SLAM_E_INVALID_ARG, "a LIST of fewer than 4 bytes");
            if (le32(w.b + data) == cc('r', 'e', 'c', ' '))
                if (int rc = walk_movi(w, data + 4, data + size, depth + 1)) return rc;
        } else if (w.have_video && s < 100 && w.b[p] == d0 && w.b[p + 1] == d1 && w.b[p + 2] == 'd' &&
                   (w.b[p + 3] == 'c' || w.b[p + 3] == 'b')) {
            if (size) w.frames->push_back(Frame{(uint64_t)data, (uint64_t)size});
            else w.frames->push_back(w.frames->empty() ? Frame{0, 0} : w.frames->back());      // a dropped frame
        }
        p = data + size + (size & 1);
        if (p > end) break;
    }
    return SLAM_OK;
}

}  // namespace

int index(const uint8_t* buf, size_t len, slam_avi_info& info, std::vector<Frame>& frames, std::string& msg)
{
    std::memset(&info, 0, sizeof(info));
    info.stream = -1;
    frames.clear();
    msg.clear();
    if (!buf || len < 12 || le32(buf) != cc('R', 'I', 'F', 'F') || le32(buf + 8) != cc('A', 'V', 'I', ' '))
        return msg = "not a RIFF AVI file", SLAM_E_INVALID_ARG;
    Walk w{buf, len, &info, &frames, &msg};
    size_t top = 0;
    bool codec_checked = false;
    while (len - top >= 12) {
        uint32_t id;
        size_t data, size;
        if (!chunk_at(w, top, len, id, data, size)) return msg = "a top-level chunk runs past the buffer", SLAM_E_INVALID_ARG;
        const bool riff = id == cc('R', 'I', 'F', 'F') && size >= 4 &&
                          (le32(buf + data) == cc('A', 'V', 'I', ' ') || le32(buf + data) == cc('A', 'V', 'I', 'X'));
        if (riff) {
            const size_t end = data + size;
            size_t p = data + 4;
            while (end - p >= 8) {
                uint32_t cid;
                size_t cdata, csize;
                if (!chunk_at(w, p, end, cid, cdata, csize)) return msg = "a chunk runs past its RIFF", SLAM_E_INVALID_ARG;
                if (cid == cc('L', 'I', 'S', 'T')) {
                    if (csize < 4) return msg = "a LIST of fewer than 4 bytes", SLAM_E_INVALID_ARG;
                    const uint32_t type = le32(buf + cdata);
                    if (type == cc('h', 'd', 'r', 'l')) {
                        if (int rc = walk_hdrl(w, cdata + 4, cdata + csize)) return rc;
                    } else if (type == cc('m', 'o', 'v', 'i')) {
                        if (w.have_hdrl && !codec_checked) {
                            codec_checked = true;
                            if (!w.have_video) return msg = "no video stream", SLAM_E_UNSUPPORTED;
                            const uint32_t codec = upper(info.handler ? info.handler : info.compression);
                            if (codec != cc('M', 'J', 'P', 'G') && codec != cc('J', 'P', 'E', 'G'))
                                return msg = "the video stream's codec is not Motion-JPEG (MJPG, mjpg or jpeg)", SLAM_E_UNSUPPORTED;
                        }
                        if (int rc = walk_movi(w, cdata + 4, cdata + csize, 0)) return rc;
                    }
                }
                p = cdata + csize + (csize & 1);
                if (p > end) break;
            }
        }
        top = data + size + (size & 1);
        if (top > len) break;
    }
    if (!w.have_hdrl) return msg = "hdrl missing", SLAM_E_INVALID_ARG;
    if (!w.have_video) return msg = "no video stream", SLAM_E_UNSUPPORTED;
    if (!codec_checked) {
        const uint32_t codec = upper(info.handler ? info.handler : info.compression);
        if (codec != cc('M', 'J', 'P', 'G') && codec != cc('J', 'P', 'E', 'G'))
            return msg = "the video stream's codec is not Motion-JPEG (MJPG, mjpg or jpeg)", SLAM_E_UNSUPPORTED;
    }
    info.frames = (int64_t)frames.size();
    return SLAM_OK;
}

}  // namespace avi

namespace {
thread_local std::string g_avi_err;
}

extern "C" const char* slam_avi_last_error(void) { return g_avi_err.c_str(); }

extern "C" int slam_avi_index(const uint8_t* buf, size_t len, struct slam_avi_info* info, uint64_t* offsets, uint64_t* sizes,
                              size_t cap)
{
    if (!info) return g_avi_err = "null info", SLAM_E_INVALID_ARG;
    std::vector<avi::Frame> frames;
    const int rc = avi::index(buf, len, *info, frames, g_avi_err);
    if (rc != SLAM_OK) return rc;
    for (size_t i = 0; i < frames.size() && i < cap; i++) {
        if (offsets) offsets[i] = frames[i].off;
        if (sizes) sizes[i] = frames[i].size;
    }
    return SLAM_OK;
}

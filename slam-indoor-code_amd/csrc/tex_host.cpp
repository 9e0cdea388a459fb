// Per-face texture atlas on the host: slam_tex_layout (host only), slam_tex_select_host and
// slam_tex_fill_host, the twins of tex.hip's kernels.  They need no context and no
// device; the arithmetic is tex_math.h's, so the results equal the device's bit for bit.
// Views (selection) and texel rows (fill) are dealt to up to 16 threads.
#include "../../include/slamhip.h"
#include "tex_math.h"

#include <algorithm>
#include <functional>
#include <thread>
#include <vector>

namespace slamhip {

int tex_check_select(const void* ids, int nv, int h, int w, int view0, int nf, const void* best_count, const void* best_view)
{
    if (nf < 0 || nv < 0 || h < 1 || w < 1 || view0 < 0 || (long long)h * w > (1ll << 30) ||
        (long long)view0 + nv > 0x7fffffffll)
        return SLAM_E_INVALID_ARG;
    if (nf > kTexMaxFaces) return SLAM_E_UNSUPPORTED;
    if ((nv > 0 && !ids) || (nf > 0 && (!best_count || !best_view))) return SLAM_E_INVALID_ARG;
    return SLAM_OK;
}

// everything of a fill call that is host memory or a scalar
int tex_check_fill(const void* V, const void* C, const void* F, int nv, int nf, const void* frames, int n, int h, int w,
                   int channels, const int32_t* frame_idx, const double* P, int nviews, const void* best_count,
                   const void* best_view, int min_pixels, int T, int page, const void* atlas)
{
    if (!tex_layout_args_ok(T, page) || min_pixels < 1 || min_pixels > kTexMaxMinPixels || nv < 0 || nf < 0 || n < 0 ||
        nviews < 0 || nviews > kTexMaxViews || h < 1 || w < 1 || (channels != 1 && channels != 3) ||
        (long long)h * w > (1ll << 30))
        return SLAM_E_INVALID_ARG;
    if (nf > kTexMaxFaces) return SLAM_E_UNSUPPORTED;
    if (nf > 0 && (!F || !best_count || !best_view || !atlas || nv < 1 || !V || !C)) return SLAM_E_INVALID_ARG;
    if (nviews > 0 && (!P || !frames)) return SLAM_E_INVALID_ARG;
    for (int m = 0; m < nviews; m++) {
        const int f = frame_idx ? frame_idx[m] : m;
        if (f < 0 || f >= n) return SLAM_E_INVALID_ARG;
    }
    return SLAM_OK;
}

void tex_make_views(const double* P, const int32_t* frame_idx, int nviews, TexView* out)
{
    for (int m = 0; m < nviews; m++) {
        for (int k = 0; k < 12; k++) out[m].P[k] = P[(size_t)m * 12 + k];
        out[m].frame = frame_idx ? frame_idx[m] : m;
        out[m].pad = 0;
    }
}

namespace {

void parallel_ranges(long long n, const std::function<void(long long, long long)>& fn)
{
    const int nthreads = (int)std::max(1ll, std::min({16ll, (long long)std::thread::hardware_concurrency(), n}));
    auto part = [&](int t) {
        const long long a = n * t / nthreads, b = n * (t + 1) / nthreads;
        if (b > a) fn(a, b);
    };
    if (nthreads == 1) {
        part(0);
        return;
    }
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; t++) pool.emplace_back(part, t);
    part(0);
    for (auto& th : pool) th.join();
}

}  // namespace
}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_tex_layout(int nf, int T, int page, int* npages, int* page_w, int32_t* page_h, int cap_pages, double* uv,
                               int32_t* face_page)
{
    if (!npages || !page_w) return SLAM_E_INVALID_ARG;
    *npages = *page_w = 0;
    if (!tex_layout_args_ok(T, page) || nf < 0 || cap_pages < 0) return SLAM_E_INVALID_ARG;
    if (nf > kTexMaxFaces) return SLAM_E_UNSUPPORTED;
    const TexLayout l = tex_layout(nf, T, page);
    *npages = l.npages;
    *page_w = l.page_w;
    if (page_h) {
        if (l.npages > cap_pages) return SLAM_E_CAPACITY;
        for (int p = 0; p < l.npages; p++) page_h[p] = tex_page_height(l, p);
    }
    if (!uv && !face_page) return SLAM_OK;
    const long long cpp = (long long)l.cells_x * l.cells_x;
    parallel_ranges(nf, [&](long long f0, long long f1) {
        for (long long f = f0; f < f1; f++) {
            const long long cell = f >> 1;
            const int half = (int)(f & 1), p = (int)(cell / cpp);
            const long long in_page = cell - (long long)p * cpp;
            const int cy = (int)(in_page / l.cells_x), cx = (int)(in_page - (long long)cy * l.cells_x);
            if (face_page) face_page[f] = p;
            if (!uv) continue;
            const double pw = (double)l.page_w, ph = (double)tex_page_height(l, p);
            for (int k = 0; k < 3; k++) {
                int x, y;
                tex_corner(T, half, k, x, y);
                uv[6 * f + 2 * k] = (double)(cx * l.S + x) / pw;
                uv[6 * f + 2 * k + 1] = 1.0 - (double)(cy * l.S + y) / ph;
            }
        }
    });
    return SLAM_OK;
}

extern "C" int slam_tex_select_host(const int32_t* ids, int nv, int h, int w, int view0, int nf, int32_t* best_count,
                                    int32_t* best_view)
{
    if (int rc = tex_check_select(ids, nv, h, w, view0, nf, best_count, best_view)) return rc;
    if (nv == 0 || nf == 0) return SLAM_OK;
    const size_t npx = (size_t)h * w;
    const int group = std::max(1, std::min({16, (int)std::thread::hardware_concurrency(), nv}));
    std::vector<std::vector<int32_t>> cnt((size_t)group);
    for (int m0 = 0; m0 < nv; m0 += group) {
        const int m1 = std::min(nv, m0 + group);
        parallel_ranges(m1 - m0, [&](long long a, long long b) {
            for (long long k = a; k < b; k++) {
                std::vector<int32_t>& c = cnt[(size_t)k];
                c.assign((size_t)nf, 0);
                const int32_t* img = ids + (size_t)(m0 + k) * npx;
                for (size_t p = 0; p < npx; p++) {
                    const int32_t f = tex_id_face(img[p], nf);
                    if (f >= 0) c[(size_t)f]++;
                }
            }
        });
        parallel_ranges(nf, [&](long long f0, long long f1) {
            for (long long f = f0; f < f1; f++)
                for (int m = m0; m < m1; m++) tex_best_step(best_count[f], best_view[f], cnt[(size_t)(m - m0)][(size_t)f], view0 + m);
        });
    }
    return SLAM_OK;
}

extern "C" int slam_tex_fill_host(const double* V, const uint8_t* C, const int32_t* F, int nv, int nf, const uint8_t* frames,
                                  int n, int h, int w, int channels, const int32_t* frame_idx, const double* P, int nviews,
                                  const int32_t* best_count, const int32_t* best_view, int min_pixels, int T, int page,
                                  uint8_t* atlas)
{
    if (int rc = tex_check_fill(V, C, F, nv, nf, frames, n, h, w, channels, frame_idx, P, nviews, best_count, best_view,
                                min_pixels, T, page, atlas))
        return rc;
    if (nf == 0) return SLAM_OK;
    for (size_t k = 0; k < 3 * (size_t)nf; k++)
        if (F[k] < 0 || F[k] >= nv) return SLAM_E_INVALID_ARG;
    for (int f = 0; f < nf; f++)
        if (best_view[f] < -1 || best_view[f] >= nviews) return SLAM_E_INVALID_ARG;
    std::vector<TexView> views((size_t)nviews);
    tex_make_views(P, frame_idx, nviews, views.data());
    const TexLayout l = tex_layout(nf, T, page);
    const long long rows = l.cell_rows * l.S;
    parallel_ranges(rows, [&](long long y0, long long y1) {
        for (long long y = y0; y < y1; y++)
            for (int x = 0; x < l.page_w; x++)
                tex_texel(l, nf, x, y, V, C, F, frames, w, h, channels, views.data(), best_count, best_view, min_pixels,
                          atlas + ((size_t)y * l.page_w + x) * 3);
    });
    return SLAM_OK;
}

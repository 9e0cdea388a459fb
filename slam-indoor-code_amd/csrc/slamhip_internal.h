// Internal declarations of libslamhip: context, device workspace, kernel launch
// entry points.  Everything here is MI355X (gfx950) HIP; nothing is a fallback.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <utility>
#include <string>
#include <vector>

#include "../../include/slamhip.h"
#include "dev_layout.h"

namespace slamhip {

// Correctly rounded f32 sqrt / divide on gfx950.  The __fsqrt_rn / __fdiv_rn
// builtins lower to the 1-ulp hardware instructions; computing in f64 (IEEE
// correctly rounded) and rounding once to f32 is exact for these ops, because
// 53 >= 2 * 24 + 2 makes the double rounding innocuous.
__device__ __forceinline__ float cr_sqrtf(float x) { return (float)sqrt((double)x); }
__device__ __forceinline__ float cr_divf(float a, float b) { return (float)((double)a / (double)b); }

// ---- numeric constants shared by kernels and host (restated from OpenCV) ----
constexpr int kSiftD = 4, kSiftN = 8;
constexpr int kSiftHist = (kSiftD + 2) * (kSiftD + 2) * (kSiftN + 2);  // 360
constexpr int kSiftDescBytes = 128;
constexpr int kOrbDescBytes = 32;
constexpr int kOrbExpBytes = 128;      // +-1 FP4 (e2m1) expansion of the 256 bits for the MFMA Hamming path
constexpr int kOrbEdge = 31;           // ORB edgeThreshold, runByImageBorder

// FAST tiles: 64 columns (one wave, one ballot per row) x 16 rows
constexpr int kFastTileW = 64, kFastTileH = 16;
// undist_remap (undistort.hip): a workgroup owns one destination tile of
// kUndistTileW x kUndistTileH pixels and loops over up to kUndistFrames frames
constexpr int kUndistTileW = 128, kUndistTileH = 8, kUndistFrames = 8;
// chess_response / chess_nms (calib.hip): level tiles of 64 columns (one wave, one
// ballot per row) x 16 rows; calib_subpix: the largest half window per axis
constexpr int kChessTileW = 64, kChessTileH = 16;
constexpr int kSubpixMaxWin = 15;
// klt_track (klt.hip): window 3 .. 31 per axis, at most 9 pyramid levels (maxLevel 0 .. 8)
constexpr int kKltMinWin = 3, kKltMaxWin = 31, kKltMaxLevels = 9;

struct SiftConsts {
    float gauss[16];   // 13-tap kernel of GaussianBlur(sigma = sig_diff)
    int ksize;
    float exptab[64];  // hal::exp32f table
};

// SIFT gradient map {magnitude, orientation} (sift_blur_grad): every frame is
// stored with a zero border of kGradPad pixels on each side, so a descriptor
// window of radius <= kGradPad around any in-image keypoint reads zeros (a +0
// contribution, exactly what the reference's 0 < r < rows - 1 test gives)
// instead of testing bounds per sample.  Pixel (f, y, x) lives at element
// f * grad_frame(w, h) + grad_origin(w) + y * grad_pitch(w) + x; the pitch is
// a multiple of 8 elements (64-byte rows) and grad_origin is even, so pixel
// parity is preserved (sift_tab's 16-byte pair loads).
constexpr int kGradPad = 48;
__host__ __device__ __forceinline__ int grad_pitch(int w) { return (w + 2 * kGradPad + 7) & ~7; }
// Slot columns per orientation position of sift_desc_band (64 floats each); the
// position byte plane of sift_blur_grad (obin 2) stores position * kBandSlotCols,
// which shifted by 8 is the position's byte offset in the slots.
constexpr int kBandSlotCols = 5;

// XCD-contiguous tile order for a 3-D grid of image tiles (x, y, frame):
// workgroups are dealt round-robin over the 8 XCDs by linear id, so raster-
// adjacent tiles land on different XCDs (separate L2s) and each fetches the
// halo rows it shares with its neighbours.  Here XCD k takes the k-th eighth of
// the tiles in raster order: neighbours (and the tiles in flight at once) share
// an L2.  The same tiles, each exactly once; on = false: the plain mapping.
// Measured (profiles/r5_xcd_ab.txt): FETCH_SIZE per launch 2.60 -> 1.19 GB
// (fast_detect) and 1.68 -> 0.40 GB (sift_blur_grad), but neither kernel is
// HBM-bound and both ran 2-3 % slower, so it is opt-in: SLAMHIP_XCD_TILES=1.
inline bool xcd_tiles_on()
{
    static const bool on = [] { const char* e = getenv("SLAMHIP_XCD_TILES"); return e && e[0] == '1'; }();
    return on;
}
// Timing probes that deliberately break results (SLAMHIP_FAST_DBG,
// SLAMHIP_SD_DBG) are read only in builds with -DSLAMHIP_DIAG; a normal build
// returns 0 and says once on stderr that it ignored the variable.
inline int diag_env_int(const char* name)
{
    const char* e = getenv(name);
    if (!e || !e[0]) return 0;
#ifdef SLAMHIP_DIAG
    return atoi(e);
#else
    fprintf(stderr, "slamhip: %s ignored (result-breaking timing probe; build with -DSLAMHIP_DIAG)\n", name);
    return 0;
#endif
}
#ifdef __HIPCC__
__device__ __forceinline__ void xcd_tile(bool on, int& x, int& y, int& z)
{
    x = blockIdx.x; y = blockIdx.y; z = blockIdx.z;
    if (!on) return;
    const unsigned gx = gridDim.x, gy = gridDim.y, n = gx * gy * gridDim.z;
    const unsigned lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const unsigned per = n >> 3;
    if (lin >= (per << 3)) return;          // the last n % 8 tiles keep their place
    const unsigned v = (lin & 7) * per + (lin >> 3);
    x = (int)(v % gx);
    y = (int)((v / gx) % gy);
    z = (int)(v / (gx * gy));
}
#endif
__host__ __device__ __forceinline__ size_t grad_frame(int w, int h)
{
    return (size_t)grad_pitch(w) * (size_t)(h + 2 * kGradPad);
}
__host__ __device__ __forceinline__ size_t grad_origin(int w) { return (size_t)kGradPad * grad_pitch(w) + kGradPad; }

// chunked per-target SIFT sample table (sift_tab.hip)
struct SiftTabMeta {
    int len;           // table rows (entries per target, padded; a multiple of the pipeline depth)
    int radius;
    float ori_deg;
};

// band-staged SIFT tables for one (angle, size) (sift_band.hip)
struct SiftBandMeta {
    int nrec = 0, nchunks = 0;
    int pitch = 0;      // grad_pitch the table's window offsets were built for
    bool neg = false;   // floor(obin) always in [-9, -1]
    int band_first[6] = {0, 0, 0, 0, 0, 0};
    int radius = 0;
    float ori_deg = 0.f;
};

// sift_desc_cols tables (sift_cols.hip): two column passes, each band-major
struct SiftColsMeta {
    int nrec = 0, nchunks = 0;
    int band_first[2][6] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
};

// sift_desc_colw tables (sift_colw.hip): one sample list per descriptor column, band-major
struct SiftColwMeta {
    int nrec = 0, nchunks = 0;
    int band_first[4][6] = {};
};

struct OrbConsts {
    float gauss[8];    // 7-tap kernel of GaussianBlur(7x7, sigma = 2)
};

// grow-only device buffer
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t n);
    void release();
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// A finished DevLayout bound to a DevBuf.  bind() sizes the buffer once and may
// move it, so slots become pointers only through a bound DevMem; the copies take
// their byte count from the slot (count: a leading part of it).
struct DevMem {
    uint8_t* base = nullptr;
    hipError_t bind(DevBuf& buf, const DevLayout& layout)
    {
        const hipError_t e = buf.ensure(layout.bytes());
        base = e == hipSuccess ? buf.as<uint8_t>() : nullptr;
        return e;
    }
    template <class T> T* ptr(Slot<T> s) const { return reinterpret_cast<T*>(base + s.off); }
    template <class T> hipError_t upload(Slot<T> s, const T* host, hipStream_t st) const { return upload(s, host, s.count, st); }
    template <class T> hipError_t upload(Slot<T> s, const T* host, size_t count, hipStream_t st) const
    {
        return count > s.count ? hipErrorInvalidValue : hipMemcpyAsync(ptr(s), host, count * sizeof(T), hipMemcpyHostToDevice, st);
    }
    template <class T> hipError_t download(T* host, Slot<T> s, hipStream_t st) const { return download(host, s, s.count, st); }
    template <class T> hipError_t download(T* host, Slot<T> s, size_t count, hipStream_t st) const
    {
        return count > s.count ? hipErrorInvalidValue : hipMemcpyAsync(host, ptr(s), count * sizeof(T), hipMemcpyDeviceToHost, st);
    }
};

// the gradient map's zero border as last written by sift_blur_grad: buffer
// (pointer + size: a reallocation changes the size), geometry, frames covered
struct SiftGradBorder {
    void* p = nullptr;
    size_t bytes = 0;
    int w = 0, h = 0, frames = 0;
    int obin = 0;          // the stored orientation form of the border (launch_sift_base)
    float ori_deg = 0.f;
    void* pp = nullptr;    // obin 2: the slot-position byte plane (gradpos) the border went to
    size_t pbytes = 0;
};

// events bracketing every launch of a kernel family (bench.py roofline timing)
constexpr int kProfFamilies = 12;   // slam_profile_read's families (include/slamhip.h)
struct ProfFamily {
    std::vector<hipEvent_t> ev;   // pairs
    int used = 0;
};

struct BatchState {
    int nframes = 0, w = 0, h = 0, matcher = -1, ntx = 0, nbands = 0;
    int total_kps = 0;
    std::vector<int32_t> kp_counts_raw;   // FAST counts (batch filter input)
    std::vector<int32_t> kp_counts;       // descriptor-bearing keypoints (ORB: border-filtered)
    std::vector<int32_t> kp_offsets;      // exclusive prefix of kp_counts
    int matched_nq = 0;                   // query count of the last slam_batch_match
    bool have_matches = false;
    bool have_desc = false;               // false after slam_batch_fast (keypoints only)
    int est_max_nt = 0;                   // largest per-frame count of the previous batch (fused path)
    // drop the published batch (frame count first: nothing indexes the vectors after this)
    void unpublish()
    {
        nframes = 0;
        have_matches = false;
        have_desc = false;
        total_kps = 0;
        kp_counts_raw.clear();
        kp_counts.clear();
        kp_offsets.clear();
    }
};

}  // namespace slamhip

namespace slamhip {
// slam_sift_detect_batch: frames per call (the pyramid is ~0.5 GB per 1080p
// frame; candidate / keypoint scratch is 1M entries per frame, int-indexed)
constexpr int kSiftDetectMaxFrames = 256;
// slam_orb_detect_batch: frames per call (levels + blurred level: ~3.2 x the gray
// frames) and pyramid levels (cv::ORB nlevels 1..16)
constexpr int kOrbDetectMaxFrames = 256, kOrbDetectMaxLevels = 16;
}  // namespace slamhip

struct slam_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_sync = nullptr;     // stream_sync's polled event
    std::string err;
    slamhip::SiftConsts sift;
    slamhip::OrbConsts orb;
    int cu_count = 256;

    // batch workspace (device)
    slamhip::DevBuf gray, scores, masks, band_cnt, band_pref, frame_info;
    slamhip::DevBuf ftmp, grad, orbblur;   // grad: float2 {mag, ori} per pixel
    slamhip::DevBuf gradpos;               // obin 2: one slot-position byte per grad pixel
    slamhip::SiftGradBorder grad_border;
    slamhip::DevBuf kps, kp_frame, desc_u8, desc_f32, desc_norm, desc_exp;
    slamhip::DevBuf query_norm, knn_part, match_rec, match_flag, match_cnt, match_out;
    void* h_rb = nullptr;     // pinned host readback buffer (small D2H results: counts, totals)
    size_t h_rb_bytes = 0;
    void* h_up = nullptr;     // pinned host image staging (upload_image); ev_up: its last copy
    size_t h_up_bytes = 0;
    hipEvent_t ev_up = nullptr;
    // slam_batch_result_begin / _end: a winner's keypoints + matches in flight
    void* h_win = nullptr;
    size_t h_win_bytes = 0;
    hipEvent_t ev_win = nullptr;
    hipEvent_t ev_rdev = nullptr;      // slam_batch_result_dev's copies on a caller stream
    slamhip::DevBuf synth_world, synth_cams;   // slam_synth_sequence_dev: world texture, per-frame cameras
    int synth_w = 0, synth_h = 0;
    uint64_t synth_seed = 0;
    int win_pending = 0, win_nk = 0;
    size_t win_kb = 0;
    slamhip::DevBuf frames_in, qbuf, tbuf, misc;
    slamhip::BatchState batch;

    // BA workspace
    slamhip::DevBuf ba_obs, ba_par, ba_jac, ba_red, ba_S, ba_aux;

    // full SIFT detector (siftdet.hip): Gaussian + DoG pyramid, candidates, keypoints
    slamhip::DevBuf sd_pyr, sd_cand, sd_kps, sd_kpc;   // sd_kpc: the refined keypoints, frame-major
    // full ORB detector (orbdet.hip): level planes, resize tables, the selection's second keypoint
    // list, the packed list + its frames, counters, angles + {cos, sin}, slam_orb_detect's device result
    slamhip::DevBuf od_pyr, od_tab, od_kps, od_list, od_frame, od_cnt, od_ang, od_out;
    bool od_tab_valid = false;            // od_tab holds the tables of (w, h, scale factor, levels built)
    int od_tab_w = 0, od_tab_h = 0, od_tab_levels = 0;
    double od_tab_scale = 0;
    // two-view geometry (geom.hip); also the staged inputs of the scene calls (cluster.hip)
    slamhip::DevBuf geom;
    // scene post-processing (cluster.hip): pair counters, then the plane fit's slots
    slamhip::DevBuf cluster;
    unsigned long long cluster_pairs_total = 0;   // n (n - 1) / 2 of the last clustering call
    hipStream_t cluster_stats_stream = nullptr;   // ... and the stream it ran on
    // Delaunay step (delaunay.hip): counters, duplicate marks, the triangle scratch
    slamhip::DevBuf delaunay;
    bool delaunay_ran = false;                    // slam_delaunay_last_stats has a call to report
    hipStream_t delaunay_stats_stream = nullptr;  // the stream of the last call

    // SIFT gather table for one (angle, size) (sift_tab.hip)
    slamhip::DevBuf sift_tab;
    bool sift_tab_valid = false;
    float sift_tab_angle = 0.f, sift_tab_size = 0.f;
    int sift_tab_nrec = 0;
    slamhip::SiftTabMeta sift_meta;
    // band-staged SIFT tables (sift_band.hip)
    slamhip::DevBuf sift_band_buf;
    slamhip::DevBuf sift_split;          // sift_desc_band split tail: the halves' rows
    slamhip::DevBuf sift_split_cnt;      // ... and their arrival counters (zero between launches)
    slamhip::DevBuf sift_deal;           // sift_desc_band: the XCD ranges' job counters (zeroed before each launch)
    bool sift_band_valid = false;
    float sift_band_angle = 0.f, sift_band_size = 0.f;
    slamhip::SiftBandMeta sift_band;
    // one-keypoint-per-lane two-pass tables (sift_cols.hip), built with the band tables
    slamhip::DevBuf sift_cols_buf;
    slamhip::DevBuf sift_cols_park;      // sift_desc_cols: pass 0's finished rows per lane
    bool sift_cols_valid = false;
    slamhip::SiftColsMeta sift_cols;
    // column-per-wave tables (sift_colw.hip), built with the band tables
    slamhip::DevBuf sift_colw_buf;
    bool sift_colw_valid = false;
    slamhip::SiftColwMeta sift_colw;

    // undistortion map of one (K, newK, D, w, h) (undistort.hip): CV_16SC2 + CV_16UC1
    slamhip::DevBuf undist_xy, undist_frac;
    slamhip::DevBuf undist_out;           // slam_undistort: the device result of a host frame
    slamhip::DevBuf undist_pts;           // slam_undistort_points: the host points and their results
    bool undist_valid = false;
    double undist_key[30] = {};           // K, newK (K when absent), the 12 coefficients (fisheye: 4, then zeros)
    int undist_model = 0;                 // kLensBrown or kLensFisheye: part of the key
    int undist_w = 0, undist_h = 0;
    bool undist_used = false;             // undist_ev has been recorded
    hipStream_t undist_stream = nullptr;  // the stream that last built or read the map
    hipEvent_t undist_ev = nullptr;       // ... and the end of that work on it

    // chessboard calibration (calib.hip): response maps, NMS masks, candidates +
    // counts, and cornerSubPix's corners + mask factors
    slamhip::DevBuf calib_resp, calib_mask, calib_out, calib_sub;
    // pyramidal LK tracking (klt.hip): host frames staged for slam_klt_track / _pyramid, the gray
    // pyramids (previous frame first, then the candidates), the previous frame's derivative
    // planes, and the points + results of one call
    slamhip::DevBuf klt_img, klt_pyr, klt_deriv, klt_pts;
    // JPEG decoding (jpeg.hip): the uploaded descriptors + segment table + status words + compressed
    // bytes, the coefficients, the component planes, and slam_jpeg_decode's device result
    slamhip::DevBuf jpeg_in, jpeg_coef, jpeg_planes, jpeg_out;
    void* h_jpeg = nullptr;               // pinned staging of jpeg_in
    size_t h_jpeg_bytes = 0;
    void* jpeg_host = nullptr;            // the parsed headers of the last batch, kept between calls (jpeg.hip)
    hipEvent_t jpeg_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    double jpeg_ms[5] = {0, 0, 0, 0, 0};  // slam_jpeg_last_timing
    uint64_t jpeg_bytes[4] = {0, 0, 0, 0};
    bool jpeg_timed = false;
    int opt_jpeg_lanes = 0;               // SLAM_OPT_JPEG_LANES: 0 = by the segment count
    // chunk-parallel entropy decoding (SLAM_OPT_JPEG_SYNC): segment table, chunk states, counts and statistics
    int opt_jpeg_sync = 0, opt_jpeg_chunk = 0;
    slamhip::DevBuf jpeg_sync;
    hipEvent_t jpeg_sync_ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    slam_jpeg_sync_stats jpeg_sync_stats = {};
    // JPEG encoding (jpeg_enc.hip): parameters + scans, coefficients, the unstuffed streams, the FF counts,
    // and slam_jpeg_encode's device frame, stream, size and status
    slamhip::DevBuf jenc_ws, jenc_coef, jenc_bits, jenc_ff, jenc_io;
    hipEvent_t jenc_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double jenc_ms[7] = {0, 0, 0, 0, 0, 0, 0};      // slam_jpeg_enc_last_timing
    uint64_t jenc_bytes[4] = {0, 0, 0, 0};
    bool jenc_timed = false;
    // scene rendering (render.hip): counters + per-view lists + the key buffer of one chunk of views;
    // slam_render's staged host primitives and its device result
    slamhip::DevBuf render_ws, render_in, render_out;
    bool render_ran = false;              // slam_render_last_stats has a call to report
    hipStream_t render_stream = nullptr;  // the stream of the last call
    unsigned long long render_in_count = 0;   // views x primitives of the last call
    std::vector<hipEvent_t> render_evs;   // five per chunk of views of the largest call so far
    double render_ms[4] = {0, 0, 0, 0};   // clear, points + lines, triangles, resolve
    // plane-sweep stereo (mvs.hip): the census maps of a call's distinct frames, the parameter block,
    // the filter's masks, slam_mvs_fuse_dev's device result, the staged host frames + maps of the host-pointer calls
    slamhip::DevBuf mvs_census, mvs_par, mvs_mask, mvs_out, mvs_in;
    hipEvent_t mvs_ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double mvs_ms[4] = {0, 0, 0, 0};      // slam_mvs_last_timing: census, sweep, filter + count, emit
    // semi-global aggregation (mvs_sgm.hip): the volume, the valid counts and S of one group of references,
    // the scratch budget a group stays under (slam_mvs_sgm_set_budget; 0 = the default)
    slamhip::DevBuf mvs_sgm;
    hipEvent_t sgm_ev[3] = {nullptr, nullptr, nullptr};
    double sgm_ms[3] = {0, 0, 0};         // slam_mvs_sgm_last_timing: volume, paths, winner
    size_t sgm_budget = 0;
    // place recognition (place.hip): the assign partials of the K splits, the centroid norms, training's
    // words + distances + sorted order, its counts + starts + cursors + changed flag, the uploaded
    // offsets + weights, the staged buffers of the host-pointer calls
    slamhip::DevBuf place_part, place_norm, place_word, place_cnt, place_par, place_in;
    // loop closing (loop.hip): the hypotheses + centres + sample table + counts + offsets of a RANSAC call (or
    // the two node lists of a point correction), the staged buffers of the host-pointer calls
    slamhip::DevBuf loop_ws, loop_in;
    slamhip::DevBuf loop_pgo;             // slam_pgo_sim3_dev: nodes, linearisations, blocks, PCG vectors, scalars, lists
    // global bundle adjustment (gba.hip): the solver's working set, the staged cameras + points of slam_gba
    slamhip::DevBuf gba_ws, gba_in;
    // TSDF fusion and marching cubes (tsdf.hip): the per-map parameter block of an integrate call, the
    // extraction scratch (flags, vertex bases, row counts and bases, totals), the staged buffers of the
    // host-pointer calls
    slamhip::DevBuf tsdf_par, tsdf_ws, tsdf_in;
    hipEvent_t tsdf_ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double tsdf_ms[4] = {0, 0, 0, 0};     // slam_tsdf_last_timing: integrate, classify + count, scan, emit
    // texture atlas (tex.hip): the per-face counts of one chunk of views, the per-view parameter block
    // and the check flag of a fill, the staged buffers of the host-pointer calls
    slamhip::DevBuf tex_ws, tex_par, tex_in;
    hipEvent_t tex_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double tex_ms[2] = {0, 0};            // slam_tex_last_timing: count + best, fill

    bool prof_on = false;
    slamhip::ProfFamily prof[slamhip::kProfFamilies];
    // slam_set_option: which SIFT descriptor kernel runs (all bit-identical)
    int opt_sift_kernel = SLAM_SIFT_KERNEL_AUTO;
    int opt_band_split = SLAM_BAND_SPLIT_AUTO;
    int opt_pnp_sums = SLAM_PNP_SUMS_ORDERED;
    int opt_fast_reuse = 0;               // SLAM_OPT_FAST_REUSE: off unless the caller vouches for the frames
    // FAST results left by slam_batch_fast (gray, masks, scores, band counts, the
    // emitted keypoint list and frame table): with SLAM_OPT_FAST_REUSE on when
    // slam_batch_fast ran, a batch extraction of the same frames at the same
    // threshold, border and capacity takes them instead of detecting again.  fast_gen counts every launch that rewrites any of them
    // (launch_gray*, launch_fast_detect, launch_fast_emit); the record is valid
    // while its gen is the current one.
    uint64_t fast_gen = 0;
    struct FastReuse {
        const void* frames = nullptr;
        int nframes = 0, w = 0, h = 0, thr = -1, border = -1, cap = 0;
        uint64_t gen = ~0ull;
    } fast_reuse;
    bool fast_reused = false;   // the last batch extraction took them (slam_batch_fast_reused)
    int last_sift_kernel = 0;             // SLAM_SIFT_KERNEL_* of the last descriptor launch
    // the last launch_knn: key mode, split count, SLAM_KNN_VARIANT_* (slam_last_knn_launch)
    int last_knn_mode = -1, last_knn_tsplit = 0, last_knn_variant = 0;
    // the last SIFT detector call that launched: SLAM_SD_FORM_* and sd_refine's grid (slam_last_sift_detect_forms)
    int last_sd_forms = -1, last_sd_refine_blocks = 0;
    hipEvent_t ev_order = nullptr;        // slam_order_after
    hipEvent_t ev_stage[2] = {nullptr, nullptr};   // the last extraction's descriptor start / end
    bool stage_recorded = false;
    // slam_batch_extract_async / _match_async / slam_batch_finish: one batch in flight
    struct Async {
        int state = 0;                    // 0 none, 1 extraction queued, 2 match queued too
        hipStream_t s = nullptr;
        int nframes = 0, w = 0, h = 0, matcher = 0, cap = 0;
        bool committed = false;           // the host batch state is already published
        int launched = 0, norm = 0, nq = 0;
        double ratio = 0;
        const void* query = nullptr;
    } async;
    void* h_async = nullptr;              // pinned: frame table + total + match counts of the batch in flight
    size_t h_async_bytes = 0;
    // slam_sift_detect_batch's host scratch, kept between calls (no fresh pages per call)
    std::vector<std::vector<slam_keypoint>> sd_per;
    std::vector<std::vector<std::pair<float, int>>> sd_ord;
};

namespace slamhip {

int set_err(slam_ctx* c, int code, const std::string& msg);
#define SLAM_HIP(ctx, call)                                                              \
    do {                                                                                 \
        hipError_t e__ = (call);                                                         \
        if (e__ != hipSuccess)                                                           \
            return ::slamhip::set_err((ctx), SLAM_E_HIP,                                 \
                                      std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

// wait for everything queued on s; poll: spin on an event (short waits on the
// hot paths: batch steps, LM iterations) instead of a blocking wait
int stream_sync(slam_ctx* c, hipStream_t s, bool poll = false);
// pinned host readback space of at least n bytes (grown on demand; one per context)
void* readback(slam_ctx* c, size_t n);
// fn(0 .. n-1) on the process's persistent host thread pool (up to 16 threads,
// the caller included; siftdet.hip); items must be independent
void host_parallel_run(int n, const std::function<void(int)>& fn);
// a host copy of n bytes split over the pool (large staging copies)
void host_copy(void* dst, const void* src, size_t n);
void prof_begin(slam_ctx* c, int fam, hipStream_t s);
void prof_end(slam_ctx* c, int fam, hipStream_t s);

// host-side restatements shared with kernels (bit-identical to the oracle's)
void init_consts(slam_ctx* c);
float sift_sigma_diff();
int gauss_kernel_f32(int n, double sigma, float* k);
float host_exp32f(float x, const float* tab);

// ---- kernel launchers (fast.hip, sift.hip, orb.hip, knn.hip) ----
// gray + FAST + NMS over nframes BGR/gray frames; writes gray, masks, scores,
// per-band counts (raw and border-filtered)
hipError_t launch_fast_detect(slam_ctx* c, hipStream_t s, const uint8_t* img, size_t frame_stride,
                              size_t row_stride, int channels, int nframes, int w, int h,
                              int threshold, int nonmax, int border, int type = SLAM_FAST_TYPE_9_16);
hipError_t launch_gray(slam_ctx* c, hipStream_t s, const uint8_t* img, size_t row_stride, int channels, int w,
                       int h);
// prefix sums of band counts -> frame_info; emits keypoints in raster order
hipError_t launch_fast_emit(slam_ctx* c, hipStream_t s, int nframes, int w, int h, int cap);

// obin: store obin = (ori - ori_deg) * 8 / 360 per pixel (for sift_desc_band with
// keypoints of orientation ori_deg) instead of the orientation
hipError_t launch_sift_base(slam_ctx* c, hipStream_t s, int nframes, int w, int h, int obin = 0, float ori_deg = 0.f);
hipError_t launch_sift_desc(slam_ctx* c, hipStream_t s, int nframes, int w, int h,
                            const float* d_kp_cs, int cap, int write_f32);
bool sift_tab_prepare(slam_ctx* c, hipStream_t s, float kp_angle, float kp_size, int w, int h);
hipError_t launch_sift_desc_tab(slam_ctx* c, hipStream_t s, int w, int h, int cap, int write_f32);
// window samples of one keypoint geometry (sift_band.hip)
struct BandSample { int i, j, r0, c0; float rf, cf, wexp; };
struct BandGeometry {
    int radius = 0, pitch = 0, pos_base = 1;
    float ori = 0.f;
    bool neg = false;                  // floor(obin) always in [-9, -1]
    std::vector<BandSample> smp;       // raster order
};
int sift_band_radius(float kp_size);
bool sift_band_geometry(slam_ctx* c, float kp_angle, float kp_size, int w, int h, BandGeometry& g);
bool sift_band_raster_ok(const BandGeometry& g, const std::vector<int>& sched);
bool sift_band_prepare(slam_ctx* c, hipStream_t s, float kp_angle, float kp_size, int w, int h);
// obin: the gradient map holds obin (launch_sift_base with obin, this table's ori_deg)
hipError_t launch_sift_desc_band(slam_ctx* c, hipStream_t s, int w, int h, int cap, int write_f32, int obin);
int sift_band_obin_mode(const slam_ctx* c);
bool sift_band4_enabled();
bool sift_cols_enabled();
bool sift_colw_enabled();
bool sift_colw_prepare(slam_ctx* c, hipStream_t s, const BandGeometry& geo);
hipError_t launch_sift_desc_colw(slam_ctx* c, hipStream_t s, int w, int h, int cap, int write_f32);
bool sift_cols_prepare(slam_ctx* c, hipStream_t s, const BandGeometry& geo);
hipError_t launch_sift_desc_cols(slam_ctx* c, hipStream_t s, int w, int h, int cap, int write_f32);
hipError_t launch_orb_blur(slam_ctx* c, hipStream_t s, int nframes, int w, int h);
hipError_t launch_orb_desc(slam_ctx* c, hipStream_t s, int nframes, int w, int h, const float* d_kp_ab,
                           int cap);
// the same two kernels on caller-named planes and lists (the ORB detector's pyramid levels):
// nframes planes of w x h at src -> dst; the keypoints' patch centres are (x, y) of kps,
// frame kp_frame[g] of img, *total of them (clipped to cap), desc / desc_exp rows per keypoint
hipError_t launch_orb_blur_planes(slam_ctx* c, hipStream_t s, const uint8_t* src, uint8_t* dst, int nframes, int w,
                                  int h);
hipError_t launch_orb_desc_on(slam_ctx* c, hipStream_t s, const uint8_t* img, int w, int h, const slam_keypoint* kps,
                              const int* kp_frame, const int* total, const float* d_kp_ab, int cap, uint8_t* desc,
                              uint32_t* desc_exp);
hipError_t launch_norms_u8(hipStream_t s, const uint8_t* d, int n, int32_t* norms);
hipError_t launch_orb_expand(hipStream_t s, const uint8_t* d, int n, int8_t* out);

// kNN top-2: queries (nq, shared) vs nframes train sets described by frame_info
// (offset/count per frame); kb = 128 (SIFT u8) or 256 (ORB +-1 i8)
hipError_t launch_knn(slam_ctx* c, hipStream_t s, int kb, const void* q, const int32_t* qnorm, int nq,
                      const void* t, const int32_t* tnorm, const int32_t* t_info, int nframes,
                      int max_nt, int norm_kind, int tsplit, int4* part);
// merge partial top-2, apply the ratio test, count survivors per frame
hipError_t launch_knn_finish(slam_ctx* c, hipStream_t s, const int4* part, int nq, int nframes,
                             int tsplit, const int32_t* qnorm, int norm_kind, double ratio,
                             const int32_t* t_info, int2* top_idx, float2* top_dist,
                             slam_dmatch* rec, uint8_t* flag, int32_t* counts);
hipError_t launch_compact(slam_ctx* c, hipStream_t s, const slam_dmatch* rec, const uint8_t* flag,
                          int nq, int nframes, slam_dmatch* out, int32_t* out_counts, int stride);

// ---- full SIFT detector (siftdet.hip) ----
// img: device frame (launch_gray layout); keypoints / descriptors to host memory
int sift_detect(slam_ctx* c, const uint8_t* dimg, size_t dstep, int channels, int w, int h, slam_keypoint* out,
                int cap, int* n_out, float* desc);
int sift_detect_batch(slam_ctx* c, hipStream_t s, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                      slam_keypoint* out, int cap, int* n_out, float* desc);
hipError_t launch_gray_batch(slam_ctx* c, hipStream_t s, const uint8_t* frames, int nframes, int w, int h, int channels);
// host cosf / sinf of 360 - angle per keypoint (calcSIFTDescriptor's rotation)
void sift_kp_cs(const slam_keypoint* k, int n, std::vector<float>& cs);

// ---- full ORB detector (orbdet.hip) ----
struct OrbDetLevel { float scale; int w, h, nfeatures; };
// ORB_Impl's level scales, sizes and per-level feature counts (nlevels <= kOrbDetectMaxLevels)
void orb_detect_geometry(int w, int h, int nfeatures, double scale_factor, int nlevels, OrbDetLevel* lv);
// d_frames: nframes packed frames; keypoints / descriptors to device memory at f * cap, counts to the host
int orb_detect_batch(slam_ctx* c, hipStream_t s, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                     int nfeatures, double scale_factor, int nlevels, int fast_threshold, int score_type,
                     slam_keypoint* d_kps, int cap, int32_t* n_out, uint8_t* d_desc);

// ---- two-view triangulation (geom.hip) ----
int triangulate(slam_ctx* c, const double* K, const double* R1, const double* t1, const double* R2,
                const double* t2, const float* pts1, const float* pts2, int n, double* out);

// ---- relative pose: findEssentialMat (RANSAC) + recoverPose (essential.hip) ----
int relative_pose(slam_ctx* c, const float* p1, const float* p2, int n, const double* K, int use_ransac,
                  double prob, double threshold, double dist, double* R, double* t, uint8_t* chirality,
                  uint8_t* ransac_mask, int* passed);

// ---- RANSACPointSetRegistrator pieces shared by essential.hip and pnp.hip ----
// cv::RNG (multiply-with-carry, state (uint64)-1 in ptsetreg.cpp)
struct CvRng {
    uint64_t s;
    unsigned next() { s = (uint64_t)(unsigned)s * 4164903690u + (unsigned)(s >> 32); return (unsigned)s; }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};
// getSubset for callbacks whose checkSubset accepts everything: iters x 5 indices
void ransac_subsets5(int count, int iters, int* idx);
int ransac_update_iters(double p, double ep, int modelPoints, int maxIters);

// ---- solvePnPRansac: EPnP RANSAC + iterative refinement (pnp.hip) ----
int pnp_ransac(slam_ctx* c, const float* op, const float* ip, int n, const double* K, int iterations,
               float reproj, double confidence, double* rvec, double* tvec, uint8_t* mask, int* ninliers,
               int* found);

// ---- undistortion (undistort.hip) ----
// the lens model of the context's cached map
constexpr int kLensBrown = 0, kLensFisheye = 1;

// cv::invert's closed form for 3x3 (DECOMP_LU takes it too); false: det == 0
__host__ __device__ inline bool invert3(const double* a, double* ir)
{
    double d = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) +
               a[2] * (a[3] * a[7] - a[4] * a[6]);
    if (d == 0) return false;
    d = 1. / d;
    ir[0] = (a[4] * a[8] - a[5] * a[7]) * d;
    ir[1] = (a[2] * a[7] - a[1] * a[8]) * d;
    ir[2] = (a[1] * a[5] - a[2] * a[4]) * d;
    ir[3] = (a[5] * a[6] - a[3] * a[8]) * d;
    ir[4] = (a[0] * a[8] - a[2] * a[6]) * d;
    ir[5] = (a[2] * a[3] - a[0] * a[5]) * d;
    ir[6] = (a[3] * a[7] - a[4] * a[6]) * d;
    ir[7] = (a[1] * a[6] - a[0] * a[7]) * d;
    ir[8] = (a[0] * a[4] - a[1] * a[3]) * d;
    return true;
}

// cvRound as the x86 conversion gives it: nearest even; a value outside int, or
// a NaN, is INT_MIN (__double2int_rn would clamp)
__device__ __forceinline__ int cv_round(double v)
{
    const double r = rint(v);
    return (r >= -2147483648.0 && r <= 2147483647.0) ? (int)r : (-2147483647 - 1);
}

// makes the context's cached map that of (model, key, w, h): on a miss `build`
// launches the map kernel on s into undist_xy / undist_frac (already sized);
// orders s after the map's last use on another stream.  Returns a SLAM_* code
int undist_cached_map(slam_ctx* c, hipStream_t s, int w, int h, const double (&key)[30], int model,
                      const std::function<hipError_t()>& build);
// validates the camera model and makes the context's cached map that of
// (K, newK, D, w, h), building it on s when anything changed; returns a SLAM_* code
int undist_prepare(slam_ctx* c, hipStream_t s, int w, int h, const double* K, const double* dist, int ndist,
                   const double* newK);
// records the end of the map's use on s (after the last launch that reads it)
int undist_mark(slam_ctx* c, hipStream_t s);
// remap of nframes packed frames (n x h x w x channels, channels 1 or 3) through the cached map
hipError_t launch_undist_remap(slam_ctx* c, hipStream_t s, const uint8_t* src, uint8_t* dst, int nframes, int w, int h,
                               int channels);
// undist_points: the camera, the 12 coefficients, RR (P, or the identity) and the criteria as kernel arguments
constexpr int kUndistMaxIter = 1000;
struct UndistPointsParams {
    double fx, fy, cx, cy, ifx, ify;
    double k[12];   // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4
    double RR[9];
    double eps;
    int max_iter, use_eps;
};
// validates the model and the criteria (max_iter 1..kUndistMaxIter, eps >= 0; eps == 0: count only)
int undist_points_params(slam_ctx* c, const double* K, const double* dist, int ndist, const double* P, int max_iter,
                         double eps, UndistPointsParams* out);
// n > 0 points read at src + i * src_stride; dst n x 2 packed, err n or null; dst == src allowed at stride 8
hipError_t launch_undist_points(hipStream_t s, const UndistPointsParams& P, const float* src, size_t src_stride, int n,
                                float* dst, float* err);

// ---- the fisheye lens model (fisheye.hip) ----
// undist_prepare for cv::fisheye (ndist == 4, finite; newK's last row (0, 0, 1)): the map goes to the same cache
int fisheye_prepare(slam_ctx* c, hipStream_t s, int w, int h, const double* K, const double* dist, int ndist,
                    const double* newK);
struct FisheyePointsParams {
    double fx, fy, cx, cy;
    double k[4];
    double RR[9];
    double eps;
    int max_iter, use_eps;
};
int fisheye_points_params(slam_ctx* c, const double* K, const double* dist, int ndist, const double* P, int max_iter,
                          double eps, FisheyePointsParams* out);
// as launch_undist_points; a rejected point is (-1000000, -1000000) with a NaN residual
hipError_t launch_fisheye_points(hipStream_t s, const FisheyePointsParams& P, const float* src, size_t src_stride, int n,
                                 float* dst, float* err);

// ---- chessboard calibration (calib.hip, calib_board.cpp, calib_solve.cpp) ----
// the level's downscale s = max(1, ceil(max(w, h) / 1024)) and the candidate bound
// ceil(W / 8) * ceil(H / 8) of a W x H level (two candidates are never within
// Chebyshev distance 7 of each other)
int chess_scale(int w, int h);
int chess_cap(int w, int h);
// candidates of nframes frames (frame f at img + f * frame_stride) into
// c->calib_out: nframes x chess_cap x 3 int32 (x, y, R) in raster order, then nframes counts
hipError_t launch_chess_candidates(slam_ctx* c, hipStream_t s, const uint8_t* img, size_t frame_stride,
                                   size_t row_stride, int channels, int nframes, int w, int h);
// cornerSubPix of n > 0 corners (device, n x 2 f32, in place); d_vx / d_vy: the mask's factors
hipError_t launch_calib_subpix(hipStream_t s, const uint8_t* img, size_t row_stride, int channels, int w, int h,
                               float* d_corners, int n, int win_w, int win_h, int max_iter, double eps,
                               const float* d_vx, const float* d_vy);
// the board_w * board_h strongest of n candidates labelled as a lattice (calib_board.cpp):
// corners in full-resolution pixels, canonical order; false: no complete board
bool label_chessboard(const int32_t* cand, int n, int scale, int board_w, int board_h, float* corners);
// the same from the 2 * board_w * board_h strongest by growing a lattice from a seed, for
// boards a lens bends (tests/fisheye_ref.py label_board_grow is the definition)
bool label_chessboard_grow(const int32_t* cand, int n, int scale, int board_w, int board_h, float* corners);
// calibrateCamera's optimum (calib_solve.cpp); returns a SLAM_* code
int calibrate_camera(const float* obj, const float* img, int nviews, int npts, int size_w, int size_h, double* K,
                     double* D, double* rvecs, double* tvecs, double* rms, int* iterations);
// the same for the model of cv::fisheye::calibrate with the skew fixed at 0: K, D 4 (k1 k2 k3 k4)
int fisheye_calibrate(const float* obj, const float* img, int nviews, int npts, int size_w, int size_h, double* K,
                      double* D, double* rvecs, double* tvecs, double* rms, int* iterations);

// ---- pyramidal Lucas-Kanade tracking (klt.hip) ----
// one frame's pyramid: level l is w[l] x h[l] unpadded 8-bit pixels at pixel offset off[l];
// frames are frame_px apart; the derivative planes (int16 x 2 per pixel) use the same offsets
struct KltLayout {
    int nlevels;
    int w[kKltMaxLevels], h[kKltMaxLevels];
    uint32_t off[kKltMaxLevels];
    uint32_t frame_px;
};
// buildOpticalFlowPyramid's levels for a w x h frame: maxLevel + 1, or fewer by the window rule
KltLayout klt_layout(int w, int h, int win_w, int win_h, int max_level);
// gray + pyrDown levels of nframes frames (frame f at img + f * frame_stride) into pyr (nframes x L.frame_px)
hipError_t launch_klt_pyramid(hipStream_t s, const uint8_t* img, size_t frame_stride, size_t row_stride, int channels,
                              int nframes, const KltLayout& L, uint8_t* pyr);
// calcScharrDeriv of every level of one frame's pyramid into deriv (L.frame_px x 2 int16)
hipError_t launch_klt_scharr(hipStream_t s, const uint8_t* pyr, const KltLayout& L, int16_t* deriv);
// n > 0 points of the previous frame tracked into nframes > 0 candidates; counts (nframes, zeroed
// by the caller) receives the number of status == 1 points per candidate
hipError_t launch_klt_track(hipStream_t s, const KltLayout& L, const uint8_t* prev_pyr, const int16_t* deriv,
                            const uint8_t* next_pyr, int nframes, const float* prev_pts, int n, float* next_pts,
                            uint8_t* status, float* err, int32_t* counts, int win_w, int win_h, int max_count,
                            double eps2, int flags, float min_eig);

// ---- JPEG decoding (jpeg.hip) ----
// frees the context's host-side JPEG state (pinned staging, parsed headers, events)
void jpeg_release(slam_ctx* c);
// ---- JPEG encoding (jpeg_enc.hip) ----
void jpeg_enc_release(slam_ctx* c);

// ---- plane-sweep stereo (mvs.hip) ----
// destroys the context's timing events
void mvs_release(slam_ctx* c);
// where a batch of references goes: the winner's three maps, or (C set) the cost volume itself
struct MvsBatchOut {
    int16_t* plane = nullptr;
    int32_t* cost = nullptr;
    float* inv = nullptr;
    uint16_t* C = nullptr;
    uint8_t* nvalid = nullptr;
};
// the body of slam_mvs_depth_batch_dev, shared with the volume's entry points (mvs_sgm.hip)
int mvs_batch_run(slam_ctx* c, void* stream, const uint8_t* d_frames, int nframes, int w, int h, int channels, int nref,
                  const int32_t* ref_idx, const int32_t* nsrc, const int32_t* src_idx, const double* M, const double* v,
                  const double* planes, int D, int radius, int uniq, int min_views, const MvsBatchOut& out, bool check_only,
                  double* ms);
// ---- TSDF fusion and marching cubes (tsdf.hip, tsdf_host.cpp) ----
// destroys the context's timing events
void tsdf_release(slam_ctx* c);
// argument checks shared by the device entry points and the host twins (tsdf_host.cpp)
int tsdf_check_volume(const void* volume, int nx, int ny, int nz, const double* origin, double voxel);
int tsdf_check_maps(double trunc, const void* frames, int nframes, int w, int h, int channels, const int32_t* frame_idx,
                    const void* inv_depth, const double* P, int nmaps);
// ---- texture atlas (tex.hip, tex_host.cpp) ----
struct TexView;
// destroys the context's timing events
void tex_release(slam_ctx* c);
// argument checks shared by the device entry points and the host twins (tex_host.cpp)
int tex_check_select(const void* ids, int nv, int h, int w, int view0, int nf, const void* best_count, const void* best_view);
int tex_check_fill(const void* V, const void* C, const void* F, int nv, int nf, const void* frames, int n, int h, int w,
                   int channels, const int32_t* frame_idx, const double* P, int nviews, const void* best_count,
                   const void* best_view, int min_pixels, int T, int page, const void* atlas);
// the views' parameter block from P (nviews x 12) and the frame indices (NULL: the identity)
void tex_make_views(const double* P, const int32_t* frame_idx, int nviews, TexView* out);
// ---- place recognition (place.hip, place_host.cpp) ----
// argument checks shared by the device entry points and the host twins (place_host.cpp)
int place_check_assign(const void* desc, int n, const void* cent, int K, int kind);
int place_check_train(const void* desc, int n, int K, int iters, int kind, const void* cent, const void* iters_run);
int place_check_vectors(const int32_t* offsets, int m, const int32_t* weights, int K);
int place_check_score(int nq, int m, int K);
int place_check_topk(int nq, int m, int first, int last, int k);
// ---- loop closing (loop.hip, loop_host.cpp) ----
// argument checks and the sample table shared by the device entry points and the host twins (loop_host.cpp)
int loop_check_ransac(const int32_t* offsets, int L, const double* centres, int H, double tau);
int loop_check_nodes(const double* nodes, int m);
// samples: L x H x 3 indices into each loop's pairs (zeros for a loop with fewer than 3)
void loop_draw_samples(const int32_t* offsets, int L, int H, uint64_t seed, int32_t* samples);
int loop_check_pgo(const double* nodes, int n, const int32_t* edges, const double* meas, const double* weight, int E,
                   double ell, double lambda0, int max_lm, int max_pcg, double pcg_tol, double cost_tol);
// a node's incident (edge, side) entries 2 e + side in ascending edge order: start (n + 1), ent (2 E)
void pgo_build_csr(int n, const int32_t* edges, int E, std::vector<int32_t>& start, std::vector<int32_t>& ent);
// zinv (E x 8) = the inverse measurements, sw (E) = sqrt(weight)
void pgo_edge_constants(const double* meas, const double* weight, int E, double* zinv, double* sw);
// ---- scene rendering (render.hip) ----
// destroys the context's render events
void render_release(slam_ctx* c);

// ---- BA (ba.hip) ----
int ba_solve(slam_ctx* c, double* K4, int nframes, double* ext6, int npoints, double* pts3, int nobs,
             const int32_t* of, const int32_t* op, const double* oxy, int loss, double a,
             int max_iters, slam_ba_summary* sum);

}  // namespace slamhip

// packed keypoint-frame info: frame_info[f] = {offset, count, raw_count, 0}

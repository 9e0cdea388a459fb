/*
 * slamhip -- MI355X (gfx950) implementation of the reference's extract -> match
 * -> windowed-BA hot path, exposed as a plain C ABI (no OpenCV / torch types).
 *
 * Each entry point names the reference interface it replaces (paths relative
 * to the reference repo, FIT-2023-SLAM-indoor/slam-indoor-code):
 *
 *   slam_fast            fastExtractor                 src/mainModule/featureExtraction/fastExtractor.h:19-21
 *   slam_describe        extractDescriptor             src/mainModule/featureMatching/featureMatching.h:12-17
 *   slam_match           matchFeatures + getGoodMatches featureMatchingCPU.cpp:17-43, featureMatchingCommon.cpp:37-50
 *   slam_match_frame     matchFramesPairFeatures (5-arg) featureMatching.h:47-53
 *   slam_knn2            DescriptorMatcher::knnMatch(k=2) featureMatchingCPU.cpp:40 / featureMatchingCUDA.cpp:41
 *   slam_matcher_type    getMatcherTypeIndex           featureMatchingCommon.h:19, featureMatchingCommon.cpp:13-21
 *   slam_select_good     findGoodFramesFromBatch* selection rule  batch.cpp:136-146 / :280-316
 *   slam_ba              bundleAdjustment              src/mainModule/bundleAdjustment/bundleAdjustment.h:50-54
 *   slam_cluster_points  clusterizePoints              src/vizualization/delauney-triangulation/geomAdditionalFunc.cpp:105-163
 *   slam_fit_plane       getBestFittingPlaneByPoints   src/vizualization/delauney-triangulation/bestFittingPlane.cpp:11-40
 *   slam_project_to_plane projectPointOnPlane + makeMesh geomAdditionalFunc.cpp:20-32, bestFittingPlane.cpp:51-63
 *   slam_delaunay_2d     builtInTriangulation + makeMesh's corner lookup  bowyerWatson.cpp:86-105, bestFittingPlane.cpp:67-95
 *   slam_mesh_filter     makeMesh's edge-length filter bestFittingPlane.cpp:96-114
 *   slam_batch_*         the data-parallel candidate scan around them, batch.cpp:59-226
 *
 * Conventions
 *   - Every call returns an int status (SLAM_OK = 0); no C++ exception crosses
 *     the ABI.  The reference's own error behaviour (throw std::exception on an
 *     invalid matcher type, featureMatchingCPU.cpp:37,63) is reproduced by the
 *     host mirror on top of SLAM_E_BAD_MATCHER.
 *   - slam_keypoint / slam_dmatch are byte-identical to cv::KeyPoint (28 B) and
 *     cv::DMatch (16 B), so a cv::Mat / std::vector buffer can be passed as is.
 *   - Host-pointer calls copy in, run on the context's HIP stream and copy out.
 *     slam_batch_* calls take device pointers and an optional HIP stream and
 *     keep every intermediate in HBM.
 *   - A context is NOT re-entrant across threads; the reference calls
 *     matchFramesPairFeatures from threadsCount std::threads (batch.cpp:181-200):
 *     give each thread its own context (contexts on one device share the GPU).
 */
#ifndef SLAMHIP_H
#define SLAMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAMHIP_ABI_VERSION 3   /* 3: slam_sift_detect_batch; 2: ORB device descriptors as 128-byte FP4 (e2m1) +-1, batch async / stage / result_dev calls, synth paths */

enum slam_status {
    SLAM_OK = 0,
    SLAM_E_INVALID_ARG = -1,
    SLAM_E_BAD_MATCHER = -2,   /* reference: throw std::exception() */
    SLAM_E_HIP = -3,
    SLAM_E_CAPACITY = -4,      /* output buffer too small; *n_out holds the needed size */
    SLAM_E_NO_DEVICE = -5,
    SLAM_E_UNSUPPORTED = -6,
    SLAM_E_SOLVER = -7
};

/* MatcherType, featureMatchingCommon.h:8-12 */
enum slam_matcher { SLAM_SIFT_BF = 0, SLAM_SIFT_FLANN = 1, SLAM_ORB_BF = 2 };

/* distance norms (cv::NORM_* values).  SLAM_NORM_DEFAULT picks the reference's
 * CPU build: SIFT_BF -> L2, SIFT_FLANN -> exact BF L2 (what the reference's CUDA
 * build runs, featureMatchingCUDA.cpp:31; the CPU build's FLANN is approximate),
 * ORB -> Hamming.  SLAM_NORM_L1 gives the CUDA build's SIFT_BF (:28). */
enum slam_norm { SLAM_NORM_DEFAULT = 0, SLAM_NORM_L1 = 2, SLAM_NORM_L2 = 4, SLAM_NORM_HAMMING = 6 };

/* cv::FastFeatureDetector::DetectorType */
enum slam_fast_type { SLAM_FAST_TYPE_5_8 = 0, SLAM_FAST_TYPE_7_12 = 1, SLAM_FAST_TYPE_9_16 = 2 };

/* robust losses, getLossFunction priority bundleAdjustment.cpp:131-151 */
enum slam_loss { SLAM_LOSS_NONE = 0, SLAM_LOSS_TRIVIAL = 1, SLAM_LOSS_HUBER = 2,
                 SLAM_LOSS_CAUCHY = 3, SLAM_LOSS_ARCTAN = 4, SLAM_LOSS_TUKEY = 5 };

/* batch.h:5-6 */
#define SLAM_EMPTY_BATCH (-2)
#define SLAM_FRAME_NOT_FOUND (-1)

typedef struct slam_keypoint {      /* == cv::KeyPoint */
    float x, y, size, angle, response;
    int32_t octave, class_id;
} slam_keypoint;

typedef struct slam_dmatch {        /* == cv::DMatch */
    int32_t queryIdx, trainIdx, imgIdx;
    float distance;
} slam_dmatch;

typedef struct slam_ba_summary {    /* the ceres::Solver::Summary fields the reference logs (:119-127) */
    double initial_cost, final_cost;
    int32_t num_residuals, iterations, successful_steps;
    int32_t termination;            /* 0 no convergence, 1 convergence, 2 min radius, 3 failure */
    int32_t usable;                 /* Summary::IsSolutionUsable() */
    double total_time_in_seconds;
} slam_ba_summary;

typedef struct slam_ctx slam_ctx;

/* ---- context ---------------------------------------------------------------- */
int         slam_abi_version(void);
int         slam_device_count(void);              /* cuda::getCudaEnabledDeviceCount, main.cpp:31 */
slam_ctx*   slam_create(int device);               /* NULL if the device cannot be opened */
/* slam_create with the context stream's priority: 0 normal, > 0 the device's
 * highest (latency-critical small launches -- the pipeline's per-frame pose
 * work -- dispatched ahead of a concurrent context's large batch kernels) */
slam_ctx*   slam_create_prio(int device, int priority);
void        slam_destroy(slam_ctx* ctx);
const char* slam_last_error(const slam_ctx* ctx);
int         slam_synchronize(slam_ctx* ctx);

/* ---- reference entry points (host buffers) ------------------------------------ */
/* getMatcherTypeIndex: priority SIFT_BF > SIFT_FLANN > ORB; none -> SLAM_E_BAD_MATCHER */
int slam_matcher_type(int use_sift_bf, int use_sift_flann, int use_orb);

/* fastExtractor(src, pts, threshold, suppression, type).  img: 8-bit, 1/3/4
 * channels (3/4 = BGR/BGRA, converted as cvtColor BGR2GRAY), row stride `step`
 * bytes.  type: SLAM_FAST_TYPE_9_16 (the reference's default and every caller's),
 * _7_12 or _5_8 (FAST_t<12> / <8>); any other -> SLAM_E_INVALID_ARG.
 * *n_out = keypoints found (raster order); SLAM_E_CAPACITY if > cap. */
int slam_fast(slam_ctx* ctx, const uint8_t* img, int w, int h, size_t step, int channels,
              int threshold, int nonmax, int type,
              slam_keypoint* out, int cap, int* n_out);
/* slam_fast on a frame already in device memory (d_img, row stride `step`),
 * queued on `stream` (NULL = the context stream): the device-resident pipeline
 * uploads each frame once (fillVideoFrameBatch, batch.cpp:245 / getNextFrame +
 * fastExtractor, mainCycleInternals.cpp:107-156) and describes / matches it
 * through the slam_batch_* calls below.  Keypoints are returned to host memory. */
int slam_fast_dev(slam_ctx* ctx, void* stream, const uint8_t* d_img, int w, int h, size_t step, int channels,
                  int threshold, int nonmax, int type,
                  slam_keypoint* out, int cap, int* n_out);

/* extractDescriptor(frame, features, type, desc).  kps is IN/OUT: ORB drops
 * keypoints closer than 31 px to the border in place (*n_inout shrinks), as
 * cv::ORB::compute does to the reference's vector.  desc: SIFT n x 128 float
 * (integer values 0..255, CV_32F), ORB n x 32 uint8. */
int slam_describe(slam_ctx* ctx, const uint8_t* img, int w, int h, size_t step, int channels,
                  int matcher_type, slam_keypoint* kps, int* n_inout, void* desc);

/* Full SIFT detector -- not on the reference's own path (its SIFT descriptors
 * are computed on FAST keypoints, slam_describe); SURVEY.md 8(f) rank 2 and the
 * north star's "DoG pyramid, extrema, orientation histogram".  Replaces
 * cv::SIFT::create()->detectAndCompute(img, noArray(), kps, desc) with the
 * defaults (3 octave layers, contrast 0.04, edge 10, sigma 1.6, doubled base
 * image).  Keypoints come in OpenCV's order (KeyPointsFilter::
 * removeDuplicatedSorted), octave packed as OpenCV packs it.  *n_out = total
 * found; SLAM_E_CAPACITY if > cap (the first cap are written).  desc
 * (nullable): cap x 128 float, integer values 0..255.  A frame 1 pixel wide or
 * tall has no octave (as in OpenCV): SLAM_OK and no keypoints. */
int slam_sift_detect(slam_ctx* ctx, const uint8_t* img, int w, int h, size_t step, int channels,
                     slam_keypoint* kps, int cap, int* n_out, float* desc);

/* The same detector over a device-resident batch (round 4): nframes u8 frames
 * (channels 1 or 3, rows packed at w * channels bytes, frames contiguous) in
 * device memory, e.g. decoded video in HBM; every kernel launch covers the
 * whole batch (one pyramid per frame).  Outputs stay on the device: frame f's
 * keypoints go to d_kps[f * cap ..] and its descriptors (nullable) to
 * d_desc[f * cap * 128 ..] (device pointers), each as slam_sift_detect returns
 * them; n_out (host) [f] = keypoints found in frame f, SLAM_E_CAPACITY if any
 * exceeds cap.  Runs on `stream` (NULL: the context's stream) and returns with
 * it drained.  At most 256 frames per call (SLAM_E_INVALID_ARG above; the
 * pyramid needs ~0.5 GB per 1080p frame).  The detector stages through the
 * context's batch buffers: a published slam_batch_* result is released. */
int slam_sift_detect_batch(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes, int w, int h,
                           int channels, slam_keypoint* d_kps, int cap, int32_t* n_out, float* d_desc);

/* Full ORB detector -- the oriented, multi-scale counterpart of slam_describe's
 * ORB (which is cv::ORB::compute on level-0 FAST corners at angle -1):
 * cv::ORB::create(nfeatures, scale_factor, nlevels, 31, 0, 2, score_type, 31,
 * fast_threshold)->detectAndCompute(img, noArray(), kps, desc).  Pyramid by
 * resize(INTER_LINEAR_EXACT) chained level to level, FAST-9/16 + border 31 +
 * retainBest per level, Harris ranking (score_type SLAM_ORB_HARRIS_SCORE) or the
 * FAST score (SLAM_ORB_FAST_SCORE), intensity-centroid angle, steered rBRIEF.
 * Restated from OpenCV 4.8 from upstream knowledge; fidelity to an OpenCV build
 * is not verified (no OpenCV where this is built): the contract is
 * tests/orb_detect_ref.py, byte for byte.  One stated deviation: keypoints come
 * level by level and in raster (y, x) order inside a level (OpenCV's order
 * inside a level is whatever std::nth_element leaves).  Fixed: edgeThreshold =
 * patchSize = 31, firstLevel 0, WTA_K 2, no mask.  nlevels 1..16, scale_factor
 * > 1 (held as the double of the float, as OpenCV does), nfeatures >= 0,
 * channels 1 / 3 / 4, else SLAM_E_INVALID_ARG.  *n_out = total found;
 * SLAM_E_CAPACITY if > cap (the first cap are written).  desc (nullable):
 * cap x 32 bytes, usable with slam_match(..., SLAM_ORB_BF). */
enum slam_orb_score { SLAM_ORB_HARRIS_SCORE = 0, SLAM_ORB_FAST_SCORE = 1 };   /* cv::ORB::ScoreType */
int slam_orb_detect(slam_ctx* ctx, const uint8_t* img, int w, int h, size_t step, int channels, int nfeatures,
                    float scale_factor, int nlevels, int fast_threshold, int score_type, slam_keypoint* kps,
                    int cap, int* n_out, uint8_t* desc);

/* The same detector over a device-resident batch, with slam_sift_detect_batch's
 * conventions: nframes packed u8 frames (channels 1, 3 or 4) in device memory,
 * every kernel launch covers one pyramid level of the whole batch; frame f's
 * keypoints go to d_kps[f * cap ..] and its descriptors (nullable) to
 * d_desc[f * cap * 32 ..] (device pointers, 4-byte aligned), n_out (host) [f] = keypoints found
 * in frame f, SLAM_E_CAPACITY if any exceeds cap.  Runs on `stream` (NULL: the
 * context's) and returns with it drained.  At most 256 frames per call; the
 * scratch is ~3.2 x the gray frames.  A published slam_batch_* result is
 * released. */
int slam_orb_detect_batch(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes, int w, int h,
                          int channels, int nfeatures, float scale_factor, int nlevels, int fast_threshold,
                          int score_type, slam_keypoint* d_kps, int cap, int32_t* n_out, uint8_t* d_desc);

/* reconstruct(calibration, rotation1, transition1, rotation2, transition2,
 * points1, points2, spatialPoints) -- src/mainModule/triangulation/
 * triangulate.cpp:74-100: P_v = K [R_v | t_v], per
 * point the 4 x 4 DLT system solved by OpenCV's Jacobi SVD, X = V(3) / w.
 * K, R: 3 x 3 row-major; t: 3; pts: n x 2 float (Point2f); out: n x 3 double
 * (Point3d). */
int slam_reconstruct(slam_ctx* ctx, const double* K, const double* R1, const double* t1,
                     const double* R2, const double* t2, const float* pts1, const float* pts2,
                     int n, double* out);

/* estimateTransformation(points1, points2, calibrationMatrix, rotationMatrix,
 * translationVector, chiralityMask) -- src/mainModule/translation/
 * cameraTranslation.cpp:32-69: findEssentialMat with
 * RANSAC (RPUseRANSAC, RPRANSACProb, RPRANSACThreshold; without RANSAC the
 * reference's default call, prob 0.999 / threshold 1) then recoverPose with
 * RPDistanceThreshold.  pts: n x 2 float; K: 3 x 3 row-major; R out 3 x 3, t
 * out 3; chirality / ransac_mask (nullable): n bytes.  *passed = recoverPose's
 * count (the reference returns passed > 0). */
int slam_estimate_transformation(slam_ctx* ctx, const float* pts1, const float* pts2, int n,
                                 const double* K, int use_ransac, double prob, double threshold,
                                 double distance_threshold, double* R, double* t,
                                 uint8_t* chirality, uint8_t* ransac_mask, int* passed);

/* solvePnPRansac(objectPoints, imagePoints, cameraMatrix, distCoeffs, rvec,
 * tvec) -- src/mainModule/cycleProcessing/mainCycle.cpp:155-161 (SURVEY.md
 * 8(f) rank 3), the reference's call with an empty distortion Mat and every
 * default (iterations_count 100, reprojection_error 8, confidence 0.99): EPnP
 * RANSAC on minimal sets of 5, then SOLVEPNP_ITERATIVE (Levenberg-Marquardt)
 * on the inliers from the RANSAC model.  obj: n x 3 float (Point3f); img: n x 2
 * float (Point2f); K: 3 x 3 row-major; rvec / tvec out: 3 double each (CV_64F
 * 3 x 1); inlier_mask (nullable): n bytes.  *found = solvePnPRansac's return
 * value (0: no model, rvec / tvec zeroed).  n == 4 (OpenCV: the P3P kernel)
 * returns SLAM_E_UNSUPPORTED; n < 4 (an OpenCV assertion) SLAM_E_INVALID_ARG. */
int slam_solve_pnp_ransac(slam_ctx* ctx, const float* obj, const float* img, int n, const double* K,
                          int iterations_count, float reprojection_error, double confidence,
                          double* rvec, double* tvec, uint8_t* inlier_mask, int* n_inliers,
                          int* found);

/* cv::Rodrigues (cvRodrigues2, host code): n == 3 -> dst = 3 x 3 row-major
 * rotation of the rotation vector src; n == 9 -> dst = rotation vector of the
 * 3 x 3 matrix src (checkRange, SVD orthonormalisation).  Replaces the calls at
 * src/mainModule/cycleProcessing/mainCycle.cpp:162 (after solvePnPRansac) and
 * src/mainModule/bundleAdjustment/bundleAdjustment.cpp:167,195
 * (convertDataForBA / convertDataFromBA).  Other n: SLAM_E_INVALID_ARG. */
int slam_rodrigues(const double* src, int n, double* dst);

/* ---- scene post-processing (src/vizualization, after slamMain / an onlyViz reload) ---- */
/* clusterizePoints -- geomAdditionalFunc.cpp:105-163.  pts: n x 3 float (the
 * Point3f the reference narrows to, main.cpp:61-64); colors: n x 3 uint8
 * (Vec3b); max_distance / euclid_weight / color_weight: the config floats
 * TriangleMaxDistance / TriangleEuclidDistanceWeight / TriangleColorDistance
 * (widened to double as the reference does).  i and j are joined iff
 * sqrt(|p_i - p_j|^2) * euclid_weight + norm(c_i, c_j) * color_weight <
 * max_distance, in the reference's exact arithmetic; labels[i] = the smallest
 * index of i's connected component, *n_components = their number.  The
 * reference's comps are the label classes ordered by label (its order of
 * discovery); it lists the members in DFS pre-order, which labels do not keep.
 * n == 0: SLAM_OK, no launch.  More than ~16.7M points: SLAM_E_UNSUPPORTED. */
int slam_cluster_points(slam_ctx* ctx, const float* pts /* n x 3 */, const uint8_t* colors /* n x 3 */,
                        int n, float max_distance, float euclid_weight, float color_weight,
                        int32_t* labels /* n */, int* n_components);
/* the same on device buffers, queued on `stream` (NULL = the context stream)
 * without a host wait; d_labels doubles as the union-find's parent array */
int slam_cluster_points_dev(slam_ctx* ctx, void* stream, const float* d_pts, const uint8_t* d_colors, int n,
                            float max_distance, float euclid_weight, float color_weight, int32_t* d_labels);
/* counters of the context's last clustering call (waits for it): *pairs =
 * n (n - 1) / 2, *exact_pairs = the pairs that passed the f32 reject and took
 * the f64 path (scripts/scene_bench.py reports the fraction) */
int slam_cluster_last_stats(slam_ctx* ctx, uint64_t* pairs, uint64_t* exact_pairs);

/* getBestFittingPlaneByPoints -- bestFittingPlane.cpp:11-40.  centroid = the
 * f64 mean of the points rounded to f32 (Point3f(mean(row)[0], ...)); normal =
 * the unit eigenvector of the smallest eigenvalue of the centred points'
 * second-moment matrix, signed so that its largest-magnitude component is
 * positive.  (The reference reads its normal with at<double> out of a CV_32F
 * SVD result -- garbage -- so this is its evident intent, DESIGN.md.)  The sums
 * are deterministic: two calls agree bit for bit.  n < 1: SLAM_E_INVALID_ARG. */
int slam_fit_plane(slam_ctx* ctx, const float* pts, int n, float* centroid /* 3 */, double* normal /* 3 */);
/* the device part of slam_fit_plane: sum = sum of the points (f64), mean =
 * sum / n, moments = {xx, xy, xz, yy, yz, zz} of the points minus the f64 mean */
int slam_plane_moments(slam_ctx* ctx, const float* pts, int n, double* sum /* 3 */, double* mean /* 3 */,
                       double* moments /* 6 */);
/* projectPointOnPlane (geomAdditionalFunc.cpp:20-32) + makeMesh's flattening
 * (bestFittingPlane.cpp:51-63) per point, bit for bit: out_xy[i] = the (x, z)
 * of the projected, centred and rescaled point (Point2f), inf / NaN where the
 * reference divides by zero. */
int slam_project_to_plane(slam_ctx* ctx, const float* pts, int n, const float* centroid /* 3 */,
                          const double* normal /* 3 */, float* out_xy /* n x 2 */);

/* builtInTriangulation (bowyerWatson.cpp:86-105: cv::Subdiv2D insert +
 * getTriangleList) with makeMesh's corner lookup (bestFittingPlane.cpp:67-95)
 * folded in: the Delaunay triangulation of n Point2f as index triples.
 *   - Point i is a vertex iff no j < i has x_j == x_i && y_j == y_i (float ==:
 *     makeMesh's "first k that matches"); no triangle names another point.
 *   - The triangles are the Delaunay triangulation of the vertices, complete up
 *     to the convex hull (collinear hull points included), decided by the exact
 *     signs of orient2d and incircle on the f32 coordinates.
 *   - >= 4 cocircular vertices on an empty circle: their polygon is fanned from
 *     its lowest-indexed vertex, a function of the input alone.
 *   - Each triangle is (i, j, k), i its smallest index, counter-clockwise in the
 *     (x, y) given; the list is sorted lexicographically.  Two calls on the same
 *     input return identical bytes.
 * Fewer than 3 vertices, or all collinear: *n_tris = 0, SLAM_OK.  A coordinate
 * that is not finite or outside [-100000, 100000) (Subdiv2D's rectangle; the
 * reference's caller catches its exception and shows no mesh): *n_tris = 0,
 * SLAM_E_INVALID_ARG.  cap too small: SLAM_E_CAPACITY with the needed number in
 * *n_tris (at most 2 n - 5).  n == 0: SLAM_OK, no launch.  The work is
 * O(n^2) exact predicates: meant for single components, not for the cloud. */
int slam_delaunay_2d(slam_ctx* ctx, const float* xy /* n x 2 */, int n, int32_t* tris /* cap x 3 */, int cap,
                     int* n_tris);
/* the same on device buffers (d_xy 8-byte aligned), on `stream` (NULL = the
 * context stream).  Unlike slam_cluster_points_dev it waits for the stream:
 * the status depends on what the kernels found.  *d_n_tris as *n_tris above. */
int slam_delaunay_2d_dev(slam_ctx* ctx, void* stream, const float* d_xy, int n, int32_t* d_tris, int cap,
                         int32_t* d_n_tris);
/* the same contract evaluated on the host with the same predicates and tie rule,
 * one vertex after the other: no context, no device, no launch.  For inputs so
 * small that a launch and its readbacks cost more than the triangulation; the
 * scene drivers (slamhip.scene.make_mesh, the C++ makeMesh) send components
 * below SLAM_DELAUNAY_HOST_BELOW points here. */
#define SLAM_DELAUNAY_HOST_BELOW 64
int slam_delaunay_2d_host(const float* xy /* n x 2 */, int n, int32_t* tris /* cap x 3 */, int cap, int* n_tris);
/* counters of the context's last Delaunay call: predicates evaluated, those of
 * them that needed the exact path, and apex searches that met an exact incircle
 * zero and ran the tie pass
 * (scripts/mesh_bench.py reports them) */
int slam_delaunay_last_stats(slam_ctx* ctx, uint64_t* predicates, uint64_t* exact_predicates, uint64_t* tie_passes);
/* the kernel's own predicates on the device, one thread per case, so that their
 * signs can be tested there (host pointers).  kind[i] = 'o': orient2d(a, b, c),
 * vals[8 i ..] = ax ay bx by cx cy; 'i': incircle(a, b, c, d), ax .. dy; 'c':
 * closer(a, p, q), ax ay px py qx qy; any other kind: SLAM_E_INVALID_ARG.
 * filter_sign[i] = what the f64 filter alone answers (-1, 0, 1, or 2 = undecided),
 * sign[i] = the exact sign as the star kernel gets it (filter, then the exact
 * path).  Coordinates as for slam_delaunay_2d: finite, magnitude <= 100000.
 * n == 0: SLAM_OK. */
int slam_delaunay_predicates(slam_ctx* ctx, const uint8_t* kind /* n */, const float* vals /* n x 8 */, int n,
                             int8_t* filter_sign /* n */, int8_t* sign /* n */);
/* makeMesh's filter (bestFittingPlane.cpp:96-114), host only: copies to `out`,
 * in order, every triangle none of whose three edges is longer than max_size
 * (the reference's 10000) by distance(Point3f, Point3f), geomAdditionalFunc.cpp:16-18:
 * f32 differences, squares summed in f64, strict >.  tris index pts (0 <= index
 * < n, else SLAM_E_INVALID_ARG); out holds n_tris triples; *n_out = the number kept. */
int slam_mesh_filter(const float* pts /* n x 3 */, int n, const int32_t* tris /* n_tris x 3 */, int n_tris,
                     double max_size, int32_t* out, int* n_out);

/* knnMatch(query, train, k = 2): idx/dist nq x 2 (idx -1 where missing). */
int slam_knn2(slam_ctx* ctx, const void* q, int nq, const void* t, int nt,
              int matcher_type, int norm, int* idx, float* dist);

/* matchFeatures: knnMatch(prevDesc = query, curDesc = train, 2) + ratio test
 * (m0.distance < ratio * m1.distance), survivors in query order. */
int slam_match(slam_ctx* ctx, const void* q, int nq, const void* t, int nt,
               int matcher_type, int norm, double ratio,
               slam_dmatch* out, int cap, int* n_out);

/* matchFramesPairFeatures(firstFrameDescriptor, secondFrame, secondFeatures,
 * type, matches): describe the frame (kps IN/OUT as above) then slam_match. */
int slam_match_frame(slam_ctx* ctx, const void* prev_desc, int nprev,
                     const uint8_t* img, int w, int h, size_t step, int channels,
                     int matcher_type, int norm, double ratio,
                     slam_keypoint* kps, int* n_inout,
                     slam_dmatch* out, int cap, int* n_out);

/* candidate selection over per-candidate match counts (batch index order):
 * scan from the tail down to skip_head, good iff count >= required and
 * count >= best so far; first_fit stops at the first good one. */
int slam_select_good(const int32_t* counts, int n, int required, int skip_head, int first_fit);

/* bundleAdjustment(K, window, global).  K4 = {fx, fy, cx, cy} (IN/OUT),
 * ext6 = nframes x {angle-axis[3], t[3]} (IN/OUT, frame 0 held constant),
 * pts3 = npoints x 3 (IN/OUT), observations (frame, point, pixel x, y).
 * Reference Ceres options (:108-114); max_iters <= 0 -> 50. */
int slam_ba(slam_ctx* ctx, double* K4, int nframes, double* ext6, int npoints, double* pts3,
            int nobs, const int32_t* obs_frame, const int32_t* obs_point, const double* obs_xy,
            int loss, double loss_param, int max_iters, slam_ba_summary* summary);

/* ---- device-resident candidate batch (batch.cpp:59-226) ------------------------ */
/* Frames are BGR u8, nframes x h x w x 3, contiguous, in device memory.  Runs
 * gray + FAST (+ORB border filter) + descriptors for every frame, on `stream`
 * (NULL = the context stream).  kp_counts (host, nframes) receives the per-frame
 * keypoint counts -- the batch filter of fillVideoFrameBatch (batch.cpp:247). */
int slam_batch_extract(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes,
                       int w, int h, int threshold, int matcher_type, int32_t* kp_counts);

/* fillVideoFrameBatch's FAST over frames already in device memory
 * (batch.cpp:245-247 with fastExtractor.cpp:7-13): gray + FAST-9 + NMS of every
 * frame in one device pass, no descriptors.  kp_counts (host, nframes)
 * receives the per-frame keypoint counts (the batch filter input); the
 * keypoints stay in the context's batch for slam_batch_get_keypoints /
 * slam_batch_counts.  Descriptor and match calls on such a batch return
 * SLAM_E_INVALID_ARG.  Only with SLAM_OPT_FAST_REUSE = 1 set when this call
 * runs (default 0): a following batch extraction (slam_batch_extract*, SIFT)
 * of the same device pointer, frame count and size at the same threshold takes
 * this pass's FAST results instead of detecting again, unless another FAST /
 * gray launch on the context came in between (the reference runs fastExtractor
 * in fillVideoFrameBatch and again for the descriptors).  Setting it is the
 * caller's promise that the frames' CONTENTS do not change in between: the
 * library compares pointers only, so a buffer refilled (or freed and
 * reallocated at the same address) in between would return the old frames'
 * keypoints and descriptors.  With the default the extraction always detects. */
int slam_batch_fast(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes, int w, int h, int threshold,
                    int32_t* kp_counts);
/* 1 when the context's last batch extraction took slam_batch_fast's results, else 0 */
int slam_batch_fast_reused(const slam_ctx* ctx);

/* match every extracted frame (train) against one query descriptor set that is
 * already in device memory in the context's internal format (see
 * slam_batch_export_desc).  match_counts (host, nframes) receives the ratio-test
 * survivor counts used by the selection rule.
 * Precondition (not checked): the batch path always ranks SIFT L2 candidates
 * with packed keys, which need d^2 < 2^21 - 1.  Extracted descriptors have a
 * norm of at most 518, so every query descriptor must have a norm of at most
 * 518 too, as slam_batch_export_desc produces. */
int slam_batch_match(slam_ctx* ctx, void* stream, const void* d_query, int nq,
                     int norm, double ratio, int32_t* match_counts);

/* slam_batch_extract + slam_batch_match in one call with one host sync (the
 * per-candidate work of findGoodFrameFromBatch, batch.cpp:162-226, when the
 * query set is already on the device).  The kNN launch is queued behind the
 * extraction without waiting for the keypoint counts: it is sized on the
 * previous batch's largest frame and redone at the actual size when a frame
 * outgrows it.  Same outputs as the two calls.  A context's first batch (or a
 * new frame size) takes the two-call path internally. */
int slam_batch_extract_match(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes,
                             int w, int h, int threshold, int matcher_type,
                             const void* d_query, int nq, int norm, double ratio,
                             int32_t* kp_counts, int32_t* match_counts);

/* slam_batch_extract_match whose kNN also waits on `query_ready` (a hipEvent_t,
 * nullable) recorded after the query set's producer -- e.g. the RCCL broadcast
 * of the previous good frame's descriptors.  The extraction is
 * queued ahead of the wait, so only the match is ordered behind the producer. */
int slam_batch_extract_match_ev(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes,
                                int w, int h, int threshold, int matcher_type,
                                const void* d_query, int nq, int norm, double ratio, void* query_ready,
                                int32_t* kp_counts, int32_t* match_counts);

/* slam_batch_extract_match in three halves, none of which waits on the host
 * until the last, so a caller with two contexts can queue the next search's
 * extraction (which needs no previous result) before it selects this one's
 * winner -- the host selection, the winner hand-over and the multi-rank
 * exchanges then overlap device work instead of idling it.
 *   _extract_async  queues gray + FAST + descriptors (on `stream`, NULL = the
 *                   context stream) and the frame-table read-back;
 *   _match_async    queues the kNN + ratio test against d_query behind
 *                   query_ready (a hipEvent_t, nullable), on the same stream;
 *                   for a context's first batch (or a new frame size) it
 *                   first waits for the extraction (the kNN is sized on its counts);
 *   _finish         waits, publishes the batch (the getters, export, result
 *                   calls work on it from here) and returns the counts, as
 *                   slam_batch_extract_match would (match_counts is left
 *                   untouched when no match was queued).
 * Between _extract_async and _finish the context's buffers belong to the batch
 * in flight: every other call that uses them returns SLAM_E_INVALID_ARG. */
int slam_batch_extract_async(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes,
                             int w, int h, int threshold, int matcher_type);
int slam_batch_match_async(slam_ctx* ctx, const void* d_query, int nq, int norm, double ratio, void* query_ready);
int slam_batch_finish(slam_ctx* ctx, int32_t* kp_counts, int32_t* match_counts);
/* the context's own HIP stream (the one NULL stands for) */
void* slam_context_stream(slam_ctx* ctx);

/* bytes per descriptor in the internal device format (SIFT: 128 u8 + i32 norm
 * side array; ORB: the 256 bits as FP4 (e2m1) +-1, 128 bytes) and the size of an exported set. */
size_t slam_batch_desc_bytes(int matcher_type, int n);
/* copy frame f's descriptors (internal format) to d_dst; returns count in *n */
int slam_batch_export_desc(slam_ctx* ctx, void* stream, int frame, void* d_dst, int* n);
/* per-frame counts of the last extract, all frames in one call: FAST keypoints
 * (the batch filter input) and descriptor-bearing keypoints (ORB: after the
 * border filter; the query size of an exported set).  Either array may be NULL.
 * Returns the frame count, or a negative status (cap < frame count).  Host-side
 * state only (no device work).  Replaces per-frame keypoints.size() reads of
 * batch.cpp:245-249 / mainCycle.cpp:99. */
int slam_batch_counts(slam_ctx* ctx, int32_t* raw_counts, int32_t* desc_counts, int cap);
/* host copies of frame f's keypoints / descriptors (reference layout) / matches */
int slam_batch_get_keypoints(slam_ctx* ctx, int frame, slam_keypoint* out, int cap, int* n);
int slam_batch_get_descriptors(slam_ctx* ctx, int frame, void* out, int cap, int* n);
int slam_batch_get_matches(slam_ctx* ctx, int frame, slam_dmatch* out, int cap, int* n);
/* frame f's keypoints and ratio-test matches (what findGoodFrameFromBatch
 * returns for its winner, batch.cpp:92-97) in one call with one host sync */
int slam_batch_get_result(slam_ctx* ctx, int frame, slam_keypoint* kps, int kcap, int* nk,
                          slam_dmatch* matches, int mcap, int* nm);
/* the same result in two halves, for a caller that overlaps the transfer with
 * its next batch: _begin queues the compaction and the copies into a pinned
 * buffer of the context and returns without waiting; _end waits for them (by
 * then usually long done) and copies out.  One result in flight per context
 * (a second _begin first waits for the first); later batch calls may run
 * between the two, on any stream (they wait on the device for the queued
 * copies before rewriting the buffers those read).  _end with a buffer that is
 * too small returns SLAM_E_CAPACITY with the needed sizes and keeps the result
 * pending, so the caller can retry. */
int slam_batch_result_begin(slam_ctx* ctx, int frame);
int slam_batch_result_end(slam_ctx* ctx, slam_keypoint* kps, int kcap, int* nk, slam_dmatch* matches, int mcap,
                          int* nm);

/* the same result into device memory, queued on `stream` (NULL = the context
 * stream) without a host sync: frame f's ratio-test matches (query order) to
 * d_matches and its keypoints to d_kps.  nm = the frame's match count as the
 * caller knows it (the batch's match_counts, or their all-gather across ranks);
 * exactly nm matches are written.  For a multi-rank scan whose winner's owner
 * broadcasts these buffers (SURVEY.md 8(e) exchange 3) with no host round trip. */
int slam_batch_result_dev(slam_ctx* ctx, void* stream, int frame, void* d_matches, int nm, void* d_kps, int kcap);

/* stream ordering at the boundary: everything queued so far on `stream` (NULL =
 * the context stream) happens before anything queued later on `waiter` (a HIP
 * stream; NULL = the legacy default stream).  A device-side wait, no host
 * block.  E.g. a descriptor export (slam_batch_export_desc on the context
 * stream) before an RCCL broadcast that torch orders behind its current stream. */
int slam_order_after(slam_ctx* ctx, void* waiter, void* stream);

/* the same for a point inside the context's last batch extraction
 * (slam_batch_extract / _extract_async / _extract_match): anything queued later
 * on `waiter` starts after that extraction's descriptor kernel has been reached
 * (SLAM_STAGE_DESC_START: gray, FAST and the blur are done) or has finished
 * (SLAM_STAGE_DESC_END).  Lets a second context's next extraction fill the
 * chip while this one's descriptor kernel drains.  SLAM_E_INVALID_ARG before
 * any extraction. */
#define SLAM_STAGE_DESC_START 0
#define SLAM_STAGE_DESC_END 1
int slam_order_after_stage(slam_ctx* ctx, void* waiter, int stage);

/* ---- undistortion ------------------------------------------------------------- */
/* cv::undistort(src, dst, K, D, newK) (OpenCV 4.8, scalar path, uncontracted
 * f64 map; INTER_LINEAR, BORDER_CONSTANT 0) at the seam the reference marks at
 * batch.cpp:244 ("here can be undistortion"), between getNextFrame and
 * fastExtractor.  K: 3x3 row-major; dist: ndist = 4, 5, 8 or 12 doubles in the
 * order k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]] (the calibration file's DC,
 * IOmisc.cpp:68-76); newK: 3x3 or NULL (= K).  ndist 14 (the tilt model):
 * SLAM_E_UNSUPPORTED; any other count, or a singular newK: SLAM_E_INVALID_ARG.
 * The fixed-point map (CV_16SC2 + CV_16UC1, built in cv::undistort's stripes)
 * is computed on the device once per (K, newK, D, w, h) and kept in the context.
 *
 * slam_undistort_batch (cv::undistort per frame, batch.cpp:244): nframes packed
 * frames in device memory (n x h x w x channels, channels 1 or 3) on `stream`
 * (NULL = the context stream), no host sync.  Source and destination must not
 * overlap (SLAM_E_INVALID_ARG); nframes == 0 succeeds without a launch. */
int slam_undistort_batch(slam_ctx* ctx, void* stream, const uint8_t* d_src, uint8_t* d_dst, int nframes, int w,
                         int h, int channels, const double* K, const double* dist, int ndist, const double* newK);
/* cv::undistort of one frame in host memory (batch.cpp:244), any row stride on
 * either side */
int slam_undistort(slam_ctx* ctx, const uint8_t* img, int w, int h, size_t step, int channels, const double* K,
                   const double* dist, int ndist, const double* newK, uint8_t* out, size_t out_step);
/* the cached map of cv::undistort (batch.cpp:244) to host memory, for callers
 * that remap themselves and for the tests: xy = h*w*2 (source x, y as shorts),
 * frac = h*w ((fy << 5) | fx, 5 bits each) */
int slam_undistort_map(slam_ctx* ctx, int w, int h, const double* K, const double* dist, int ndist,
                       const double* newK, int16_t* xy, uint16_t* frac);

/* cv::undistortPoints(src, dst, K, D, noArray(), P, criteria) (OpenCV 4.8,
 * cvUndistortPointsInternal for CV_32FC2 points, uncontracted f64, no tilt): the
 * seams the reference marks at batch.cpp:244 and mainCycleInternals.cpp:142 ("In
 * future we can do UNDISTORTION here") taken for the keypoints that reach
 * geometry instead of the frames.  n points (x, y as floats) are read at src + i *
 * src_stride bytes (src_stride >= 8 and a multiple of 4; 28 reads slam_keypoint.pt
 * in place) and written packed to dst (n x 2); dst == src with stride 8 is
 * allowed, any other overlap is refused.  K and dist as above (only fx, fy, cx,
 * cy of K are used: a skew entry is ignored, as OpenCV ignores it); P: 3x3
 * row-major applied to the normalised result, or NULL for normalised
 * coordinates.  Criteria: max_iter in 1..1000; eps == 0 iterates max_iter times
 * (OpenCV's default is 5, 0), eps > 0 also stops once the reprojection error
 * is below eps pixels.  A criterion without a count is not offered: OpenCV's
 * loops forever on a point that never converges.  OpenCV's exit on a negative
 * inverse radial factor (the point goes back to its start value) is kept.
 * err (n floats, or NULL): the distance in pixels between the input point and
 * the forward model of the returned one, which OpenCV does not report; a point
 * beyond the fold of the radial polynomial has no preimage and keeps a large
 * residual, so callers test err <= tol (a NaN fails it).
 * SLAM_E_UNSUPPORTED for ndist 14; SLAM_E_INVALID_ARG for any other bad count,
 * null pointers with n > 0, n < 0, bad criteria, a bad stride or a device
 * pointer that is not 4-byte aligned; n == 0 succeeds without a launch.
 *
 * slam_undistort_points: host memory in and out, synchronous. */
int slam_undistort_points(slam_ctx* ctx, const float* src, size_t src_stride, int n, const double* K,
                          const double* dist, int ndist, const double* P, int max_iter, double eps, float* dst,
                          float* err);
/* the same on device memory on `stream` (NULL = the context stream), no host sync */
int slam_undistort_points_dev(slam_ctx* ctx, void* stream, const float* d_src, size_t src_stride, int n,
                              const double* K, const double* dist, int ndist, const double* P, int max_iter,
                              double eps, float* d_dst, float* d_err);

/* ---- the fisheye lens model ------------------------------------------------------ */
/* cv::fisheye of OpenCV 4.8 with the skew fixed at 0 (DESIGN.md section 19;
 * tests/fisheye_ref.py defines every value): theta = atan(r), theta_d = theta (1 +
 * k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8), in uncontracted f64 with the
 * library's own atan and tan (csrc/fisheye_math.h).  The five entry points mirror
 * the five above argument for argument; dist is exactly ndist = 4 finite doubles
 * k1 k2 k3 k4 (anything else: SLAM_E_INVALID_ARG).  The model is opt-in: nothing
 * above changes, and a 4-coefficient dist means k1 k2 p1 p2 there.
 *
 * Frames: fisheye::undistortImage(src, dst, K, D, newK), i.e. the fixed-point
 * map of fisheye::initUndistortRectifyMap(K, D, I, newK, size, CV_16SC2) and
 * remap(INTER_LINEAR, BORDER_CONSTANT 0).  The map is built in one piece (no
 * stripes), with the closed-form inverse of newK; a newK (K when NULL) whose
 * last row is not (0, 0, 1), or a singular one: SLAM_E_INVALID_ARG.  It shares
 * the context's map cache, keyed by the model too. */
int slam_fisheye_undistort_batch(slam_ctx* ctx, void* stream, const uint8_t* d_src, uint8_t* d_dst, int nframes, int w,
                                 int h, int channels, const double* K, const double* dist, int ndist,
                                 const double* newK);
int slam_fisheye_undistort(slam_ctx* ctx, const uint8_t* img, int w, int h, size_t step, int channels, const double* K,
                           const double* dist, int ndist, const double* newK, uint8_t* out, size_t out_step);
int slam_fisheye_undistort_map(slam_ctx* ctx, int w, int h, const double* K, const double* dist, int ndist,
                               const double* newK, int16_t* xy, uint16_t* frac);
/* fisheye::undistortPoints(src, dst, K, D, noArray(), P, criteria): Newton on
 * theta from theta_d = |(p - c) / f| clamped to pi/2, for theta_d > 1e-8 (scale 1
 * below).  Criteria as slam_undistort_points (OpenCV's default is 10, 1e-8): eps
 * == 0 iterates max_iter times, eps > 0 also stops once |step| < eps.  A point
 * that did not converge under an eps criterion, or whose theta changed sign, is
 * (-1000000, -1000000), as OpenCV writes it, and its err is NaN; err is
 * otherwise the distance in pixels between the input point and the forward
 * model of the result. */
int slam_fisheye_undistort_points(slam_ctx* ctx, const float* src, size_t src_stride, int n, const double* K,
                                  const double* dist, int ndist, const double* P, int max_iter, double eps,
                                  float* dst, float* err);
int slam_fisheye_undistort_points_dev(slam_ctx* ctx, void* stream, const float* d_src, size_t src_stride, int n,
                                      const double* K, const double* dist, int ndist, const double* P, int max_iter,
                                      double eps, float* d_dst, float* d_err);

/* ---- chessboard calibration ------------------------------------------------------ */
/* The reference's "calibrate" mode (cameraCalibration.cpp:142-203):
 * findChessboardCorners -> cornerSubPix -> calibrateCamera.  The detector is this
 * library's own (tests/calib_ref.py defines it); cornerSubPix
 * restates OpenCV 4.8; calibrateCamera returns the optimum of OpenCV's model.
 *
 * slam_chess_candidates: corner candidates of one frame in host memory (8-bit,
 * channels 1 or 3 = BGR).  The level image is the s x s area mean of the gray
 * frame, s = max(1, ceil(max(w, h) / 1024)) (returned in *scale); out holds
 * *n_out rows (x, y, R) of int32 in level coordinates, raster order.  A level of
 * W x H pixels has at most ceil(W / 8) * ceil(H / 8) candidates; SLAM_E_CAPACITY
 * if more than cap were found (*n_out = the needed number, nothing written). */
int slam_chess_candidates(slam_ctx* ctx, const uint8_t* img, int w, int h, size_t step, int channels, int32_t* out,
                          int cap, int* n_out, int* scale);
/* the same for nframes packed frames resident in HBM (n x h x w x channels), one
 * launch per kernel for the batch, on `stream` (NULL = the context stream).
 * out (host): nframes x cap x 3; n_out (host): nframes counts; synchronous. */
int slam_chess_candidates_dev(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes, int w, int h,
                              int channels, int32_t* out, int cap, int32_t* n_out, int* scale);
/* Host only, no device: the board_w * board_h strongest of n candidates (ties to
 * the lower raster index) labelled as a complete lattice.  corners: board_w *
 * board_h x 2 f32 in full-resolution pixels (scale * x + (scale - 1) / 2), row-major
 * with rows of board_w, right-handed in image coordinates, first corner with the
 * least x + y (ties: least y).  *found = 0 when they are no complete board. */
int slam_label_chessboard(const int32_t* cand, int n, int scale, int board_w, int board_h, float* corners,
                          int* found);
/* Host only, no device: the labeller for boards that a lens bends (DESIGN.md
 * section 19; tests/fisheye_ref.py label_board_grow defines it).  Among the 2 *
 * board_w * board_h strongest candidates a lattice is grown breadth-first from a
 * seed, each new node predicted from its two predecessors and taken when a
 * candidate lies within 0.3 of the local step; the complete board_w x board_h
 * window with the largest response sum that bends smoothly is returned in the
 * order slam_label_chessboard uses.  At most board_w * board_h + 9 seeds are
 * tried.  Integer exact: boards of at most 256 corners and coordinates within
 * +-8192 (level coordinates are below 1024), so that every product of the
 * labeller stays below 2^60 (SLAM_E_INVALID_ARG beyond). */
int slam_label_chessboard_grow(const int32_t* cand, int n, int scale, int board_w, int board_h, float* corners,
                               int* found);
/* findChessboardCorners(gray, Size(board_w, board_h), corners) of a host frame:
 * slam_chess_candidates, then slam_label_chessboard. */
int slam_find_chessboard(slam_ctx* ctx, const uint8_t* img, int w, int h, size_t step, int channels, int board_w,
                         int board_h, float* corners, int* found);
/* the same for nframes resident frames: corners nframes x board_w * board_h x 2,
 * found nframes flags (host) */
int slam_find_chessboard_dev(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes, int w, int h,
                             int channels, int board_w, int board_h, float* corners, int32_t* found);
/* cv::cornerSubPix(gray, corners, Size(win_w, win_h), Size(zero_w, zero_h),
 * TermCriteria(COUNT + EPS, max_iter, eps)) of n corners (host, n x 2 f32, refined
 * in place) on a host frame (channels 1 or 3: the gray FAST sees).  win 1..15 per
 * axis; only the zero zone (-1, -1) is supported (SLAM_E_UNSUPPORTED otherwise);
 * max_iter is clamped to 1..100 as OpenCV does; a start corner outside the image
 * is SLAM_E_INVALID_ARG.  n == 0: SLAM_OK, no launch. */
int slam_corner_subpix(slam_ctx* ctx, const uint8_t* img, int w, int h, size_t step, int channels, float* corners,
                       int n, int win_w, int win_h, int zero_w, int zero_h, int max_iter, double eps);
/* the same on one frame resident in HBM (row stride `step`); corners stay in host
 * memory; synchronous */
int slam_corner_subpix_dev(slam_ctx* ctx, void* stream, const uint8_t* d_img, int w, int h, size_t step,
                           int channels, float* corners, int n, int win_w, int win_h, int zero_w, int zero_h,
                           int max_iter, double eps);
/* Host only, f64: the optimum of calibrateCamera(obj, img, Size(size_w, size_h), K,
 * D, R, T) with default flags: fx fy cx cy, k1 k2 p1 p2 k3 and a rotation vector
 * and translation per view.  obj: npts x 3 f32 with z = 0 (one board for all
 * views); img: nviews x npts x 2 f32.  K 9, D 5, rvecs / tvecs nviews x 3 doubles;
 * *rms = sqrt(sum |r|^2 / (nviews * npts)).  The size moves only the initial
 * principal point.  nviews < 3, npts < 4 or z != 0: SLAM_E_INVALID_ARG; points
 * that give no homography or focal length: SLAM_E_SOLVER. */
int slam_calibrate_camera(const float* obj, const float* img, int nviews, int npts, int size_w, int size_h,
                          double* K, double* D, double* rvecs, double* tvecs, double* rms, int* iterations);
/* Host only, f64: the same for the fisheye lens model, the optimum of
 * cv::fisheye::calibrate's model with the skew fixed at 0 (flags = 0 would
 * estimate it): fx fy cx cy, k1 k2 k3 k4 and a pose per view.  D: 4 doubles.
 * Initial values as OpenCV's: f = max(size_w, size_h) / pi, the principal point
 * at the centre, poses from the homographies of the points undistorted with D =
 * 0.  Arguments, *rms and the status codes as slam_calibrate_camera. */
int slam_fisheye_calibrate(const float* obj, const float* img, int nviews, int npts, int size_w, int size_h,
                           double* K, double* D, double* rvecs, double* tvecs, double* rms, int* iterations);

/* ---- pyramidal Lucas-Kanade tracking ------------------------------------------------ */
/* The reference's second front-end mode (README.md:173 "useFeatureTracker",
 * docs/artifact/2dWorldPoseRefining.md): frame-to-frame tracking of keypoints
 * without descriptors, cv::calcOpticalFlowPyrLK over cv::buildOpticalFlowPyramid
 * (OpenCV 4.8, lkpyramid.cpp / pyramids.cpp), on one 8-bit channel: frames with 3
 * or 4 channels are tracked on the gray FAST sees.  tests/klt_ref.py defines every
 * value; DESIGN.md section 15 has the contract.
 *
 * One deliberate deviation: the five window sums of a point (Ix^2, Ix Iy, Iy^2,
 * diff Ix, diff Iy: integer terms below 2^26) are exact.  OpenCV adds them into
 * f32 accumulators in an order that differs between its scalar, SSE and AVX
 * builds, which therefore disagree in the last bits; here they are summed in
 * int64 and converted to f32 once, round to nearest even, before the 2^-20
 * scale.  Everything downstream is f32 in the source's order.  Further: reads
 * outside a level reflect (101) for intensities at any distance and are 0 for
 * derivatives; a window position whose floor is not an int (NaN, infinite, beyond
 * the int range) is outside; err of a point that no level wrote is 0.
 *
 * Parameters: win_w, win_h in 3..31; max_level 0..8; max_count >= 1 (clamped to
 * 100 as OpenCV does) and eps >= 0 (clamped to 10) of TermCriteria(COUNT + EPS);
 * flags: SLAM_KLT_USE_INITIAL_FLOW | SLAM_KLT_GET_MIN_EIGENVALS.  Anything else,
 * a null pointer that is needed, channels other than 1, 3, 4 or a short row step:
 * SLAM_E_INVALID_ARG.  n == 0 succeeds.
 *
 * slam_klt_pyramid (cv::buildOpticalFlowPyramid + calcScharrDeriv): the levels of a
 * host frame.  *nlevels: the number of levels built (max_level + 1, or fewer when
 * the next level would be no larger than the window); sizes: nlevels x (w, h);
 * gray: the levels' pixels packed one after another, unpadded; deriv (or NULL):
 * int16 {Ix, Iy} per pixel, the same packing.  cap_pixels: the room in gray (and
 * deriv / 2); SLAM_E_CAPACITY with *need_pixels set when it is too small. */
enum slam_klt_flags { SLAM_KLT_USE_INITIAL_FLOW = 4, SLAM_KLT_GET_MIN_EIGENVALS = 8 };
int slam_klt_pyramid(slam_ctx* ctx, const uint8_t* img, int w, int h, size_t step, int channels, int win_w, int win_h,
                     int max_level, int* nlevels, int32_t* sizes, uint8_t* gray, int16_t* deriv, size_t cap_pixels,
                     size_t* need_pixels);
/* cv::calcOpticalFlowPyrLK(prev, next, prevPts, nextPts, status, err, Size(win_w,
 * win_h), max_level, TermCriteria(COUNT + EPS, max_count, eps), flags, min_eig) on
 * two host frames of one size.  prev_pts, next_pts: n x 2 f32 (next_pts is read
 * with SLAM_KLT_USE_INITIAL_FLOW); status n u8; err n f32; all host, synchronous. */
int slam_klt_track(slam_ctx* ctx, const uint8_t* prev, size_t prev_step, const uint8_t* next, size_t next_step, int w,
                   int h, int channels, const float* prev_pts, int n, float* next_pts, uint8_t* status, float* err,
                   int win_w, int win_h, int max_level, int max_count, double eps, int flags, double min_eig);
/* the same on two frames resident in HBM (row stride `step`), on `stream` (NULL =
 * the context stream); points and results stay in host memory; synchronous */
int slam_klt_track_dev(slam_ctx* ctx, void* stream, const uint8_t* d_prev, const uint8_t* d_next, int w, int h,
                       size_t step, int channels, const float* prev_pts, int n, float* next_pts, uint8_t* status,
                       float* err, int win_w, int win_h, int max_level, int max_count, double eps, int flags,
                       double min_eig);
/* one previous frame's points tracked into nframes packed resident candidates
 * (nframes x h x w x channels) in one pass: one pyramid launch per level for the
 * batch, one tracking launch.  next_pts nframes x n x 2, status nframes x n, err
 * nframes x n (host; candidate f's rows equal slam_klt_track_dev on that frame;
 * with SLAM_KLT_USE_INITIAL_FLOW next_pts is read and required, otherwise all three
 * may be NULL together: only the counts are returned); counts (host, nframes):
 * the number of status == 1 points per candidate.  The scratch (pyramids,
 * derivative planes, points) is the context's, grown on demand.  Synchronous. */
int slam_klt_track_batch_dev(slam_ctx* ctx, void* stream, const uint8_t* d_prev, const uint8_t* d_frames, int nframes,
                             int w, int h, int channels, const float* prev_pts, int n, float* next_pts,
                             uint8_t* status, float* err, int32_t* counts, int win_w, int win_h, int max_level,
                             int max_count, double eps, int flags, double min_eig);

/* ---- JPEG decoding: cv::imread / cv::imdecode on baseline JPEG ------------------- */
/* cv::imread(path, IMREAD_COLOR / IMREAD_GRAYSCALE) and cv::imdecode on a JPEG
 * stream (modules/imgcodecs/src/grfmt_jpeg.cpp over libjpeg's defaults: jdhuff.c,
 * jidctint.c jpeg_idct_islow, jdsample.c fancy upsampling, jdcolor.c), restated
 * in 32-bit integers; the numpy restatement tests/jpeg_ref.py is the contract.
 * The reference reads its frames and calibration photos through cv::imread
 * (usePhotosCycle / photosPathPattern; cameraCalibration.cpp:153).
 *
 * Accepted: SOF0 (baseline, Huffman, 8 bit), one interleaved scan; one component,
 * or three YCbCr components with luma sampling 1x1, 2x1 or 2x2 and both chroma
 * 1x1; 8-bit quantisation tables; up to 4 + 4 Huffman tables; restart intervals;
 * width and height 1 .. 16384.  Read besides: the Exif orientation (APP1, tag
 * 0x0112) and the Adobe transform flag (APP14).
 * SLAM_E_UNSUPPORTED: SOF1 / SOF2 and the other frame types (progressive,
 * lossless, arithmetic coding), 12-bit precision, any other sampling, 2 or 4
 * components, RGB-coded streams (libjpeg's rule: without JFIF, Adobe transform 0
 * or the component ids 'R' 'G' 'B'), non-interleaved or multiple scans, 16-bit
 * quantisation tables, larger dimensions.
 * SLAM_E_INVALID_ARG: no SOI, a segment length past the buffer, a DHT whose counts
 * oversubscribe the code space or exceed 256 symbols, a scan that references an
 * undefined table, no frame header or no scan.
 *
 * *status (per image): 0 clean, else the entropy faults met:
 *   1 ran out of bytes, 2 no such Huffman code, 4 a run past coefficient 63,
 *   8 a restart marker missing or out of sequence.
 * The restart interval (or the whole scan of a stream without DRI) that meets a
 * fault stops and its remaining blocks stay zero (gray 128); the output of a
 * flagged stream is the same on host and device and is not libjpeg's recovery.
 * No stream, however corrupt, makes either decoder read or write out of bounds
 * (tests/cpp/jpeg_fuzz_test.cpp runs the shared code under the sanitizers).
 *
 * Deviation: libjpeg-turbo's SIMD IDCT keeps 16-bit intermediates and so differs
 * from its own scalar code on hostile streams (quantisation tables scaled x5 and
 * above); the definition here is the scalar arithmetic, modulo 2^32. */
enum slam_jpeg_sampling { SLAM_JPEG_GRAY = 0, SLAM_JPEG_444 = 0x11, SLAM_JPEG_422 = 0x21, SLAM_JPEG_420 = 0x22 };
struct slam_jpeg_info {
    int32_t width, height;       /* as stored (before the orientation is applied) */
    int32_t channels;            /* 1 or 3 */
    int32_t sampling;            /* SLAM_JPEG_* */
    int32_t restart_interval;    /* MCUs per restart interval, 0 without DRI */
    int32_t segments;            /* independently decodable pieces of the scan */
    int32_t orientation;         /* Exif 1 .. 8; 1 when absent or out of range */
};
/* the message of the calling thread's last failing slam_jpeg_info / slam_jpeg_decode_host ("" when none) */
const char* slam_jpeg_last_error(void);
/* parses and validates the headers; host only */
int slam_jpeg_info(const uint8_t* buf, size_t len, struct slam_jpeg_info* out);
/* the whole decoder on the host (the contract of slam_jpeg_decode, as
 * slam_delaunay_2d_host is slam_delaunay_2d's): out receives height rows of
 * width * channels bytes, `step` bytes apart; channels 3 = BGR (IMREAD_COLOR: a
 * gray stream gives three equal channels), 1 = gray (IMREAD_GRAYSCALE: libjpeg's
 * luma plane of a colour stream).  The orientation is not applied. */
int slam_jpeg_decode_host(const uint8_t* buf, size_t len, uint8_t* out, size_t step, int channels, int* status);
/* the same with the entropy decoding, IDCT, upsampling and colour conversion on
 * the device; buf and out are host memory; synchronous */
int slam_jpeg_decode(slam_ctx* ctx, const uint8_t* buf, size_t len, uint8_t* out, size_t step, int channels,
                     int* status);
/* n streams of one size w x h (host memory) decoded into resident packed BGR
 * frames d_frames (n x h x w x 3, device) on `stream` (NULL = the context
 * stream).  The headers are parsed on the host thread pool, the bytes and tables
 * uploaded once, and three kernels run over the whole batch: jpeg_huff (one lane
 * per restart interval), jpeg_idct, jpeg_upcolor.  Sampling, tables and restart
 * intervals may differ between the streams.  Returns SLAM_OK whenever the batch
 * ran: status[i] (host, n) is a stream's negative SLAM_E_* when it is
 * unsupported, invalid or of another size (its frame is zeroed), else its
 * entropy fault bits.  Synchronous. */
int slam_jpeg_decode_batch_dev(slam_ctx* ctx, void* stream, const uint8_t* const* bufs, const size_t* lens, int n,
                               int w, int h, uint8_t* d_frames, int* status);
/* the Exif orientations (1 .. 8; 1 for a stream that failed) of the n streams of the context's last
 * slam_jpeg_decode_batch_dev, which cv::imread would apply to the decoded frames */
int slam_jpeg_last_orientations(slam_ctx* ctx, int32_t* out, int n);
/* timing of the context's last slam_jpeg_decode_batch_dev, in ms: 0 host parse +
 * segment table, 1 staging + upload, 2 jpeg_huff (with the clearing of the
 * coefficients), 3 jpeg_idct, 4 jpeg_upcolor; bytes (may be NULL): 0 compressed
 * bytes uploaded, 1 table + segment bytes uploaded, 2 coefficient bytes, 3 frame bytes written */
int slam_jpeg_last_timing(slam_ctx* ctx, double* ms5, uint64_t* bytes4);

/* ---- Motion-JPEG: the two stream rules, and chunk-parallel entropy decoding ------ */
/* Parse flags of the _ex entry points (the calls above take none).  SLAM_JPEG_MJPEG:
 * the stream is a frame of a Motion-JPEG video, read as OpenCV's CAP_OPENCV_MJPEG
 * backend and libjpeg read it: an undefined Huffman table slot 0 or 1 is the Annex K
 * table of its class (AVI frames usually carry no DHT; slots 2 and 3 stay undefined),
 * and a frame whose AVI1 APP0 says it is one field of an interlaced pair is
 * SLAM_E_UNSUPPORTED (polarity 0, a progressive frame, is taken).  Unknown flag bits:
 * SLAM_E_INVALID_ARG. */
enum slam_jpeg_flags { SLAM_JPEG_MJPEG = 1 };
int slam_jpeg_info_ex(const uint8_t* buf, size_t len, struct slam_jpeg_info* out, int flags);
int slam_jpeg_decode_host_ex(const uint8_t* buf, size_t len, uint8_t* out, size_t step, int channels, int flags,
                             int* status);
int slam_jpeg_decode_batch_dev_ex(slam_ctx* ctx, void* stream, const uint8_t* const* bufs, const size_t* lens, int n,
                                  int w, int h, uint8_t* d_frames, int* status, int flags);
/* the Annex K table of a class (0 DC, 1 AC) and slot (0 luminance, 1 chrominance):
 * counts16[16] codes per length, the values (vals256: room for 256) and their number */
int slam_jpeg_std_table(int klass, int slot, uint8_t* counts16, uint8_t* vals256, int* nvals);

/* Chunk-parallel entropy decoding (SLAM_OPT_JPEG_SYNC, jpeg_huff.h): a segment
 * without restart markers is decoded by one lane per chunk of its bytes instead of
 * one lane in all: speculative decoding from every chunk start that synchronises
 * with the true symbol sequence (rounds inside a workgroup of `lanes` chunks, then a
 * fixed number of launches that pass states between workgroups), a verified count
 * of blocks and DC sums per chunk, a scan, and a write pass through the serial
 * decoder's own block function.  The result of a stream is by definition the serial
 * decoder's: a segment whose chain of states does not verify, that meets a fault
 * or whose block count is not the expected one is cleared and decoded serially. */
struct slam_jpeg_sync_stats {
    int32_t parallel_segments;     /* segments that took the parallel path */
    int32_t fallback_segments;     /* ... of which were decoded serially after all */
    int32_t chunk_bytes, lanes;    /* the geometry: bytes per chunk, chunks per workgroup */
    int64_t chunks;                /* chunks of the parallel segments */
    int32_t wg_rounds_max;         /* rounds inside a workgroup: the most any workgroup needed in a launch */
    int32_t launch_rounds_max;     /* launches in which a segment still changed: the most any segment needed */
    int64_t wg_rounds_total;       /* ... summed over workgroups and launches */
    int64_t launch_rounds_total;   /* ... summed over segments */
    double ms[5];                  /* device only: jpeg_sync (all launches), jpeg_sync_count, jpeg_sync_scan,
                                      jpeg_sync_write, the fall-back (clear + jpeg_huff); 0 from the host driver */
};
/* of the context's last slam_jpeg_decode_batch_dev[_ex] (all zero when SLAM_OPT_JPEG_SYNC was 0) */
int slam_jpeg_last_sync(slam_ctx* ctx, struct slam_jpeg_sync_stats* stats);
/* slam_jpeg_decode_host_ex with every segment of more than one chunk on the
 * parallel path (SLAM_OPT_JPEG_SYNC = 2), run on the host by the functions the
 * kernels share, in their round structure and geometry: pixels and status are
 * slam_jpeg_decode_host_ex's, and stats (nullable) are what the device reports for
 * the same stream.  chunk_bytes: 0 = the default, or a power of two from 16 to 1024. */
int slam_jpeg_decode_host_sync(const uint8_t* buf, size_t len, uint8_t* out, size_t step, int channels,
                               int chunk_bytes, int flags, int* status, struct slam_jpeg_sync_stats* stats);

/* ---- Motion-JPEG AVI container (avi_parse.cpp): host only ----------------------- */
/* The frames of the first video stream of an AVI file held in memory, found by
 * walking the chunks: every top-level RIFF (AVI and OpenDML AVIX), LIST hdrl (avih,
 * the first strl whose strh is 'vids', its strf BITMAPINFOHEADER), every LIST movi
 * and nested LIST rec; the NNdc / NNdb chunks of that stream in file order.  Other
 * streams, JUNK and every index (idx1, indx, ixNN) are skipped: the walk is the
 * definition (OpenCV trusts idx1; the two agree on well-formed files).  A video
 * chunk of no bytes is a dropped frame and repeats the one before it (a first
 * frame of no bytes stays empty).  offsets / sizes (nullable, cap entries): the
 * frames' byte ranges in buf; info->frames is the number found, also beyond cap.
 * SLAM_E_UNSUPPORTED: no video stream, or a codec other than MJPG (any letter case)
 * or jpeg.  SLAM_E_INVALID_ARG: not RIFF / AVI, a chunk or list that runs past its
 * parent or the buffer, no hdrl.  slam_avi_last_error: the message of the calling
 * thread's last failing slam_avi_index. */
struct slam_avi_info {
    int32_t width, height;
    uint32_t rate, scale;          /* frames per second = rate / scale */
    int64_t frames;
    uint32_t handler, compression; /* FourCCs (little endian): strh's fccHandler, strf's biCompression */
    int32_t stream;                /* the stream's number NN */
};
const char* slam_avi_last_error(void);
int slam_avi_index(const uint8_t* buf, size_t len, struct slam_avi_info* info, uint64_t* offsets, uint64_t* sizes,
                   size_t cap);

/* ---- JPEG encoding: cv::imencode / cv::imwrite of baseline JPEG ------------------ */
/* What cv::imencode(".jpg") and PIL's save(format="JPEG") run: libjpeg's encoder
 * with its defaults (jpeg_set_defaults, jpeg_set_quality(q, TRUE), JDCT_ISLOW, the
 * Annex K Huffman tables, no optimisation, no smoothing), restated in 32-bit
 * integers; the numpy restatement tests/jpeg_enc_ref.py is the contract, and the
 * host encoder and the kernels equal it byte for byte.
 * Frames: 8-bit, 3 channels (BGR) or 1 (gray; written as a gray stream whatever the
 * sampling), 1 .. 16384 pixels a side.  sampling: SLAM_JPEG_444, _422, _420, or
 * SLAM_JPEG_GRAY (a BGR frame's luma alone).  quality is clamped to 1 .. 100.
 * restart_interval: MCUs per restart interval, 0 .. 65535, 0 = none.
 * Not written: optimised tables, progressive / arithmetic / 12-bit streams, 4:4:0
 * and 4:1:1, Exif.
 * The stream length is known before a byte is written: size always reports the
 * length needed.  When it exceeds the capacity, the first cap bytes are written,
 * nothing at or past the capacity, status carries SLAM_JPEG_ENC_OVERFLOW and the
 * call still returns SLAM_OK.  SLAM_JPEG_ENC_CATEGORY: a coefficient past the
 * Huffman tables' categories (11 for DC, 10 for AC), which 8-bit input cannot
 * produce; it is clamped, and no table is indexed past its end. */
enum slam_jpeg_enc_status { SLAM_JPEG_ENC_OVERFLOW = 1, SLAM_JPEG_ENC_CATEGORY = 2 };
/* A capacity no stream of this geometry exceeds (0 for arguments slam_jpeg_encode
 * refuses).  Derivation: a block is at most an 11-bit DC code with 11 more bits and
 * 63 AC terms of a 16-bit code with 10 more bits, 1660 bits; every restart interval
 * adds at most one byte of padding; every scan byte may be FF and so doubles;
 * every interval but the last is followed by a 2-byte RSTn; the markers SOI .. SOS
 * are 629 bytes at the most (640 is taken); EOI is 2:
 *   640 + 2 (ceil(1660 blocks / 8) + intervals) + 2 intervals + 2. */
size_t slam_jpeg_encode_bound(int h, int w, int sampling, int restart_interval);
/* the whole encoder on the host (the contract of slam_jpeg_encode) */
int slam_jpeg_encode_host(const uint8_t* img, int h, int w, int channels, size_t row_step, int quality, int sampling,
                          int restart_interval, uint8_t* out, size_t cap, size_t* size, int* status);
/* the message of the calling thread's last failing slam_jpeg_encode_host / slam_jpeg_encode_bound */
const char* slam_jpeg_enc_last_error(void);
/* one host image through the device encoder (status nullable) */
int slam_jpeg_encode(slam_ctx* ctx, const uint8_t* img, int h, int w, int channels, size_t row_step, int quality,
                     int sampling, int restart_interval, uint8_t* out, size_t cap, size_t* size, int* status);
/* n resident frames of one size (frame i at frames_dev + i frame_step, rows
 * row_step apart) into n streams, one set of launches for the batch: stream i goes
 * to out_dev + i cap_per_image, its length to sizes_dev[i], its status bits to
 * status_dev[i] (all device memory).  n: 1 .. 65535 (an image is a row of the
 * launch grid), else SLAM_E_INVALID_ARG.  stream: a hipStream_t, NULL = the context's.
 * Synchronous: the unstuffed lengths are read back once mid-way to size the
 * stuffing pass. */
int slam_jpeg_encode_batch_dev(slam_ctx* ctx, void* stream, const uint8_t* frames_dev, int n, int h, int w, int channels,
                               size_t row_step, size_t frame_step, int quality, int sampling, int restart_interval,
                               uint8_t* out_dev, size_t cap_per_image, uint64_t* sizes_dev, int32_t* status_dev);
/* timing of the context's last device encode, in ms: 0 jpeg_enc_dct, 1
 * jpeg_enc_count, 2 the tile scans with jpeg_enc_intervals, 3 the readback of the
 * lengths, 4 clearing + jpeg_enc_pack, 5 jpeg_enc_ffcount + its scan, 6
 * jpeg_enc_write; bytes (may be NULL): 0 frames read, 1 coefficients (written
 * once, read twice), 2 unstuffed streams, 3 read back mid-way */
int slam_jpeg_enc_last_timing(slam_ctx* ctx, double* ms7, uint64_t* bytes4);

/* ---- scene rendering (the cv::viz window of vizualizePointsAndCameras, headless) -- */
/* A deterministic z-buffer rasteriser for the onlyViz scene: the coloured cloud
 * (WCloud: n_pts x 3 f32 points, n_pts x 3 u8 BGR colours), the meshes (WMesh:
 * n_faces x 3 int32 indices into the cloud, vertex colours = the cloud's) and the
 * trajectory (WTrajectory: n_lines x 6 f32 segments a b, n_lines x 3 u8 BGR).
 * tests/render_ref.py is the definition and the kernels equal it byte for byte
 * from any launch order; csrc/render_setup.h states every rounding.
 *   view    12 f64: R (3 x 3, row major) then t of the camera-to-world pose, as
 *           viz::Viz3d::setViewerPose takes an Affine3d.  The camera looks along
 *           +z, x right, y down; p_cam = R^T (p - t).
 *   cam     6 f64: fx fy cx cy near far.  u = fx X / Z + cx, v = fy Y / Z + cy,
 *           pixel (i, j) covers [i, i + 1) x [j, j + 1).
 *   points  a square of point_size (odd, 1 .. 7) pixels about the pixel holding
 *           the projection, at the point's 1/Z; culled outside near <= Z <= far
 *           or the viewport
 *   lines   clipped, endpoints snapped to pixels, walked from the endpoint lower
 *           in (y, x) by the midpoint rule, 1/Z affine along the major axis
 *   faces   clipped against near, far and a guard band of 32768 pixels about the
 *           viewport, fanned, snapped to 1/16 pixel, two-sided, int64 edge
 *           functions with the top-left rule, exact integer Gouraud blend,
 *           1/Z affine in screen space, rounded to f32.  No lighting.
 * Per pixel the smallest key (~bits(f32 1/Z) << 32 | kind << 30 | index) wins,
 * kind 0 point, 1 line, 2 face: the nearer fragment; at equal depth a point
 * beats a line beats a face, then the lower index.  Outputs per view: d_out
 * h x w x 3 BGR (white where nothing is drawn), d_ids (nullable) the key's low
 * word as an int32 ((id >> 30) & 3 is the kind, id & 0x3fffffff the index, so a
 * face's id is negative) or -1, d_depth (nullable) f32 1/Z or 0.  A primitive with a
 * non-finite coordinate or a face index outside the cloud is skipped.
 * views is host memory (nv x 12), everything d_* is device memory; the work
 * runs on `stream` (NULL = the context stream) in chunks of views that fit the
 * context's key buffer (chunk_views > 0 lowers the chunk; the result does not
 * depend on it) and the call returns when it is done.  raster_mode: 0 = faces
 * by bounding-box size, 1 = a thread per face, 2 = a wave per tile for every
 * face, 3 = as 2 with a tile list of 64 entries, so that nearly every tile takes
 * the path of a full list (same result; for tests).  w, h 1 .. 8192; fx, fy finite and non-zero;
 * 0 < near < far; at most 2^30 primitives of a kind; else SLAM_E_INVALID_ARG
 * and nothing is launched.  nv = 0 and no primitives (white frames) are fine. */
int slam_render_views_dev(slam_ctx* ctx, void* stream, const float* d_pts, const uint8_t* d_colors, int n_pts,
                          const int32_t* d_faces, int n_faces, const float* d_lines, const uint8_t* d_line_colors,
                          int n_lines, const double* views, int nv, const double* cam, int w, int h, int point_size,
                          uint8_t* d_out, int32_t* d_ids, float* d_depth, int chunk_views, int raster_mode);
/* one view of host primitives into host memory (ids, depth nullable); synchronous */
int slam_render(slam_ctx* ctx, const float* pts, const uint8_t* colors, int n_pts, const int32_t* faces, int n_faces,
                const float* lines, const uint8_t* line_colors, int n_lines, const double* view, const double* cam, int w,
                int h, int point_size, uint8_t* out, int32_t* ids, float* depth);
/* the context's last rendering call, summed over its views.  stats[5]: 0 primitives
 * in (views x primitives), 1 skipped (non-finite, bad index, or outside the
 * fixed-point range), 2 clipped away (nothing left inside the clip volume or the
 * viewport), 3 rasterised (points, segments and fan triangles walked), 4 fragments
 * tested.  ms[4] (nullable), HIP events on the call's stream: 0 clear, 1 points +
 * lines, 2 faces (set-up and both raster paths), 3 resolve. */
int slam_render_last_stats(slam_ctx* ctx, uint64_t* stats, double* ms);

/* ---- options ------------------------------------------------------------------ */
/* Per-context choices; all but SLAM_OPT_PNP_SUMS (below) never change results.  SLAM_OPT_SIFT_KERNEL picks the
 * kernel for SIFT descriptors of keypoints sharing one angle and size (FAST
 * keypoints): AUTO = band-staged scatter when its schedule reproduces the raster
 * order, else the per-target gather, else the general kernel; the others force
 * one (the parity tests run each against the oracle); a forced kernel whose
 * schedule does not apply to the keypoints makes the describing call fail with
 * SLAM_E_UNSUPPORTED instead of running another.  SLAM_OPT_SIFT_BAND_SPLIT: how
 * the band kernel runs a launch's last, partial round of keypoint groups --
 * OFF = whole walks, AUTO (default) = as part-walks that each finish some of
 * the descriptor rows (two: rows 0-1 and 2-3; four: one row each) when that
 * round would leave at most one wave per CU, ALL / ALL4 = every group as two /
 * four part-walks (the tests' way to run those paths on every keypoint).
 * Unknown option or value: SLAM_E_INVALID_ARG. */
enum slam_option { SLAM_OPT_SIFT_KERNEL = 1, SLAM_OPT_SIFT_BAND_SPLIT = 2, SLAM_OPT_PNP_SUMS = 3,
                   SLAM_OPT_FAST_REUSE = 4, SLAM_OPT_JPEG_LANES = 5, SLAM_OPT_JPEG_SYNC = 6, SLAM_OPT_JPEG_CHUNK = 7 };
/* SLAM_OPT_JPEG_SYNC: which segments of a batch decode take the chunk-parallel path
 * (slam_jpeg_sync_stats above): 0 (default) = none, 1 = those of at least 16384
 * bytes, 2 = every one of more than one chunk (for tests).  SLAM_OPT_JPEG_CHUNK: bytes
 * per chunk, a power of two from 16 to 1024; 0 (default) = 256.  Neither changes results. */
/* SLAM_OPT_JPEG_LANES: how many lanes of a wave of jpeg_huff take a segment each
 * (1 .. 64); 0 (default) = one per wave until the device's wave slots are full,
 * then as many as the segment count needs.  Never changes results. */
/* SLAM_OPT_FAST_REUSE: 1 = slam_batch_fast's results may be taken by the next
 * batch extraction of the same frames (see slam_batch_fast for the contract the
 * caller accepts); 0 (default) = every extraction detects. */
/* SLAM_OPT_PNP_SUMS (the one option that changes results): how solvePnPRansac's
 * refinement forms J'J, J'e and |e|^2 over the inliers each LM step --
 * ORDERED (default) = sequential sums in the oracle's order (bit-exact poses,
 * 2 m dependent f64 adds per sum: ~90 us per step at m = 1750), PAIRWISE = per-
 * thread partial sums and a fixed tree (deterministic; poses within 1e-9 of
 * the oracle's, the same inlier mask; a few us per step). */
enum slam_pnp_sums { SLAM_PNP_SUMS_ORDERED = 0, SLAM_PNP_SUMS_PAIRWISE = 1 };
enum slam_band_split { SLAM_BAND_SPLIT_OFF = 0, SLAM_BAND_SPLIT_AUTO = 1, SLAM_BAND_SPLIT_ALL = 2,
                       SLAM_BAND_SPLIT_ALL4 = 3 };
/* SLAM_SIFT_KERNEL_COLS: the one-keypoint-per-lane, two-column-pass variant of the
 * band kernel (same descriptors; an A/B kernel, never picked by AUTO).
 * SLAM_SIFT_KERNEL_COLW: one descriptor column per wave (same descriptors). */
enum slam_sift_kernel { SLAM_SIFT_KERNEL_AUTO = 0, SLAM_SIFT_KERNEL_BAND = 1, SLAM_SIFT_KERNEL_TAB = 2,
                        SLAM_SIFT_KERNEL_GENERAL = 3, SLAM_SIFT_KERNEL_COLS = 4, SLAM_SIFT_KERNEL_COLW = 5 };
int slam_set_option(slam_ctx* ctx, int option, int value);
/* the SLAM_SIFT_KERNEL_* that ran the context's last SIFT descriptor launch (0 before any) */
int slam_last_sift_kernel(const slam_ctx* ctx);

/* which kNN kernel the context's last matcher launch ran (slam_knn2, slam_match,
 * slam_batch_match and their fused / asynchronous forms).  *mode: the key mode
 * (SLAM_KNN_MODE_*), *tsplit: the train-set split count of the launch (grid z),
 * *variant: the template instance (SLAM_KNN_VARIANT_*), with
 * SLAM_KNN_VARIANT_XCD or'ed in when the blocks ran in XCD-contiguous order.
 * Any pointer may be NULL.  Returns SLAM_OK, or SLAM_E_INVALID_ARG before the
 * context's first launch.  For tests: the choice of kernel is internal. */
enum slam_knn_mode { SLAM_KNN_MODE_L2 = 0, SLAM_KNN_MODE_SQRT = 2, SLAM_KNN_MODE_L2_PACKED = 3,
                     SLAM_KNN_MODE_HAMMING_PACKED = 4, SLAM_KNN_MODE_L1_PACKED = 5 };
enum slam_knn_variant { SLAM_KNN_VARIANT_NONE = 0, SLAM_KNN_VARIANT_MFMA = 1, SLAM_KNN_VARIANT_MFMA_PK_QT2 = 2,
                        SLAM_KNN_VARIANT_MFMA_PK_QT1 = 3, SLAM_KNN_VARIANT_PIPE_QT2 = 4,
                        SLAM_KNN_VARIANT_PIPE_QT1 = 5, SLAM_KNN_VARIANT_L1 = 6, SLAM_KNN_VARIANT_XCD = 0x100 };
int slam_last_knn_launch(const slam_ctx* ctx, int* mode, int* tsplit, int* variant);

/* which forms of the full SIFT detector the context's last slam_sift_detect /
 * slam_sift_detect_batch call ran (the last one that launched anything: a call
 * that returns before its first launch leaves them as they were).  *forms: the
 * SLAM_SD_FORM_* bits -- DoG planes stored by the blurs (else taken from the
 * Gaussian layers), pyramid and extrema tiles in XCD-contiguous order, and, set
 * by the call's descriptor launch only (no bits without one): the staged
 * descriptor kernel (else the direct one), two cells per lane, its blocks in
 * XCD-contiguous order.  *refine_blocks: sd_refine's grid size.  Either pointer
 * may be NULL.  Returns SLAM_OK, or SLAM_E_INVALID_ARG before the context's first
 * such call.  For tests: the forms are chosen once per process and never
 * change results. */
enum slam_sd_form { SLAM_SD_FORM_DOG_PLANES = 1, SLAM_SD_FORM_XCD = 2, SLAM_SD_FORM_DESC_STAGED = 4,
                    SLAM_SD_FORM_DESC_CPL2 = 8, SLAM_SD_FORM_DESC_XCD = 16 };
int slam_last_sift_detect_forms(const slam_ctx* ctx, int* forms, int* refine_blocks);

/* ---- profiling hooks (bench.py) ---------------------------------------------- */
/* average duration (ms) of the last batch's launches of one kernel family,
 * measured with HIP events on the launch stream: 0 fast, 1 sift_desc, 2 knn,
 * 3 orb_desc, 4 sift_blur, 5 ratio/compact, 6 klt pyramids + derivatives, 7 klt_track,
 * 8 orbdet_gray + orbdet_down, 9 orbdet_select + orbdet_pack, 10 orbdet_harris + orbdet_angle,
 * 11 orbdet_emit */
int slam_profile_enable(slam_ctx* ctx, int on);
int slam_profile_read(slam_ctx* ctx, int family, double* avg_ms, int* launches);

/* ---- synthetic indoor sequence (test / bench input, host memory) ---------------- */
/* camera paths: DRIFT zooms in without bound (the texture in view thins out
 * along the sequence: the round-1..3 fixtures and tests); STEADY is a bounded
 * loop whose FAST count stays near frame 0's for any frame index (the bench's
 * configs[1] batches: every candidate at 10k +- 10 % keypoints) */
enum slam_synth_path { SLAM_SYNTH_DRIFT = 0, SLAM_SYNTH_STEADY = 1 };
int slam_synth_sequence(int w, int h, int first, int count, uint64_t seed, int path, uint8_t* out_bgr);
/* the same frames rendered on the device into d_out (count x h x w x 3, on
 * `stream`, NULL = the context stream), byte-identical to slam_synth_sequence:
 * a video "decoded" straight into HBM for the device-resident pipeline */
int slam_synth_sequence_dev(slam_ctx* ctx, void* stream, int w, int h, int first, int count, uint64_t seed, int path,
                            uint8_t* d_out);
/* slam_synth_sequence(..., SLAM_SYNTH_DRIFT, ...) */
int slam_synth_frames(int w, int h, int first, int count, uint64_t seed, uint8_t* out_bgr);

/* ---- dense points: plane-sweep stereo (multi-view densification) ---------------- */
/* An opt-in stage between the poses and the mesh.  The
 * definition of every value is tests/mvs_ref.py; the device and the host twin
 * equal it bit for bit.  Frames are 8-bit with channels 1 or 3 (BGR); gray is the
 * fixed-point conversion FAST sees.  The reference has no such stage.
 *
 * Projection of reference pixel (x, y) into a source at inverse depth w, from the
 * caller's M (3 x 3 row-major, mathematically K R K^-1) and v (3, K t), in f64 in
 * this order without contraction:
 *   q_i = (M[i][0] x + M[i][1] y) + M[i][2],  h_i = q_i + w v[i],  u = h_0 / h_2,  vv = h_1 / h_2,
 * valid iff h_2 > 0, -0.5 <= u < W - 0.5 and -0.5 <= vv < H - 0.5 (a NaN or an
 * infinity is invalid), then ix = (int)floor(u + 0.5), iy likewise.
 *
 * slam_mvs_census_dev: the 9 x 7 census of nframes resident frames (n x h x w x
 * channels) into d_out (n x h x w uint64, device): bit b, counted in the order dy
 * = -3..3 outer, dx = -4..4 inner with the centre skipped, is set iff the gray at
 * (clamp(x + dx), clamp(y + dy)) is below the centre's; bits 62 and 63 are 0.
 * One launch; synchronous.  w > 4096: SLAM_E_UNSUPPORTED. */
int slam_mvs_census_dev(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                        uint64_t* d_out);
/* Depth maps of nref references among nframes resident frames.  Reference i is
 * frame ref_idx[i] with nsrc[i] (1..4) sources src_idx[4 i ..], their M at M + 36
 * i + 9 s, v at v + 12 i + 3 s, and D (4..256) inverse depths planes[D i ..].  The
 * census is computed once per distinct frame of the call.  Per pixel and plane d
 * the cost of a source is the Hamming distance of the two census words (64 when
 * the projection is invalid), summed over the (2 radius + 1)^2 window (radius
 * 0..3, coordinates clamped to the image, every window pixel projected itself)
 * and over the sources: C[d]; nvalid[d] counts the sources valid at the pixel.
 * best = the lowest d of minimal C, second = the least C with |d - best| > 1; the
 * pixel is accepted iff C[best] * 100 < uniq * second (uniq 1..100) and
 * nvalid[best] >= min_views (1..S).  With a, b, c = C[best - 1], C[best], C[best +
 * 1], 0 < best < D - 1 and den = a - 2 b + c > 0: off = (double)(a - c) / (double)(2
 * den), else 0; wq = w[best] + off (w[best + 1] - w[best]) for off >= 0, w[best] +
 * off (w[best] - w[best - 1]) below (w[best] at the two ends).
 * Outputs (device, nref x h x w): plane int16 = best, cost int32 = C[best],
 * inv_depth f32 = (float)wq when accepted, else 0.  The cost volume is never
 * stored.  Synchronous.  S outside 1..4, D outside 4..256, radius > 3, uniq or
 * min_views out of range, an index outside the frames, or a non-finite M, v or
 * plane: SLAM_E_INVALID_ARG; w > 4096: SLAM_E_UNSUPPORTED.  Huge finite values are
 * legal and come out invalid. */
int slam_mvs_depth_batch_dev(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes, int w, int h,
                             int channels, int nref, const int32_t* ref_idx, const int32_t* nsrc,
                             const int32_t* src_idx, const double* M, const double* v, const double* planes, int D,
                             int radius, int uniq, int min_views, int16_t* d_plane, int32_t* d_cost,
                             float* d_inv_depth);
/* Pairwise consistency filter and point emission over nmaps depth maps
 * (d_inv_depth: nmaps x h x w f32, device); map i belongs to frame frame_idx[i]
 * and lists nnbr[i] (0..4) neighbour maps nbr_idx[4 i ..] with M and v of the
 * motion map i -> neighbour, laid out as above.  A pixel with wi = inv_depth > 0
 * is consistent with neighbour j iff its projection at w = (double)wi is valid,
 * wj (the neighbour's value at the nearest pixel) > 0 and fabs(h_2 (double)wj /
 * (double)wi - 1.0) <= eps.  It is kept iff its consistent count >= min_consistent
 * (0..4), x % step == 0 and y % step == 0, and it lies outside the radius + 4
 * border.  Survivors leave in raster order, map after map: points (host, cap x 3
 * f64) X = c + (B (x, y, 1)) * (1.0 / (double)wi) with B (9) and c (3) of map i at B
 * + 9 i and c + 3 i, evaluated as ((B[k][0] x + B[k][1] y) + B[k][2]); colors
 * (host, cap x 3) the frame's BGR bytes (gray three times for one channel).
 * *n_out = the number of survivors; SLAM_E_CAPACITY when it exceeds cap (nothing
 * written).  Synchronous. */
int slam_mvs_fuse_dev(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                      int nmaps, const int32_t* frame_idx, const float* d_inv_depth, const int32_t* nnbr,
                      const int32_t* nbr_idx, const double* M, const double* v, const double* B, const double* c,
                      double eps, int min_consistent, int step, int radius, double* points, uint8_t* colors, int cap,
                      int* n_out);
/* slam_mvs_depth_batch_dev for one reference and its S sources in host memory
 * (rows `step` bytes apart); M (S x 9), v (S x 3), planes (D); outputs h x w in
 * host memory. */
int slam_mvs_depth(slam_ctx* ctx, const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h, size_t step,
                   int channels, const double* M, const double* v, const double* planes, int D, int radius, int uniq,
                   int min_views, int16_t* plane, int32_t* cost, float* inv_depth);
/* slam_mvs_fuse_dev for nmaps host frames (frames[i] is map i's) and host maps
 * (inv_depth: nmaps x h x w). */
int slam_mvs_fuse(slam_ctx* ctx, const uint8_t* const* frames, int w, int h, size_t step, int channels, int nmaps,
                  const float* inv_depth, const int32_t* nnbr, const int32_t* nbr_idx, const double* M, const double* v,
                  const double* B, const double* c, double eps, int min_consistent, int step_px, int radius,
                  double* points, uint8_t* colors, int cap, int* n_out);
/* HIP-event times (ms) of the kernels of the context's last slam_mvs_depth_batch_dev
 * (ms[0] mvs_census, ms[1] mvs_sweep, every launch of the call) and of its last
 * slam_mvs_fuse_dev (ms[2] mvs_filter + mvs_count, ms[3] mvs_emit; 0 when nothing
 * survived); 0 before the first call. */
int slam_mvs_last_timing(slam_ctx* ctx, double* ms);
/* The host twin of slam_mvs_depth: no context, no device, the same arithmetic
 * (csrc/mvs_math.h) on up to 16 threads, the same results bit for bit. */
int slam_mvs_depth_host(const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h, size_t step, int channels,
                        const double* M, const double* v, const double* planes, int D, int radius, int uniq,
                        int min_views, int16_t* plane, int32_t* cost, float* inv_depth);

/* ---- semi-global aggregation of the plane-sweep cost volume (mvs_sgm.hip) ---------- */
/* An opt-in rule beside the winner-take-all of slam_mvs_depth_batch_dev (DESIGN.md
 * section 28).  The definition of every value is tests/mvs_sgm_ref.py; the device
 * and the host twins equal it bit for bit (integers only, so no schedule matters).
 * The reference has no such stage.
 *
 * Volume: C[d] and nvalid[d] exactly as slam_mvs_depth_batch_dev defines them, C <=
 * 64 (2 radius + 1)^2 S <= 12544 as uint16, nvalid as uint8, both h x w x D per
 * reference with the plane index innermost.
 * Paths: steps (dx, dy) in the order (1,0) (-1,0) (0,1) (0,-1) (1,1) (-1,-1) (1,-1)
 * (-1,1); paths = 4 takes the first four, 8 all.  For path r and q = p - r:
 * L_r(p, d) = C(p, d) when q is outside the image, else with m = min_k L_r(q, k)
 *   L_r(p, d) = C(p, d) + min(L_r(q, d), L_r(q, d - 1) + P1, L_r(q, d + 1) + P1, m + P2) - m,
 * the d - 1 and d + 1 terms absent at the two end planes.  C <= L_r <= C + P2 fits
 * uint16; S(p, d) = the sum of L_r over the paths <= 8 * 65535 fits int32.
 * Penalties: the caller's p1, p2 (0 <= p1 <= p2 <= 255) are per window pixel and
 * source in Hamming bits; a reference with S sources at radius r uses P1 = p1 (2 r +
 * 1)^2 S and P2 likewise, so one setting means the same at every radius and S.
 * Winner: the rule of slam_mvs_depth_batch_dev on S in place of C (best, second,
 * uniq, nvalid[best] >= min_views, the parabola): plane = best, cost = S[best],
 * inv_depth.  With p1 = p2 = 0 every L_r is C: plane and inv_depth equal the
 * winner-take-all result bit for bit and cost is paths times its cost.
 *
 * slam_mvs_cost_volume_dev: the volume alone of nref references (arguments as
 * slam_mvs_depth_batch_dev) into d_C and d_nvalid (device, nref x h x w x D).
 * Synchronous; the errors of slam_mvs_depth_batch_dev. */
int slam_mvs_cost_volume_dev(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                             int nref, const int32_t* ref_idx, const int32_t* nsrc, const int32_t* src_idx, const double* M,
                             const double* v, const double* planes, int D, int radius, uint16_t* d_C, uint8_t* d_nvalid);
/* S of n given volumes (d_C: n x h x w x D uint16, device, every value <= 12544)
 * with the effective penalties P1 <= P2 <= 65535 - 12544 into d_S (n x h x w x D
 * int32, device).  n 0..65535, D 4..256, paths 4 or 8, else SLAM_E_INVALID_ARG; w >
 * 4096: SLAM_E_UNSUPPORTED.  Synchronous. */
int slam_mvs_sgm_aggregate_dev(slam_ctx* ctx, void* stream, const uint16_t* d_C, int n, int w, int h, int D, int P1, int P2,
                               int paths, int32_t* d_S);
/* slam_mvs_depth_batch_dev with the aggregation between the volume and the winner.
 * The references are worked through in groups whose scratch (7 bytes per pixel and
 * plane: C, nvalid, S) stays under the context's budget (8 GiB unless
 * slam_mvs_sgm_set_budget says otherwise; a single reference that exceeds it still
 * runs alone); the results do not depend on the grouping.  p1 > p2, either outside
 * 0..255 or paths not 4 or 8: SLAM_E_INVALID_ARG, as is everything
 * slam_mvs_depth_batch_dev refuses; w > 4096: SLAM_E_UNSUPPORTED. */
int slam_mvs_depth_sgm_batch_dev(slam_ctx* ctx, void* stream, const uint8_t* d_frames, int nframes, int w, int h,
                                 int channels, int nref, const int32_t* ref_idx, const int32_t* nsrc,
                                 const int32_t* src_idx, const double* M, const double* v, const double* planes, int D,
                                 int radius, int uniq, int min_views, int p1, int p2, int paths, int16_t* d_plane,
                                 int32_t* d_cost, float* d_inv_depth);
/* slam_mvs_depth_sgm_batch_dev for one reference and its S sources in host memory,
 * as slam_mvs_depth is to slam_mvs_depth_batch_dev. */
int slam_mvs_depth_sgm(slam_ctx* ctx, const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h, size_t step,
                       int channels, const double* M, const double* v, const double* planes, int D, int radius, int uniq,
                       int min_views, int p1, int p2, int paths, int16_t* plane, int32_t* cost, float* inv_depth);
/* the scratch budget in bytes of the context's later slam_mvs_depth_sgm_batch_dev
 * calls; 0 = the default (8 GiB).  Never changes results. */
int slam_mvs_sgm_set_budget(slam_ctx* ctx, size_t bytes);
/* HIP-event times (ms) of the context's last slam_mvs_depth_sgm_batch_dev, summed
 * over its groups: ms[0] mvs_volume, ms[1] the clear of S + sgm_path, ms[2]
 * sgm_winner.  slam_mvs_cost_volume_dev sets ms[0], slam_mvs_sgm_aggregate_dev
 * ms[1] alone.  0 before the first call. */
int slam_mvs_sgm_last_timing(slam_ctx* ctx, double* ms);
/* The host twins: no context, no device, the same arithmetic (csrc/mvs_sgm_math.h)
 * on up to 16 threads, the same results bit for bit.  slam_mvs_cost_volume_host:
 * the volume of one reference (C, nvalid: h x w x D).  slam_mvs_sgm_aggregate_host:
 * slam_mvs_sgm_aggregate_dev on host memory.  slam_mvs_depth_sgm_host:
 * slam_mvs_depth_sgm. */
int slam_mvs_cost_volume_host(const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h, size_t step, int channels,
                              const double* M, const double* v, const double* planes, int D, int radius, uint16_t* C,
                              uint8_t* nvalid);
int slam_mvs_sgm_aggregate_host(const uint16_t* C, int n, int w, int h, int D, int P1, int P2, int paths, int32_t* S);
int slam_mvs_depth_sgm_host(const uint8_t* ref, const uint8_t* const* srcs, int S, int w, int h, size_t step, int channels,
                            const double* M, const double* v, const double* planes, int D, int radius, int uniq,
                            int min_views, int p1, int p2, int paths, int16_t* plane, int32_t* cost, float* inv_depth);

/* ---- surface from the depth maps: TSDF fusion and marching cubes (tsdf.hip) -------- */
/* An opt-in stage after the depth maps.  The definition of
 * every value is tests/tsdf_ref.py; the device and the host twins equal it bit for
 * bit.  The reference has no such stage.
 *
 * The volume: a grid of nx x ny x nz nodes, each dimension in 2..2048 and nx ny nz
 * <= 2^30 (else SLAM_E_UNSUPPORTED); node (i, j, k) sits at X = origin[0] +
 * (double)i voxel, Y and Z likewise.  Its state is six int32 planes [6][nz][ny][nx]
 * (x fastest) D, W, CW, B, G, R owned by the caller; all zeros is the empty volume.
 * Every sum is an integer, so the volume after a set of maps does not depend on
 * their order or on how they are split over calls.  A volume takes at most 2^20
 * maps in total (the caller counts); a call takes at most 2^20.
 *
 * slam_tsdf_integrate_dev adds nmaps depth maps (d_inv_depth: nmaps x h x w f32,
 * device; map m belongs to frame frame_idx[m] of the nframes resident frames, m
 * itself when frame_idx is NULL) with the projections P (host, nmaps x 12, row-
 * major 3 x 4, mathematically K [R | t]; the library never forms one).  Per node
 * and map, in f64 in this order without contraction:
 *   h_i = ((P[i][0] X + P[i][1] Y) + P[i][2] Z) + P[i][3],  u = h_0 / h_2,  v = h_1 / h_2,
 * valid iff h_2 > 0, -0.5 <= u < W - 0.5 and -0.5 <= v < H - 0.5 (a NaN or an
 * infinity is invalid), then ix = (int)floor(u + 0.5), iy likewise; w =
 * inv_depth[iy][ix], skipped unless w > 0; r = (1.0 / (double)w - h_2) / trunc,
 * skipped when r < -1.0 (hidden behind the surface), r = 1.0 when r > 1.0; D +=
 * (int32)floor(r * 1024.0 + 0.5), W += 1; iff r < 1.0 also CW += 1 and B, G, R += the
 * frame's bytes at (ix, iy) (gray three times for one channel).  Synchronous; one
 * launch reads and writes the volume once whatever nmaps is.  A non-finite P,
 * origin, voxel or trunc, voxel <= 0, trunc <= 0, a frame index outside the batch,
 * channels other than 1 or 3, nmaps outside 0..2^20: SLAM_E_INVALID_ARG.  Huge
 * finite entries are legal and come out invalid.  nmaps == 0: SLAM_OK, no launch. */
int slam_tsdf_integrate_dev(slam_ctx* ctx, void* stream, int32_t* d_volume, int nx, int ny, int nz, const double* origin,
                            double voxel, double trunc, const uint8_t* d_frames, int nframes, int w, int h, int channels,
                            const int32_t* frame_idx, const float* d_inv_depth, const double* P, int nmaps);
/* Marching cubes on the node lattice.  A node is known iff W >= min_weight (>= 1),
 * inside iff known and D < 0; cell (i, j, k) is active iff its eight corners are
 * known.  Corner c = dx | dy << 1 | dz << 2; the edge along `axis` is owned by its
 * lower corner and has id axis * 4 + the owner's rank among the four corners with
 * bit axis clear; the triangles of the 256 sign cases are csrc/tsdf_table.h,
 * generated by the rule in tests/tsdf_ref.py.  Node (i, j, k) owns its +x, +y, +z
 * edges; an edge carries a vertex iff its far node is in the grid, both ends are
 * known, exactly one is inside and one of the up to four cells around it is
 * active.  With a the owner, fa = (double)Da / (double)Wa, fb likewise, t = fa / (fa -
 * fb): the vertex sits at origin[axis] + ((double)i_axis + t) voxel along the axis
 * and at the node's coordinates otherwise; per channel a node's colour is ca = CW ?
 * (2 sum + CW) / (2 CW) : 0 in integers and the vertex's is (uint8)floor(((double)ca
 * + t ((double)cb - (double)ca)) + 0.5).  Vertices are numbered by owner node in
 * raster order (z outer, x inner), +x, +y, +z within a node; faces come cell by cell
 * in raster order, in the table's order within a cell; zero-area triangles are
 * kept.  Outputs (device): d_vertices cap_vertices x 3 f64, d_colors cap_vertices x
 * 3 u8 (blue, green, red), d_faces cap_faces x 3 int32.  *nv / *nf = the counts;
 * when either exceeds its capacity: SLAM_E_CAPACITY with both needed counts and
 * nothing written.  More than 2^31 - 1 of either: SLAM_E_UNSUPPORTED.  Synchronous. */
int slam_tsdf_mesh_dev(slam_ctx* ctx, void* stream, const int32_t* d_volume, int nx, int ny, int nz, const double* origin,
                       double voxel, int min_weight, double* d_vertices, uint8_t* d_colors, int32_t* d_faces,
                       int cap_vertices, int cap_faces, int* nv, int* nf);
/* slam_tsdf_integrate_dev for a volume, packed frames (nframes x h x w x channels)
 * and maps in host memory; the volume is updated in place. */
int slam_tsdf_integrate(slam_ctx* ctx, int32_t* volume, int nx, int ny, int nz, const double* origin, double voxel,
                        double trunc, const uint8_t* frames, int nframes, int w, int h, int channels,
                        const int32_t* frame_idx, const float* inv_depth, const double* P, int nmaps);
/* slam_tsdf_mesh_dev for a volume and outputs in host memory. */
int slam_tsdf_mesh(slam_ctx* ctx, const int32_t* volume, int nx, int ny, int nz, const double* origin, double voxel,
                   int min_weight, double* vertices, uint8_t* colors, int32_t* faces, int cap_vertices, int cap_faces,
                   int* nv, int* nf);
/* The host twins: no context, no device, the same arithmetic (csrc/tsdf_math.h, csrc/
 * tsdf_table.h) on up to 16 threads, the same results and error codes bit for bit. */
int slam_tsdf_integrate_host(int32_t* volume, int nx, int ny, int nz, const double* origin, double voxel, double trunc,
                             const uint8_t* frames, int nframes, int w, int h, int channels, const int32_t* frame_idx,
                             const float* inv_depth, const double* P, int nmaps);
int slam_tsdf_mesh_host(const int32_t* volume, int nx, int ny, int nz, const double* origin, double voxel, int min_weight,
                        double* vertices, uint8_t* colors, int32_t* faces, int cap_vertices, int cap_faces, int* nv,
                        int* nf);
/* Library HIP-event times (ms) of the context's last slam_tsdf_integrate_dev (ms[0]
 * tsdf_integrate) and of its last slam_tsdf_mesh_dev (ms[1] tsdf_classify +
 * tsdf_count, ms[2] tsdf_scan, ms[3] tsdf_emit_vertices + tsdf_emit_faces; 0 when
 * nothing was emitted); 0 before the first call. */
int slam_tsdf_last_timing(slam_ctx* ctx, double* ms);

/* ---- texture of the fused surface: a per-face atlas from the keyframes (tex.hip) ---- */
/* An opt-in stage after the surface.  The definition of every
 * value is tests/tex_ref.py; the device and the host twins equal it bit for bit.  The
 * reference has no such stage.  The mesh is slam_tsdf_mesh's: V nv x 3 f64, C nv x 3 u8
 * (blue, green, red), F nf x 3 int32.  A view is a frame and its projection P (3 x 4
 * row-major f64, mathematically K [R | t], pixel centres at integer coordinates).
 *
 * slam_tex_select_dev: d_ids are nv id images (nv x h x w int32, device) as
 * slam_render_views_dev writes them for the mesh seen from nv views.  count[m][f] = the
 * pixels of image m whose kind is 2 (face) and whose index is f < nf; everything else
 * (the background -1, points, lines, indices >= nf) is ignored.  The caller owns the
 * state d_best_count / d_best_view (nf int32 each, device), initially 0 / -1; the
 * views are folded in with their global index view0 + m: a view with count c replaces
 * the state iff c > best_count or (c == best_count and c > 0 and its index < best_view).
 * All of it is integer, so the state after a set of views does not depend on how they
 * are split over calls nor on the calls' order.  nf > 2^30: SLAM_E_UNSUPPORTED; nv, nf
 * or view0 < 0, view0 + nv > 2^31 - 1, h or w < 1, h w > 2^30, a null pointer with a
 * non-zero count: SLAM_E_INVALID_ARG.  nv == 0 or nf == 0: SLAM_OK, no launch.
 * Synchronous. */
int slam_tex_select_dev(slam_ctx* ctx, void* stream, const int32_t* d_ids, int nv, int h, int w, int view0, int nf,
                        int32_t* d_best_count, int32_t* d_best_view);
/* The atlas layout, a pure function of (nf, T, page); host only.  T (1..64) is the
 * texels per triangle leg, S = T + 4 the cell size, cells_x = page / S with page in
 * S..8192.  Face f lives in cell f >> 1, half f & 1; cells are in raster order,
 * cells_x per row and cells_x rows per page.  Every page is *page_w = cells_x S texels
 * wide; page p is S x (the cell rows it uses) high.  In cell-local texel coordinates
 * (texel (i, j) has its centre at (i + 0.5, j + 0.5)) half 0 maps the corners a, b, c to
 * (1, 1), (1 + T, 1), (1, 1 + T), half 1 to (T + 3, T + 3), (3, T + 3), (T + 3, 3);
 * texel (i, j) belongs to half 0 iff i + j <= T + 2.  Outputs, each nullable: page_h
 * (cap_pages int32; *npages > cap_pages: SLAM_E_CAPACITY, *npages and *page_w are set),
 * uv (nf x 3 x 2 f64: (x / page_w, 1 - y / page_h) of a corner at page texel (x, y)),
 * face_page (nf int32).  nf == 0: zero pages.  T or page out of range, nf < 0:
 * SLAM_E_INVALID_ARG; nf > 2^30: SLAM_E_UNSUPPORTED. */
int slam_tex_layout(int nf, int T, int page, int* npages, int* page_w, int32_t* page_h, int cap_pages, double* uv,
                    int32_t* face_page);
/* Fills the atlas: d_atlas holds the pages one after the other, each page_h x page_w x 3
 * u8 (blue, green, red), exactly the sum of slam_tex_layout's page sizes.  frames: n
 * resident frames of h x w x channels (1 or 3) bytes; view m is frame frame_idx[m] (host;
 * NULL: m itself) with the projection P[m] (host, nviews x 12).  Per texel: (0, 0, 0)
 * when its owner half's face is >= nf.  Otherwise, with (x', y') its centre in the cell,
 * half 0: beta = (x' - 1) / T, gamma = (y' - 1) / T; half 1: beta = (T + 3 - x') / T,
 * gamma = (T + 3 - y') / T; alpha = (1 - beta) - gamma; X = (alpha Va + beta Vb) + gamma
 * Vc per component (f64, this order, no contraction).  If best_count[f] >= min_pixels
 * and best_view[f] >= 0: h_i = ((P[i][0] X + P[i][1] Y) + P[i][2] Z) + P[i][3] of the
 * best view; h_2 > 0 and u = h_0 / h_2, v = h_1 / h_2 finite are required; u is clamped
 * to [0, w - 1], v to [0, h - 1]; x0 = floor(u), x1 = min(x0 + 1, w - 1), wx =
 * (int)floor((u - x0) 256 + 0.5), y alike; per channel top = p00 (256 - wx) + p01 wx, bot
 * alike, value = (top (256 - wy) + bot wy + 32768) >> 16; a gray frame fills the three
 * channels alike.  Any failed test takes the Gouraud fallback per channel:
 * (uint8)clamp(floor(((alpha ca + beta cb) + gamma cc) + 0.5), 0, 255) of the vertex
 * colours.  A NaN or an infinity in P, V or the projection fails a test and never
 * reaches an integer conversion.  SLAM_E_INVALID_ARG: T outside 1..64, page outside
 * T + 4..8192, min_pixels outside 1..2^30, a face index outside nv, a best view outside
 * -1..nviews - 1, a frame index outside n, channels other than 1 or 3, nviews outside
 * 0..2^20, a null pointer with a non-zero count; nf > 2^30 (or more than 2^39 texels):
 * SLAM_E_UNSUPPORTED; nothing is filled then.  nf == 0: SLAM_OK, nothing written.
 * Synchronous. */
int slam_tex_fill_dev(slam_ctx* ctx, void* stream, const double* d_V, const uint8_t* d_C, const int32_t* d_F, int nv, int nf,
                      const uint8_t* d_frames, int n, int h, int w, int channels, const int32_t* frame_idx, const double* P,
                      int nviews, const int32_t* d_best_count, const int32_t* d_best_view, int min_pixels, int T, int page,
                      uint8_t* d_atlas);
/* slam_tex_select_dev / slam_tex_fill_dev for ids, state, mesh, frames and atlas in host
 * memory; the state is updated in place. */
int slam_tex_select(slam_ctx* ctx, const int32_t* ids, int nv, int h, int w, int view0, int nf, int32_t* best_count,
                    int32_t* best_view);
int slam_tex_fill(slam_ctx* ctx, const double* V, const uint8_t* C, const int32_t* F, int nv, int nf, const uint8_t* frames,
                  int n, int h, int w, int channels, const int32_t* frame_idx, const double* P, int nviews,
                  const int32_t* best_count, const int32_t* best_view, int min_pixels, int T, int page, uint8_t* atlas);
/* The host twins: no context, no device, the same arithmetic (csrc/tex_math.h) on up to
 * 16 threads, the same results and error codes bit for bit. */
int slam_tex_select_host(const int32_t* ids, int nv, int h, int w, int view0, int nf, int32_t* best_count, int32_t* best_view);
int slam_tex_fill_host(const double* V, const uint8_t* C, const int32_t* F, int nv, int nf, const uint8_t* frames, int n, int h,
                       int w, int channels, const int32_t* frame_idx, const double* P, int nviews, const int32_t* best_count,
                       const int32_t* best_view, int min_pixels, int T, int page, uint8_t* atlas);
/* Library HIP-event times (ms) of the context's last slam_tex_select_dev (ms[0]:
 * tex_count + tex_best over all its chunks) and of its last slam_tex_fill_dev (ms[1]:
 * tex_fill); 0 before the first call and when nothing was launched. */
int slam_tex_last_timing(slam_ctx* ctx, double* ms);

/* ---- place recognition: a flat visual vocabulary and bag-of-words retrieval (place.hip) ----
 * All arithmetic is integer except the one IEEE division of a score, so device,
 * host twin and the numpy contract (tests/place_ref.py) agree bit for bit.
 * kind: SLAM_VOC_SIFT rows of 128 u8 compared by squared L2 (the whole u8 range is
 * legal, d^2 up to 128 * 255^2), SLAM_VOC_ORB rows of 32 bytes compared by Hamming
 * distance.  Limits: 1 <= K <= 65536 words, at most 2^24 descriptors per call, at
 * most 65535 descriptors per image, idf weights in [0, 1023], k <= 32.  A bad size,
 * an unknown kind, a weight out of range or too many descriptors in an image is
 * SLAM_E_INVALID_ARG; none of them reads or writes out of bounds.  Device pointers
 * of descriptors and centroids are 16-byte aligned.  Every call is synchronous. */
enum { SLAM_VOC_SIFT = 0, SLAM_VOC_ORB = 1 };
/* word[i] = the centroid (row of d_cent, K x B bytes) with the least distance to
 * descriptor i (d_desc, n x B bytes), ties to the lowest centroid index; dist[i] =
 * that distance.  n = 0 is legal and writes nothing. */
int slam_voc_assign_dev(slam_ctx* ctx, void* stream, const uint8_t* d_desc, int n, const uint8_t* d_cent, int K,
                        int kind, int32_t* d_word, int32_t* d_dist);
/* Lloyd's algorithm in integers: d_cent[c] = d_desc[floor(c n / K)], then at most
 * `iters` times: assign, then for every non-empty cluster of count n_c the new
 * centroid is floor((2 S + n_c) / (2 n_c)) per dimension (SIFT, S the integer sum)
 * or bit = (2 ones > n_c) (ORB); an empty cluster keeps its centroid.  Stops after
 * an iteration that changes no centroid; *iters_run (host) = iterations performed.
 * 1 <= n; iters >= 0.  Only the changed flag is read back per iteration. */
int slam_voc_train_dev(slam_ctx* ctx, void* stream, const uint8_t* d_desc, int n, int K, int iters, int kind,
                       uint8_t* d_cent, int32_t* iters_run);
/* tf-idf vectors of m images: image r owns the words d_word[offsets[r] ..
 * offsets[r + 1]) (offsets: host, m + 1 ascending values); h_k counts its words,
 * d_vec[r K + k] = h_k weights[k] (u32) and d_total[r] = sum_k of them (u64).
 * weights: host, K values.  An image without descriptors gives the zero vector;
 * a word outside [0, K) in device memory is ignored. */
int slam_bow_vectors_dev(slam_ctx* ctx, void* stream, const int32_t* d_word, const int32_t* offsets, int m,
                         const int32_t* weights, int K, uint32_t* d_vec, uint64_t* d_total);
/* d_scores[i m + r] = score of query i (d_q: nq x K, d_qtotal) against database
 * row r (d_db: m x K, d_dbtotal): num = sum_k min(a_k B, b_k A) in int64 (exact:
 * at most A B <= 2^52), score = (double)num / ((double)A (double)B), 0.0 when A or
 * B is 0 -- the histogram intersection of the L1-normalised vectors. */
int slam_bow_score_dev(slam_ctx* ctx, void* stream, const uint32_t* d_q, const uint64_t* d_qtotal, int nq,
                       const uint32_t* d_db, const uint64_t* d_dbtotal, int m, int K, double* d_scores);
/* For each of nq rows of d_scores (m values each): the k best columns of [first,
 * last) by (score descending, index ascending) into d_idx / d_score (nq x k),
 * padded with index -1 and score 0.0.  0 <= first <= last <= m, 1 <= k <= 32. */
int slam_bow_topk_dev(slam_ctx* ctx, void* stream, const double* d_scores, int nq, int m, int first, int last, int k,
                      int32_t* d_idx, double* d_score);
/* The same calls on host buffers (staged through the context's workspace);
 * slam_bow_vectors also refuses a word outside [0, K); slam_bow_query is the score
 * followed by the top-k. */
int slam_voc_assign(slam_ctx* ctx, const uint8_t* desc, int n, const uint8_t* cent, int K, int kind, int32_t* word,
                    int32_t* dist);
int slam_voc_train(slam_ctx* ctx, const uint8_t* desc, int n, int K, int iters, int kind, uint8_t* cent,
                   int32_t* iters_run);
int slam_bow_vectors(slam_ctx* ctx, const int32_t* word, const int32_t* offsets, int m, const int32_t* weights, int K,
                     uint32_t* vec, uint64_t* total);
int slam_bow_query(slam_ctx* ctx, const uint32_t* q, const uint64_t* qtotal, int nq, const uint32_t* db,
                   const uint64_t* dbtotal, int m, int K, int first, int last, int k, int32_t* idx, double* score);
/* The host twins: no context, no device, the same arithmetic (csrc/place_math.h)
 * on up to 16 threads, the same results bit for bit. */
int slam_voc_assign_host(const uint8_t* desc, int n, const uint8_t* cent, int K, int kind, int32_t* word,
                         int32_t* dist);
int slam_voc_train_host(const uint8_t* desc, int n, int K, int iters, int kind, uint8_t* cent, int32_t* iters_run);
int slam_bow_vectors_host(const int32_t* word, const int32_t* offsets, int m, const int32_t* weights, int K,
                          uint32_t* vec, uint64_t* total);
int slam_bow_score_host(const uint32_t* q, const uint64_t* qtotal, int nq, const uint32_t* db, const uint64_t* dbtotal,
                        int m, int K, double* scores);

/* ---- loop closing: the Sim(3) constraint of a loop and the map correction (loop.hip) ----
 * Only + - * / and sqrt in f64, nothing contracted, every sum in the order that
 * tests/loop_ref.py states, so device, host twin and reference agree bit for bit.
 * A similarity is 8 doubles S = (sigma, qw, qx, qy, qz, tx, ty, tz) with a unit
 * quaternion: x' = sigma R(q) x + t.  Every call is synchronous. */
enum { SLAM_SIM3_OK = 0, SLAM_SIM3_NO_MODEL = 1, SLAM_SIM3_TOO_FEW = 2, SLAM_SIM3_CHOLESKY = 3 };
/* The similarity between the two copies of the map at each of L loops, by RANSAC.
 * Loop l owns the pairs [offsets[l], offsets[l + 1]) of d_a / d_b (n x 3 f64, device;
 * offsets: host, L + 1 ascending values from >= 0) that should satisfy b = s R a + t;
 * centres (host, L x 6) holds the camera centre that saw a, then the one that saw b.
 * H hypotheses per loop (1..65536) come from three distinct pairs each, drawn on the
 * host by the counter-based generator of loop_ref.py from `seed`; a hypothesis whose
 * triangle is degenerate scores 0.  A pair is an inlier of (s, R, t) iff e^2 = |b - (s R
 * a + t)|^2 <= tau^2 |b - c_b|^2 and e^2 <= tau^2 s^2 |a - c_a|^2 (an angle of about tau
 * seen from either camera).  The most inliers win, ties to the lowest hypothesis; the
 * winner is refined on its inliers by 4 Gauss-Newton steps (7 x 7 normal equations
 * summed in the stated order, solved by Cholesky).  Outputs per loop: d_sim (8 f64),
 * d_mask (one byte per pair, at the pair's index), d_count (the winner's inliers),
 * d_status: SLAM_SIM3_OK; SLAM_SIM3_TOO_FEW (fewer than 3 pairs) and
 * SLAM_SIM3_NO_MODEL (no hypothesis with 3 inliers) give the identity, a zero mask and
 * count 0; SLAM_SIM3_CHOLESKY keeps the similarity reached before the failed step. */
int slam_sim3_ransac_dev(slam_ctx* ctx, void* stream, const double* d_a, const double* d_b, const int32_t* offsets,
                         int L, const double* centres, int H, double tau, uint64_t seed, double* d_sim,
                         uint8_t* d_mask, int32_t* d_count, int32_t* d_status);
/* The same on host buffers (staged through the context's workspace). */
int slam_sim3_ransac(slam_ctx* ctx, const double* a, const double* b, const int32_t* offsets, int L,
                     const double* centres, int H, double tau, uint64_t seed, double* sim, uint8_t* mask,
                     int32_t* count, int32_t* status);
/* Moves n map points (n x 3 f64, device) after their anchor nodes changed from
 * nodes[anchor] to nodes_new[anchor] (host, m x 8 each): X' = S'^-1 (S (X)).  anchor
 * (device, int32) -1, or outside [0, m), keeps the point; a node whose 8 values did not
 * change returns its points' bits.  A node with sigma <= 0 or a zero quaternion is
 * SLAM_E_INVALID_ARG. */
int slam_sim3_apply_points_dev(slam_ctx* ctx, void* stream, const double* d_points, const int32_t* d_anchor, int n,
                               const double* nodes, const double* nodes_new, int m, double* d_out);
/* The same on host buffers; an anchor outside [-1, m) is SLAM_E_INVALID_ARG. */
int slam_sim3_apply_points(slam_ctx* ctx, const double* points, const int32_t* anchor, int n, const double* nodes,
                           const double* nodes_new, int m, double* out);
/* Pose-graph optimisation over Sim(3).  d_nodes (device, n x 8, in and out): the
 * keyframes' similarities, node 0 stays fixed.  Edge e joins nodes edges[2 e] = i and
 * edges[2 e + 1] = j (host) with the measurement meas[e] (host, 8 f64, Z ~ S_i o
 * S_j^-1) and weight[e] >= 0; its residual is sqrt(w) (sigma_E - 1, 2 sign(qw) vec(q_E),
 * t_E / ell) of E = Z^-1 o S_i o S_j^-1, with analytic Jacobians in the local steps
 * sigma (1 + ds), q (x) (1, dr / 2), t + dt.  Levenberg-Marquardt: lambda starts at
 * lambda0 and multiplies the diagonal; a step that lowers the cost is accepted and
 * lambda /= 10, otherwise the nodes are restored and lambda *= 10; it ends after max_lm
 * steps, at cost 0, or after an accepted step with (cost - new) / cost < cost_tol.  Each
 * step is solved by conjugate gradients on the normal equations, preconditioned by the
 * Cholesky factors of the damped 7 x 7 diagonal blocks, until r.z <= pcg_tol (r.z)_0 or
 * max_pcg iterations; the loop stays on the stream and the host reads its stop flag
 * every 8 iterations.  Sums run in the orders of tests/loop_ref.py.  cost (host, 2):
 * initial and final sum of squares; iters (host, 3): LM steps, accepted steps, PCG
 * iterations in total.  SLAM_E_INVALID_ARG: an edge with i == j or an index outside
 * [0, n), a node or measurement with sigma <= 0 or a zero quaternion, ell <= 0, a
 * negative weight, cap or tolerance, a node that no edge reaches. */
int slam_pgo_sim3_dev(slam_ctx* ctx, void* stream, double* d_nodes, int n, const int32_t* edges, const double* meas,
                      const double* weight, int E, double ell, double lambda0, int max_lm, int max_pcg, double pcg_tol,
                      double cost_tol, double* cost, int32_t* iters);
/* The same with the nodes in host memory. */
int slam_pgo_sim3(slam_ctx* ctx, double* nodes, int n, const int32_t* edges, const double* meas, const double* weight,
                  int E, double ell, double lambda0, int max_lm, int max_pcg, double pcg_tol, double cost_tol,
                  double* cost, int32_t* iters);
/* The host twins: no context, no device, the same arithmetic (csrc/loop_math.h), the
 * same results bit for bit. */
int slam_pgo_sim3_host(double* nodes, int n, const int32_t* edges, const double* meas, const double* weight, int E,
                       double ell, double lambda0, int max_lm, int max_pcg, double pcg_tol, double cost_tol, double* cost,
                       int32_t* iters);
int slam_sim3_ransac_host(const double* a, const double* b, const int32_t* offsets, int L, const double* centres,
                          int H, double tau, uint64_t seed, double* sim, uint8_t* mask, int32_t* count,
                          int32_t* status);
int slam_sim3_apply_points_host(const double* points, const int32_t* anchor, int n, const double* nodes,
                                const double* nodes_new, int m, double* out);

/* ---- global bundle adjustment after loop closing (csrc/gba.hip; the contract is tests/gba_ref.py) ----
 * Minimises the reprojection error over all n cameras and m points with the intrinsics
 * K4 = {fx, fy, cx, cy} (host) held constant.  A camera is 7 f64 (qw, qx, qy, qz, tx,
 * ty, tz), X_c = R(q) X + t with q a unit quaternion; camera 0 is fixed.  Observation o
 * is (obs_cam[o], obs_point[o], obs_xy[2 o], obs_xy[2 o + 1]), host arrays; its residual
 * is pi(X_c) - xy.  Excluded at entry and for the whole solve: an observation with
 * z_c <= zmin, then every observation of a point left with fewer than two; such a point
 * keeps its bits, and a camera left with no observation is held like camera 0.  A trial
 * step that brings a kept observation to z_c <= zmin is rejected.  Loss 0: squares;
 * loss 1: Huber with parameter loss_param on s = |r|^2 (rho = s for s <= a^2, else
 * 2 a sqrt(s) - a^2), entering as plain reweighting: r and J times sqrt(rho').
 * Levenberg-Marquardt with slam_pgo_sim3's rule; each step solves the Schur complement
 * onto the cameras by conjugate gradients without forming it (two passes over the
 * observations per iteration), preconditioned by its 6 x 6 diagonal blocks, until
 * r.z <= pcg_tol (r.z)_0 or max_pcg iterations; a point whose damped 3 x 3 block has no
 * Cholesky factor is frozen for that step.  Sums run in the orders of tests/gba_ref.py.
 * n <= 1 or no kept observation: SLAM_OK, nothing changes, both costs 0.
 * SLAM_E_INVALID_ARG: an index out of range, a zero quaternion, fx or fy <= 0,
 * zmin <= 0, a negative cap, tolerance or lambda0, an unknown loss, Huber with
 * loss_param <= 0, a pixel that is not finite. */
enum { SLAM_GBA_LOSS_SQUARE = 0, SLAM_GBA_LOSS_HUBER = 1 };
typedef struct slam_gba_params {
    int32_t loss;
    double loss_param, zmin, lambda0;
    int32_t max_lm, max_pcg;
    double pcg_tol, cost_tol;
} slam_gba_params;
typedef struct slam_gba_summary {
    double cost0, cost;          /* sum of rho over the kept observations, before and after */
    int32_t lm_steps, accepted, pcg_iters;
    int32_t kept_obs, behind_obs, points_held, cams_held;
} slam_gba_summary;
/* d_cams (n x 7) and d_points (m x 3) are device pointers, updated in place. */
int slam_gba_dev(slam_ctx* ctx, void* stream, const double* K4, double* d_cams, int n, double* d_points, int m,
                 const int32_t* obs_cam, const int32_t* obs_point, const double* obs_xy, int nobs,
                 const slam_gba_params* prm, slam_gba_summary* out);
/* The same with cameras and points in host memory. */
int slam_gba(slam_ctx* ctx, const double* K4, double* cams, int n, double* points, int m, const int32_t* obs_cam,
             const int32_t* obs_point, const double* obs_xy, int nobs, const slam_gba_params* prm,
             slam_gba_summary* out);
/* The host twin: no context, no device, the same arithmetic (csrc/gba_math.h), the same bits. */
int slam_gba_host(const double* K4, double* cams, int n, double* points, int m, const int32_t* obs_cam,
                  const int32_t* obs_point, const double* obs_xy, int nobs, const slam_gba_params* prm,
                  slam_gba_summary* out);

#ifdef __cplusplus
}
#endif
#endif

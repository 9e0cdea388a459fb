// Global bundle adjustment after loop closing for gfx950: Levenberg-Marquardt over every camera and every
// point, each step solved on the Schur complement onto the cameras by conjugate gradients without forming it.
// The contract (problem, exclusion rule, summation orders) is tests/gba_ref.py; the arithmetic is gba_math.h's,
// shared with the host twin (gba_host.cpp), so device, twin and reference agree bit for bit.  No atomics.
//
//   gba_linearize     one thread per kept observation (camera order): r, rho, J_c, J_p, component-major
//   gba_cam_cost      one wave per camera: its cost through the 64-lane tree
//   gba_point_blocks  one thread per point, serially down its list: C^-1 and g_p
//   gba_cam_blocks    one wave per camera: the 54 sums through the 64-lane tree, then lane 0 factors the Schur
//                     diagonal block and writes lambda diag(B), the factor and the reduced right-hand side
//   gba_pt_gather     one thread per point: w_p = C^-1 sum J_p^T (J_c p_k); with mode 1 the back-substitution
//   gba_cam_apply     one wave per camera: p_k is loaded once, the camera's observations stream once
//   pgo_reduce / gba_update / pgo_pupdate   the scalars, x r z and the search direction (pcg_kernels.h)
//   gba_step_cams / gba_step_points         the trial state
// The PCG loop stays on the stream; the host reads the stop flag every kPgoChunk iterations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "gba_math.h"
#include "gba_plan.h"
#include "pcg_kernels.h"
#include "slamhip_internal.h"

namespace slamhip {

namespace {

struct GbaConst {
    double K4[4], a, zmin;
    int loss;
};

// lane l < off takes lane l + off's value, for off = 32 .. 1: lane 0 ends with the tree's sum
template <int S> __device__ inline void wave_fold(double* acc)
{
    for (int off = kGbaLanes / 2; off >= 1; off >>= 1)
        for (int j = 0; j < S; j++) acc[j] = acc[j] + __shfl_down(acc[j], off, kGbaLanes);
}

__global__ __launch_bounds__(256) void gba_linearize(const double* cams, const double* pts, GbaConst k, const int32_t* obs_cam,
                                                     const int32_t* obs_pt, const double* xy, const uint8_t* held, int nk,
                                                     double* lin)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= nk) return;
    const int cam = obs_cam[o];
    double cm[7], X[3], out[kGbaLin];
    for (int i = 0; i < 7; i++) cm[i] = cams[7 * (size_t)cam + i];
    for (int i = 0; i < 3; i++) X[i] = pts[3 * (size_t)obs_pt[o] + i];
    gba_obs_lin(cm, X, k.K4, xy[2 * (size_t)o], xy[2 * (size_t)o + 1], k.loss, k.a, k.zmin, held[cam] != 0, out);
    for (int c = 0; c < kGbaLin; c++) lin[(size_t)c * nk + o] = out[c];
}

__global__ __launch_bounds__(kGbaLanes) void gba_cam_cost(const double* lin, int nk, const int32_t* cam_off, double* ccost)
{
    const int k = blockIdx.x;
    double acc = 0.0;
    for (int o = cam_off[k] + (int)threadIdx.x; o < cam_off[k + 1]; o += kGbaLanes) acc = acc + lin[(size_t)kGbaRho * nk + o];
    wave_fold<1>(&acc);
    if (threadIdx.x == 0) ccost[k] = acc;
}

__global__ __launch_bounds__(256) void gba_point_blocks(const double* lin, int nk, const int32_t* pt_off, const int32_t* pt_obs, int m,
                                                        double lambda, double* Ci, double* gp)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    double ci[9], g[3];
    gba_point_block(lin, (size_t)nk, pt_obs + pt_off[q], pt_off[q + 1] - pt_off[q], lambda, ci, g);
    for (int c = 0; c < 9; c++) Ci[(size_t)c * m + q] = ci[c];
    for (int c = 0; c < 3; c++) gp[(size_t)c * m + q] = g[c];
}

__global__ __launch_bounds__(kGbaLanes) void gba_cam_blocks(const double* lin, int nk, const int32_t* cam_off, const int32_t* obs_pt,
                                                            const double* Ci, const double* gp, int m, double lambda, double* dl,
                                                            double* Lm, double* b)
{
    const int k = blockIdx.x;
    double acc[kGbaCamSums];
    for (int j = 0; j < kGbaCamSums; j++) acc[j] = 0.0;
    for (int o = cam_off[k] + (int)threadIdx.x; o < cam_off[k + 1]; o += kGbaLanes) {
        double v[kGbaLin], ci[9], g[3], t[kGbaCamSums];
        gba_load(lin, (size_t)nk, (size_t)o, 0, kGbaLin, v);
        const size_t q = (size_t)obs_pt[o];
        for (int c = 0; c < 9; c++) ci[c] = Ci[(size_t)c * m + q];
        for (int c = 0; c < 3; c++) g[c] = gp[(size_t)c * m + q];
        gba_cam_terms(v + kGbaJc, v + kGbaJp, v + kGbaR, ci, g, t);
        for (int j = 0; j < kGbaCamSums; j++) acc[j] = acc[j] + t[j];
    }
    wave_fold<kGbaCamSums>(acc);
    if (threadIdx.x != 0) return;
    double d[6], l[36], bb[6];
    gba_cam_finish(acc, lambda, d, l, bb);
    for (int i = 0; i < 6; i++) {
        dl[6 * (size_t)k + i] = d[i];
        b[6 * (size_t)k + i] = bb[i];
    }
    for (int i = 0; i < 36; i++) Lm[36 * (size_t)k + i] = l[i];
}

__global__ __launch_bounds__(64) void gba_pcg_init(const double* b, const double* Lm, int n, double* x, double* r, double* z, double* p)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    double rr[6], zz[6], l[36];
    for (int i = 0; i < 6; i++) rr[i] = b[6 * (size_t)k + i];
    for (int i = 0; i < 36; i++) l[i] = Lm[36 * (size_t)k + i];
    gba_chol_solve<6>(l, rr, zz);
    for (int i = 0; i < 6; i++) {
        x[6 * (size_t)k + i] = 0.0;
        r[6 * (size_t)k + i] = rr[i];
        z[6 * (size_t)k + i] = zz[i];
        p[6 * (size_t)k + i] = zz[i];
    }
}

__global__ __launch_bounds__(256) void gba_pt_gather(const double* lin, int nk, const int32_t* pt_off, const int32_t* pt_obs,
                                                     const int32_t* obs_cam, const double* vec, const double* Ci, const double* gp, int m,
                                                     int mode, double* w, const PgoSc* sc)
{
    if (mode == 0 && sc->done) return;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    double ci[9], g[3], out[3];
    for (int c = 0; c < 9; c++) ci[c] = Ci[(size_t)c * m + q];
    for (int c = 0; c < 3; c++) g[c] = gp[(size_t)c * m + q];
    gba_point_gather(lin, (size_t)nk, pt_obs + pt_off[q], pt_off[q + 1] - pt_off[q], obs_cam, vec, ci, g, mode, out);
    for (int c = 0; c < 3; c++) w[(size_t)c * m + q] = out[c];
}

__global__ __launch_bounds__(kGbaLanes) void gba_cam_apply(const double* lin, int nk, const int32_t* cam_off, const int32_t* obs_pt,
                                                           const double* w, int m, const double* dl, const double* p, double* Ap,
                                                           const PgoSc* sc)
{
    if (sc->done) return;
    const int k = blockIdx.x;
    double pk[6], acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 6; i++) pk[i] = p[6 * (size_t)k + i];
    for (int o = cam_off[k] + (int)threadIdx.x; o < cam_off[k + 1]; o += kGbaLanes) {
        double J[18], wp[3], t[6];
        gba_load(lin, (size_t)nk, (size_t)o, kGbaJc, 18, J);
        const size_t q = (size_t)obs_pt[o];
        for (int c = 0; c < 3; c++) wp[c] = w[(size_t)c * m + q];
        gba_apply_terms(J, J + 12, pk, wp, t);
        for (int i = 0; i < 6; i++) acc[i] = acc[i] + t[i];
    }
    wave_fold<6>(acc);
    if (threadIdx.x != 0) return;
    for (int i = 0; i < 6; i++) Ap[6 * (size_t)k + i] = dl[6 * (size_t)k + i] * pk[i] + acc[i];
}

__global__ __launch_bounds__(64) void gba_update(const double* Lm, int n, const double* p, const double* Ap, double* x, double* r,
                                                 double* z, const PgoSc* sc)
{
    if (sc->done) return;
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const double alpha = sc->alpha;
    double rr[6], zz[6], l[36];
    for (int i = 0; i < 6; i++) {
        const size_t at = 6 * (size_t)k + i;
        x[at] = x[at] + alpha * p[at];
        rr[i] = r[at] - alpha * Ap[at];
        r[at] = rr[i];
    }
    for (int i = 0; i < 36; i++) l[i] = Lm[36 * (size_t)k + i];
    gba_chol_solve<6>(l, rr, zz);
    for (int i = 0; i < 6; i++) z[6 * (size_t)k + i] = zz[i];
}

__global__ __launch_bounds__(256) void gba_step_cams(const double* cams, const double* x, const uint8_t* held, int n, double* out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    double cm[7], d[6];
    for (int i = 0; i < 7; i++) cm[i] = cams[7 * (size_t)k + i];
    for (int i = 0; i < 6; i++) d[i] = x[6 * (size_t)k + i];
    if (!held[k]) gba_cam_step(cm, d);
    for (int i = 0; i < 7; i++) out[7 * (size_t)k + i] = cm[i];
}

__global__ __launch_bounds__(256) void gba_step_points(const double* pts, const double* dX, const int32_t* pt_off, int m, double* out)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    const bool seen = pt_off[q + 1] != pt_off[q];
    for (int c = 0; c < 3; c++) {
        const double v = pts[3 * (size_t)q + c];
        out[3 * (size_t)q + c] = seen ? v + dX[(size_t)c * m + q] : v;
    }
}

}  // namespace

}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_gba_dev(slam_ctx* c, void* stream, const double* K4, double* d_cams, int n, double* d_points, int m,
                            const int32_t* obs_cam, const int32_t* obs_point, const double* obs_xy, int nobs,
                            const slam_gba_params* prm, slam_gba_summary* out)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!out || n < 0 || m < 0 || (n > 0 && !d_cams) || (m > 0 && !d_points)) return set_err(c, SLAM_E_INVALID_ARG, "gba: null argument");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    std::vector<double> h_cams(7 * (size_t)n), h_pts(3 * (size_t)m);
    if (n > 0) SLAM_HIP(c, hipMemcpyAsync(h_cams.data(), d_cams, 7 * 8 * (size_t)n, hipMemcpyDeviceToHost, s));
    if (m > 0) SLAM_HIP(c, hipMemcpyAsync(h_pts.data(), d_points, 3 * 8 * (size_t)m, hipMemcpyDeviceToHost, s));
    if (int rc = stream_sync(c, s)) return rc;
    if (gba_check(K4, h_cams.data(), n, h_pts.data(), m, obs_cam, obs_point, obs_xy, nobs, prm))
        return set_err(c, SLAM_E_INVALID_ARG, "gba: indices inside [0, n) and [0, m), non-zero quaternions, fx and fy > 0, zmin > 0, "
                                              "lambda0, caps and tolerances >= 0, loss 0 or 1 (Huber with a > 0), finite pixels");
    GbaPlan pl;
    gba_plan(h_cams.data(), n, h_pts.data(), m, obs_cam, obs_point, obs_xy, nobs, prm->zmin, pl);
    gba_summary_init(pl, out);
    if (n <= 1 || pl.nk == 0) return SLAM_OK;

    const size_t nn = (size_t)n, M = (size_t)m, nk = (size_t)pl.nk, N = 6 * nn;
    DevLayout lay;
    const auto s_cA = lay.add<double>(7 * nn), s_cB = lay.add<double>(7 * nn), s_xA = lay.add<double>(3 * M), s_xB = lay.add<double>(3 * M);
    const auto s_linA = lay.add<double>(kGbaLin * nk), s_linB = lay.add<double>(kGbaLin * nk), s_xy = lay.add<double>(2 * nk);
    const auto s_cc = lay.add<double>(nn), s_Ci = lay.add<double>(9 * M), s_gp = lay.add<double>(3 * M), s_w = lay.add<double>(3 * M);
    const auto s_dl = lay.add<double>(N), s_Lm = lay.add<double>(36 * nn), s_b = lay.add<double>(N);
    const auto s_x = lay.add<double>(N), s_r = lay.add<double>(N), s_z = lay.add<double>(N), s_p = lay.add<double>(N), s_Ap = lay.add<double>(N);
    const auto s_sc = lay.add<PgoSc>(1);
    const auto s_oc = lay.add<int32_t>(nk), s_op = lay.add<int32_t>(nk), s_po = lay.add<int32_t>(nk);
    const auto s_coff = lay.add<int32_t>(nn + 1), s_poff = lay.add<int32_t>(M + 1);
    const auto s_held = lay.add<uint8_t>(nn);
    DevMem w;
    SLAM_HIP(c, w.bind(c->gba_ws, lay));
    double *C = w.ptr(s_cA), *Ct = w.ptr(s_cB), *X = w.ptr(s_xA), *Xt = w.ptr(s_xB), *linA = w.ptr(s_linA), *linB = w.ptr(s_linB);
    double *xy = w.ptr(s_xy), *cc = w.ptr(s_cc), *Ci = w.ptr(s_Ci), *gp = w.ptr(s_gp), *wv = w.ptr(s_w);
    double *dl = w.ptr(s_dl), *Lm = w.ptr(s_Lm), *b = w.ptr(s_b), *x = w.ptr(s_x), *r = w.ptr(s_r), *z = w.ptr(s_z), *p = w.ptr(s_p);
    double* Ap = w.ptr(s_Ap);
    PgoSc* sc = w.ptr(s_sc);
    int32_t *oc = w.ptr(s_oc), *op = w.ptr(s_op), *po = w.ptr(s_po), *coff = w.ptr(s_coff), *poff = w.ptr(s_poff);
    uint8_t* held = w.ptr(s_held);
    PgoSc* h_sc = static_cast<PgoSc*>(readback(c, sizeof(PgoSc)));
    if (!h_sc) return set_err(c, SLAM_E_HIP, "gba: no pinned readback space");

    SLAM_HIP(c, hipMemcpyAsync(C, d_cams, 7 * 8 * nn, hipMemcpyDeviceToDevice, s));
    SLAM_HIP(c, hipMemcpyAsync(X, d_points, 3 * 8 * M, hipMemcpyDeviceToDevice, s));
    SLAM_HIP(c, w.upload(s_xy, pl.xy.data(), s));
    SLAM_HIP(c, w.upload(s_oc, pl.obs_cam.data(), s));
    SLAM_HIP(c, w.upload(s_op, pl.obs_pt.data(), s));
    SLAM_HIP(c, w.upload(s_po, pl.pt_obs.data(), s));
    SLAM_HIP(c, w.upload(s_coff, pl.cam_off.data(), s));
    SLAM_HIP(c, w.upload(s_poff, pl.pt_off.data(), s));
    SLAM_HIP(c, w.upload(s_held, pl.held.data(), s));
    PgoSc init = {};
    init.tol = prm->pcg_tol;
    SLAM_HIP(c, w.upload(s_sc, &init, s));
    if (int rc = stream_sync(c, s)) return rc;      // the plan's vectors and `init` are free from here

    GbaConst k = {};
    for (int i = 0; i < 4; i++) k.K4[i] = K4[i];
    k.a = prm->loss_param;
    k.zmin = prm->zmin;
    k.loss = prm->loss;
    const unsigned gO = (unsigned)((nk + 255) / 256), gM = (unsigned)((M + 255) / 256), gN = (unsigned)((nn + 63) / 64);
    const unsigned gN6 = (unsigned)((N + 255) / 256), gNc = (unsigned)((nn + 255) / 256);
    const int inK = pl.nk;
    auto linearize = [&](const double* cams, const double* pts, double* L, double* cost) -> int {
        hipLaunchKernelGGL(gba_linearize, dim3(gO), dim3(256), 0, s, cams, pts, k, oc, op, xy, held, inK, L);
        hipLaunchKernelGGL(gba_cam_cost, dim3(n), dim3(kGbaLanes), 0, s, L, inK, coff, cc);
        hipLaunchKernelGGL(pgo_reduce, dim3(1), dim3(kPgoLanes), 0, s, cc, (const double*)nullptr, nn, sc, 0);
        SLAM_HIP(c, hipGetLastError());
        SLAM_HIP(c, hipMemcpyAsync(h_sc, sc, sizeof(PgoSc), hipMemcpyDeviceToHost, s));
        if (int rc = stream_sync(c, s, true)) return rc;
        *cost = h_sc->cost;
        return SLAM_OK;
    };
    double c0 = 0.0;
    if (int rc = linearize(C, X, linA, &c0)) return rc;
    double cur = c0, lambda = prm->lambda0;
    int lm = 0, accepted = 0, pcg_total = 0;
    while (lm < prm->max_lm && cur > 0.0) {
        hipLaunchKernelGGL(gba_point_blocks, dim3(gM), dim3(256), 0, s, linA, inK, poff, po, m, lambda, Ci, gp);
        hipLaunchKernelGGL(gba_cam_blocks, dim3(n), dim3(kGbaLanes), 0, s, linA, inK, coff, op, Ci, gp, m, lambda, dl, Lm, b);
        hipLaunchKernelGGL(gba_pcg_init, dim3(gN), dim3(64), 0, s, b, Lm, n, x, r, z, p);
        hipLaunchKernelGGL(pgo_reduce, dim3(1), dim3(kPgoLanes), 0, s, r, z, N, sc, 1);
        SLAM_HIP(c, hipGetLastError());
        int launched = 0;
        for (;;) {
            const int chunk = std::min(kPgoChunk, prm->max_pcg - launched);
            for (int it = 0; it < chunk; it++) {
                hipLaunchKernelGGL(gba_pt_gather, dim3(gM), dim3(256), 0, s, linA, inK, poff, po, oc, p, Ci, gp, m, 0, wv, sc);
                hipLaunchKernelGGL(gba_cam_apply, dim3(n), dim3(kGbaLanes), 0, s, linA, inK, coff, op, wv, m, dl, p, Ap, sc);
                hipLaunchKernelGGL(pgo_reduce, dim3(1), dim3(kPgoLanes), 0, s, p, Ap, N, sc, 2);
                hipLaunchKernelGGL(gba_update, dim3(gN), dim3(64), 0, s, Lm, n, p, Ap, x, r, z, sc);
                hipLaunchKernelGGL(pgo_reduce, dim3(1), dim3(kPgoLanes), 0, s, r, z, N, sc, 3);
                hipLaunchKernelGGL(pgo_pupdate, dim3(gN6), dim3(256), 0, s, (int)N, z, p, sc);
            }
            launched += chunk;
            SLAM_HIP(c, hipGetLastError());
            SLAM_HIP(c, hipMemcpyAsync(h_sc, sc, sizeof(PgoSc), hipMemcpyDeviceToHost, s));
            if (int rc = stream_sync(c, s, true)) return rc;
            if (h_sc->done || launched >= prm->max_pcg) break;
        }
        pcg_total += h_sc->iters;
        hipLaunchKernelGGL(gba_pt_gather, dim3(gM), dim3(256), 0, s, linA, inK, poff, po, oc, x, Ci, gp, m, 1, wv, sc);
        hipLaunchKernelGGL(gba_step_cams, dim3(gNc), dim3(256), 0, s, C, x, held, n, Ct);
        hipLaunchKernelGGL(gba_step_points, dim3(gM), dim3(256), 0, s, X, wv, poff, m, Xt);
        double ct = 0.0;
        if (int rc = linearize(Ct, Xt, linB, &ct)) return rc;
        lm++;
        if (ct < cur) {
            const double rel = (cur - ct) / cur;
            std::swap(C, Ct);
            std::swap(X, Xt);
            std::swap(linA, linB);
            cur = ct;
            accepted++;
            lambda = lambda / 10.0;
            if (rel < prm->cost_tol) break;
        } else {
            lambda = lambda * 10.0;
        }
    }
    SLAM_HIP(c, hipMemcpyAsync(d_cams, C, 7 * 8 * nn, hipMemcpyDeviceToDevice, s));
    SLAM_HIP(c, hipMemcpyAsync(d_points, X, 3 * 8 * M, hipMemcpyDeviceToDevice, s));
    out->cost0 = c0;
    out->cost = cur;
    out->lm_steps = lm;
    out->accepted = accepted;
    out->pcg_iters = pcg_total;
    return stream_sync(c, s);
}

extern "C" int slam_gba(slam_ctx* c, const double* K4, double* cams, int n, double* points, int m, const int32_t* obs_cam,
                        const int32_t* obs_point, const double* obs_xy, int nobs, const slam_gba_params* prm, slam_gba_summary* out)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (!out || gba_check(K4, cams, n, points, m, obs_cam, obs_point, obs_xy, nobs, prm)) return set_err(c, SLAM_E_INVALID_ARG, "gba: bad arguments");
    SLAM_HIP(c, hipSetDevice(c->device));
    DevLayout lay;
    const auto s_cams = lay.add<double>(7 * (size_t)n), s_pts = lay.add<double>(3 * (size_t)m);
    DevMem d;
    SLAM_HIP(c, d.bind(c->gba_in, lay));
    if (n > 0) SLAM_HIP(c, d.upload(s_cams, cams, c->stream));
    if (m > 0) SLAM_HIP(c, d.upload(s_pts, points, c->stream));
    if (int rc = slam_gba_dev(c, c->stream, K4, d.ptr(s_cams), n, d.ptr(s_pts), m, obs_cam, obs_point, obs_xy, nobs, prm, out)) return rc;
    if (n > 0) SLAM_HIP(c, d.download(cams, s_cams, c->stream));
    if (m > 0) SLAM_HIP(c, d.download(points, s_pts, c->stream));
    return stream_sync(c, c->stream);
}

// Global bundle adjustment on the host: slam_gba_host, the twin of gba.hip's kernels, and the argument check and
// observation plan both paths share.  No context and no device; the arithmetic is gba_math.h's in the order
// tests/gba_ref.py states, so the results equal the device's and the reference's bit for bit.
#include "gba_plan.h"
#include "gba_math.h"

#include <cstring>
#include <utility>
#include <vector>

namespace slamhip {

namespace {
bool finite(double v) { return v - v == 0.0; }
}  // namespace

int gba_check(const double* K4, const double* cams, int n, const double* points, int m, const int32_t* obs_cam,
              const int32_t* obs_point, const double* obs_xy, int nobs, const slam_gba_params* prm)
{
    if (!K4 || !prm || n < 0 || m < 0 || nobs < 0 || (n > 0 && !cams) || (m > 0 && !points) ||
        (nobs > 0 && (!obs_cam || !obs_point || !obs_xy)))
        return SLAM_E_INVALID_ARG;
    if (!(K4[0] > 0.0) || !(K4[1] > 0.0) || !finite(K4[0]) || !finite(K4[1]) || !finite(K4[2]) || !finite(K4[3]))
        return SLAM_E_INVALID_ARG;
    if (!(prm->zmin > 0.0) || !finite(prm->zmin) || !(prm->lambda0 >= 0.0) || !finite(prm->lambda0) || prm->max_lm < 0 ||
        prm->max_pcg < 0 || !(prm->pcg_tol >= 0.0) || !(prm->cost_tol >= 0.0))
        return SLAM_E_INVALID_ARG;
    if (prm->loss != SLAM_GBA_LOSS_SQUARE && prm->loss != SLAM_GBA_LOSS_HUBER) return SLAM_E_INVALID_ARG;
    if (prm->loss == SLAM_GBA_LOSS_HUBER && (!(prm->loss_param > 0.0) || !finite(prm->loss_param))) return SLAM_E_INVALID_ARG;
    for (int k = 0; k < n; k++) {
        const double* q = cams + 7 * (size_t)k;
        const double nq = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
        if (!(nq > 0.0) || !(nq < 1e300)) return SLAM_E_INVALID_ARG;
    }
    for (int o = 0; o < nobs; o++) {
        if (obs_cam[o] < 0 || obs_cam[o] >= n || obs_point[o] < 0 || obs_point[o] >= m) return SLAM_E_INVALID_ARG;
        if (!finite(obs_xy[2 * (size_t)o]) || !finite(obs_xy[2 * (size_t)o + 1])) return SLAM_E_INVALID_ARG;
    }
    return SLAM_OK;
}

void gba_plan(const double* cams, int n, const double* points, int m, const int32_t* obs_cam, const int32_t* obs_point,
              const double* obs_xy, int nobs, double zmin, GbaPlan& plan)
{
    std::vector<uint8_t> keep((size_t)nobs, 0);
    std::vector<int32_t> left((size_t)m, 0);
    plan.behind = 0;
    for (int o = 0; o < nobs; o++) {
        const double z = gba_depth(cams + 7 * (size_t)obs_cam[o], points + 3 * (size_t)obs_point[o]);
        keep[o] = z > zmin ? 1 : 0;
        if (keep[o])
            left[obs_point[o]]++;
        else
            plan.behind++;
    }
    plan.cam_off.assign((size_t)n + 1, 0);
    plan.pt_off.assign((size_t)m + 1, 0);
    plan.nk = 0;
    for (int o = 0; o < nobs; o++) {
        keep[o] = keep[o] && left[obs_point[o]] >= 2;
        if (keep[o]) {
            plan.cam_off[obs_cam[o] + 1]++;
            plan.pt_off[obs_point[o] + 1]++;
            plan.nk++;
        }
    }
    for (int k = 0; k < n; k++) plan.cam_off[k + 1] += plan.cam_off[k];
    for (int p = 0; p < m; p++) plan.pt_off[p + 1] += plan.pt_off[p];
    const size_t nk = (size_t)plan.nk;
    plan.obs_cam.assign(nk, 0);
    plan.obs_pt.assign(nk, 0);
    plan.xy.assign(2 * nk, 0.0);
    plan.pt_obs.assign(nk, 0);
    std::vector<int32_t> cur(plan.cam_off.begin(), plan.cam_off.end() - 1);
    for (int o = 0; o < nobs; o++) {        // ascending o: a stable sort by camera
        if (!keep[o]) continue;
        const int32_t at = cur[obs_cam[o]]++;
        plan.obs_cam[at] = obs_cam[o];
        plan.obs_pt[at] = obs_point[o];
        plan.xy[2 * (size_t)at] = obs_xy[2 * (size_t)o];
        plan.xy[2 * (size_t)at + 1] = obs_xy[2 * (size_t)o + 1];
    }
    cur.assign(plan.pt_off.begin(), plan.pt_off.end() - 1);
    for (size_t at = 0; at < nk; at++) plan.pt_obs[cur[plan.obs_pt[at]]++] = (int32_t)at;      // ascending positions
    plan.held.assign((size_t)n, 0);
    plan.cams_held = 0;
    for (int k = 0; k < n; k++) {
        plan.held[k] = k == 0 || plan.cam_off[k + 1] == plan.cam_off[k];
        plan.cams_held += plan.held[k];
    }
    plan.points_held = 0;
    for (int p = 0; p < m; p++) plan.points_held += plan.pt_off[p + 1] == plan.pt_off[p];
}

void gba_summary_init(const GbaPlan& plan, slam_gba_summary* out)
{
    memset(out, 0, sizeof(*out));
    out->kept_obs = plan.nk;
    out->behind_obs = plan.behind;
    out->points_held = plan.points_held;
    out->cams_held = plan.cams_held;
}

namespace {

// sum of a[i] (b null) or a[i] b[i]: 1024 strided partials in ascending i, then the binary tree
double tree_sum(const double* a, const double* b, size_t n)
{
    std::vector<double> part(kPgoLanes, 0.0);
    for (size_t i = 0; i < n; i++) part[i % kPgoLanes] = part[i % kPgoLanes] + (b ? a[i] * b[i] : a[i]);
    for (int off = kPgoLanes / 2; off >= 1; off >>= 1)
        for (int l = 0; l < off; l++) part[l] = part[l] + part[l + off];
    return part[0];
}

// The S sums of one camera over its positions lo .. hi: lane l adds positions lo + l, lo + l + 64, ... in ascending
// order, then the lanes fold +32 .. +1.  term(o, out) gives the S terms of position o.
template <int S, class F> void lane_tree(int lo, int hi, F term, double* sums)
{
    double part[kGbaLanes][S];
    for (int l = 0; l < kGbaLanes; l++)
        for (int j = 0; j < S; j++) part[l][j] = 0.0;
    for (int o = lo; o < hi; o++) {
        double t[S];
        term(o, t);
        const int l = (o - lo) % kGbaLanes;
        for (int j = 0; j < S; j++) part[l][j] = part[l][j] + t[j];
    }
    for (int off = kGbaLanes / 2; off >= 1; off >>= 1)
        for (int l = 0; l < off; l++)
            for (int j = 0; j < S; j++) part[l][j] = part[l][j] + part[l + off][j];
    for (int j = 0; j < S; j++) sums[j] = part[0][j];
}

struct Problem {
    const GbaPlan& pl;
    const double* K4;
    const slam_gba_params& prm;
    int n, m;
};

double linearize(const Problem& P, const double* cams, const double* pts, std::vector<double>& lin, std::vector<double>& ccost)
{
    const size_t nk = (size_t)P.pl.nk;
    for (size_t o = 0; o < nk; o++) {
        double out[kGbaLin];
        const int k = P.pl.obs_cam[o];
        gba_obs_lin(cams + 7 * (size_t)k, pts + 3 * (size_t)P.pl.obs_pt[o], P.K4, P.pl.xy[2 * o], P.pl.xy[2 * o + 1], P.prm.loss,
                    P.prm.loss_param, P.prm.zmin, P.pl.held[k] != 0, out);
        for (int c = 0; c < kGbaLin; c++) lin[(size_t)c * nk + o] = out[c];
    }
    for (int k = 0; k < P.n; k++)
        lane_tree<1>(P.pl.cam_off[k], P.pl.cam_off[k + 1], [&](int o, double* t) { t[0] = lin[(size_t)kGbaRho * nk + o]; }, &ccost[k]);
    return tree_sum(ccost.data(), nullptr, (size_t)P.n);
}

}  // namespace

}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_gba_host(const double* K4, double* cams, int n, double* points, int m, const int32_t* obs_cam,
                             const int32_t* obs_point, const double* obs_xy, int nobs, const slam_gba_params* prm,
                             slam_gba_summary* out)
{
    if (!out || gba_check(K4, cams, n, points, m, obs_cam, obs_point, obs_xy, nobs, prm)) return SLAM_E_INVALID_ARG;
    GbaPlan pl;
    gba_plan(cams, n, points, m, obs_cam, obs_point, obs_xy, nobs, prm->zmin, pl);
    gba_summary_init(pl, out);
    if (n <= 1 || pl.nk == 0) return SLAM_OK;
    const Problem P = {pl, K4, *prm, n, m};
    const size_t nk = (size_t)pl.nk, N = 6 * (size_t)n, M = (size_t)m;
    std::vector<double> C(cams, cams + 7 * (size_t)n), Ct(7 * (size_t)n), X(points, points + 3 * M), Xt(3 * M);
    std::vector<double> linA(kGbaLin * nk), linB(kGbaLin * nk), ccost((size_t)n);
    std::vector<double> Ci(9 * M), gp(3 * M), w(3 * M), dl(N), Lm(36 * (size_t)n), b(N), x(N), r(N), z(N), p(N), Ap(N);
    const double c0 = linearize(P, C.data(), X.data(), linA, ccost);
    double cur = c0, lambda = prm->lambda0;
    int lm = 0, accepted = 0, pcg_total = 0;
    // a point's values are component-major like a linearisation's: value c of point q is v[c * m + q]
    auto point_pass = [&](const std::vector<double>& lin, const double* vec, int mode, std::vector<double>& dst) {
        for (int q = 0; q < m; q++) {
            double ci[9], g[3], o3[3];
            for (int c = 0; c < 9; c++) ci[c] = Ci[(size_t)c * M + q];
            for (int c = 0; c < 3; c++) g[c] = gp[(size_t)c * M + q];
            gba_point_gather(lin.data(), nk, pl.pt_obs.data() + pl.pt_off[q], pl.pt_off[q + 1] - pl.pt_off[q], pl.obs_cam.data(), vec,
                             ci, g, mode, o3);
            for (int c = 0; c < 3; c++) dst[(size_t)c * M + q] = o3[c];
        }
    };
    while (lm < prm->max_lm && cur > 0.0) {
        const double* lin = linA.data();
        for (int q = 0; q < m; q++) {
            double ci[9], g[3];
            gba_point_block(lin, nk, pl.pt_obs.data() + pl.pt_off[q], pl.pt_off[q + 1] - pl.pt_off[q], lambda, ci, g);
            for (int c = 0; c < 9; c++) Ci[(size_t)c * M + q] = ci[c];
            for (int c = 0; c < 3; c++) gp[(size_t)c * M + q] = g[c];
        }
        for (int k = 0; k < n; k++) {
            double sums[kGbaCamSums];
            lane_tree<kGbaCamSums>(pl.cam_off[k], pl.cam_off[k + 1], [&](int o, double* t) {
                double v[kGbaLin], ci[9], g[3];
                gba_load(lin, nk, (size_t)o, 0, kGbaLin, v);
                const size_t q = (size_t)pl.obs_pt[o];
                for (int c = 0; c < 9; c++) ci[c] = Ci[(size_t)c * M + q];
                for (int c = 0; c < 3; c++) g[c] = gp[(size_t)c * M + q];
                gba_cam_terms(v + kGbaJc, v + kGbaJp, v + kGbaR, ci, g, t);
            }, sums);
            gba_cam_finish(sums, lambda, &dl[6 * (size_t)k], &Lm[36 * (size_t)k], &b[6 * (size_t)k]);
        }
        // PCG on the Schur complement
        for (size_t i = 0; i < N; i++) {
            x[i] = 0.0;
            r[i] = b[i];
        }
        for (int k = 0; k < n; k++) gba_chol_solve<6>(&Lm[36 * (size_t)k], &r[6 * (size_t)k], &z[6 * (size_t)k]);
        p = z;
        double rz = tree_sum(r.data(), z.data(), N);
        const double rz0 = rz;
        bool done = !(rz0 > 0.0);
        int it = 0;
        while (it < prm->max_pcg && !done) {
            point_pass(linA, p.data(), 0, w);
            for (int k = 0; k < n; k++) {
                double sums[6];
                lane_tree<6>(pl.cam_off[k], pl.cam_off[k + 1], [&](int o, double* t) {
                    double v[kGbaLin], wp[3];
                    gba_load(lin, nk, (size_t)o, 0, kGbaLin, v);
                    for (int c = 0; c < 3; c++) wp[c] = w[(size_t)c * M + (size_t)pl.obs_pt[o]];
                    gba_apply_terms(v + kGbaJc, v + kGbaJp, &p[6 * (size_t)k], wp, t);
                }, sums);
                for (int i = 0; i < 6; i++) Ap[6 * (size_t)k + i] = dl[6 * (size_t)k + i] * p[6 * (size_t)k + i] + sums[i];
            }
            const double pAp = tree_sum(p.data(), Ap.data(), N);
            if (!(pAp > 0.0)) break;
            const double alpha = rz / pAp;
            for (size_t i = 0; i < N; i++) {
                x[i] = x[i] + alpha * p[i];
                r[i] = r[i] - alpha * Ap[i];
            }
            for (int k = 0; k < n; k++) gba_chol_solve<6>(&Lm[36 * (size_t)k], &r[6 * (size_t)k], &z[6 * (size_t)k]);
            const double rzn = tree_sum(r.data(), z.data(), N);
            it++;
            if (rzn <= prm->pcg_tol * rz0) {
                done = true;
            } else {
                const double beta = rzn / rz;
                for (size_t i = 0; i < N; i++) p[i] = z[i] + beta * p[i];
            }
            rz = rzn;
        }
        pcg_total += it;
        point_pass(linA, x.data(), 1, w);      // w: the points' steps
        for (int k = 0; k < n; k++) {
            memcpy(&Ct[7 * (size_t)k], &C[7 * (size_t)k], 7 * sizeof(double));
            if (!pl.held[k]) gba_cam_step(&Ct[7 * (size_t)k], &x[6 * (size_t)k]);
        }
        for (int q = 0; q < m; q++)
            for (int c = 0; c < 3; c++) {
                const double v = X[3 * (size_t)q + c];
                Xt[3 * (size_t)q + c] = pl.pt_off[q + 1] == pl.pt_off[q] ? v : v + w[(size_t)c * M + q];
            }
        const double ct = linearize(P, Ct.data(), Xt.data(), linB, ccost);
        lm++;
        if (ct < cur) {
            const double rel = (cur - ct) / cur;
            C.swap(Ct);
            X.swap(Xt);
            linA.swap(linB);
            cur = ct;
            accepted++;
            lambda = lambda / 10.0;
            if (rel < prm->cost_tol) break;
        } else {
            lambda = lambda * 10.0;
        }
    }
    memcpy(cams, C.data(), 7 * (size_t)n * sizeof(double));
    memcpy(points, X.data(), 3 * M * sizeof(double));
    out->cost0 = c0;
    out->cost = cur;
    out->lm_steps = lm;
    out->accepted = accepted;
    out->pcg_iters = pcg_total;
    return SLAM_OK;
}

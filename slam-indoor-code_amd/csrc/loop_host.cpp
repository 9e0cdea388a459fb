// Loop closing on the host: slam_sim3_ransac_host, slam_pgo_sim3_host and
// slam_sim3_apply_points_host, the twins of loop.hip's kernels, and the argument checks both paths share.  They need no
// context and no device; the arithmetic is loop_math.h's in the order tests/loop_ref.py
// states, so the results equal the device's and the reference's bit for bit.
#include "../../include/slamhip.h"
#include "loop_math.h"

#include <cstring>
#include <utility>
#include <vector>

namespace slamhip {

int loop_check_ransac(const int32_t* offsets, int L, const double* centres, int H, double tau)
{
    if (L < 0 || L > kSim3MaxLoops || H < 1 || H > kSim3MaxHyp || !(tau > 0.0) || !(tau < 1e150)) return SLAM_E_INVALID_ARG;
    if (L == 0) return SLAM_OK;
    if (!offsets || !centres || offsets[0] < 0) return SLAM_E_INVALID_ARG;
    for (int l = 0; l < L; l++) {
        const int64_t n = (int64_t)offsets[l + 1] - offsets[l];
        if (n < 0 || n > kSim3MaxPairs) return SLAM_E_INVALID_ARG;
    }
    return SLAM_OK;
}

int loop_check_nodes(const double* nodes, int m)
{
    if (m < 0 || (m > 0 && !nodes)) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < m; i++)
        if (!sim3_valid(nodes + 8 * (size_t)i)) return SLAM_E_INVALID_ARG;
    return SLAM_OK;
}

void loop_draw_samples(const int32_t* offsets, int L, int H, uint64_t seed, int32_t* samples)
{
    for (int l = 0; l < L; l++) {
        const int n = offsets[l + 1] - offsets[l];
        for (int h = 0; h < H; h++) {
            int32_t* s = samples + 3 * ((size_t)l * H + h);
            if (n >= 3)
                sim3_sample(seed, (uint32_t)l, (uint32_t)h, n, s);
            else
                s[0] = s[1] = s[2] = 0;
        }
    }
}

int loop_check_pgo(const double* nodes, int n, const int32_t* edges, const double* meas, const double* weight, int E,
                   double ell, double lambda0, int max_lm, int max_pcg, double pcg_tol, double cost_tol)
{
    if (n < 1 || n > kSim3MaxPairs || E < 0 || E > kSim3MaxPairs || !nodes || (E > 0 && (!edges || !meas || !weight)))
        return SLAM_E_INVALID_ARG;
    if (!(ell > 0.0) || !(ell < 1e300) || !(lambda0 >= 0.0) || !(lambda0 < 1e300) || max_lm < 0 || max_pcg < 0 ||
        !(pcg_tol >= 0.0) || !(cost_tol >= 0.0))
        return SLAM_E_INVALID_ARG;
    if (loop_check_nodes(nodes, n) || loop_check_nodes(meas, E)) return SLAM_E_INVALID_ARG;
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int e = 0; e < E; e++) {
        const int i = edges[2 * (size_t)e], j = edges[2 * (size_t)e + 1];
        if (i < 0 || i >= n || j < 0 || j >= n || i == j) return SLAM_E_INVALID_ARG;
        if (!(weight[e] >= 0.0) || !(weight[e] < 1e300)) return SLAM_E_INVALID_ARG;
        seen[i] = 1;
        seen[j] = 1;
    }
    for (int a = 0; a < n; a++)
        if (!seen[a]) return SLAM_E_INVALID_ARG;
    return SLAM_OK;
}

void pgo_build_csr(int n, const int32_t* edges, int E, std::vector<int32_t>& start, std::vector<int32_t>& ent)
{
    start.assign((size_t)n + 1, 0);
    for (int e = 0; e < E; e++) {
        start[edges[2 * (size_t)e] + 1]++;
        start[edges[2 * (size_t)e + 1] + 1]++;
    }
    for (int a = 0; a < n; a++) start[a + 1] += start[a];
    ent.assign(2 * (size_t)E, 0);
    std::vector<int32_t> cur(start.begin(), start.end() - 1);
    for (int e = 0; e < E; e++) {       // ascending edges: a node's list is in edge order
        ent[cur[edges[2 * (size_t)e]]++] = 2 * e;
        ent[cur[edges[2 * (size_t)e + 1]]++] = 2 * e + 1;
    }
}

void pgo_edge_constants(const double* meas, const double* weight, int E, double* zinv, double* sw)
{
    for (int e = 0; e < E; e++) {
        sim3_inverse(meas + 8 * (size_t)e, zinv + 8 * (size_t)e);
        sw[e] = sqrt(weight[e]);
    }
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

struct PgoLin {
    std::vector<double> r, J, c;      // E x 7, E x 2 x 49, E
};

double pgo_linearize(const double* S, const int32_t* edges, const double* zinv, const double* sw, int E, double ell, PgoLin& o)
{
    o.r.resize(7 * (size_t)E);
    o.J.resize(98 * (size_t)E);
    o.c.resize((size_t)E);
    for (int e = 0; e < E; e++) {
        const int i = edges[2 * (size_t)e], j = edges[2 * (size_t)e + 1];
        pgo_edge(S + 8 * (size_t)i, S + 8 * (size_t)j, zinv + 8 * (size_t)e, sw[e], ell, i == 0, j == 0, &o.r[7 * (size_t)e],
                 &o.J[98 * (size_t)e], &o.J[98 * (size_t)e + 49]);
        o.c[e] = pgo_edge_cost(&o.r[7 * (size_t)e]);
    }
    return tree_sum(o.c.data(), nullptr, (size_t)E);
}

void identity_sim(double* S)
{
    for (int k = 0; k < 8; k++) S[k] = 0.0;
    S[0] = 1.0;
    S[1] = 1.0;
}

// one loop: pairs a, b (n x 3), centres ci (a's camera) and cj (b's camera)
void ransac_one(const double* a, const double* b, int n, const double* ci, const double* cj, int H, double tau,
                const int32_t* samples, double* S, uint8_t* mask, int32_t* count, int32_t* status)
{
    identity_sim(S);
    *count = 0;
    if (n > 0) memset(mask, 0, (size_t)n);
    if (n < 3) {
        *status = kSim3TooFew;
        return;
    }
    const double tau2 = tau * tau;
    std::vector<double> da2(n), db2(n);
    for (int k = 0; k < n; k++) {
        da2[k] = dist2(a + 3 * (size_t)k, ci);
        db2[k] = dist2(b + 3 * (size_t)k, cj);
    }
    int best = 0, best_h = -1;
    double Sb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int h = 0; h < H; h++) {
        const int32_t* s = samples + 3 * (size_t)h;
        double Sh[8], R[9];
        if (!sim3_hypothesis(a + 3 * (size_t)s[0], a + 3 * (size_t)s[1], a + 3 * (size_t)s[2], b + 3 * (size_t)s[0],
                             b + 3 * (size_t)s[1], b + 3 * (size_t)s[2], Sh))
            continue;
        quat_matrix(Sh + 1, R);
        int cnt = 0;
        for (int k = 0; k < n; k++)
            cnt += sim3_inlier(Sh[0], R, Sh + 5, a + 3 * (size_t)k, b + 3 * (size_t)k, da2[k], db2[k], tau2) ? 1 : 0;
        if (cnt > best) {
            best = cnt;
            best_h = h;
            memcpy(Sb, Sh, sizeof(Sb));
        }
    }
    if (best < 3 || best_h < 0) {
        *status = kSim3NoModel;
        return;
    }
    double R[9];
    quat_matrix(Sb + 1, R);
    for (int k = 0; k < n; k++)
        mask[k] = sim3_inlier(Sb[0], R, Sb + 5, a + 3 * (size_t)k, b + 3 * (size_t)k, da2[k], db2[k], tau2) ? 1 : 0;
    *count = best;
    *status = kSim3Ok;
    memcpy(S, Sb, sizeof(Sb));
    // the refit: lane l sums the pairs l, l + 64, ... in ascending order, then the lanes fold as a
    // binary tree (l += l + 32, l += l + 16, ... l += l + 1); a pair outside the mask adds +0.0
    for (int it = 0; it < kSim3RefitSteps; it++) {
        double part[kSim3Lanes][kSim3Terms];
        for (int l = 0; l < kSim3Lanes; l++)
            for (int j = 0; j < kSim3Terms; j++) part[l][j] = 0.0;
        quat_matrix(S + 1, R);
        for (int k = 0; k < n; k++) {
            double term[kSim3Terms];
            sim3_terms(S[0], R, S + 5, a + 3 * (size_t)k, b + 3 * (size_t)k, term);
            for (int j = 0; j < kSim3Terms; j++) part[k % kSim3Lanes][j] = part[k % kSim3Lanes][j] + (mask[k] ? term[j] : 0.0);
        }
        for (int off = kSim3Lanes / 2; off >= 1; off >>= 1)
            for (int l = 0; l < off; l++)
                for (int j = 0; j < kSim3Terms; j++) part[l][j] = part[l][j] + part[l + off][j];
        double d[7];
        if (!chol7_solve(part[0], part[0] + 28, d)) {
            *status = kSim3Cholesky;      // S keeps the last state that was reached
            return;
        }
        sim3_step(S, d);
    }
}

}  // namespace

}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_sim3_ransac_host(const double* a, const double* b, const int32_t* offsets, int L,
                                     const double* centres, int H, double tau, uint64_t seed, double* sim,
                                     uint8_t* mask, int32_t* count, int32_t* status)
{
    if (loop_check_ransac(offsets, L, centres, H, tau)) return SLAM_E_INVALID_ARG;
    if (L == 0) return SLAM_OK;
    const int32_t np = offsets[L] - offsets[0];
    if (!sim || !count || !status || (np > 0 && (!a || !b || !mask))) return SLAM_E_INVALID_ARG;
    std::vector<int32_t> samples(3 * (size_t)L * H);
    loop_draw_samples(offsets, L, H, seed, samples.data());
    for (int l = 0; l < L; l++) {
        const int lo = offsets[l], n = offsets[l + 1] - lo;
        ransac_one(a + 3 * (size_t)lo, b + 3 * (size_t)lo, n, centres + 6 * (size_t)l, centres + 6 * (size_t)l + 3, H, tau,
                   samples.data() + 3 * (size_t)l * H, sim + 8 * (size_t)l, mask ? mask + lo : nullptr, count + l, status + l);
    }
    return SLAM_OK;
}

extern "C" int slam_sim3_apply_points_host(const double* points, const int32_t* anchor, int n, const double* nodes,
                                           const double* nodes_new, int m, double* out)
{
    if (n < 0 || loop_check_nodes(nodes, m) || loop_check_nodes(nodes_new, m)) return SLAM_E_INVALID_ARG;
    if (n == 0) return SLAM_OK;
    if (!points || !anchor || !out) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < n; i++)
        if (anchor[i] < -1 || anchor[i] >= m) return SLAM_E_INVALID_ARG;
    for (int i = 0; i < n; i++) {
        const int a = anchor[i];
        if (a < 0)
            for (int k = 0; k < 3; k++) out[3 * (size_t)i + k] = points[3 * (size_t)i + k];
        else
            sim3_move_point(nodes + 8 * (size_t)a, nodes_new + 8 * (size_t)a, points + 3 * (size_t)i, out + 3 * (size_t)i);
    }
    return SLAM_OK;
}

extern "C" int slam_pgo_sim3_host(double* nodes, int n, const int32_t* edges, const double* meas, const double* weight, int E,
                                  double ell, double lambda0, int max_lm, int max_pcg, double pcg_tol, double cost_tol,
                                  double* cost, int32_t* iters)
{
    if (loop_check_pgo(nodes, n, edges, meas, weight, E, ell, lambda0, max_lm, max_pcg, pcg_tol, cost_tol) || !cost || !iters)
        return SLAM_E_INVALID_ARG;
    std::vector<int32_t> start, ent;
    pgo_build_csr(n, edges, E, start, ent);
    std::vector<double> zinv(8 * (size_t)E), sw((size_t)E);
    pgo_edge_constants(meas, weight, E, zinv.data(), sw.data());
    const size_t N = 7 * (size_t)n;
    std::vector<double> S(nodes, nodes + 8 * (size_t)n), St(8 * (size_t)n);
    std::vector<double> H(49 * (size_t)n), g(N), Hd(49 * (size_t)n), Lm(49 * (size_t)n), x(N), rr(N), z(N), p(N), Ap(N),
        u(14 * (size_t)E);
    PgoLin cur, tri;
    double c0 = pgo_linearize(S.data(), edges, zinv.data(), sw.data(), E, ell, cur), c = c0, lambda = lambda0;
    int lm = 0, accepted = 0, pcg_total = 0;
    while (lm < max_lm && c > 0.0) {
        // assemble: per node and row over its incident list in order
        for (int a = 0; a < n; a++)
            for (int row = 0; row < 7; row++) {
                double h[7] = {0, 0, 0, 0, 0, 0, 0}, gs = 0.0;
                for (int q = start[a]; q < start[a + 1]; q++) {
                    double hb[7], gb;
                    pgo_block_row(&cur.J[49 * (size_t)ent[q]], &cur.r[7 * (size_t)(ent[q] >> 1)], row, hb, &gb);
                    for (int k = 0; k < 7; k++) h[k] = h[k] + hb[k];
                    gs = gs - gb;
                }
                for (int k = 0; k < 7; k++) H[49 * (size_t)a + 7 * row + k] = h[k];
                g[7 * (size_t)a + row] = gs;
            }
        for (int a = 0; a < n; a++) pgo_damp_block(&H[49 * (size_t)a], lambda, a == 0, &Hd[49 * (size_t)a], &Lm[49 * (size_t)a]);
        // PCG on (J^T J + lambda D) x = g
        for (size_t i = 0; i < N; i++) {
            x[i] = 0.0;
            rr[i] = g[i];
        }
        for (int a = 0; a < n; a++) pgo_block_solve(&Lm[49 * (size_t)a], &rr[7 * (size_t)a], &z[7 * (size_t)a]);
        p = z;
        double rz = tree_sum(rr.data(), z.data(), N);
        const double rz0 = rz;
        bool done = !(rz0 > 0.0);
        int it = 0;
        while (it < max_pcg && !done) {
            for (int q = 0; q < 2 * E; q++) {
                const int node = edges[q];      // edges[2 e + side]
                pgo_jp(&cur.J[49 * (size_t)q], &p[7 * (size_t)node], &u[7 * (size_t)q]);
            }
            for (int a = 0; a < n; a++)
                for (int row = 0; row < 7; row++) {
                    const double* hd = &Hd[49 * (size_t)a + 7 * row];
                    const double* pa = &p[7 * (size_t)a];
                    double y = hd[0] * pa[0];
                    for (int k = 1; k < 7; k++) y = y + hd[k] * pa[k];
                    for (int q = start[a]; q < start[a + 1]; q++) y = y + pgo_jtu(&cur.J[49 * (size_t)ent[q]], &u[7 * (size_t)(ent[q] ^ 1)], row);
                    Ap[7 * (size_t)a + row] = y;
                }
            const double pAp = tree_sum(p.data(), Ap.data(), N);
            if (!(pAp > 0.0)) {
                done = true;
                break;
            }
            const double alpha = rz / pAp;
            for (size_t i = 0; i < N; i++) {
                x[i] = x[i] + alpha * p[i];
                rr[i] = rr[i] - alpha * Ap[i];
            }
            for (int a = 0; a < n; a++) pgo_block_solve(&Lm[49 * (size_t)a], &rr[7 * (size_t)a], &z[7 * (size_t)a]);
            const double rzn = tree_sum(rr.data(), z.data(), N);
            it++;
            if (rzn <= pcg_tol * rz0) {
                done = true;
            } else {
                const double beta = rzn / rz;
                for (size_t i = 0; i < N; i++) p[i] = z[i] + beta * p[i];
            }
            rz = rzn;
        }
        pcg_total += it;
        for (int a = 0; a < n; a++) {
            memcpy(&St[8 * (size_t)a], &S[8 * (size_t)a], 8 * sizeof(double));
            if (a > 0) sim3_step(&St[8 * (size_t)a], &x[7 * (size_t)a]);
        }
        const double ct = pgo_linearize(St.data(), edges, zinv.data(), sw.data(), E, ell, tri);
        lm++;
        if (ct < c) {
            const double rel = (c - ct) / c;
            S.swap(St);
            std::swap(cur, tri);
            c = ct;
            accepted++;
            lambda = lambda / 10.0;
            if (rel < cost_tol) break;
        } else {
            lambda = lambda * 10.0;
        }
    }
    memcpy(nodes, S.data(), 8 * (size_t)n * sizeof(double));
    cost[0] = c0;
    cost[1] = c;
    iters[0] = lm;
    iters[1] = accepted;
    iters[2] = pcg_total;
    return SLAM_OK;
}

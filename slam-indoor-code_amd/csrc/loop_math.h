// Loop closing: the arithmetic shared by the kernels (loop.hip) and the host twin
// (loop_host.cpp).  Only + - * / and sqrt in f64, nothing contracted, every sum in
// the order tests/loop_ref.py states, so device, twin and reference agree bit for bit.
//
// A similarity is 8 doubles S = (sigma, qw, qx, qy, qz, tx, ty, tz): x' = sigma R(q) x + t.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LOOP_HD __host__ __device__ inline
#else
#define LOOP_HD inline
#endif

namespace slamhip {

enum { kSim3Ok = 0, kSim3NoModel = 1, kSim3TooFew = 2, kSim3Cholesky = 3 };   // SLAM_SIM3_*
constexpr int kSim3MaxHyp = 65536;          // hypotheses per loop
constexpr int kSim3MaxPairs = 1 << 24;      // pairs per loop
constexpr int kSim3MaxLoops = 65535;        // loops per call (the grid's y)
constexpr int kSim3RefitSteps = 4;          // Gauss-Newton steps of the refit
constexpr int kSim3Lanes = 64;              // the refit's sums: 64 strided partials, then a binary tree
constexpr double kSim3Degenerate = 1e-12;   // a triangle with |u x v|^2 <= this |u|^2 |v|^2 gives no frame

// ---- the sample generator: splitmix64 of (seed, loop, hypothesis, draw) ----
LOOP_HD uint64_t loop_mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

LOOP_HD uint64_t loop_draw(uint64_t seed, uint32_t loop, uint32_t hyp, uint32_t k)
{
    const uint64_t ctr = ((uint64_t)loop << 40) ^ ((uint64_t)hyp << 8) ^ (uint64_t)k;
    return loop_mix64(loop_mix64(seed + 0x9e3779b97f4a7c15ull) ^ (ctr * 0x9e3779b97f4a7c15ull + 0x632be59bd9b4e019ull));
}

// three distinct indices of [0, n), n >= 3
LOOP_HD void sim3_sample(uint64_t seed, uint32_t loop, uint32_t hyp, int n, int32_t* idx)
{
    const int i0 = (int)(loop_draw(seed, loop, hyp, 0) % (uint64_t)n);
    int i1 = (int)(loop_draw(seed, loop, hyp, 1) % (uint64_t)(n - 1));
    if (i1 >= i0) i1++;
    int i2 = (int)(loop_draw(seed, loop, hyp, 2) % (uint64_t)(n - 2));
    const int lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
    if (i2 >= lo) i2++;
    if (i2 >= hi) i2++;
    idx[0] = i0;
    idx[1] = i1;
    idx[2] = i2;
}

// ---- small vectors ----
LOOP_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

LOOP_HD void cross3(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- quaternions (w, x, y, z) ----
LOOP_HD void quat_mul(const double* a, const double* b, double* c)
{
    const double w = ((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3];
    const double x = ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2];
    const double y = ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1];
    const double z = ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0];
    c[0] = w;
    c[1] = x;
    c[2] = y;
    c[3] = z;
}

LOOP_HD void quat_normalise(double* q)
{
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    q[0] = q[0] / n;
    q[1] = q[1] / n;
    q[2] = q[2] / n;
    q[3] = q[3] / n;
}

// R(q), row-major, of a unit quaternion
LOOP_HD void quat_matrix(const double* q, double* R)
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// the unit quaternion of a rotation matrix (Shepperd's branches), normalised
LOOP_HD void matrix_quat(const double* R, double* q)
{
    const double tr = (R[0] + R[4]) + R[8];
    if (tr > 0.0) {
        const double r = sqrt(1.0 + tr), f = 0.5 / r;
        q[0] = 0.5 * r;
        q[1] = (R[7] - R[5]) * f;
        q[2] = (R[2] - R[6]) * f;
        q[3] = (R[3] - R[1]) * f;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        const double r = sqrt(((1.0 + R[0]) - R[4]) - R[8]), f = 0.5 / r;
        q[0] = (R[7] - R[5]) * f;
        q[1] = 0.5 * r;
        q[2] = (R[1] + R[3]) * f;
        q[3] = (R[2] + R[6]) * f;
    } else if (R[4] >= R[8]) {
        const double r = sqrt(((1.0 + R[4]) - R[0]) - R[8]), f = 0.5 / r;
        q[0] = (R[2] - R[6]) * f;
        q[1] = (R[1] + R[3]) * f;
        q[2] = 0.5 * r;
        q[3] = (R[5] + R[7]) * f;
    } else {
        const double r = sqrt(((1.0 + R[8]) - R[0]) - R[4]), f = 0.5 / r;
        q[0] = (R[3] - R[1]) * f;
        q[1] = (R[2] + R[6]) * f;
        q[2] = (R[5] + R[7]) * f;
        q[3] = 0.5 * r;
    }
    quat_normalise(q);
}

LOOP_HD void mat_vec(const double* R, const double* v, double* o)
{
    o[0] = (R[0] * v[0] + R[1] * v[1]) + R[2] * v[2];
    o[1] = (R[3] * v[0] + R[4] * v[1]) + R[5] * v[2];
    o[2] = (R[6] * v[0] + R[7] * v[1]) + R[8] * v[2];
}

LOOP_HD void mat_t_vec(const double* R, const double* v, double* o)
{
    o[0] = (R[0] * v[0] + R[3] * v[1]) + R[6] * v[2];
    o[1] = (R[1] * v[0] + R[4] * v[1]) + R[7] * v[2];
    o[2] = (R[2] * v[0] + R[5] * v[1]) + R[8] * v[2];
}

// sigma (R x) + t with R = R(q) given
LOOP_HD void sim3_map(double sigma, const double* R, const double* t, const double* x, double* o)
{
    double y[3];
    mat_vec(R, x, y);
    o[0] = sigma * y[0] + t[0];
    o[1] = sigma * y[1] + t[1];
    o[2] = sigma * y[2] + t[2];
}

// true when a similarity can be used: sigma > 0 and finite, q not zero and finite
LOOP_HD bool sim3_valid(const double* S)
{
    const double n = ((S[1] * S[1] + S[2] * S[2]) + S[3] * S[3]) + S[4] * S[4];
    return S[0] > 0.0 && S[0] < 1e300 && n > 0.0 && n < 1e300 && S[5] == S[5] && S[6] == S[6] && S[7] == S[7];
}

// ---- the hypothesis of one minimal set ----
// orthonormal frame (columns e1 e2 e3, stored F[r * 3 + k] = e_k[r]) on the triangle p0 p1 p2;
// false: |u x v|^2 <= kSim3Degenerate |u|^2 |v|^2 (collinear, repeated or not finite)
LOOP_HD bool sim3_frame(const double* p0, const double* p1, const double* p2, double* F)
{
    double u[3], v[3], c[3], e1[3], e2[3], e3[3], w[3];
    for (int k = 0; k < 3; k++) {
        u[k] = p1[k] - p0[k];
        v[k] = p2[k] - p0[k];
    }
    cross3(u, v, c);
    const double lu2 = dot3(u, u), lv2 = dot3(v, v), lc2 = dot3(c, c);
    if (!(lc2 > (kSim3Degenerate * lu2) * lv2) || !(lc2 < 1e300)) return false;
    const double lu = sqrt(lu2);
    for (int k = 0; k < 3; k++) e1[k] = u[k] / lu;
    const double d = dot3(v, e1);
    for (int k = 0; k < 3; k++) w[k] = v[k] - d * e1[k];
    const double lw = sqrt(dot3(w, w));
    if (!(lw > 0.0)) return false;
    for (int k = 0; k < 3; k++) e2[k] = w[k] / lw;
    cross3(e1, e2, e3);
    for (int r = 0; r < 3; r++) {
        F[r * 3 + 0] = e1[r];
        F[r * 3 + 1] = e2[r];
        F[r * 3 + 2] = e3[r];
    }
    return true;
}

// sum over the three points of |p - mean|^2; mean = ((p0 + p1) + p2) / 3
LOOP_HD double sim3_spread(const double* p0, const double* p1, const double* p2, double* mean)
{
    for (int k = 0; k < 3; k++) mean[k] = ((p0[k] + p1[k]) + p2[k]) / 3.0;
    double d0[3], d1[3], d2[3];
    for (int k = 0; k < 3; k++) {
        d0[k] = p0[k] - mean[k];
        d1[k] = p1[k] - mean[k];
        d2[k] = p2[k] - mean[k];
    }
    return (dot3(d0, d0) + dot3(d1, d1)) + dot3(d2, d2);
}

// S (8 doubles) with b = s R a + t on the three pairs; false (S all zero): no model
LOOP_HD bool sim3_hypothesis(const double* a0, const double* a1, const double* a2, const double* b0, const double* b1,
                             const double* b2, double* S)
{
    for (int k = 0; k < 8; k++) S[k] = 0.0;
    double Fa[9], Fb[9], R[9], ma[3], mb[3], q[4];
    if (!sim3_frame(a0, a1, a2, Fa) || !sim3_frame(b0, b1, b2, Fb)) return false;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[r * 3 + c] = (Fb[r * 3] * Fa[c * 3] + Fb[r * 3 + 1] * Fa[c * 3 + 1]) + Fb[r * 3 + 2] * Fa[c * 3 + 2];
    const double sa = sim3_spread(a0, a1, a2, ma), sb = sim3_spread(b0, b1, b2, mb);
    if (!(sa > 0.0)) return false;
    const double s = sqrt(sb / sa);
    if (!(s > 0.0) || !(s < 1e300)) return false;
    matrix_quat(R, q);
    if (!(q[0] == q[0])) return false;
    double Rq[9], y[3];
    quat_matrix(q, Rq);
    mat_vec(Rq, ma, y);
    S[0] = s;
    S[1] = q[0];
    S[2] = q[1];
    S[3] = q[2];
    S[4] = q[3];
    S[5] = mb[0] - s * y[0];
    S[6] = mb[1] - s * y[1];
    S[7] = mb[2] - s * y[2];
    return true;
}

// ---- the scale-free inlier test ----
// e^2 = |b - (s R a + t)|^2 <= tau^2 |b - cj|^2 (db2) and <= (tau^2 s^2) |a - ci|^2 (da2)
LOOP_HD bool sim3_inlier(double s, const double* R, const double* t, const double* a, const double* b, double da2,
                         double db2, double tau2)
{
    double p[3], e[3];
    sim3_map(s, R, t, a, p);
    e[0] = b[0] - p[0];
    e[1] = b[1] - p[1];
    e[2] = b[2] - p[2];
    const double e2 = dot3(e, e);
    return e2 <= tau2 * db2 && e2 <= (tau2 * (s * s)) * da2;
}

LOOP_HD double dist2(const double* a, const double* c)
{
    const double d[3] = {a[0] - c[0], a[1] - c[1], a[2] - c[2]};
    return dot3(d, d);
}

// ---- the refit: Gauss-Newton on r = b - (s R(q) a + t) in (ds, dr, dt) ----
// the 35 terms of one pair: the upper triangle of J^T J row by row (28), then J^T r (7)
constexpr int kSim3Terms = 35;
LOOP_HD void sim3_terms(double s, const double* R, const double* t, const double* a, const double* b, double* out)
{
    double y[3], J[3][7], r[3];
    mat_vec(R, a, y);
    for (int k = 0; k < 3; k++) {
        const double p = s * y[k];
        r[k] = b[k] - (p + t[k]);
        J[k][0] = p;
        J[k][1] = s * (R[k * 3 + 2] * a[1] - R[k * 3 + 1] * a[2]);
        J[k][2] = s * (R[k * 3 + 0] * a[2] - R[k * 3 + 2] * a[0]);
        J[k][3] = s * (R[k * 3 + 1] * a[0] - R[k * 3 + 0] * a[1]);
        J[k][4] = k == 0 ? 1.0 : 0.0;
        J[k][5] = k == 1 ? 1.0 : 0.0;
        J[k][6] = k == 2 ? 1.0 : 0.0;
    }
    int o = 0;
    for (int i = 0; i < 7; i++)
        for (int j = i; j < 7; j++) out[o++] = (J[0][i] * J[0][j] + J[1][i] * J[1][j]) + J[2][i] * J[2][j];
    for (int i = 0; i < 7; i++) out[o++] = (J[0][i] * r[0] + J[1][i] * r[1]) + J[2][i] * r[2];
}

// solves A x = g for the symmetric 7 x 7 A given by its upper triangle (row by row) by Cholesky;
// false: a pivot is not positive
LOOP_HD bool chol7_solve(const double* upper, const double* g, double* x)
{
    double A[7][7], Lm[7][7], y[7];
    int o = 0;
    for (int i = 0; i < 7; i++)
        for (int j = i; j < 7; j++) {
            A[i][j] = upper[o];
            A[j][i] = upper[o];
            o++;
        }
    for (int j = 0; j < 7; j++) {
        double d = A[j][j];
        for (int k = 0; k < j; k++) d = d - Lm[j][k] * Lm[j][k];
        if (!(d > 0.0) || !(d < 1e300)) return false;
        Lm[j][j] = sqrt(d);
        for (int i = j + 1; i < 7; i++) {
            double v = A[i][j];
            for (int k = 0; k < j; k++) v = v - Lm[i][k] * Lm[j][k];
            Lm[i][j] = v / Lm[j][j];
        }
    }
    for (int i = 0; i < 7; i++) {
        double v = g[i];
        for (int k = 0; k < i; k++) v = v - Lm[i][k] * y[k];
        y[i] = v / Lm[i][i];
    }
    for (int i = 6; i >= 0; i--) {
        double v = y[i];
        for (int k = i + 1; k < 7; k++) v = v - Lm[k][i] * x[k];
        x[i] = v / Lm[i][i];
    }
    return true;
}

// the local step: sigma <- sigma (1 + ds), q <- normalise(q (x) (1, dr / 2)), t <- t + dt
LOOP_HD void sim3_step(double* S, const double* d)
{
    const double dq[4] = {1.0, d[1] / 2.0, d[2] / 2.0, d[3] / 2.0};
    double q[4];
    S[0] = S[0] * (1.0 + d[0]);
    quat_mul(S + 1, dq, q);
    quat_normalise(q);
    S[1] = q[0];
    S[2] = q[1];
    S[3] = q[2];
    S[4] = q[3];
    S[5] = S[5] + d[4];
    S[6] = S[6] + d[5];
    S[7] = S[7] + d[6];
}

// ---- the map correction: X' = S'^-1 (S (X)); a node whose 8 values did not change leaves X alone ----
LOOP_HD void sim3_move_point(const double* S, const double* Sn, const double* X, double* out)
{
    bool same = true;
    for (int k = 0; k < 8; k++) same = same && S[k] == Sn[k];
    if (same) {
        out[0] = X[0];
        out[1] = X[1];
        out[2] = X[2];
        return;
    }
    double R[9], Rn[9], Y[3], d[3], z[3];
    quat_matrix(S + 1, R);
    quat_matrix(Sn + 1, Rn);
    sim3_map(S[0], R, S + 5, X, Y);
    d[0] = Y[0] - Sn[5];
    d[1] = Y[1] - Sn[6];
    d[2] = Y[2] - Sn[7];
    mat_t_vec(Rn, d, z);
    out[0] = z[0] / Sn[0];
    out[1] = z[1] / Sn[0];
    out[2] = z[2] / Sn[0];
}

// ---- the pose graph over Sim(3) ----
constexpr int kPgoLanes = 1024;     // sums over edges / unknowns: 1024 strided partials, then a binary tree
constexpr int kPgoChunk = 8;        // PCG iterations launched between two reads of the stop flag

LOOP_HD void sim3_inverse(const double* S, double* I)
{
    const double qc[4] = {S[1], -S[2], -S[3], -S[4]};
    double R[9], y[3];
    quat_matrix(qc, R);
    mat_vec(R, S + 5, y);
    I[0] = 1.0 / S[0];
    I[1] = qc[0];
    I[2] = qc[1];
    I[3] = qc[2];
    I[4] = qc[3];
    I[5] = -(y[0] / S[0]);
    I[6] = -(y[1] / S[0]);
    I[7] = -(y[2] / S[0]);
}

// x -> A(B(x)); the quaternion product is not normalised
LOOP_HD void sim3_compose(const double* A, const double* B, double* C)
{
    double q[4], R[9], t[3];
    quat_mul(A + 1, B + 1, q);
    quat_matrix(A + 1, R);
    sim3_map(A[0], R, A + 5, B + 5, t);
    C[0] = A[0] * B[0];
    C[1] = q[0];
    C[2] = q[1];
    C[3] = q[2];
    C[4] = q[3];
    C[5] = t[0];
    C[6] = t[1];
    C[7] = t[2];
}

// One edge (i, j, Z, w): E = Zinv o S_i o S_j^-1, r = sw (sigma_E - 1, 2 sign(qw) vec(q_E), t_E / ell)
// with sw = sqrt(w), and the Jacobians of r in the local steps of S_i and S_j (7 x 7, row-major,
// J[row * 7 + col], columns ds, dr, dt).  fix_i / fix_j: that node is the fixed one, its Jacobian is 0.
LOOP_HD void pgo_edge(const double* Si, const double* Sj, const double* A, double sw, double ell, bool fix_i, bool fix_j,
                      double* r, double* Ji, double* Jj)
{
    double Ri[9], Rjc[9], Rz[9], u[3], v[3], tM[3], P[4], qE[4], y[3], tE[3];
    const double qjc[4] = {Sj[1], -Sj[2], -Sj[3], -Sj[4]};
    quat_matrix(Si + 1, Ri);
    quat_matrix(qjc, Rjc);
    quat_matrix(A + 1, Rz);
    mat_vec(Rjc, Sj + 5, u);
    mat_vec(Ri, u, v);
    const double sM = Si[0] / Sj[0];
    for (int k = 0; k < 3; k++) tM[k] = Si[5 + k] - sM * v[k];
    quat_mul(A + 1, Si + 1, P);
    quat_mul(P, qjc, qE);
    const double sE = A[0] * sM;
    mat_vec(Rz, tM, y);
    for (int k = 0; k < 3; k++) tE[k] = A[0] * y[k] + A[5 + k];
    const double sgn = qE[0] >= 0.0 ? 1.0 : -1.0;
    r[0] = sw * (sE - 1.0);
    for (int k = 0; k < 3; k++) {
        r[1 + k] = sw * ((2.0 * sgn) * qE[1 + k]);
        r[4 + k] = sw * (tE[k] / ell);
    }
    for (int k = 0; k < 49; k++) {
        Ji[k] = 0.0;
        Jj[k] = 0.0;
    }
    const double c = (sw * A[0]) / ell;
    const double j00 = sw * sE;
    double w0[3];
    mat_vec(Rz, v, w0);
    if (!fix_i) Ji[0] = j00;
    if (!fix_j) Jj[0] = -j00;
    for (int m = 0; m < 3; m++) {
        const double a = sM * (c * w0[m]);
        if (!fix_i) Ji[(4 + m) * 7] = -a;
        if (!fix_j) Jj[(4 + m) * 7] = a;
    }
    for (int k = 0; k < 3; k++) {
        const double ek[4] = {0.0, k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        double t4[4], g[4], x[3], w1[3], w2[3], w3[3];
        quat_mul(P, ek, t4);
        quat_mul(t4, qjc, g);
        // e_k x u
        const double cr[3] = {k == 0 ? 0.0 : k == 1 ? u[2] : -u[1], k == 0 ? -u[2] : k == 1 ? 0.0 : u[0],
                              k == 0 ? u[1] : k == 1 ? -u[0] : 0.0};
        mat_vec(Ri, cr, x);
        mat_vec(Rz, x, w1);
        // R_M e_k = Ri (column k of Rjc)
        const double col[3] = {Rjc[k], Rjc[3 + k], Rjc[6 + k]};
        mat_vec(Ri, col, w2);
        mat_vec(Rz, w2, w3);
        for (int m = 0; m < 3; m++) {
            const double gq = sw * (sgn * g[1 + m]);
            const double a = sM * (c * w1[m]);
            if (!fix_i) {
                Ji[(1 + m) * 7 + 1 + k] = gq;
                Ji[(4 + m) * 7 + 1 + k] = -a;
                Ji[(4 + m) * 7 + 4 + k] = c * Rz[m * 3 + k];
            }
            if (!fix_j) {
                Jj[(1 + m) * 7 + 1 + k] = -gq;
                Jj[(4 + m) * 7 + 1 + k] = a;
                Jj[(4 + m) * 7 + 4 + k] = -(sM * (c * w3[m]));
            }
        }
    }
}

// |r|^2 of one edge, summed in component order
LOOP_HD double pgo_edge_cost(const double* r)
{
    double s = r[0] * r[0];
    for (int k = 1; k < 7; k++) s = s + r[k] * r[k];
    return s;
}

// row `row` of J^T J (7 values) and of J^T r of one 7 x 7 Jacobian: sums over the residual's components in order
LOOP_HD void pgo_block_row(const double* J, const double* r, int row, double* h, double* g)
{
    for (int c = 0; c < 7; c++) {
        double s = J[row] * J[c];
        for (int k = 1; k < 7; k++) s = s + J[k * 7 + row] * J[k * 7 + c];
        h[c] = s;
    }
    double s = J[row] * r[0];
    for (int k = 1; k < 7; k++) s = s + J[k * 7 + row] * r[k];
    *g = s;
}

// u = J p (7 values)
LOOP_HD void pgo_jp(const double* J, const double* p, double* u)
{
    for (int k = 0; k < 7; k++) {
        double s = J[k * 7] * p[0];
        for (int c = 1; c < 7; c++) s = s + J[k * 7 + c] * p[c];
        u[k] = s;
    }
}

// (J^T u)[row]
LOOP_HD double pgo_jtu(const double* J, const double* u, int row)
{
    double s = J[row] * u[0];
    for (int k = 1; k < 7; k++) s = s + J[k * 7 + row] * u[k];
    return s;
}

// Hd = H + lambda diag(H) and its Cholesky factor L (lower, row-major 7 x 7); the fixed node, or a block
// with a pivot that is not positive, gets Hd = L = I
LOOP_HD void pgo_damp_block(const double* H, double lambda, bool fixed, double* Hd, double* Lm)
{
    bool ok = !fixed;
    for (int i = 0; i < 49; i++) Hd[i] = H[i];
    for (int i = 0; i < 7; i++) Hd[i * 7 + i] = H[i * 7 + i] + lambda * H[i * 7 + i];
    for (int i = 0; i < 49; i++) Lm[i] = 0.0;
    // straight through (a failed pivot only clears `ok`; what follows it is thrown away below)
    for (int j = 0; j < 7; j++) {
        double d = Hd[j * 7 + j];
        for (int k = 0; k < j; k++) d = d - Lm[j * 7 + k] * Lm[j * 7 + k];
        ok = ok && d > 0.0 && d < 1e300;
        Lm[j * 7 + j] = sqrt(d);
        for (int i = j + 1; i < 7; i++) {
            double v = Hd[i * 7 + j];
            for (int k = 0; k < j; k++) v = v - Lm[i * 7 + k] * Lm[j * 7 + k];
            Lm[i * 7 + j] = v / Lm[j * 7 + j];
        }
    }
    if (!ok)
        for (int i = 0; i < 7; i++)
            for (int j = 0; j < 7; j++) {
                Hd[i * 7 + j] = i == j ? 1.0 : 0.0;
                Lm[i * 7 + j] = i == j ? 1.0 : 0.0;
            }
}

// z = (L L^T)^-1 r
LOOP_HD void pgo_block_solve(const double* Lm, const double* r, double* z)
{
    double y[7];
    for (int i = 0; i < 7; i++) {
        double v = r[i];
        for (int k = 0; k < i; k++) v = v - Lm[i * 7 + k] * y[k];
        y[i] = v / Lm[i * 7 + i];
    }
    for (int i = 6; i >= 0; i--) {
        double v = y[i];
        for (int k = i + 1; k < 7; k++) v = v - Lm[k * 7 + i] * z[k];
        z[i] = v / Lm[i * 7 + i];
    }
}

}  // namespace slamhip

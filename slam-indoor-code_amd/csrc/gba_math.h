// Global bundle adjustment: the arithmetic shared by the kernels (gba.hip) and the host twin
// (gba_host.cpp).  Only + - * / and sqrt in f64, nothing contracted, every sum in the order
// tests/gba_ref.py states, so device, twin and reference agree bit for bit.
//
// A camera is 7 doubles (qw, qx, qy, qz, tx, ty, tz): X_c = R(q) X + t, q a unit quaternion.
// A local step is q <- normalise(q (x) (1, dr / 2)), t <- t + dt (loop_math.h's rule).
//
// A linearisation holds kGbaLin doubles per kept observation, component-major: value c of
// observation o is lin[c * nk + o] (r 2, rho 1, J_c 2 x 6 row-major, J_p 2 x 3 row-major).
#pragma once

#include "loop_math.h"

namespace slamhip {

constexpr int kGbaLanes = 64;       // a per-camera sum: 64 strided partials, then a binary tree
constexpr int kGbaLin = 21;         // doubles per kept observation
constexpr int kGbaR = 0, kGbaRho = 2, kGbaJc = 3, kGbaJp = 15;
constexpr int kGbaCamSums = 54;     // B_k upper (21), sum J_c^T r (6), sum W C^-1 W^T upper (21), sum W C^-1 g_p (6)

// L (lower, row-major) of the symmetric N x N A; straight through, false when a pivot is not in (0, 1e300)
template <int N> LOOP_HD bool gba_chol(const double* A, double* Lm)
{
    bool ok = true;
    for (int i = 0; i < N * N; i++) Lm[i] = 0.0;
    for (int j = 0; j < N; j++) {
        double d = A[j * N + j];
        for (int k = 0; k < j; k++) d = d - Lm[j * N + k] * Lm[j * N + k];
        ok = ok && d > 0.0 && d < 1e300;
        Lm[j * N + j] = sqrt(d);
        for (int i = j + 1; i < N; i++) {
            double v = A[i * N + j];
            for (int k = 0; k < j; k++) v = v - Lm[i * N + k] * Lm[j * N + k];
            Lm[i * N + j] = v / Lm[j * N + j];
        }
    }
    return ok;
}

// z = (L L^T)^-1 r
template <int N> LOOP_HD void gba_chol_solve(const double* Lm, const double* r, double* z)
{
    double y[N];
    for (int i = 0; i < N; i++) {
        double v = r[i];
        for (int k = 0; k < i; k++) v = v - Lm[i * N + k] * y[k];
        y[i] = v / Lm[i * N + i];
    }
    for (int i = N - 1; i >= 0; i--) {
        double v = y[i];
        for (int k = i + 1; k < N; k++) v = v - Lm[k * N + i] * z[k];
        z[i] = v / Lm[i * N + i];
    }
}

// depth of X in a camera
LOOP_HD double gba_depth(const double* cam, const double* X)
{
    double R[9], Y[3];
    quat_matrix(cam, R);
    mat_vec(R, X, Y);
    return Y[2] + cam[6];
}

// One observation (px, py) of X by cam: out holds the kGbaLin values.  r = w (pi(X_c) - pixel), rho the loss of
// s = |pi(X_c) - pixel|^2 (+inf when z_c <= zmin), the Jacobians times w = sqrt(rho'); held: J_c = 0.
LOOP_HD void gba_obs_lin(const double* cam, const double* X, const double* K4, double px, double py, int loss, double a,
                         double zmin, bool held, double* out)
{
    double R[9], Y[3], M[9];
    quat_matrix(cam, R);
    mat_vec(R, X, Y);
    const double xc = Y[0] + cam[4], yc = Y[1] + cam[5], zc = Y[2] + cam[6];
    const double u = xc / zc, v = yc / zc;
    const double r0 = (K4[0] * u + K4[2]) - px, r1 = (K4[1] * v + K4[3]) - py;
    const double s = r0 * r0 + r1 * r1;
    double rho = s, w = 1.0;
    if (loss == 1 && s > a * a) {
        const double rs = sqrt(s);
        rho = (2.0 * a) * rs - a * a;
        w = sqrt(a / rs);
    }
    if (!(zc > zmin)) rho = __builtin_huge_val();
    const double a0 = K4[0] / zc, a1 = K4[1] / zc, b0 = -(a0 * u), b1 = -(a1 * v);
    // M = -R [X]x: column j is R (e_j x X)
    for (int i = 0; i < 3; i++) {
        M[3 * i + 0] = R[3 * i + 2] * X[1] - R[3 * i + 1] * X[2];
        M[3 * i + 1] = R[3 * i + 0] * X[2] - R[3 * i + 2] * X[0];
        M[3 * i + 2] = R[3 * i + 1] * X[0] - R[3 * i + 0] * X[1];
    }
    out[kGbaR] = w * r0;
    out[kGbaR + 1] = w * r1;
    out[kGbaRho] = rho;
    double* Jc = out + kGbaJc;
    double* Jp = out + kGbaJp;
    for (int j = 0; j < 3; j++) {
        Jc[j] = w * (a0 * M[j] + b0 * M[6 + j]);
        Jc[6 + j] = w * (a1 * M[3 + j] + b1 * M[6 + j]);
        Jp[j] = w * (a0 * R[j] + b0 * R[6 + j]);
        Jp[3 + j] = w * (a1 * R[3 + j] + b1 * R[6 + j]);
    }
    Jc[3] = w * a0;
    Jc[4] = 0.0;
    Jc[5] = w * b0;
    Jc[9] = 0.0;
    Jc[10] = w * a1;
    Jc[11] = w * b1;
    if (held)
        for (int k = 0; k < 12; k++) Jc[k] = 0.0;
}

// loads values [first, first + count) of observation o
LOOP_HD void gba_load(const double* lin, size_t nk, size_t o, int first, int count, double* out)
{
    for (int k = 0; k < count; k++) out[k] = lin[(size_t)(first + k) * nk + o];
}

// One point over its list (serial, in list order): C = sum J_p^T J_p, damped on its diagonal, by Cholesky; Ci (3 x 3,
// row-major) its inverse column by column, all zero when the Cholesky fails; g = -sum J_p^T r.
LOOP_HD void gba_point_block(const double* lin, size_t nk, const int32_t* list, int cnt, double lambda, double* Ci, double* g)
{
    double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sp[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < cnt; q++) {
        double Jp[6], r[2];
        gba_load(lin, nk, (size_t)list[q], kGbaJp, 6, Jp);
        gba_load(lin, nk, (size_t)list[q], kGbaR, 2, r);
        int t = 0;
        for (int i = 0; i < 3; i++) {
            for (int j = i; j < 3; j++, t++) C[t] = C[t] + (Jp[i] * Jp[j] + Jp[3 + i] * Jp[3 + j]);
            sp[i] = sp[i] + (Jp[i] * r[0] + Jp[3 + i] * r[1]);
        }
    }
    const double A[9] = {C[0] + lambda * C[0], C[1], C[2], C[1], C[3] + lambda * C[3], C[4], C[2], C[4], C[5] + lambda * C[5]};
    double Lm[9];
    const bool ok = gba_chol<3>(A, Lm);
    for (int j = 0; j < 3; j++) {
        const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
        double x[3];
        gba_chol_solve<3>(Lm, e, x);
        for (int i = 0; i < 3; i++) Ci[3 * i + j] = ok ? x[i] : 0.0;
    }
    for (int i = 0; i < 3; i++) g[i] = -sp[i];
}

// o = A v, A 3 x 3 row-major
LOOP_HD void gba_mul3(const double* A, const double* v, double* o)
{
    for (int i = 0; i < 3; i++) o[i] = (A[3 * i] * v[0] + A[3 * i + 1] * v[1]) + A[3 * i + 2] * v[2];
}

// the kGbaCamSums terms of one observation: Jc 2 x 6, Jp 2 x 3, r 2, Ci and gp of its point
LOOP_HD void gba_cam_terms(const double* Jc, const double* Jp, const double* r, const double* Ci, const double* gp, double* out)
{
    double W[18], T[18], y[3];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 3; j++) W[3 * i + j] = Jc[i] * Jp[j] + Jc[6 + i] * Jp[3 + j];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 3; j++) T[3 * i + j] = (W[3 * i] * Ci[j] + W[3 * i + 1] * Ci[3 + j]) + W[3 * i + 2] * Ci[6 + j];
    gba_mul3(Ci, gp, y);
    int t = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) out[t++] = Jc[i] * Jc[j] + Jc[6 + i] * Jc[6 + j];
    for (int i = 0; i < 6; i++) out[t++] = Jc[i] * r[0] + Jc[6 + i] * r[1];
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) out[t++] = (T[3 * i] * W[3 * j] + T[3 * i + 1] * W[3 * j + 1]) + T[3 * i + 2] * W[3 * j + 2];
    for (int i = 0; i < 6; i++) out[t++] = (W[3 * i] * y[0] + W[3 * i + 1] * y[1]) + W[3 * i + 2] * y[2];
}

// From a camera's kGbaCamSums sums: dl = lambda diag(B), the Cholesky factor Lm (6 x 6) of the Schur diagonal block
// (B + lambda diag(B)) - sum W C^-1 W^T (the identity where it fails), and the reduced right-hand side b.
LOOP_HD void gba_cam_finish(const double* s, double lambda, double* dl, double* Lm, double* b)
{
    double A[36];
    int t = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++, t++) {
            const double bij = i == j ? s[t] + lambda * s[t] : s[t];
            A[6 * i + j] = bij - s[27 + t];
            A[6 * j + i] = A[6 * i + j];
            if (i == j) dl[i] = lambda * s[t];
        }
    if (!gba_chol<6>(A, Lm))
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) Lm[6 * i + j] = i == j ? 1.0 : 0.0;
    for (int i = 0; i < 6; i++) b[i] = (-s[21 + i]) - s[48 + i];
}

// u = J_c p (2 values), each a sum in column order
LOOP_HD void gba_jc_p(const double* Jc, const double* p, double* u)
{
    for (int a = 0; a < 2; a++) {
        double s = Jc[6 * a] * p[0];
        for (int c = 1; c < 6; c++) s = s + Jc[6 * a + c] * p[c];
        u[a] = s;
    }
}

// One point over its list (serial): v = sum J_p^T (J_c vec_k).  mode 0: out = Ci v (the gather of the operator);
// mode 1: out = Ci (g - v) (the back-substitution, vec the camera step).
LOOP_HD void gba_point_gather(const double* lin, size_t nk, const int32_t* list, int cnt, const int32_t* obs_cam, const double* vec,
                              const double* Ci, const double* g, int mode, double* out)
{
    double v[3] = {0.0, 0.0, 0.0};
    for (int q = 0; q < cnt; q++) {
        const size_t o = (size_t)list[q];
        double Jc[12], Jp[6], p[6], u[2];
        gba_load(lin, nk, o, kGbaJc, 12, Jc);
        gba_load(lin, nk, o, kGbaJp, 6, Jp);
        for (int k = 0; k < 6; k++) p[k] = vec[6 * (size_t)obs_cam[o] + k];
        gba_jc_p(Jc, p, u);
        for (int i = 0; i < 3; i++) v[i] = v[i] + (Jp[i] * u[0] + Jp[3 + i] * u[1]);
    }
    if (mode == 1)
        for (int i = 0; i < 3; i++) v[i] = g[i] - v[i];
    gba_mul3(Ci, v, out);
}

// the 6 terms of one observation in S p: J_c^T (J_c p_k - J_p w_p)
LOOP_HD void gba_apply_terms(const double* Jc, const double* Jp, const double* p, const double* w, double* out)
{
    double u[2], e[2];
    gba_jc_p(Jc, p, u);
    for (int a = 0; a < 2; a++) e[a] = u[a] - ((Jp[3 * a] * w[0] + Jp[3 * a + 1] * w[1]) + Jp[3 * a + 2] * w[2]);
    for (int i = 0; i < 6; i++) out[i] = Jc[i] * e[0] + Jc[6 + i] * e[1];
}

// the local step of one camera
LOOP_HD void gba_cam_step(double* cam, const double* d)
{
    const double dq[4] = {1.0, d[0] / 2.0, d[1] / 2.0, d[2] / 2.0};
    double q[4];
    quat_mul(cam, dq, q);
    quat_normalise(q);
    for (int k = 0; k < 4; k++) cam[k] = q[k];
    for (int k = 0; k < 3; k++) cam[4 + k] = cam[4 + k] + d[3 + k];
}

}  // namespace slamhip

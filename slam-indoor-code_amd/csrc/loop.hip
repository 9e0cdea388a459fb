// Loop closing: the Sim(3) constraint of each verified loop by a batched RANSAC, and the
// correction of the map points, gfx950.
//
// The contract is tests/loop_ref.py; the arithmetic shared with the host twin
// (loop_host.cpp) is loop_math.h: + - * / and sqrt in f64, nothing contracted, every
// sum in a stated order, so every result equals the reference bit for bit.
//
//   sim3_hyp     one thread per (loop, hypothesis): the similarity of the sampled triangle
//                pair (Gram-Schmidt frames), all zero when a triangle is degenerate.
//   sim3_score   grid = (64-hypothesis tiles, loops), one wave per workgroup: a lane keeps
//                one hypothesis in registers, the loop's pairs stream once through LDS in
//                64-pair chunks (a, b and the two squared camera distances), every lane
//                reads a pair as an LDS broadcast.  Integer counts, no atomics.
//   sim3_refit   one wave per loop: the winner (most inliers, then the lowest hypothesis),
//                its inlier mask, then kSim3RefitSteps Gauss-Newton steps.  The 35 sums of
//                a step: lane l adds the pairs l, l + 64, ... in ascending order, then the
//                lanes fold as a binary tree in LDS (+32, +16, ... +1); every lane solves
//                the same 7 x 7 system by Cholesky.
//   sim3_apply_points  one thread per map point: X' = S'^-1 (S (X)) of its anchor node.
#include <algorithm>
#include <utility>

#include <vector>

#include "loop_math.h"
#include "pcg_kernels.h"
#include "slamhip_internal.h"

namespace slamhip {

namespace {

__global__ __launch_bounds__(256) void sim3_hyp(const double* a, const double* b, const int32_t* offsets, int L, int H,
                                                const int32_t* samples, double* hyp)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)L * H) return;
    const int l = (int)(i / H);
    const int lo = offsets[l], n = offsets[l + 1] - lo;
    double S[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int s0 = samples[3 * i], s1 = samples[3 * i + 1], s2 = samples[3 * i + 2];
    if (n >= 3 && (unsigned)s0 < (unsigned)n && (unsigned)s1 < (unsigned)n && (unsigned)s2 < (unsigned)n) {
        const double* pa = a + 3 * (size_t)lo;
        const double* pb = b + 3 * (size_t)lo;
        double p[6][3];
        for (int k = 0; k < 3; k++) {
            p[0][k] = pa[3 * (size_t)s0 + k];
            p[1][k] = pa[3 * (size_t)s1 + k];
            p[2][k] = pa[3 * (size_t)s2 + k];
            p[3][k] = pb[3 * (size_t)s0 + k];
            p[4][k] = pb[3 * (size_t)s1 + k];
            p[5][k] = pb[3 * (size_t)s2 + k];
        }
        sim3_hypothesis(p[0], p[1], p[2], p[3], p[4], p[5], S);
    }
    for (int k = 0; k < 8; k++) hyp[8 * i + k] = S[k];
}

constexpr int kScoreTile = 64;      // hypotheses per workgroup = pairs per LDS chunk

__global__ __launch_bounds__(kScoreTile) void sim3_score(const double* a, const double* b, const int32_t* offsets,
                                                         const double* centres, int H, double tau2, const double* hyp,
                                                         int32_t* counts)
{
    __shared__ double pr[kScoreTile][8];        // a (3), b (3), |a - ci|^2, |b - cj|^2
    const int l = blockIdx.y, lane = threadIdx.x;
    const int h = blockIdx.x * kScoreTile + lane;
    const int lo = offsets[l], n = offsets[l + 1] - lo;
    double ci[3], cj[3];
    for (int k = 0; k < 3; k++) {
        ci[k] = centres[6 * (size_t)l + k];
        cj[k] = centres[6 * (size_t)l + 3 + k];
    }
    double S[8] = {0, 0, 0, 0, 0, 0, 0, 0}, R[9];
    if (h < H)
        for (int k = 0; k < 8; k++) S[k] = hyp[8 * ((size_t)l * H + h) + k];
    const bool live = h < H && S[0] > 0.0;
    const double q1[4] = {1.0, 0.0, 0.0, 0.0};
    quat_matrix(live ? S + 1 : q1, R);
    int cnt = 0;
    for (int base = 0; base < n; base += kScoreTile) {
        const int k = base + lane;
        if (k < n) {
            double pa[3], pb[3];
            for (int j = 0; j < 3; j++) {
                pa[j] = a[3 * ((size_t)lo + k) + j];
                pb[j] = b[3 * ((size_t)lo + k) + j];
                pr[lane][j] = pa[j];
                pr[lane][3 + j] = pb[j];
            }
            pr[lane][6] = dist2(pa, ci);
            pr[lane][7] = dist2(pb, cj);
        }
        __syncthreads();
        const int m = min(kScoreTile, n - base);
        if (live)
            for (int r = 0; r < m; r++) cnt += sim3_inlier(S[0], R, S + 5, &pr[r][0], &pr[r][3], pr[r][6], pr[r][7], tau2) ? 1 : 0;
        __syncthreads();
    }
    if (h < H) counts[(size_t)l * H + h] = cnt;
}

__global__ __launch_bounds__(kSim3Lanes) void sim3_refit(const double* a, const double* b, const int32_t* offsets,
                                                         const double* centres, int H, double tau2, const double* hyp,
                                                         const int32_t* counts, double* sim, uint8_t* mask, int32_t* count,
                                                         int32_t* status)
{
    __shared__ double part[kSim3Lanes][kSim3Terms];
    const int l = blockIdx.x, lane = threadIdx.x;
    const int lo = offsets[l], n = offsets[l + 1] - lo;
    const double* pa = a + 3 * (size_t)lo;
    const double* pb = b + 3 * (size_t)lo;
    uint8_t* mk = mask + lo;

    // the winner: most inliers, then the lowest hypothesis
    int bc = -1, bh = 0x7fffffff;
    if (n >= 3)
        for (int h = lane; h < H; h += kSim3Lanes) {
            const int c = counts[(size_t)l * H + h];
            if (c > bc) {       // ascending h per lane: strict keeps the lower
                bc = c;
                bh = h;
            }
        }
    for (int off = 32; off >= 1; off >>= 1) {
        const int oc = __shfl_xor(bc, off, 64), oh = __shfl_xor(bh, off, 64);
        if (oc > bc || (oc == bc && oh < bh)) {
            bc = oc;
            bh = oh;
        }
    }
    double S[8] = {1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (n < 3 || bc < 3) {
        for (int k = lane; k < n; k += kSim3Lanes) mk[k] = 0;
        if (lane == 0) {
            for (int k = 0; k < 8; k++) sim[8 * (size_t)l + k] = S[k];
            count[l] = 0;
            status[l] = n < 3 ? kSim3TooFew : kSim3NoModel;
        }
        return;
    }
    for (int k = 0; k < 8; k++) S[k] = hyp[8 * ((size_t)l * H + bh) + k];
    double ci[3], cj[3], R[9];
    for (int k = 0; k < 3; k++) {
        ci[k] = centres[6 * (size_t)l + k];
        cj[k] = centres[6 * (size_t)l + 3 + k];
    }
    quat_matrix(S + 1, R);
    for (int k = lane; k < n; k += kSim3Lanes) {
        double xa[3], xb[3];
        for (int j = 0; j < 3; j++) {
            xa[j] = pa[3 * (size_t)k + j];
            xb[j] = pb[3 * (size_t)k + j];
        }
        mk[k] = sim3_inlier(S[0], R, S + 5, xa, xb, dist2(xa, ci), dist2(xb, cj), tau2) ? 1 : 0;
    }
    // a lane reads back only the mask bytes it wrote itself (k = lane mod 64)
    int st = kSim3Ok;
    for (int it = 0; it < kSim3RefitSteps; it++) {
        double acc[kSim3Terms];
        for (int j = 0; j < kSim3Terms; j++) acc[j] = 0.0;
        quat_matrix(S + 1, R);
        for (int k = lane; k < n; k += kSim3Lanes) {
            double xa[3], xb[3], term[kSim3Terms];
            for (int j = 0; j < 3; j++) {
                xa[j] = pa[3 * (size_t)k + j];
                xb[j] = pb[3 * (size_t)k + j];
            }
            sim3_terms(S[0], R, S + 5, xa, xb, term);
            const bool in = mk[k] != 0;
            for (int j = 0; j < kSim3Terms; j++) acc[j] = acc[j] + (in ? term[j] : 0.0);
        }
        __syncthreads();        // the previous step's reads of part[0] are done
        for (int j = 0; j < kSim3Terms; j++) part[lane][j] = acc[j];
        __syncthreads();
        for (int off = kSim3Lanes / 2; off >= 1; off >>= 1) {
            if (lane < off)
                for (int j = 0; j < kSim3Terms; j++) part[lane][j] = part[lane][j] + part[lane + off][j];
            __syncthreads();
        }
        double sum[kSim3Terms], d[7];
        for (int j = 0; j < kSim3Terms; j++) sum[j] = part[0][j];
        if (!chol7_solve(sum, sum + 28, d)) {       // uniform: every lane has the same sums
            st = kSim3Cholesky;
            break;
        }
        sim3_step(S, d);
    }
    if (lane == 0) {
        for (int k = 0; k < 8; k++) sim[8 * (size_t)l + k] = S[k];
        count[l] = bc;
        status[l] = st;
    }
}

__global__ __launch_bounds__(256) void sim3_apply_points(const double* pts, const int32_t* anchor, int n, const double* nodes,
                                                         const double* nodes_new, int m, double* out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int an = anchor[i];
    double X[3], Y[3];
    for (int k = 0; k < 3; k++) X[k] = pts[3 * (size_t)i + k];
    if ((unsigned)an < (unsigned)m) {
        double S[8], Sn[8];
        for (int k = 0; k < 8; k++) {
            S[k] = nodes[8 * (size_t)an + k];
            Sn[k] = nodes_new[8 * (size_t)an + k];
        }
        sim3_move_point(S, Sn, X, Y);
    } else {
        for (int k = 0; k < 3; k++) Y[k] = X[k];
    }
    for (int k = 0; k < 3; k++) out[3 * (size_t)i + k] = Y[k];
}

// ---- the pose graph over Sim(3): LM with a block-Jacobi PCG whose loop stays on the stream ----
//   pgo_linearize  one thread per edge: residual, both Jacobians, |r|^2
//   pgo_assemble   one thread per (node, row): the row of H_aa and g_a over the node's incident list in order
//   pgo_damp       one thread per node: Hd = H + lambda diag(H) and its Cholesky factor
//   pgo_edge_mul   one thread per (edge, side): u = J p
//   pgo_apply      one thread per (node, row): Hd_aa p_a + sum J_a^T u_b over the same list
//   pgo_reduce     (pcg_kernels.h, shared with gba.hip) one workgroup of 1024: the 1024 strided partial sums, the binary tree in LDS, and the
//                  scalar work of its step (cost; rz0 and the start flag; alpha; beta, the count and the
//                  stop flag).  Once the stop flag is set every kernel of the loop returns at once.
__global__ __launch_bounds__(64) void pgo_linearize(const double* S, const int32_t* edges, const double* zinv,
                                                    const double* sw, int E, double ell, double* r, double* J, double* c)
{
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    const int i = edges[2 * (size_t)e], j = edges[2 * (size_t)e + 1];
    double Si[8], Sj[8], A[8], rr[7], Ji[49], Jj[49];
    for (int k = 0; k < 8; k++) {
        Si[k] = S[8 * (size_t)i + k];
        Sj[k] = S[8 * (size_t)j + k];
        A[k] = zinv[8 * (size_t)e + k];
    }
    pgo_edge(Si, Sj, A, sw[e], ell, i == 0, j == 0, rr, Ji, Jj);
    for (int k = 0; k < 7; k++) r[7 * (size_t)e + k] = rr[k];
    for (int k = 0; k < 49; k++) {
        J[98 * (size_t)e + k] = Ji[k];
        J[98 * (size_t)e + 49 + k] = Jj[k];
    }
    c[e] = pgo_edge_cost(rr);
}

__global__ __launch_bounds__(256) void pgo_assemble(const double* r, const double* J, const int32_t* start, const int32_t* ent,
                                                    int n, double* H, double* g)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 7 * n) return;
    const int a = i / 7, row = i - 7 * a;
    double h[7] = {0, 0, 0, 0, 0, 0, 0}, gs = 0.0;
    for (int q = start[a]; q < start[a + 1]; q++) {
        const int en = ent[q];
        double hb[7], gb;
        pgo_block_row(J + 49 * (size_t)en, r + 7 * (size_t)(en >> 1), row, hb, &gb);
        for (int k = 0; k < 7; k++) h[k] = h[k] + hb[k];
        gs = gs - gb;
    }
    for (int k = 0; k < 7; k++) H[49 * (size_t)a + 7 * row + k] = h[k];
    g[i] = gs;
}

__global__ __launch_bounds__(64) void pgo_damp(const double* H, double lambda, int n, double* Hd, double* Lm)
{
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= n) return;
    double h[49], hd[49], l[49];
    for (int k = 0; k < 49; k++) h[k] = H[49 * (size_t)a + k];
    pgo_damp_block(h, lambda, a == 0, hd, l);
    for (int k = 0; k < 49; k++) {
        Hd[49 * (size_t)a + k] = hd[k];
        Lm[49 * (size_t)a + k] = l[k];
    }
}

__global__ __launch_bounds__(64) void pgo_pcg_init(const double* g, const double* Lm, int n, double* x, double* r, double* z,
                                                   double* p)
{
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= n) return;
    double rr[7], zz[7];
    for (int k = 0; k < 7; k++) rr[k] = g[7 * (size_t)a + k];
    pgo_block_solve(Lm + 49 * (size_t)a, rr, zz);
    for (int k = 0; k < 7; k++) {
        x[7 * (size_t)a + k] = 0.0;
        r[7 * (size_t)a + k] = rr[k];
        z[7 * (size_t)a + k] = zz[k];
        p[7 * (size_t)a + k] = zz[k];
    }
}

__global__ __launch_bounds__(256) void pgo_edge_mul(const double* J, const int32_t* edges, int E2, const double* p, double* u,
                                                    const PgoSc* sc)
{
    if (sc->done) return;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= E2) return;
    double pp[7], uu[7];
    const int node = edges[q];
    for (int k = 0; k < 7; k++) pp[k] = p[7 * (size_t)node + k];
    pgo_jp(J + 49 * (size_t)q, pp, uu);
    for (int k = 0; k < 7; k++) u[7 * (size_t)q + k] = uu[k];
}

__global__ __launch_bounds__(256) void pgo_apply(const double* J, const double* Hd, const int32_t* start, const int32_t* ent, int n,
                                                 const double* p, const double* u, double* Ap, const PgoSc* sc)
{
    if (sc->done) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 7 * n) return;
    const int a = i / 7, row = i - 7 * a;
    const double* hd = Hd + 49 * (size_t)a + 7 * row;
    const double* pa = p + 7 * (size_t)a;
    double y = hd[0] * pa[0];
    for (int k = 1; k < 7; k++) y = y + hd[k] * pa[k];
    for (int q = start[a]; q < start[a + 1]; q++) {
        const int en = ent[q];
        y = y + pgo_jtu(J + 49 * (size_t)en, u + 7 * (size_t)(en ^ 1), row);
    }
    Ap[i] = y;
}

__global__ __launch_bounds__(64) void pgo_update(const double* Lm, int n, const double* p, const double* Ap, double* x, double* r,
                                                 double* z, const PgoSc* sc)
{
    if (sc->done) return;
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= n) return;
    const double alpha = sc->alpha;
    double rr[7], zz[7];
    for (int k = 0; k < 7; k++) {
        const size_t i = 7 * (size_t)a + k;
        x[i] = x[i] + alpha * p[i];
        rr[k] = r[i] - alpha * Ap[i];
        r[i] = rr[k];
    }
    pgo_block_solve(Lm + 49 * (size_t)a, rr, zz);
    for (int k = 0; k < 7; k++) z[7 * (size_t)a + k] = zz[k];
}

__global__ __launch_bounds__(256) void pgo_step(const double* S, const double* x, int n, double* St)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    double s[8], d[7];
    for (int k = 0; k < 8; k++) s[k] = S[8 * (size_t)a + k];
    for (int k = 0; k < 7; k++) d[k] = x[7 * (size_t)a + k];
    if (a > 0) sim3_step(s, d);
    for (int k = 0; k < 8; k++) St[8 * (size_t)a + k] = s[k];
}

}  // namespace

}  // namespace slamhip

using namespace slamhip;

extern "C" int slam_sim3_ransac_dev(slam_ctx* c, void* stream, const double* d_a, const double* d_b, const int32_t* offsets,
                                    int L, const double* centres, int H, double tau, uint64_t seed, double* d_sim,
                                    uint8_t* d_mask, int32_t* d_count, int32_t* d_status)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (loop_check_ransac(offsets, L, centres, H, tau))
        return set_err(c, SLAM_E_INVALID_ARG, "sim3 ransac: 0 <= L <= 65535, 1 <= H <= 65536, tau > 0, offsets ascending "
                                              "from >= 0 with at most 2^24 pairs per loop");
    if (L == 0) return SLAM_OK;
    const int np = offsets[L] - offsets[0];
    if (!d_sim || !d_count || !d_status || (np > 0 && (!d_a || !d_b || !d_mask)))
        return set_err(c, SLAM_E_INVALID_ARG, "sim3 ransac: null argument");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    const size_t LH = (size_t)L * H;
    std::vector<int32_t> samples(3 * LH);
    loop_draw_samples(offsets, L, H, seed, samples.data());
    DevLayout lay;
    const auto s_hyp = lay.add<double>(8 * LH), s_cen = lay.add<double>(6 * (size_t)L);
    const auto s_smp = lay.add<int32_t>(3 * LH), s_cnt = lay.add<int32_t>(LH), s_off = lay.add<int32_t>((size_t)L + 1);
    DevMem w;
    SLAM_HIP(c, w.bind(c->loop_ws, lay));
    double *hyp = w.ptr(s_hyp), *cen = w.ptr(s_cen);
    int32_t *smp = w.ptr(s_smp), *cnt = w.ptr(s_cnt), *off = w.ptr(s_off);
    SLAM_HIP(c, w.upload(s_cen, centres, s));
    SLAM_HIP(c, w.upload(s_smp, samples.data(), s));
    SLAM_HIP(c, w.upload(s_off, offsets, s));
    const double tau2 = tau * tau;
    hipLaunchKernelGGL(sim3_hyp, dim3((unsigned)((LH + 255) / 256)), dim3(256), 0, s, d_a, d_b, off, L, H, smp, hyp);
    hipLaunchKernelGGL(sim3_score, dim3((H + kScoreTile - 1) / kScoreTile, L), dim3(kScoreTile), 0, s, d_a, d_b, off, cen, H,
                       tau2, hyp, cnt);
    hipLaunchKernelGGL(sim3_refit, dim3(L), dim3(kSim3Lanes), 0, s, d_a, d_b, off, cen, H, tau2, hyp, cnt, d_sim, d_mask,
                       d_count, d_status);
    SLAM_HIP(c, hipGetLastError());
    return stream_sync(c, s);       // the sample table lives until here
}

extern "C" int slam_sim3_apply_points_dev(slam_ctx* c, void* stream, const double* d_points, const int32_t* d_anchor, int n,
                                          const double* nodes, const double* nodes_new, int m, double* d_out)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (n < 0 || loop_check_nodes(nodes, m) || loop_check_nodes(nodes_new, m))
        return set_err(c, SLAM_E_INVALID_ARG, "sim3 apply points: n, m >= 0, every node with sigma > 0 and a non-zero quaternion");
    if (n == 0) return SLAM_OK;
    if (!d_points || !d_anchor || !d_out) return set_err(c, SLAM_E_INVALID_ARG, "sim3 apply points: null argument");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    DevLayout lay;
    const auto s_old = lay.add<double>(8 * (size_t)m), s_new = lay.add<double>(8 * (size_t)m);
    DevMem w;
    SLAM_HIP(c, w.bind(c->loop_ws, lay));
    if (m > 0) {
        SLAM_HIP(c, w.upload(s_old, nodes, s));
        SLAM_HIP(c, w.upload(s_new, nodes_new, s));
    }
    hipLaunchKernelGGL(sim3_apply_points, dim3((n + 255) / 256), dim3(256), 0, s, d_points, d_anchor, n, w.ptr(s_old), w.ptr(s_new),
                       m, d_out);
    SLAM_HIP(c, hipGetLastError());
    return stream_sync(c, s);
}

extern "C" int slam_pgo_sim3_dev(slam_ctx* c, void* stream, double* d_nodes, int n, const int32_t* edges, const double* meas,
                                 const double* weight, int E, double ell, double lambda0, int max_lm, int max_pcg,
                                 double pcg_tol, double cost_tol, double* cost, int32_t* iters)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (n < 1 || n > kSim3MaxPairs || !d_nodes || !cost || !iters)
        return set_err(c, SLAM_E_INVALID_ARG, "pgo sim3: null argument or no node");
    SLAM_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    std::vector<double> h_nodes(8 * (size_t)n);
    SLAM_HIP(c, hipMemcpyAsync(h_nodes.data(), d_nodes, 8 * 8 * (size_t)n, hipMemcpyDeviceToHost, s));
    if (int rc = stream_sync(c, s)) return rc;
    if (loop_check_pgo(h_nodes.data(), n, edges, meas, weight, E, ell, lambda0, max_lm, max_pcg, pcg_tol, cost_tol))
        return set_err(c, SLAM_E_INVALID_ARG, "pgo sim3: every node and measurement with sigma > 0 and a non-zero quaternion, "
                                              "edges i != j inside [0, n) that reach every node, weights >= 0, ell > 0, "
                                              "lambda0, caps and tolerances >= 0");
    std::vector<int32_t> start, ent;
    pgo_build_csr(n, edges, E, start, ent);
    std::vector<double> zs(9 * (size_t)E);
    pgo_edge_constants(meas, weight, E, zs.data(), zs.data() + 8 * (size_t)E);
    const size_t N = 7 * (size_t)n, nE = (size_t)E;
    // a linearisation is r (7 E), J (98 E), c (E); zinv (8 E) and sw (E) share a slot, as the host's zs holds them
    const size_t lin = 7 * nE + 98 * nE + nE;
    DevLayout lay;
    const auto s_S = lay.add<double>(8 * (size_t)n), s_St = lay.add<double>(8 * (size_t)n), s_zs = lay.add<double>(9 * nE);
    const auto s_linA = lay.add<double>(lin), s_linB = lay.add<double>(lin);
    const auto s_H = lay.add<double>(49 * (size_t)n), s_Hd = lay.add<double>(49 * (size_t)n), s_Lm = lay.add<double>(49 * (size_t)n);
    const auto s_g = lay.add<double>(N), s_x = lay.add<double>(N), s_r = lay.add<double>(N), s_z = lay.add<double>(N);
    const auto s_p = lay.add<double>(N), s_Ap = lay.add<double>(N), s_u = lay.add<double>(14 * nE);
    const auto s_sc = lay.add<PgoSc>(1);
    const auto s_edges = lay.add<int32_t>(2 * nE), s_start = lay.add<int32_t>((size_t)n + 1), s_ent = lay.add<int32_t>(2 * nE);
    DevMem w;
    SLAM_HIP(c, w.bind(c->loop_pgo, lay));
    double *S = w.ptr(s_S), *St = w.ptr(s_St), *zinv = w.ptr(s_zs), *sw = zinv + 8 * nE, *linA = w.ptr(s_linA), *linB = w.ptr(s_linB);
    double *H = w.ptr(s_H), *Hd = w.ptr(s_Hd), *Lm = w.ptr(s_Lm), *g = w.ptr(s_g);
    double *x = w.ptr(s_x), *r = w.ptr(s_r), *z = w.ptr(s_z), *p = w.ptr(s_p), *Ap = w.ptr(s_Ap), *u = w.ptr(s_u);
    PgoSc* sc = w.ptr(s_sc);
    int32_t *d_edges = w.ptr(s_edges), *d_start = w.ptr(s_start), *d_ent = w.ptr(s_ent);
    PgoSc* h_sc = static_cast<PgoSc*>(readback(c, sizeof(PgoSc)));
    if (!h_sc) return set_err(c, SLAM_E_HIP, "pgo sim3: no pinned readback space");

    SLAM_HIP(c, hipMemcpyAsync(S, d_nodes, 8 * 8 * (size_t)n, hipMemcpyDeviceToDevice, s));
    if (E > 0) {
        SLAM_HIP(c, w.upload(s_zs, zs.data(), s));
        SLAM_HIP(c, w.upload(s_edges, edges, s));
        SLAM_HIP(c, w.upload(s_ent, ent.data(), s));
    }
    SLAM_HIP(c, w.upload(s_start, start.data(), s));
    PgoSc init = {};
    init.tol = pcg_tol;
    SLAM_HIP(c, w.upload(s_sc, &init, s));
    if (int rc = stream_sync(c, s)) return rc;      // the host vectors and `init` are free from here

    const unsigned gE = (unsigned)((E + 63) / 64), gN7 = (unsigned)((N + 255) / 256), gN = (unsigned)((n + 63) / 64);
    auto linearize = [&](const double* nodes, double* L, double* out) -> int {
        if (E > 0) hipLaunchKernelGGL(pgo_linearize, dim3(gE), dim3(64), 0, s, nodes, d_edges, zinv, sw, E, ell, L, L + 7 * nE, L + 105 * nE);
        hipLaunchKernelGGL(pgo_reduce, dim3(1), dim3(kPgoLanes), 0, s, L + 105 * nE, (const double*)nullptr, nE, sc, 0);
        SLAM_HIP(c, hipGetLastError());
        SLAM_HIP(c, hipMemcpyAsync(h_sc, sc, sizeof(PgoSc), hipMemcpyDeviceToHost, s));
        if (int rc = stream_sync(c, s, true)) return rc;
        *out = h_sc->cost;
        return SLAM_OK;
    };
    double c0 = 0.0;
    if (int rc = linearize(S, linA, &c0)) return rc;
    double cur = c0, lambda = lambda0;
    int lm = 0, accepted = 0, pcg_total = 0;
    while (lm < max_lm && cur > 0.0) {
        const double *rA = linA, *JA = linA + 7 * nE;
        hipLaunchKernelGGL(pgo_assemble, dim3(gN7), dim3(256), 0, s, rA, JA, d_start, d_ent, n, H, g);
        hipLaunchKernelGGL(pgo_damp, dim3(gN), dim3(64), 0, s, H, lambda, n, Hd, Lm);
        hipLaunchKernelGGL(pgo_pcg_init, dim3(gN), dim3(64), 0, s, g, Lm, n, x, r, z, p);
        hipLaunchKernelGGL(pgo_reduce, dim3(1), dim3(kPgoLanes), 0, s, r, z, N, sc, 1);
        SLAM_HIP(c, hipGetLastError());
        int launched = 0;
        for (;;) {
            const int chunk = std::min(kPgoChunk, max_pcg - launched);
            for (int k = 0; k < chunk; k++) {
                if (E > 0) hipLaunchKernelGGL(pgo_edge_mul, dim3((unsigned)((2 * nE + 255) / 256)), dim3(256), 0, s, JA, d_edges, 2 * E, p, u, sc);
                hipLaunchKernelGGL(pgo_apply, dim3(gN7), dim3(256), 0, s, JA, Hd, d_start, d_ent, n, p, u, Ap, sc);
                hipLaunchKernelGGL(pgo_reduce, dim3(1), dim3(kPgoLanes), 0, s, p, Ap, N, sc, 2);
                hipLaunchKernelGGL(pgo_update, dim3(gN), dim3(64), 0, s, Lm, n, p, Ap, x, r, z, sc);
                hipLaunchKernelGGL(pgo_reduce, dim3(1), dim3(kPgoLanes), 0, s, r, z, N, sc, 3);
                hipLaunchKernelGGL(pgo_pupdate, dim3(gN7), dim3(256), 0, s, (int)N, z, p, sc);
            }
            launched += chunk;
            SLAM_HIP(c, hipGetLastError());
            SLAM_HIP(c, hipMemcpyAsync(h_sc, sc, sizeof(PgoSc), hipMemcpyDeviceToHost, s));
            if (int rc = stream_sync(c, s, true)) return rc;
            if (h_sc->done || launched >= max_pcg) break;
        }
        pcg_total += h_sc->iters;
        hipLaunchKernelGGL(pgo_step, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, S, x, n, St);
        double ct = 0.0;
        if (int rc = linearize(St, linB, &ct)) return rc;
        lm++;
        if (ct < cur) {
            const double rel = (cur - ct) / cur;
            std::swap(S, St);
            std::swap(linA, linB);
            cur = ct;
            accepted++;
            lambda = lambda / 10.0;
            if (rel < cost_tol) break;
        } else {
            lambda = lambda * 10.0;
        }
    }
    SLAM_HIP(c, hipMemcpyAsync(d_nodes, S, 8 * 8 * (size_t)n, hipMemcpyDeviceToDevice, s));
    cost[0] = c0;
    cost[1] = cur;
    iters[0] = lm;
    iters[1] = accepted;
    iters[2] = pcg_total;
    return stream_sync(c, s);
}

extern "C" int slam_pgo_sim3(slam_ctx* c, double* nodes, int n, const int32_t* edges, const double* meas, const double* weight,
                             int E, double ell, double lambda0, int max_lm, int max_pcg, double pcg_tol, double cost_tol,
                             double* cost, int32_t* iters)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (loop_check_pgo(nodes, n, edges, meas, weight, E, ell, lambda0, max_lm, max_pcg, pcg_tol, cost_tol) || !cost || !iters)
        return set_err(c, SLAM_E_INVALID_ARG, "pgo sim3: bad arguments");
    SLAM_HIP(c, hipSetDevice(c->device));
    DevLayout lay;
    const auto s_nodes = lay.add<double>(8 * (size_t)n);
    DevMem d;
    SLAM_HIP(c, d.bind(c->loop_in, lay));
    SLAM_HIP(c, d.upload(s_nodes, nodes, c->stream));
    if (int rc = slam_pgo_sim3_dev(c, c->stream, d.ptr(s_nodes), n, edges, meas, weight, E, ell, lambda0, max_lm, max_pcg, pcg_tol,
                                   cost_tol, cost, iters))
        return rc;
    SLAM_HIP(c, d.download(nodes, s_nodes, c->stream));
    return stream_sync(c, c->stream);
}

// ---- host-buffer wrappers: stage, run the device entry points, copy back ----

extern "C" int slam_sim3_ransac(slam_ctx* c, const double* a, const double* b, const int32_t* offsets, int L,
                                const double* centres, int H, double tau, uint64_t seed, double* sim, uint8_t* mask,
                                int32_t* count, int32_t* status)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (loop_check_ransac(offsets, L, centres, H, tau)) return set_err(c, SLAM_E_INVALID_ARG, "sim3 ransac: bad arguments");
    if (L == 0) return SLAM_OK;
    const int32_t p0 = offsets[0], np = offsets[L] - offsets[0];
    if (!sim || !count || !status || (np > 0 && (!a || !b || !mask))) return set_err(c, SLAM_E_INVALID_ARG, "sim3 ransac: null argument");
    SLAM_HIP(c, hipSetDevice(c->device));
    std::vector<int32_t> off((size_t)L + 1);
    for (int i = 0; i <= L; i++) off[i] = offsets[i] - p0;
    DevLayout lay;
    const auto s_a = lay.add<double>(3 * (size_t)np), s_b = lay.add<double>(3 * (size_t)np);
    const auto s_sim = lay.add<double>(8 * (size_t)L);
    const auto s_cnt = lay.add<int32_t>((size_t)L), s_st = lay.add<int32_t>((size_t)L);
    const auto s_mask = lay.add<uint8_t>((size_t)np);
    DevMem d;
    SLAM_HIP(c, d.bind(c->loop_in, lay));
    hipStream_t s = c->stream;
    if (np > 0) {
        SLAM_HIP(c, d.upload(s_a, a + 3 * (size_t)p0, s));
        SLAM_HIP(c, d.upload(s_b, b + 3 * (size_t)p0, s));
    }
    if (int rc = slam_sim3_ransac_dev(c, s, d.ptr(s_a), d.ptr(s_b), off.data(), L, centres, H, tau, seed, d.ptr(s_sim), d.ptr(s_mask),
                                      d.ptr(s_cnt), d.ptr(s_st)))
        return rc;
    SLAM_HIP(c, d.download(sim, s_sim, s));
    SLAM_HIP(c, d.download(count, s_cnt, s));
    SLAM_HIP(c, d.download(status, s_st, s));
    if (np > 0) SLAM_HIP(c, d.download(mask + p0, s_mask, s));
    return stream_sync(c, s);
}

extern "C" int slam_sim3_apply_points(slam_ctx* c, const double* points, const int32_t* anchor, int n, const double* nodes,
                                      const double* nodes_new, int m, double* out)
{
    if (!c) return SLAM_E_INVALID_ARG;
    if (n < 0 || loop_check_nodes(nodes, m) || loop_check_nodes(nodes_new, m))
        return set_err(c, SLAM_E_INVALID_ARG, "sim3 apply points: bad arguments");
    if (n == 0) return SLAM_OK;
    if (!points || !anchor || !out) return set_err(c, SLAM_E_INVALID_ARG, "sim3 apply points: null argument");
    for (int i = 0; i < n; i++)
        if (anchor[i] < -1 || anchor[i] >= m) return set_err(c, SLAM_E_INVALID_ARG, "sim3 apply points: anchor outside [-1, m)");
    SLAM_HIP(c, hipSetDevice(c->device));
    DevLayout lay;
    const auto s_pts = lay.add<double>(3 * (size_t)n), s_out = lay.add<double>(3 * (size_t)n);
    const auto s_an = lay.add<int32_t>((size_t)n);
    DevMem d;
    SLAM_HIP(c, d.bind(c->loop_in, lay));
    hipStream_t s = c->stream;
    SLAM_HIP(c, d.upload(s_pts, points, s));
    SLAM_HIP(c, d.upload(s_an, anchor, s));
    if (int rc = slam_sim3_apply_points_dev(c, s, d.ptr(s_pts), d.ptr(s_an), n, nodes, nodes_new, m, d.ptr(s_out))) return rc;
    SLAM_HIP(c, d.download(out, s_out, s));
    return stream_sync(c, s);
}

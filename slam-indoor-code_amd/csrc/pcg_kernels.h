// The conjugate-gradient kernels that the on-stream solvers share (loop.hip's pose graph, gba.hip's Schur
// complement): the scalars in device memory, the 1024-lane reduction that also does the scalar work of its
// step, and the update of the search direction.  Included by each .hip file into its own unnamed namespace.
#pragma once

#include <hip/hip_runtime.h>

#include "loop_math.h"

namespace slamhip {

namespace {

struct PgoSc {
    double rz, rz0, alpha, beta, cost, tol;
    int done, iters;
};

__global__ __launch_bounds__(kPgoLanes) void pgo_reduce(const double* a, const double* b, size_t n, PgoSc* sc, int mode)
{
    __shared__ double part[kPgoLanes];
    if (mode >= 2 && sc->done) return;      // uniform
    const int t = threadIdx.x;
    double acc = 0.0;
    for (size_t i = t; i < n; i += kPgoLanes) acc = acc + (b ? a[i] * b[i] : a[i]);
    part[t] = acc;
    __syncthreads();
    for (int off = kPgoLanes / 2; off >= 1; off >>= 1) {
        if (t < off) part[t] = part[t] + part[t + off];
        __syncthreads();
    }
    if (t != 0) return;
    const double sum = part[0];
    if (mode == 0) {
        sc->cost = sum;
    } else if (mode == 1) {
        sc->rz = sum;
        sc->rz0 = sum;
        sc->done = sum > 0.0 ? 0 : 1;
        sc->iters = 0;
    } else if (mode == 2) {
        if (!(sum > 0.0))
            sc->done = 1;
        else
            sc->alpha = sc->rz / sum;
    } else {
        sc->iters = sc->iters + 1;
        if (sum <= sc->tol * sc->rz0)
            sc->done = 1;
        else
            sc->beta = sum / sc->rz;
        sc->rz = sum;
    }
}

__global__ __launch_bounds__(256) void pgo_pupdate(int N, const double* z, double* p, const PgoSc* sc)
{
    if (sc->done) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    p[i] = z[i] + sc->beta * p[i];
}

}  // namespace

}  // namespace slamhip

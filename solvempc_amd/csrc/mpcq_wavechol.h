// solvempc_amd/csrc/mpcq_wavechol.h — dense fp64 helpers of the one-QP-per-wave post-passes (mpcq_polish.hip,
// mpcq_sens.hip): a Cholesky factorisation in LDS with lane i owning row i, the two triangular solves with the
// vector kept in registers, and the wave-wide NaN-propagating max.  Internal linkage: each translation unit
// compiles its own copy.
#ifndef MPCQ_WAVECHOL_H
#define MPCQ_WAVECHOL_H

#include <hip/hip_runtime.h>

namespace mpcq {

namespace {

__device__ __forceinline__ double nan_max(double a, double b) { return (a > b || a != a) ? a : b; }

// max over the wave's 64 lanes, a NaN anywhere giving NaN
__device__ __forceinline__ double wave_nan_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o));
    return v;
}

// In-place lower Cholesky M = L L' of the leading N x N block (stride ld; N <= 64, lane i owns row i), left
// looking: column k = (M(:, k) - L(:, 0:k) L(k, 0:k)') / L(k, k).  dinv[k] = 1 / L(k, k).  False when a
// pivot is not positive.
__device__ bool wave_cholesky(double *M, int ld, int N, double *dinv, int lane)
{
    bool ok = true;
    for (int k = 0; k < N; k++) {
        double v = 0.0;
        if (lane >= k && lane < N) {
            v = M[lane * ld + k];
            for (int j = 0; j < k; j++) v -= M[lane * ld + j] * M[k * ld + j];
        }
        const double d = __shfl(v, k);
        if (!(d > 0.0)) {  // (wave-uniform)
            ok = false;
            break;
        }
        const double lkk = sqrt(d), inv = 1.0 / lkk;
        if (lane >= k && lane < N) M[lane * ld + k] = lane == k ? lkk : v * inv;
        if (lane == k) dinv[k] = inv;
        __syncthreads();
    }
    __syncthreads();
    return ok;
}

// r <- (L L')^-1 r for the factor above; lane i holds r_i (lanes >= N: unused)
__device__ __forceinline__ double wave_chol_solve(const double *M, int ld, int N, const double *dinv, double r, int lane)
{
    for (int k = 0; k < N; k++) {  // L y = r
        const double yk = __shfl(r, k) * dinv[k];
        if (lane == k) r = yk;
        else if (lane > k && lane < N) r -= M[lane * ld + k] * yk;
    }
    for (int k = N - 1; k >= 0; k--) {  // L' x = y
        const double xk = __shfl(r, k) * dinv[k];
        if (lane == k) r = xk;
        else if (lane < k) r -= M[k * ld + lane] * xk;
    }
    return r;
}

}  // namespace

}  // namespace mpcq
#endif  // MPCQ_WAVECHOL_H

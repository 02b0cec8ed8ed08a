// solvempc_amd/csrc/mpcq_condense_vjp.hip — the reverse of the condensing (mpcq_condense.hip): cotangents of the
// condensed operators P, A, Fx, Fu, Fr, Sbar, Ku -> cotangents of the plant data Ad, Bd, Cd, K, Q, R, RD
// (include/mpcq.h, mpcq_condense_vjp*).
//
// With r_k = Cd Ad^k (k = 0..N), c_k = r_k Bd, cum_d = c_0 + .. + c_d, S(i,j) = cum_(i-j) for j <= i (else 0),
// Sx(i) = r_(i+1), L the lower-triangular ones, the forward pass is
//   P = 2 (R L'L + RD I + Q S'S)     Fu = 2 (R 1 + Q S'S(:,0))     Fr = -2 Q S'     Fx = 2 Q S'Sx
//   A = [K0 L; -K0 L]                Sbar(i) = K, Sbar(N+i) = -K (i < s_rows)       Ku = [-K0 1; K0 1]
// and the reverse pass below follows the header's contract line by line.  One wavefront per plant, everything in
// LDS, fp64, no atomics; sums run in a fixed order (per-lane partial sums in ascending element index, then a
// butterfly over the 64 lanes), so two calls give identical bits.  Nothing is kept from a forward call: r_k, S and
// Sx are recomputed (r_k by the recursion r_k = r_(k-1) Ad).  The one O(N^3) term is the lower triangle of S Ps.
#include "mpcq_internal.h"

namespace mpcq {

// Sum over the wavefront's 64 lanes, the same bits in every lane (a + b == b + a at every butterfly stage).
__device__ inline double vjp_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(64) void condense_vjp_kernel(CondenseVjpArgs a)
{
    // LDS carved to the call's N and nx (condense_vjp_lds doubles: 10 KiB at N = 20, nx = 4, 25 KiB at N = 32,
    // nx = 8), so that a CU holds as many plants as its wave slots allow.  S itself is not stored: S(i,j) = cum[i-j].
    extern __shared__ double lds[];
    const int N = a.N, nx = a.nx, LD = N | 1;
    double *sAd = lds, *sBd = sAd + nx * nx, *r = sBd + nx, *rho = r + (N + 1) * nx, *cum = rho + (N + 1) * nx;
    double *Gc = cum + N, *sFu = Gc + N, *sFx = sFu + N, *GSx = sFx + N * nx, *Ps = GSx + N * nx, *GS = Ps + N * LD;
    const int p = blockIdx.x;
    if (p >= a.n_plants) return;
    const int t = threadIdx.x;
    const size_t P = (size_t)p;
    const double *Ad = a.Ad + P * nx * nx, *Bd = a.Bd + P * nx, *Cd = a.Cd + P * nx;
    const double Q = a.Q[p];
    const double *gP = a.gP ? a.gP + P * N * N : nullptr, *gA = a.gA ? a.gA + P * 2 * N * N : nullptr;
    const double *gFx = a.gFx ? a.gFx + P * N * nx : nullptr, *gFu = a.gFu ? a.gFu + P * N : nullptr;
    const double *gFr = a.gFr ? a.gFr + P * N * N : nullptr, *gSbar = a.gSbar ? a.gSbar + P * 2 * N * nx : nullptr;
    const double *gKu = a.gKu ? a.gKu + P * 2 * N : nullptr;

    // the plant, r_0 = Cd and the cotangents that are read more than once
    if (t < nx * nx) sAd[t] = Ad[t];
    if (t < nx) {
        sBd[t] = Bd[t];
        r[t] = Cd[t];
    }
    if (t < N) sFu[t] = gFu ? gFu[t] : 0.0;
    for (int e = t; e < N * nx; e += 64) sFx[e] = gFx ? gFx[e] : 0.0;
    for (int e = t; e < N * N; e += 64) {
        const int i = e / N, j = e % N;
        Ps[i * LD + j] = gP ? gP[i * N + j] + gP[j * N + i] : 0.0;
    }
    __syncthreads();
    // r_k = r_(k-1) Ad
    for (int k = 1; k <= N; k++) {
        if (t < nx) {
            double v = 0.0;
            for (int j = 0; j < nx; j++) v += r[(k - 1) * nx + j] * sAd[j * nx + t];
            r[k * nx + t] = v;
        }
        __syncthreads();
    }
    // c_k = r_k Bd, cum its running sum (the sequential sum of condense_wave_kernel): S(i,j) = cum[i-j]
    if (t < N) {
        double v = 0.0;
        for (int j = 0; j < nx; j++) v += r[t * nx + j] * sBd[j];
        cum[t] = v;
    }
    __syncthreads();
    if (t == 0) {
        double v = 0.0;
        for (int k = 0; k < N; k++) { v += cum[k]; cum[k] = v; }
    }
    __syncthreads();

    // The lower triangle of  E = S Ps + 2 (S(:,0) gFu' - gFr' + Sx gFx'):  gQ = <S, E>, and
    // GS = 2Q (S Ps + S(:,0) gFu' - gFr' + Sx gFx'); gR's <Ps, L'L> and gRD = tr Ps ride along.
    const double tq = 2.0 * Q;
    double accQ = 0.0, accR = 0.0, accRD = 0.0, accA = 0.0;
    for (int e = t; e < N * N; e += 64) {
        const int i = e / N, j = e % N;
        accR += Ps[i * LD + j] * (double)(N - (i > j ? i : j));  // (L'L)(i,j) = N - max(i,j)
        if (i == j) accRD += Ps[i * LD + i];
        if (j > i) continue;
        if (gA) accA += gA[i * N + j] - gA[(N + i) * N + j];
        double m = 0.0;
        for (int k = 0; k <= i; k++) m += cum[i - k] * Ps[k * LD + j];
        double rest = cum[i] * sFu[j] - (gFr ? gFr[j * N + i] : 0.0);
        double sx = 0.0;
        for (int c = 0; c < nx; c++) sx += r[(i + 1) * nx + c] * sFx[j * nx + c];
        rest += sx;
        GS[i * LD + j] = tq * (m + rest);
        accQ += cum[i - j] * (m + 2.0 * rest);
    }
    __syncthreads();
    // GS(:,0) += 2Q S gFu
    if (t < N) {
        double v = 0.0;
        for (int j = 0; j <= t; j++) v += cum[t - j] * sFu[j];
        GS[t * LD] += tq * v;
    }
    // GSx = 2Q S gFx
    for (int e = t; e < N * nx; e += 64) {
        const int k = e / nx, c = e % nx;
        double v = 0.0;
        for (int j = 0; j <= k; j++) v += cum[k - j] * sFx[j * nx + c];
        GSx[e] = tq * v;
    }
    __syncthreads();
    // Gc_d = sum of GS's d-th subdiagonal; GCAB_k = sum_(d >= k) Gc_d (in place)
    if (t < N) {
        double v = 0.0;
        for (int j = 0; j + t < N; j++) v += GS[(j + t) * LD + j];
        Gc[t] = v;
    }
    __syncthreads();
    if (t == 0) {
        double v = 0.0;
        for (int k = N - 1; k >= 0; k--) { v += Gc[k]; Gc[k] = v; }
    }
    __syncthreads();
    // gBd = sum_k GCAB_k r_k';  rho_k = GCAB_k Bd' (k < N) + GSx(k-1) (k >= 1)
    if (t < nx && a.gBd) {
        double v = 0.0;
        for (int k = 0; k < N; k++) v += Gc[k] * r[k * nx + t];
        a.gBd[P * nx + t] = v;
    }
    for (int e = t; e < (N + 1) * nx; e += 64) {
        const int k = e / nx, c = e % nx;
        double v = (k < N) ? Gc[k] * sBd[c] : 0.0;
        if (k >= 1) v = (k < N) ? v + GSx[(k - 1) * nx + c] : GSx[(k - 1) * nx + c];
        rho[e] = v;
    }
    __syncthreads();
    // the reverse recursion: rho_(k-1) += rho_k Ad'  (rho_k is final when it is read)
    for (int k = N; k >= 1; k--) {
        if (t < nx) {
            double v = 0.0;
            for (int j = 0; j < nx; j++) v += rho[k * nx + j] * sAd[t * nx + j];
            rho[(k - 1) * nx + t] += v;
        }
        __syncthreads();
    }
    // gAd = sum_(k = N..1) r_(k-1)' rho_k;  gCd = rho_0
    if (t < nx * nx && a.gAd) {
        const int rr = t / nx, c = t % nx;
        double v = 0.0;
        for (int k = N; k >= 1; k--) v += r[(k - 1) * nx + rr] * rho[k * nx + c];
        a.gAd[P * nx * nx + t] = v;
    }
    if (t < nx && a.gCd) a.gCd[P * nx + t] = rho[t];

    // the scalars and gK
    const double sQ = vjp_wave_sum(accQ), sR = vjp_wave_sum(accR), sRD = vjp_wave_sum(accRD), sA = vjp_wave_sum(accA);
    if (t == 0) {
        double fu = 0.0;
        for (int j = 0; j < N; j++) fu += sFu[j];
        if (a.gQ) a.gQ[p] = sQ;
        if (a.gR) a.gR[p] = sR + 2.0 * fu;
        if (a.gRD) a.gRD[p] = sRD;
    }
    if (t < nx && a.gK) {
        const int rows = a.s_rows < N ? a.s_rows : N;
        double v = 0.0;
        if (gSbar)
            for (int i = 0; i < rows; i++) v += gSbar[i * nx + t] - gSbar[(N + i) * nx + t];
        if (t == 0) {
            double ku = 0.0;
            if (gKu)
                for (int i = 0; i < N; i++) ku += gKu[N + i] - gKu[i];
            v += sA + ku;
        }
        a.gK[P * nx + t] = v;
    }
}

__host__ __device__ inline size_t condense_vjp_lds(int nx, int N)
{
    return (size_t)nx * nx + nx + 2 * (size_t)(N + 1) * nx + 3 * (size_t)N + 2 * (size_t)N * nx + 2 * (size_t)N * (N | 1);
}

}  // namespace mpcq

extern "C" int mpcq_internal_condense_vjp_launch(const mpcq::CondenseVjpArgs *a, hipStream_t s)
{
    if (a->N < 1 || a->N > 32 || a->nx < 1 || a->nx > 8 || a->n_plants < 1) return -1;
    hipLaunchKernelGGL(mpcq::condense_vjp_kernel, dim3(a->n_plants), dim3(64),
                       8 * mpcq::condense_vjp_lds(a->nx, a->N), s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

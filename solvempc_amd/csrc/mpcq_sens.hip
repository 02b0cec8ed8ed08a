// solvempc_amd/csrc/mpcq_sens.hip — active-set sensitivities of the last solve, one QP per 64-lane wave.
//
// For every QP that ended SOLVED, in fp64 whatever the context's dtype:
//   1. scaled data P^ = c D P D, A^ = E A D and the bounds l^ = E l, u^ = E u, as polish_kernel forms them;
//   2. the final scaled iterate z^, y^ from the warm state (type T, converted; x^ = W x' is not needed: the
//      rule reads z^ and y^ only);
//   3. OSQP's active sets by polish's rule: row lower-active when z^ - l^ < -y^, else upper-active when
//      u^ - z^ < y^; A_red holds the lower-active rows followed by the upper-active ones (mr rows);
//   4. the cotangent g (or e_0) scaled, g^ = c D g, and the regularised reduced KKT system
//      [P^ + delta I, A_red'; A_red, -delta I] [v^; w^] = [g^; 0] by the Cholesky factor of H = P^ + delta I
//      and of the Schur complement S = delta I + A_red H^-1 A_red', then `refine` steps of iterative refinement
//      against the unregularised matrix;
//   5. gq = -D v^, and w = E_a w^ / c scattered into gl (lower-active rows) and gu (upper-active rows).
// Nothing of the context is written: the kernel only reads the warm state and the QP's data.
//
// Layout as in mpcq_polish.hip: matrices in LDS at odd fp64 strides, vectors in registers with lane i holding
// element i, triangular solves by shuffles.  A shared plant's P^, A^, the factor of H and G = A^ H^-1 A^'
// (m x m) are formed once per workgroup, so a QP's Schur complement is the gather delta I + G[act, act]; a
// per-plant context forms V = (L^-1 A_red')' and S = delta I + V V' per QP, as polish does.  The two share
// one carve-up: region R1 holds V (while G is formed, or per QP) and then S for a shared plant; region R2
// holds G for a shared plant and S otherwise.
//
// sens_chain_kernel: the MPC chain rule of the step gains, q = Fx X + Fu U + Fr ref, u = W0 + Sbar X + Ku U:
//   dX = Fx' gq + Sbar' gu, dU = Fu' gq + Ku' gu, dref = Fr' gq, one thread per output element, fp64 sums in
//   ascending row index.
#include <algorithm>

#include "mpcq_internal.h"
#include "mpcq_wavechol.h"

namespace mpcq {

__global__ __launch_bounds__(64) void sens_kernel(SensArgs a)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int n = a.n, m = a.m, nc = a.nc, mc = a.mc;
    const int ldn = n | 1, ldS = m | 1, ld1 = ldn > ldS ? ldn : ldS;
    const bool ln = lane < n, lm = lane < m;
    double *const Ph = lds;                 // n x ldn   P^
    double *const Ah = Ph + n * ldn;        // m x ldn   A^
    double *const Lh = Ah + m * ldn;        // n x ldn   Cholesky factor of H = P^ + delta I
    double *const R1 = Lh + n * ldn;        // m x ld1   V (row j: L^-1 a_j), then S of a shared plant
    double *const R2 = R1 + m * ld1;        // m x ldS   G of a shared plant, S of a per-plant context
    double *const xv = R2 + m * ldS;        // n         staging (an n-vector read by every lane)
    double *const mv = xv + n;              // m         staging (an m-vector)
    double *const dH = mv + m;              // n         1 / diag of Lh
    double *const dS = dH + n;              // m         1 / diag of the factor of S
    int *const act = (int *)(dS + m);       // m         row of A^ behind each reduced row
    double *const V = R1;
    double *const G = R2;
    double *const S = a.shared ? R1 : R2;
    const OpsLayout L = OpsLayout::make(nc, mc);
    bool have_plant = false, h_ok = false;

    for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
        __syncthreads();  // the previous QP of this workgroup is done with the staging buffers
        bool ok = a.status[b] == kSolved;  // (wave-uniform)
        const size_t pp = a.shared ? 0 : (size_t)b;
        const double *ops = a.ops + pp * a.ops_stride;
        int mr = 0, pos = 0;
        bool low = false, upp = false;
        unsigned long long mlow = 0ull, mupp = 0ull;
        double sx = 0.0, sn = 0.0;
        if (ok) {
            const double c = ops[L.cs];
            const double Ej = lm ? ops[L.E + lane] : 0.0;

            // ---- 1. scaled data, the factor of H and (shared plant) G, once per workgroup for a shared plant
            if (!a.shared || !have_plant) {
                const double *P = a.P + pp * n * n, *A = a.A + pp * m * n;
                for (int e = lane; e < n * n; e += 64) {
                    const int i = e / n, j = e - i * n;
                    const double p = i <= j ? P[i * n + j] : P[j * n + i];  // upper triangle, as OSQP reads it
                    const double v = (c * ops[L.D + i]) * p * ops[L.D + j];
                    Ph[i * ldn + j] = v;
                    Lh[i * ldn + j] = i == j ? v + a.delta : v;
                }
                for (int e = lane; e < m * n; e += 64) {
                    const int j = e / n, k = e - j * n;
                    Ah[j * ldn + k] = (ops[L.E + j] * A[j * n + k]) * ops[L.D + k];
                }
                __syncthreads();
                h_ok = wave_cholesky(Lh, ldn, n, dH, lane);
                have_plant = true;
                if (a.shared && h_ok) {  // V = (L^-1 A^')' over every row, then G = V V'
                    if (lm) {
                        for (int i = 0; i < n; i++) {
                            double v = Ah[lane * ldn + i];
                            for (int k = 0; k < i; k++) v -= Lh[i * ldn + k] * V[lane * ld1 + k];
                            V[lane * ld1 + i] = v * dH[i];
                        }
                    }
                    __syncthreads();
                    if (lm) {
                        for (int j = 0; j < m; j++) {
                            double v = 0.0;
                            for (int k = 0; k < n; k++) v += V[lane * ld1 + k] * V[j * ld1 + k];
                            G[lane * ldS + j] = v;
                        }
                    }
                    __syncthreads();  // (V is dead: R1 is S from here on)
                }
            }
            ok = h_ok;

            // ---- 2./3. the final scaled iterate's z^, y^ and the active sets
            const double lo = lm ? a.l[(size_t)b * m + lane] * Ej : 0.0;  // (-DBL_MAX E may be -inf: only compared)
            const double up = lm ? a.u[(size_t)b * m + lane] * Ej : 0.0;
            auto state = [&](const void *p, size_t i) -> double {
                return a.is_f32 ? (double)((const float *)p)[i] : ((const double *)p)[i];
            };
            const double zh = lm ? state(a.zs, (size_t)b * mc + lane) : 0.0;
            const double yh = lm ? state(a.ys, (size_t)b * mc + lane) : 0.0;
            low = lm && (zh - lo < -yh);
            upp = lm && !low && (up - zh < yh);
            mlow = __ballot(low);
            mupp = __ballot(upp);
            const unsigned long long below = (1ull << lane) - 1ull;
            const int n_low = __popcll(mlow);
            mr = n_low + __popcll(mupp);
            pos = low ? __popcll(mlow & below) : n_low + __popcll(mupp & below);
            if (low || upp) act[pos] = lane;
            __syncthreads();
        }
        const bool lr = lane < mr;
        const int aj = lr ? act[lane] : 0;

        // ---- 4. Schur complement and its factor
        if (ok) {
            if (a.shared) {
                if (lr)
                    for (int j = 0; j <= lane; j++) S[lane * ld1 + j] = (j == lane ? a.delta : 0.0) + G[aj * ldS + act[j]];
            } else {
                if (lr) {
                    for (int i = 0; i < n; i++) {
                        double v = Ah[aj * ldn + i];
                        for (int k = 0; k < i; k++) v -= Lh[i * ldn + k] * V[lane * ld1 + k];
                        V[lane * ld1 + i] = v * dH[i];
                    }
                }
                __syncthreads();
                if (lr) {
                    for (int j = 0; j <= lane; j++) {
                        double v = j == lane ? a.delta : 0.0;
                        for (int k = 0; k < n; k++) v += V[lane * ld1 + k] * V[j * ld1 + k];
                        S[lane * ldS + j] = v;
                    }
                }
            }
            __syncthreads();
            ok = wave_cholesky(S, a.shared ? ld1 : ldS, mr, dS, lane);
        }
        const int lds_s = a.shared ? ld1 : ldS;

        // K_reg^-1 [r1; r2]: nu = S^-1 (A_red H^-1 r1 - r2), x = H^-1 (r1 - A_red' nu)
        auto kkt_solve = [&](double r1, double r2, double &ox, double &on) {
            const double t = wave_chol_solve(Lh, ldn, n, dH, r1, lane);
            if (ln) xv[lane] = t;
            __syncthreads();
            double w = 0.0;
            if (lr) {
                for (int k = 0; k < n; k++) w += Ah[aj * ldn + k] * xv[k];
                w -= r2;
            }
            on = wave_chol_solve(S, lds_s, mr, dS, w, lane);
            if (lr) mv[lane] = on;
            __syncthreads();
            double r = r1;
            if (ln)
                for (int j = 0; j < mr; j++) r -= Ah[act[j] * ldn + lane] * mv[j];
            ox = wave_chol_solve(Lh, ldn, n, dH, r, lane);
            __syncthreads();  // (xv, mv free again)
        };

        if (ok) {
            const double c = ops[L.cs];
            const double Di = ln ? ops[L.D + lane] : 0.0;
            const double gi = a.g ? (ln ? a.g[(size_t)b * n + lane] : 0.0) : (lane == 0 ? 1.0 : 0.0);
            const double b1 = (gi * Di) * c;
            kkt_solve(b1, 0.0, sx, sn);
            for (int it = 0; it < a.refine; it++) {  // s += K_reg^-1 (b - K s), K without delta
                if (ln) xv[lane] = sx;
                if (lr) mv[lane] = sn;
                __syncthreads();
                double r1 = b1, r2 = 0.0;
                if (ln) {
                    for (int k = 0; k < n; k++) r1 -= Ph[lane * ldn + k] * xv[k];
                    for (int j = 0; j < mr; j++) r1 -= Ah[act[j] * ldn + lane] * mv[j];
                }
                if (lr)
                    for (int k = 0; k < n; k++) r2 -= Ah[aj * ldn + k] * xv[k];
                __syncthreads();
                double dx, dn;
                kkt_solve(r1, r2, dx, dn);
                sx += dx;
                sn += dn;
            }
            if (lr) mv[lane] = sn;
            __syncthreads();
        }

        // ---- 5. results: zeros and n_active = -1 where the QP did not end SOLVED (or a factor failed)
        double gqv = 0.0, wv = 0.0;
        if (ok) {
            const double cinv = ops[L.cs + 1];
            gqv = ln ? -(sx * ops[L.D + lane]) : 0.0;
            if (low || upp) wv = (mv[pos] * ops[L.E + lane]) * cinv;
        }
        if (ln && a.gq) a.gq[(size_t)b * n + lane] = gqv;
        if (lm && a.gl) a.gl[(size_t)b * m + lane] = low ? wv : 0.0;
        if (lm && a.gu) a.gu[(size_t)b * m + lane] = upp ? wv : 0.0;
        if (lane == 0 && a.n_active) a.n_active[b] = ok ? mr : -1;
        if (lane < 2 && a.active) a.active[2 * (size_t)b + lane] = ok ? (lane ? mupp : mlow) : 0ull;
    }
}

__global__ __launch_bounds__(256) void sens_chain_kernel(SensChainArgs a)
{
    const int per = a.nx + 1 + a.n;
    const long long total = (long long)a.batch * per;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(t / per), o = (int)(t - (long long)b * per);
        const size_t pp = a.shared ? 0 : (size_t)b;
        const double *gq = a.gq + (size_t)b * a.n, *gu = a.gu + (size_t)b * a.m;
        double s = 0.0;
        if (o < a.nx) {
            const double *Fx = a.Fx + pp * a.n * a.nx, *Sbar = a.Sbar + pp * a.m * a.nx;
            for (int i = 0; i < a.n; i++) s += Fx[i * a.nx + o] * gq[i];
            for (int j = 0; j < a.m; j++) s += Sbar[j * a.nx + o] * gu[j];
            if (a.dX) a.dX[(size_t)b * a.nx + o] = s;
        } else if (o == a.nx) {
            const double *Fu = a.Fu + pp * a.n, *Ku = a.Ku + pp * a.m;
            for (int i = 0; i < a.n; i++) s += Fu[i] * gq[i];
            for (int j = 0; j < a.m; j++) s += Ku[j] * gu[j];
            if (a.dU) a.dU[b] = s;
        } else {
            const int tt = o - a.nx - 1;
            const double *Fr = a.Fr + pp * a.n * a.n;
            for (int i = 0; i < a.n; i++) s += Fr[i * a.n + tt] * gq[i];
            if (a.dref) a.dref[(size_t)b * a.n + tt] = s;
        }
    }
}

}  // namespace mpcq

// LDS bytes of one workgroup (the kernel's carve-up: three matrices of stride n|1, R1, R2, the vectors)
static size_t sens_lds(int n, int m)
{
    const size_t ldn = (size_t)(n | 1), ldS = (size_t)(m | 1), ld1 = std::max(ldn, ldS);
    const size_t doubles = 2 * n * ldn + m * ldn + m * ld1 + m * ldS + 2 * (size_t)n + 3 * (size_t)m;
    return 8 * doubles;
}

extern "C" int mpcq_internal_sens_launch(const mpcq::SensArgs *a, int cus, hipStream_t s, hipError_t *err)
{
    *err = hipSuccess;
    if (a->n <= 0 || a->n > 32 || a->m < 0 || a->m > 64) return -1;
    if (a->batch <= 0) return 0;
    const size_t lds = sens_lds(a->n, a->m);
    if (lds > 160 * 1024) return -1;
    if (lds > 64 * 1024 &&
        (*err = hipFuncSetAttribute((const void *)mpcq::sens_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds)) != hipSuccess)
        return -2;
    // one wave per workgroup; as many workgroups as the LDS lets a CU hold (at most 8), striding over the batch
    const int per_cu = (int)std::min<size_t>(8, std::max<size_t>(1, (160 * 1024) / lds));
    const int grid = std::min(a->batch, std::max(1, cus) * per_cu);
    hipLaunchKernelGGL(mpcq::sens_kernel, dim3(grid), dim3(64), lds, s, *a);
    *err = hipGetLastError();
    return *err == hipSuccess ? 0 : -2;
}

extern "C" int mpcq_internal_sens_chain_launch(const mpcq::SensChainArgs *a, hipStream_t s)
{
    if (a->batch <= 0) return 0;
    const long long total = (long long)a->batch * (a->nx + 1 + a->n);
    const int grid = (int)std::min<long long>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(mpcq::sens_chain_kernel, dim3(grid), dim3(256), 0, s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

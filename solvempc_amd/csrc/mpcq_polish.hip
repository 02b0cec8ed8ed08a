// solvempc_amd/csrc/mpcq_polish.hip — OSQP v0.6 solution polishing (polish.c), one QP per 64-lane wave.
//
// Runs after the ADMM launches of a solve when settings.polish is set, in fp64 whatever the context's
// dtype, on every QP that ended SOLVED:
//   1. scaled data P^ = c D P D (symmetrised from P's upper triangle), A^ = E A D, q^ = c D q, l^ = E l,
//      u^ = E u from the context's unscaled setup data and the plant's Ruiz scaling;
//   2. the final scaled iterate x^ = W x', z^, y^ from the warm state (type T, converted);
//   3. OSQP's active sets: row lower-active when z^ - l^ < -y^, upper-active when u^ - z^ < y^; A_red holds
//      the lower-active rows followed by the upper-active ones (mr rows, 0 <= mr <= m);
//   4. the regularised KKT system [P^ + delta I, A_red'; A_red, -delta I] s = [-q^; l^_low; u^_upp] by
//      Cholesky of H = P^ + delta I and of the Schur complement S = delta I + A_red H^-1 A_red' (positive
//      definite thanks to delta, whatever the rank of A_red), then polish_refine_iter steps of iterative
//      refinement against the unregularised matrix, s += K_reg^-1 (b - K s);
//   5. x_pol = s[0:n], z_pol = A^ x_pol, y_pol scattered from s[n:], then project_normalcone:
//      t = z + y, z = clip(t, l^, u^), y = t - z;
//   6. success when both residuals (termination norms) are reduced, or one is and the other was already
//      below 1e-10; then x = D x_pol, y = E y_pol / c and the warm state (x' = W^-1 x_pol, z_pol, y_pol) are
//      written, else the ADMM result stays;
//   7. in an MPC step, U += x[0] for every SOLVED QP, polished or not.
//
// Layout: matrices in LDS at odd fp64 strides (lane i walks row i: conflict-free; a broadcast row costs
// one access), vectors in registers, lane i holding element i (n <= 32 and m <= 64 both fit the 64 lanes).
// A triangular solve keeps its vector in registers: step k broadcasts element k with a shuffle and every
// later lane subtracts its multiple, so it needs no LDS write and no barrier.  A shared plant's P^, A^ and
// the factor of H are formed once per workgroup; the grid strides over the batch.
#include <algorithm>

#include "mpcq_internal.h"
#include "mpcq_wavechol.h"

namespace mpcq {

__global__ __launch_bounds__(64) void polish_kernel(PolishArgs a)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int n = a.n, m = a.m, nc = a.nc, mc = a.mc;
    const int ldn = n | 1, ldS = m | 1;
    const bool ln = lane < n, lm = lane < m;
    double *const Ph = lds;                 // n x ldn   P^
    double *const Ah = Ph + n * ldn;        // m x ldn   A^
    double *const Lh = Ah + m * ldn;        // n x ldn   Cholesky factor of H = P^ + delta I
    double *const V = Lh + n * ldn;         // m x ldn   row j: L^-1 a_red_j
    double *const S = V + m * ldn;          // m x ldS   Schur complement, then its factor
    double *const xv = S + m * ldS;         // n         staging (an n-vector read by every lane)
    double *const mv = xv + n;              // m         staging (an m-vector)
    double *const dH = mv + m;              // n         1 / diag of Lh
    double *const dS = dH + n;              // m         1 / diag of the factor of S
    double *const bact = dS + m;            // m         rhs of the reduced rows (l^ / u^ of the active rows)
    int *const act = (int *)(bact + m);     // m         row of A^ behind each reduced row
    const OpsLayout L = OpsLayout::make(nc, mc);
    const double nanv = __builtin_nan("");
    bool have_plant = false, h_ok = false;

    for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
        __syncthreads();  // the previous QP of this workgroup is done with the staging buffers
        if (a.status[b] != kSolved) {  // (wave-uniform)
            if (lane == 0) {
                a.pol_status[b] = 0;
                a.pol_nact[b] = 0;
                a.pol_res[2 * (size_t)b] = nanv;
                a.pol_res[2 * (size_t)b + 1] = nanv;
            }
            continue;
        }
        const size_t pp = a.shared ? 0 : (size_t)b;
        const double *ops = a.ops + pp * a.ops_stride;
        const double c = ops[L.cs], cinv = ops[L.cs + 1];
        const double Di = ln ? ops[L.D + lane] : 0.0, Dinvi = ln ? ops[L.Dinv + lane] : 0.0;
        const double Ej = lm ? ops[L.E + lane] : 0.0, Einvj = lm ? ops[L.Einv + lane] : 0.0;

        // ---- 1. scaled data (once per workgroup for a shared plant) and the factor of H
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
        }

        // ---- per-QP data
        const double qh = ln ? (a.q[(size_t)b * n + lane] * Di) * c : 0.0;
        const double lo = lm ? a.l[(size_t)b * m + lane] * Ej : 0.0;  // (-DBL_MAX E may be -inf: only compared)
        const double up = lm ? a.u[(size_t)b * m + lane] * Ej : 0.0;

        // ---- 2. final scaled iterate
        auto state = [&](const void *p, size_t i) -> double {
            return a.is_f32 ? (double)((const float *)p)[i] : ((const double *)p)[i];
        };
        if (ln) xv[lane] = state(a.xs, (size_t)b * nc + lane);
        const double zh = lm ? state(a.zs, (size_t)b * mc + lane) : 0.0;
        const double yh = lm ? state(a.ys, (size_t)b * mc + lane) : 0.0;
        __syncthreads();
        double xh = 0.0;
        if (ln)
            for (int k = 0; k < n; k++) xh += ops[L.W + (size_t)lane * nc + k] * xv[k];
        __syncthreads();

        // ---- 3. active sets
        const bool low = lm && (zh - lo < -yh);
        const bool upp = lm && !low && (up - zh < yh);  // (exclusive by l <= u; enforced for the bounds' sake)
        const unsigned long long mlow = __ballot(low), mupp = __ballot(upp);
        const unsigned long long below = (1ull << lane) - 1ull;
        const int n_low = __popcll(mlow), mr = n_low + __popcll(mupp);
        const int pos = low ? __popcll(mlow & below) : n_low + __popcll(mupp & below);
        if (low || upp) {
            act[pos] = lane;
            bact[pos] = low ? lo : up;
        }
        __syncthreads();
        const bool lr = lane < mr;
        const int aj = lr ? act[lane] : 0;
        const double b2 = lr ? bact[lane] : 0.0;
        const double b1 = -qh;

        // ---- 4. Schur complement S = delta I + V V', V = (L^-1 A_red')' (lane j: row j, forward substitution)
        bool ok = h_ok;
        if (ok) {
            if (lr) {
                for (int i = 0; i < n; i++) {
                    double v = Ah[aj * ldn + i];
                    for (int k = 0; k < i; k++) v -= Lh[i * ldn + k] * V[lane * ldn + k];
                    V[lane * ldn + i] = v * dH[i];
                }
            }
            __syncthreads();
            if (lr) {
                for (int j = 0; j <= lane; j++) {
                    double v = j == lane ? a.delta : 0.0;
                    for (int k = 0; k < n; k++) v += V[lane * ldn + k] * V[j * ldn + k];
                    S[lane * ldS + j] = v;
                }
            }
            __syncthreads();
            ok = wave_cholesky(S, ldS, mr, dS, lane);
        }

        // K_reg^-1 [r1; r2]: nu = S^-1 (A_red H^-1 r1 - r2), x = H^-1 (r1 - A_red' nu)
        auto kkt_solve = [&](double r1, double r2, double &sx, double &sn) {
            const double t = wave_chol_solve(Lh, ldn, n, dH, r1, lane);
            if (ln) xv[lane] = t;
            __syncthreads();
            double w = 0.0;
            if (lr) {
                for (int k = 0; k < n; k++) w += Ah[aj * ldn + k] * xv[k];
                w -= r2;
            }
            sn = wave_chol_solve(S, ldS, mr, dS, w, lane);
            if (lr) mv[lane] = sn;
            __syncthreads();
            double r = r1;
            if (ln)
                for (int j = 0; j < mr; j++) r -= Ah[act[j] * ldn + lane] * mv[j];
            sx = wave_chol_solve(Lh, ldn, n, dH, r, lane);
            __syncthreads();  // (xv, mv free again)
        };

        double sx = 0.0, sn = 0.0;
        if (ok) {
            kkt_solve(b1, b2, sx, sn);
            for (int it = 0; it < a.refine; it++) {  // s += K_reg^-1 (b - K s), K without delta
                if (ln) xv[lane] = sx;
                if (lr) mv[lane] = sn;
                __syncthreads();
                double r1 = b1, r2 = b2;
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
        }

        // ---- 5./6. residuals of a point (x in xv, y in mv; lane j's (A^ x)_j and z_j): termination norms
        auto row_ax = [&]() {
            double ax = 0.0;
            if (lm)
                for (int k = 0; k < n; k++) ax += Ah[lane * ldn + k] * xv[k];
            return ax;
        };
        auto residuals = [&](double ax, double zj, double &pri, double &dua) {
            double d = 0.0;
            if (ln) {
                for (int k = 0; k < n; k++) d += Ph[lane * ldn + k] * xv[k];
                d += qh;
                for (int j = 0; j < m; j++) d += Ah[j * ldn + lane] * mv[j];
            }
            double p = lm ? ax - zj : 0.0;
            if (!a.scaled_termination) {
                p *= Einvj;
                d = (d * Dinvi) * cinv;
            }
            pri = wave_nan_max(lm ? fabs(p) : 0.0);
            dua = wave_nan_max(ln ? fabs(d) : 0.0);
        };
        // the ADMM iterate
        if (ln) xv[lane] = xh;
        if (lm) mv[lane] = yh;
        __syncthreads();
        double pri_a, dua_a;
        residuals(row_ax(), zh, pri_a, dua_a);
        __syncthreads();
        // the polished point: y scattered from the reduced duals, z = A^ x, then project_normalcone
        double pri_p = nanv, dua_p = nanv, zp = 0.0, yp = 0.0;
        if (ok) {
            if (lr) mv[lane] = sn;
            if (ln) xv[lane] = sx;
            __syncthreads();
            yp = (low || upp) ? mv[pos] : 0.0;
            const double ax = row_ax();
            const double t = ax + yp;
            zp = fmin(fmax(t, lo), up);
            yp = t - zp;
            __syncthreads();
            if (lm) mv[lane] = yp;
            __syncthreads();
            residuals(ax, zp, pri_p, dua_p);
        }
        const bool success = ok && ((pri_p < pri_a && dua_p < dua_a) || (pri_p < pri_a && dua_a < 1e-10) ||
                                    (dua_p < dua_a && pri_a < 1e-10));

        // ---- 7./8. results
        double x0 = 0.0;  // the returned x[0] (lane 0)
        if (success) {
            // (xv still holds x_pol)
            if (ln) {
                const double xo = sx * Di;
                a.x[(size_t)b * n + lane] = xo;
                x0 = xo;
                double xp = 0.0;
                for (int i = 0; i < n; i++) xp += ops[L.Winv + (size_t)lane * nc + i] * xv[i];
                if (a.is_f32) ((float *)a.xs)[(size_t)b * nc + lane] = (float)xp;
                else ((double *)a.xs)[(size_t)b * nc + lane] = xp;
            }
            if (lm) {
                a.y[(size_t)b * m + lane] = (yp * Ej) * cinv;
                if (a.is_f32) {
                    ((float *)a.zs)[(size_t)b * mc + lane] = (float)zp;
                    ((float *)a.ys)[(size_t)b * mc + lane] = (float)yp;
                } else {
                    ((double *)a.zs)[(size_t)b * mc + lane] = zp;
                    ((double *)a.ys)[(size_t)b * mc + lane] = yp;
                }
            }
        } else if (lane == 0 && a.U) {
            x0 = a.x[(size_t)b * n];
        }
        if (lane == 0) {
            if (a.U) a.U[b] += x0;  // U += x(0)  (ModelPredictiveControlAPI.cpp:105)
            a.pol_status[b] = success ? 1 : -1;
            a.pol_nact[b] = mr;
            a.pol_res[2 * (size_t)b] = success ? pri_p : pri_a;
            a.pol_res[2 * (size_t)b + 1] = success ? dua_p : dua_a;
        }
    }
}

}  // namespace mpcq

// LDS bytes of one workgroup (the kernel's carve-up: four matrices of stride n|1, S of stride m|1, the vectors)
static size_t polish_lds(int n, int m)
{
    const size_t ldn = (size_t)(n | 1), ldS = (size_t)(m | 1);
    const size_t doubles = 2 * n * ldn + 2 * m * ldn + m * ldS + 2 * (size_t)n + 4 * (size_t)m;
    return 8 * doubles;
}

extern "C" int mpcq_internal_polish_launch(const mpcq::PolishArgs *a, int cus, hipStream_t s, hipError_t *err)
{
    *err = hipSuccess;
    if (a->n <= 0 || a->n > 32 || a->m < 0 || a->m > 64) return -1;
    if (a->batch <= 0) return 0;
    const size_t lds = polish_lds(a->n, a->m);
    if (lds > 160 * 1024) return -1;
    if (lds > 64 * 1024 &&
        (*err = hipFuncSetAttribute((const void *)mpcq::polish_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds)) != hipSuccess)
        return -2;
    // one wave per workgroup; as many workgroups as the LDS lets a CU hold (at most 8), striding over the batch
    const int per_cu = (int)std::min<size_t>(8, std::max<size_t>(1, (160 * 1024) / lds));
    const int grid = std::min(a->batch, std::max(1, cus) * per_cu);
    hipLaunchKernelGGL(mpcq::polish_kernel, dim3(grid), dim3(64), lds, s, *a);
    *err = hipGetLastError();
    return *err == hipSuccess ? 0 : -2;
}

// solvempc_amd/csrc/mpcq_polish.hip — OSQP v0.6 solution polishing (polish.c), one QP per 64-lane wave.
//
// Runs after the ADMM launches of a solve when settings.polish is set, in fp64 whatever the context's
// dtype, on every QP that ended SOLVED:
//   1. scaled data P^ = c D P D (symmetrised from P's upper triangle), A^ = E A D, q^ = c D q, l^ = E l,
//      u^ = E u from the context's unscaled setup data and the plant's Ruiz scaling;
//   2. the final scaled iterate x^ = W x', z^, y^ from the warm state (type T, converted);
//   3. OSQP's active sets and A_red, the lower-active rows followed by the upper-active ones (mr rows,
//      0 <= mr <= m): WaveKkt::active_sets (mpcq_wavekkt.h);
//   4. the regularised KKT system [P^ + delta I, A_red'; A_red, -delta I] s = [-q^; l^_low; u^_upp] and
//      polish_refine_iter steps of iterative refinement against the unregularised matrix:
//      WaveKkt::schur_from_rows and solve_refined;
//   5. x_pol = s[0:n], z_pol = A^ x_pol, y_pol scattered from s[n:], then project_normalcone:
//      t = z + y, z = clip(t, l^, u^), y = t - z;
//   6. success when both residuals (termination norms) are reduced, or one is and the other was already
//      below 1e-10; then x = D x_pol, y = E y_pol / c and the warm state (x' = W^-1 x_pol, z_pol, y_pol) are
//      written, else the ADMM result stays;
//   7. in an MPC step, U += x[0] for every SOLVED QP, polished or not.
//
// Layout: mpcq_wavekkt.h's (matrices in LDS at odd fp64 strides, vectors in registers, lane i holding element i);
// the forming of step 1's P^ and A^ and the factor of H is WaveKkt::form.  A shared plant's P^, A^ and the factor
// of H are formed once per workgroup; the grid strides over the batch.
#include "mpcq_internal.h"
#include "mpcq_wavekkt.h"

namespace mpcq {

__global__ __launch_bounds__(64) void polish_kernel(PolishArgs a)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int n = a.n, m = a.m, nc = a.nc, mc = a.mc;
    const bool ln = lane < n, lm = lane < m;
    WaveKkt K(n, m, a.delta, lane);
    const int ldn = K.ldn;
    double *const V = K.head(lds);          // m x ldn   row j: L^-1 a_red_j
    K.S = V + m * ldn;                      // m x ldS   Schur complement, then its factor
    K.ldS = m | 1;
    double *const bact = K.tail(K.S + m * K.ldS);  // m  rhs of the reduced rows (l^ / u^ of the active rows)
    K.act = (int *)(bact + m);
    double *const Ph = K.Ph, *const Ah = K.Ah, *const xv = K.xv, *const mv = K.mv;
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
            h_ok = K.form(a.P + pp * n * n, a.A + pp * m * n, ops + L.D, ops + L.E, c);
            have_plant = true;
        }

        // ---- per-QP data
        const double qh = ln ? (a.q[(size_t)b * n + lane] * Di) * c : 0.0;
        const double lo = lm ? a.l[(size_t)b * m + lane] * Ej : 0.0;  // (-DBL_MAX E may be -inf: only compared)
        const double up = lm ? a.u[(size_t)b * m + lane] * Ej : 0.0;

        // ---- 2. final scaled iterate
        if (ln) xv[lane] = warm_state(a.xs, a.is_f32, (size_t)b * nc + lane);
        const double zh = lm ? warm_state(a.zs, a.is_f32, (size_t)b * mc + lane) : 0.0;
        const double yh = lm ? warm_state(a.ys, a.is_f32, (size_t)b * mc + lane) : 0.0;
        __syncthreads();
        double xh = 0.0;
        if (ln)
            for (int k = 0; k < n; k++) xh += ops[L.W + (size_t)lane * nc + k] * xv[k];
        __syncthreads();

        // ---- 3. active sets
        K.active_sets(zh, yh, lo, up, bact);
        const bool low = K.low, upp = K.upp, lr = K.lr;
        const int mr = K.mr, pos = K.pos;

        // ---- 4. the reduced KKT system [-q^; l^_low; u^_upp], refined
        const bool ok = h_ok && K.schur_from_rows(V, ldn);
        double sx = 0.0, sn = 0.0;
        if (ok) K.solve_refined(-qh, lr ? bact[lane] : 0.0, a.refine, sx, sn);

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
    return mpcq::launch_per_qp(mpcq::polish_kernel, *a, a->batch, 64, polish_lds(a->n, a->m), 0, cus, s, err);
}

// solvempc_amd/csrc/mpcq_mimo_polish.hip — OSQP v0.6 solution polishing (polish.c) of a MIMO step
// (mpcq_mimo_step_polish_device), one 256-thread workgroup per QP, the grid striding over the batch; fp64
// (DESIGN.md 4.16).
//
// Runs after the step's kernel on the same stream, on every QP that ended SOLVED:
//   1. the active set by OSQP's rule on the step's scaled iterate (z^, y^) with u^ = E u of the step's bounds
//      (l = -DBL_MAX: upper-active rows only, ascending row index);
//   2. H = P^ + delta I and S = delta I + A_a H^-1 A_a' factored and inverted in place (mpcq_wgkkt.h);
//   3. [H, A_a'; A_a, -delta I] [x^; y_a] = [-q^; u^_a], q^ = c D q of the step's q, and polish_refine_iter steps of
//      iterative refinement against the unregularised matrix;
//   4. y^ scattered from y_a, t = A^ x^ + y^, z^ = min(t, u^), y^ = t - z^ (project_normalcone);
//   5. both points' residuals in the step's termination norm, all 2n rows through the structured products, P^ read
//      as symmetric from the operator block;
//   6. success when both residuals are reduced, or one is and the other was already below 1e-10; then x = D x^,
//      y = E y^ / c, the warm state (x^, z^, y^) and U = U_prev + x[0:n_u] are written, else everything stays.
// A QP with more than n active rows (some bound pair j, n + j both active) or a non-positive pivot is reported
// unsuccessful with everything kept: the Schur region and the register tiles hold at most n reduced rows.
//
// An m-vector is at most 256 entries: u^, z^, y^ of row t live in thread t's registers; only y^ also goes to LDS, for
// A^' y^.  No atomics anywhere: two calls on equal state give identical bits.
#include "mpcq_internal.h"
#include "mpcq_wavechol.h"
#include "mpcq_wgkkt.h"

namespace mpcq {

// LDS carve-up (doubles) of polish_mimo_kernel for n variables: the reduced KKT system's (b1: -q^; sx: the ADMM x^,
// then the polished x^; sn: y_a; r1 also: the top half of A^ x^), then the kernel's own
struct MimoPolishShape {
    WgKktShape k;
    int dx, dn, bu, ym, total;
    __host__ __device__ static MimoPolishShape make(int n)
    {
        MimoPolishShape s{};
        s.k = WgKktShape::make(n);
        int o = s.k.total;
        s.dx = o; o += n;              // a refinement step's update; P^ x^ + q^ + A^' y^
        s.dn = o; o += s.k.n8;
        s.bu = o; o += s.k.n8;         // u^ of the reduced rows
        s.ym = o; o += 2 * n;          // y^ of all 2n rows
        s.total = o;
        return s;
    }
};

template <int NU>
__global__ __launch_bounds__(kWgThreads) void polish_mimo_kernel(MimoPolishArgs a)
{
    extern __shared__ double lds[];
    __shared__ double s_K0[16], s_piv[2], s_red[8];
    __shared__ int s_cnt[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int N = a.N, n = N * NU, m = 2 * n;
    const MimoLayout L = MimoLayout::make(N, a.nx, NU, a.ny);
    const MimoPolishShape S = MimoPolishShape::make(n);
    WgKkt<NU> K(lds, S.k, s_K0, s_piv, N, t);
    double *const sD = K.sD, *const b1 = K.b1, *const sx = K.sx, *const sn = K.sn, *const r1 = K.r1;
    double *const ta = K.ta, *const tc = K.tc, *const pp = K.pp;
    double *const dx = lds + S.dx, *const dn = lds + S.dn, *const bu = lds + S.bu, *const ym = lds + S.ym;
    const int *const posm = K.posm;
    const double nanv = __builtin_nan("");

    for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
        __syncthreads();  // the previous QP of this workgroup is done with every buffer
        if (a.status[b] != kSolved) {  // (uniform) not performed
            if (t == 0) {
                a.pol_status[b] = 0;
                a.pol_nact[b] = 0;
                a.pol_res[2 * (size_t)b] = nanv;
                a.pol_res[2 * (size_t)b + 1] = nanv;
            }
            continue;
        }
        const double *ops = a.ops + (size_t)b * a.ops_stride;
        const double c = ops[L.cs], cinv = ops[L.cs + 1];
        // ---- P^ + delta I (lower triangle, packed), D, E, K0, -q^ and the step's iterate
        const double *Ph = ops + L.Ph;
        K.load(ops, L, a.delta);
        if (t < n) {
            b1[t] = -((a.q[(size_t)b * n + t] * sD[t]) * c);
            sx[t] = a.xs[(size_t)b * n + t];
        }
        // ---- 1. the active set (l = -DBL_MAX: no lower-active row); row t's u^, z^, y^ stay in thread t
        double Er = 1.0, uh = 0.0, zh = 0.0, yh = 0.0;
        bool upp = false;
        if (t < m) {
            Er = ops[L.E + (t < n ? t : t - n)];
            const double ut = a.u[(size_t)b * m + t];
            uh = ut * Er;
            zh = a.zs[(size_t)b * m + t];
            yh = a.ys[(size_t)b * m + t];
            upp = mimo_upper_active(ut, Er, zh, yh);
            ym[t] = yh;
        }
        const int mr = K.mr = wg_reduced_rows(upp, m, t, s_cnt, K.posm, K.act);

        // row t of A^ x for the x in xv (r1: its top half)
        auto row_ax = [&](const double *xv) {
            K.apply_A_rows(xv, r1);
            return t < m ? (t < n ? r1[t] : -r1[t - n]) : 0.0;
        };
        // the residuals of the point (xv, row t's z, ym) whose A^ x is ax, in the termination norm (uniform)
        auto residuals = [&](const double *xv, double ax, double zj, double &pri, double &dua) {
            wg_sym_mv_halves(Ph, L.ldp, n, xv, pp, t);
            __syncthreads();
            if (t < n) tc[t] = (pp[t] + pp[128 + t]) - b1[t];  // P^ x^ + q^
            __syncthreads();
            K.apply_At_rows(ym, tc, ta, dx);
            double p = t < m ? ax - zj : 0.0, d = t < n ? dx[t] : 0.0;
            if (!a.scaled_termination) {
                p = p / Er;
                if (t < n) d = (d / sD[t]) * cinv;
            }
            p = wave_nan_max(fabs(p));
            d = wave_nan_max(fabs(d));
            if (lane == 0) {
                s_red[wave] = p;
                s_red[4 + wave] = d;
            }
            __syncthreads();
            pri = nan_max(nan_max(s_red[0], s_red[1]), nan_max(s_red[2], s_red[3]));
            dua = nan_max(nan_max(s_red[4], s_red[5]), nan_max(s_red[6], s_red[7]));
            __syncthreads();
        };

        // ---- 5a. the ADMM iterate's residuals
        double pri_a, dua_a;
        residuals(sx, row_ax(sx), zh, pri_a, dua_a);

        // ---- 2. the factors
        bool ok = mr <= n;  // (more than n reduced rows: unsuccessful, everything kept)
        if (ok) {
            if (upp) bu[posm[t]] = uh;
            ok = K.factor(a.delta);
        }

        double pri_p = nanv, dua_p = nanv, zp = 0.0, yp = 0.0;
        if (ok) {
            // ---- 3. the regularised solve, refined against the unregularised matrix
            K.solve(b1, bu, sx, sn);
            K.refine(Ph, L.ldp, bu, a.refine, dx, dn);
            // ---- 4. the polished point
            const double ax = row_ax(sx);
            if (t < m) {
                const int p = posm[t];
                const double tt = ax + (p >= 0 ? sn[p] : 0.0);
                zp = fmin(tt, uh);
                yp = tt - zp;
                ym[t] = yp;
            }
            __syncthreads();
            // ---- 5b. its residuals
            residuals(sx, ax, zp, pri_p, dua_p);
        }
        // ---- 6. OSQP's success test and the results
        const bool success = ok && ((pri_p < pri_a && dua_p < dua_a) || (pri_p < pri_a && dua_a < 1e-10) ||
                                    (dua_p < dua_a && pri_a < 1e-10));
        if (success) {
#pragma clang fp contract(off)  // (U is U_prev plus the published x, rounded once each)
            if (t < n) {
                const double xo = sx[t] * sD[t];
                a.x[(size_t)b * n + t] = xo;
                a.xs[(size_t)b * n + t] = sx[t];
                if (t < NU) a.U[(size_t)b * NU + t] = a.U_prev[(size_t)b * NU + t] + xo;
            }
            if (t < m) {
                a.y[(size_t)b * m + t] = (yp * Er) * cinv;
                a.zs[(size_t)b * m + t] = zp;
                a.ys[(size_t)b * m + t] = yp;
            }
        }
        if (t == 0) {
            a.pol_status[b] = success ? 1 : -1;
            a.pol_nact[b] = mr;
            a.pol_res[2 * (size_t)b] = success ? pri_p : pri_a;
            a.pol_res[2 * (size_t)b + 1] = success ? dua_p : dua_a;
        }
    }
}

}  // namespace mpcq

extern "C" size_t mpcq_internal_mimo_polish_lds(int n) { return 8 * (size_t)mpcq::MimoPolishShape::make(n).total; }

extern "C" int mpcq_internal_mimo_polish_launch(const mpcq::MimoPolishArgs *a, int cus, hipStream_t s, hipError_t *err)
{
    *err = hipSuccess;
    if (!mpcq::mimo_shape_ok(a->N, a->nx, a->nu, a->ny)) return -1;
    if (a->batch <= 0) return 0;
    return mpcq::mimo_with_nu(a->nu, [&](auto nu) {
        // (256: the kernel's few static words)
        return mpcq::launch_per_qp(mpcq::polish_mimo_kernel<decltype(nu)::value>, *a, a->batch, mpcq::kWgThreads,
                                   mpcq_internal_mimo_polish_lds(a->N * a->nu), 256, cus, s, err);
    });
}

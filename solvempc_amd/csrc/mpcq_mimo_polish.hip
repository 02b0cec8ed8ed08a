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

// LDS carve-up (doubles) of polish_mimo_kernel for n variables
struct MimoPolishShape {
    int n, n8, ntri, rows, region;
    int X, R, sD, sE, b1, sx, sn, r1, r2, ta, tb, tc, wv, pre, dx, dn, bu, ym, pp, sg, ae, posm, act, total;
    __host__ __device__ static MimoPolishShape make(int n)
    {
        MimoPolishShape s{};
        const WgTriShape w = WgTriShape::make(n);
        s.n = n; s.n8 = w.n8; s.ntri = w.ntri; s.rows = w.rows; s.region = w.region;
        int o = 0;
        s.X = o; o += s.ntri;          // H, its factor L, then X = L^-1 (packed lower)
        s.R = o; o += s.region;        // chunk buffers (prefix sums, V rows), then S, its factor, its inverse
        s.sD = o; o += n;
        s.sE = o; o += n;
        s.b1 = o; o += n;              // -q^
        s.sx = o; o += n;              // the ADMM x^, then the polished x^
        s.sn = o; o += s.n8;           // y_a
        s.r1 = o; o += n;              // residual, variables; the top half of A^ x^
        s.r2 = o; o += s.n8;           // residual, reduced rows
        s.ta = o; o += n;              // scratch n-vectors of the solves
        s.tb = o; o += n;
        s.tc = o; o += n;
        s.wv = o; o += s.n8;           // scratch reduced-row vector
        s.pre = o; o += n;             // prefix / suffix sums of the structured products
        s.dx = o; o += n;              // a refinement step's update; P^ x^ + q^ + A^' y^
        s.dn = o; o += s.n8;
        s.bu = o; o += s.n8;           // u^ of the reduced rows
        s.ym = o; o += 2 * n;          // y^ of all 2n rows
        s.pp = o; o += 2 * 128;        // the two halves of P^ x
        s.sg = o; o += s.n8;           // sign_a E_a of reduced row a
        s.ae = o; o += (s.n8 + 1) / 2; // (ints) element (k, r) of reduced row a
        s.posm = o; o += n;            // (ints, 2n) reduced row of QP row i, -1: inactive
        s.act = o; o += n;             // (ints, 2n) QP row of reduced row a
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
    double *const X = lds + S.X, *const R = lds + S.R;
    double *const sD = lds + S.sD, *const sE = lds + S.sE, *const b1 = lds + S.b1, *const sx = lds + S.sx;
    double *const sn = lds + S.sn, *const r1 = lds + S.r1, *const r2 = lds + S.r2, *const ta = lds + S.ta;
    double *const tb = lds + S.tb, *const tc = lds + S.tc, *const wvv = lds + S.wv, *const pre = lds + S.pre;
    double *const dx = lds + S.dx, *const dn = lds + S.dn, *const bu = lds + S.bu, *const ym = lds + S.ym;
    double *const pp = lds + S.pp, *const sg = lds + S.sg;
    int *const ae = (int *)(lds + S.ae), *const posm = (int *)(lds + S.posm), *const act = (int *)(lds + S.act);
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
        for (int e = t; e < n * L.ldp; e += kWgThreads) {
            const int i = e / L.ldp, k = e - i * L.ldp;
            if (k <= i) X[tri(i) + k] = k == i ? Ph[e] + a.delta : Ph[e];
        }
        if (t < n) {
            const double Dt = ops[L.D + t];
            sD[t] = Dt;
            sE[t] = ops[L.E + t];
            b1[t] = -((a.q[(size_t)b * n + t] * Dt) * c);
            sx[t] = a.xs[(size_t)b * n + t];
        }
        if (t < 16) s_K0[t] = ((t >> 2) < NU && (t & 3) < NU) ? ops[L.K0 + (t >> 2) * NU + (t & 3)] : 0.0;
        // ---- 1. the active set (l = -DBL_MAX: no lower-active row); row t's u^, z^, y^ stay in thread t
        double Er = 1.0, uh = 0.0, zh = 0.0, yh = 0.0;
        bool upp = false;
        if (t < m) {
            Er = ops[L.E + (t < n ? t : t - n)];
            uh = a.u[(size_t)b * m + t] * Er;
            zh = a.zs[(size_t)b * m + t];
            yh = a.ys[(size_t)b * m + t];
            upp = uh - zh < yh;
            ym[t] = yh;
        }
        const int mr = wg_reduced_rows(upp, m, t, s_cnt, posm, act);
        const WgKkt<NU> K{N, n, mr, t, X, R, sD, sE, sg, s_K0, ae, posm, pre, ta, tb, tc, wvv};

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
            if (t < mr) {
                const int row = act[t], e = row < n ? row : row - n;
                ae[t] = e;
                sg[t] = row < n ? sE[e] : -sE[e];
            }
            if (upp) bu[posm[t]] = uh;
            ok = wg_cholesky(X, n, t, s_piv);
            if (ok) wg_tri_invert(X, n, t, ta);
        }
        if (ok && mr > 0) ok = K.schur(S.rows, S.n8, a.delta, s_piv);

        double pri_p = nanv, dua_p = nanv, zp = 0.0, yp = 0.0;
        if (ok) {
            // ---- 3. the regularised solve, refined against the unregularised matrix
            K.solve(b1, bu, sx, sn);
            for (int it = 0; it < a.refine; it++) {  // s += K_reg^-1 (b - K s), K without delta
                wg_sym_mv_halves(Ph, L.ldp, n, sx, pp, t);
                __syncthreads();
                if (t < n) tc[t] = b1[t] - (pp[t] + pp[128 + t]);
                __syncthreads();
                K.apply_At(sn, tc, ta, r1);
                K.apply_A(sx, bu, wvv);
                if (t < mr) r2[t] = -wvv[t];  // (u^_a - A_a x^)
                __syncthreads();
                K.solve(r1, r2, dx, dn);
                if (t < n) sx[t] += dx[t];
                if (t < mr) sn[t] += dn[t];
                __syncthreads();
            }
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
    const int n = a->N * a->nu;
    if (a->nx <= 0 || a->nx > 12 || a->ny <= 0 || a->ny > 12 || a->N <= 0 || a->N > 32 || n > 128) return -1;
    if (a->batch <= 0) return 0;
    void (*kernel)(mpcq::MimoPolishArgs) = nullptr;
    switch (a->nu) {
    case 1: kernel = mpcq::polish_mimo_kernel<1>; break;
    case 2: kernel = mpcq::polish_mimo_kernel<2>; break;
    case 4: kernel = mpcq::polish_mimo_kernel<4>; break;
    default: return -1;
    }
    // (256: the kernel's few static words)
    return mpcq::launch_per_qp(kernel, *a, a->batch, mpcq::kWgThreads, mpcq_internal_mimo_polish_lds(n), 256, cus, s, err);
}

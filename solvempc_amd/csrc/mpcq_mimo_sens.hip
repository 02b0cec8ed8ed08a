// solvempc_amd/csrc/mpcq_mimo_sens.hip — active-set sensitivities of the last MIMO step (mpcq_mimo_step_device),
// one 256-thread workgroup per QP, the grid striding over the batch; fp64.
//
// The definition is mpcq_sens.hip's on the MIMO context's own data: the scaled iterate z^, y^ the
// step left, u^ = E u of the step's bounds, polish's rule (l = -DBL_MAX: upper-active rows only, ascending row
// index), and per right-hand side r < n_rhs the reduced KKT system [P^, A_a'; A_a, 0] [v^; w^] = [c D g_r; 0] by
// the Cholesky factor of H = P^ + delta I and of the Schur complement S = delta I + A_a H^-1 A_a', refined against
// the unregularised matrix; gq = -D v^, gu = E_a w^ / c scattered to the active rows.  One factorisation per QP
// serves every right-hand side.
//
// Storage: mpcq_wgkkt.h (the packed in-LDS factors of H and of S, inverted in place; the structured A^ products).
// Two packed triangles (66,048 B each at n = 128) and the vectors: 153,088 B at n = 128, one workgroup per CU.
//
// The chain rule of the step gains (q = Fx X + Fu U + Frs yref, u = W0 + Sbar X + Ku U) is the kernel's tail: gq
// and gu of a right-hand side are still in LDS, one thread per output element, sums in ascending row index.
// With a horizon reference per QP (mpcq_mimo_step_ref_vjp_device) the tail also forms dref = Fr' gq
// from Frs alone, one thread per output.
// No atomics anywhere: two calls give identical bits.  Nothing of the context is written.
#include "mpcq_internal.h"
#include "mpcq_wgkkt.h"

namespace mpcq {

constexpr int kMsThreads = kWgThreads;

// LDS carve-up (doubles) of mimo_sens_kernel for n variables
struct MimoSensShape {
    int n, n8, ntri, rows, region;
    int X, R, sD, sE, b1, sx, sn, r1, r2, ta, tb, tc, wv, pre, gq, gu, pp, sg, ae, posm, act, total;
    __host__ __device__ static MimoSensShape make(int n)
    {
        MimoSensShape s{};
        const WgTriShape w = WgTriShape::make(n);
        s.n = n; s.n8 = w.n8; s.ntri = w.ntri; s.rows = w.rows; s.region = w.region;
        int o = 0;
        s.X = o; o += s.ntri;          // H, its factor L, then X = L^-1 (packed lower)
        s.R = o; o += s.region;        // chunk buffers (prefix sums, V rows), then S, its factor, its inverse
        s.sD = o; o += n;
        s.sE = o; o += n;
        s.b1 = o; o += n;              // the scaled right-hand side
        s.sx = o; o += n;              // v^
        s.sn = o; o += s.n8;           // w^
        s.r1 = o; o += n;              // residual / update, variables
        s.r2 = o; o += s.n8;           // residual / update, reduced rows
        s.ta = o; o += n;              // scratch n-vectors of the solves
        s.tb = o; o += n;
        s.tc = o; o += n;
        s.wv = o; o += s.n8;           // scratch reduced-row vector
        s.pre = o; o += n;             // prefix / suffix sums of the structured products
        s.gq = o; o += n;              // this right-hand side's gq, gu (the chain rule reads them)
        s.gu = o; o += 2 * n;
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
__global__ __launch_bounds__(kMsThreads) void mimo_sens_kernel(MimoSensArgs a)
{
    extern __shared__ double lds[];
    __shared__ double s_K0[16], s_piv[2];
    __shared__ int s_cnt[4];
    const int t = threadIdx.x;
    const int N = a.N, nx = a.nx, ny = a.ny, n = N * NU, m = 2 * n;
    const MimoLayout L = MimoLayout::make(N, nx, NU, ny);
    const MimoSensShape S = MimoSensShape::make(n);
    double *const X = lds + S.X, *const R = lds + S.R;
    double *const sD = lds + S.sD, *const sE = lds + S.sE, *const b1 = lds + S.b1, *const sx = lds + S.sx;
    double *const sn = lds + S.sn, *const r1 = lds + S.r1, *const r2 = lds + S.r2, *const ta = lds + S.ta;
    double *const tb = lds + S.tb, *const tc = lds + S.tc, *const wvv = lds + S.wv, *const pre = lds + S.pre;
    double *const gqv = lds + S.gq, *const guv = lds + S.gu, *const pp = lds + S.pp, *const sg = lds + S.sg;
    int *const ae = (int *)(lds + S.ae), *const posm = (int *)(lds + S.posm), *const act = (int *)(lds + S.act);
    const int per = nx + NU + ny;                 // chain-rule outputs of one right-hand side

    for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
        __syncthreads();  // the previous QP of this workgroup is done with every buffer
        const double *ops = a.ops + (size_t)b * a.ops_stride;
        bool ok = a.status[b] == kSolved;  // (uniform)
        int mr = 0;
        if (ok) {
            // ---- 1. P^ + delta I (lower triangle, packed), D, E, K0
            const double *Ph = ops + L.Ph;
            for (int e = t; e < n * L.ldp; e += kMsThreads) {
                const int i = e / L.ldp, k = e - i * L.ldp;
                if (k <= i) X[tri(i) + k] = k == i ? Ph[e] + a.delta : Ph[e];
            }
            for (int e = t; e < n; e += kMsThreads) {
                sD[e] = ops[L.D + e];
                sE[e] = ops[L.E + e];
            }
            if (t < 16) s_K0[t] = ((t >> 2) < NU && (t & 3) < NU) ? ops[L.K0 + (t >> 2) * NU + (t & 3)] : 0.0;
            // ---- 2. the active set by polish's rule on the scaled iterate (l = -DBL_MAX: no lower-active row)
            bool upp = false;
            if (t < m) {
                const int e = t < n ? t : t - n;
                const double uh = a.u[(size_t)b * m + t] * ops[L.E + e];
                const double zh = a.zs[(size_t)b * m + t], yh = a.ys[(size_t)b * m + t];
                upp = uh - zh < yh;
            }
            mr = wg_reduced_rows(upp, m, t, s_cnt, posm, act);
            if (mr > n) ok = false;  // a degenerate bound pair (rows j and n + j both active): no sensitivity
        }
        const WgKkt<NU> K{N, n, mr, t, X, R, sD, sE, sg, s_K0, ae, posm, pre, ta, tb, tc, wvv};
        if (ok) {
            if (t < mr) {
                const int row = act[t], e = row < n ? row : row - n;
                ae[t] = e;
                sg[t] = row < n ? sE[e] : -sE[e];
            }
            // ---- 3. H = L L', X = L^-1
            ok = wg_cholesky(X, n, t, s_piv);
            if (ok) wg_tri_invert(X, n, t, ta);
        }
        // ---- 4. S = delta I + V'V, V = X A_a' formed kWgChunk rows at a time
        if (ok && mr > 0) ok = K.schur(S.rows, S.n8, a.delta, s_piv);

        for (int r = 0; r < a.n_rhs; r++) {
            const size_t br = (size_t)b * a.n_rhs + r;
            if (ok) {
                const double c = ops[L.cs], cinv = ops[L.cs + 1];
                if (t < n) {
                    const double gi = a.g ? a.g[br * n + t] : (t == r ? 1.0 : 0.0);
                    b1[t] = (gi * sD[t]) * c;
                }
                __syncthreads();
                K.solve(b1, nullptr, sx, sn);
                for (int it = 0; it < a.refine; it++) {  // s += K_reg^-1 (b - K s), K without delta
                    wg_sym_mv_halves(ops + L.Ph, L.ldp, n, sx, pp, t);  // P^ v^
                    __syncthreads();
                    if (t < n) tc[t] = b1[t] - (pp[t] + pp[128 + t]);
                    __syncthreads();
                    K.apply_At(sn, tc, ta, r1);
                    K.apply_A(sx, nullptr, wvv);
                    if (t < mr) r2[t] = -wvv[t];  // (the unregularised matrix: 0 - A_a v^)
                    __syncthreads();
                    K.solve(r1, r2, gqv, guv);  // (gqv, guv: free until the results below)
                    if (t < n) sx[t] += gqv[t];
                    if (t < mr) sn[t] += guv[t];
                    __syncthreads();
                }
                if (t < n) gqv[t] = -(sx[t] * sD[t]);
                if (t < m) {
                    const int e = t < n ? t : t - n, p = posm[t];
                    guv[t] = p >= 0 ? (sn[p] * sE[e]) * cinv : 0.0;
                }
            } else {
                if (t < n) gqv[t] = 0.0;
                if (t < m) guv[t] = 0.0;
            }
            __syncthreads();
            if (a.gq && t < n) a.gq[br * n + t] = gqv[t];
            if (a.gu && t < m) a.gu[br * m + t] = guv[t];
            // ---- the front end's chain rule: dX = Fx' gq + K' sum_{k < s_rows} (gt_k - gb_k),
            //      dU = Fu' gq + K0' sum_k (gb_k - gt_k), dyref = Frs' gq
            for (int o = t; o < per; o += kMsThreads) {
                double s = 0.0;
                if (o < nx) {
                    if (a.dX) {
                        for (int i = 0; i < n; i++) s += ops[L.Fx + i * nx + o] * gqv[i];
                        const int ks = a.s_rows < N ? a.s_rows : N;
                        for (int c = 0; c < NU; c++) {
                            double d = 0.0;
                            for (int k = 0; k < ks; k++) d += guv[k * NU + c] - guv[n + k * NU + c];
                            s += ops[L.K + c * nx + o] * d;
                        }
                        a.dX[br * nx + o] = s;
                    }
                } else if (o < nx + NU) {
                    const int oo = o - nx;
                    if (a.dU) {
                        for (int i = 0; i < n; i++) s += ops[L.Fu + i * NU + oo] * gqv[i];
                        for (int c = 0; c < NU; c++) {
                            double d = 0.0;
                            for (int k = 0; k < N; k++) d += guv[n + k * NU + c] - guv[k * NU + c];
                            s += ops[L.K0 + c * NU + oo] * d;
                        }
                        a.dU[br * NU + oo] = s;
                    }
                } else {
                    const int oo = o - nx - NU;
                    if (a.dyref) {
                        for (int i = 0; i < n; i++) s += ops[L.Frs + i * ny + oo] * gqv[i];
                        a.dyref[br * ny + oo] = s;
                    }
                }
            }
            // dref = Fr' gq from the row sums alone (F[j]: block row j of Frs): one thread per
            // (i, y), w_i = sum_{j<=i} F[N-1-i+j]' gq_j and w_{i-1} in ascending j, then their difference
            if (a.dref)
                for (int o = t; o < N * ny; o += kMsThreads) {
                    const int i = o / ny, y = o - i * ny;
                    const double *F = ops + L.Frs + y;
                    double w1 = 0.0, w0 = 0.0;
                    for (int j = 0; j <= i; j++)
                        for (int c = 0; c < NU; c++) w1 += F[((N - 1 - i + j) * NU + c) * ny] * gqv[j * NU + c];
                    for (int j = 0; j < i; j++)
                        for (int c = 0; c < NU; c++) w0 += F[((N - i + j) * NU + c) * ny] * gqv[j * NU + c];
                    a.dref[(br * N + i) * ny + y] = w1 - w0;
                }
            __syncthreads();  // (gqv, guv are the next right-hand side's scratch)
        }
        if (t == 0 && a.n_active) a.n_active[b] = ok ? mr : -1;
    }
}

}  // namespace mpcq

extern "C" size_t mpcq_internal_mimo_sens_lds(int n) { return 8 * (size_t)mpcq::MimoSensShape::make(n).total; }

extern "C" int mpcq_internal_mimo_sens_launch(const mpcq::MimoSensArgs *a, int cus, hipStream_t s, hipError_t *err)
{
    *err = hipSuccess;
    const int n = a->N * a->nu;
    if (a->nx <= 0 || a->nx > 12 || a->ny <= 0 || a->ny > 12 || a->N <= 0 || a->N > 32 || n > 128) return -1;
    if (a->n_rhs < 1 || a->n_rhs > 4) return -1;
    if (a->batch <= 0) return 0;
    void (*kernel)(mpcq::MimoSensArgs) = nullptr;
    switch (a->nu) {
    case 1: kernel = mpcq::mimo_sens_kernel<1>; break;
    case 2: kernel = mpcq::mimo_sens_kernel<2>; break;
    case 4: kernel = mpcq::mimo_sens_kernel<4>; break;
    default: return -1;
    }
    // (256: the kernel's few static words)
    return mpcq::launch_per_qp(kernel, *a, a->batch, mpcq::kMsThreads, mpcq_internal_mimo_sens_lds(n), 256, cus, s, err);
}

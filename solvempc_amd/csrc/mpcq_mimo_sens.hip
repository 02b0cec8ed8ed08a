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

// LDS carve-up (doubles) of mimo_sens_kernel for n variables: the reduced KKT system's, then the kernel's own
struct MimoSensShape {
    WgKktShape k;
    int gq, gu, total;
    __host__ __device__ static MimoSensShape make(int n)
    {
        MimoSensShape s{};
        s.k = WgKktShape::make(n);
        int o = s.k.total;
        s.gq = o; o += n;              // this right-hand side's gq, gu (the chain rule reads them)
        s.gu = o; o += 2 * n;
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
    WgKkt<NU> K(lds, S.k, s_K0, s_piv, N, t);
    double *const sD = K.sD, *const sE = K.sE, *const b1 = K.b1, *const sx = K.sx, *const sn = K.sn;
    double *const gqv = lds + S.gq, *const guv = lds + S.gu;
    const int *const posm = K.posm;
    const int per = nx + NU + ny;                 // chain-rule outputs of one right-hand side

    for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
        __syncthreads();  // the previous QP of this workgroup is done with every buffer
        const double *ops = a.ops + (size_t)b * a.ops_stride;
        bool ok = a.status[b] == kSolved;  // (uniform)
        int mr = 0;
        if (ok) {
            // ---- 1. P^ + delta I (lower triangle, packed), D, E, K0
            K.load(ops, L, a.delta);
            // ---- 2. the active set by polish's rule on the scaled iterate (l = -DBL_MAX: no lower-active row)
            bool upp = false;
            if (t < m)
                upp = mimo_upper_active(a.u[(size_t)b * m + t], ops[L.E + (t < n ? t : t - n)], a.zs[(size_t)b * m + t],
                                        a.ys[(size_t)b * m + t]);
            mr = wg_reduced_rows(upp, m, t, s_cnt, K.posm, K.act);
            if (mr > n) ok = false;  // a degenerate bound pair (rows j and n + j both active): no sensitivity
        }
        K.mr = mr;
        // ---- 3. H = L L', X = L^-1;  4. S = delta I + V'V, V = X A_a' formed kWgChunk rows at a time
        if (ok) ok = K.factor(a.delta);

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
                K.refine(ops + L.Ph, L.ldp, nullptr, a.refine, gqv, guv);  // (gqv, guv: free until the results below)
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
    if (!mpcq::mimo_shape_ok(a->N, a->nx, a->nu, a->ny) || a->n_rhs < 1 || a->n_rhs > 4) return -1;
    if (a->batch <= 0) return 0;
    return mpcq::mimo_with_nu(a->nu, [&](auto nu) {
        // (256: the kernel's few static words)
        return mpcq::launch_per_qp(mpcq::mimo_sens_kernel<decltype(nu)::value>, *a, a->batch, mpcq::kMsThreads,
                                   mpcq_internal_mimo_sens_lds(a->N * a->nu), 256, cus, s, err);
    });
}

// solvempc_amd/csrc/mpcq_sens.hip — active-set sensitivities of the last solve, one QP per 64-lane wave.
//
// For every QP that ended SOLVED, in fp64 whatever the context's dtype:
//   1. scaled data P^ = c D P D, A^ = E A D (WaveKkt::form, mpcq_wavekkt.h) and the bounds l^ = E l, u^ = E u, as
//      polish_kernel forms them;
//   2. the final scaled iterate z^, y^ from the warm state (type T, converted; x^ = W x' is not needed: the
//      rule reads z^ and y^ only);
//   3. OSQP's active sets by polish's rule, and A_red (mr rows): WaveKkt::active_sets;
//   4. the cotangent g (or e_0) scaled, g^ = c D g, and the regularised reduced KKT system
//      [P^ + delta I, A_red'; A_red, -delta I] [v^; w^] = [g^; 0] with `refine` steps of iterative refinement
//      against the unregularised matrix: WaveKkt::solve_refined;
//   5. gq = -D v^, and w = E_a w^ / c scattered into gl (lower-active rows) and gu (upper-active rows).
// Nothing of the context is written: the kernel only reads the warm state and the QP's data.
//
// Layout: mpcq_wavekkt.h's, as in mpcq_polish.hip.  A shared plant's P^, A^, the factor of H and G = A^ H^-1 A^'
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
#include "mpcq_wavekkt.h"

namespace mpcq {

__global__ __launch_bounds__(64) void sens_kernel(SensArgs a)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int n = a.n, m = a.m, nc = a.nc, mc = a.mc;
    const int ldS = m | 1, ld1 = (n | 1) > ldS ? (n | 1) : ldS;
    const bool ln = lane < n, lm = lane < m;
    WaveKkt K(n, m, a.delta, lane);
    double *const R1 = K.head(lds);         // m x ld1   V (row j: L^-1 a_j), then S of a shared plant
    double *const R2 = R1 + m * ld1;        // m x ldS   G of a shared plant, S of a per-plant context
    K.act = (int *)K.tail(R2 + m * ldS);
    double *const V = R1;
    double *const G = R2;
    K.S = a.shared ? R1 : R2;
    K.ldS = a.shared ? ld1 : ldS;
    const OpsLayout L = OpsLayout::make(nc, mc);
    bool have_plant = false, h_ok = false;

    for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
        __syncthreads();  // the previous QP of this workgroup is done with the staging buffers
        bool ok = a.status[b] == kSolved;  // (wave-uniform)
        const size_t pp = a.shared ? 0 : (size_t)b;
        const double *ops = a.ops + pp * a.ops_stride;
        K.no_active();
        double sx = 0.0, sn = 0.0;
        if (ok) {
            const double c = ops[L.cs];
            const double Ej = lm ? ops[L.E + lane] : 0.0;

            // ---- 1. scaled data, the factor of H and (shared plant) G, once per workgroup for a shared plant
            if (!a.shared || !have_plant) {
                h_ok = K.form(a.P + pp * n * n, a.A + pp * m * n, ops + L.D, ops + L.E, c);
                have_plant = true;
                if (a.shared && h_ok) {  // V = (L^-1 A^')' over every row, then G = V V'
                    if (lm) K.v_row(V, ld1, lane);
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
            const double zh = lm ? warm_state(a.zs, a.is_f32, (size_t)b * mc + lane) : 0.0;
            const double yh = lm ? warm_state(a.ys, a.is_f32, (size_t)b * mc + lane) : 0.0;
            K.active_sets(zh, yh, lo, up, nullptr);
        }

        // ---- 4. Schur complement and its factor: the gather delta I + G[act, act] for a shared plant
        if (ok) {
            if (a.shared) {
                if (K.lr)
                    for (int j = 0; j <= lane; j++)
                        K.S[lane * ld1 + j] = (j == lane ? a.delta : 0.0) + G[K.aj * ldS + K.act[j]];
                ok = K.factor_schur();
            } else {
                ok = K.schur_from_rows(V, ld1);
            }
        }

        // the cotangent g (or e_0) scaled, g^ = c D g, through the refined solve
        if (ok) {
            const double c = ops[L.cs];
            const double Di = ln ? ops[L.D + lane] : 0.0;
            const double gi = a.g ? (ln ? a.g[(size_t)b * n + lane] : 0.0) : (lane == 0 ? 1.0 : 0.0);
            K.solve_refined((gi * Di) * c, 0.0, a.refine, sx, sn);
            if (K.lr) K.mv[lane] = sn;
            __syncthreads();
        }

        // ---- 5. results: zeros and n_active = -1 where the QP did not end SOLVED (or a factor failed)
        const bool low = K.low, upp = K.upp;
        double gqv = 0.0, wv = 0.0;
        if (ok) {
            const double cinv = ops[L.cs + 1];
            gqv = ln ? -(sx * ops[L.D + lane]) : 0.0;
            if (low || upp) wv = (K.mv[K.pos] * ops[L.E + lane]) * cinv;
        }
        if (ln && a.gq) a.gq[(size_t)b * n + lane] = gqv;
        if (lm && a.gl) a.gl[(size_t)b * m + lane] = low ? wv : 0.0;
        if (lm && a.gu) a.gu[(size_t)b * m + lane] = upp ? wv : 0.0;
        if (lane == 0 && a.n_active) a.n_active[b] = ok ? K.mr : -1;
        if (lane < 2 && a.active) a.active[2 * (size_t)b + lane] = ok ? (lane ? K.mupp : K.mlow) : 0ull;
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
    return mpcq::launch_per_qp(mpcq::sens_kernel, *a, a->batch, 64, sens_lds(a->n, a->m), 0, cus, s, err);
}

extern "C" int mpcq_internal_sens_chain_launch(const mpcq::SensChainArgs *a, hipStream_t s)
{
    if (a->batch <= 0) return 0;
    const long long total = (long long)a->batch * (a->nx + 1 + a->n);
    const int grid = (int)std::min<long long>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(mpcq::sens_chain_kernel, dim3(grid), dim3(256), 0, s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

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
// Storage.  The context keeps no dense A: A^ = E [L (x) K0; -(L (x) K0)] D, so a reduced row is (sign, block k,
// component r) and every product with A_a or A_a' is a prefix / suffix sum over the horizon blocks and a K0 mix.
// H is factored in LDS as a packed lower triangle (row i at i (i + 1) / 2) and its factor is then inverted in
// place, X = L^-1: a solve with H is two triangular products (every row in parallel, no substitution chain), and
// row i of V = L^-1 A_a' depends on row i of X alone,
//     V(i, a) = sign_a E_a sum_c K0(r_a, c) sum_{j <= k_a} X(i, (j, c)) D(j, c),
// so V is never stored: it is formed 32 rows at a time in the region that later holds S, and S = delta I + V'V is
// accumulated in registers (thread (ty, tx) of a 16 x 16 grid owns the 8 x 8 tile at (8 ty, 8 tx), every index
// static) over the chunks.  S is then written as a packed triangle over the dead chunk buffers, factored and
// inverted in place like H.  Two packed triangles (66,048 B each at n = 128) and the vectors: 153,088 B at
// n = 128, one workgroup per CU.
//
// The chain rule of the step gains (q = Fx X + Fu U + Frs yref, u = W0 + Sbar X + Ku U) is the kernel's tail: gq
// and gu of a right-hand side are still in LDS, one thread per output element, sums in ascending row index.
// No atomics anywhere: two calls give identical bits.  Nothing of the context is written.
#include "mpcq_internal.h"

namespace mpcq {

constexpr int kMsThreads = 256;
constexpr int kMsChunk = 32;   // rows of V formed at a time (n = 128: 32 x (128 + 128) doubles fit S's region)

// LDS carve-up (doubles) of mimo_sens_kernel for n variables
struct MimoSensShape {
    int n, n8, ntri, rows, region;
    int X, R, sD, sE, b1, sx, sn, r1, r2, ta, tb, tc, wv, pre, gq, gu, pp, sg, ae, posm, act, total;
    __host__ __device__ static MimoSensShape make(int n)
    {
        MimoSensShape s{};
        s.n = n;
        s.n8 = (n + 7) & ~7;
        s.ntri = n * (n + 1) / 2;
        const int per_row = n + s.n8;  // one chunk row: the prefix sums (n) and the row of V (n8)
        int rows = s.ntri / per_row;
        rows = rows < 1 ? 1 : (rows > kMsChunk ? kMsChunk : rows);
        s.rows = rows;
        s.region = s.ntri > rows * per_row ? s.ntri : rows * per_row;
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

namespace {

__device__ __forceinline__ int tri(int i) { return (i * (i + 1)) >> 1; }

// sum of a[k] b[k] over k = k0, k0 + 2, ... < k1, in four partial sums: with one wave per SIMD nothing else hides
// the LDS latency, so four terms' reads are kept in flight together (a fixed order: the result is deterministic)
__device__ __forceinline__ double dot_step2(const double *a, const double *b, int k0, int k1)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int k = k0;
    for (; k + 6 < k1; k += 8) {
        const double a0 = a[k], a1 = a[k + 2], a2 = a[k + 4], a3 = a[k + 6];
        const double b0 = b[k], b1 = b[k + 2], b2 = b[k + 4], b3 = b[k + 6];
        s0 += a0 * b0;
        s1 += a1 * b1;
        s2 += a2 * b2;
        s3 += a3 * b3;
    }
    for (; k < k1; k += 2) s0 += a[k] * b[k];
    return (s0 + s1) + (s2 + s3);
}

// In-place lower Cholesky M = L L' of a packed lower triangle (row i at tri(i)), N <= 128: two threads per row
// (t >> 1, parity t & 1), left looking as mpcq_wavechol.h's wave_cholesky.  False (for every thread) when a pivot
// is not positive.  Ends with a barrier.
__device__ bool wg_cholesky(double *M, int N, int t, double *piv)
{
    const int row = t >> 1, h = t & 1;
    for (int k = 0; k < N; k++) {
        double v = 0.0;
        if (row >= k && row < N) {
            const double *ri = M + tri(row), *rk = M + tri(k);
            double s = dot_step2(ri, rk, h, k);
            s += __shfl_xor(s, 1);
            v = ri[k] - s;
            if (row == k && h == 0) piv[0] = v;
        }
        __syncthreads();
        const double d = piv[0];
        if (!(d > 0.0)) return false;  // (uniform: every thread reads the same pivot)
        const double lkk = sqrt(d), inv = 1.0 / lkk;
        if (row >= k && row < N && h == 0) M[tri(row) + k] = row == k ? lkk : v * inv;
        __syncthreads();
    }
    return true;
}

// In-place inverse of a packed lower-triangular matrix, X = L^-1, columns from the last to the first:
// X(j, j) = 1 / L(j, j), X(i, j) = -(sum_{j < k <= i} X(i, k) L(k, j)) X(j, j); tmp: N doubles.
__device__ void wg_tri_invert(double *M, int N, int t, double *tmp)
{
    const int row = t >> 1, h = t & 1;
    for (int j = N - 1; j >= 0; j--) {
        if (h == 0 && row >= j && row < N) tmp[row] = row == j ? 1.0 / M[tri(j) + j] : M[tri(row) + j];
        __syncthreads();
        if (row >= j && row < N) {
            const double xjj = tmp[j];
            const double *ri = M + tri(row);
            double s = dot_step2(ri, tmp, j + 1 + h, row + 1);
            s += __shfl_xor(s, 1);
            if (h == 0) M[tri(row) + j] = row == j ? xjj : -(s * xjj);
        }
        __syncthreads();
    }
}

// out = X in (lower triangular product); in != out.  Ends with a barrier.
__device__ __forceinline__ void tri_mv(const double *M, int N, const double *in, double *out, int t)
{
    const int row = t >> 1, h = t & 1;
    if (row < N) {
        const double *ri = M + tri(row);
        double s = dot_step2(ri, in, h, row + 1);
        s += __shfl_xor(s, 1);
        if (h == 0) out[row] = s;
    }
    __syncthreads();
}

// out = X' in; in != out.  Ends with a barrier.
__device__ __forceinline__ void tri_mv_t(const double *M, int N, const double *in, double *out, int t)
{
    const int col = t >> 1, h = t & 1;
    if (col < N) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int i = col + h;
        for (; i + 6 < N; i += 8) {  // (four terms in flight, as dot_step2)
            const double m0 = M[tri(i) + col], m1 = M[tri(i + 2) + col], m2 = M[tri(i + 4) + col], m3 = M[tri(i + 6) + col];
            s0 += m0 * in[i];
            s1 += m1 * in[i + 2];
            s2 += m2 * in[i + 4];
            s3 += m3 * in[i + 6];
        }
        for (; i < N; i += 2) s0 += M[tri(i) + col] * in[i];
        double s = (s0 + s1) + (s2 + s3);
        s += __shfl_xor(s, 1);
        if (h == 0) out[col] = s;
    }
    __syncthreads();
}

}  // namespace

template <int NU>
__global__ __launch_bounds__(kMsThreads) void mimo_sens_kernel(MimoSensArgs a)
{
    extern __shared__ double lds[];
    __shared__ double s_K0[16], s_piv[2];
    __shared__ int s_cnt[4];
    constexpr int LNU = NU == 4 ? 2 : (NU == 2 ? 1 : 0);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int N = a.N, nx = a.nx, ny = a.ny, n = N * NU, m = 2 * n;
    const MimoLayout L = MimoLayout::make(N, nx, NU, ny);
    const MimoSensShape S = MimoSensShape::make(n);
    double *const X = lds + S.X, *const R = lds + S.R;
    double *const sD = lds + S.sD, *const sE = lds + S.sE, *const b1 = lds + S.b1, *const sx = lds + S.sx;
    double *const sn = lds + S.sn, *const r1 = lds + S.r1, *const r2 = lds + S.r2, *const ta = lds + S.ta;
    double *const tb = lds + S.tb, *const tc = lds + S.tc, *const wvv = lds + S.wv, *const pre = lds + S.pre;
    double *const gqv = lds + S.gq, *const guv = lds + S.gu, *const pp = lds + S.pp, *const sg = lds + S.sg;
    int *const ae = (int *)(lds + S.ae), *const posm = (int *)(lds + S.posm), *const act = (int *)(lds + S.act);
    double *const preC = R;                       // [rows][n]   prefix sums of the chunk's rows of X D
    double *const Vc = R + S.rows * n;            // [rows][n8]  the chunk's rows of V
    const int n8 = S.n8;
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
            const unsigned long long mask = __ballot(upp);
            if (lane == 0) s_cnt[wv] = __popcll(mask);
            __syncthreads();
            int base = 0;
            for (int w = 0; w < 4; w++) {
                if (w < wv) base += s_cnt[w];
                mr += s_cnt[w];
            }
            const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
            if (t < m) posm[t] = upp ? pos : -1;
            if (upp) act[pos] = t;
            __syncthreads();
            if (mr > n) ok = false;  // a degenerate bound pair (rows j and n + j both active): no sensitivity
        }
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
        if (ok && mr > 0) {
            // ---- 4. S = delta I + V'V, V = X A_a' formed kMsChunk rows at a time
            const int ty = t >> 4, tx = t & 15;
            const bool mine = tx <= ty && 8 * ty < mr;
            double acc[8][8];
#pragma unroll
            for (int p = 0; p < 8; p++)
#pragma unroll
                for (int q = 0; q < 8; q++) acc[p][q] = 0.0;
            const int mr8 = (mr + 7) & ~7;
            for (int i0 = 0; i0 < n; i0 += S.rows) {
                const int rows = n - i0 < S.rows ? n - i0 : S.rows;
                for (int w = t; w < rows * NU; w += kMsThreads) {  // prefix sums over the blocks, per (row, component)
                    const int ii = w >> LNU, c = w & (NU - 1), i = i0 + ii;
                    const double *xi = X + tri(i);
                    double s = 0.0;
                    for (int kb = 0; kb < N; kb++) {
                        const int idx = kb * NU + c;
                        if (idx <= i) s += xi[idx] * sD[idx];
                        preC[ii * n + idx] = s;
                    }
                }
                __syncthreads();
                for (int w = t; w < rows * mr8; w += kMsThreads) {
                    const int ii = w / mr8, ar = w - ii * mr8;
                    double v = 0.0;
                    if (ar < mr) {
                        const int e = ae[ar], k = e >> LNU, r = e & (NU - 1);
                        double s = 0.0;
#pragma unroll
                        for (int c = 0; c < NU; c++) s += s_K0[r * 4 + c] * preC[ii * n + k * NU + c];
                        v = sg[ar] * s;
                    }
                    Vc[ii * n8 + ar] = v;
                }
                __syncthreads();
                if (mine) {
                    for (int ii = 0; ii < rows; ii++) {
                        const double *vr = Vc + ii * n8;
                        double va[8], vb[8];
#pragma unroll
                        for (int p = 0; p < 8; p++) {
                            va[p] = vr[8 * ty + p];
                            vb[p] = vr[8 * tx + p];
                        }
#pragma unroll
                        for (int p = 0; p < 8; p++)
#pragma unroll
                            for (int q = 0; q < 8; q++) acc[p][q] = __builtin_fma(va[p], vb[q], acc[p][q]);
                    }
                }
                __syncthreads();  // (the chunk buffers are rewritten)
            }
            if (mine) {
#pragma unroll
                for (int p = 0; p < 8; p++)
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        const int ra = 8 * ty + p, cb = 8 * tx + q;
                        if (ra < mr && cb <= ra) R[tri(ra) + cb] = ra == cb ? acc[p][q] + a.delta : acc[p][q];
                    }
            }
            __syncthreads();
            ok = wg_cholesky(R, mr, t, s_piv);
            if (ok) wg_tri_invert(R, mr, t, ta);
        }

        // out = A_a in (mr entries), minus sub where non-null
        auto apply_A = [&](const double *in, const double *sub, double *out) {
            if (t < n) {
                const int k = t >> LNU, c = t & (NU - 1);
                double s = 0.0;
                for (int j = 0; j <= k; j++) s += sD[j * NU + c] * in[j * NU + c];
                pre[t] = s;
            }
            __syncthreads();
            if (t < mr) {
                const int e = ae[t], k = e >> LNU, r = e & (NU - 1);
                double s = 0.0;
#pragma unroll
                for (int c = 0; c < NU; c++) s += s_K0[r * 4 + c] * pre[k * NU + c];
                s *= sg[t];
                out[t] = sub ? s - sub[t] : s;
            }
            __syncthreads();
        };
        // out = base - A_a' w (n entries; tmp: an n-vector)
        auto apply_At = [&](const double *w, const double *base, double *tmp, double *out) {
            if (t < n) {
                const int pt = posm[t], pb = posm[n + t];
                tmp[t] = sE[t] * ((pt >= 0 ? w[pt] : 0.0) - (pb >= 0 ? w[pb] : 0.0));
            }
            __syncthreads();
            if (t < n) {
                const int j = t >> LNU, r = t & (NU - 1);
                double s = 0.0;
                for (int k = j; k < N; k++) s += tmp[k * NU + r];
                pre[t] = s;
            }
            __syncthreads();
            if (t < n) {
                const int j = t >> LNU, c = t & (NU - 1);
                double s = 0.0;
#pragma unroll
                for (int r = 0; r < NU; r++) s += s_K0[r * 4 + c] * pre[j * NU + r];
                out[t] = base[t] - sD[t] * s;
            }
            __syncthreads();
        };
        // K_reg^-1 [p1; p2]: nu = S^-1 (A_a H^-1 p1 - p2), x = H^-1 (p1 - A_a' nu); p2 null: zero.
        // ox, on must differ from p1, p2 and the scratch vectors ta, tb, tc, wvv.
        auto kkt_solve = [&](const double *p1, const double *p2, double *ox, double *on) {
            tri_mv(X, n, p1, ta, t);
            tri_mv_t(X, n, ta, tb, t);
            apply_A(tb, p2, wvv);
            tri_mv(R, mr, wvv, tc, t);
            tri_mv_t(R, mr, tc, on, t);
            apply_At(on, p1, ta, tb);
            tri_mv(X, n, tb, ta, t);
            tri_mv_t(X, n, ta, ox, t);
        };

        for (int r = 0; r < a.n_rhs; r++) {
            const size_t br = (size_t)b * a.n_rhs + r;
            if (ok) {
                const double c = ops[L.cs], cinv = ops[L.cs + 1];
                if (t < n) {
                    const double gi = a.g ? a.g[br * n + t] : (t == r ? 1.0 : 0.0);
                    b1[t] = (gi * sD[t]) * c;
                }
                __syncthreads();
                kkt_solve(b1, nullptr, sx, sn);
                for (int it = 0; it < a.refine; it++) {  // s += K_reg^-1 (b - K s), K without delta
                    if (t < 2 * 128) {  // P^ v^: thread (column i, half of the rows), P^ read as symmetric
                        const int i = t & 127, hf = t >> 7, kh = (n + 1) >> 1;
                        const int k0 = hf * kh, k1 = k0 + kh < n ? k0 + kh : n;
                        double s = 0.0;
                        if (i < n)
                            for (int k = k0; k < k1; k++) s += ops[L.Ph + (size_t)k * L.ldp + i] * sx[k];
                        pp[t] = s;
                    }
                    __syncthreads();
                    if (t < n) tc[t] = b1[t] - (pp[t] + pp[128 + t]);
                    __syncthreads();
                    apply_At(sn, tc, ta, r1);
                    apply_A(sx, nullptr, wvv);
                    if (t < mr) r2[t] = -wvv[t];  // (the unregularised matrix: 0 - A_a v^)
                    __syncthreads();
                    kkt_solve(r1, r2, gqv, guv);  // (gqv, guv: free until the results below)
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

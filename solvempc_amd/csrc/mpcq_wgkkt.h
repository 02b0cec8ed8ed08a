// solvempc_amd/csrc/mpcq_wgkkt.h — the reduced KKT system of a MIMO QP on one 256-thread workgroup, fp64: what
// mpcq_mimo_sens.hip (the sensitivities) and mpcq_mimo_polish.hip (polish) share.
//
// Storage.  A MIMO context keeps no dense A: A^ = E [L (x) K0; -(L (x) K0)] D, so a reduced row is (sign, block k,
// component r) and every product with A_a or A_a' is a prefix / suffix sum over the horizon blocks and a K0 mix.
// H = P^ + delta I is factored in LDS as a packed lower triangle (row i at i (i + 1) / 2) and its factor is then
// inverted in place, X = L^-1: a solve with H is two triangular products (every row in parallel, no substitution
// chain), and row i of V = L^-1 A_a' depends on row i of X alone,
//     V(i, a) = sign_a E_a sum_c K0(r_a, c) sum_{j <= k_a} X(i, (j, c)) D(j, c),
// so V is never stored: it is formed kWgChunk rows at a time in the region that later holds S, and
// S = delta I + V'V is accumulated in registers (thread (ty, tx) of a 16 x 16 grid owns the 8 x 8 tile at
// (8 ty, 8 tx), every index static) over the chunks.  S is then written as a packed triangle over the dead chunk
// buffers, factored and inverted in place like H.
//
// Every sum runs in a fixed order and nothing here uses an atomic: equal inputs give identical bits.
#pragma once
#include "mpcq_internal.h"

namespace mpcq {

constexpr int kWgThreads = 256;
constexpr int kWgChunk = 32;   // rows of V formed at a time (n = 128: 32 x (128 + 128) doubles fit S's region)

// LDS carve-up (doubles) of the reduced KKT system for n variables: what both kernels keep there.  A kernel's own
// vectors follow from `total` on.  The two packed triangles are H's (ntri) and the region that holds the chunk buffers
// (`rows` rows of n prefix sums and n8 entries of V) and then S (at most n reduced rows).
struct WgKktShape {
    int n, n8, ntri, rows, region;
    int X, R, sD, sE, b1, sx, sn, r1, r2, ta, tb, tc, wv, pre, pp, sg, ae, posm, act, total;
    __host__ __device__ static WgKktShape make(int n)
    {
        WgKktShape s{};
        s.n = n;
        s.n8 = (n + 7) & ~7;
        s.ntri = n * (n + 1) / 2;
        const int per_row = n + s.n8;  // one chunk row: the prefix sums (n) and the row of V (n8)
        int rows = s.ntri / per_row;
        rows = rows < 1 ? 1 : (rows > kWgChunk ? kWgChunk : rows);
        s.rows = rows;
        s.region = s.ntri > rows * per_row ? s.ntri : rows * per_row;
        int o = 0;
        s.X = o; o += s.ntri;          // H, its factor L, then X = L^-1 (packed lower)
        s.R = o; o += s.region;        // chunk buffers (prefix sums, V rows), then S, its factor, its inverse
        s.sD = o; o += n;
        s.sE = o; o += n;
        s.b1 = o; o += n;              // the scaled right-hand side, variables
        s.sx = o; o += n;              // the solution, variables
        s.sn = o; o += s.n8;           // the solution, reduced rows
        s.r1 = o; o += n;              // residual, variables
        s.r2 = o; o += s.n8;           // residual, reduced rows
        s.ta = o; o += n;              // scratch n-vectors of the solves
        s.tb = o; o += n;
        s.tc = o; o += n;
        s.wv = o; o += s.n8;           // scratch reduced-row vector
        s.pre = o; o += n;             // prefix / suffix sums of the structured products
        s.pp = o; o += 2 * 128;        // the two halves of P^ x
        s.sg = o; o += s.n8;           // sign_a E_a of reduced row a
        s.ae = o; o += (s.n8 + 1) / 2; // (ints) element (k, r) of reduced row a
        s.posm = o; o += n;            // (ints, 2n) reduced row of QP row i, -1: inactive
        s.act = o; o += n;             // (ints, 2n) QP row of reduced row a
        s.total = o;
        return s;
    }
};

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
static __device__ bool wg_cholesky(double *M, int N, int t, double *piv)
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
static __device__ void wg_tri_invert(double *M, int N, int t, double *tmp)
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

// The reduced rows of a QP from its rows' flags (thread t < m: row t is active), ascending row index: posm[row] =
// its reduced row or -1, act[reduced row] = its QP row (m ints each).  Returns their number (uniform), which may
// exceed n: the callers refuse such a QP before anything indexed by a reduced row is touched.  cnt: 4 ints.
// Ends with a barrier.
__device__ __forceinline__ int wg_reduced_rows(bool upp, int m, int t, int *cnt, int *posm, int *act)
{
    const int lane = t & 63, wv = t >> 6;
    const unsigned long long mask = __ballot(upp);
    if (lane == 0) cnt[wv] = __popcll(mask);
    __syncthreads();
    int base = 0, mr = 0;
    for (int w = 0; w < 4; w++) {
        if (w < wv) base += cnt[w];
        mr += cnt[w];
    }
    const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
    if (t < m) posm[t] = upp ? pos : -1;
    if (upp) act[pos] = t;
    __syncthreads();
    return mr;
}

// y = P^ x for a P^ read as symmetric from the operator block (row stride ldp), in two halves: thread (column i,
// half hf of the rows) leaves its partial sum in pp[128 hf + i]; (P^ x)_i = pp[i] + pp[128 + i] after the caller's
// barrier.
__device__ __forceinline__ void wg_sym_mv_halves(const double *Ph, int ldp, int n, const double *x, double *pp, int t)
{
    if (t < 2 * 128) {
        const int i = t & 127, hf = t >> 7, kh = (n + 1) >> 1;
        const int k0 = hf * kh, k1 = k0 + kh < n ? k0 + kh : n;
        double s = 0.0;
        if (i < n)
            for (int k = k0; k < k1; k++) s += Ph[(size_t)k * ldp + i] * x[k];
        pp[t] = s;
    }
}

// The reduced KKT system [H, A_a'; A_a, -delta I] of one QP in the LDS of WgKktShape: its load from the operator
// block, its factors, the structured products with A_a (mr reduced rows; ae: element (k, r) of a reduced row, sg: its
// sign times E) and A_a' (posm: the reduced row of a QP row or -1), the solve by the two inverted factors X (of H)
// and R (of S), and its refinement.  K0: 4 x 4, zero padded; piv: 2 doubles.  mr is the caller's to set
// (wg_reduced_rows on posm, act) before factor().  Every member but load() ends with a barrier.
template <int NU>
struct WgKkt {
    static constexpr int LNU = NU == 4 ? 2 : (NU == 2 ? 1 : 0);
    int N, n, n8, rows_cap, t, mr = 0;
    double *X, *R, *sD, *sE, *b1, *sx, *sn, *r1, *r2, *ta, *tb, *tc, *wv, *pre, *pp, *sg, *K0, *piv;
    int *ae, *posm, *act;

    __device__ __forceinline__ WgKkt(double *lds, const WgKktShape &S, double *K0_, double *piv_, int N_, int t_)
        : N(N_), n(S.n), n8(S.n8), rows_cap(S.rows), t(t_), X(lds + S.X), R(lds + S.R), sD(lds + S.sD), sE(lds + S.sE),
          b1(lds + S.b1), sx(lds + S.sx), sn(lds + S.sn), r1(lds + S.r1), r2(lds + S.r2), ta(lds + S.ta), tb(lds + S.tb),
          tc(lds + S.tc), wv(lds + S.wv), pre(lds + S.pre), pp(lds + S.pp), sg(lds + S.sg), K0(K0_), piv(piv_),
          ae((int *)(lds + S.ae)), posm((int *)(lds + S.posm)), act((int *)(lds + S.act))
    {
    }

    // P^ + delta I (lower triangle, packed) into X, D, E and K0 from a plant's operator block.  No trailing barrier.
    __device__ __forceinline__ void load(const double *ops, const MimoLayout &L, double delta) const
    {
        const double *Ph = ops + L.Ph;
        for (int e = t; e < n * L.ldp; e += kWgThreads) {
            const int i = e / L.ldp, k = e - i * L.ldp;
            if (k <= i) X[tri(i) + k] = k == i ? Ph[e] + delta : Ph[e];
        }
        if (t < n) {
            sD[t] = ops[L.D + t];
            sE[t] = ops[L.E + t];
        }
        if (t < 16) K0[t] = ((t >> 2) < NU && (t & 3) < NU) ? ops[L.K0 + (t >> 2) * NU + (t & 3)] : 0.0;
    }

    // ae, sg of the mr <= n reduced rows, H = L L' and X = L^-1, then S (mr > 0).  False when a pivot is not positive.
    __device__ __forceinline__ bool factor(double delta) const
    {
        if (t < mr) {
            const int row = act[t], e = row < n ? row : row - n;
            ae[t] = e;
            sg[t] = row < n ? sE[e] : -sE[e];
        }
        bool ok = wg_cholesky(X, n, t, piv);
        if (ok) wg_tri_invert(X, n, t, ta);
        if (ok && mr > 0) ok = schur(delta);
        return ok;
    }

    // S = delta I + V'V into R (V = X A_a' formed `rows_cap` rows at a time in R's chunk buffers), factored and
    // inverted in place; mr > 0.  False when a pivot of S is not positive.
    __device__ __forceinline__ bool schur(double delta) const
    {
        double *const preC = R;                  // [rows][n]   prefix sums of the chunk's rows of X D
        double *const Vc = R + rows_cap * n;     // [rows][n8]  the chunk's rows of V
        const int ty = t >> 4, tx = t & 15;
        const bool mine = tx <= ty && 8 * ty < mr;
        double acc[8][8];
#pragma unroll
        for (int p = 0; p < 8; p++)
#pragma unroll
            for (int q = 0; q < 8; q++) acc[p][q] = 0.0;
        const int mr8 = (mr + 7) & ~7;
        for (int i0 = 0; i0 < n; i0 += rows_cap) {
            const int rows = n - i0 < rows_cap ? n - i0 : rows_cap;
            for (int w = t; w < rows * NU; w += kWgThreads) {  // prefix sums over the blocks, per (row, component)
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
            for (int w = t; w < rows * mr8; w += kWgThreads) {
                const int ii = w / mr8, ar = w - ii * mr8;
                double v = 0.0;
                if (ar < mr) {
                    const int e = ae[ar], k = e >> LNU, r = e & (NU - 1);
                    double s = 0.0;
#pragma unroll
                    for (int c = 0; c < NU; c++) s += K0[r * 4 + c] * preC[ii * n + k * NU + c];
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
                    if (ra < mr && cb <= ra) R[tri(ra) + cb] = ra == cb ? acc[p][q] + delta : acc[p][q];
                }
        }
        __syncthreads();
        const bool ok = wg_cholesky(R, mr, t, piv);
        if (ok) wg_tri_invert(R, mr, t, ta);
        return ok;
    }

    // out = A_a in (mr entries), minus sub where non-null
    __device__ __forceinline__ void apply_A(const double *in, const double *sub, double *out) const
    {
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
            for (int c = 0; c < NU; c++) s += K0[r * 4 + c] * pre[k * NU + c];
            s *= sg[t];
            out[t] = sub ? s - sub[t] : s;
        }
        __syncthreads();
    }

    // out = the top half of A^ in (n entries; the bottom half of the 2n rows is its negation)
    __device__ __forceinline__ void apply_A_rows(const double *in, double *out) const
    {
        if (t < n) {
            const int k = t >> LNU, c = t & (NU - 1);
            double s = 0.0;
            for (int j = 0; j <= k; j++) s += sD[j * NU + c] * in[j * NU + c];
            pre[t] = s;
        }
        __syncthreads();
        if (t < n) {
            const int k = t >> LNU, r = t & (NU - 1);
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < NU; c++) s += K0[r * 4 + c] * pre[k * NU + c];
            out[t] = sE[t] * s;
        }
        __syncthreads();
    }

    // D (L (x) K0)' tmp for tmp = E (w_top - w_bot), which the caller has left in tmp before a barrier: the
    // calling thread's entry (t < n), after the suffix sums over the blocks.  No trailing barrier.
    __device__ __forceinline__ double at_of(const double *tmp) const
    {
        if (t < n) {
            const int j = t >> LNU, r = t & (NU - 1);
            double s = 0.0;
            for (int k = j; k < N; k++) s += tmp[k * NU + r];
            pre[t] = s;
        }
        __syncthreads();
        double s = 0.0;
        if (t < n) {
            const int j = t >> LNU, c = t & (NU - 1);
#pragma unroll
            for (int r = 0; r < NU; r++) s += K0[r * 4 + c] * pre[j * NU + r];
        }
        return s;
    }

    // out = base - A_a' w (n entries; tmp: an n-vector)
    __device__ __forceinline__ void apply_At(const double *w, const double *base, double *tmp, double *out) const
    {
        if (t < n) {
            const int pt = posm[t], pb = posm[n + t];
            tmp[t] = sE[t] * ((pt >= 0 ? w[pt] : 0.0) - (pb >= 0 ? w[pb] : 0.0));
        }
        __syncthreads();
        const double s = at_of(tmp);
        if (t < n) out[t] = base[t] - sD[t] * s;
        __syncthreads();
    }

    // out = base + A^' y for all 2n rows' y (n entries; tmp: an n-vector)
    __device__ __forceinline__ void apply_At_rows(const double *y, const double *base, double *tmp, double *out) const
    {
        if (t < n) tmp[t] = sE[t] * (y[t] - y[n + t]);
        __syncthreads();
        const double s = at_of(tmp);
        if (t < n) out[t] = base[t] + sD[t] * s;
        __syncthreads();
    }

    // K_reg^-1 [p1; p2]: nu = S^-1 (A_a H^-1 p1 - p2), x = H^-1 (p1 - A_a' nu); p2 null: zero.
    // ox, on must differ from p1, p2 and the scratch vectors ta, tb, tc, wv.
    __device__ __forceinline__ void solve(const double *p1, const double *p2, double *ox, double *on) const
    {
        tri_mv(X, n, p1, ta, t);
        tri_mv_t(X, n, ta, tb, t);
        apply_A(tb, p2, wv);
        tri_mv(R, mr, wv, tc, t);
        tri_mv_t(R, mr, tc, on, t);
        apply_At(on, p1, ta, tb);
        tri_mv(X, n, tb, ta, t);
        tri_mv_t(X, n, ta, ox, t);
    }

    // `iters` steps of s += K_reg^-1 (b - K s) on s = (sx, sn), K without delta: b = (b1, sub), sub null: zero; P^ is
    // read as symmetric from the operator block (Ph, row stride ldp).  ux, un: the update's buffers, as solve()'s.
    __device__ __forceinline__ void refine(const double *Ph, int ldp, const double *sub, int iters, double *ux,
                                           double *un) const
    {
        for (int it = 0; it < iters; it++) {
            wg_sym_mv_halves(Ph, ldp, n, sx, pp, t);
            __syncthreads();
            if (t < n) tc[t] = b1[t] - (pp[t] + pp[128 + t]);
            __syncthreads();
            apply_At(sn, tc, ta, r1);
            apply_A(sx, sub, wv);
            if (t < mr) r2[t] = -wv[t];  // (sub - A_a x^)
            __syncthreads();
            solve(r1, r2, ux, un);
            if (t < n) sx[t] += ux[t];
            if (t < mr) sn[t] += un[t];
            __syncthreads();
        }
    }
};

}  // namespace mpcq

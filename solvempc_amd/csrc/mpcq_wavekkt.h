// solvempc_amd/csrc/mpcq_wavekkt.h — the regularised reduced KKT system of the one-QP-per-wave post-passes
// (mpcq_polish.hip, mpcq_sens.hip):
//
//     [P^ + delta I, A_red'; A_red, -delta I] [x; nu] = [r1; r2],    A_red = the active rows of A^,
//
// solved by the Cholesky factor of H = P^ + delta I and of the Schur complement S = delta I + A_red H^-1 A_red'
// (positive definite thanks to delta, whatever the rank of A_red), with iterative refinement against the
// unregularised matrix.  WaveKkt is a view of the workgroup's LDS carve-up plus the wave's active set; the
// kernels own the carve-up's kernel-specific regions (V, S, G) and everything that is not this linear algebra.
//
// Layout: matrices in LDS at odd fp64 strides (lane i walks row i: conflict-free; a broadcast row costs one
// access), vectors in registers, lane i holding element i (n <= 32 and m <= 64 both fit the 64 lanes).  A
// triangular solve keeps its vector in registers (mpcq_wavechol.h).  Every member function is called by the
// whole wave in uniform control flow: they contain barriers and shuffles.
#ifndef MPCQ_WAVEKKT_H
#define MPCQ_WAVEKKT_H

#include "mpcq_internal.h"
#include "mpcq_wavechol.h"

namespace mpcq {

namespace {

// one element of the warm state, stored in the context's dtype
__device__ __forceinline__ double warm_state(const void *p, bool is_f32, size_t i)
{
    return is_f32 ? (double)((const float *)p)[i] : ((const double *)p)[i];
}

struct WaveKkt {
    int n, m, ldn, lane;
    bool ln;       // lane < n
    double delta;
    // the carve-up: head() and tail() place the regions both kernels have, the kernel sets S
    double *Ph;    // n x ldn   P^
    double *Ah;    // m x ldn   A^
    double *Lh;    // n x ldn   Cholesky factor of H = P^ + delta I
    double *xv;    // n         staging (an n-vector read by every lane)
    double *mv;    // m         staging (an m-vector)
    double *dH;    // n         1 / diag of Lh
    double *dS;    // m         1 / diag of the factor of S
    int *act;      // m         row of A^ behind each reduced row
    double *S;     // mr x ldS  Schur complement, then its factor
    int ldS;
    // the QP's active sets (active_sets): A_red holds the lower-active rows followed by the upper-active ones
    bool low, upp;                   // this lane's row is lower- / upper-active
    unsigned long long mlow, mupp;   // the two sets as lane masks
    int mr, pos;                     // rows of A_red; this lane's row's place among them (low || upp)
    bool lr;                         // lane < mr: this lane owns reduced row `lane`, row aj of A^
    int aj;

    __device__ __forceinline__ WaveKkt(int n_, int m_, double delta_, int lane_)
        : n(n_), m(m_), ldn(n_ | 1), lane(lane_), ln(lane_ < n_), delta(delta_)
    {
        no_active();
    }
    // Ph, Ah, Lh from `p`; the first double after them
    __device__ __forceinline__ double *head(double *p)
    {
        Ph = p;
        Ah = Ph + n * ldn;
        Lh = Ah + m * ldn;
        return Lh + n * ldn;
    }
    // xv, mv, dH, dS from `p`; the first double after them (act is the kernel's to place: it ends the carve-up)
    __device__ __forceinline__ double *tail(double *p)
    {
        xv = p;
        mv = xv + n;
        dH = mv + m;
        dS = dH + n;
        return dS + m;
    }
    __device__ __forceinline__ void no_active()
    {
        low = upp = lr = false;
        mlow = mupp = 0ull;
        mr = pos = aj = 0;
    }

    // P^ = c D P D (symmetrised from P's upper triangle), A^ = E A D and the factor of H; false when H has a
    // non-positive pivot.  D, E: the plant's Ruiz scaling.
    __device__ __forceinline__ bool form(const double *P, const double *A, const double *D, const double *E, double c)
    {
        for (int e = lane; e < n * n; e += 64) {
            const int i = e / n, j = e - i * n;
            const double p = i <= j ? P[i * n + j] : P[j * n + i];  // upper triangle, as OSQP reads it
            const double v = (c * D[i]) * p * D[j];
            Ph[i * ldn + j] = v;
            Lh[i * ldn + j] = i == j ? v + delta : v;
        }
        for (int e = lane; e < m * n; e += 64) {
            const int j = e / n, k = e - j * n;
            Ah[j * ldn + k] = (E[j] * A[j * n + k]) * D[k];
        }
        __syncthreads();
        return wave_cholesky(Lh, ldn, n, dH, lane);
    }

    // OSQP's active sets (polish.c) from lane j's z^_j, y^_j and scaled bounds: lower-active when z^ - l^ < -y^,
    // else upper-active when u^ - z^ < y^ (exclusive by l <= u; enforced for the bounds' sake).  Fills act[] and,
    // when given, bact[]: the active bound of each reduced row.
    __device__ __forceinline__ void active_sets(double zh, double yh, double lo, double up, double *bact)
    {
        const bool lm = lane < m;
        low = lm && (zh - lo < -yh);
        upp = lm && !low && (up - zh < yh);
        mlow = __ballot(low);
        mupp = __ballot(upp);
        const unsigned long long below = (1ull << lane) - 1ull;
        const int n_low = __popcll(mlow);
        mr = n_low + __popcll(mupp);
        pos = low ? __popcll(mlow & below) : n_low + __popcll(mupp & below);
        if (low || upp) {
            act[pos] = lane;
            if (bact) bact[pos] = low ? lo : up;
        }
        __syncthreads();
        lr = lane < mr;
        aj = lr ? act[lane] : 0;
    }

    // row `lane` of V (stride ldv) = L^-1 (row `src` of A^)', by forward substitution
    __device__ __forceinline__ void v_row(double *V, int ldv, int src)
    {
        for (int i = 0; i < n; i++) {
            double v = Ah[src * ldn + i];
            for (int k = 0; k < i; k++) v -= Lh[i * ldn + k] * V[lane * ldv + k];
            V[lane * ldv + i] = v * dH[i];
        }
    }
    // the factor of S once its lower triangle is written; false on a non-positive pivot
    __device__ __forceinline__ bool factor_schur()
    {
        __syncthreads();
        return wave_cholesky(S, ldS, mr, dS, lane);
    }
    // S = delta I + V V' from the active rows, V = (L^-1 A_red')' in the kernel's region V, and its factor
    __device__ __forceinline__ bool schur_from_rows(double *V, int ldv)
    {
        if (lr) v_row(V, ldv, aj);
        __syncthreads();
        if (lr) {
            for (int j = 0; j <= lane; j++) {
                double v = j == lane ? delta : 0.0;
                for (int k = 0; k < n; k++) v += V[lane * ldv + k] * V[j * ldv + k];
                S[lane * ldS + j] = v;
            }
        }
        return factor_schur();
    }

    // K_reg^-1 [r1; r2]: nu = S^-1 (A_red H^-1 r1 - r2), x = H^-1 (r1 - A_red' nu)
    __device__ __forceinline__ void solve(double r1, double r2, double &sx, double &sn)
    {
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
    }
    // s = K_reg^-1 b, then `refine` steps s += K_reg^-1 (b - K s), K without delta
    __device__ __forceinline__ void solve_refined(double b1, double b2, int refine, double &sx, double &sn)
    {
        solve(b1, b2, sx, sn);
        for (int it = 0; it < refine; it++) {
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
            solve(r1, r2, dx, dn);
            sx += dx;
            sn += dn;
        }
    }
};

}  // namespace

}  // namespace mpcq
#endif  // MPCQ_WAVEKKT_H

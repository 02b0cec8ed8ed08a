// solvempc_amd/csrc/mpcq_mimo.hip — BASELINE config 4: per-plant MIMO condensed MPC (quad-rotor
// hover linearisations, n_x 12, n_u 4, N 30 => n = 120 variables, m = 240 rows), fp64.
//
// The reference builds the condensed QP of one SISO plant on the CPU (ModelPredictiveControlAPI.cpp
// :180-369) and hands it to OSQP (:51-64) every control step (:81-108).  Config 4 asks for that
// pipeline for 262,144 distinct MIMO plants per GPU; its formulation is oracle/mpc_mimo.h (every SISO
// scalar a block).  Two kernels:
//
//  * mimo_setup_kernel — one 1024-thread workgroup (16 waves) per plant, two per CU, everything in LDS
//    (under 80 KiB per plant at config 4: P as its packed upper triangle, regions shared by lifetime,
//    MimoSetupShape).  The horizon-stacked
//    contraction H = Su' Qbar Su is never formed densely: Su is block-Toeplitz (Su(i, j) = CS_{i-j},
//    CS_d = sum_{k<=d} Cd Ad^k Bd), so H(j1, j1+delta) is a prefix sum over the horizon,
//    G(delta, T) = sum_{t<=T} CS_{t+delta}' Q CS_t, and all of P costs N^2 nu^2 n_y multiply-adds
//    (0.18 MFLOP at config 4) instead of the dense 2 (N nu)^2 N n_y (10.4 MFLOP).  Then OSQP's Ruiz
//    equilibration (scale_data) on P (dense, LDS) and on A = [L (x) K0; -(L (x) K0)] (structured: its
//    row / column norms are prefix / suffix maxima over the horizon).  Writes P^ = c D P D and the
//    operator block of MimoLayout.
//
//  * mimo_solve_kernel — one 256-thread workgroup per QP, two per CU.  The reduced KKT matrix
//    M(rho) = P^ + sigma I + rho A^'A^ (A^'A^ from the suffix sums SW of the setup) lives in VGPRs as
//    4 x 16 blocks (thread (rg, cg): rows 4 rg.., columns 16 cg..) and is inverted in place by
//    Gauss-Jordan (SPD: no pivoting; one LDS row/column broadcast and one barrier per step).  An ADMM
//    iteration is then one GEMV with M^-1 (all 4 waves) plus O(n) vector work on wave 0 (lane k =
//    horizon block k), where A^ x and A^' w are lane prefix / suffix scans (DPP) and K0 products.  OSQP's adaptive rho
//    (adapt_rho at multiples of the interval) re-inverts M(rho_new) in place from P^ (global); the
//    dual residual's P^ x is carried through the KKT identity P^ x~ = rhs - sigma x~ - rho A^'A^ x~
//    (exact algebra; no P^ product per check).  Checks, certificates and statuses are OSQP v0.6's
//    (auxil.c), as in the tile kernel.
#include <cstdlib>

#include "mpcq_internal.h"
#include "mpcq_lane.h"
#include "mpcq_wave.h"

namespace mpcq {

// ----------------------------------------------------------------------------------------------
// setup: one 1024-thread workgroup (16 waves) per plant, two plants per CU; LDS carve (doubles), under
// 80 KiB per plant for config 4 (n 120).  P is symmetric and kept as its packed upper triangle (row i holds
// columns i .. n-1 at i n - i (i - 1) / 2), the diagonal nu x nu blocks of its construction in full (Dblk).
// Regions are shared by lifetime: X holds the recurrences' histories (QCA_d = Q Cd Ad^(d+1), Ad^d Bd, the
// powers Ad^1..Ad^4, then the Fx partial tiles) until P is built there, and after the last scan the Ruiz
// scalings D~, E~ take Dblk's place; Y holds CS until P is complete, then the Ruiz column partials.
struct MimoSetupShape {
    int N, nx, nu, ny, n, np;
    size_t P, Dblk, QCAh, ABh, Pw4, part, Dt, Et, CS, cm, wk;
    size_t Ad, Bd, Cd, Q, R, RD, K0, CA, Dv, Ev, red, sh, total;
    __host__ __device__ static size_t mx(size_t a, size_t b) { return a > b ? a : b; }
    __host__ __device__ static MimoSetupShape make(int N, int nx, int nu, int ny)
    {
        MimoSetupShape s{};
        s.N = N; s.nx = nx; s.nu = nu; s.ny = ny; s.n = N * nu;
        s.np = s.n * (s.n + 1) / 2;
        // region X
        s.QCAh = 0;
        s.ABh = s.QCAh + (size_t)N * ny * nx;
        s.Pw4 = s.ABh + (size_t)N * nx * nu;
        s.part = s.ABh;  // (Fx partial tiles: after the recurrences, over AB_d and the powers)
        const size_t xa = s.ABh + mx((size_t)N * nx * nu + (size_t)4 * nx * nx, (size_t)((s.n + 15) / 16) * 256);
        s.P = 0;
        s.Dblk = s.np;
        s.Dt = s.np;      // (after the scans: D~, E~ of the Ruiz passes where Dblk was)
        s.Et = s.np + s.n;
        const size_t xb = s.np + mx((size_t)N * nu * nu, (size_t)2 * s.n);
        size_t o = mx(xa, xb);
        // region Y
        s.CS = o;
        s.cm = o;         // (column-max partials, 8 row slices, once CS is dead)
        s.wk = o + 8 * 128;  // (A-norm block maxima, columns and rows)
        o += mx((size_t)N * ny * nu, (size_t)8 * 128 + 2 * 32 * 4);
        s.Ad = o; o += (size_t)nx * nx;
        s.Bd = o; o += (size_t)nx * nu;
        s.Cd = o; o += (size_t)ny * nx;
        s.Q = o; o += (size_t)ny * ny;
        s.R = o; o += (size_t)nu * nu;
        s.RD = o; o += (size_t)nu * nu;
        s.K0 = o; o += (size_t)nu * nu;
        s.CA = o; o += (size_t)ny * nx;
        s.Dv = o; o += s.n;
        s.Ev = o; o += s.n;
        s.red = o; o += 16;
        s.sh = o; o += 8;
        s.total = o;
        return s;
    }
};
// packed upper-triangle index of P(i, j), i <= j
__device__ __forceinline__ int pk_up(int i, int j, int n) { return i * n - (i * (i - 1)) / 2 + (j - i); }
__device__ __forceinline__ int pk(int i, int j, int n) { return i <= j ? pk_up(i, j, n) : pk_up(j, i, n); }

constexpr int kMimoSetupThreads = 1024;

// y = sum_k a[k * sa] b[k * sb] over k < len <= 12 (unrolled: the 12 loads are in flight together)
__device__ __forceinline__ double dot12(const double *a, int sa, const double *b, int sb, int len)
{
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int k = 0; k < 12; k += 2) {
        if (k < len) s0 = __builtin_fma(a[k * sa], b[k * sb], s0);
        if (k + 1 < len) s1 = __builtin_fma(a[(k + 1) * sa], b[(k + 1) * sb], s1);
    }
    return s0 + s1;
}

// One 16 x 16 tile (ti, tj) of C = A B with K <= 12 on v_mfma_f64_16x16x4f64, the operands read from LDS
// through index functors (entries outside M x K, K x N read as 0) and the valid outputs handed to `put`.
// The whole wave runs it.  Operand layouts as in the Fx product below: lane (g = lane >> 4, c = lane & 15)
// holds A(16 ti + c, 4 ks + g) and B(4 ks + g, 16 tj + c); accumulator v is C(16 ti + g + 4 v, 16 tj + c).
template <typename FA, typename FB, typename FC>
__device__ __forceinline__ void lds_mma_tile(int lane, int ti, int tj, int M, int N, int K, FA a_at, FB b_at, FC put)
{
    typedef double v4d __attribute__((ext_vector_type(4)));
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    const int c = lane & 15, g = lane >> 4, m = 16 * ti + c, nn = 16 * tj + c;
#pragma unroll
    for (int ks = 0; ks < 3; ks++) {
        const int k = 4 * ks + g;
        const double av = (m < M && k < K) ? a_at(m, k) : 0.0;
        const double bv = (nn < N && k < K) ? b_at(k, nn) : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const int mm = 16 * ti + g + 4 * v;
        if (mm < M && nn < N) put(mm, nn, acc[v]);
    }
}

__global__ __launch_bounds__(kMimoSetupThreads, 8) void mimo_setup_kernel(MimoSetupArgs a)
{
    extern __shared__ double sm[];
    const int pl = blockIdx.x;
    if (pl >= a.n_plants) return;
    const int t = threadIdx.x;
    constexpr int T = kMimoSetupThreads;
    const int N = a.N, nx = a.nx, nu = a.nu, ny = a.ny;
    const MimoSetupShape S = MimoSetupShape::make(N, nx, nu, ny);
    const int n = S.n;
    double *P = sm + S.P, *Dblk = sm + S.Dblk, *Ad = sm + S.Ad, *Bd = sm + S.Bd, *Cd = sm + S.Cd, *Q = sm + S.Q;
    double *R = sm + S.R, *RD = sm + S.RD, *K0 = sm + S.K0, *CA = sm + S.CA, *CS = sm + S.CS;
    double *Dv = sm + S.Dv, *Ev = sm + S.Ev, *Dt = sm + S.Dt, *Et = sm + S.Et, *cm = sm + S.cm, *wk = sm + S.wk;
    double *red = sm + S.red;
    const MimoLayout L = MimoLayout::make(N, nx, nu, ny);
    double *out = a.ops + (size_t)pl * L.total;
#define MPCQ_SSTAMP(k)                                                                              \
    do {                                                                                            \
        if (a.stamps && t == 0) a.stamps[(size_t)pl * 16 + (k)] = (long long)__builtin_amdgcn_s_memtime(); \
    } while (0)
    MPCQ_SSTAMP(0);
    if (a.stamps && t == 0) {  // (debug: where and when the workgroup ran, for co-residency)
        a.stamps[(size_t)pl * 16 + 12] = (long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
        a.stamps[(size_t)pl * 16 + 13] = (long long)__builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
        a.stamps[(size_t)pl * 16 + 14] = (long long)__builtin_amdgcn_s_memrealtime();
    }

    // ---- plant data -> LDS
    for (int e = t; e < nx * nx; e += T) Ad[e] = a.Ad[(size_t)pl * nx * nx + e];
    for (int e = t; e < nx * nu; e += T) Bd[e] = a.Bd[(size_t)pl * nx * nu + e];
    for (int e = t; e < ny * nx; e += T) Cd[e] = a.Cd[(size_t)pl * ny * nx + e];
    for (int e = t; e < ny * ny; e += T) Q[e] = a.Q[(size_t)pl * ny * ny + e];
    for (int e = t; e < nu * nu; e += T) {
        R[e] = a.R[(size_t)pl * nu * nu + e];
        RD[e] = a.RD[(size_t)pl * nu * nu + e];
        K0[e] = a.K0[(size_t)pl * nu * nu + e];
        out[L.K0 + e] = K0[e];
    }
    for (int e = t; e < nu * nx; e += T) out[L.K + e] = a.K[(size_t)pl * nu * nx + e];
    for (int e = t; e < nu; e += T) out[L.w0 + e] = a.w0[(size_t)pl * nu + e];
    __syncthreads();
    MPCQ_SSTAMP(1);

    // ---- setTransformations (:187-204): CS_d = sum_{k<=d} Cd Ad^k Bd (the distinct blocks of Su) and
    // QCA_d = Q Cd Ad^(d+1) (for Fx = 2 (Sx' Qbar Su)', :307).  By doubling: with Ad^2, Ad^4, Ad^8, Ad^16 at
    // hand, AB_(d + 2^k) = Ad^(2^k) AB_d and QCA_(d + 2^k) = QCA_d Ad^(2^k) give 2^k new steps per round, so
    // the N <= 32 steps take 5 rounds (one barrier each) instead of a step-by-step recurrence.
    double *QCAh = sm + S.QCAh;                         // QCA_d, [d][ny][nx]
    double *ABh = sm + S.ABh;                           // Ad^d Bd, [d][nx][nu]
    double *Pw = sm + S.Pw4;                            // Ad^(2^(s+1)) at Pw + s nx^2, s = 0..3
    double *QC = CA;                                    // Q Cd (ny x nx)
    const int ann = nx * nx, anu = nx * nu, ayx = ny * nx;
    // round r (r = 0..4) forms, each item a dot12 over LDS: Ad^(2^(r+1)) = (Ad^(2^r))^2 (r < 4), the AB steps
    // [2^r, 2^(r+1)) from [0, 2^r) (Ad^(2^r) times them; r = 0: AB_1 = Ad Bd) and the QCA steps ... likewise
    // one round behind (QCA_0 = QC Ad, QCA_1 = QC Ad^2 need QC: round 1)
    for (int e = t; e < ayx; e += T) QC[e] = dot12(Q + (e / nx) * ny, 1, Cd + e % nx, nx, ny);
    for (int e = t; e < anu; e += T) ABh[e] = Bd[e];
    // each round's products as 16 x 16 MFMA tiles, one wave per tile (Ad^(2h): one tile; the AB steps: the
    // columns of [AB_0 .. AB_(nab-1)] in tiles of 16; the QCA steps: the rows of [QCA_0; ..] in tiles of 16)
    const int lane = t & 63, wv = t >> 6;
    constexpr int NW = T / 64;
    for (int r = 0; r <= 5; r++) {
        __syncthreads();
        const int h = 1 << r;                          // AB: steps [h, 2h) from [0, h)
        const double *Ph = r == 0 ? Ad : Pw + (r - 1) * ann;  // Ad^h
        const int nab = N > h ? (N - h < h ? N - h : h) : 0;
        // QCA: round 1 forms steps 0, 1 from QC; round r >= 2 steps [2^(r-1), 2^r) from [0, 2^(r-1))
        const int hq = r >= 2 ? 1 << (r - 1) : 0;
        const int nqa = r == 1 ? (N < 2 ? N : 2) : (r >= 2 && N > hq ? (N - hq < hq ? N - hq : hq) : 0);
        const int ta = (r < 4 && ((2 << r) < N || r == 0)) ? 1 : 0;  // Ad^(2h): needed while 2h < N (Ad^2: QCA_1)
        const int tb = (nab * nu + 15) / 16;
        const int tc = r == 1 ? nqa : (nqa * ny + 15) / 16;
        for (int tile = wv; tile < ta + tb + tc; tile += NW) {  // (wave-uniform)
            if (tile < ta) {
                lds_mma_tile(lane, 0, 0, nx, nx, nx, [&](int i, int k) { return Ph[i * nx + k]; },
                             [&](int k, int c) { return Ph[k * nx + c]; },
                             [&](int i, int c, double v) { Pw[r * ann + i * nx + c] = v; });
            } else if (tile < ta + tb) {  // AB_(h + s) = Ad^h AB_s, column (s, c) of the stacked AB
                lds_mma_tile(lane, 0, tile - ta, nx, nab * nu, nx, [&](int i, int k) { return Ph[i * nx + k]; },
                             [&](int k, int col) { return ABh[(size_t)(col / nu) * anu + k * nu + col % nu]; },
                             [&](int i, int col, double v) { ABh[(size_t)(h + col / nu) * anu + i * nu + col % nu] = v; });
            } else if (r == 1) {          // QCA_0 = QC Ad, QCA_1 = QC Ad^2
                const int sdx = tile - ta - tb;
                const double *B = sdx ? Pw : Ad;
                lds_mma_tile(lane, 0, 0, ny, nx, nx, [&](int i, int k) { return QC[i * nx + k]; },
                             [&](int k, int c) { return B[k * nx + c]; },
                             [&](int i, int c, double v) { QCAh[(size_t)sdx * ayx + i * nx + c] = v; });
            } else {                      // QCA_(hq + s) = QCA_s Ad^hq (Ad^hq = Pw slot r - 2), row (s, i)
                const double *B = Pw + (r - 2) * ann;
                lds_mma_tile(lane, tile - ta - tb, 0, nqa * ny, nx, nx,
                             [&](int row, int k) { return QCAh[(size_t)(row / ny) * ayx + (row % ny) * nx + k]; },
                             [&](int k, int c) { return B[k * nx + c]; },
                             [&](int row, int c, double v) { QCAh[(size_t)(hq + row / ny) * ayx + (row % ny) * nx + c] = v; });
            }
        }
    }
    __syncthreads();
    for (int tile = wv; tile < (N * nu + 15) / 16; tile += NW)  // CS_d = Cd Ad^d Bd: Cd [AB_0 .. AB_(N-1)]
        lds_mma_tile(lane, 0, tile, ny, N * nu, nx, [&](int i, int k) { return Cd[i * nx + k]; },
                     [&](int k, int col) { return ABh[(size_t)(col / nu) * anu + k * nu + col % nu]; },
                     [&](int i, int col, double v) { CS[(size_t)(col / nu) * ny * nu + i * nu + col % nu] = v; });
    __syncthreads();
    for (int e = t; e < ny * nu; e += T) {  // prefix over the horizon
        double acc = 0.0;
        for (int d = 0; d < N; d++) {
            acc += CS[(size_t)d * ny * nu + e];
            CS[(size_t)d * ny * nu + e] = acc;
        }
    }
    __syncthreads();
    MPCQ_SSTAMP(2);
    // Fx_j = 2 sum_{d >= j} CS_{d-j}' QCA_d (block row j, nu x nx) on the matrix cores: Fx = sum_d A_d B_d
    // with A_d((j,r), kk) = CS_{d-j}(kk, r) (j <= d) and B_d = QCA_d, every horizon step accumulated in
    // the same 16 x 16 output tile (rows (j, r), columns c < nx <= 16); two waves per row tile split the
    // steps by parity and add through LDS.  (Q CS_d is formed where it is read, below: no LDS copy.)
    {
        typedef double v4d __attribute__((ext_vector_type(4)));
        const int lane = t & 63, wv = t >> 6, nt = (n + 15) >> 4, nks = (ny + 3) >> 2;
        double *part = sm + S.part;  // [tile][64 lanes][4], past the live histories
        const int ti = wv % 8, half = wv / 8;
        v4d acc = {0.0, 0.0, 0.0, 0.0};
        if (ti < nt) {
            const int g = ti * 16 + (lane & 15), j = g / nu, r = g % nu, cc = lane & 15;
            for (int d = half; d < N; d += 2) {
                for (int ks = 0; ks < nks; ks++) {
                    const int kk = ks * 4 + (lane >> 4);
                    const double av = (g < n && kk < ny && j <= d) ? CS[((size_t)(d - j) * ny + kk) * nu + r] : 0.0;
                    const double bv = (cc < nx && kk < ny) ? QCAh[((size_t)d * ny + kk) * nx + cc] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
                }
            }
            if (half == 1)
#pragma unroll
                for (int v = 0; v < 4; v++) part[((size_t)ti * 64 + lane) * 4 + v] = acc[v];
        }
        __syncthreads();
        if (ti < nt && half == 0) {
#pragma unroll
            for (int v = 0; v < 4; v++) {  // D(row = (lane >> 4) + 4 v, col = lane & 15)
                const int g = ti * 16 + (lane >> 4) + 4 * v, c = lane & 15;
                const double f = acc[v] + part[((size_t)ti * 64 + lane) * 4 + v];
                if (g < n && c < nx) out[L.Fx + (size_t)g * nx + c] = 2.0 * f;
            }
        }
    }
    __syncthreads();  // (the QCA history is dead: P is written below)
    MPCQ_SSTAMP(3);

    // ---- setH (:250-251): H(j1, j1+delta) = G(delta, N-1-j1-delta), G(delta, T) = sum_{t<=T}
    // CS_{t+delta}' Q CS_t; H1 = 2 ((N - max(j1, j2)) R + RD delta_{j1 j2} + H) (LL' Rbar LL has block
    // (j1, j2) = sum_{k >= max} R); P = (H1 + H1') / 2.  The block products are one GEMM on the matrix
    // cores, Z = CS' (Q CS) with CS = [CS_0 .. CS_{N-1}] (n_y x n): Z((i,r),(k,c)) = (CS_i' Q CS_k)(r,c),
    // needed for i >= k (delta = i - k, T = k) -- v_mfma_f64_16x16x4_f64 over the lower 16 x 16 tiles,
    // each product stored to its P slot (row block N-1-i, column block N-1-k); then one prefix scan over
    // T per (delta, r, c).
    {
        typedef double v4d __attribute__((ext_vector_type(4)));
        const int lane = t & 63, wv = t >> 6, nt = (n + 15) >> 4, nks = (ny + 3) >> 2;
        const int ntiles = nt * (nt + 1) / 2;
        for (int tile = wv; tile < ntiles; tile += T / 64) {  // wave-uniform: (ti >= tk) pairs
            int ti = 0, rem = tile;
            while (rem > ti) { rem -= ti + 1; ti++; }
            const int tk = rem;
            const int ga = ti * 16 + (lane & 15), gb = tk * 16 + (lane & 15);  // A row / B column of this lane
            const int ia = ga / nu, ra = ga % nu, kb = gb / nu, cb = gb % nu;
            v4d acc = {0.0, 0.0, 0.0, 0.0};
            for (int ks = 0; ks < nks; ks++) {
                const int kk = ks * 4 + (lane >> 4);
                const double av = (ga < n && kk < ny) ? CS[((size_t)ia * ny + kk) * nu + ra] : 0.0;
                const double bv = (gb < n && kk < ny) ? dot12(Q + kk * ny, 1, CS + (size_t)kb * ny * nu + cb, nu, ny) : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int v = 0; v < 4; v++) {  // D(row = (lane >> 4) + 4 v, col = lane & 15)
                const int gi = ti * 16 + (lane >> 4) + 4 * v, gk = gb;
                const int i = gi / nu, r = gi % nu, k = kb, c = cb;
                if (gi < n && gk < n && i >= k) {  // block (N-1-i, N-1-k): strictly upper, or a diagonal block
                    if (i > k) P[pk_up((N - 1 - i) * nu + r, (N - 1 - k) * nu + c, n)] = acc[v];
                    else Dblk[((N - 1 - i) * nu + r) * nu + c] = acc[v];
                }
            }
        }
    }
    __syncthreads();
    // Fu = 2 (R' + H(j, 0)) per block (:305, the .diagonal() quirk as blocks; Q symmetric): block j of
    // sum_u CS_u' Q CS_(u+j) is G(j, N-1-j)', the last value of the scan over delta = j below
    // P = (H1 + H1') / 2: an off-diagonal block's entry and its mirror come from the same scan, so the
    // thread stores their mean; a diagonal block's (r, c) and (c, r) come from two scans (Dblk, merged below)
    for (int it = t; it < N * nu * nu; it += T) {
        const int dl = it / (nu * nu), r = (it / nu) % nu, c = it % nu;
        double acc = 0.0;
        for (int tt = 0; tt + dl < N; tt++) {
            const int j2 = N - 1 - tt, j1 = j2 - dl;
            double *pe = dl ? P + pk_up(j1 * nu + r, j2 * nu + c, n) : Dblk + (j1 * nu + r) * nu + c;
            acc += *pe;
            const double rr = (double)(N - j2);  // N - max(j1, j2)
            const double up = 2.0 * (rr * R[r * nu + c] + (dl == 0 ? RD[r * nu + c] : 0.0) + acc);
            if (dl > 0) *pe = (up + 2.0 * (rr * R[c * nu + r] + acc)) / 2.0;  // H(j2, j1) = H(j1, j2)'
            else *pe = up;
        }
        out[L.Fu + (dl * nu + c) * nu + r] = 2.0 * (R[r * nu + c] + acc);
    }
    // Frs = -2 sum_{d <= N-1-j} (Q CS_d)' = -2 (Q PCS_(N-1-j))' with PCS_k = sum_{d<=k} CS_d (Fr = -2 (Qbar Su)',
    // :306, summed over the horizon blocks): CS becomes its prefix in place (setH has read it), then one
    // Q product per block
    for (int e = t; e < ny * nu; e += T) {
        double acc = 0.0;
        for (int d = 0; d < N; d++) {
            acc += CS[(size_t)d * ny * nu + e];
            CS[(size_t)d * ny * nu + e] = acc;
        }
    }
    __syncthreads();
    for (int it = t; it < n * ny; it += T) {
        const int j = it / (nu * ny), r = (it / ny) % nu, i = it % ny;
        out[L.Frs + it] = -2.0 * dot12(Q + i * ny, 1, CS + (size_t)(N - 1 - j) * ny * nu + r, nu, ny);
    }
    __syncthreads();
    MPCQ_SSTAMP(4);
    for (int e = t; e < N * nu * nu; e += T) {  // the diagonal blocks into the packed triangle
        const int j = e / (nu * nu), r = (e / nu) % nu, c = e % nu;
        if (r <= c) {
            const double v = Dblk[(j * nu + r) * nu + c];
            P[pk_up(j * nu + r, j * nu + c, n)] = r == c ? v : (v + Dblk[(j * nu + c) * nu + r]) / 2.0;
        }
    }
    for (int j = t; j < n; j += T) { Dv[j] = 1.0; Ev[j] = 1.0; }
    __syncthreads();
    MPCQ_SSTAMP(5);

    // ---- Ruiz equilibration + cost scaling (OSQP scale_data, q0 = 0 at setup, :22-23,38-39), with P
    // kept unscaled: the scaled matrix is c D P D, so its column norms are c D_j max_i D_i |P_ij| (two
    // read-only sweeps per pass instead of rescaling P).  A = [L (x) K0; -(L (x) K0)]:
    // |A^((k, r), (j, c))| = E(k,r) |K0(r, c)| D(j, c) for j <= k, and the bottom rows mirror the top
    // ones (same norms, so the same E): column norms are suffix maxima over k, row norms prefix maxima.
    const int sc = t >> 7, cj = t & 127;  // column sweeps: column cj, row slice sc (8 x 16 rows)
    auto colpart = [&](const double *Dv) {  // cm[sc][j] = max over the slice's rows of D_i |P_ij|
        if (cj < n) {
            double m0 = 0.0, m1 = 0.0;
            const int i0 = sc * 16;
            // packed index of (i, cj) walked down the column: +(n - i - 1) above the diagonal, +1 below
            int idx = pk(i0, cj, n);
#pragma unroll
            for (int ii = 0; ii < 16; ii += 2) {
                const int i = i0 + ii;
                const int idx1 = idx + (i < cj ? n - i - 1 : 1);
                if (i < n) m0 = fmax(m0, Dv[i] * fabs(P[idx]));
                if (i + 1 < n) m1 = fmax(m1, Dv[i + 1] * fabs(P[idx1]));
                idx = idx1 + (i + 1 < cj ? n - i - 2 : 1);
            }
            cm[sc * 128 + cj] = fmax(m0, m1);
        }
    };
    auto colfull = [&](int j) {
        double m = cm[j];
#pragma unroll
        for (int q = 1; q < 8; q++) m = fmax(m, cm[q * 128 + j]);
        return m;
    };
    // One column sweep per pass: pass p's Dt uses the norms of c_p D_p P D_p, and pass p-1's cost
    // scaling uses the norms of c_(p-1) D_p P D_p -- the same sweep.  Per pass: sweep | column norms,
    // A-norm block maxima, mean partials | cost scaling of the previous pass, Dt, Et, D, E | ...
    double cst = 1.0;
    double *Dc = Dv, *Dn = Dt, *Ec = Ev, *En = Et;  // current / next scaling (double-buffered)
    colpart(Dc);
    for (int pass = 0; pass <= a.scaling; pass++) {
        if (pass == 1) MPCQ_SSTAMP(8);
        __syncthreads();  // the sweep's partials; the previous pass's D, E
        if (pass == 1) MPCQ_SSTAMP(9);
        double cmt = 0.0;
        if (t < n) cmt = colfull(t);
        if ((t >> 6) >= 2 && (t >> 6) < 6) {  // waves 2..5 (no column of their own), wave 2 + c for component c,
                                                // lane k = block k: A-norm block maxima, suffix / prefix maxima
            const int k = t & 63, c = (t >> 6) - 2;  // (components >= nu are zero)
            double w0 = 0.0, w1 = 0.0;  // max_r E(k,r) |K0(r,c)|, max_q |K0(c,q)| D(k,q)
            if (k < N && c < nu)
                for (int q = 0; q < nu; q++) {
                    w0 = fmax(w0, Ec[k * nu + q] * fabs(K0[q * nu + c]));
                    w1 = fmax(w1, fabs(K0[c * nu + q]) * Dc[k * nu + q]);
                }
            // (inclusive max scans over lanes 0..31 of non-negative values; the whole wave is here)
            const auto maxd = [](double a, double b) { return fmax(a, b); };
            w0 = lane_suffix(w0, maxd, k);
            w1 = lane_prefix(w1, maxd, k);
            if (k < 32) {
                wk[k * 4 + c] = w0;
                wk[128 + k * 4 + c] = w1;
            }
        }
        if (pass > 0 && t < 128) {  // mean column norm of c D P D (previous pass's cost scaling)
            const double sv = wsum(t < n ? cst * Dc[t] * cmt : 0.0);
            if ((t & 63) == 0) red[t >> 6] = sv;
        }
        __syncthreads();
        if (pass > 0) {
            const double mean = (red[0] + red[1]) / n;
            const double qn = limit_scaling(0.0);  // |q^| = 0 at setup
            cst *= 1.0 / limit_scaling(fmax(mean, qn));
        }
        if (pass == a.scaling) break;
        if (pass == 1) MPCQ_SSTAMP(10);
        if (t < n) {
            const int bj = t / nu, c = t % nu;
            const double va = wk[bj * 4 + c], vr = wk[128 + bj * 4 + c];  // suffix / prefix maxima (wave 0)
            const double v = fmax(cst * Dc[t] * cmt, va * Dc[t]);
            Dn[t] = Dc[t] / sqrt(limit_scaling(v));
            En[t] = Ec[t] / sqrt(limit_scaling(Ec[t] * vr));
        }
        __syncthreads();
        if (pass == 1) MPCQ_SSTAMP(11);
        double *tp = Dc; Dc = Dn; Dn = tp;
        tp = Ec; Ec = En; En = tp;
        colpart(Dc);  // norms of the rescaled P
    }
    if (Dc != Dv) {  // the final scaling back in Dv, Ev
        if (t < n) {
            Dv[t] = Dc[t];
            Ev[t] = Ec[t];
        }
        __syncthreads();
    }
    MPCQ_SSTAMP(6);

    // ---- outputs: P^ = c D P D, D, E, c, SW (suffix sums of K0' diag(2 E_k^2) K0), row-type check
    for (int e = t; e < n * L.ldp; e += T) {
        const int i = e / L.ldp, j = e % L.ldp;
        const double v = j < n ? ((cst * Dv[i]) * P[pk(i, j, n)]) * Dv[j] : 0.0;
        out[L.Ph + e] = v;
        // osqp_setup fails on a non-convex P (the reference's ctor: solverFlag false); a diagonal of
        // P^ + sigma I that is not positive proves it.  (Necessary only: a P with positive diagonal
        // that is still indefinite surfaces as the QP's NON_CVX status at the solve's factorisation.)
        if (i == j && !(v + a.sigma > 0.0)) atomicOr(a.flags, 1);
    }
    for (int j = t; j < n; j += T) {
        out[L.D + j] = Dv[j];
        out[L.E + j] = Ev[j];
        // u0 = W0 (X = U = 0): a row with E w0 beyond OSQP_INFTY * MIN_SCALING would be free
        if (!(fabs(a.w0[(size_t)pl * nu + j % nu] * Ev[j]) < kInfty * kMinScaling)) atomicOr(a.flags, 2);
    }
    if (t < nu * nu && t / nu != t % nu && K0[t] != 0.0) atomicOr(a.flags, 4);  // off-diagonal K0
    if (t == 0) {
        out[L.cs] = cst;
        out[L.cs + 1] = 1.0 / cst;
    }
    // SW: the terms s_k (c1, c2) = sum_r K0(r, c1) K0(r, c2) 2 E(k, r)^2 of every k at once (into the Ruiz
    // partials' space, dead by now), then one suffix sum over k per (c1, c2), k descending as before
    for (int it = t; it < N * nu * nu; it += T) {
        const int k = it / (nu * nu), c1 = (it / nu) % nu, c2 = it % nu;
        double sk = 0.0;
        for (int r = 0; r < nu; r++) sk += K0[r * nu + c1] * K0[r * nu + c2] * (2.0 * Ev[k * nu + r] * Ev[k * nu + r]);
        cm[it] = sk;
    }
    __syncthreads();
    for (int it = t; it < nu * nu; it += T) {
        double acc = 0.0;
        for (int k = N - 1; k >= 0; k--) {
            acc += cm[k * nu * nu + it];
            out[L.SW + k * nu * nu + it] = acc;
        }
    }
    MPCQ_SSTAMP(7);
    if (a.stamps && t == 0) a.stamps[(size_t)pl * 16 + 15] = (long long)__builtin_amdgcn_s_memrealtime();
#undef MPCQ_SSTAMP
}

// ----------------------------------------------------------------------------------------------
// solve: one 256-thread workgroup (4 waves, one per SIMD) per QP, three QPs per CU (<= 168 VGPRs).
//
// M(rho) = P^ + sigma I + rho A^'A^ lives in VGPRs, padded to 128 x 128 with the identity: thread
// (rg, cg) = (t >> 3, t & 7) holds rows 4 rg .. 4 rg + 3, columns 16 cg .. 16 cg + 15 (64 doubles).
// Gauss-Jordan inverts it in place (SPD: no pivoting), one LDS row / column broadcast and one barrier
// per step; the step loop is unrolled by 16 so the owners of row / column k address their registers
// with compile-time indices.  An ADMM iteration is one GEMV with M^-1 (the 8-lane partial sums of a
// row group reduced by DPP) and O(n) vector work spread over the same four waves: wave c holds
// component c of every horizon block (lane k = block k), so A^ x and A^' w are lane prefix / suffix
// scans (DPP row shifts plus one cross-row readlane) followed by one LDS exchange for the K0 mix
// (one barrier per product).  Per-element state lives in LDS (component-major), so only the matrix
// holds registers across the loop.
constexpr int kMimoThreads = 256;
constexpr int kSegLd = 18;                  // padded stride of a 16-element segment (LDS banks)
constexpr int kSegN = 8 * kSegLd;
__device__ __forceinline__ int seg_of(int i) { return i + 2 * (i >> 4); }
constexpr int kMimoN = 128;       // n capacity

struct B4 {
    double v[4];
};

__device__ __forceinline__ B4 ldb(const double *arr, int lane)
{
    const double2 *p = (const double2 *)(arr + 4 * lane);
    const double2 u = p[0], w = p[1];
    return {{u.x, u.y, w.x, w.y}};
}
__device__ __forceinline__ void stb(double *arr, int lane, const B4 &x)
{
    double2 *p = (double2 *)(arr + 4 * lane);
    p[0] = make_double2(x.v[0], x.v[1]);
    p[1] = make_double2(x.v[2], x.v[3]);
}
// inclusive sums over lanes 0..31 (horizon blocks; N <= 32; lanes >= 32 are ignored by the callers; for the
// suffix, lanes N..31 must hold 0)
__device__ __forceinline__ double lane_psum(double v, int lane)
{
    return lane_prefix(v, [](double a, double b) { return a + b; }, lane);
}
__device__ __forceinline__ double lane_ssum(double v, int lane)
{
    return lane_suffix(v, [](double a, double b) { return a + b; }, lane);
}

#define MPCQ_MSTAMP(k, v)                                                                  \
    do {                                                                                   \
        if (a.stamps && t == 0) a.stamps[(size_t)blockIdx.x * 8 + (k)] = (long long)(v);  \
    } while (0)

#ifndef MPCQ_MIMO_WAVES_PER_EU
#define MPCQ_MIMO_WAVES_PER_EU 2  // two QPs per CU (256 VGPRs); 3 spills the matrix path
#endif
// Both solve kernels are one body, mpcq_mimo_solve.inc, included into each kernel with REF, ref and ref_stride
// defined by the kernel.  (A __forceinline__ function template on <NU, DK, REF> was tried first: the callee is
// simplified on its own before it is inlined, and the six mimo_solve_kernel instantiations came out with other scalar
// address arithmetic and register assignments than before.  Included, their ISA is what it was, instruction for
// instruction)
template <int NU, bool DK>
__global__ __launch_bounds__(kMimoThreads, MPCQ_MIMO_WAVES_PER_EU) void mimo_solve_kernel(MimoArgs a)
{
    constexpr bool REF = false;
    const double *const ref = nullptr;
    const long long ref_stride = 0;
#include "mpcq_mimo_solve.inc"
}

// mpcq_mimo_step_ref_device's kernel: MimoArgs as they are (yref unread), then the per-QP horizon reference.  REF: only
// the front end's Fr term differs.  Fr is block-Toeplitz, so with F[j] = block row j of the stored
// row sums Frs, F[N] = 0 and ref_N = 0,
//   (Fr ref)_j = sum_{d=0}^{N-1-j} F[N-1-d] (ref_{j+d} - ref_{j+d+1})   (summation by parts)
// from the operator block as it is.  A horizon-constant reference leaves exact zeros but the last difference, whose
// term is F[j] yref in mimo_solve_kernel's order.  All of it is prologue: nothing lives across the solve loop.
struct MimoRefArgs {
    MimoArgs a;
    const double *ref;      // [batch] ref_stride doubles apart, N*ny each (block i, then y)
    long long ref_stride;   // 0: one horizon reference shared by the batch
};
template <int NU, bool DK>
__global__ __launch_bounds__(kMimoThreads, MPCQ_MIMO_WAVES_PER_EU) void mimo_solve_ref_kernel(MimoRefArgs r)
{
    constexpr bool REF = true;
    const MimoArgs &a = r.a;
    const double *const ref = r.ref;
    const long long ref_stride = r.ref_stride;
#include "mpcq_mimo_solve.inc"
}

}  // namespace mpcq

extern "C" int mpcq_internal_mimo_setup_launch(const mpcq::MimoSetupArgs *a, hipStream_t s)
{
    const mpcq::MimoSetupShape S = mpcq::MimoSetupShape::make(a->N, a->nx, a->nu, a->ny);
    const size_t lds = 8 * S.total;
    if (!mpcq::mimo_shape_ok(a->N, a->nx, a->nu, a->ny) || lds > 160 * 1024) return -1;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void *)mpcq::mimo_setup_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess)
        return -2;
    hipLaunchKernelGGL(mpcq::mimo_setup_kernel, dim3(a->n_plants), dim3(mpcq::kMimoSetupThreads), lds, s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int mpcq_internal_mimo_solve_launch(const mpcq::MimoArgs *a, hipStream_t s)
{
    if (!mpcq::mimo_shape_ok(a->N, a->nx, a->nu, a->ny)) return -1;
    const dim3 grid(a->batch), block(mpcq::kMimoThreads);
    mpcq::mimo_with_nu(a->nu, [&](auto nu) {
        constexpr int U = decltype(nu)::value;
        if (a->diag_k0)
            hipLaunchKernelGGL((mpcq::mimo_solve_kernel<U, true>), grid, block, 0, s, *a);
        else
            hipLaunchKernelGGL((mpcq::mimo_solve_kernel<U, false>), grid, block, 0, s, *a);
    });
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// The same step with a horizon reference per QP (mimo_solve_ref_kernel): ref_stride 0 or >= N*ny, the caller's check
extern "C" int mpcq_internal_mimo_solve_ref_launch(const mpcq::MimoArgs *a, const double *ref, long long ref_stride,
                                                   hipStream_t s)
{
    if (!mpcq::mimo_shape_ok(a->N, a->nx, a->nu, a->ny)) return -1;
    if (!ref || (ref_stride != 0 && ref_stride < (long long)a->N * a->ny)) return -1;
    const dim3 grid(a->batch), block(mpcq::kMimoThreads);
    const mpcq::MimoRefArgs r{*a, ref, ref_stride};
    const size_t lds = 8 * (size_t)a->N * a->nu * a->ny;  // the plant's Frs, staged (<= 12 KiB; 20.3 KiB static)
    mpcq::mimo_with_nu(a->nu, [&](auto nu) {
        constexpr int U = decltype(nu)::value;
        if (a->diag_k0)
            hipLaunchKernelGGL((mpcq::mimo_solve_ref_kernel<U, true>), grid, block, lds, s, r);
        else
            hipLaunchKernelGGL((mpcq::mimo_solve_ref_kernel<U, false>), grid, block, lds, s, r);
    });
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// solvempc_amd/csrc/mpcq_setup_wave.hip — per-plant QP setup, one wavefront per plant, LDS-resident.
//
// Same computation and output block as setup_kernel (mpcq_setup.hip; osqp_setup behind
// OsqpEigen::Solver::initSolver, ModelPredictiveControlAPI.cpp:64), restructured for batches of
// distinct plants (BASELINE config 3): every matrix of the plant lives in LDS (fp64, row stride
// ld = odd, so column walks by lane are conflict-free), and the O(n^3) stages run wave-parallel:
//   * Ruiz passes: lane-per-column / lane-per-row maxima, element-parallel rescale; the cost
//     scaling sums run serially on lane 0 in the order of setup_kernel (same c bit for bit);
//   * Cholesky of P~ and the triangular solves for C = L^-1 G L^-T: right-looking, one column (or
//     row) step at a time, the trailing update spread over the 64 lanes;
//   * Jacobi on C with the round-robin ("circle") ordering: ne/2 disjoint rotations per round, each
//     2x2 block of C owned by one lane, so a round is two LDS passes and no serial rotation chain;
//   * W = L^-T V, W^-1 = V' L', and the operator products element-parallel into the global block.
// A single-wave workgroup makes every __syncthreads a wave-level ordering point (no s_barrier cost).
// Shapes n <= 32, m <= 64 (the wave kernel's capacities); larger plants use setup_kernel.
// setup_wave_keep_kernel / setup_inv_keep_kernel (mpcq_update_P_A_device, rescale = 0) are the same bodies with the
// scaling read from the plant's operator block instead of recomputed: the factor stage alone on new matrices.
#include "mpcq_internal.h"
#include "mpcq_lane.h"

#include <algorithm>

namespace mpcq {

// Debug hook (MPCQ_SETUP_PROF): per-plant shader-clock stamps at the stage boundaries.
#define MPCQ_STAMP(k) \
    do { if (a.prof && t == 0) a.prof[(size_t)pl * 16 + (k)] = (long long)clock64(); } while (0)

struct SetupWaveShape {
    int n, m, ne, ld;
    size_t Ph, Ah, L, T, C, V, Dv, Ev, Dt, Et, qh, rot, total;  // offsets in doubles
    __host__ __device__ static SetupWaveShape make(int n, int m)
    {
        SetupWaveShape s{};
        s.n = n; s.m = m;
        s.ne = n + (n & 1);      // Jacobi pads to an even order (the pad row/column stays decoupled)
        s.ld = s.ne + 1;         // odd stride
        size_t o = 0;
        s.Ph = o; o += (size_t)n * s.ld;
        s.Ah = o; o += (size_t)m * s.ld;
        s.L = o;  o += (size_t)n * s.ld;
        s.T = o;  o += (size_t)s.ne * s.ld;
        s.C = o;  o += (size_t)s.ne * s.ld;
        s.V = s.T;  // V reuses T's space: T (L^-1 G) is dead once C = T' is formed
        s.Dv = o; o += n;
        s.Ev = o; o += m;
        s.Dt = o; o += n;
        s.Et = o; o += m;
        s.qh = o; o += n;
        s.rot = o; o += 5 * 16;  // per pair: c, s, new app, new aqq, (p | q << 8)
        s.total = o + 8;         // + cost-scaling slots
        return s;
    }
};

// Whole-wave sum with every lane ending on the same bits (symmetric pairwise adds): DPP quad swaps and
// row mirrors, then the 16/32-lane swaps (VALU only; a __shfl_xor ladder is 12 LDS-path permutes).
__device__ inline double wave_sum(double v)
{
    return wave_reduce(v, [](double a, double b) { return a + b; });
}

// Pair u of round r of the circle ordering on ne (even) indices.
__device__ inline void circle_pair(int r, int u, int ne, int &p, int &q)
{
    const int k = ne - 1;
    if (u == 0) { p = r; q = k; }
    else { p = (r + u) % k; q = (r - u + k) % k; }
}

// OSQP scale_data (Ruiz equilibration + cost normalisation) and set_rho_vec's constraint typing, on
// the LDS-resident plant (one wave).  On exit Ph, Ah hold P^, A^; Dv, Ev the scalings; Et the rho
// scale of each row (0 free, 1 inequality, RHO_EQ_OVER_RHO_INEQ equality); returns c.
__device__ double ruiz_and_types(const SetupArgs &a, int pl, int t, int n, int m, int mc, int ld, double *Ph,
                                 double *Ah, double *Dv, double *Ev, double *Dt, double *Et, double *qh, double *sh,
                                 int *ctype)
{
    const double *l0 = a.l0 + (size_t)pl * m;
    const double *u0 = a.u0 + (size_t)pl * m;
    // ---- Ruiz equilibration + cost normalisation (OSQP scale_data).  A pass's cost factor ct is not
    // swept over P^ on its own: it stays pending (cp) and is applied inside the next pass's column
    // norms (max |cp P| = cp max |P|: rounding is monotone) and D-scaling, or by one sweep after the
    // last pass, so every P^ element is rounded exactly as in the eager order.
    double cp = 1.0;
    for (int it = 0; it < a.scaling; it++) {
        if (t < n) {
            double vp = 0.0, va = 0.0;
            for (int i = 0; i < n; i++) vp = fmax(vp, fabs(Ph[i * ld + t]));
            for (int i = 0; i < m; i++) va = fmax(va, fabs(Ah[i * ld + t]));
            Dt[t] = 1.0 / sqrt(limit_scaling(fmax(cp * vp, va)));
        }
        for (int i = t; i < m; i += 64) {
            double v = 0.0;
            for (int j = 0; j < n; j++) v = fmax(v, fabs(Ah[i * ld + j]));
            Et[i] = 1.0 / sqrt(limit_scaling(v));
        }
        __syncthreads();
        for (int e = t; e < n * n; e += 64) {
            const int i = e / n, k = e % n;
            Ph[i * ld + k] = (Dt[i] * (Ph[i * ld + k] * cp)) * Dt[k];
        }
        for (int e = t; e < m * n; e += 64) {
            const int i = e / n, k = e % n;
            Ah[i * ld + k] = (Et[i] * Ah[i * ld + k]) * Dt[k];
        }
        if (t < n) { qh[t] *= Dt[t]; Dv[t] *= Dt[t]; }
        for (int i = t; i < m; i += 64) Ev[i] *= Et[i];
        __syncthreads();
        if (t < n) {
            double v = 0.0;
            for (int i = 0; i < n; i++) v = fmax(v, fabs(Ph[i * ld + t]));
            Dt[t] = v;
        }
        __syncthreads();
        if (t == 0) {
            double mean = 0.0, qn = 0.0;
            for (int j = 0; j < n; j++) mean += Dt[j];
            mean /= n;
            for (int j = 0; j < n; j++) qn = fmax(qn, fabs(qh[j]));
            qn = limit_scaling(qn);
            const double ct = 1.0 / limit_scaling(fmax(mean, qn));
            sh[1] = ct;
            sh[0] *= ct;
        }
        __syncthreads();
        cp = sh[1];  // (sh[1] is next written three barriers on)
        if (t < n) qh[t] *= cp;
    }
    if (a.scaling > 0) {
        for (int e = t; e < n * n; e += 64) Ph[(e / n) * ld + e % n] *= cp;
        __syncthreads();
    }
    const double cost = sh[0];

    // ---- constraint types from the scaled setup bounds (OSQP set_rho_vec); Et <- rscale
    for (int i = t; i < m; i += 64) {
        const double lo = l0[i] * Ev[i], up = u0[i] * Ev[i];
        int ty;
        double rs;
        if (lo < -kInfty * kMinScaling && up > kInfty * kMinScaling) { ty = -1; rs = 0.0; }
        else if (up - lo < kRhoTol) { ty = 1; rs = kRhoEqOverIneq; }
        else { ty = 0; rs = 1.0; }
        ctype[i] = ty;
        Et[i] = rs;
        if (ty != 0) atomicOr(a.flags, 2);
    }
    for (int i = m + t; i < mc; i += 64) ctype[i] = 0;
    __syncthreads();

    return cost;
}

// The scaling stage of the keep-scaling kernels (mpcq_update_P_A_device, rescale = 0), in place of the data
// load and ruiz_and_types: D, E, c and the rows' rho scales are those the plant's operator block holds (read,
// never rewritten: they and ctype keep their bits), and the new matrices are scaled once,
//   P^_ij = (D_i (c P_ij)) D_j,   A^_ij = (E_i A_ij) D_j     (left to right: three and two roundings),
// P symmetrised from its upper triangle first.  On exit Ph, Ah, Dv, Ev and Et (rscale) are as ruiz_and_types
// leaves them.
__device__ inline void load_kept_scaling(const SetupArgs &a, int pl, int t, int n, int m, int ld, const double *blk,
                                         const OpsLayout &Lo, double *Ph, double *Ah, double *Dv, double *Ev, double *Et)
{
    const double *P = a.P + (size_t)pl * n * n;
    const double *A = a.A + (size_t)pl * m * n;
    for (int j = t; j < n; j += 64) Dv[j] = blk[Lo.D + j];
    for (int i = t; i < m; i += 64) { Ev[i] = blk[Lo.E + i]; Et[i] = blk[Lo.rscale + i]; }
    const double c = blk[Lo.cs];
    __syncthreads();
    for (int e = t; e < n * n; e += 64) {
        const int i = e / n, j = e % n;
        const double p = (i <= j) ? P[i * n + j] : P[j * n + i];
        Ph[i * ld + j] = (Dv[i] * (c * p)) * Dv[j];
    }
    for (int e = t; e < m * n; e += 64) {
        const int i = e / n, j = e % n;
        Ah[i * ld + j] = (Ev[i] * A[e]) * Dv[j];
    }
    __syncthreads();
}

// KEEP: the keep-scaling form (setup_wave_keep_kernel): load_kept_scaling for the stages up to ruiz_and_types,
// the same factor stage, and nothing of the scaling written back.
template <bool KEEP>
__device__ __forceinline__ void setup_wave_body(const SetupArgs &a)
{
    extern __shared__ double sm[];
    const int pl = blockIdx.x;
    if (pl >= a.n_plants) return;
    const int t = threadIdx.x;
    const int n = a.n, m = a.m, nc = a.nc, mc = a.mc;
    const SetupWaveShape S = SetupWaveShape::make(n, m);
    const int ld = S.ld, ne = S.ne;
    double *Ph = sm + S.Ph, *Ah = sm + S.Ah, *L = sm + S.L, *Tm = sm + S.T, *C = sm + S.C, *V = sm + S.V;
    double *Dv = sm + S.Dv, *Ev = sm + S.Ev, *Dt = sm + S.Dt, *Et = sm + S.Et, *qh = sm + S.qh;
    double *rot = sm + S.rot, *sh = sm + S.total - 8;

    const double *P = a.P + (size_t)pl * n * n;
    const double *q0 = a.q0 + (size_t)pl * n;
    const double *A = a.A + (size_t)pl * m * n;
    const OpsLayout Lo = OpsLayout::make(nc, mc);
    double *out = a.ops + (size_t)pl * Lo.total;
    int *ctype = a.ctype + (size_t)pl * mc;

    MPCQ_STAMP(0);
    double cost = 1.0;
    if constexpr (KEEP) {
        load_kept_scaling(a, pl, t, n, m, ld, out, Lo, Ph, Ah, Dv, Ev, Et);
    } else {
        // ---- data (osqp-eigen keeps the upper triangle of the Hessian)
        for (int e = t; e < n * n; e += 64) {
            const int i = e / n, j = e % n;
            Ph[i * ld + j] = (i <= j) ? P[i * n + j] : P[j * n + i];
        }
        for (int e = t; e < m * n; e += 64) Ah[(e / n) * ld + e % n] = A[e];
        for (int j = t; j < n; j += 64) { qh[j] = q0[j]; Dv[j] = 1.0; }
        for (int i = t; i < m; i += 64) Ev[i] = 1.0;
        if (t == 0) sh[0] = 1.0;
        __syncthreads();

        MPCQ_STAMP(1);
        cost = ruiz_and_types(a, pl, t, n, m, mc, ld, Ph, Ah, Dv, Ev, Dt, Et, qh, sh, ctype);
    }
    MPCQ_STAMP(3);
    // ---- P~ = P^ + sigma I + RHO_MIN sum_free a a' (into L), G = sum rscale a a' (into Tm)
    for (int e = t; e < n * n; e += 64) {
        const int i = e / n, k = e % n;
        double pt = Ph[i * ld + k] + (i == k ? a.sigma : 0.0), g = 0.0;
        for (int r = 0; r < m; r++) {
            const double aa = Ah[r * ld + i] * Ah[r * ld + k];
            const double rs = Et[r];
            if (rs == 0.0) pt += kRhoMin * aa;
            else g += rs * aa;
        }
        L[i * ld + k] = pt;
        Tm[i * ld + k] = g;
    }
    __syncthreads();

    MPCQ_STAMP(4);
    // ---- Cholesky P~ = L L' in place (right-looking; upper triangle zeroed at the end)
    int fail = 0;
    for (int j = 0; j < n; j++) {
        double d = L[j * ld + j];
        if (!(d > 0.0)) { fail = 1; d = 1.0; }
        d = sqrt(d);
        __syncthreads();
        if (t == 0) L[j * ld + j] = d;
        for (int i = j + 1 + t; i < n; i += 64) L[i * ld + j] /= d;
        __syncthreads();
        const int w = n - j - 1;  // trailing lower triangle rows/cols j+1..n-1
        for (int e = t; e < w * w; e += 64) {
            const int i = j + 1 + e / w, k = j + 1 + e % w;
            if (k <= i) L[i * ld + k] -= L[i * ld + j] * L[k * ld + j];
        }
        __syncthreads();
    }
    for (int e = t; e < n * n; e += 64) {
        const int i = e / n, k = e % n;
        if (k > i) L[i * ld + k] = 0.0;
    }
    __syncthreads();

    MPCQ_STAMP(5);
    // ---- C = L^-1 G L^-T: Tm <- L^-1 G (row steps), C <- Tm', C <- L^-1 C, symmetrise
    for (int i = 0; i < n; i++) {
        const double li = L[i * ld + i];
        if (t < n) Tm[i * ld + t] /= li;
        __syncthreads();
        for (int e = t; e < (n - i - 1) * n; e += 64) {
            const int r = i + 1 + e / n, c = e % n;
            Tm[r * ld + c] -= L[r * ld + i] * Tm[i * ld + c];
        }
        __syncthreads();
    }
    for (int e = t; e < ne * ne; e += 64) {
        const int i = e / ne, k = e % ne;
        C[i * ld + k] = (i < n && k < n) ? Tm[k * ld + i] : 0.0;
    }
    __syncthreads();
    for (int e = t; e < ne * ne; e += 64) {  // (V aliases Tm)
        const int i = e / ne, k = e % ne;
        V[i * ld + k] = (i == k) ? 1.0 : 0.0;
    }
    __syncthreads();
    for (int i = 0; i < n; i++) {
        const double li = L[i * ld + i];
        if (t < n) C[i * ld + t] /= li;
        __syncthreads();
        for (int e = t; e < (n - i - 1) * n; e += 64) {
            const int r = i + 1 + e / n, c = e % n;
            C[r * ld + c] -= L[r * ld + i] * C[i * ld + c];
        }
        __syncthreads();
    }
    for (int e = t; e < n * n; e += 64) {
        const int i = e / n, k = e % n;
        if (i < k) {
            const double v = 0.5 * (C[i * ld + k] + C[k * ld + i]);
            C[i * ld + k] = v;
            C[k * ld + i] = v;
        }
    }
    __syncthreads();

    MPCQ_STAMP(6);
    // ---- parallel-ordering Jacobi: C = V diag(lambda) V'
    const int np = ne / 2, nblk = np * (np + 1) / 2;
    // Block b = t of the upper-triangular pair grid, decoded once (the grid is the same every round).
    const int dq64 = np > 0 ? 64 / np : 0, dr64 = np > 0 ? 64 % np : 0;  // (row, u) step of the V-update walk (e += 64)
    int bu0 = 0, bv0 = 0;
    {
        int bb = t;
        while (bu0 < np && bb >= np - bu0) { bb -= np - bu0; bu0++; }
        bv0 = bu0 + bb;
    }
    bool converged = ne <= 1;
    for (int sweep = 0; sweep < 60 && ne > 1; sweep++) {
        double off = 0.0, dia = 0.0;
        for (int e = t; e < n * n; e += 64) {
            const int i = e / n, k = e % n;
            const double v = C[i * ld + k] * C[i * ld + k];
            if (i == k) dia += v; else off += v;
        }
        off = wave_sum(off);
        dia = wave_sum(dia);
        if (a.prof && t == 0) a.prof[(size_t)pl * 16 + 15] = sweep;
        if (off <= a.jacobi_tol * dia || off < 1e-300) { converged = true; break; }
        for (int r = 0; r < ne - 1; r++) {
            if (t < np) {
                int pp, qq;
                circle_pair(r, t, ne, pp, qq);
                const double apq = C[pp * ld + qq], app = C[pp * ld + pp], aqq = C[qq * ld + qq];
                double cs = 1.0, sn = 0.0, tt = 0.0;
                if (apq != 0.0) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    cs = 1.0 / sqrt(tt * tt + 1.0);
                    sn = tt * cs;
                }
                rot[5 * t + 0] = cs;
                rot[5 * t + 1] = sn;
                rot[5 * t + 2] = app - tt * apq;
                rot[5 * t + 3] = aqq + tt * apq;
                rot[5 * t + 4] = (double)(pp | (qq << 8));
            }
            __syncthreads();
            for (int b = t; b < nblk; b += 64) {
                int u = bu0, v = bv0;
                if (b != t) {
                    int bb = b;
                    u = 0;
                    while (bb >= np - u) { bb -= np - u; u++; }
                    v = u + bb;
                }
                const int pu = (int)rot[5 * u + 4] & 255, qu = (int)rot[5 * u + 4] >> 8;
                if (u == v) {
                    C[pu * ld + pu] = rot[5 * u + 2];
                    C[qu * ld + qu] = rot[5 * u + 3];
                    C[pu * ld + qu] = 0.0;
                    C[qu * ld + pu] = 0.0;
                } else {
                    const int pv = (int)rot[5 * v + 4] & 255, qv = (int)rot[5 * v + 4] >> 8;
                    const double cu = rot[5 * u], su = rot[5 * u + 1], cv = rot[5 * v], sv = rot[5 * v + 1];
                    const double x00 = C[pu * ld + pv], x01 = C[pu * ld + qv];
                    const double x10 = C[qu * ld + pv], x11 = C[qu * ld + qv];
                    const double y00 = cv * x00 - sv * x01, y01 = sv * x00 + cv * x01;
                    const double y10 = cv * x10 - sv * x11, y11 = sv * x10 + cv * x11;
                    const double z00 = cu * y00 - su * y10, z10 = su * y00 + cu * y10;
                    const double z01 = cu * y01 - su * y11, z11 = su * y01 + cu * y11;
                    C[pu * ld + pv] = z00; C[pv * ld + pu] = z00;
                    C[pu * ld + qv] = z01; C[qv * ld + pu] = z01;
                    C[qu * ld + pv] = z10; C[pv * ld + qu] = z10;
                    C[qu * ld + qv] = z11; C[qv * ld + qu] = z11;
                }
            }
            for (int e = t, row = t / np, u = t % np; e < n * np; e += 64) {
                const int pu = (int)rot[5 * u + 4] & 255, qu = (int)rot[5 * u + 4] >> 8;
                const double cu = rot[5 * u], su = rot[5 * u + 1];
                const double vp = V[row * ld + pu], vq = V[row * ld + qu];
                V[row * ld + pu] = cu * vp - su * vq;
                V[row * ld + qu] = su * vp + cu * vq;
                row += dq64; u += dr64;
                if (u >= np) { u -= np; row++; }
            }
            __syncthreads();
        }
    }

    MPCQ_STAMP(7);
    // ---- W^-1 = V' L' (needs V before it is overwritten), then W = L^-T V in place on V
    double *o_lam = out + Lo.lam, *o_W = out + Lo.W, *o_sWtW = out + Lo.sWtW, *o_WtA = out + Lo.WtA;
    double *o_PW = out + Lo.PW, *o_Winv = out + Lo.Winv, *o_Ah = out + Lo.Ah, *o_D = out + Lo.D, *o_E = out + Lo.E;
    double *o_Dinv = out + Lo.Dinv, *o_Einv = out + Lo.Einv, *o_cs = out + Lo.cs, *o_rs = out + Lo.rscale;
    for (int e = t; e < nc * nc; e += 64) {
        const int i = e / nc, k = e % nc;
        double wi = 0.0;
        if (i < n && k < n)
            for (int r = 0; r <= k; r++) wi += V[r * ld + i] * L[k * ld + r];
        o_Winv[e] = wi;
    }
    for (int k = t; k < nc; k += 64) {
        o_lam[k] = k < n ? fmax(C[k * ld + k], 0.0) : 0.0;
        if constexpr (!KEEP) {
            o_D[k] = k < n ? Dv[k] : 1.0;
            o_Dinv[k] = k < n ? 1.0 / Dv[k] : 1.0;
        }
    }
    if constexpr (!KEEP) {
        for (int i = t; i < mc; i += 64) {
            o_E[i] = i < m ? Ev[i] : 1.0;
            o_Einv[i] = i < m ? 1.0 / Ev[i] : 1.0;
            o_rs[i] = i < m ? Et[i] : 1.0;
        }
        if (t == 0) { o_cs[0] = cost; o_cs[1] = 1.0 / cost; }
    }
    __syncthreads();
    for (int i = n - 1; i >= 0; i--) {  // (L')[r][i] = L[i][r]
        const double li = L[i * ld + i];
        if (t < n) V[i * ld + t] /= li;
        __syncthreads();
        for (int e = t; e < i * n; e += 64) {
            const int r = e / n, c = e % n;
            V[r * ld + c] -= L[i * ld + r] * V[i * ld + c];
        }
        __syncthreads();
    }
    const double *W = V;
    for (int e = t; e < nc * nc; e += 64) {
        const int i = e / nc, k = e % nc;
        double w = 0.0, wtw = 0.0, pw = 0.0;
        if (i < n && k < n) {
            w = W[i * ld + k];
            for (int r = 0; r < n; r++) {
                wtw += W[r * ld + i] * W[r * ld + k];
                pw += Ph[i * ld + r] * W[r * ld + k];
            }
            wtw *= a.sigma;
        }
        o_W[e] = w;
        o_sWtW[e] = wtw;
        o_PW[e] = pw;
    }
    for (int e = t; e < mc * nc; e += 64) {
        const int j = e / nc, k = e % nc;
        double b = 0.0, ah = 0.0;
        if (j < m && k < n) {
            ah = Ah[j * ld + k];
            for (int r = 0; r < n; r++) b += Ah[j * ld + r] * W[r * ld + k];
        }
        o_WtA[e] = b;
        o_Ah[e] = ah;
        out[Lo.Bt + e] = b;  // eigen-basis: Bt = A^ W, G = W
    }
    for (int e = t; e < nc * nc; e += 64) out[Lo.G + e] = o_W[e];
    if (t == 0) out[Lo.rho0] = -1.0;
    MPCQ_STAMP(8);
    if (t == 0) {
        a.status[pl] = fail ? kNonCvx : 0;
        if (fail) atomicOr(a.flags, 1);
        if (!converged) atomicOr(a.flags, 4);  // sweep cap hit: (lambda, W) would be inaccurate
    }
}

__global__ __launch_bounds__(64) void setup_wave_kernel(SetupArgs a) { setup_wave_body<false>(a); }
// The factor stage alone on new matrices under the kept scaling (Cholesky, Jacobi eigen-basis, operator products).
__global__ __launch_bounds__(64) void setup_wave_keep_kernel(SetupArgs a) { setup_wave_body<true>(a); }

// In-place Gauss-Jordan inverse of an SPD matrix in LDS (n <= 32, row stride ld), 64 threads; no
// pivoting (SPD: every pivot is positive).  Returns false when a pivot is not positive (P^ + sigma I
// + rho A^'A^ not positive definite: OSQP's setup would fail to factor it).
// (forced inline: with two kernels calling it, a real call would cost each the worst-case register budget)
__device__ __forceinline__ bool gj_invert_spd(double *M, int n, int ld, int t)
{
    bool ok = true;
    for (int k = 0; k < n; k++) {
        const double piv = M[k * ld + k];
        if (!(piv > 0.0)) ok = false;
        const double ip = 1.0 / piv;
        double nv[16];  // this thread's elements t + 64 c (n*n <= 1024): static indices, registers
#pragma unroll
        for (int c = 0; c < 16; c++) {
            const int e = t + 64 * c;
            if (e < n * n) {
                const int i = e / n, j = e % n;
                double v;
                if (i == k && j == k) v = ip;
                else if (i == k) v = M[k * ld + j] * ip;
                else if (j == k) v = -M[i * ld + k] * ip;
                else v = M[i * ld + j] - M[i * ld + k] * (M[k * ld + j] * ip);
                nv[c] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 16; c++) {
            const int e = t + 64 * c;
            if (e < n * n) M[(e / n) * ld + e % n] = nv[c];
        }
        __syncthreads();
    }
    return ok;
}

// Per-plant setup with the direct inverse (batches of distinct plants, BASELINE config 3): OSQP's
// scale_data and set_rho_vec as setup_wave_kernel, then M(rho0) = P^ + sigma I + sum_j rho_j a_j a_j'
// (rho_j = rho0 * rscale_j, RHO_MIN on free rows) and its inverse by Gauss-Jordan: O(n^3) in place
// of the eigen-basis's Cholesky + Jacobi sweeps.  Writes the operator block in the direct-inverse
// reading of OpsLayout (mpcq_internal.h): W = W^-1 = I, lambda = 0, sigma W'W = sigma M^-1,
// G = M^-1, Bt = A^ M^-1, PW = P^, WtA = Ah = A^, rho0.
template <bool KEEP>
__device__ __forceinline__ void setup_inv_body(const SetupArgs &a)
{
    extern __shared__ double sm[];
    const int pl = blockIdx.x;
    if (pl >= a.n_plants) return;
    const int t = threadIdx.x;
    const int n = a.n, m = a.m, nc = a.nc, mc = a.mc;
    const SetupWaveShape S = SetupWaveShape::make(n, m);
    const int ld = S.ld;
    double *Ph = sm + S.Ph, *Ah = sm + S.Ah, *Mi = sm + S.L;
    double *Dv = sm + S.Dv, *Ev = sm + S.Ev, *Dt = sm + S.Dt, *Et = sm + S.Et, *qh = sm + S.qh;
    double *sh = sm + S.total - 8;
    const double *P = a.P + (size_t)pl * n * n;
    const double *q0 = a.q0 + (size_t)pl * n;
    const double *A = a.A + (size_t)pl * m * n;
    const OpsLayout Lo = OpsLayout::make(nc, mc);
    double *out = a.ops + (size_t)pl * Lo.total;
    int *ctype = a.ctype + (size_t)pl * mc;

    MPCQ_STAMP(0);
    double cost = 1.0;
    if constexpr (KEEP) {
        load_kept_scaling(a, pl, t, n, m, ld, out, Lo, Ph, Ah, Dv, Ev, Et);
    } else {
        for (int e = t; e < n * n; e += 64) {  // (osqp-eigen keeps the upper triangle of the Hessian)
            const int i = e / n, j = e % n;
            Ph[i * ld + j] = (i <= j) ? P[i * n + j] : P[j * n + i];
        }
        for (int e = t; e < m * n; e += 64) Ah[(e / n) * ld + e % n] = A[e];
        for (int j = t; j < n; j += 64) { qh[j] = q0[j]; Dv[j] = 1.0; }
        for (int i = t; i < m; i += 64) Ev[i] = 1.0;
        if (t == 0) sh[0] = 1.0;
        __syncthreads();
        MPCQ_STAMP(1);
        cost = ruiz_and_types(a, pl, t, n, m, mc, ld, Ph, Ah, Dv, Ev, Dt, Et, qh, sh, ctype);
    }
    MPCQ_STAMP(3);

    // ---- M(rho0) and its inverse
    const double rho = fmin(fmax(a.rho, kRhoMin), kRhoMax);
    for (int e = t; e < n * n; e += 64) {
        const int i = e / n, k = e % n;
        double v = Ph[i * ld + k] + (i == k ? a.sigma : 0.0);
        for (int r = 0; r < m; r++) {
            const double rr = Et[r] == 0.0 ? kRhoMin : rho * Et[r];
            v += rr * (Ah[r * ld + i] * Ah[r * ld + k]);
        }
        Mi[i * ld + k] = v;
    }
    __syncthreads();
    const bool ok = gj_invert_spd(Mi, n, ld, t);
    MPCQ_STAMP(6);

    // ---- operator block (zero padded to nc x mc)
    for (int e = t; e < nc * nc; e += 64) {
        const int i = e / nc, k = e % nc;
        const bool in = i < n && k < n;
        const double mi = in ? Mi[i * ld + k] : 0.0, id = (i == k && i < n) ? 1.0 : 0.0;
        out[Lo.W + e] = id;
        out[Lo.Winv + e] = id;
        out[Lo.sWtW + e] = a.sigma * mi;
        out[Lo.G + e] = mi;
        out[Lo.PW + e] = in ? Ph[i * ld + k] : 0.0;
    }
    for (int e = t; e < mc * nc; e += 64) {
        const int j = e / nc, k = e % nc;
        double ah = 0.0, bt = 0.0;
        if (j < m && k < n) {
            ah = Ah[j * ld + k];
            for (int r = 0; r < n; r++) bt += Ah[j * ld + r] * Mi[r * ld + k];
        }
        out[Lo.WtA + e] = ah;
        out[Lo.Ah + e] = ah;
        out[Lo.Bt + e] = bt;
    }
    for (int k = t; k < nc; k += 64) {
        out[Lo.lam + k] = 0.0;
        if constexpr (!KEEP) {
            out[Lo.D + k] = k < n ? Dv[k] : 1.0;
            out[Lo.Dinv + k] = k < n ? 1.0 / Dv[k] : 1.0;
        }
    }
    if constexpr (!KEEP) {
        for (int i = t; i < mc; i += 64) {
            out[Lo.E + i] = i < m ? Ev[i] : 1.0;
            out[Lo.Einv + i] = i < m ? 1.0 / Ev[i] : 1.0;
            out[Lo.rscale + i] = i < m ? Et[i] : 1.0;
        }
    }
    if (t == 0) {
        if constexpr (!KEEP) {
            out[Lo.cs] = cost;
            out[Lo.cs + 1] = 1.0 / cost;
        }
        out[Lo.rho0] = rho;
        a.status[pl] = ok ? 0 : kNonCvx;
        if (!ok) atomicOr(a.flags, 1);
    }
    MPCQ_STAMP(8);
}

__global__ __launch_bounds__(64) void setup_inv_kernel(SetupArgs a) { setup_inv_body<false>(a); }
// M(rho0) and its Gauss-Jordan inverse alone on new matrices under the kept scaling.
__global__ __launch_bounds__(64) void setup_inv_keep_kernel(SetupArgs a) { setup_inv_body<true>(a); }

// ---- what mpcq_update_P_A_device checks on the device (its one flag word carries the answers back)
// Shared plant: flag 8 when some QP's scaled lower bound is not below -OSQP_INFTY * MIN_SCALING under the block's
// E (the host rule of mpcq_update_lower_bound: l E < -INFTY MIN_SCALING, or l <= -1e300).
__global__ __launch_bounds__(256) void lower_free_kernel(const double *l, const double *E, int m, size_t total, int *flags)
{
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const double v = l[i];
        if (!(v * E[i % m] < -kInfty * kMinScaling) && !(v <= -1e300)) bad = true;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flags, 8);
}
// Flag 16 when rows n + j of A are not the negated rows j bit for bit (mpcq_setup's test for the paired loop).
__global__ __launch_bounds__(256) void paired_kernel(const double *A, int nn, int *flags)
{
    bool bad = false;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nn; i += gridDim.x * 256)
        if (!(A[nn + i] == -A[i])) bad = true;
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flags, 16);
}
// A QP whose previous x or y holds a non-finite entry starts cold: its warm-state rows (x', z, y; `es` bytes
// per element) are zeroed after the warm-start kernel has filled them.
__global__ __launch_bounds__(64) void cold_nonfinite_kernel(const double *x, const double *y, int n, int m, int nc, int mc,
                                                            int batch, int es, void *xs, void *zs, void *ys)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    bool fin = true;
    for (int i = 0; i < n; i++) fin = fin && isfinite(x[(size_t)b * n + i]);
    for (int j = 0; j < m; j++) fin = fin && isfinite(y[(size_t)b * m + j]);
    if (fin) return;
    const int wx = nc * es / 4, wz = mc * es / 4;  // 32-bit words per row
    unsigned *px = (unsigned *)xs + (size_t)b * wx, *pz = (unsigned *)zs + (size_t)b * wz, *py = (unsigned *)ys + (size_t)b * wz;
    for (int i = 0; i < wx; i++) px[i] = 0u;
    for (int j = 0; j < wz; j++) { pz[j] = 0u; py[j] = 0u; }
}

}  // namespace mpcq

extern "C" int mpcq_internal_setup_inv_launch(const mpcq::SetupArgs *args, hipStream_t stream)
{
    if (args->n < 1 || args->n > 32 || args->m > 64) return -1;
    const size_t lds = 8 * mpcq::SetupWaveShape::make(args->n, args->m).total;
    hipLaunchKernelGGL(mpcq::setup_inv_kernel, dim3(args->n_plants), dim3(64), lds, stream, *args);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// The keep-scaling kernels (mpcq_update_P_A_device, rescale = 0): `inv` selects the direct-inverse reading.
extern "C" int mpcq_internal_setup_keep_launch(const mpcq::SetupArgs *args, int inv, hipStream_t stream)
{
    const size_t lds = mpcq_internal_setup_wave_lds(args->n, args->m);
    if (!lds || lds > 65536) return -1;
    if (inv) hipLaunchKernelGGL(mpcq::setup_inv_keep_kernel, dim3(args->n_plants), dim3(64), lds, stream, *args);
    else hipLaunchKernelGGL(mpcq::setup_wave_keep_kernel, dim3(args->n_plants), dim3(64), lds, stream, *args);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int mpcq_internal_lower_free_check(const double *l, const double *E, int m, size_t total, int *flags,
                                              hipStream_t stream)
{
    if (!total) return 0;
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 1024);
    hipLaunchKernelGGL(mpcq::lower_free_kernel, dim3(grid), dim3(256), 0, stream, l, E, m, total, flags);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int mpcq_internal_paired_check(const double *A, int nn, int *flags, hipStream_t stream)
{
    hipLaunchKernelGGL(mpcq::paired_kernel, dim3(std::min((nn + 255) / 256, 64)), dim3(256), 0, stream, A, nn, flags);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int mpcq_internal_cold_nonfinite(const double *x, const double *y, int n, int m, int nc, int mc, int batch,
                                            int is_f32, void *xs, void *zs, void *ys, hipStream_t stream)
{
    hipLaunchKernelGGL(mpcq::cold_nonfinite_kernel, dim3((batch + 63) / 64), dim3(64), 0, stream, x, y, n, m, nc, mc,
                       batch, is_f32 ? 4 : 8, xs, zs, ys);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" size_t mpcq_internal_setup_wave_lds(int n, int m)
{
    if (n < 1 || n > 32 || m > 64) return 0;
    return 8 * mpcq::SetupWaveShape::make(n, m).total;
}

extern "C" int mpcq_internal_setup_wave_launch(const mpcq::SetupArgs *args, hipStream_t stream)
{
    const size_t lds = mpcq_internal_setup_wave_lds(args->n, args->m);
    if (!lds || lds > 65536) return -1;
    hipLaunchKernelGGL(mpcq::setup_wave_kernel, dim3(args->n_plants), dim3(64), lds, stream, *args);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

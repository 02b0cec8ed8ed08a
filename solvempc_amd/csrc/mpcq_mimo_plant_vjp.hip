// solvempc_amd/csrc/mpcq_mimo_plant_vjp.hip — the last MIMO step's cotangents pulled back through the MIMO
// condensing to the plant data Ad, Bd, Cd, Q, R, RD, K, K0, w0 (include/mpcq.h, mpcq_mimo_plant_vjp*; DESIGN.md
// 4.17).  One 256-thread workgroup per plant, the grid striding over the batch; fp64, everything in LDS.
//
// The operator cotangents are rank two (gP = 1/2 (gq x' + x gq'), gA = y_a gq' - w x', the front end's: outer
// products of gq, w with X, U_prev, yref) and the condensing is block-Toeplitz (Su(i, j) = C_(i-j)) or block prefix
// sums (LL, A = [L (x) K0; -(L (x) K0)]), so no n x n object is formed: with a = gq, b = x in N blocks of n_u,
//   pa, pb        block prefix sums (lane_prefix over the horizon, one lane per block)
//   r_k           Cd Ad^k by the recursion r_k = r_(k-1) Ad, k = 0..N
//   C_d           running sums of r_k Bd (lane_prefix per entry)
//   sa_i, sb_i    sum_(j <= i) C_(i-j) a_j, b_j: the block-Toeplitz products Su a, Su b
//   e_i           r_(i+1) X + C_i U_prev - yref: the predicted output error without the moves
//   qs, v, w      Q sa_i;  (Q+Q') sb_i + 2 Q' e_i;  (Q+Q') sa_i
//   Gc_d          sum_(i >= d) (v_i a_(i-d)' + w_i b_(i-d)') + 2 qs_d U_prev': the correlation sums, then their
//                 suffix sums GCAB_k (lane_suffix per entry), in C's storage (C is dead by then)
//   rho           the reverse recursion rho_(k-1) = rho_k Ad' + GCAB_(k-1) Bd' + 2 qs_(k-2) X', double-buffered, one
//                 barrier per step; gAd += r_(k-1)' rho_k and gBd += r_(k-1)' GCAB_(k-1) ride along in registers
// Every output element is owned by one thread that sums in a fixed index order, and the scans are mpcq_lane.h's on
// one wavefront: no atomics, two calls give identical bits.  Everything is computed whichever outputs are asked for;
// a null pointer only skips the store.  The active set of y_a is mimo_sens_kernel's (mimo_upper_active on the step's
// scaled iterate).  Nothing of the context is written.
#include "mpcq_internal.h"
#include "mpcq_lane.h"

namespace mpcq {

constexpr int kPvThreads = 256;
constexpr int kPvWaves = kPvThreads / 64;

// LDS carve-up (doubles) of mimo_plant_vjp_kernel for the call's own N, nx, nu, ny
struct MimoPlantVjpShape {
    int Ad, At, Bd, Q, X, U, yr, sums, a, b, dw, sw, yd, pa, pb, r, C, sa, sb, e, qs, v, w, rho, total;
    __host__ __device__ static MimoPlantVjpShape make(int N, int nx, int nu, int ny)
    {
        MimoPlantVjpShape s{};
        const int n = N * nu;
        int o = 0;
        s.Ad = o; o += nx * nx;
        s.At = o; o += nx * nx;            // Ad' (the reverse recursion reads Ad by columns)
        s.Bd = o; o += nx * nu;
        s.Q = o; o += ny * ny;
        s.X = o; o += nx;
        s.U = o; o += nu;
        s.yr = o; o += ny;
        s.sums = o; o += 4 * nu;           // sum_k a_k, sum_k dw_k, sum_(k < s_rows) dw_k, sum_k sw_k
        s.a = o; o += n;                   // gq
        s.b = o; o += n;                   // x
        s.dw = o; o += n;                  // w_top - w_bot
        s.yd = o; o += n;                  // ya_top - ya_bot
        s.pa = o; o += n;
        s.pb = o; o += n;
        s.r = o; o += (N + 1) * ny * nx;
        s.C = o; o += N * ny * nu;         // r_k Bd, C_d, then Gc_d, GCAB_k
        s.sw = o;                          // w_top + w_bot: n <= 6 N ny doubles over sa .. w, read by the block sums
                                           // of stage 1 alone, long before stage 5 writes sa
        s.sa = o; o += N * ny;
        s.sb = o; o += N * ny;
        s.e = o; o += N * ny;
        s.qs = o; o += N * ny;
        s.v = o; o += N * ny;
        s.w = o; o += N * ny;
        s.rho = o; o += 2 * ny * nx;
        s.total = o;
        return s;
    }
};

template <int NU>
__global__ __launch_bounds__(kPvThreads) void mimo_plant_vjp_kernel(MimoPlantVjpArgs A)
{
    extern __shared__ double lds[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int N = A.N, nx = A.nx, ny = A.ny, n = N * NU, m = 2 * n;
    const int nxx = nx * nx, nyx = ny * nx, nyu = ny * NU, nxu = nx * NU, Ny = N * ny;
    const int ks = A.s_rows < N ? A.s_rows : N;
    const MimoPlantVjpShape S = MimoPlantVjpShape::make(N, nx, NU, ny);
    const int offE = MimoLayout::make(N, nx, NU, ny).E;
    double *const sAd = lds + S.Ad, *const sAt = lds + S.At, *const sBd = lds + S.Bd, *const sQ = lds + S.Q;
    double *const sX = lds + S.X, *const sU = lds + S.U, *const syr = lds + S.yr, *const sums = lds + S.sums;
    double *const a = lds + S.a, *const b = lds + S.b, *const dw = lds + S.dw, *const sw = lds + S.sw;
    double *const yd = lds + S.yd, *const pa = lds + S.pa, *const pb = lds + S.pb, *const r = lds + S.r;
    double *const Cc = lds + S.C, *const sa = lds + S.sa, *const sb = lds + S.sb, *const ev = lds + S.e;
    double *const qs = lds + S.qs, *const vv = lds + S.v, *const wv = lds + S.w, *const rho = lds + S.rho;
    const auto add = [](double x, double y) { return x + y; };

    for (int p = blockIdx.x; p < A.batch; p += gridDim.x) {
        __syncthreads();  // the previous plant of this workgroup is done with every buffer
        const size_t P = (size_t)p;
        const int na = A.nact[p];  // (uniform)
        if (t == 0 && A.n_active) A.n_active[p] = na;
        if (na < 0) {  // no sensitivity exists: all-zero outputs
            for (int e = t; e < nxx; e += kPvThreads)
                if (A.gAd) A.gAd[P * nxx + e] = 0.0;
            for (int e = t; e < nxu; e += kPvThreads) {
                if (A.gBd) A.gBd[P * nxu + e] = 0.0;
                if (A.gK) A.gK[P * nxu + e] = 0.0;
            }
            for (int e = t; e < nyx; e += kPvThreads)
                if (A.gCd) A.gCd[P * nyx + e] = 0.0;
            for (int e = t; e < ny * ny; e += kPvThreads)
                if (A.gQ) A.gQ[P * ny * ny + e] = 0.0;
            if (t < NU * NU) {
                if (A.gR) A.gR[P * NU * NU + t] = 0.0;
                if (A.gRD) A.gRD[P * NU * NU + t] = 0.0;
                if (A.gK0) A.gK0[P * NU * NU + t] = 0.0;
            }
            if (t < NU && A.gw0) A.gw0[P * NU + t] = 0.0;
            continue;
        }

        // ---- 0. the plant, the step's data, the cotangents; r_0 = Cd
        for (int e = t; e < nxx; e += kPvThreads) {
            const double v = A.Ad[P * nxx + e];
            sAd[e] = v;
            sAt[(e % nx) * nx + e / nx] = v;
        }
        for (int e = t; e < nxu; e += kPvThreads) sBd[e] = A.Bd[P * nxu + e];
        for (int e = t; e < ny * ny; e += kPvThreads) sQ[e] = A.Q[P * ny * ny + e];
        for (int e = t; e < nyx; e += kPvThreads) r[e] = A.Cd[P * nyx + e];
        if (t < nx) sX[t] = A.X[P * nx + t];
        if (t < NU) sU[t] = A.U_prev[P * NU + t];
        if (t < ny) syr[t] = A.yref ? A.yref[t] : 0.0;
        for (int e = t; e < n; e += kPvThreads) {
            const double E = A.ops[P * A.ops_stride + offE + e];
            const size_t it = P * m + e, ib = it + n;
            const bool upt = mimo_upper_active(A.u[it], E, A.zs[it], A.ys[it]);
            const bool upb = mimo_upper_active(A.u[ib], E, A.zs[ib], A.ys[ib]);
            const double wt = A.gu[it], wb = A.gu[ib];
            a[e] = A.gq[P * n + e];
            b[e] = A.x[P * n + e];
            dw[e] = wt - wb;
            sw[e] = wt + wb;
            yd[e] = (upt ? A.y[it] : 0.0) - (upb ? A.y[ib] : 0.0);
        }
        __syncthreads();

        // ---- 1. block prefix sums pa = LL a, pb = LL b (wave 0: one lane per horizon block); the four block sums
        if (wave == 0) {
#pragma unroll
            for (int c = 0; c < NU; c++) {
                const int i = (lane < N ? lane : 0) * NU + c;
                double va = lane < N ? a[i] : 0.0, vb = lane < N ? b[i] : 0.0;
                va = lane_prefix(va, add, lane);
                vb = lane_prefix(vb, add, lane);
                if (lane < N) {
                    pa[i] = va;
                    pb[i] = vb;
                }
            }
        } else if (wave == 1 && lane < 4 * NU) {
            const int kind = lane / NU, c = lane - kind * NU;
            const double *src = kind == 0 ? a : kind == 3 ? sw : dw;
            const int cnt = kind == 2 ? ks : N;
            double s = 0.0;
            for (int k = 0; k < cnt; k++) s += src[k * NU + c];
            sums[lane] = s;
        }
        __syncthreads();

        // ---- 2. the outputs that need no recursion: gRD, gR, gK0 (n_u x n_u), gK (n_u x n_x), gw0
        if (t < NU * NU) {
            const int c = t / NU, d = t - c * NU;
            double sRD = 0.0, sR = 0.0, sK0 = 0.0;
            for (int k = 0; k < N; k++) {
                const int ic = k * NU + c, id = k * NU + d;
                sRD += a[ic] * b[id] + b[ic] * a[id];
                sR += pa[ic] * pb[id] + pb[ic] * pa[id];
                sK0 += yd[ic] * pa[id] - dw[ic] * pb[id];
            }
            if (A.gRD) A.gRD[P * NU * NU + t] = sRD;
            if (A.gR) A.gR[P * NU * NU + t] = sR + 2.0 * (sU[c] * sums[d]);
            if (A.gK0) A.gK0[P * NU * NU + t] = sK0 - sums[NU + c] * sU[d];
        } else if (t >= 64 && t < 64 + nxu) {
            const int e = t - 64, c = e / nx, j = e - c * nx;
            if (A.gK) A.gK[P * nxu + e] = sums[2 * NU + c] * sX[j];
        } else if (t >= 128 && t < 128 + NU) {
            if (A.gw0) A.gw0[P * NU + t - 128] = sums[3 * NU + t - 128];
        }

        // ---- 3. r_k = r_(k-1) Ad, k = 1..N
        {
            const int row = t / nx, col = t - row * nx;
            for (int k = 1; k <= N; k++) {
                if (t < nyx) {
                    const double *rp = r + (k - 1) * nyx + row * nx;
                    double s = 0.0;
                    for (int j = 0; j < nx; j++) s += rp[j] * sAd[j * nx + col];
                    r[k * nyx + t] = s;
                }
                __syncthreads();
            }
        }
        // ---- 4. CAB_k = r_k Bd (k < N), then C_d = sum_(k <= d) CAB_k per entry
        for (int e = t; e < N * nyu; e += kPvThreads) {
            const int k = e / nyu, q = e - k * nyu, rr = q / NU, c = q - rr * NU;
            const double *rp = r + k * nyx + rr * nx;
            double s = 0.0;
            for (int j = 0; j < nx; j++) s += rp[j] * sBd[j * NU + c];
            Cc[e] = s;
        }
        __syncthreads();
        for (int q = wave; q < nyu; q += kPvWaves) {
            double s = lane < N ? Cc[lane * nyu + q] : 0.0;
            s = lane_prefix(s, add, lane);
            if (lane < N) Cc[lane * nyu + q] = s;
        }
        __syncthreads();

        // ---- 5. sa = Su a, sb = Su b (block-Toeplitz), e_i = r_(i+1) X + C_i U_prev - yref
        for (int o = t; o < 3 * Ny; o += kPvThreads) {
            const int kind = o / Ny, q = o - kind * Ny, i = q / ny, rr = q - i * ny;
            double s = 0.0;
            if (kind < 2) {
                const double *src = kind == 0 ? a : b;
                for (int j = 0; j <= i; j++) {
                    const double *cp = Cc + (i - j) * nyu + rr * NU;
#pragma unroll
                    for (int c = 0; c < NU; c++) s += cp[c] * src[j * NU + c];
                }
                (kind == 0 ? sa : sb)[q] = s;
            } else {
                const double *rp = r + (i + 1) * nyx + rr * nx;
                for (int j = 0; j < nx; j++) s += rp[j] * sX[j];
                double cu = 0.0;
#pragma unroll
                for (int c = 0; c < NU; c++) cu += Cc[i * nyu + rr * NU + c] * sU[c];
                ev[q] = (s + cu) - syr[rr];
            }
        }
        __syncthreads();

        // ---- 6. gQ; qs = Q sa, v = (Q+Q') sb + 2 Q' e, w = (Q+Q') sa
        if (t < ny * ny) {
            const int rr = t / ny, s2 = t - rr * ny;
            double s = 0.0;
            for (int i = 0; i < N; i++) {
                const int ir = i * ny + rr, is = i * ny + s2;
                s += (sa[ir] * sb[is] + sb[ir] * sa[is]) + 2.0 * (ev[ir] * sa[is]);
            }
            if (A.gQ) A.gQ[P * ny * ny + t] = s;
        }
        for (int o = t; o < 3 * Ny; o += kPvThreads) {
            const int kind = o / Ny, q = o - kind * Ny, i = q / ny, rr = q - i * ny;
            double s = 0.0;
            if (kind == 0) {
                for (int j = 0; j < ny; j++) s += sQ[rr * ny + j] * sa[i * ny + j];
                qs[q] = s;
            } else if (kind == 1) {
                double s2 = 0.0;
                for (int j = 0; j < ny; j++) {
                    s += (sQ[rr * ny + j] + sQ[j * ny + rr]) * sb[i * ny + j];
                    s2 += sQ[j * ny + rr] * ev[i * ny + j];
                }
                vv[q] = s + 2.0 * s2;
            } else {
                for (int j = 0; j < ny; j++) s += (sQ[rr * ny + j] + sQ[j * ny + rr]) * sa[i * ny + j];
                wv[q] = s;
            }
        }
        __syncthreads();

        // ---- 7. Gc_d (over C, which nothing reads any more), then GCAB_k = sum_(d >= k) Gc_d per entry
        for (int e = t; e < N * nyu; e += kPvThreads) {
            const int d = e / nyu, q = e - d * nyu, rr = q / NU, c = q - rr * NU;
            double s = 0.0;
            for (int i = d; i < N; i++) s += vv[i * ny + rr] * a[(i - d) * NU + c] + wv[i * ny + rr] * b[(i - d) * NU + c];
            Cc[e] = s + 2.0 * (qs[d * ny + rr] * sU[c]);
        }
        __syncthreads();
        for (int q = wave; q < nyu; q += kPvWaves) {
            double s = lane < N ? Cc[lane * nyu + q] : 0.0;
            s = lane_suffix(s, add, lane);
            if (lane < N) Cc[lane * nyu + q] = s;
        }
        // rho_N = 2 qs_(N-1) X'
        if (t < nyx) {
            const int rr = t / nx, j = t - rr * nx;
            rho[(N & 1) * nyx + t] = 2.0 * (qs[(N - 1) * ny + rr] * sX[j]);
        }
        __syncthreads();

        // ---- 8. the reverse recursion, k = N..1: gAd += r_(k-1)' rho_k, gBd += r_(k-1)' GCAB_(k-1),
        //         rho_(k-1) = rho_k Ad' + GCAB_(k-1) Bd' + 2 qs_(k-2) X'
        {
            // rho's threads from the bottom, gAd's from the top, gBd's after rho's: the three overlap on few threads
            const int tr = t, rr = tr / nx, rj = tr - rr * nx;
            const int ta = kPvThreads - 1 - t, ai = ta / nx, aj = ta - ai * nx;
            const int tb = t - nyx, bj = tb / NU, bc = tb - bj * NU;
            double accA = 0.0, accB = 0.0;
            for (int k = N; k >= 1; k--) {
                const double *rk = rho + (k & 1) * nyx, *r1 = r + (k - 1) * nyx, *G1 = Cc + (k - 1) * nyu;
                if (ta < nxx) {
                    double s = 0.0;
                    for (int q = 0; q < ny; q++) s += r1[q * nx + ai] * rk[q * nx + aj];
                    accA += s;
                }
                if (tb >= 0 && tb < nxu) {
                    double s = 0.0;
                    for (int q = 0; q < ny; q++) s += r1[q * nx + bj] * G1[q * NU + bc];
                    accB += s;
                }
                if (tr < nyx) {
                    double s = 0.0;
                    for (int l = 0; l < nx; l++) s += rk[rr * nx + l] * sAt[l * nx + rj];
                    double g = 0.0;
#pragma unroll
                    for (int c = 0; c < NU; c++) g += G1[rr * NU + c] * sBd[rj * NU + c];
                    s += g;
                    if (k >= 2) s += 2.0 * (qs[(k - 2) * ny + rr] * sX[rj]);
                    rho[((k - 1) & 1) * nyx + tr] = s;
                }
                __syncthreads();
            }
            if (ta < nxx && A.gAd) A.gAd[P * nxx + ta] = accA;
            if (tb >= 0 && tb < nxu && A.gBd) A.gBd[P * nxu + tb] = accB;
            if (tr < nyx && A.gCd) A.gCd[P * nyx + tr] = rho[tr];
        }
    }
}

}  // namespace mpcq

extern "C" size_t mpcq_internal_mimo_plant_vjp_lds(int N, int nx, int nu, int ny)
{
    return 8 * (size_t)mpcq::MimoPlantVjpShape::make(N, nx, nu, ny).total;
}

extern "C" int mpcq_internal_mimo_plant_vjp_launch(const mpcq::MimoPlantVjpArgs *a, int cus, hipStream_t s, hipError_t *err)
{
    *err = hipSuccess;
    if (!mpcq::mimo_shape_ok(a->N, a->nx, a->nu, a->ny)) return -1;
    if (a->batch <= 0) return 0;
    return mpcq::mimo_with_nu(a->nu, [&](auto nu) {
        // (no static LDS: the carve-up is the call's own N, nx, nu, ny, so a CU holds as many plants as they allow)
        return mpcq::launch_per_qp(mpcq::mimo_plant_vjp_kernel<decltype(nu)::value>, *a, a->batch, mpcq::kPvThreads,
                                   mpcq_internal_mimo_plant_vjp_lds(a->N, a->nx, a->nu, a->ny), 0, cus, s, err);
    });
}

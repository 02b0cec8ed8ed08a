// solvempc_amd/csrc/mpcq_sensdata.hip — gradients with respect to the QP's matrices from a sensitivity call's
// (gq, gl, gu, active sets) and the solve's (x, y).  Per QP, with w = gl + gu and y_a = y on the
// active rows, 0 elsewhere:
//   gP = 1/2 (gq x' + x gq')     n x n, symmetric
//   gA = y_a gq' - w x'          m x n, zero on inactive rows
// A QP with n_active < 0 (not SOLVED, or no factorisation) contributes nothing and none of its arrays is read:
// its x may be NaN.
//
// Per-plant contexts: sens_outer_kernel, one thread per output element.
//
// Shared plant: the sums over the batch, a contraction whose K index is the QP.  sens_contract_kernel runs it on
// v_mfma_f64_16x16x4_f64: lane (g = lane >> 4, c = lane & 15) of a K step holds element 16 t + c of QP b0 + g's
// vectors -- one contiguous 128-byte segment per QP and tile, straight from global memory -- as the A operand
// (the output's row index) or the B operand (its column index); accumulator v is C(16 ti + g + 4 v, 16 tj + c).
// gP accumulates S = sum_b gq_b x_b'; gA takes y_a (x) gq and (-w) (x) x into the same accumulators.  Elements
// past n or m, QPs past the batch and skipped QPs are loaded as 0.0 (the load itself is guarded).
//   The batch is cut into chunks of kSensChunk QPs, one workgroup each; its four waves take 64 consecutive QPs
// each in ascending K order and their accumulators are added in wave order through LDS, which gives the chunk's
// partial.  sens_reduce_kernel adds the partials in ascending chunk order, one thread per element, and forms
// gP = 1/2 (S + S').  No atomics: the result depends on the batch alone, not on the device or the grid.
#include <algorithm>

#include "mpcq_internal.h"

namespace mpcq {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kSensMaxN = 32, kSensMaxM = 64;
constexpr int kSensNT = kSensMaxN / 16, kSensMT = kSensMaxM / 16;
constexpr int kSensWaves = kSensChunk / 64;  // K steps of 4 QPs: 16 per wave

__global__ __launch_bounds__(kSensChunk) void sens_contract_kernel(SensDataArgs a)
{
    __shared__ double red[kSensMaxN * kSensMaxN + kSensMaxM * kSensMaxN];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int n = a.n, m = a.m;
    const int nt = (n + 15) >> 4, mt = (m + 15) >> 4;
    const bool doP = a.gP != nullptr, doA = a.gA != nullptr && m > 0;
    v4d accP[kSensNT][kSensNT], accA[kSensMT][kSensNT];
#pragma unroll
    for (int ti = 0; ti < kSensNT; ti++)
#pragma unroll
        for (int tj = 0; tj < kSensNT; tj++) accP[ti][tj] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ti = 0; ti < kSensMT; ti++)
#pragma unroll
        for (int tj = 0; tj < kSensNT; tj++) accA[ti][tj] = v4d{0.0, 0.0, 0.0, 0.0};

    const long long q0 = (long long)blockIdx.x * kSensChunk + wave * 64;
    if (q0 < a.batch) {  // (wave-uniform)
#pragma unroll 2
        for (int ks = 0; ks < 16; ks++) {
            const long long b = q0 + 4 * ks + g;
            const bool valid = b < a.batch && a.n_active[b] >= 0;
            const unsigned long long rows = valid ? (a.active[2 * b] | a.active[2 * b + 1]) : 0ull;
            double gqv[kSensNT], xv[kSensNT], yv[kSensMT], wv[kSensMT];
#pragma unroll
            for (int t = 0; t < kSensNT; t++) {
                const int i = 16 * t + c;
                const bool in = valid && i < n;
                gqv[t] = in ? a.gq[b * n + i] : 0.0;
                xv[t] = in ? a.x[b * n + i] : 0.0;
            }
#pragma unroll
            for (int t = 0; t < kSensMT; t++) {
                const int r = 16 * t + c;
                const bool in = doA && valid && r < m;
                wv[t] = in ? -(a.gl[b * m + r] + a.gu[b * m + r]) : 0.0;  // (one of the two is 0: exact)
                yv[t] = (in && ((rows >> r) & 1ull)) ? a.y[b * m + r] : 0.0;
            }
            if (doP) {
#pragma unroll
                for (int ti = 0; ti < kSensNT; ti++)
#pragma unroll
                    for (int tj = 0; tj < kSensNT; tj++)
                        if (ti < nt && tj < nt)
                            accP[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(gqv[ti], xv[tj], accP[ti][tj], 0, 0, 0);
            }
            if (doA) {
#pragma unroll
                for (int ti = 0; ti < kSensMT; ti++)
#pragma unroll
                    for (int tj = 0; tj < kSensNT; tj++)
                        if (ti < mt && tj < nt) {
                            accA[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(yv[ti], gqv[tj], accA[ti][tj], 0, 0, 0);
                            accA[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv[ti], xv[tj], accA[ti][tj], 0, 0, 0);
                        }
            }
        }
    }

    // the chunk's partial: the waves' accumulators added in wave order
    for (int w = 0; w < kSensWaves; w++) {
        if (wave == w) {
#pragma unroll
            for (int tj = 0; tj < kSensNT; tj++) {
                const int col = 16 * tj + c;
#pragma unroll
                for (int v = 0; v < 4; v++) {
#pragma unroll
                    for (int ti = 0; ti < kSensNT; ti++) {
                        const int row = 16 * ti + g + 4 * v;
                        if (row < n && col < n) {
                            double *p = red + row * n + col;
                            *p = w ? *p + accP[ti][tj][v] : accP[ti][tj][v];
                        }
                    }
#pragma unroll
                    for (int ti = 0; ti < kSensMT; ti++) {
                        const int row = 16 * ti + g + 4 * v;
                        if (row < m && col < n) {
                            double *p = red + n * n + row * n + col;
                            *p = w ? *p + accA[ti][tj][v] : accA[ti][tj][v];
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    const int E = n * n + m * n;
    double *out = a.part + (size_t)blockIdx.x * E;
    for (int e = threadIdx.x; e < E; e += kSensChunk) out[e] = red[e];
}

// gP = 1/2 (S + S'), gA: the partials added in ascending chunk order, one thread per element
__global__ __launch_bounds__(256) void sens_reduce_kernel(SensDataArgs a, int chunks)
{
    const int n = a.n, nn = n * n, E = nn + a.m * n;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    if (e < nn) {
        if (!a.gP) return;
        const int i = e / n, j = e - i * n, et = j * n + i;
        double s = 0.0, st = 0.0;
        for (int ch = 0; ch < chunks; ch++) {
            s += a.part[(size_t)ch * E + e];
            st += a.part[(size_t)ch * E + et];
        }
        a.gP[e] = 0.5 * (s + st);
    } else {
        if (!a.gA) return;
        double s = 0.0;
        for (int ch = 0; ch < chunks; ch++) s += a.part[(size_t)ch * E + e];
        a.gA[e - nn] = s;
    }
}

// per-plant contexts: each QP's two outer products, one thread per element (zeros for a skipped QP)
__global__ __launch_bounds__(256) void sens_outer_kernel(SensDataArgs a)
{
    const int n = a.n, m = a.m, nn = n * n, E = nn + m * n;
    const long long total = (long long)a.batch * E;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long b = t / E;
        const int e = (int)(t - b * E);
        const bool valid = a.n_active[b] >= 0;
        const double *gq = a.gq + b * n, *x = a.x + b * n;
        if (e < nn) {
            if (!a.gP) continue;
            const int i = e / n, j = e - i * n;
            a.gP[b * nn + e] = valid ? 0.5 * (gq[i] * x[j] + x[i] * gq[j]) : 0.0;
        } else {
            if (!a.gA) continue;
            const int r = (e - nn) / n, j = (e - nn) - r * n;
            double v = 0.0;
            if (valid) {
                const unsigned long long rows = a.active[2 * b] | a.active[2 * b + 1];
                const double ya = ((rows >> r) & 1ull) ? a.y[b * m + r] : 0.0;
                const double w = a.gl[b * m + r] + a.gu[b * m + r];
                v = ya * gq[j] - w * x[j];
            }
            a.gA[b * (long long)(m * n) + (e - nn)] = v;
        }
    }
}

}  // namespace mpcq

extern "C" int mpcq_internal_sens_data_launch(const mpcq::SensDataArgs *a, hipStream_t s)
{
    if (a->n <= 0 || a->n > mpcq::kSensMaxN || a->m < 0 || a->m > mpcq::kSensMaxM) return -1;
    if (a->batch <= 0 || (!a->gP && !a->gA)) return 0;
    const int E = a->n * a->n + a->m * a->n;
    if (a->shared) {
        const int chunks = (a->batch + mpcq::kSensChunk - 1) / mpcq::kSensChunk;
        hipLaunchKernelGGL(mpcq::sens_contract_kernel, dim3(chunks), dim3(mpcq::kSensChunk), 0, s, *a);
        if (hipGetLastError() != hipSuccess) return -2;
        hipLaunchKernelGGL(mpcq::sens_reduce_kernel, dim3((E + 255) / 256), dim3(256), 0, s, *a, chunks);
    } else {
        const long long total = (long long)a->batch * E;
        const int grid = (int)std::min<long long>((total + 255) / 256, 65536);
        hipLaunchKernelGGL(mpcq::sens_outer_kernel, dim3(grid), dim3(256), 0, s, *a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

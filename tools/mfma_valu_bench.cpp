// tools/mfma_valu_bench.cpp — micro-benchmark of the gfx950 issue model that the tile kernel's hot
// loop lives in (dev tool, run on the GPU box): cycles per loop iteration (s_memtime, shader clock)
// of a wave that issues MF v_mfma_f32_16x16x4_f32 (4 independent accumulators) and NV vector ops
// (v_fma_f32, or v_pk_fma_f32 when PK), spread evenly between the MFMAs, at W waves per SIMD.
// f64 part: v_mfma_f64_16x16x4_f64 against v_mfma_f64_4x4x4_4b_f64 (back to back, dependent chains,
// and the tile kernel's pattern: NF 5-deep 16x16x4 chains interleaved k-step by k-step with NR 5-deep
// 4x4x4 chains), and an exact layout check of a 20-row product as one 16x16x4 tile + one 4x4x4
// remainder in the tile layout (exit status 1 on a mismatch).
//   build: hipcc -O3 --offload-arch=gfx950 -o /tmp/mvb tools/mfma_valu_bench.cpp
//   run:   /tmp/mvb            (all)      /tmp/mvb f64      (f64 part only)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

template <int MF, int NV, bool PK, int KIND = 0>
__global__ __launch_bounds__(64) void bench(long long *out, int iters, float seed)
{
    f4 acc[4] = {{seed, 0, 0, 0}, {0, seed, 0, 0}, {0, 0, seed, 0}, {0, 0, 0, seed}};
    typedef float f16v __attribute__((ext_vector_type(16)));
    f16v acc16[2] = {f16v{} + seed, f16v{} + 2 * seed};
    float v[8];
    f2 p[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        v[i] = seed * (i + 1);
        p[i] = f2{seed * i, seed + i};
    }
    const float a = seed * 0.5f, b = seed * 0.25f;
    const f2 a2 = {a, b};
    long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int m = 0; m < (MF > 0 ? MF : 1); m++) {
            if (MF > 0 && KIND == 0) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[m & 3]) : "v"(a), "v"(b));
            if (MF > 0 && KIND == 1) asm volatile("v_mfma_f32_4x4x1_16b_f32 %0, %1, %2, %0" : "+v"(acc[m & 3]) : "v"(a), "v"(b));
            if (MF > 0 && KIND == 2) asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+v"(acc16[m & 1]) : "v"(a), "v"(b));
            constexpr int per = MF > 0 ? NV / MF : NV;
#pragma unroll
            for (int k = 0; k < per; k++) {
                if (PK)
                    asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(p[k & 7]) : "v"(a2), "v"(a2));
                else
                    asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(v[k & 7]) : "v"(a), "v"(b));
            }
        }
    }
    long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    s += acc16[0][0] + acc16[1][5];
#pragma unroll
    for (int i = 0; i < 8; i++) s += v[i] + p[i][0] + p[i][1];
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = t1 - t0;
        out[2 * blockIdx.x + 1] = (long long)s;  // keep the arithmetic alive
    }
}

template <int MF, int NV, bool PK, int KIND = 0>
void run(int waves_per_simd)
{
    const int blocks = 1024 * waves_per_simd, iters = 2000;
    long long *d;
    hipMalloc(&d, 16 * blocks);
    hipLaunchKernelGGL((bench<MF, NV, PK, KIND>), dim3(blocks), dim3(64), 0, 0, d, 10, 1.0f);  // warm
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipEventRecord(e0, 0);
    hipLaunchKernelGGL((bench<MF, NV, PK, KIND>), dim3(blocks), dim3(64), 0, 0, d, iters, 1.0f);
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    std::vector<long long> h(2 * blocks);
    hipMemcpy(h.data(), d, 16 * blocks, hipMemcpyDeviceToHost);
    double sum = 0;
    for (int i = 0; i < blocks; i++) sum += h[2 * i];
    const double cyc = sum / blocks / iters;
    const double fl = KIND == 0 ? 2048.0 : (KIND == 1 ? 512.0 : 4096.0);
    const double mf_tflops = (double)blocks * iters * MF * fl / (ms * 1e-3) / 1e12;
    std::printf("{\"kind\": %d, \"mfma\": %d, \"valu\": %d, \"pk\": %d, \"waves_per_simd\": %d, \"cycles_per_iter_per_wave\": %.1f, "
                "\"simd_cycles_per_wave_iter\": %.1f, \"ms\": %.3f, \"mfma_tflops\": %.1f, \"clk_ghz\": %.3f}\n",
                KIND, MF, NV, (int)PK, waves_per_simd, cyc, cyc / waves_per_simd, ms, mf_tflops, cyc * iters / (ms * 1e-3) / 1e9);
    hipFree(d);
}

typedef double d4 __attribute__((ext_vector_type(4)));

// One loop iteration = one "product": KS k-steps, each issuing NF v_mfma_f64_16x16x4_f64 (one per full-tile
// chain) and then NR v_mfma_f64_4x4x4_4b_f64 (one per remainder chain).  DEP: the chains run on from
// iteration to iteration (every MFMA depends on the one KS.. before it); else 4 (16x16x4) / 8 (4x4x4)
// accumulators rotate, so nothing waits on a result.
template <int NF, int NR, int KS, bool DEP>
__global__ __launch_bounds__(64) void bench64(long long *out, int iters, double seed)
{
    constexpr int AF = DEP ? (NF > 0 ? NF : 1) : 4, AR = DEP ? (NR > 0 ? NR : 1) : 8;
    d4 acc[AF];
    double rem[AR];
#pragma unroll
    for (int i = 0; i < AF; i++) acc[i] = d4{seed, 0, seed * i, 0};
#pragma unroll
    for (int i = 0; i < AR; i++) rem[i] = seed * i;
    const double a = seed * 0.5, b = seed * 0.25;
    long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int s = 0; s < KS; s++) {
#pragma unroll
            for (int t = 0; t < NF; t++) {
                const int k = DEP ? t : (s * NF + t) % AF;
                acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[k], 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < NR; t++) {
                const int k = DEP ? t : (s * NR + t) % AR;
                rem[k] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, rem[k], 0, 0, 0);
            }
        }
    }
    long long t1 = __builtin_amdgcn_s_memtime();
    double sum = 0;
#pragma unroll
    for (int i = 0; i < AF; i++) sum += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
#pragma unroll
    for (int i = 0; i < AR; i++) sum += rem[i];
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = t1 - t0;
        out[2 * blockIdx.x + 1] = (long long)sum;  // keep the arithmetic alive
    }
}

template <int NF, int NR, int KS, bool DEP>
void run64(int waves_per_simd)
{
    const int blocks = 1024 * waves_per_simd, iters = 2000;
    long long *d;
    hipMalloc(&d, 16 * blocks);
    hipLaunchKernelGGL((bench64<NF, NR, KS, DEP>), dim3(blocks), dim3(64), 0, 0, d, 10, 1.0);  // warm
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipEventRecord(e0, 0);
    hipLaunchKernelGGL((bench64<NF, NR, KS, DEP>), dim3(blocks), dim3(64), 0, 0, d, iters, 1.0);
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    std::vector<long long> h(2 * blocks);
    hipMemcpy(h.data(), d, 16 * blocks, hipMemcpyDeviceToHost);
    double sum = 0;
    for (int i = 0; i < blocks; i++) sum += h[2 * i];
    const double cyc = sum / blocks / iters;
    std::printf("{\"kind\": \"f64\", \"mfma_16x16x4\": %d, \"mfma_4x4x4\": %d, \"k_steps\": %d, \"dependent\": %d, "
                "\"waves_per_simd\": %d, \"cycles_per_iter_per_wave\": %.1f, \"simd_cycles_per_wave_iter\": %.1f, "
                "\"ms\": %.3f, \"clk_ghz\": %.3f}\n",
                NF, NR, KS, (int)DEP, waves_per_simd, cyc, cyc / waves_per_simd, ms, cyc * iters / (ms * 1e-3) / 1e9);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipFree(d);
}

// Layout check: Y = A X, A 20 x 20, X 20 x 16 (one QP per column), as the tile kernel lays it out: lane
// (g, c) = 16 g + c holds x[4 s + g] of column c in register s; rows 0-15 on one 16x16x4 tile (A
// fragment of lane l and k-step s = A[l & 15][4 s + (l >> 4)], result register r = row 4 r + g), rows
// 16-19 on one 4x4x4 chain with the four blocks as the four column quads (A fragment = A[16 + (c & 3)]
// [4 s + g], same B register, result = row 16 + g of column c).
constexpr int LN = 20, LC = 16;
__global__ __launch_bounds__(64) void layout_probe(const double *A, const double *X, double *Y)
{
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
    d4 acc = {0, 0, 0, 0};
    double rem = 0;
#pragma unroll
    for (int s = 0; s < LN / 4; s++) {
        const double x = X[(4 * s + g) * LC + c];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(lane & 15) * LN + 4 * s + g], x, acc, 0, 0, 0);
        rem = __builtin_amdgcn_mfma_f64_4x4x4f64(A[(16 + (c & 3)) * LN + 4 * s + g], x, rem, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) Y[(4 * r + g) * LC + c] = acc[r];
    Y[(16 + g) * LC + c] = rem;
}

int layout_check()
{
    std::vector<double> A(LN * LN), X(LN * LC), Y(LN * LC, -1.0), R(LN * LC, 0.0);
    unsigned u = 12345u;
    auto next = [&]() { u = u * 1664525u + 1013904223u; return (double)((int)((u >> 16) % 19u) - 9); };
    for (auto &v : A) v = next();
    for (auto &v : X) v = next();
    for (int i = 0; i < LN; i++)
        for (int j = 0; j < LC; j++)
            for (int k = 0; k < LN; k++) R[i * LC + j] += A[i * LN + k] * X[k * LC + j];
    double *dA, *dX, *dY;
    hipMalloc(&dA, A.size() * 8);
    hipMalloc(&dX, X.size() * 8);
    hipMalloc(&dY, Y.size() * 8);
    hipMemcpy(dA, A.data(), A.size() * 8, hipMemcpyHostToDevice);
    hipMemcpy(dX, X.data(), X.size() * 8, hipMemcpyHostToDevice);
    hipMemcpy(dY, Y.data(), Y.size() * 8, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(layout_probe, dim3(1), dim3(64), 0, 0, dA, dX, dY);
    const hipError_t err = hipMemcpy(Y.data(), dY, Y.size() * 8, hipMemcpyDeviceToHost);
    hipFree(dA);
    hipFree(dX);
    hipFree(dY);
    if (err != hipSuccess) {
        std::printf("{\"layout_check\": \"error\", \"hip\": \"%s\"}\n", hipGetErrorString(err));
        return 1;
    }
    int bad_full = 0, bad_rem = 0;
    for (int i = 0; i < LN; i++)
        for (int j = 0; j < LC; j++)
            if (Y[i * LC + j] != R[i * LC + j]) (i < 16 ? bad_full : bad_rem)++;
    std::printf("{\"layout_check\": \"%s\", \"mismatch_rows_0_15\": %d, \"mismatch_rows_16_19\": %d}\n",
                bad_full + bad_rem ? "FAIL" : "ok", bad_full, bad_rem);
    if (bad_full + bad_rem)  // the remainder rows as computed and as expected, to read the real mapping from
        for (int i = 16; i < LN; i++) {
            std::printf("row %d got:", i);
            for (int j = 0; j < LC; j++) std::printf(" %g", Y[i * LC + j]);
            std::printf("\nrow %d ref:", i);
            for (int j = 0; j < LC; j++) std::printf(" %g", R[i * LC + j]);
            std::printf("\n");
        }
    return bad_full + bad_rem ? 1 : 0;
}

int f64_part()
{
    const int rc = layout_check();
    for (int w : {1, 2}) {
        run64<1, 0, 32, false>(w);  // back to back, independent accumulators: 32 MFMAs per iteration
        run64<0, 1, 32, false>(w);
        run64<1, 0, 5, true>(w);    // one dependent chain, 5 per iteration
        run64<0, 1, 5, true>(w);
        run64<0, 2, 5, true>(w);
        run64<1, 1, 5, true>(w);    // the kernel's patterns: full-tile chains + remainder chains
        run64<1, 2, 5, true>(w);
        run64<2, 0, 5, true>(w);    // (= 1 + 1 with the remainder as a padded tile)
        run64<2, 1, 5, true>(w);
        run64<2, 2, 5, true>(w);    // the stacked [B~; S] product at n = 20
        run64<3, 0, 5, true>(w);    // (= 2 + 1 or 2 + 2 padded)
        run64<4, 0, 5, true>(w);    // G = 2 groups of 2 padded tiles
        run64<2, 4, 5, true>(w);    // G = 2 groups of 1 tile + 2 chains
        run64<4, 4, 5, true>(w);    // G = 2 groups of 2 tiles + 2 chains
        run64<6, 0, 5, true>(w);    // G = 2 groups of 3 padded tiles
    }
    return rc;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "f64")) return f64_part();
    for (int w : {1, 2, 4}) {
        run<32, 0, false, 0>(w);
        run<32, 0, false, 1>(w);
        run<32, 0, false, 2>(w);
        run<32, 64, false, 1>(w);
        run<32, 64, false, 2>(w);
    }
    return f64_part();
}

// solvempc_amd/csrc/mpcq_mimo_run.hip — what runs between the control steps of a closed-loop MIMO run
// (mpcq_mimo_simulate_device, mpcq_mimo_run_device, mpcq_mimo_run_ref_device).  The control step
// itself is mpcq_mimo.hip's kernels, launched once per step by the host (mpcq_host_mimo.cpp), unchanged.
//   mimo_plant_kernel       the plant update, its noise, the record row and the two totals of one step, one pass
//   mimo_sched_tail_kernel  the padded tail of a reference schedule, at most once per call
#include "mpcq_internal.h"
#include "mpcq_mimo_plant_sim.h"

namespace mpcq {

constexpr int kPlantThreads = 256;  // four wavefronts of four 16-lane groups: 16 QPs per workgroup
constexpr int kPlantGroup = 16;     // lanes per QP (n_x <= 12, n_u <= 4)

// One 16-lane group per QP.  Lane i < n_x loads x_i once, lane j < n_u loads u_j once; the rows are
// mpcq_mimo_plant_sim.h's.  Every QP is owned by one group, so the totals are plain read-add-writes (no atomics) and
// two runs give identical bits.  With every record pointer NULL this is mpcq_mimo_simulate_device's update.
__global__ __launch_bounds__(kPlantThreads) void mimo_plant_kernel(MimoPlantArgs a)
{
    const long long tid = (long long)blockIdx.x * kPlantThreads + threadIdx.x;
    const long long b = tid / kPlantGroup;
    const int l = (int)(tid % kPlantGroup);
    const bool qp = b < a.batch;            // (whole groups beyond the batch stay for the shuffles, and touch nothing)
    const bool row = qp && l < a.nx, col = qp && l < a.nu;
    const size_t xi = (size_t)b * a.nx + l, ui = (size_t)b * a.nu + l;
    const double x = row ? a.X[xi] : 0.0;
    const double u = col ? a.U[ui] : 0.0;
    double w = 0.0;
    if (row) w = mimo_sim_noise(l, a.nx, sim_key(a.seed), (unsigned long long)(a.first_qp + b), a.step, a.noise_std);
    const double xn = mimo_sim_row(row, a.nx, a.nu, a.Ad + xi * a.nx, a.Bd + xi * a.nu, x, u, w);
    if (row) {
        a.X[xi] = xn;
        if (a.log_X) a.log_X[xi] = xn;
    }
    if (col && a.log_U) a.log_U[ui] = u;
    if (qp && l == 0) {
        if (a.log_status) a.log_status[b] = a.status[b];
        if (a.log_iter) a.log_iter[b] = a.iter[b];
        if (a.iters_total) a.iters_total[b] += a.iter[b];
        if (a.unsolved_total) a.unsolved_total[b] += a.status[b] != kSolved;
    }
}

// tail[r][j*ny + y] = sched[r*stride + min(base + j, len-1)*ny + y], j < blocks: one thread per value
__global__ void mimo_sched_tail_kernel(MimoTailArgs a)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (long long)a.blocks * a.ny;
    if (i >= a.rows * per) return;
    const long long r = i / per;
    const int j = (int)(i % per) / a.ny, y = (int)(i % per) % a.ny;
    const long long blk = a.base + j < a.len - 1 ? a.base + j : a.len - 1;
    a.tail[i] = a.sched[r * a.stride + blk * a.ny + y];
}

}  // namespace mpcq

extern "C" int mpcq_internal_mimo_plant_launch(const mpcq::MimoPlantArgs *a, hipStream_t s)
{
    if (a->nx < 1 || a->nx > 12 || a->nu < 1 || a->nu > 4) return -1;
    if (a->batch < 1) return 0;
    const long long threads = (long long)a->batch * mpcq::kPlantGroup;
    const unsigned grid = (unsigned)((threads + mpcq::kPlantThreads - 1) / mpcq::kPlantThreads);
    hipLaunchKernelGGL(mpcq::mimo_plant_kernel, dim3(grid), dim3(mpcq::kPlantThreads), 0, s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int mpcq_internal_mimo_sched_tail_launch(const mpcq::MimoTailArgs *a, hipStream_t s)
{
    if (a->rows < 1 || a->blocks < 1 || a->ny < 1 || a->len < 1 || a->base < 0) return -1;
    const long long total = a->rows * a->blocks * a->ny;
    hipLaunchKernelGGL(mpcq::mimo_sched_tail_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, *a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

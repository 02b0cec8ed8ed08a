// solvempc_amd/csrc/mpcq_log.hip — one row of a receding-horizon stream's per-step record
// (mpcq_mpc_set_stream_log) on the per-step path of mpcq_mpc_run_device: launched (captured) after each step's
// plant update and before the step counter's tick, so the row index comes from the context's device step
// counter, as the captured plant simulation's noise draw does.  The one-launch stream kernels write their
// rows themselves (mpcq_tile.h, mpcq_wave.h LOG variants).
#include "mpcq_internal.h"

namespace mpcq {

// One thread per QP: U and X as the step left them, status and iter of its solve.
__global__ void log_row_kernel(int nx, const double *X, const double *U, const int *status, const int *iter, LogArgs lg)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= lg.batch) return;
    const size_t e = lg.at(0, b);
    if (lg.U) lg.U[e] = U[b];
    if (lg.status) lg.status[e] = status[b];
    if (lg.iter) lg.iter[e] = iter[b];
    if (lg.X)
        for (int i = 0; i < nx; i++) lg.X[e * (size_t)nx + i] = X[(size_t)b * nx + i];
}

}  // namespace mpcq

extern "C" int mpcq_internal_log_row(int nx, const double *X, const double *U, const int *status, const int *iter,
                                     const mpcq::LogArgs *lg, hipStream_t s)
{
    if (!lg || lg->batch <= 0) return -1;
    hipLaunchKernelGGL(mpcq::log_row_kernel, dim3((lg->batch + 255) / 256), dim3(256), 0, s, nx, X, U, status, iter, *lg);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

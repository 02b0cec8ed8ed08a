// solvempc_amd/csrc/mpcq_mimo_plant_sim.h — one row of the simulated MIMO plant between two control steps of a
// closed-loop run (mpcq_mimo_simulate_device, mpcq_mimo_run*_device),
//     X_b <- Ad_b X_b + Bd_b U_b + w,   w ~ N(0, noise_std^2 I),
// for a 16-lane group per QP (n_x <= 12, n_u <= 4): lane i holds x_i and u_i and forms row i.  The noise is
// mpcq_plant_sim.h's counter-based generator (uni, sim_key) read exactly as sim_row reads it, so
// workload.plant_noise(seed, first_qp + b, 1, step, n_x, noise_std) restates every draw on the host.
#pragma once
#include "mpcq_plant_sim.h"

namespace mpcq {

// w_i of the QP with global index idx at control step `step`: component i < ceil(nx/2) is the cosine of Box-Muller
// pair i, the others the sine of pair i - ceil(nx/2); the pair p reads draws step*64 + 2p, 2p + 1.  noise_std == 0
// draws nothing.
__device__ __forceinline__ double mimo_sim_noise(int i, int nx, unsigned long long key, unsigned long long idx,
                                                 long long step, double noise_std)
{
    if (noise_std == 0.0) return 0.0;
    const int np = (nx + 1) / 2;
    const int p = i < np ? i : i - np;
    const unsigned long long d0 = (unsigned long long)step * 64ull + 2ull * p;
    const double r = sqrt(-2.0 * log(uni(key, idx, d0)));
    const double th = 2.0 * M_PI * uni(key, idx, d0 + 1);
    return noise_std * (i < np ? r * cos(th) : r * sin(th));
}

// Row i of Ad x + Bd u + w for lane i of a 16-lane group: x and u are this lane's x_i and u_i (0 beyond n_x, n_u),
// every other component arrives by __shfl(., t, 16), so no lane reads X from memory after any lane has written it
// and the in-place update does not depend on lockstep execution.  Every lane of the wavefront must call it (the
// shuffles are wave-wide); `live` lanes (i < n_x of a QP inside the batch) read A_row = Ad_b + i n_x and
// B_row = Bd_b + i n_u, the others read nothing and return 0.
// The sum is sum_t Ad[i,t] x_t in ascending t, then sum_j Bd[i,j] u_j in ascending j, then + w, in fp64 with every
// product rounded before it is added (no FMA: the library is built with -ffp-contract=off), which is the order
// of workload.simulate_mimo's per-QP loop.
__device__ __forceinline__ double mimo_sim_row(bool live, int nx, int nu, const double *A_row, const double *B_row,
                                               double x, double u, double w)
{
    double s = 0.0;
    for (int t = 0; t < nx; t++) {
        const double xt = __shfl(x, t, 16);
        if (live) s += A_row[t] * xt;
    }
    for (int j = 0; j < nu; j++) {
        const double uj = __shfl(u, j, 16);
        if (live) s += B_row[j] * uj;
    }
    return s + w;
}

}  // namespace mpcq

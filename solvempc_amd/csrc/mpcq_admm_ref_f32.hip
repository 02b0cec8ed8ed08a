// solvempc_amd/csrc/mpcq_admm_ref_f32.hip — f32 instantiations of the lane kernel's REF variant (per-QP horizon
// references, RefArgs: mpcq_mpc_step_ref*, the per-step graph of mpcq_mpc_run_ref_device).
#define MPCQ_LANE_REF 1
#include "mpcq_admm.h"

extern "C" int mpcq_internal_admm_ref_launch_f32(const mpcq::AdmmArgs<float> *a, int nc, int mc, const mpcq::RefArgs *ref,
                                                 hipStream_t s)
{
    if (!ref || !ref->p) return -1;
    return mpcq::launch_any<float>(*a, nc, mc, s, ref);
}

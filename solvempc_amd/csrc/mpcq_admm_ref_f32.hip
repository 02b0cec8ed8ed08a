// solvempc_amd/csrc/mpcq_admm_ref_f32.hip — f32 instantiations of the lane kernel's REF variant (per-QP horizon
// references, RefArgs: mpcq_mpc_step_ref*, the per-step graph of mpcq_mpc_run_ref_device).
#define MPCQ_LANE_REF 1
#include "mpcq_admm.h"

template <> int mpcq::lane_unit<mpcq::Variant::Ref, float>(const AdmmArgs<float> &a, int nc, int mc, const RefArgs *ref, hipStream_t s)
{
    return launch_any<float>(a, nc, mc, s, ref);
}

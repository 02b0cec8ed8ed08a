// solvempc_amd/csrc/mpcq_wave_ref_f32.hip — f32 instantiations of the one-QP-per-wave kernel's REF variant
// (per-QP horizon references, RefArgs: mpcq_mpc_step_ref*, mpcq_mpc_run_ref_device).
#define MPCQ_WAVE_REF 1
#include "mpcq_wave.h"

extern "C" int mpcq_internal_wave_ref_launch_f32(const mpcq::AdmmArgs<float> *a, int nc, int mc, int grid,
                                                 const mpcq::RefArgs *ref, hipStream_t s)
{
    if (!ref || !ref->p) return -1;
    return mpcq::wave_launch_any<float>(*a, nc, mc, grid, s, ref);
}

extern "C" int mpcq_internal_stream_ref_launch_f32(const mpcq::AdmmArgs<float> *a, int nc, int mc, const mpcq::StreamArgs *sa,
                                                   const mpcq::RefArgs *ref, hipStream_t s)
{
    if (!ref || !ref->p) return -1;
    return mpcq::stream_launch_any<float>(*a, nc, mc, *sa, s, ref);
}

// solvempc_amd/csrc/mpcq_wave_ref_f32.hip — f32 instantiations of the one-QP-per-wave kernel's REF variant
// (per-QP horizon references, RefArgs: mpcq_mpc_step_ref*, mpcq_mpc_run_ref_device).
#define MPCQ_WAVE_REF 1
#include "mpcq_wave.h"

template <> int mpcq::wave_unit<mpcq::Variant::Ref, float>(const AdmmArgs<float> &a, int nc, int mc, int grid, const RefArgs *ref, hipStream_t s)
{
    return wave_launch_any<float>(a, nc, mc, grid, s, ref);
}

template <> int mpcq::wave_stream_unit<mpcq::Variant::Ref, float>(const AdmmArgs<float> &a, int nc, int mc, const StreamArgs &sa,
                                                                   const RefArgs *ref, const LogArgs *, hipStream_t s)
{
    return stream_launch_any<float>(a, nc, mc, sa, s, ref);
}

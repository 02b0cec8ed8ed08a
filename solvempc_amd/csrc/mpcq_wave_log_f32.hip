// solvempc_amd/csrc/mpcq_wave_log_f32.hip — f32 instantiations of the one-QP-per-wave stream kernel with the per-step
// record (REF + LOG: RefArgs and LogArgs as trailing kernel arguments; mpcq_mpc_set_stream_log).
#define MPCQ_WAVE_REF 1
#define MPCQ_WAVE_LOG 1
#include "mpcq_wave.h"

template <> int mpcq::wave_stream_unit<mpcq::Variant::RefLog, float>(const AdmmArgs<float> &a, int nc, int mc, const StreamArgs &sa,
                                                                      const RefArgs *ref, const LogArgs *lg, hipStream_t s)
{
    return stream_launch_any<float>(a, nc, mc, sa, s, ref, lg);
}

// solvempc_amd/csrc/mpcq_wave_log_f32.hip — f32 instantiations of the one-QP-per-wave stream kernel with the per-step
// record (REF + LOG: RefArgs and LogArgs as trailing kernel arguments; mpcq_mpc_set_stream_log).
#define MPCQ_WAVE_REF 1
#define MPCQ_WAVE_LOG 1
#include "mpcq_wave.h"

extern "C" int mpcq_internal_stream_log_launch_f32(const mpcq::AdmmArgs<float> *a, int nc, int mc, const mpcq::StreamArgs *sa,
                                                   const mpcq::RefArgs *ref, const mpcq::LogArgs *lg, hipStream_t s)
{
    if (!ref || !ref->p || !lg) return -1;
    return mpcq::stream_launch_any<float>(*a, nc, mc, *sa, s, ref, lg);
}

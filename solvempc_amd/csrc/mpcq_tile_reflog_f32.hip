// solvempc_amd/csrc/mpcq_tile_reflog_f32.hip — fp32 instantiations of the tile kernel's stream mode with the
// per-step record (REF + LOG: RefArgs and LogArgs as trailing kernel arguments; mpcq_mpc_set_stream_log).
#define MPCQ_TILE_REF 1
#define MPCQ_TILE_LOG 1
#include "mpcq_tile.h"

extern "C" int mpcq_internal_tile_reflog_stream_launch_f32(const mpcq::AdmmArgs<float> *a, int KN, int KM,
                                                           const mpcq::RefArgs *ref, const mpcq::LogArgs *lg, hipStream_t s)
{
    if (!ref || !ref->p || !lg) return -1;
    return mpcq::tile_stream_launch_any<float>(*a, KN, KM, s, ref, lg);
}

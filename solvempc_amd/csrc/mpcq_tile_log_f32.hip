// solvempc_amd/csrc/mpcq_tile_log_f32.hip — fp32 instantiations of the scalar tile kernel's stream mode with the
// per-step record (LOG: LogArgs as a trailing kernel argument; mpcq_mpc_set_stream_log on mpcq_mpc_run_device).
#define MPCQ_TILE_LOG 1
#include "mpcq_tile.h"

template <> int mpcq::tile_stream_unit<mpcq::Variant::Log, float>(const AdmmArgs<float> &a, int KN, int KM, const RefArgs *,
                                                                   const LogArgs *lg, hipStream_t s)
{
    return tile_stream_launch_any<float>(a, KN, KM, s, nullptr, lg);
}

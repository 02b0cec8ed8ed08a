// solvempc_amd/csrc/mpcq_tile_log_f64.hip — fp64 and mixed instantiations of the scalar tile kernel's stream mode with the
// per-step record (LOG: LogArgs as a trailing kernel argument; mpcq_mpc_set_stream_log on mpcq_mpc_run_device).
#define MPCQ_TILE_LOG 1
#include "mpcq_tile.h"

extern "C" int mpcq_internal_tile_log_stream_launch_f64(const mpcq::AdmmArgs<double> *a, int KN, int KM, const mpcq::LogArgs *lg,
                                                        hipStream_t s)
{
    if (!lg) return -1;
    return mpcq::tile_stream_launch_any<double>(*a, KN, KM, s, nullptr, lg);
}

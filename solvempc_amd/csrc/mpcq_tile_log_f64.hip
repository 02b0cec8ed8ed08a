// solvempc_amd/csrc/mpcq_tile_log_f64.hip — fp64 and mixed instantiations of the scalar tile kernel's stream mode with the
// per-step record (LOG: LogArgs as a trailing kernel argument; mpcq_mpc_set_stream_log on mpcq_mpc_run_device).
#define MPCQ_TILE_LOG 1
#include "mpcq_tile.h"

template <> int mpcq::tile_stream_unit<mpcq::Variant::Log, double>(const AdmmArgs<double> &a, int KN, int KM, const RefArgs *,
                                                                    const LogArgs *lg, hipStream_t s)
{
    return tile_stream_launch_any<double>(a, KN, KM, s, nullptr, lg);
}

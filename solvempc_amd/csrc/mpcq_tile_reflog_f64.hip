// solvempc_amd/csrc/mpcq_tile_reflog_f64.hip — fp64 and mixed instantiations of the tile kernel's stream mode with
// the per-step record (REF + LOG: RefArgs and LogArgs as trailing kernel arguments; mpcq_mpc_set_stream_log).
#define MPCQ_TILE_REF 1
#define MPCQ_TILE_LOG 1
#include "mpcq_tile.h"

template <> int mpcq::tile_stream_unit<mpcq::Variant::RefLog, double>(const AdmmArgs<double> &a, int KN, int KM, const RefArgs *ref,
                                                                       const LogArgs *lg, hipStream_t s)
{
    return tile_stream_launch_any<double>(a, KN, KM, s, ref, lg);
}

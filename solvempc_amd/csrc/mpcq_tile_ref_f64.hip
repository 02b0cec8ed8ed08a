// solvempc_amd/csrc/mpcq_tile_ref_f64.hip — fp64 instantiations of the tile (MFMA) ADMM kernel's REF variant
// (per-QP horizon references, RefArgs: mpcq_mpc_step_ref*, mpcq_mpc_run_ref_device).
#define MPCQ_TILE_REF 1
#include "mpcq_tile.h"

template <> int mpcq::tile_unit<mpcq::Variant::Ref, double>(const AdmmArgs<double> &a, int KN, int KM, const RefArgs *ref, hipStream_t s)
{
    return tile_launch_any<double>(a, KN, KM, s, ref);
}

template <> int mpcq::tile_stream_unit<mpcq::Variant::Ref, double>(const AdmmArgs<double> &a, int KN, int KM, const RefArgs *ref,
                                                                    const LogArgs *, hipStream_t s)
{
    return tile_stream_launch_any<double>(a, KN, KM, s, ref);
}

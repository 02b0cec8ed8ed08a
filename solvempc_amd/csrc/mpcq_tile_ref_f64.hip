// solvempc_amd/csrc/mpcq_tile_ref_f64.hip — fp64 instantiations of the tile (MFMA) ADMM kernel's REF variant
// (per-QP horizon references, RefArgs: mpcq_mpc_step_ref*, mpcq_mpc_run_ref_device).
#define MPCQ_TILE_REF 1
#include "mpcq_tile.h"

extern "C" int mpcq_internal_tile_ref_launch_f64(const mpcq::AdmmArgs<double> *a, int KN, int KM, const mpcq::RefArgs *ref,
                                                 hipStream_t s)
{
    if (!ref || !ref->p) return -1;
    return mpcq::tile_launch_any<double>(*a, KN, KM, s, ref);
}

extern "C" int mpcq_internal_tile_ref_stream_launch_f64(const mpcq::AdmmArgs<double> *a, int KN, int KM,
                                                        const mpcq::RefArgs *ref, hipStream_t s)
{
    if (!ref || !ref->p) return -1;
    return mpcq::tile_stream_launch_any<double>(*a, KN, KM, s, ref);
}

// solvempc_amd/csrc/mpcq_tile_f64.hip — fp64 instantiations of the tile (MFMA) ADMM kernel.
#include "mpcq_tile.h"

template <> int mpcq::tile_unit<mpcq::Variant::Scalar, double>(const AdmmArgs<double> &a, int KN, int KM, const RefArgs *, hipStream_t s)
{
    return tile_launch_any<double>(a, KN, KM, s);
}

template <> int mpcq::tile_stream_unit<mpcq::Variant::Scalar, double>(const AdmmArgs<double> &a, int KN, int KM, const RefArgs *,
                                                                       const LogArgs *, hipStream_t s)
{
    return tile_stream_launch_any<double>(a, KN, KM, s);
}

template <> int mpcq::launch_tile_publish<double>(const AdmmArgs<double> &a, int KN, int KM, bool paired, hipStream_t s)
{
    return tile_publish_any<double>(a, KN, KM, paired, s);
}

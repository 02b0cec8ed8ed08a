// solvempc_amd/csrc/mpcq_tile_f32.hip — fp32 instantiations of the tile (MFMA) ADMM kernel.
#include "mpcq_tile.h"

template <> int mpcq::tile_unit<mpcq::Variant::Scalar, float>(const AdmmArgs<float> &a, int KN, int KM, const RefArgs *, hipStream_t s)
{
    return tile_launch_any<float>(a, KN, KM, s);
}

template <> int mpcq::tile_stream_unit<mpcq::Variant::Scalar, float>(const AdmmArgs<float> &a, int KN, int KM, const RefArgs *,
                                                                      const LogArgs *, hipStream_t s)
{
    return tile_stream_launch_any<float>(a, KN, KM, s);
}

template <> int mpcq::launch_tile_publish<float>(const AdmmArgs<float> &a, int KN, int KM, bool paired, hipStream_t s)
{
    return tile_publish_any<float>(a, KN, KM, paired, s);
}

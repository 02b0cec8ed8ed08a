// solvempc_amd/csrc/mpcq_wave_f32.hip — f32 instantiations of the one-QP-per-wave kernel (mpcq_wave.h).
#include "mpcq_wave.h"

template <> int mpcq::wave_unit<mpcq::Variant::Scalar, float>(const AdmmArgs<float> &a, int nc, int mc, int grid, const RefArgs *, hipStream_t s)
{
    return wave_launch_any<float>(a, nc, mc, grid, s);
}

template <> int mpcq::wave_stream_unit<mpcq::Variant::Scalar, float>(const AdmmArgs<float> &a, int nc, int mc, const StreamArgs &sa,
                                                                      const RefArgs *, const LogArgs *, hipStream_t s)
{
    return stream_launch_any<float>(a, nc, mc, sa, s);
}

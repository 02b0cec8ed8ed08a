// solvempc_amd/csrc/mpcq_wave_f64.hip — f64 instantiations of the one-QP-per-wave kernel (mpcq_wave.h).
#include "mpcq_wave.h"

template <> int mpcq::wave_unit<mpcq::Variant::Scalar, double>(const AdmmArgs<double> &a, int nc, int mc, int grid, const RefArgs *, hipStream_t s)
{
    return wave_launch_any<double>(a, nc, mc, grid, s);
}

template <> int mpcq::wave_stream_unit<mpcq::Variant::Scalar, double>(const AdmmArgs<double> &a, int nc, int mc, const StreamArgs &sa,
                                                                       const RefArgs *, const LogArgs *, hipStream_t s)
{
    return stream_launch_any<double>(a, nc, mc, sa, s);
}

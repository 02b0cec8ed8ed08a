// solvempc_amd/csrc/mpcq_admm_f64.hip — fp64 instantiations of the lane kernel (mpcq_admm.h).
#include "mpcq_admm.h"

extern "C" int mpcq_internal_caps(int n, int m, int *nc, int *mc)
{
    static constexpr mpcq::Cap caps[] = {MPCQ_CAPS(MPCQ_CAP_ITEM)};
    return mpcq::smallest_cap(caps, n, m, nc, mc) ? 0 : -1;
}

template <> int mpcq::lane_unit<mpcq::Variant::Scalar, double>(const AdmmArgs<double> &a, int nc, int mc, const RefArgs *, hipStream_t s)
{
    return launch_any<double>(a, nc, mc, s);
}

template <> int mpcq::launch_warm_start<double>(const AdmmArgs<double> &a, int nc, int mc, const double *x, const double *y, hipStream_t s)
{
    return warm_any<double>(a, nc, mc, x, y, s);
}

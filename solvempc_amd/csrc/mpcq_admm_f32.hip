// solvempc_amd/csrc/mpcq_admm_f32.hip — fp32 instantiations of the lane kernel (mpcq_admm.h).
#include "mpcq_admm.h"

template <> int mpcq::lane_unit<mpcq::Variant::Scalar, float>(const AdmmArgs<float> &a, int nc, int mc, const RefArgs *, hipStream_t s)
{
    return launch_any<float>(a, nc, mc, s);
}

template <> int mpcq::launch_warm_start<float>(const AdmmArgs<float> &a, int nc, int mc, const double *x, const double *y, hipStream_t s)
{
    return warm_any<float>(a, nc, mc, x, y, s);
}

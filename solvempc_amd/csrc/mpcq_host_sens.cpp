// solvempc_amd/csrc/mpcq_host_sens.cpp — host side of the C ABI declared in include/mpcq.h: the sensitivities
// of the last solve of a generic context.
#include "mpcq_ctx.h"

// ---- active-set sensitivities of the last solve (mpcq_sens.hip; include/mpcq.h)
namespace {

// Staging block of the host forms, of the step gains' (gq, gu) and of what the data gradients read that the caller
// did not ask for: offsets in doubles, the ints and then the active-set masks (2 words per QP) last
struct SensStage {
    size_t g, gq, gl, gu, dX, dU, dref, nact, act, total;
    explicit SensStage(const mpcq_ctx *c)
    {
        const size_t B = c->dims.batch, n = c->dims.n, m = c->dims.m;
        g = 0; gq = g + B * n; gl = gq + B * n; gu = gl + B * m; dX = gu + B * m; dU = dX + B * 8;
        dref = dU + B; nact = dref + B * n; act = nact + (B + 1) / 2; total = act + 2 * B;
    }
};

int sens_stage(mpcq_ctx *c)
{
    return c->d_sens.alloc(8 * SensStage(c).total, "sensitivity staging");
}

// The refusals of include/mpcq.h, before anything is enqueued or written
int sens_check(mpcq_ctx *c, const char *fn, bool gains, bool any_out, hipStream_t s)
{
    if (!c) return fail(MPCQ_ERR_ARG, "null context");
    if (c->mimo_only || c->mode == mpcq_ctx::Mode::Mimo || c->dims.n > 32 || c->dims.m > 64)
        return fail(MPCQ_ERR_ARG, std::string(fn) + ": serves n <= 32, m <= 64 and no MIMO context");
    if (!any_out) return fail(MPCQ_ERR_ARG, std::string(fn) + ": every output is NULL");
    int rc = check_ctx(c, kGeneric);
    if (rc) return rc;
    if (gains && !c->mpc_ready) return fail(MPCQ_ERR_ARG, std::string(fn) + ": the context has no MPC operators");
    if (!c->sens_ok)
        return fail(MPCQ_ERR_ORDER, std::string(fn) + ": needs a solve (mpcq_solve / mpcq_mpc_step*) as the context's "
                                                      "last solver call; stream runs are not served");
    return refuse_capture(fn, s);
}

// The kernels on s, ordered after the context's last stream; the context's next launches ordered after them.
// Whatever the solve left lazy that the kernel reads (u of a tile-path controllerStep; status of an ordered
// chain) is published first, on the context's last stream.  dX .. dref non-null: the step gains' chain rule on
// (gq, gu), which are then staging buffers.
int sens_enqueue(mpcq_ctx *c, const double *g, double *gq, double *gl, double *gu, int *nact, double *dX, double *dU,
                 double *dref, bool chain, hipStream_t s, unsigned long long *act = nullptr, double *gP = nullptr,
                 double *gA = nullptr, double *part = nullptr)
{
    int rc = materialize_qu(c);
    if (rc || (rc = materialize_info(c))) return rc;
    if ((gP || gA) && (rc = materialize_xy(c))) return rc;  // (the data gradients read the solve's x, y)
    if ((rc = order_after_last(c, s))) return rc;
    mpcq::SensArgs a{};
    a.batch = c->dims.batch; a.n = c->dims.n; a.m = c->dims.m; a.nc = c->nc; a.mc = c->mc;
    a.shared = c->dims.n_plants == 1;
    a.is_f32 = c->dims.dtype == MPCQ_F32;
    a.ops_stride = c->ops_stride;
    a.ops = c->d_ops; a.P = c->d_P; a.A = c->d_A; a.l = c->d_l; a.u = c->d_u;
    a.zs = c->d_zs; a.ys = c->d_ys; a.status = c->d_status;
    a.g = g; a.gq = gq; a.gl = gl; a.gu = gu; a.n_active = nact; a.active = act;
    a.delta = c->set.delta;
    a.refine = c->set.polish_refine_iter;
    hipError_t err = hipSuccess;
    const int src = mpcq_internal_sens_launch(&a, c->cus, s, &err);
    if (src == -1) return fail(MPCQ_ERR_ARG, "sensitivity: the kernel serves n <= 32, m <= 64");
    if (src) return fail(MPCQ_ERR_HIP, std::string("sensitivity kernel launch failed: ") + hipGetErrorString(err));
    if (chain) {
        mpcq::SensChainArgs ca{};
        ca.batch = c->dims.batch; ca.n = c->dims.n; ca.m = c->dims.m; ca.nx = c->nx;
        ca.shared = c->dims.n_plants == 1;
        ca.Fx = c->d_Fx; ca.Fu = c->d_Fu; ca.Fr = c->d_Fr; ca.Sbar = c->d_Sbar; ca.Ku = c->d_Ku;
        ca.gq = gq; ca.gu = gu; ca.dX = dX; ca.dU = dU; ca.dref = dref;
        if (mpcq_internal_sens_chain_launch(&ca, s)) return fail(MPCQ_ERR_HIP, "step-gain kernel launch failed");
    }
    if (gP || gA) {
        mpcq::SensDataArgs da{};
        da.batch = c->dims.batch; da.n = c->dims.n; da.m = c->dims.m;
        da.shared = c->dims.n_plants == 1;
        da.gq = gq; da.gl = gl; da.gu = gu; da.x = c->d_x; da.y = c->d_y;
        da.active = act; da.n_active = nact; da.part = part; da.gP = gP; da.gA = gA;
        if (mpcq_internal_sens_data_launch(&da, s)) return fail(MPCQ_ERR_HIP, "data-gradient kernel launch failed");
    }
    return order_last_after(c, s);
}

// d_sdata with room for `doubles`
int sens_data_room(mpcq_ctx *c, size_t doubles)
{
    return c->d_sdata.grow(8 * doubles, c->last, "data-gradient staging");
}

// doubles of the shared plant's partial sums (0 for a per-plant context)
size_t sens_partials(const mpcq_ctx *c)
{
    if (c->dims.n_plants != 1) return 0;
    const size_t B = c->dims.batch, n = c->dims.n, m = c->dims.m;
    return (B + mpcq::kSensChunk - 1) / mpcq::kSensChunk * (n * n + m * n);
}

}  // namespace

extern "C" {

int mpcq_sensitivity_device(mpcq_ctx *c, const double *g, double *gq, double *gl, double *gu, int *n_active,
                            void *stream)
{
    int rc = sens_check(c, "mpcq_sensitivity_device", false, gq || gl || gu || n_active, (hipStream_t)stream);
    if (rc) return rc;
    return sens_enqueue(c, g, gq, gl, gu, n_active, nullptr, nullptr, nullptr, false, (hipStream_t)stream);
}

int mpcq_sensitivity(mpcq_ctx *c, const double *g, double *gq, double *gl, double *gu, int *n_active)
{
    int rc = sens_check(c, "mpcq_sensitivity", false, gq || gl || gu || n_active, c ? c->last : nullptr);
    if (rc || (rc = sens_stage(c))) return rc;
    const size_t B = c->dims.batch, n = c->dims.n, m = c->dims.m;
    const SensStage o(c);
    double *d = c->d_sens;
    if (g && (rc = h2d(d + o.g, g, 8 * B * n, c->last))) return rc;
    if ((rc = sens_enqueue(c, g ? d + o.g : nullptr, d + o.gq, d + o.gl, d + o.gu, (int *)(d + o.nact), nullptr, nullptr,
                           nullptr, false, c->last)))
        return rc;
    if ((rc = d2h(c, gq, d + o.gq, 8 * B * n)) || (rc = d2h(c, gl, d + o.gl, 8 * B * m)) ||
        (rc = d2h(c, gu, d + o.gu, 8 * B * m)) || (rc = d2h(c, n_active, d + o.nact, 4 * B)))
        return rc;
    HIPCHK(hipStreamSynchronize(c->last));
    return MPCQ_OK;
}

int mpcq_sensitivity_data_device(mpcq_ctx *c, const double *g, double *gq, double *gl, double *gu, double *gP, double *gA,
                                 unsigned long long *active, int *n_active, void *stream)
{
    int rc = sens_check(c, "mpcq_sensitivity_data_device", false, gq || gl || gu || gP || gA || active || n_active,
                        (hipStream_t)stream);
    if (rc) return rc;
    double *part = nullptr;
    if (gP || gA) {  // what the contraction reads and the caller did not ask for: the context's staging
        if ((rc = sens_stage(c)) || (rc = sens_data_room(c, sens_partials(c)))) return rc;
        const SensStage o(c);
        double *d = c->d_sens;
        if (!gq) gq = d + o.gq;
        if (!gl) gl = d + o.gl;
        if (!gu) gu = d + o.gu;
        if (!n_active) n_active = (int *)(d + o.nact);
        if (!active) active = (unsigned long long *)(d + o.act);
        part = c->d_sdata;
    }
    return sens_enqueue(c, g, gq, gl, gu, n_active, nullptr, nullptr, nullptr, false, (hipStream_t)stream, active, gP, gA,
                        part);
}

int mpcq_sensitivity_data(mpcq_ctx *c, const double *g, double *gq, double *gl, double *gu, double *gP, double *gA,
                          unsigned long long *active, int *n_active)
{
    int rc = sens_check(c, "mpcq_sensitivity_data", false, gq || gl || gu || gP || gA || active || n_active,
                        c ? c->last : nullptr);
    if (rc || (rc = sens_stage(c))) return rc;
    const size_t B = c->dims.batch, n = c->dims.n, m = c->dims.m;
    const size_t k = c->dims.n_plants == 1 ? 1 : B, np = sens_partials(c);
    if ((gP || gA) && (rc = sens_data_room(c, np + k * (n * n + m * n)))) return rc;
    const SensStage o(c);
    double *d = c->d_sens;
    double *dP = gP ? c->d_sdata + np : nullptr, *dA = gA ? c->d_sdata + np + k * n * n : nullptr;
    auto *dact = (unsigned long long *)(d + o.act);
    if (g && (rc = h2d(d + o.g, g, 8 * B * n, c->last))) return rc;
    if ((rc = sens_enqueue(c, g ? d + o.g : nullptr, d + o.gq, d + o.gl, d + o.gu, (int *)(d + o.nact), nullptr, nullptr,
                           nullptr, false, c->last, dact, dP, dA, c->d_sdata)))
        return rc;
    if ((rc = d2h(c, gq, d + o.gq, 8 * B * n)) || (rc = d2h(c, gl, d + o.gl, 8 * B * m)) ||
        (rc = d2h(c, gu, d + o.gu, 8 * B * m)) || (rc = d2h(c, n_active, d + o.nact, 4 * B)) ||
        (rc = d2h(c, active, dact, 16 * B)) || (rc = d2h(c, gP, dP, 8 * k * n * n)) || (rc = d2h(c, gA, dA, 8 * k * m * n)))
        return rc;
    HIPCHK(hipStreamSynchronize(c->last));
    return MPCQ_OK;
}

int mpcq_mpc_step_gains_device(mpcq_ctx *c, double *dX, double *dU, double *dref, int *n_active, void *stream)
{
    int rc = sens_check(c, "mpcq_mpc_step_gains_device", true, dX || dU || dref || n_active, (hipStream_t)stream);
    if (rc || (rc = sens_stage(c))) return rc;
    const SensStage o(c);
    double *d = c->d_sens;
    return sens_enqueue(c, nullptr, d + o.gq, nullptr, d + o.gu, n_active, dX, dU, dref, true, (hipStream_t)stream);
}

int mpcq_mpc_step_gains(mpcq_ctx *c, double *dX, double *dU, double *dref, int *n_active)
{
    int rc = sens_check(c, "mpcq_mpc_step_gains", true, dX || dU || dref || n_active, c ? c->last : nullptr);
    if (rc || (rc = sens_stage(c))) return rc;
    const size_t B = c->dims.batch, n = c->dims.n;
    const SensStage o(c);
    double *d = c->d_sens;
    if ((rc = sens_enqueue(c, nullptr, d + o.gq, nullptr, d + o.gu, (int *)(d + o.nact), d + o.dX, d + o.dU, d + o.dref,
                           true, c->last)))
        return rc;
    if ((rc = d2h(c, dX, d + o.dX, 8 * B * c->nx)) || (rc = d2h(c, dU, d + o.dU, 8 * B)) ||
        (rc = d2h(c, dref, d + o.dref, 8 * B * n)) || (rc = d2h(c, n_active, d + o.nact, 4 * B)))
        return rc;
    HIPCHK(hipStreamSynchronize(c->last));
    return MPCQ_OK;
}

}  // extern "C"

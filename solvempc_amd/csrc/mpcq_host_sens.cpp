// solvempc_amd/csrc/mpcq_host_sens.cpp — host side of the C ABI declared in include/mpcq.h: the sensitivities
// of the last solve, of generic and of MIMO contexts.
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

// The refusals of include/mpcq.h for the MIMO sensitivity calls, before anything is enqueued or written
int mimo_sens_check(mpcq_ctx *c, const char *fn, bool implicit_g, int n_rhs, bool any_out, hipStream_t s)
{
    int rc = check_ctx(c, kNone);
    if (rc) return rc;
    if (c->mode != mpcq_ctx::Mode::Mimo)
        return fail(MPCQ_ERR_ORDER, std::string(fn) + ": mpcq_mimo_setup_plants_device has not succeeded");
    if (!c->mimo_stepped)
        return fail(MPCQ_ERR_ORDER, std::string(fn) + ": needs a mpcq_mimo_step_device since the last setup");
    if (n_rhs < 1 || n_rhs > 4) return fail(MPCQ_ERR_ARG, std::string(fn) + ": 1 <= n_rhs <= 4");
    if (implicit_g && n_rhs > c->mimo_nu)
        return fail(MPCQ_ERR_ARG, std::string(fn) + ": g == NULL stands for the applied move's components, n_rhs <= n_u");
    if (!any_out) return fail(MPCQ_ERR_ARG, std::string(fn) + ": every output is NULL");
    return refuse_capture(fn, s);
}

// The kernel on s, ordered after the context's last stream; the context's next launches ordered after it.
// dref (batch * n_rhs * N n_y, or null): the chain rule on a horizon reference, Fr' gq.
int mimo_sens_enqueue(mpcq_ctx *c, const double *g, int n_rhs, double *gq, double *gu, double *dX, double *dU,
                      double *dyref, int *nact, hipStream_t s, double *dref = nullptr)
{
    if (int rc = order_after_last(c, s)) return rc;
    mpcq::MimoSensArgs a{};
    a.batch = c->dims.batch;
    a.N = c->mimo_N; a.nx = c->mimo_nx; a.nu = c->mimo_nu; a.ny = c->mimo_ny; a.s_rows = c->mimo_srows;
    a.n_rhs = n_rhs;
    a.ops_stride = (size_t)mpcq::MimoLayout::make(a.N, a.nx, a.nu, a.ny).total;
    a.ops = c->d_mimo;
    a.u = c->d_u;
    a.zs = (const double *)c->d_zs;
    a.ys = (const double *)c->d_ys;
    a.status = c->d_status;
    a.g = g;
    a.gq = gq; a.gu = gu;
    a.dX = dX; a.dU = dU; a.dyref = dyref; a.dref = dref;
    a.n_active = nact;
    a.delta = c->set.delta;
    a.refine = c->set.polish_refine_iter;
    hipError_t err = hipSuccess;
    const int lr = mpcq_internal_mimo_sens_launch(&a, c->cus, s, &err);
    if (lr == -1) return fail(MPCQ_ERR_ARG, "mimo sensitivity: shape beyond the kernel's capacity");
    if (lr) return fail(MPCQ_ERR_HIP, std::string("mimo sensitivity kernel launch failed: ") + hipGetErrorString(err));
    return order_last_after(c, s);
}

// ---- the MIMO step pulled back to the plant data (mpcq_mimo_plant_vjp.hip; include/mpcq.h)
// The nine plant arrays in the header's order (Ad, Bd, Cd, Q, R, RD, K, K0, w0) and their element counts per plant
struct MimoPlantPtrs {
    const double *in[9];
    double *out[9];
};

void mimo_plant_sizes(const mpcq_ctx *c, size_t sz[9])
{
    const size_t nx = c->mimo_nx, nu = c->mimo_nu, ny = c->mimo_ny;
    const size_t s[9] = {nx * nx, nx * nu, ny * nx, ny * ny, nu * nu, nu * nu, nu * nx, nu * nu, nu};
    std::copy(s, s + 9, sz);
}

// The refusals of include/mpcq.h, before anything is allocated, enqueued or written
int mimo_plant_vjp_check(mpcq_ctx *c, const char *fn, const MimoPlantPtrs &p, const double *X, const double *U_prev,
                         const int *n_active, hipStream_t s)
{
    int rc = check_ctx(c, kNone);
    if (rc) return rc;
    if (c->mode == mpcq_ctx::Mode::None)
        return fail(MPCQ_ERR_ORDER, std::string(fn) + ": mpcq_mimo_setup_plants_device has not succeeded");
    if (c->mode != mpcq_ctx::Mode::Mimo)
        return fail(MPCQ_ERR_ARG, std::string(fn) + ": the context was not set up by mpcq_mimo_setup_plants_device");
    if (!c->mimo_stepped)
        return fail(MPCQ_ERR_ORDER, std::string(fn) + ": needs a mpcq_mimo_step_device since the last setup");
    if (c->mimo_ref_step)  // (gFr would be formed from a yref the step did not use)
        return fail(MPCQ_ERR_ORDER, std::string(fn) + ": the last step was a mpcq_mimo_step_ref*, whose horizon "
                                                      "reference this call does not know; needs a mpcq_mimo_step_device");
    bool any_out = n_active != nullptr;
    for (int k = 0; k < 9; k++) {
        if (!p.in[k]) return fail(MPCQ_ERR_ARG, std::string(fn) + ": null plant array");
        any_out = any_out || p.out[k];
    }
    if (!X || !U_prev) return fail(MPCQ_ERR_ARG, std::string(fn) + ": null X / U_prev");
    if (!any_out) return fail(MPCQ_ERR_ARG, std::string(fn) + ": every output is NULL");
    return refuse_capture(fn, s);
}

// mimo_sens_kernel (n_rhs = 1) into the context's staging, then mimo_plant_vjp_kernel, both on s
int mimo_plant_vjp_enqueue(mpcq_ctx *c, const double *g, const MimoPlantPtrs &p, const double *X, const double *U_prev,
                           const double *yref, int *n_active, hipStream_t s)
{
    const size_t B = c->dims.batch, n = c->dims.n, m = c->dims.m;
    if (int rc = c->d_mimo_pv.alloc(8 * (B * (n + m) + (B + 1) / 2), "mimo plant-gradient staging")) return rc;
    double *gq = c->d_mimo_pv, *gu = gq + B * n;
    int *nact = (int *)(gu + B * m);
    if (int rc = mimo_sens_enqueue(c, g, 1, gq, gu, nullptr, nullptr, nullptr, nact, s)) return rc;
    mpcq::MimoPlantVjpArgs a{};
    a.batch = c->dims.batch;
    a.N = c->mimo_N; a.nx = c->mimo_nx; a.nu = c->mimo_nu; a.ny = c->mimo_ny; a.s_rows = c->mimo_srows;
    a.ops_stride = (size_t)mpcq::MimoLayout::make(a.N, a.nx, a.nu, a.ny).total;
    a.ops = c->d_mimo;
    a.u = c->d_u;
    a.zs = (const double *)c->d_zs;
    a.ys = (const double *)c->d_ys;
    a.x = c->d_x; a.y = c->d_y;
    a.gq = gq; a.gu = gu; a.nact = nact;
    a.Ad = p.in[0]; a.Bd = p.in[1]; a.Cd = p.in[2]; a.Q = p.in[3];
    a.X = X; a.U_prev = U_prev; a.yref = yref;
    a.gAd = p.out[0]; a.gBd = p.out[1]; a.gCd = p.out[2]; a.gQ = p.out[3]; a.gR = p.out[4]; a.gRD = p.out[5];
    a.gK = p.out[6]; a.gK0 = p.out[7]; a.gw0 = p.out[8];
    a.n_active = n_active;
    hipError_t err = hipSuccess;
    const int lr = mpcq_internal_mimo_plant_vjp_launch(&a, c->cus, s, &err);
    if (lr == -1) return fail(MPCQ_ERR_ARG, "mimo plant gradients: shape beyond the kernel's capacity");
    if (lr) return fail(MPCQ_ERR_HIP, std::string("mimo plant-gradient kernel launch failed: ") + hipGetErrorString(err));
    return order_last_after(c, s);
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

int mpcq_mimo_sensitivity_device(mpcq_ctx *c, const double *g, int n_rhs, double *gq, double *gu, int *n_active,
                                 void *stream)
{
    int rc = mimo_sens_check(c, "mpcq_mimo_sensitivity_device", !g, n_rhs, gq || gu || n_active, (hipStream_t)stream);
    if (rc) return rc;
    return mimo_sens_enqueue(c, g, n_rhs, gq, gu, nullptr, nullptr, nullptr, n_active, (hipStream_t)stream);
}

int mpcq_mimo_sensitivity(mpcq_ctx *c, const double *g, int n_rhs, double *gq, double *gu, int *n_active)
{
    int rc = mimo_sens_check(c, "mpcq_mimo_sensitivity", !g, n_rhs, gq || gu || n_active, c ? c->last : nullptr);
    if (rc) return rc;
    const size_t B = c->dims.batch, n = c->dims.n, m = c->dims.m, R = (size_t)n_rhs;
    // staging of this call alone: g and gq (B R n each), gu (B R m), then B ints
    DevBuf<double> d;
    if ((rc = d.alloc(8 * (B * R * (2 * n + m) + (B + 1) / 2), "mimo sensitivity staging"))) return rc;
    struct Drain {  // (the stream is waited for, whatever the outcome, before the staging goes away)
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{c->last};
    double *dg = d, *dgq = dg + B * R * n, *dgu = dgq + B * R * n;
    int *dna = (int *)(dgu + B * R * m);
    if (g && (rc = h2d(dg, g, 8 * B * R * n, c->last))) return rc;
    if ((rc = mimo_sens_enqueue(c, g ? dg : nullptr, n_rhs, dgq, dgu, nullptr, nullptr, nullptr, dna, c->last))) return rc;
    if ((rc = d2h(c, gq, dgq, 8 * B * R * n)) || (rc = d2h(c, gu, dgu, 8 * B * R * m))) return rc;
    return d2h(c, n_active, dna, 4 * B);
}

int mpcq_mimo_step_vjp_device(mpcq_ctx *c, const double *g, int n_rhs, double *dX, double *dU, double *dyref,
                              int *n_active, void *stream)
{
    int rc = mimo_sens_check(c, "mpcq_mimo_step_vjp_device", !g, n_rhs, dX || dU || dyref || n_active,
                             (hipStream_t)stream);
    if (rc) return rc;
    return mimo_sens_enqueue(c, g, n_rhs, nullptr, nullptr, dX, dU, dyref, n_active, (hipStream_t)stream);
}

int mpcq_mimo_step_gains_device(mpcq_ctx *c, double *dX, double *dU, double *dyref, int *n_active, void *stream)
{
    int rc = mimo_sens_check(c, "mpcq_mimo_step_gains_device", true, c ? std::max(c->mimo_nu, 1) : 1,
                             dX || dU || dyref || n_active, (hipStream_t)stream);
    if (rc) return rc;
    return mimo_sens_enqueue(c, nullptr, c->mimo_nu, nullptr, nullptr, dX, dU, dyref, n_active, (hipStream_t)stream);
}

int mpcq_mimo_step_ref_vjp_device(mpcq_ctx *c, const double *g, int n_rhs, double *dX, double *dU, double *dref,
                                  int *n_active, void *stream)
{
    int rc = mimo_sens_check(c, "mpcq_mimo_step_ref_vjp_device", !g, n_rhs, dX || dU || dref || n_active,
                             (hipStream_t)stream);
    if (rc) return rc;
    return mimo_sens_enqueue(c, g, n_rhs, nullptr, nullptr, dX, dU, nullptr, n_active, (hipStream_t)stream, dref);
}

int mpcq_mimo_step_ref_gains_device(mpcq_ctx *c, double *dX, double *dU, double *dref, int *n_active, void *stream)
{
    int rc = mimo_sens_check(c, "mpcq_mimo_step_ref_gains_device", true, c ? std::max(c->mimo_nu, 1) : 1,
                             dX || dU || dref || n_active, (hipStream_t)stream);
    if (rc) return rc;
    return mimo_sens_enqueue(c, nullptr, c->mimo_nu, nullptr, nullptr, dX, dU, nullptr, n_active, (hipStream_t)stream, dref);
}

int mpcq_mimo_step_ref_gains(mpcq_ctx *c, double *dX, double *dU, double *dref, int *n_active)
{
    int rc = mimo_sens_check(c, "mpcq_mimo_step_ref_gains", true, c ? std::max(c->mimo_nu, 1) : 1,
                             dX || dU || dref || n_active, c ? c->last : nullptr);
    if (rc) return rc;
    const size_t B = c->dims.batch, nx = c->mimo_nx, R = c->mimo_nu, nr = (size_t)c->mimo_N * c->mimo_ny;
    // staging of this call alone: dX, dU, dref of the n_u right-hand sides, then B ints
    DevBuf<double> d;
    if ((rc = d.alloc(8 * (B * R * (nx + R + nr) + (B + 1) / 2), "mimo step-gain staging"))) return rc;
    struct Drain {  // (the stream is waited for, whatever the outcome, before the staging goes away)
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{c->last};
    double *ddX = d, *ddU = ddX + B * R * nx, *ddr = ddU + B * R * R;
    int *dna = (int *)(ddr + B * R * nr);
    if ((rc = mimo_sens_enqueue(c, nullptr, (int)R, nullptr, nullptr, ddX, ddU, nullptr, dna, c->last, ddr))) return rc;
    if ((rc = d2h(c, dX, ddX, 8 * B * R * nx)) || (rc = d2h(c, dU, ddU, 8 * B * R * R)) ||
        (rc = d2h(c, dref, ddr, 8 * B * R * nr)))
        return rc;
    return d2h(c, n_active, dna, 4 * B);
}

int mpcq_mimo_plant_vjp_device(mpcq_ctx *c, const double *g, const double *Ad, const double *Bd, const double *Cd,
                               const double *Q, const double *R, const double *RD, const double *K, const double *K0,
                               const double *w0, const double *X, const double *U_prev, const double *yref, double *gAd,
                               double *gBd, double *gCd, double *gQ, double *gR, double *gRD, double *gK, double *gK0,
                               double *gw0, int *n_active, void *stream)
{
    const MimoPlantPtrs p{{Ad, Bd, Cd, Q, R, RD, K, K0, w0}, {gAd, gBd, gCd, gQ, gR, gRD, gK, gK0, gw0}};
    int rc = mimo_plant_vjp_check(c, "mpcq_mimo_plant_vjp_device", p, X, U_prev, n_active, (hipStream_t)stream);
    if (rc) return rc;
    return mimo_plant_vjp_enqueue(c, g, p, X, U_prev, yref, n_active, (hipStream_t)stream);
}

int mpcq_mimo_plant_vjp(mpcq_ctx *c, const double *g, const double *Ad, const double *Bd, const double *Cd,
                        const double *Q, const double *R, const double *RD, const double *K, const double *K0,
                        const double *w0, const double *X, const double *U_prev, const double *yref, double *gAd,
                        double *gBd, double *gCd, double *gQ, double *gR, double *gRD, double *gK, double *gK0, double *gw0,
                        int *n_active)
{
    const MimoPlantPtrs h{{Ad, Bd, Cd, Q, R, RD, K, K0, w0}, {gAd, gBd, gCd, gQ, gR, gRD, gK, gK0, gw0}};
    int rc = mimo_plant_vjp_check(c, "mpcq_mimo_plant_vjp", h, X, U_prev, n_active, c ? c->last : nullptr);
    if (rc) return rc;
    const size_t B = c->dims.batch, n = c->dims.n, nx = c->mimo_nx, nu = c->mimo_nu, ny = c->mimo_ny;
    size_t sz[9], per = 0;
    mimo_plant_sizes(c, sz);
    for (size_t k : sz) per += k;
    // staging of this call alone: g (B n), the plant arrays and their gradients (B per each), X, U_prev, yref, B ints
    DevBuf<double> d;
    if ((rc = d.alloc(8 * (B * (n + 2 * per + nx + nu) + ny + (B + 1) / 2), "mimo plant-gradient staging"))) return rc;
    struct Drain {  // (the stream is waited for, whatever the outcome, before the staging goes away)
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{c->last};
    double *o = d, *dg = o;
    o += B * n;
    MimoPlantPtrs p{};
    for (int k = 0; k < 9; k++) {
        if ((rc = h2d(o, h.in[k], 8 * B * sz[k], c->last))) return rc;
        p.in[k] = o;
        o += B * sz[k];
    }
    for (int k = 0; k < 9; k++) {
        p.out[k] = h.out[k] ? o : nullptr;
        o += B * sz[k];
    }
    double *dX = o, *dU = dX + B * nx, *dy = dU + B * nu;
    int *dna = (int *)(dy + ny);
    if ((g && (rc = h2d(dg, g, 8 * B * n, c->last))) || (rc = h2d(dX, X, 8 * B * nx, c->last)) ||
        (rc = h2d(dU, U_prev, 8 * B * nu, c->last)) || (yref && (rc = h2d(dy, yref, 8 * ny, c->last))))
        return rc;
    if ((rc = mimo_plant_vjp_enqueue(c, g ? dg : nullptr, p, dX, dU, yref ? dy : nullptr, dna, c->last))) return rc;
    for (int k = 0; k < 9; k++)
        if ((rc = d2h(c, h.out[k], p.out[k], 8 * B * sz[k]))) return rc;
    return d2h(c, n_active, dna, 4 * B);
}

}  // extern "C"

// solvempc_amd/csrc/mpcq_host_mimo.cpp — host side of the C ABI declared in include/mpcq.h: every mpcq_mimo_*
// entry point.  The MIMO setup and step, its polish and horizon-reference forms, the sensitivities and plant
// gradients of the last step, the simulated plant and the closed-loop runs.
#include "mpcq_ctx.h"

namespace {

// The reference of one MIMO step: yref (n_y values for the whole batch, held over the horizon; NULL: 0) of
// mpcq_mimo_step_device, or with `horizon` a horizon of N*n_y values per QP, `stride` doubles apart (0: one for the
// batch), of mpcq_mimo_step_ref_device
struct MimoRef {
    const double *yref = nullptr, *ref = nullptr;
    long long stride = 0;
    bool horizon = false;
};

// The refusals of a MIMO step, in the order of include/mpcq.h, before anything is enqueued or written
int mimo_step_check(mpcq_ctx *c, const char *fn, const double *X, const double *U, const MimoRef &r, bool polish,
                    hipStream_t s)
{
    int rc = check_ctx(c, kNone);
    if (rc) return rc;
    if (c->set.polish) return fail(MPCQ_ERR_ARG, polish_refusal(fn));
    if (c->mode != mpcq_ctx::Mode::Mimo) return fail(MPCQ_ERR_ORDER, "mpcq_mimo_setup_plants_device has not succeeded");
    if (!X || !U) return fail(MPCQ_ERR_ARG, "null X/U");
    if (r.horizon) {
        if (!r.ref) return fail(MPCQ_ERR_ARG, std::string(fn) + ": null ref");
        if (r.stride != 0 && r.stride < (long long)c->mimo.N * c->mimo.ny)
            return fail(MPCQ_ERR_ARG, std::string(fn) + ": ref_stride is 0 (one reference for the batch) or >= N*n_y");
    }
    return polish ? refuse_capture(fn, s) : MPCQ_OK;
}

int mimo_step_enqueue(mpcq_ctx *c, const double *X, double *U, const MimoRef &r, void *stream)
{
    int rc = materialize_xy(c);  // (a pending lazy x, y first: the kernel below rewrites the state)
    if (rc) return rc;
    mpcq::MimoArgs a{};
    set_mimo_ops(c, a);
    a.s_rows = c->mimo.srows;
    a.diag_k0 = c->mimo.diag_k0 && !*test_hook("MPCQ_MIMO_GENERAL_K0");
    a.st = to_solver(c->set);
    const int ct = c->set.check_termination;
    a.adaptive_interval = c->set.adaptive_rho_interval ? c->set.adaptive_rho_interval : (ct ? 4 * ct : 100);
    a.X = X; a.U = U; a.yref = r.horizon ? nullptr : r.yref;
    a.q_out = c->d_q; a.u_out = c->d_u;
    a.xs = (double *)c->d_xs; a.zs = (double *)c->d_zs; a.ys = (double *)c->d_ys; a.rhos = (double *)c->d_rhos;
    a.warm = c->set.warm_start;
    a.fresh = c->fresh;
    a.x = c->d_x; a.y = c->d_y; a.status = c->d_status; a.iter = c->d_iter; a.rho_out = c->d_rho;
    const char *stp = debug_hook("MPCQ_MIMO_STAMPS");  // per-QP stage stamps
    if (stp && *stp) {
        if ((rc = c->d_stamps.alloc(8 * 8 * (size_t)a.batch, "stamps"))) return rc;
        a.stamps = c->d_stamps;
    }
    hipStream_t s = (hipStream_t)stream;
    const int lr = r.horizon ? mpcq_internal_mimo_solve_ref_launch(&a, r.ref, r.stride, s)
                             : mpcq_internal_mimo_solve_launch(&a, s);
    if (lr) return fail(lr == -1 ? MPCQ_ERR_ARG : MPCQ_ERR_HIP, "mimo solve launch failed");
    if (stp && *stp && (rc = dump_stamps(stp, c->d_stamps, 8 * (size_t)a.batch, s))) return rc;
    c->last = s;
    c->fresh = false;
    c->mimo.stepped = true;
    c->mimo.ref_step = r.horizon;
    c->pol_valid = false;
    return MPCQ_OK;
}

// The step, then OSQP's polish of every SOLVED QP on the same stream (mpcq_mimo_polish.hip)
int mimo_step_polish_enqueue(mpcq_ctx *c, const double *X, double *U, const MimoRef &r, void *stream)
{
    int rc = MPCQ_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t B = c->dims.batch, nu = c->mimo.nu;
    if ((rc = c->d_pol_status.alloc(4 * B)) || (rc = c->d_pol_nact.alloc(4 * B)) || (rc = c->d_pol_res.alloc(8 * 2 * B)) ||
        (rc = c->mimo.Uprev.grow(8 * B * nu, s, "mimo polish staging")))
        return rc;
    HIPCHK(hipMemcpyAsync(c->mimo.Uprev, U, 8 * B * nu, hipMemcpyDeviceToDevice, s));
    if ((rc = mimo_step_enqueue(c, X, U, r, stream))) return rc;
    mpcq::MimoPolishArgs a{};
    set_mimo_ops(c, a);
    a.q = c->d_q; a.u = c->d_u;
    a.xs = (double *)c->d_xs; a.zs = (double *)c->d_zs; a.ys = (double *)c->d_ys;
    a.status = c->d_status;
    a.x = c->d_x; a.y = c->d_y;
    a.U_prev = c->mimo.Uprev; a.U = U;
    a.pol_status = c->d_pol_status; a.pol_nact = c->d_pol_nact; a.pol_res = c->d_pol_res;
    a.delta = c->set.delta;
    a.refine = c->set.polish_refine_iter;
    a.scaled_termination = c->set.scaled_termination;
    hipError_t err = hipSuccess;
    const int lr = mpcq_internal_mimo_polish_launch(&a, c->cus, s, &err);
    if (lr == -1) return fail(MPCQ_ERR_ARG, "mimo polish: shape beyond the kernel's capacity");
    if (lr) return fail(MPCQ_ERR_HIP, std::string("mimo polish kernel launch failed: ") + hipGetErrorString(err));
    c->pol_valid = true;
    return MPCQ_OK;
}

// ---- closed-loop MIMO runs: the existing step, launched once per control step, and
// mpcq_mimo_run.hip's plant kernel between two steps
// A MIMO context with a simulated plant (MPCQ_ERR_ORDER otherwise)
int mimo_plant_check(mpcq_ctx *c, const char *fn)
{
    int rc = check_ctx(c, kNone);
    if (rc) return rc;
    if (c->mode != mpcq_ctx::Mode::Mimo) return fail(MPCQ_ERR_ORDER, "mpcq_mimo_setup_plants_device has not succeeded");
    if (!c->mimo.plant)
        return fail(MPCQ_ERR_ORDER, std::string(fn) + ": no simulated plant (mpcq_mimo_set_plant_device) for this setup's n_x, n_u");
    return MPCQ_OK;
}

// One plant update of every QP at absolute control step `step`; with a log, the step's record row and totals
int mimo_plant_enqueue(mpcq_ctx *c, double *X, const double *U, unsigned long long seed, long long first_qp,
                       long long step, double noise_std, const mpcq_mimo_log *log, hipStream_t s)
{
    mpcq::MimoPlantArgs a{};
    a.batch = c->dims.batch;
    a.nx = c->mimo.nx; a.nu = c->mimo.nu;
    a.Ad = c->mimo.Ad; a.Bd = c->mimo.Bd;
    a.X = X; a.U = U;
    a.seed = seed; a.first_qp = first_qp; a.step = step; a.noise_std = noise_std;
    a.status = c->d_status; a.iter = c->d_iter;
    if (log) {
        const size_t B = c->dims.batch, row = (size_t)(step - log->step0) * B;
        a.log_U = log->U ? log->U + row * a.nu : nullptr;
        a.log_X = log->X ? log->X + row * a.nx : nullptr;
        a.log_status = log->status ? log->status + row : nullptr;
        a.log_iter = log->iter ? log->iter + row : nullptr;
        a.iters_total = log->iters_total;
        a.unsolved_total = log->unsolved_total;
    }
    const int lr = mpcq_internal_mimo_plant_launch(&a, s);
    if (lr) return fail(lr == -1 ? MPCQ_ERR_ARG : MPCQ_ERR_HIP, "mimo plant kernel launch failed");
    return MPCQ_OK;
}

// The refusals of a run, before anything is enqueued or written (include/mpcq.h)
int mimo_run_check(mpcq_ctx *c, const char *fn, const double *X, const double *U, int steps, long long first_step,
                   int polish, const mpcq_mimo_log *log, hipStream_t s)
{
    int rc = check_ctx(c, kNone);
    if (rc) return rc;
    if (c->set.polish) return fail(MPCQ_ERR_ARG, polish_refusal(fn));
    if ((rc = mimo_plant_check(c, fn))) return rc;
    if (!X || !U) return fail(MPCQ_ERR_ARG, std::string(fn) + ": null X/U");
    if (steps < 0 || first_step < 0) return fail(MPCQ_ERR_ARG, std::string(fn) + ": steps >= 0, first_step >= 0");
    if (polish != 0 && polish != 1) return fail(MPCQ_ERR_ARG, std::string(fn) + ": polish is 0 or 1");
    if (log && (log->U || log->X || log->status || log->iter)) {
        if (log->rows < 1 || log->step0 < 0) return fail(MPCQ_ERR_ARG, std::string(fn) + ": log with rows < 1 or step0 < 0");
        if (steps > 0 && (first_step < log->step0 || first_step + steps - 1 - log->step0 >= log->rows))
            return fail(MPCQ_ERR_ARG, std::string(fn) + ": a control step of the call falls outside the log's rows");
    }
    return refuse_capture(fn, s);
}

// `steps` rounds of [control step; plant update].  sched == NULL: every step is mpcq_mimo_step(_polish)_device(yref);
// otherwise step s is mpcq_mimo_step_ref_device on the window of the schedule that starts at block s, last block held:
// the schedule itself while s + N <= sched_len, else the padded tail (2N-1 blocks per schedule row from block
// base = max(sched_len - N, 0), mimo_sched_tail_kernel, built once here) at block min(s - base, N-1).
int mimo_run_enqueue(mpcq_ctx *c, double *X, double *U, const double *yref, const double *sched, long long sched_len,
                     long long sched_stride, int steps, unsigned long long seed, long long first_qp,
                     long long first_step, double noise_std, int polish, const mpcq_mimo_log *log, hipStream_t s)
{
    if (steps == 0) return MPCQ_OK;
    int rc = MPCQ_OK;
    const size_t B = c->dims.batch;
    const long long N = c->mimo.N, ny = c->mimo.ny, blocks = 2 * N - 1, base = std::max(sched_len - N, 0ll);
    const double *tail = nullptr;
    if (sched && first_step + steps - 1 + N > sched_len) {
        mpcq::MimoTailArgs t{};
        t.rows = sched_stride ? (long long)B : 1;
        t.stride = sched_stride;
        t.len = sched_len; t.base = base;
        t.blocks = (int)blocks; t.ny = (int)ny;
        t.sched = sched;
        if ((rc = c->mimo.tail.grow(8 * (size_t)(t.rows * blocks * ny), s, "mimo schedule tail"))) return rc;
        tail = t.tail = c->mimo.tail;
        const int lr = mpcq_internal_mimo_sched_tail_launch(&t, s);
        if (lr) return fail(lr == -1 ? MPCQ_ERR_ARG : MPCQ_ERR_HIP, "mimo schedule tail kernel launch failed");
    }
    if (log && log->iters_total) HIPCHK(hipMemsetAsync(log->iters_total, 0, 4 * B, s));
    if (log && log->unsolved_total) HIPCHK(hipMemsetAsync(log->unsolved_total, 0, 4 * B, s));
    for (int k = 0; k < steps; k++) {
        const long long step = first_step + k;
        MimoRef r;
        if (!sched) {
            r.yref = yref;
        } else if (step + N <= sched_len) {
            r.ref = sched + step * ny; r.stride = sched_stride; r.horizon = true;
        } else {
            r.ref = tail + std::min(step - base, N - 1) * ny;
            r.stride = sched_stride ? blocks * ny : 0;
            r.horizon = true;
        }
        if ((rc = polish ? mimo_step_polish_enqueue(c, X, U, r, s) : mimo_step_enqueue(c, X, U, r, s))) return rc;
        if ((rc = mimo_plant_enqueue(c, X, U, seed, first_qp, step, noise_std, log, s))) return rc;
    }
    return MPCQ_OK;
}

// ---- active-set sensitivities of the last MIMO step (mpcq_mimo_sens.hip; include/mpcq.h)
// The refusals of include/mpcq.h for the MIMO sensitivity calls, before anything is enqueued or written
int mimo_sens_check(mpcq_ctx *c, const char *fn, bool implicit_g, int n_rhs, bool any_out, hipStream_t s)
{
    int rc = check_ctx(c, kNone);
    if (rc) return rc;
    if (c->mode != mpcq_ctx::Mode::Mimo)
        return fail(MPCQ_ERR_ORDER, std::string(fn) + ": mpcq_mimo_setup_plants_device has not succeeded");
    if (!c->mimo.stepped)
        return fail(MPCQ_ERR_ORDER, std::string(fn) + ": needs a mpcq_mimo_step_device since the last setup");
    if (n_rhs < 1 || n_rhs > 4) return fail(MPCQ_ERR_ARG, std::string(fn) + ": 1 <= n_rhs <= 4");
    if (implicit_g && n_rhs > c->mimo.nu)
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
    set_mimo_ops(c, a);
    a.s_rows = c->mimo.srows;
    a.n_rhs = n_rhs;
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
    const size_t nx = c->mimo.nx, nu = c->mimo.nu, ny = c->mimo.ny;
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
    if (!c->mimo.stepped)
        return fail(MPCQ_ERR_ORDER, std::string(fn) + ": needs a mpcq_mimo_step_device since the last setup");
    if (c->mimo.ref_step)  // (gFr would be formed from a yref the step did not use)
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
    if (int rc = c->mimo.pv.alloc(8 * (B * (n + m) + (B + 1) / 2), "mimo plant-gradient staging")) return rc;
    double *gq = c->mimo.pv, *gu = gq + B * n;
    int *nact = (int *)(gu + B * m);
    if (int rc = mimo_sens_enqueue(c, g, 1, gq, gu, nullptr, nullptr, nullptr, nact, s)) return rc;
    mpcq::MimoPlantVjpArgs a{};
    set_mimo_ops(c, a);
    a.s_rows = c->mimo.srows;
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

int mpcq_mimo_setup_plants_device(mpcq_ctx *c, int nx, int nu, int ny, int s_rows, const double *Ad, const double *Bd,
                                  const double *Cd, const double *Q, const double *R, const double *RD, const double *K,
                                  const double *K0, const double *w0, void *stream)
{
    int rc = check_ctx(c, kNone);
    if (rc) return rc;
    if (c->set.polish) return fail(MPCQ_ERR_ARG, polish_refusal("mpcq_mimo_setup_plants_device"));
    if ((rc = materialize_xy(c))) return rc;  // (the operator blocks below replace the tile images' role)
    const int n = c->dims.n, m = c->dims.m;
    if (nu != 1 && nu != 2 && nu != 4) return fail(MPCQ_ERR_ARG, "mimo: n_u must be 1, 2 or 4");
    if (nx <= 0 || nx > 12 || ny <= 0 || ny > 12 || s_rows < 0) return fail(MPCQ_ERR_ARG, "mimo: 1 <= n_x, n_y <= 12");
    if (n % nu || n / nu > 32 || n > 128 || m != 2 * n) return fail(MPCQ_ERR_ARG, "mimo: n = N n_u <= 128 (N <= 32), m = 2n");
    if (c->dims.n_plants != c->dims.batch || c->dims.dtype == MPCQ_F32)
        return fail(MPCQ_ERR_ARG, "mimo: one plant per QP (n_plants == batch), dtype MPCQ_F64 or MPCQ_F64_MIXED");
    if (!Ad || !Bd || !Cd || !Q || !R || !RD || !K || !K0 || !w0) return fail(MPCQ_ERR_ARG, "mimo: null plant array");
    const int N = n / nu;
    const mpcq::MimoLayout L = mpcq::MimoLayout::make(N, nx, nu, ny);
    c->mimo.invalidate(N, nx, nu, ny);
    if ((rc = c->mimo.ops.alloc(8 * (size_t)L.total * c->dims.n_plants, "mimo operator blocks"))) return rc;
    c->mimo.N = N; c->mimo.nx = nx; c->mimo.nu = nu; c->mimo.ny = ny; c->mimo.srows = s_rows;
    c->mode = mpcq_ctx::Mode::None;
    c->sens_ok = false;
    c->pol_valid = false;
    c->gen++;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(c->d_flags, 0, 4, s));
    mpcq::MimoSetupArgs a{};
    a.n_plants = c->dims.n_plants;
    a.N = N; a.nx = nx; a.nu = nu; a.ny = ny; a.s_rows = s_rows;
    a.scaling = c->set.scaling;
    a.sigma = c->set.sigma;
    a.Ad = Ad; a.Bd = Bd; a.Cd = Cd; a.Q = Q; a.R = R; a.RD = RD; a.K = K; a.K0 = K0; a.w0 = w0;
    a.ops = c->mimo.ops;
    a.flags = c->d_flags;
    const char *sst = debug_hook("MPCQ_MIMO_SETUP_STAMPS");  // per-plant phase stamps
    if (sst && *sst) {
        c->d_stamps.release();
        if ((rc = c->d_stamps.alloc(8 * 16 * (size_t)a.n_plants, "stamps"))) return rc;
        a.stamps = c->d_stamps;
    }
    const int lr = mpcq_internal_mimo_setup_launch(&a, s);
    if (lr == -1) return fail(MPCQ_ERR_ARG, "mimo: shape beyond the setup kernel's LDS capacity");
    if (lr) return fail(MPCQ_ERR_HIP, std::string("mimo setup launch failed: ") + hipGetErrorString(hipGetLastError()));
    int flags = 0;
    HIPCHK(hipMemcpyAsync(&flags, c->d_flags, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (sst && *sst) {
        rc = dump_stamps(sst, c->d_stamps, 16 * (size_t)a.n_plants, s);
        c->d_stamps.release();
        if (rc) return rc;
    }
    if (flags & 1) return fail(MPCQ_ERR_SETUP, "mimo: P + sigma I is not positive definite (non-convex QP)");
    if (flags & 2) return fail(MPCQ_ERR_SETUP, "mimo: a constraint row is not an inequality (|w0| beyond OSQP_INFTY)");
    c->mimo.diag_k0 = (flags & 4) ? 0 : 1;
    c->last = s;
    c->fresh = true;  // the first step starts from x = z = y = 0, rho = settings.rho (initSolver, :64)
    c->mpc_ready = false;  // the generic front-end operators no longer describe this context
    c->mode = mpcq_ctx::Mode::Mimo;
    return MPCQ_OK;
}

int mpcq_mimo_step_device(mpcq_ctx *c, const double *X, double *U, const double *yref, void *stream)
{
    MimoRef r;
    r.yref = yref;
    int rc = mimo_step_check(c, "mpcq_mimo_step_device", X, U, r, false, (hipStream_t)stream);
    if (rc) return rc;
    return mimo_step_enqueue(c, X, U, r, stream);
}

int mpcq_mimo_step_polish_device(mpcq_ctx *c, const double *X, double *U, const double *yref, void *stream)
{
    MimoRef r;
    r.yref = yref;
    int rc = mimo_step_check(c, "mpcq_mimo_step_polish_device", X, U, r, true, (hipStream_t)stream);
    if (rc) return rc;
    return mimo_step_polish_enqueue(c, X, U, r, stream);
}

int mpcq_mimo_step_ref_device(mpcq_ctx *c, const double *X, double *U, const double *ref, long long ref_stride,
                              int polish, void *stream)
{
    const char *fn = "mpcq_mimo_step_ref_device";
    if (polish != 0 && polish != 1) return fail(MPCQ_ERR_ARG, std::string(fn) + ": polish is 0 or 1");
    MimoRef r;
    r.ref = ref; r.stride = ref_stride; r.horizon = true;
    int rc = mimo_step_check(c, fn, X, U, r, polish == 1, (hipStream_t)stream);
    if (rc) return rc;
    return polish ? mimo_step_polish_enqueue(c, X, U, r, stream) : mimo_step_enqueue(c, X, U, r, stream);
}

int mpcq_mimo_step_ref(mpcq_ctx *c, const double *X, double *U, const double *ref, long long ref_stride, int polish)
{
    const char *fn = "mpcq_mimo_step_ref";
    if (polish != 0 && polish != 1) return fail(MPCQ_ERR_ARG, std::string(fn) + ": polish is 0 or 1");
    MimoRef r;
    r.ref = ref; r.stride = ref_stride; r.horizon = true;
    int rc = mimo_step_check(c, fn, X, U, r, polish == 1, c ? c->last : nullptr);
    if (rc) return rc;
    const size_t B = c->dims.batch, nx = c->mimo.nx, nu = c->mimo.nu, nr = (size_t)c->mimo.N * c->mimo.ny;
    const size_t rows = ref_stride ? B : 1;
    // staging of this call alone: X, U, then the references packed (B rows of N*n_y, or the one shared row)
    Staging d(c->last);
    if ((rc = d.alloc(B * (nx + nu) + rows * nr, "mimo reference staging"))) return rc;
    double *dX = d.take(B * nx), *dU = d.take(B * nu), *dr = d.take(rows * nr);
    if ((rc = h2d(dX, X, 8 * B * nx, c->last)) || (rc = h2d(dU, U, 8 * B * nu, c->last))) return rc;
    if (rows == 1 || ref_stride == (long long)nr) {
        if ((rc = h2d(dr, ref, 8 * rows * nr, c->last))) return rc;
    } else {
        HIPCHK(hipMemcpy2DAsync(dr, 8 * nr, ref, 8 * (size_t)ref_stride, 8 * nr, rows, hipMemcpyHostToDevice, c->last));
        HIPCHK(hipStreamSynchronize(c->last));
    }
    r.ref = dr;
    r.stride = ref_stride ? (long long)nr : 0;
    if ((rc = polish ? mimo_step_polish_enqueue(c, dX, dU, r, c->last) : mimo_step_enqueue(c, dX, dU, r, c->last)))
        return rc;
    return d2h(c, U, dU, 8 * B * nu);
}

int mpcq_mimo_set_plant_device(mpcq_ctx *c, const double *Ad, const double *Bd, void *stream)
{
    const char *fn = "mpcq_mimo_set_plant_device";
    int rc = check_ctx(c, kNone);
    if (rc) return rc;
    if (c->mode != mpcq_ctx::Mode::Mimo) return fail(MPCQ_ERR_ORDER, "mpcq_mimo_setup_plants_device has not succeeded");
    if (!Ad || !Bd) return fail(MPCQ_ERR_ARG, std::string(fn) + ": null Ad/Bd");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = refuse_capture(fn, s))) return rc;
    const size_t B = c->dims.batch, nx = c->mimo.nx, nu = c->mimo.nu;
    // (both buffers are released whenever a MIMO setup changes n_x or n_u, so an allocated one has this size)
    if ((rc = c->mimo.Ad.alloc(8 * B * nx * nx, "mimo simulated plant")) ||
        (rc = c->mimo.Bd.alloc(8 * B * nx * nu, "mimo simulated plant")))
        return rc;
    HIPCHK(hipMemcpyAsync(c->mimo.Ad, Ad, 8 * B * nx * nx, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(c->mimo.Bd, Bd, 8 * B * nx * nu, hipMemcpyDeviceToDevice, s));
    c->mimo.plant = true;
    return MPCQ_OK;
}

int mpcq_mimo_simulate_device(mpcq_ctx *c, double *X, const double *U, unsigned long long seed, long long first_qp,
                              long long step, double noise_std, void *stream)
{
    const char *fn = "mpcq_mimo_simulate_device";
    int rc = mimo_plant_check(c, fn);
    if (rc) return rc;
    if (!X || !U) return fail(MPCQ_ERR_ARG, std::string(fn) + ": null X/U");
    if (step < 0) return fail(MPCQ_ERR_ARG, std::string(fn) + ": step >= 0");
    return mimo_plant_enqueue(c, X, U, seed, first_qp, step, noise_std, nullptr, (hipStream_t)stream);
}

int mpcq_mimo_run_device(mpcq_ctx *c, double *X, double *U, const double *yref, int steps, unsigned long long seed,
                         long long first_qp, long long first_step, double noise_std, int polish,
                         const mpcq_mimo_log *log, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    int rc = mimo_run_check(c, "mpcq_mimo_run_device", X, U, steps, first_step, polish, log, s);
    if (rc) return rc;
    return mimo_run_enqueue(c, X, U, yref, nullptr, 0, 0, steps, seed, first_qp, first_step, noise_std, polish, log, s);
}

int mpcq_mimo_run_ref_device(mpcq_ctx *c, double *X, double *U, const double *sched, int sched_len,
                             long long sched_stride, int steps, unsigned long long seed, long long first_qp,
                             long long first_step, double noise_std, int polish, const mpcq_mimo_log *log, void *stream)
{
    const char *fn = "mpcq_mimo_run_ref_device";
    hipStream_t s = (hipStream_t)stream;
    int rc = mimo_run_check(c, fn, X, U, steps, first_step, polish, log, s);
    if (rc) return rc;
    if (!sched || sched_len < 1) return fail(MPCQ_ERR_ARG, std::string(fn) + ": null schedule or sched_len < 1");
    if (sched_stride != 0 && sched_stride < (long long)sched_len * c->mimo.ny)
        return fail(MPCQ_ERR_ARG, std::string(fn) + ": sched_stride is 0 (one schedule for the batch) or >= sched_len*n_y");
    return mimo_run_enqueue(c, X, U, nullptr, sched, sched_len, sched_stride, steps, seed, first_qp, first_step,
                            noise_std, polish, log, s);
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
    Staging d(c->last);
    if ((rc = d.alloc(B * R * (2 * n + m) + (B + 1) / 2, "mimo sensitivity staging"))) return rc;
    double *dg = d.take(B * R * n), *dgq = d.take(B * R * n), *dgu = d.take(B * R * m);
    int *dna = d.take<int>((B + 1) / 2);
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
    int rc = mimo_sens_check(c, "mpcq_mimo_step_gains_device", true, c ? std::max(c->mimo.nu, 1) : 1,
                             dX || dU || dyref || n_active, (hipStream_t)stream);
    if (rc) return rc;
    return mimo_sens_enqueue(c, nullptr, c->mimo.nu, nullptr, nullptr, dX, dU, dyref, n_active, (hipStream_t)stream);
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
    int rc = mimo_sens_check(c, "mpcq_mimo_step_ref_gains_device", true, c ? std::max(c->mimo.nu, 1) : 1,
                             dX || dU || dref || n_active, (hipStream_t)stream);
    if (rc) return rc;
    return mimo_sens_enqueue(c, nullptr, c->mimo.nu, nullptr, nullptr, dX, dU, nullptr, n_active, (hipStream_t)stream, dref);
}

int mpcq_mimo_step_ref_gains(mpcq_ctx *c, double *dX, double *dU, double *dref, int *n_active)
{
    int rc = mimo_sens_check(c, "mpcq_mimo_step_ref_gains", true, c ? std::max(c->mimo.nu, 1) : 1,
                             dX || dU || dref || n_active, c ? c->last : nullptr);
    if (rc) return rc;
    const size_t B = c->dims.batch, nx = c->mimo.nx, R = c->mimo.nu, nr = (size_t)c->mimo.N * c->mimo.ny;
    // staging of this call alone: dX, dU, dref of the n_u right-hand sides, then B ints
    Staging d(c->last);
    if ((rc = d.alloc(B * R * (nx + R + nr) + (B + 1) / 2, "mimo step-gain staging"))) return rc;
    double *ddX = d.take(B * R * nx), *ddU = d.take(B * R * R), *ddr = d.take(B * R * nr);
    int *dna = d.take<int>((B + 1) / 2);
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
    const size_t B = c->dims.batch, n = c->dims.n, nx = c->mimo.nx, nu = c->mimo.nu, ny = c->mimo.ny;
    size_t sz[9], per = 0;
    mimo_plant_sizes(c, sz);
    for (size_t k : sz) per += k;
    // staging of this call alone: g (B n), the plant arrays and their gradients (B per each), X, U_prev, yref, B ints
    Staging d(c->last);
    if ((rc = d.alloc(B * (n + 2 * per + nx + nu) + ny + (B + 1) / 2, "mimo plant-gradient staging"))) return rc;
    double *dg = d.take(B * n);
    MimoPlantPtrs p{};
    for (int k = 0; k < 9; k++) {
        double *in = d.take(B * sz[k]);
        if ((rc = h2d(in, h.in[k], 8 * B * sz[k], c->last))) return rc;
        p.in[k] = in;
    }
    for (int k = 0; k < 9; k++) {
        double *out = d.take(B * sz[k]);
        p.out[k] = h.out[k] ? out : nullptr;
    }
    double *dX = d.take(B * nx), *dU = d.take(B * nu), *dy = d.take(ny);
    int *dna = d.take<int>((B + 1) / 2);
    if ((g && (rc = h2d(dg, g, 8 * B * n, c->last))) || (rc = h2d(dX, X, 8 * B * nx, c->last)) ||
        (rc = h2d(dU, U_prev, 8 * B * nu, c->last)) || (yref && (rc = h2d(dy, yref, 8 * ny, c->last))))
        return rc;
    if ((rc = mimo_plant_vjp_enqueue(c, g ? dg : nullptr, p, dX, dU, yref ? dy : nullptr, dna, c->last))) return rc;
    for (int k = 0; k < 9; k++)
        if ((rc = d2h(c, h.out[k], p.out[k], 8 * B * sz[k]))) return rc;
    return d2h(c, n_active, dna, 4 * B);
}

}  // extern "C"

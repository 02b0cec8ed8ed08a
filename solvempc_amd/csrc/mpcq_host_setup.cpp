// solvempc_amd/csrc/mpcq_host_setup.cpp — host side of the C ABI declared in include/mpcq.h: mpcq_setup, the
// data and matrix updates, warm / cold start, and the hardest-first order map.
#include "mpcq_ctx.h"

namespace {

size_t setup_scratch_len(int n, int m)
{
    return 7 * (size_t)n * n + (size_t)m * n + 3 * (size_t)n + 2 * (size_t)m + 64;
}

// True when every scaled lower bound is below -OSQP_INFTY*MIN_SCALING (the reference's
// l = -DBL_MAX, :42), which selects the kernel variant without the lower clamp.  Exact for a
// shared plant (its E is on the host); conservative (|l| >= 1e300) for per-plant contexts.
bool lower_all_free(const mpcq_ctx *c, const double *l)
{
    const size_t B = (l == nullptr) ? 0 : (size_t)c->dims.m;
    const size_t rows = c->dims.n_plants == 1 ? B : 0;
    if (c->dims.n_plants == 1) {
        for (size_t j = 0; j < rows; j++)
            if (!(l[j] * c->hE[j] < -mpcq::kInfty * mpcq::kMinScaling)) return false;
        return true;
    }
    return false;
}

bool lower_all_free_batch(const mpcq_ctx *c, const double *l)
{
    const size_t total = (size_t)c->dims.batch * c->dims.m;
    for (size_t i = 0; i < total; i++) {
        const double e = c->dims.n_plants == 1 ? c->hE[i % c->dims.m] : 1e-250;
        if (!(l[i] * e < -mpcq::kInfty * mpcq::kMinScaling) && !(l[i] <= -1e300)) return false;
    }
    return true;
}

// Lower bounds kappa on ||P^ dx|| / ||dx|| in the two norms OSQP's is_dual_infeasible compares
// (AdmmArgs::dinf_kappa), for a shared plant in the eigen-basis with every row an inequality: then
// P~ = P^ + sigma I and W' P~ W = I, so lambda_min(P~) = 1 / ||W||_2^2 >= 1 / ||W||_F^2 and
// mu = 1 / ||W||_F^2 - sigma <= lambda_min(P^).  With v = dx (scaled space):
//   ||P^ v||_inf >= mu ||v||_2 / sqrt(n) >= (mu / sqrt(n)) ||v||_inf                     (scaled_termination)
//   ||D^-1 P^ v||_inf >= (min_i D_i^-1) (mu / sqrt(n)) ||v||_inf
//                     >= (min_i D_i^-1) mu / (sqrt(n) max_i D_i) ||D v||_inf              (unscaled)
void dinf_bounds(mpcq_ctx *c, const double *blk, const mpcq::OpsLayout &L)
{
    c->dinf_ks = c->dinf_ku = 0.0;
    const size_t n = c->dims.n;
    if (c->dims.n_plants != 1 || c->inv_ops || !c->all_ineq || n == 0) return;
    double fro = 0.0, dmax = 0.0, dinv_min = HUGE_VAL;
    for (size_t i = 0; i < (size_t)c->nc * c->nc; i++) fro += blk[L.W + i] * blk[L.W + i];
    for (size_t i = 0; i < n; i++) {
        dmax = std::max(dmax, blk[L.D + i]);
        dinv_min = std::min(dinv_min, 1.0 / blk[L.D + i]);
    }
    const double mu = 1.0 / fro - c->set.sigma;
    if (!(fro > 0.0) || !(mu > 0.0) || !(dmax > 0.0)) return;
    c->dinf_ks = mu / std::sqrt((double)n);
    c->dinf_ku = dinv_min * mu / (std::sqrt((double)n) * dmax);
}

// setup_on_device: setup kernels on the device-resident setup data (d_P, d_q0, d_A, d_l0, d_u0), operator
// conversion / tile images, the plant-0 scaling readback (run_setup), then the per-QP broadcast of q0/u0/l0 and
// the state reset.  One 4-byte flag word (non-convex plant, non-inequality row) comes back to the host.
// run_setup's options: keep_scaling: the keep-scaling kernels (mpcq_update_P_A_device,
// rescale = 0), which rebuild the factor stage alone and leave D, E, c, the rho scales and the constraint types as
// the operator blocks hold them.  check_lower / check_paired: the device-side checks of mpcq_update_P_A_device,
// enqueued behind the setup kernel so that the one flag word carries their answers too (*flags_out).
struct SetupRun {
    bool keep_scaling = false, check_lower = false, check_paired = false;
};

int run_setup(mpcq_ctx *c, hipStream_t s, const SetupRun &run = SetupRun{}, int *flags_out = nullptr)
{
    c->gen++;
    const size_t Pn = c->dims.n_plants, n = c->dims.n, m = c->dims.m;
    if (!run.keep_scaling) HIPCHK(hipMemsetAsync(c->d_ops, 0, 8 * Pn * c->ops_stride, s));
    HIPCHK(hipMemsetAsync(c->d_flags, 0, 4, s));
    mpcq::SetupArgs a{};
    a.n = (int)n;
    a.m = (int)m;
    a.nc = c->nc;
    a.mc = c->mc;
    a.n_plants = (int)Pn;
    a.scaling = c->set.scaling;
    a.sigma = c->set.sigma;
    a.rho = c->set.rho;
    // an fp32 solve reads W to ~1e-7: a basis orthogonal to ~1e-10 saves the last Jacobi sweep
    a.jacobi_tol = c->dims.dtype == MPCQ_F32 ? 1e-20 : 1e-32;
    a.P = c->d_P;
    a.q0 = c->d_q0;
    a.A = c->d_A;
    a.l0 = c->d_l0;
    a.u0 = c->d_u0;
    a.ops = c->d_ops;
    a.ctype = c->d_ctype;
    a.status = c->d_setup_status;
    a.flags = c->d_flags;
    // One wavefront per plant, LDS-resident (mpcq_setup_wave.hip), where the plant fits: per-plant
    // batches take the direct inverse of M(rho) (no eigen-solve: their QPs are solved once or a few
    // times each), a shared plant the eigen-basis (every QP of the batch reuses it, whatever rho it
    // reaches; the tile kernel's images).  The global-scratch workgroup kernel (eigen-basis) serves
    // larger plants.  Test hook MPCQ_SETUP: "ref" forces the workgroup kernel, "eigen" the wave
    // kernel's eigen-basis for per-plant batches.
    const char *hook = test_hook("MPCQ_SETUP");
    const bool fits = mpcq_internal_setup_wave_lds((int)n, (int)m) != 0;
    const bool ref_setup = !std::strcmp(hook, "ref") || !fits;
    if (run.keep_scaling) {  // (in the reading the blocks were built in; the caller has checked that the plant fits)
        if (mpcq_internal_setup_keep_launch(&a, c->inv_ops, s) != 0) return fail(MPCQ_ERR_HIP, "setup kernel launch failed");
    } else if ((c->inv_ops = !ref_setup && Pn > 1 && std::strcmp(hook, "eigen") != 0)) {
        if (mpcq_internal_setup_inv_launch(&a, s) != 0) return fail(MPCQ_ERR_HIP, "setup kernel launch failed");
    } else if (ref_setup) {
        if (int rc = c->d_scratch.alloc(8 * Pn * setup_scratch_len((int)n, (int)m), "setup scratch")) return rc;
        a.scratch = c->d_scratch;
        if (mpcq_internal_setup_launch(&a, s) != 0) return fail(MPCQ_ERR_HIP, "setup kernel launch failed");
    } else {
        const char *pe = debug_hook("MPCQ_SETUP_PROF");  // per-stage clock stamps to a file
        DevBuf<long long> prof;
        if (*pe && prof.alloc(8 * 16 * Pn) == MPCQ_OK) {
            (void)hipMemsetAsync(prof, 0, 8 * 16 * Pn, s);
            a.prof = prof;
        }
        if (mpcq_internal_setup_wave_launch(&a, s) != 0) return fail(MPCQ_ERR_HIP, "setup kernel launch failed");
        if (prof) {
            std::vector<long long> h(16 * Pn);
            HIPCHK(hipMemcpyAsync(h.data(), prof, 8 * 16 * Pn, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (FILE *f = std::fopen(pe, "wb")) {
                std::fwrite(h.data(), 8, h.size(), f);
                std::fclose(f);
            } else {
                std::fprintf(stderr, "[mpcq] MPCQ_SETUP_PROF: cannot open %s for writing\n", pe);
            }
        }
    }
    // plant-0 scaling (mpcq_get_scaling, host-side bound checks) and the flag word: one sync
    const mpcq::OpsLayout L = mpcq::OpsLayout::make(c->nc, c->mc);
    if (run.check_lower &&
        mpcq_internal_lower_free_check(c->d_l, c->d_ops + L.E, (int)m, (size_t)c->dims.batch * m, c->d_flags, s) != 0)
        return fail(MPCQ_ERR_HIP, "lower-bound check kernel failed");
    if (run.check_paired && mpcq_internal_paired_check(c->d_A, (int)(n * n), c->d_flags, s) != 0)
        return fail(MPCQ_ERR_HIP, "paired-rows check kernel failed");
    std::vector<double> blk(c->ops_stride);
    int flags = 0;
    HIPCHK(hipMemcpyAsync(&flags, c->d_flags, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(blk.data(), c->d_ops, 8 * c->ops_stride, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (flags & 1) return fail(MPCQ_ERR_SETUP, "setup: P + sigma I (+ rho A'A) not positive definite (non-convex QP)");
    if (flags & 4) return fail(MPCQ_ERR_SETUP, "setup: Jacobi eigen-solve of the KKT family did not converge in 60 sweeps");
    if (flags_out) *flags_out = flags;
    if (!run.keep_scaling) c->all_ineq = !(flags & 2);  // (kept constraint types: the kept flag)
    for (size_t i = 0; i < n; i++) c->hD[i] = blk[L.D + i];
    for (size_t j = 0; j < m; j++) c->hE[j] = blk[L.E + j];
    c->hc = blk[L.cs];
    dinf_bounds(c, blk.data(), L);
    if (c->dims.dtype == MPCQ_F32 &&
        mpcq_internal_f64_to_f32(c->d_ops, c->d_ops32, Pn * c->ops_stride, s) != 0)
        return fail(MPCQ_ERR_HIP, "operator conversion failed");
    if (c->tile && mpcq_internal_tile_images(c->d_ops, c->nc, c->mc, c->KN, c->KM, c->dims.dtype == MPCQ_F32,
                                             c->d_img, s) != 0)
        return fail(MPCQ_ERR_HIP, "tile image kernel failed");
    return MPCQ_OK;
}

// Every QP's rho back to settings.rho, clamped as OSQP clamps it
int fill_rho(mpcq_ctx *c, hipStream_t s)
{
    const double r = std::min(std::max(c->set.rho, mpcq::kRhoMin), mpcq::kRhoMax);
    if (mpcq_internal_fill(c->d_rhos, c->dims.dtype == MPCQ_F32, r, c->dims.batch, s) != 0)
        return fail(MPCQ_ERR_HIP, "fill kernel failed");
    return MPCQ_OK;
}

// The warm state x = z = y = 0
int zero_warm_state(mpcq_ctx *c, hipStream_t s)
{
    const size_t B = c->dims.batch, es = c->dims.dtype == MPCQ_F32 ? 4 : 8;
    HIPCHK(hipMemsetAsync(c->d_xs, 0, es * c->nc * B, s));
    HIPCHK(hipMemsetAsync(c->d_zs, 0, es * c->mc * B, s));
    HIPCHK(hipMemsetAsync(c->d_ys, 0, es * c->mc * B, s));
    return MPCQ_OK;
}

// ---- osqp_update_P / osqp_update_A / osqp_update_P_A with a warm start (include/mpcq.h)

// The refusals of include/mpcq.h, before anything is enqueued or written
int update_check(mpcq_ctx *c, const char *fn, const void *P, const void *A, int rescale, hipStream_t s)
{
    if (!c) return fail(MPCQ_ERR_ARG, "null context");
    if (c->mimo_only || c->mode == mpcq_ctx::Mode::Mimo)
        return fail(MPCQ_ERR_ARG, std::string(fn) + ": MIMO contexts are not served");
    int rc = check_ctx(c, kGeneric);
    if (rc) return rc;
    // (a context without constraints has no A: an A alone is then nothing to update)
    if (!P && (!A || !c->dims.m)) return fail(MPCQ_ERR_ARG, std::string(fn) + ": P and A are both NULL");
    if (rescale != 0 && rescale != 1) return fail(MPCQ_ERR_ARG, std::string(fn) + ": rescale must be 0 or 1");
    if (rescale == 0 && !mpcq_internal_setup_wave_lds(c->dims.n, c->dims.m))
        return fail(MPCQ_ERR_ARG, std::string(fn) + ": rescale = 0 serves n <= 32, m <= 64 (the keep-scaling kernels)");
    return refuse_capture(fn, s);
}

// host: P, A are host arrays (copied before the call returns); otherwise device arrays read on s.
int update_P_A(mpcq_ctx *c, const double *P, const double *A, bool host, int rescale, hipStream_t s)
{
    // what the last solve left lazy, published with the operators and images it ran on: q, u stay the QPs' own,
    // x, y are the warm start, and rho, status, iter stay readable until the next solve
    int rc = materialize_qu(c);
    if (rc || (rc = materialize_xy(c)) || (rc = materialize_rho(c)) || (rc = materialize_info(c))) return rc;
    if ((rc = order_after_last(c, s))) return rc;
    c->last = s;
    c->sens_ok = false;
    c->pol_valid = false;
    c->mode = mpcq_ctx::Mode::None;  // (until the new factors stand: a failed update needs mpcq_setup)
    const size_t Pn = c->dims.n_plants, n = c->dims.n, m = c->dims.m, B = c->dims.batch;
    if (!m) A = nullptr;
    const hipMemcpyKind kind = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    if (P) HIPCHK(hipMemcpyAsync(c->d_P, P, 8 * Pn * n * n, kind, s));
    if (A) HIPCHK(hipMemcpyAsync(c->d_A, A, 8 * Pn * m * n, kind, s));
    if (host) HIPCHK(hipStreamSynchronize(s));
    SetupRun run;
    run.keep_scaling = rescale == 0;
    // a shared plant's lower_free follows E (exact rule); a per-plant context's rule does not read the scaling
    run.check_lower = Pn == 1 && m > 0;
    run.check_paired = A && Pn == 1 && m == 2 * n && n % 4 == 0;
    int flags = 0;
    if ((rc = run_setup(c, s, run, &flags))) return rc;
    if (A) c->paired = run.check_paired && !(flags & 16);
    if (run.check_lower) c->lower_free = !(flags & 8);
    // every QP's rho back to settings.rho; the warm state from the previous unscaled (x, y) under the new operators
    const bool f32 = c->dims.dtype == MPCQ_F32;
    if ((rc = fill_rho(c, s))) return rc;
    if (c->have_xy) {
        rc = f32 ? mpcq::launch_warm_start(make_args<float>(c), c->nc, c->mc, c->d_x, c->d_y, s)
                 : mpcq::launch_warm_start(make_args<double>(c), c->nc, c->mc, c->d_x, c->d_y, s);
        if (rc || mpcq_internal_cold_nonfinite(c->d_x, c->d_y, (int)n, (int)m, c->nc, c->mc, (int)B, f32, c->d_xs, c->d_zs,
                                               c->d_ys, s) != 0)
            return fail(MPCQ_ERR_HIP, "warm start kernel failed");
    } else if ((rc = zero_warm_state(c, s))) {
        return rc;
    }
    c->mode = mpcq_ctx::Mode::Generic;  // (gen: bumped once, by run_setup)
    if ((rc = build_order_map(c))) return rc;  // (new P, A: the MPC step's order map, if operators are set)
    verbose_header(c, rescale ? "mpcq_update_P_A (osqp_update_P_A: scaling, KKT basis, warm start)"
                              : "mpcq_update_P_A (kept scaling: KKT basis, warm start)");
    return MPCQ_OK;
}


}  // namespace

int reset_state(mpcq_ctx *c, bool reset_rho)
{
    if (int rc = materialize_xy(c)) return rc;  // (the warm state it zeroes is the last solve's x, y)
    if (int rc = materialize_rho(c)) return rc;
    if (int rc = zero_warm_state(c, c->last)) return rc;
    return reset_rho ? fill_rho(c, c->last) : MPCQ_OK;
}

int setup_on_device(mpcq_ctx *c, hipStream_t s)
{
    if (int rc = materialize_xy(c)) return rc;  // (with the images of the solve that left it)
    c->lazy.qu = false;  // (q, u are re-broadcast from the setup data below)
    c->have_xy = false;
    if (int rc = run_setup(c, s)) return rc;
    const size_t Pn = c->dims.n_plants, n = c->dims.n, m = c->dims.m, B = c->dims.batch;
    const int per = Pn > 1;
    if (mpcq_internal_broadcast(c->d_q0, c->d_q, (int)n, (int)B, per, s) ||
        mpcq_internal_broadcast(c->d_u0, c->d_u, (int)m, (int)B, per, s) ||
        mpcq_internal_broadcast(c->d_l0, c->d_l, (int)m, (int)B, per, s))
        return fail(MPCQ_ERR_HIP, "broadcast failed");
    return reset_state(c, true);
}

// The bound-violation map of the hardest-first order (mpcq_order.hip) for a shared plant with MPC
// operators: x_u = -P^-1 q is the QP's unconstrained optimum and v = A x_u - u, with q = Fx X + Fu U +
// (Fr 1) xref and u = W0 + Sbar X + Ku U (setF :372-375, setUpperBound :360-369), so
//   v = (-A P^-1 Fx - Sbar) X + (-A P^-1 Fu - Ku) U + (-A P^-1 Fr 1) xref - W0   (OrderBins row layout).
// Host fp64 (Cholesky of plant 0's P, upper triangle as OSQP reads it), once per setup / operator set;
// the map only orders the batch (no result depends on it), so a P that is not positive definite or a
// shape the kernel does not take just leaves the order off.
// The order map's rows from one plant's condensed operators (host fp64): false when P is not positive
// definite or a row is not finite (no order then).
bool order_map_rows(int n, int m, int nx, const std::vector<double> &P, const std::vector<double> &A,
                    const std::vector<double> &Fx, const std::vector<double> &Fu, const std::vector<double> &Fr,
                    const std::vector<double> &Sb, const std::vector<double> &Ku, const std::vector<double> &W0,
                    std::vector<double> &map, std::vector<double> *G)
{
    // Cholesky P = L L' (lower L in place, from P's upper triangle)
    std::vector<double> L((size_t)n * n, 0.0);
    for (int j = 0; j < n; j++) {
        for (int i = j; i < n; i++) {
            double v = P[(size_t)j * n + i];  // P(j, i), j <= i: upper triangle
            for (int k = 0; k < j; k++) v -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            if (i == j) {
                if (!(v > 0.0)) return false;  // not positive definite: no order
                L[(size_t)j * n + j] = std::sqrt(v);
            } else {
                L[(size_t)i * n + j] = v / L[(size_t)j * n + j];
            }
        }
    }
    // Z = P^-1 [Fx Fu Fr1] (n x (nx + 2)), then the map rows
    const int nr = nx + 2;
    std::vector<double> Z((size_t)n * nr);
    for (int i = 0; i < n; i++) {
        for (int t = 0; t < nx; t++) Z[(size_t)i * nr + t] = Fx[(size_t)i * nx + t];
        Z[(size_t)i * nr + nx] = Fu[i];
        double fr = 0.0;
        for (int t = 0; t < n; t++) fr += Fr[(size_t)i * n + t];
        Z[(size_t)i * nr + nx + 1] = fr;
    }
    for (int r = 0; r < nr; r++) {
        for (int i = 0; i < n; i++) {  // L y = b
            double v = Z[(size_t)i * nr + r];
            for (int k = 0; k < i; k++) v -= L[(size_t)i * n + k] * Z[(size_t)k * nr + r];
            Z[(size_t)i * nr + r] = v / L[(size_t)i * n + i];
        }
        for (int i = n - 1; i >= 0; i--) {  // L' z = y
            double v = Z[(size_t)i * nr + r];
            for (int k = i + 1; k < n; k++) v -= L[(size_t)k * n + i] * Z[(size_t)k * nr + r];
            Z[(size_t)i * nr + r] = v / L[(size_t)i * n + i];
        }
    }
    constexpr int KS = mpcq::OrderBins::kStride;
    map.assign((size_t)m * KS, 0.0);
    for (int j = 0; j < m; j++) {
        double az[10] = {0};
        for (int r = 0; r < nr; r++)
            for (int i = 0; i < n; i++) az[r] += A[(size_t)j * n + i] * Z[(size_t)i * nr + r];
        double *row = map.data() + (size_t)j * KS;
        for (int t = 0; t < nx; t++) row[t] = -az[t] - Sb[(size_t)j * nx + t];
        row[8] = -az[nx] - Ku[j];
        row[9] = -W0[j];
        row[10] = -az[nx + 1];
        for (int k = 0; k < KS; k++)
            if (!std::isfinite(row[k])) return false;
    }
    // per-QP references (mpcq_mpc_step_ref*): the xref column generalises to G = -A P^-1 Fr (m x n), so that
    // v gains G ref_b; G left empty where a row is not finite (reference steps then run in index order)
    if (G) {
        std::vector<double> Y((size_t)n * n);  // P^-1 Fr, column by column
        for (int r = 0; r < n; r++) {
            for (int i = 0; i < n; i++) {  // L y = b
                double v = Fr[(size_t)i * n + r];
                for (int k = 0; k < i; k++) v -= L[(size_t)i * n + k] * Y[(size_t)k * n + r];
                Y[(size_t)i * n + r] = v / L[(size_t)i * n + i];
            }
            for (int i = n - 1; i >= 0; i--) {  // L' z = y
                double v = Y[(size_t)i * n + r];
                for (int k = i + 1; k < n; k++) v -= L[(size_t)k * n + i] * Y[(size_t)k * n + r];
                Y[(size_t)i * n + r] = v / L[(size_t)i * n + i];
            }
        }
        G->assign((size_t)m * n, 0.0);
        for (int j = 0; j < m && !G->empty(); j++)
            for (int r = 0; r < n; r++) {
                double s = 0.0;
                for (int i = 0; i < n; i++) s += A[(size_t)j * n + i] * Y[(size_t)i * n + r];
                if (!std::isfinite(s)) { G->clear(); break; }
                (*G)[(size_t)j * n + r] = -s;
            }
    }
    return true;
}

// The map to the device, with the order's counters and lists (allocated once per context).
int upload_order_map(mpcq_ctx *c, const std::vector<double> &map, hipStream_t s)
{
    constexpr int KS = mpcq::OrderBins::kStride;
    const size_t ord_ints = (size_t)mpcq::OrderBins::kBins + 4 * (size_t)c->dims.batch;  // counters, keys, list, info
    if (int rc = c->d_ordmap.alloc(8 * (size_t)mpcq::OrderBins::kMaxRows * KS, "order map")) return rc;
    if (!c->d_ord) {
        if (int rc = c->d_ord.alloc(4 * ord_ints, "order lists")) return rc;
        HIPCHK(hipMemsetAsync(c->d_ord, 0, 4 * ord_ints, s));  // (list entries are batch indices, from the start)
        c->ord_clean = true;
        c->gen++;
    }
    if (int rc2 = h2d(c->d_ordmap, map.data(), 8 * map.size(), s)) return rc2;
    return MPCQ_OK;
}

int build_order_map(mpcq_ctx *c)
{
    c->ord_ok = false;
    const int n = c->dims.n, m = c->dims.m, nx = c->nx;
    if (!c->tile || !c->mpc_ready || c->dims.n_plants != 1 || c->mode != mpcq_ctx::Mode::Generic || nx <= 0 ||
        nx > 8 || m > mpcq::OrderBins::kMaxRows)
        return MPCQ_OK;
    std::vector<double> P((size_t)n * n), A((size_t)m * n), Fx((size_t)n * nx), Fu(n), Fr((size_t)n * n),
        Sb((size_t)m * nx), Ku(m), W0(m);
    hipStream_t s = c->last;
    HIPCHK(hipMemcpyAsync(P.data(), c->d_P, 8 * P.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(A.data(), c->d_A, 8 * A.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(Fx.data(), c->d_Fx, 8 * Fx.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(Fu.data(), c->d_Fu, 8 * Fu.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(Fr.data(), c->d_Fr, 8 * Fr.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(Sb.data(), c->d_Sbar, 8 * Sb.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(Ku.data(), c->d_Ku, 8 * Ku.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(W0.data(), c->d_W0, 8 * W0.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<double> map, G;
    c->ordG_ok = false;
    if (!order_map_rows(n, m, nx, P, A, Fx, Fu, Fr, Sb, Ku, W0, map, &G)) return MPCQ_OK;
    if (int rc = upload_order_map(c, map, s)) return rc;
    if (!G.empty() && n <= 32) {  // (the order kernel's LDS rows of G: kOrderRefN columns)
        if (int rc = c->d_ordG.alloc(8 * (size_t)mpcq::OrderBins::kMaxRows * 32, "order map")) return rc;
        if (int rc = h2d(c->d_ordG, G.data(), 8 * G.size(), s)) return rc;
        c->ordG_ok = true;
    }
    c->ord_ok = true;
    c->pord_ok = false;  // (the map is now this plant's)
    return MPCQ_OK;
}

extern "C" {

int mpcq_setup(mpcq_ctx *c, const double *P, const double *q0, const double *A, const double *l0,
               const double *u0)
{
    int rc = check_generic_dims(c);
    if (rc) return rc;
    const size_t Pn = c->dims.n_plants, n = c->dims.n, m = c->dims.m;
    if (!P || !q0 || (m && (!A || !l0 || !u0))) return fail(MPCQ_ERR_ARG, "null setup array");
    for (size_t i = 0; i < Pn * m; i++)
        if (l0[i] > u0[i]) return fail(MPCQ_ERR_BOUNDS, "lower bound above upper bound (osqp validate_data)");
    if ((rc = ensure_plant_buffers(c))) return rc;
    c->mode = mpcq_ctx::Mode::None;
    c->sens_ok = false;
    // rows n + j of A are the negated rows j (the reference's Gbar = [K0 L; -K0 L],
    // ModelPredictiveControlAPI.cpp:332-347), checked bit for bit: the tile kernel's paired loop
    c->paired = Pn == 1 && m == 2 * n && n % 4 == 0;
    for (size_t i = 0; c->paired && i < n * n; i++)
        if (!(A[n * n + i] == -A[i])) c->paired = false;
    hipStream_t s = c->last;
    if ((rc = h2d(c->d_P, P, 8 * Pn * n * n, s)) || (rc = h2d(c->d_q0, q0, 8 * Pn * n, s)) ||
        (rc = h2d(c->d_A, A, 8 * Pn * m * n, s)) || (rc = h2d(c->d_l0, l0, 8 * Pn * m, s)) ||
        (rc = h2d(c->d_u0, u0, 8 * Pn * m, s)))
        return rc;
    if ((rc = setup_on_device(c, s))) return rc;
    c->lower_free = lower_all_free(c, l0);
    c->gen++;
    c->mode = mpcq_ctx::Mode::Generic;
    if ((rc = build_order_map(c))) return rc;  // (new P, A: the MPC step's order map, if operators are set)
    verbose_header(c, "mpcq_setup (osqp_setup: Ruiz scaling, constraint types, KKT basis)");
    return MPCQ_OK;
}

int mpcq_update_lin_cost(mpcq_ctx *c, const double *q)
{
    int rc = check_ctx(c, kGeneric);
    if (rc) return rc;
    if ((rc = materialize_qu(c))) return rc;  // (the other vector of the pending step)
    if (!q) return fail(MPCQ_ERR_ARG, "null q");
    c->sens_ok = false;  // (d_q, d_l, d_u are no longer the last solve's)
    return h2d(c->d_q, q, 8 * (size_t)c->dims.batch * c->dims.n, c->last);
}

int mpcq_update_upper_bound(mpcq_ctx *c, const double *u)
{
    int rc = check_ctx(c, kGeneric);
    if (rc) return rc;
    if ((rc = materialize_qu(c))) return rc;  // (the other vector of the pending step)
    if (!u) return fail(MPCQ_ERR_ARG, "null u");
    c->sens_ok = false;
    return h2d(c->d_u, u, 8 * (size_t)c->dims.batch * c->dims.m, c->last);
}

int mpcq_update_lower_bound(mpcq_ctx *c, const double *l)
{
    int rc = check_ctx(c, kGeneric);
    if (rc) return rc;
    if ((rc = materialize_qu(c))) return rc;  // (the other vector of the pending step)
    if (!l) return fail(MPCQ_ERR_ARG, "null l");
    const bool lf = lower_all_free_batch(c, l);
    if (lf != c->lower_free) c->gen++;
    c->lower_free = lf;
    c->sens_ok = false;
    return h2d(c->d_l, l, 8 * (size_t)c->dims.batch * c->dims.m, c->last);
}

int mpcq_update_bounds(mpcq_ctx *c, const double *l, const double *u)
{
    int rc = mpcq_update_lower_bound(c, l);
    return rc ? rc : mpcq_update_upper_bound(c, u);
}

int mpcq_cold_start(mpcq_ctx *c)
{
    int rc = check_ctx(c, kGeneric);
    if (rc) return rc;
    c->sens_ok = false;  // (the warm state is no longer the last solve's iterate)
    c->have_xy = false;  // (a matrix update before the next solve keeps the cold start: mpcq_update_P_A_device)
    if ((rc = reset_state(c, false))) return rc;
    HIPCHK(hipStreamSynchronize(c->last));
    return MPCQ_OK;
}

int mpcq_warm_start(mpcq_ctx *c, const double *x, const double *y)
{
    int rc = check_ctx(c, kGeneric);
    if (rc) return rc;
    if (!x || (c->dims.m && !y)) return fail(MPCQ_ERR_ARG, "null x/y");
    c->lazy.xy = false;  // (x, y are staged in the output buffers below; a rejected call keeps a pending x, y)
    c->sens_ok = false;
    // stage in the output buffers (overwritten by the next solve)
    if ((rc = h2d(c->d_x, x, 8 * (size_t)c->dims.batch * c->dims.n, c->last))) return rc;
    if ((rc = h2d(c->d_y, y, 8 * (size_t)c->dims.batch * c->dims.m, c->last))) return rc;
    rc = c->dims.dtype == MPCQ_F32 ? mpcq::launch_warm_start(make_args<float>(c), c->nc, c->mc, c->d_x, c->d_y, c->last)
                                   : mpcq::launch_warm_start(make_args<double>(c), c->nc, c->mc, c->d_x, c->d_y, c->last);
    if (rc) return fail(MPCQ_ERR_HIP, "warm start kernel failed");
    HIPCHK(hipStreamSynchronize(c->last));
    c->have_xy = true;
    return MPCQ_OK;
}

int mpcq_update_P_A_device(mpcq_ctx *c, const double *P_dev, const double *A_dev, int rescale, void *stream)
{
    int rc = update_check(c, "mpcq_update_P_A_device", P_dev, A_dev, rescale, (hipStream_t)stream);
    return rc ? rc : update_P_A(c, P_dev, A_dev, false, rescale, (hipStream_t)stream);
}

int mpcq_update_P_A(mpcq_ctx *c, const double *P, const double *A, int rescale)
{
    int rc = update_check(c, "mpcq_update_P_A", P, A, rescale, c ? c->last : nullptr);
    if (rc || (rc = update_P_A(c, P, A, true, rescale, c->last))) return rc;
    HIPCHK(hipStreamSynchronize(c->last));
    return MPCQ_OK;
}

}  // extern "C"

// solvempc_amd/csrc/mpcq_host_plants.cpp — host side of the C ABI declared in include/mpcq.h: condensing and its
// VJP, the per-plant MPC setup and one-pass step.
#include "mpcq_ctx.h"

namespace {

// The argument refusals of mpcq_condense_vjp* (include/mpcq.h), before anything is enqueued or written
int condense_vjp_check(int n_plants, int nx, int N, int s_rows, const double *const (&plant)[7],
                       const double *const (&cot)[7], double *const (&out)[7])
{
    if (n_plants < 1 || nx < 1 || nx > 8 || N < 1 || N > 32 || s_rows < 0)
        return fail(MPCQ_ERR_ARG, "condense_vjp: n_plants >= 1, 1 <= nx <= 8, 1 <= N <= 32, s_rows >= 0");
    bool any_cot = false, any_out = false;
    for (auto p : plant)
        if (!p) return fail(MPCQ_ERR_ARG, "condense_vjp: null plant array");
    for (auto p : cot) any_cot |= p != nullptr;
    for (auto p : out) any_out |= p != nullptr;
    if (!any_cot) return fail(MPCQ_ERR_ARG, "condense_vjp: every cotangent is NULL");
    if (!any_out) return fail(MPCQ_ERR_ARG, "condense_vjp: every output is NULL");
    return MPCQ_OK;
}

int condense_vjp_launch(int n_plants, int nx, int N, int s_rows, const double *const (&plant)[7],
                        const double *const (&cot)[7], double *const (&out)[7], hipStream_t s)
{
    mpcq::CondenseVjpArgs a{};
    a.n_plants = n_plants;
    a.nx = nx;
    a.N = N;
    a.s_rows = s_rows;
    a.Ad = plant[0]; a.Bd = plant[1]; a.Cd = plant[2]; a.K = plant[3]; a.Q = plant[4]; a.R = plant[5]; a.RD = plant[6];
    a.gP = cot[0]; a.gA = cot[1]; a.gFx = cot[2]; a.gFu = cot[3]; a.gFr = cot[4]; a.gSbar = cot[5]; a.gKu = cot[6];
    a.gAd = out[0]; a.gBd = out[1]; a.gCd = out[2]; a.gK = out[3]; a.gQ = out[4]; a.gR = out[5]; a.gRD = out[6];
    if (mpcq_internal_condense_vjp_launch(&a, s) != 0) return fail(MPCQ_ERR_HIP, "condense_vjp launch failed");
    return MPCQ_OK;
}

// hipSetDevice(device) for the length of a stateless call; the caller's current device is put back afterwards
struct DeviceScope {
    int prev = -1, rc = MPCQ_OK;
    explicit DeviceScope(int device)
    {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
            (void)hipGetLastError();
            rc = fail(MPCQ_ERR_HIP, "no HIP device with this ordinal");
            return;
        }
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || (cur != device && hipSetDevice(device) != hipSuccess))
            rc = fail(MPCQ_ERR_HIP, "hipSetDevice failed");
        else if (cur != device)
            prev = cur;
    }
    ~DeviceScope()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// The hardest-first map of a batch of distinct plants: the first plant's condensed operators (mpcq_condense,
// synchronous: once per set of plant arrays), folded as build_order_map folds a shared plant's.  The plants of
// config 3 are perturbations of one nominal plant (Ad, Bd +-2 %), so one plant's map ranks every QP's
// unconstrained-optimum violation closely enough to group QPs of like iteration counts in a wave and to run
// the slow ones first; the map only orders the batch, no result depends on it (a stale map, after the
// arrays' contents change under the same pointers, costs time only).
int plants_order_map(mpcq_ctx *c, int nx, int s_rows, const double *Ad, const double *Bd, const double *Cd,
                            const double *K, const double *Q, const double *R, const double *RD, hipStream_t s)
{
    const int n = c->dims.n, m = c->dims.m;
    if (c->pord_ok && c->pord_key.Ad == Ad && c->pord_key.Bd == Bd && c->pord_key.Cd == Cd && c->pord_key.K == K &&
        c->pord_key.Q == Q && c->pord_key.R == R && c->pord_key.RD == RD && c->pord_key.nx == nx &&
        c->pord_key.s_rows == s_rows)
        return MPCQ_OK;
    c->pord_ok = false;
    c->ord_ok = false;  // (d_ordmap is about to hold the plants' map)
    if (m > mpcq::OrderBins::kMaxRows || nx > 8) return MPCQ_OK;
    std::vector<double> in((size_t)nx * nx + 3 * nx + 3);
    double *hAd = in.data(), *hBd = hAd + nx * nx, *hCd = hBd + nx, *hK = hCd + nx, *hQ = hK + nx;
    HIPCHK(hipMemcpyAsync(hAd, Ad, 8 * (size_t)nx * nx, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hBd, Bd, 8 * (size_t)nx, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hCd, Cd, 8 * (size_t)nx, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hK, K, 8 * (size_t)nx, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hQ, Q, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hQ + 1, R, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hQ + 2, RD, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<double> P((size_t)n * n), A((size_t)m * n), Fx((size_t)n * nx), Fu(n), Fr((size_t)n * n),
        Sb((size_t)m * nx), Ku(m), W0(m);
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (mpcq_condense(dev, 1, nx, n, s_rows, hAd, hBd, hCd, hK, hQ, hQ + 1, hQ + 2, P.data(), A.data(), Fx.data(),
                      Fu.data(), Fr.data(), Sb.data(), Ku.data(), W0.data()) != MPCQ_OK)
        return MPCQ_OK;  // (no order: the step itself reports any error with these arrays)
    std::vector<double> map;
    if (!order_map_rows(n, m, nx, P, A, Fx, Fu, Fr, Sb, Ku, W0, map)) return MPCQ_OK;
    if (int rc = upload_order_map(c, map, s)) return rc;
    c->pord_ok = true;
    c->pord_key = {Ad, Bd, Cd, K, Q, R, RD, nx, s_rows};
    return MPCQ_OK;
}

}  // namespace

extern "C" {

int mpcq_condense(int device, int n_plants, int nx, int N, int s_rows, const double *Ad, const double *Bd,
                  const double *Cd, const double *K, const double *Q, const double *R, const double *RD, double *P,
                  double *A, double *Fx, double *Fu, double *Fr, double *Sbar, double *Ku, double *W0)
{
    if (n_plants <= 0 || nx <= 0 || nx > 8 || N <= 0 || s_rows < 0)
        return fail(MPCQ_ERR_ARG, "condense: n_plants > 0, 1 <= nx <= 8, N > 0, s_rows >= 0");
    const double *in[] = {Ad, Bd, Cd, K, Q, R, RD};
    double *outp[] = {P, A, Fx, Fu, Fr, Sbar, Ku, W0};
    for (auto p : in)
        if (!p) return fail(MPCQ_ERR_ARG, "condense: null input");
    for (auto p : outp)
        if (!p) return fail(MPCQ_ERR_ARG, "condense: null output");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail(MPCQ_ERR_HIP, "no HIP device with this ordinal");
    HIPCHK(hipSetDevice(device));
    const size_t Pn = n_plants, X = nx, n = N;
    const size_t in_cnt[] = {Pn * X * X, Pn * X, Pn * X, Pn * X, Pn, Pn, Pn};
    const size_t out_cnt[] = {Pn * n * n, Pn * 2 * n * n, Pn * n * X, Pn * n, Pn * n * n, Pn * 2 * n * X, Pn * 2 * n, Pn * 2 * n};
    const bool force_ref = !std::strcmp(test_hook("MPCQ_CONDENSE"), "ref");  // the workgroup kernel
    const size_t scr = (N > 32 || force_ref) ? Pn * mpcq_internal_condense_scratch(nx, N) : 0;
    size_t total = scr;
    for (size_t c : in_cnt) total += c;
    for (size_t c : out_cnt) total += c;
    DevBuf<double> buf;
    if (int rc = buf.alloc(8 * total)) return rc;
    mpcq::CondenseArgs a{};
    double *p = buf;
    const double **din[] = {&a.Ad, &a.Bd, &a.Cd, &a.K, &a.Q, &a.R, &a.RD};
    double **dout[] = {&a.P, &a.A, &a.Fx, &a.Fu, &a.Fr, &a.Sbar, &a.Ku, &a.W0};
    for (int i = 0; i < 7; i++) {
        *din[i] = p;
        if (hipMemcpy(p, in[i], 8 * in_cnt[i], hipMemcpyHostToDevice) != hipSuccess) return fail(MPCQ_ERR_HIP, "h2d");
        p += in_cnt[i];
    }
    for (int i = 0; i < 8; i++) {
        *dout[i] = p;
        p += out_cnt[i];
    }
    a.scratch = scr ? p : nullptr;
    a.force_ref = force_ref;
    a.n_plants = n_plants;
    a.nx = nx;
    a.N = N;
    a.s_rows = s_rows;
    if (mpcq_internal_condense_launch(&a, nullptr) != 0) return fail(MPCQ_ERR_HIP, "condense launch failed");
    if (hipDeviceSynchronize() != hipSuccess) return fail(MPCQ_ERR_HIP, "condense kernel failed");
    for (int i = 0; i < 8; i++)
        if (hipMemcpy(outp[i], *dout[i], 8 * out_cnt[i], hipMemcpyDeviceToHost) != hipSuccess)
            return fail(MPCQ_ERR_HIP, "d2h");
    return MPCQ_OK;
}

int mpcq_condense_vjp_device(int device, int n_plants, int nx, int N, int s_rows, const double *Ad, const double *Bd,
                             const double *Cd, const double *K, const double *Q, const double *R, const double *RD,
                             const double *gP, const double *gA, const double *gFx, const double *gFu,
                             const double *gFr, const double *gSbar, const double *gKu, double *gAd, double *gBd,
                             double *gCd, double *gK, double *gQ, double *gR, double *gRD, void *stream)
{
    const double *const plant[7] = {Ad, Bd, Cd, K, Q, R, RD}, *const cot[7] = {gP, gA, gFx, gFu, gFr, gSbar, gKu};
    double *const out[7] = {gAd, gBd, gCd, gK, gQ, gR, gRD};
    int rc = condense_vjp_check(n_plants, nx, N, s_rows, plant, cot, out);
    if (rc) return rc;
    DeviceScope dev(device);
    if (dev.rc) return dev.rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = refuse_capture("mpcq_condense_vjp_device", s))) return rc;
    return condense_vjp_launch(n_plants, nx, N, s_rows, plant, cot, out, s);
}

int mpcq_condense_vjp(int device, int n_plants, int nx, int N, int s_rows, const double *Ad, const double *Bd,
                      const double *Cd, const double *K, const double *Q, const double *R, const double *RD,
                      const double *gP, const double *gA, const double *gFx, const double *gFu, const double *gFr,
                      const double *gSbar, const double *gKu, double *gAd, double *gBd, double *gCd, double *gK,
                      double *gQ, double *gR, double *gRD)
{
    const double *const plant[7] = {Ad, Bd, Cd, K, Q, R, RD}, *const cot[7] = {gP, gA, gFx, gFu, gFr, gSbar, gKu};
    double *const out[7] = {gAd, gBd, gCd, gK, gQ, gR, gRD};
    int rc = condense_vjp_check(n_plants, nx, N, s_rows, plant, cot, out);
    if (rc) return rc;
    DeviceScope dev(device);
    if (dev.rc) return dev.rc;
    const size_t Pn = n_plants, X = nx, n = N;
    const size_t plant_cnt[7] = {Pn * X * X, Pn * X, Pn * X, Pn * X, Pn, Pn, Pn};
    const size_t cot_cnt[7] = {Pn * n * n, Pn * 2 * n * n, Pn * n * X, Pn * n, Pn * n * n, Pn * 2 * n * X, Pn * 2 * n};
    size_t total = 0;
    for (int i = 0; i < 7; i++) total += 2 * plant_cnt[i] + (cot[i] ? cot_cnt[i] : 0);
    DevBuf<double> buf;
    if ((rc = buf.alloc(8 * total))) return rc;
    const double *dplant[7], *dcot[7];
    double *dout[7], *p = buf;
    for (int i = 0; i < 7; i++) {
        dplant[i] = p;
        if (hipMemcpy(p, plant[i], 8 * plant_cnt[i], hipMemcpyHostToDevice) != hipSuccess) return fail(MPCQ_ERR_HIP, "h2d");
        p += plant_cnt[i];
    }
    for (int i = 0; i < 7; i++) {
        dcot[i] = cot[i] ? p : nullptr;
        if (!cot[i]) continue;
        if (hipMemcpy(p, cot[i], 8 * cot_cnt[i], hipMemcpyHostToDevice) != hipSuccess) return fail(MPCQ_ERR_HIP, "h2d");
        p += cot_cnt[i];
    }
    for (int i = 0; i < 7; i++) {
        dout[i] = out[i] ? p : nullptr;
        p += plant_cnt[i];
    }
    if ((rc = condense_vjp_launch(n_plants, nx, N, s_rows, dplant, dcot, dout, nullptr))) return rc;
    if (hipDeviceSynchronize() != hipSuccess) return fail(MPCQ_ERR_HIP, "condense_vjp kernel failed");
    for (int i = 0; i < 7; i++)
        if (out[i] && hipMemcpy(out[i], dout[i], 8 * plant_cnt[i], hipMemcpyDeviceToHost) != hipSuccess)
            return fail(MPCQ_ERR_HIP, "d2h");
    return MPCQ_OK;
}

int mpcq_mpc_setup_plants_device(mpcq_ctx *c, int nx, int s_rows, const double *Ad, const double *Bd,
                                 const double *Cd, const double *K, const double *Q, const double *R,
                                 const double *RD, void *stream)
{
    int rc = check_generic_dims(c);
    if (rc) return rc;
    const size_t Pn = c->dims.n_plants, n = c->dims.n, m = c->dims.m;
    if (nx <= 0 || nx > 8 || s_rows < 0) return fail(MPCQ_ERR_ARG, "setup_plants: 1 <= nx <= 8, s_rows >= 0");
    if (m != 2 * n) return fail(MPCQ_ERR_ARG, "MPC front end needs m == 2n (ModelPredictiveControlAPI.cpp:47-48)");
    if (!Ad || !Bd || !Cd || !K || !Q || !R || !RD) return fail(MPCQ_ERR_ARG, "setup_plants: null plant array");
    if ((rc = ensure_plant_buffers(c))) return rc;
    if ((rc = materialize_qu(c))) return rc;  // (with the operators the pending step used)
    if ((rc = alloc_mpc_ops(c, nx))) return rc;
    c->nx = nx;
    c->mode = mpcq_ctx::Mode::None;
    c->sens_ok = false;
    hipStream_t s = (hipStream_t)stream;
    c->last = s;
    mpcq::CondenseArgs a{};
    a.n_plants = (int)Pn;
    a.nx = nx;
    a.N = (int)n;
    a.s_rows = s_rows;
    a.Ad = Ad; a.Bd = Bd; a.Cd = Cd; a.K = K; a.Q = Q; a.R = R; a.RD = RD;
    a.P = c->d_P; a.A = c->d_A;
    set_front_end_ops(c, a);
    a.q0 = c->d_q0; a.l0 = c->d_l0; a.u0 = c->d_u0;
    DevBuf<double> scr;  // (setup_on_device synchronises s before it goes)
    if (n > 32 && (rc = scr.alloc(8 * Pn * mpcq_internal_condense_scratch(nx, (int)n), "condense scratch"))) return rc;
    a.scratch = scr;
    if (mpcq_internal_condense_launch(&a, s) != 0) return fail(MPCQ_ERR_HIP, "condense launch failed");
    if ((rc = setup_on_device(c, s))) return rc;
    c->last = s;
    c->lower_free = true;  // l0 = -DBL_MAX on every row (:42)
    c->gen++;
    c->mpc_ready = true;
    c->mode = mpcq_ctx::Mode::Generic;
    if ((rc = build_order_map(c))) return rc;  // (a shared plant's tile path: the step's order map)
    verbose_header(c, "mpcq_mpc_setup_plants_device (condensing + osqp_setup per plant)");
    return MPCQ_OK;
}

int mpcq_mpc_plants_step_device(mpcq_ctx *c, int nx, int s_rows, const double *Ad, const double *Bd,
                                const double *Cd, const double *K, const double *Q, const double *R,
                                const double *RD, const double *X, double *U, double xref, void *stream)
{
    int rc = check_generic_dims(c);
    if (rc) return rc;
    if (c->set.polish) return fail(MPCQ_ERR_ARG, polish_refusal("mpcq_mpc_plants_step_device"));
    const int n = c->dims.n, m = c->dims.m;
    if (nx <= 0 || nx > 8 || s_rows < 0) return fail(MPCQ_ERR_ARG, "plants_step: 1 <= nx <= 8, s_rows >= 0");
    if (m != 2 * n || n > 32) return fail(MPCQ_ERR_ARG, "plants_step: n = N <= 32, m = 2N (ModelPredictiveControlAPI.cpp:47-48)");
    if (c->dims.n_plants != c->dims.batch) return fail(MPCQ_ERR_ARG, "plants_step: one plant per QP (n_plants == batch)");
    if (!Ad || !Bd || !Cd || !K || !Q || !R || !RD || !X || !U) return fail(MPCQ_ERR_ARG, "plants_step: null array");
    hipStream_t s = (hipStream_t)stream;
    // the kernel below rewrites x, y, rho, status and iter of every QP on `s`: a pending lazy publication of an
    // earlier solve is dropped, not formed (it would be wasted work, and on another stream unordered with s)
    c->lazy.clear_results();
    // (the earlier solve's work on its stream before this one's writes)
    if (c->last && order_after_last(c, s)) return fail(MPCQ_ERR_HIP, "plants_step: stream ordering failed");
    HIPCHK(hipMemsetAsync(c->d_flags, 0, 4, s));
    mpcq::PlantStepArgs a{};
    a.n_plants = c->dims.batch;
    a.nx = nx; a.N = n; a.s_rows = s_rows;
    a.Ad = Ad; a.Bd = Bd; a.Cd = Cd; a.K = K; a.Q = Q; a.R = R; a.RD = RD;
    a.X = X; a.U = U; a.xref = xref;
    a.st = to_solver(c->set);
    const int ct = c->set.check_termination;
    a.adaptive_interval = c->set.adaptive_rho_interval ? c->set.adaptive_rho_interval : (ct ? 4 * ct : 100);
    a.x = c->d_x; a.y = c->d_y; a.rho_out = c->d_rho; a.status = c->d_status; a.iter = c->d_iter;
    a.flags = c->d_flags;
    {
        // fp64 at 3 waves/SIMD (189 -> 168 VGPRs, a few spills in the check code: 39.4-40.0 M QP/s against
        // 35.5-35.9 M at 2), fp32 at 2 (3 spills into its loop: slower); MPCQ_PLANT_WPE=2|3 for A/B
        const char *w = test_hook("MPCQ_PLANT_WPE");
        a.wpe = *w ? std::atoi(w) : (c->dims.dtype == MPCQ_F32 ? 2 : 3);
        const char *l = test_hook("MPCQ_PLANT_LAYOUT");  // 2: two plants per wave at N 17 .. 20 (A/B, parity)
        a.layout = *l ? std::atoi(l) : 0;
    }
    // hardest-first (the first plant's map, mpcq_order.hip; test hook MPCQ_PLANT_ORDER=0: index order): slot i
    // of the grid runs plant list[i], and the kernel's workgroup 0 clears the bin counters for the next sort
    const bool want = test_hook("MPCQ_PLANT_ORDER")[0] != '0' && c->dims.batch < (1 << mpcq::OrderBins::kRankBits) &&
                      !stream_capturing(s);
    if (want && (rc = plants_order_map(c, nx, s_rows, Ad, Bd, Cd, K, Q, R, RD, s))) return rc;
    const bool ordered = want && c->pord_ok;
    if (ordered) {
        const int B = c->dims.batch;
        int *const cnt = c->d_ord, *const key = cnt + mpcq::OrderBins::kBins, *const list = key + B;
        if (!c->ord_clean) HIPCHK(hipMemsetAsync(cnt, 0, 4 * (size_t)mpcq::OrderBins::kBins, s));
        c->ord_clean = false;
        if (mpcq_internal_order(B, nx, m, X, U, c->d_ordmap, xref, cnt, key, list, nullptr, nullptr, s) != 0)
            return fail(MPCQ_ERR_HIP, "plants_step order launch failed");
        a.order = list;
        a.ord_zero = cnt;
    }
    const char *pst = debug_hook("MPCQ_PLANT_STAMPS");  // per-wave stage stamps (a -DMPCQ_PLANT_STAMPS build)
    const size_t nwaves = (size_t)c->dims.batch;  // (an upper bound on the grid)
    if (pst && *pst) {
        c->d_stamps.release();
        if ((rc = c->d_stamps.alloc(8 * 16 * nwaves, "stamps"))) return rc;
        HIPCHK(hipMemsetAsync(c->d_stamps, 0, 8 * 16 * nwaves, s));
        a.stamps = c->d_stamps;
    }
    const int lr = mpcq_internal_plant_step_launch(&a, c->dims.dtype == MPCQ_F32, s);
    if (lr) return fail(lr == -1 ? MPCQ_ERR_ARG : MPCQ_ERR_HIP, "plants_step kernel launch failed");
    if (pst && *pst && (rc = dump_stamps(pst, c->d_stamps, 16 * nwaves, s))) return rc;
    if (ordered) c->ord_clean = true;
    c->lazy.ord = ordered;
    c->mode = mpcq_ctx::Mode::OneShot;  // results only: no operator blocks were written
    c->sens_ok = false;
    c->mpc_ready = false;
    c->last = s;
    return MPCQ_OK;
}

}  // extern "C"

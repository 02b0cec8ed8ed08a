// solvempc_amd/csrc/mpcq_host_plants.cpp — host side of the C ABI declared in include/mpcq.h: condensing and its
// VJP, the per-plant MPC setup and one-pass step, the MIMO setup and step.
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
    if (pst && *pst) {
        std::vector<long long> h(16 * nwaves);
        HIPCHK(hipMemcpyAsync(h.data(), c->d_stamps, 8 * h.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (FILE *f = std::fopen(pst, "wb")) {
            std::fwrite(h.data(), 8, h.size(), f);
            std::fclose(f);
        }
    }
    if (ordered) c->ord_clean = true;
    c->lazy.ord = ordered;
    c->mode = mpcq_ctx::Mode::OneShot;  // results only: no operator blocks were written
    c->sens_ok = false;
    c->mpc_ready = false;
    c->last = s;
    return MPCQ_OK;
}

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
    if (c->mimo_N != N || c->mimo_nx != nx || c->mimo_nu != nu || c->mimo_ny != ny) c->d_mimo.release();
    if (c->mimo_nx != nx || c->mimo_nu != nu) {  // (the simulated plant of mpcq_mimo_set_plant_device has these shapes)
        c->d_mimo_Ad.release();
        c->d_mimo_Bd.release();
        c->mimo_plant = false;
    }
    if ((rc = c->d_mimo.alloc(8 * (size_t)L.total * c->dims.n_plants, "mimo operator blocks"))) return rc;
    c->mimo_N = N; c->mimo_nx = nx; c->mimo_nu = nu; c->mimo_ny = ny; c->mimo_srows = s_rows;
    c->mode = mpcq_ctx::Mode::None;
    c->sens_ok = false;
    c->mimo_stepped = false;
    c->mimo_ref_step = false;
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
    a.ops = c->d_mimo;
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
        std::vector<long long> h(16 * (size_t)a.n_plants);
        HIPCHK(hipMemcpy(h.data(), c->d_stamps, 8 * h.size(), hipMemcpyDeviceToHost));
        c->d_stamps.release();
        if (FILE *f = std::fopen(sst, "wb")) {
            std::fwrite(h.data(), 8, h.size(), f);
            std::fclose(f);
        }
    }
    if (flags & 1) return fail(MPCQ_ERR_SETUP, "mimo: P + sigma I is not positive definite (non-convex QP)");
    if (flags & 2) return fail(MPCQ_ERR_SETUP, "mimo: a constraint row is not an inequality (|w0| beyond OSQP_INFTY)");
    c->mimo_diag_k0 = (flags & 4) ? 0 : 1;
    c->last = s;
    c->fresh = true;  // the first step starts from x = z = y = 0, rho = settings.rho (initSolver, :64)
    c->mpc_ready = false;  // the generic front-end operators no longer describe this context
    c->mode = mpcq_ctx::Mode::Mimo;
    return MPCQ_OK;
}

}  // extern "C"

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
        if (r.stride != 0 && r.stride < (long long)c->mimo_N * c->mimo_ny)
            return fail(MPCQ_ERR_ARG, std::string(fn) + ": ref_stride is 0 (one reference for the batch) or >= N*n_y");
    }
    return polish ? refuse_capture(fn, s) : MPCQ_OK;
}

int mimo_step_enqueue(mpcq_ctx *c, const double *X, double *U, const MimoRef &r, void *stream)
{
    int rc = materialize_xy(c);  // (a pending lazy x, y first: the kernel below rewrites the state)
    if (rc) return rc;
    mpcq::MimoArgs a{};
    a.batch = c->dims.batch;
    a.N = c->mimo_N; a.nx = c->mimo_nx; a.nu = c->mimo_nu; a.ny = c->mimo_ny; a.s_rows = c->mimo_srows;
    a.diag_k0 = c->mimo_diag_k0 && !*test_hook("MPCQ_MIMO_GENERAL_K0");
    a.ops_stride = (size_t)mpcq::MimoLayout::make(a.N, a.nx, a.nu, a.ny).total;
    a.ops = c->d_mimo;
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
    if (stp && *stp) {
        std::vector<long long> h(8 * (size_t)a.batch);
        HIPCHK(hipMemcpyAsync(h.data(), c->d_stamps, 8 * h.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (FILE *f = std::fopen(stp, "wb")) {
            std::fwrite(h.data(), 8, h.size(), f);
            std::fclose(f);
        }
    }
    c->last = s;
    c->fresh = false;
    c->mimo_stepped = true;
    c->mimo_ref_step = r.horizon;
    c->pol_valid = false;
    return MPCQ_OK;
}

// The step, then OSQP's polish of every SOLVED QP on the same stream (mpcq_mimo_polish.hip)
int mimo_step_polish_enqueue(mpcq_ctx *c, const double *X, double *U, const MimoRef &r, void *stream)
{
    int rc = MPCQ_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t B = c->dims.batch, nu = c->mimo_nu;
    if ((rc = c->d_pol_status.alloc(4 * B)) || (rc = c->d_pol_nact.alloc(4 * B)) || (rc = c->d_pol_res.alloc(8 * 2 * B)) ||
        (rc = c->d_mimo_Uprev.grow(8 * B * nu, s, "mimo polish staging")))
        return rc;
    HIPCHK(hipMemcpyAsync(c->d_mimo_Uprev, U, 8 * B * nu, hipMemcpyDeviceToDevice, s));
    if ((rc = mimo_step_enqueue(c, X, U, r, stream))) return rc;
    mpcq::MimoPolishArgs a{};
    a.batch = c->dims.batch;
    a.N = c->mimo_N; a.nx = c->mimo_nx; a.nu = c->mimo_nu; a.ny = c->mimo_ny;
    a.ops_stride = (size_t)mpcq::MimoLayout::make(a.N, a.nx, a.nu, a.ny).total;
    a.ops = c->d_mimo;
    a.q = c->d_q; a.u = c->d_u;
    a.xs = (double *)c->d_xs; a.zs = (double *)c->d_zs; a.ys = (double *)c->d_ys;
    a.status = c->d_status;
    a.x = c->d_x; a.y = c->d_y;
    a.U_prev = c->d_mimo_Uprev; a.U = U;
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

}  // namespace

extern "C" {

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
    const size_t B = c->dims.batch, nx = c->mimo_nx, nu = c->mimo_nu, nr = (size_t)c->mimo_N * c->mimo_ny;
    const size_t rows = ref_stride ? B : 1;
    // staging of this call alone: X, U, then the references packed (B rows of N*n_y, or the one shared row)
    DevBuf<double> d;
    if ((rc = d.alloc(8 * (B * (nx + nu) + rows * nr), "mimo reference staging"))) return rc;
    struct Drain {  // (the stream is waited for, whatever the outcome, before the staging goes away)
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{c->last};
    double *dX = d, *dU = dX + B * nx, *dr = dU + B * nu;
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

}  // extern "C"

// ---- closed-loop MIMO runs: the existing step, launched once per control step, and
// mpcq_mimo_run.hip's plant kernel between two steps
namespace {

// A MIMO context with a simulated plant (MPCQ_ERR_ORDER otherwise)
int mimo_plant_check(mpcq_ctx *c, const char *fn)
{
    int rc = check_ctx(c, kNone);
    if (rc) return rc;
    if (c->mode != mpcq_ctx::Mode::Mimo) return fail(MPCQ_ERR_ORDER, "mpcq_mimo_setup_plants_device has not succeeded");
    if (!c->mimo_plant)
        return fail(MPCQ_ERR_ORDER, std::string(fn) + ": no simulated plant (mpcq_mimo_set_plant_device) for this setup's n_x, n_u");
    return MPCQ_OK;
}

// One plant update of every QP at absolute control step `step`; with a log, the step's record row and totals
int mimo_plant_enqueue(mpcq_ctx *c, double *X, const double *U, unsigned long long seed, long long first_qp,
                       long long step, double noise_std, const mpcq_mimo_log *log, hipStream_t s)
{
    mpcq::MimoPlantArgs a{};
    a.batch = c->dims.batch;
    a.nx = c->mimo_nx; a.nu = c->mimo_nu;
    a.Ad = c->d_mimo_Ad; a.Bd = c->d_mimo_Bd;
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
    const long long N = c->mimo_N, ny = c->mimo_ny, blocks = 2 * N - 1, base = std::max(sched_len - N, 0ll);
    const double *tail = nullptr;
    if (sched && first_step + steps - 1 + N > sched_len) {
        mpcq::MimoTailArgs t{};
        t.rows = sched_stride ? (long long)B : 1;
        t.stride = sched_stride;
        t.len = sched_len; t.base = base;
        t.blocks = (int)blocks; t.ny = (int)ny;
        t.sched = sched;
        if ((rc = c->d_mimo_tail.grow(8 * (size_t)(t.rows * blocks * ny), s, "mimo schedule tail"))) return rc;
        tail = t.tail = c->d_mimo_tail;
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

}  // namespace

extern "C" {

int mpcq_mimo_set_plant_device(mpcq_ctx *c, const double *Ad, const double *Bd, void *stream)
{
    const char *fn = "mpcq_mimo_set_plant_device";
    int rc = check_ctx(c, kNone);
    if (rc) return rc;
    if (c->mode != mpcq_ctx::Mode::Mimo) return fail(MPCQ_ERR_ORDER, "mpcq_mimo_setup_plants_device has not succeeded");
    if (!Ad || !Bd) return fail(MPCQ_ERR_ARG, std::string(fn) + ": null Ad/Bd");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = refuse_capture(fn, s))) return rc;
    const size_t B = c->dims.batch, nx = c->mimo_nx, nu = c->mimo_nu;
    // (both buffers are released whenever a MIMO setup changes n_x or n_u, so an allocated one has this size)
    if ((rc = c->d_mimo_Ad.alloc(8 * B * nx * nx, "mimo simulated plant")) ||
        (rc = c->d_mimo_Bd.alloc(8 * B * nx * nu, "mimo simulated plant")))
        return rc;
    HIPCHK(hipMemcpyAsync(c->d_mimo_Ad, Ad, 8 * B * nx * nx, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_mimo_Bd, Bd, 8 * B * nx * nu, hipMemcpyDeviceToDevice, s));
    c->mimo_plant = true;
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
    if (sched_stride != 0 && sched_stride < (long long)sched_len * c->mimo_ny)
        return fail(MPCQ_ERR_ARG, std::string(fn) + ": sched_stride is 0 (one schedule for the batch) or >= sched_len*n_y");
    return mimo_run_enqueue(c, X, U, nullptr, sched, sched_len, sched_stride, steps, seed, first_qp, first_step,
                            noise_std, polish, log, s);
}

}  // extern "C"

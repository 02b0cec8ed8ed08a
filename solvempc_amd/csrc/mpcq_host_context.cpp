// solvempc_amd/csrc/mpcq_host_context.cpp — host side of the C ABI declared in include/mpcq.h: the context and
// its buffers, the result readers, and the helpers every other host file shares.
//
// Orchestration only: argument checks, device buffers, kernel launches.  All arithmetic on the
// QPs (setup, ADMM, MPC front end) runs in the HIP kernels of mpcq_setup.hip / mpcq_admm.hip.
// There is no CPU solve path: without a gfx950 device mpcq_create fails with MPCQ_ERR_HIP.
#include "mpcq_ctx.h"

namespace {
thread_local std::string g_err;
}  // namespace

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

// The single-launch entry points cannot fit the polish pass (include/mpcq.h mpcq_settings)
std::string polish_refusal(const char *fn)
{
    return std::string(fn) + ": settings.polish is set, and this single-launch path has no polish pass (use mpcq_solve / "
                             "mpcq_mpc_step_device / mpcq_mpc_step, or a context without polish)";
}

// kGeneric: the generic / condensed-MPC operators (the generic kernels run on them); kAnySetup:
// either formulation (result readers).  A MIMO-only context never passes kGeneric.
int check_ctx(mpcq_ctx *c, Need need)
{
    if (!c) return fail(MPCQ_ERR_ARG, "null context");
    if (need == kGeneric && c->mimo_only)
        return fail(MPCQ_ERR_ARG, "n > 32 or m > 64 per plant: this context is served by mpcq_mimo_* only");
    if (need == kGeneric && c->mode != mpcq_ctx::Mode::Generic)
        return fail(MPCQ_ERR_ORDER, c->mode == mpcq_ctx::Mode::Mimo
                                        ? "the context was last set up by mpcq_mimo_setup_plants_device (MIMO)"
                                    : c->mode == mpcq_ctx::Mode::OneShot
                                        ? "mpcq_mpc_plants_step_device keeps no operators: set the plants up again"
                                        : "mpcq_setup has not succeeded");
    if (need == kAnySetup && c->mode == mpcq_ctx::Mode::None) return fail(MPCQ_ERR_ORDER, "no setup has succeeded");
    HIPCHK(hipSetDevice(c->dims.device));
    return MPCQ_OK;
}

// The plants' setup data and operator blocks (generic setups; mimo-only contexts keep one unused block)
int ensure_plant_buffers(mpcq_ctx *c)
{
    // (no early return on one pointer: after a failed allocation the next call allocates whatever is still
    // missing, so a call that returns MPCQ_OK always leaves every non-empty buffer allocated)
    const size_t Pg = c->mimo_only ? 1 : c->dims.n_plants, n = c->dims.n, m = c->dims.m;
    const mpcq::OpsLayout L = mpcq::OpsLayout::make(c->nc, c->mc);
    const char *what = "plant setup buffers";
    auto some = [what](auto &buf, size_t bytes) { return bytes ? buf.alloc(bytes, what) : MPCQ_OK; };
    int rc = some(c->d_P, 8 * Pg * n * n);
    if (rc || (rc = some(c->d_q0, 8 * Pg * n)) || (rc = some(c->d_A, 8 * Pg * m * n)) || (rc = some(c->d_l0, 8 * Pg * m)) ||
        (rc = some(c->d_u0, 8 * Pg * m)) || (rc = some(c->d_ops, 8 * Pg * L.total)) ||
        (rc = some(c->d_ops32, c->dims.dtype == MPCQ_F32 ? 4 * Pg * L.total : 0)) || (rc = some(c->d_ctype, 4 * Pg * c->mc)))
        return rc;
    return MPCQ_OK;
}

// Generic entry points that only need the device and the generic buffers (no setup yet)
int check_generic_dims(mpcq_ctx *c)
{
    int rc = check_ctx(c, kNone);
    if (rc) return rc;
    if (c->mimo_only) return fail(MPCQ_ERR_ARG, "n > 32 or m > 64 per plant: this context is served by mpcq_mimo_* only");
    return MPCQ_OK;
}

int h2d(void *dst, const void *src, size_t bytes, hipStream_t s)
{
    if (!bytes) return MPCQ_OK;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return MPCQ_OK;
}

int d2h(mpcq_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!dst || !bytes) return MPCQ_OK;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->last));
    HIPCHK(hipStreamSynchronize(c->last));
    return MPCQ_OK;
}

// True while s is under graph capture (or the query fails): nothing may synchronise it then.
bool stream_capturing(hipStream_t s)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
}

// The refusal of the entry points that take no stream under capture (include/mpcq.h)
int refuse_capture(const char *fn, hipStream_t s)
{
    if (!stream_capturing(s)) return MPCQ_OK;
    (void)hipGetLastError();
    return fail(MPCQ_ERR_ARG, std::string(fn) + ": the stream is under graph capture");
}

// What is enqueued on s from here on runs after the work on the context's last stream ...
int order_after_last(mpcq_ctx *c, hipStream_t s)
{
    if (s == c->last) return MPCQ_OK;
    if (!c->order_ev) HIPCHK(hipEventCreateWithFlags(&c->order_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->order_ev, c->last));
    HIPCHK(hipStreamWaitEvent(s, c->order_ev, 0));
    return MPCQ_OK;
}

// ... and the context's next launches on its last stream after what has been enqueued on s.
int order_last_after(mpcq_ctx *c, hipStream_t s)
{
    if (s == c->last) return MPCQ_OK;
    HIPCHK(hipEventRecord(c->order_ev, s));
    HIPCHK(hipStreamWaitEvent(c->last, c->order_ev, 0));
    return MPCQ_OK;
}

// d_q, d_u from the last tile-path controllerStep's saved X, U (mpcq_internal_front_end), once.
int materialize_qu(mpcq_ctx *c)
{
    if (!c->lazy.qu) return MPCQ_OK;
    c->lazy.qu = false;
    if (mpcq_internal_front_end((int)c->dims.batch, c->nx, (int)c->dims.n, (int)c->dims.m, c->d_Xs, c->d_Us,
                                c->lazy.xref, c->d_Fx, c->d_Fu, c->d_Fr, c->d_Sbar, c->d_Ku, c->d_W0, c->d_q,
                                c->d_u, c->last) != 0)
        return fail(MPCQ_ERR_HIP, "front-end kernel launch failed");
    return MPCQ_OK;
}

// d_x, d_y of the last tile solve from its stored warm state (mpcq_tile.h tile_publish_kernel), once.
int materialize_xy(mpcq_ctx *c)
{
    if (!c->lazy.xy) return MPCQ_OK;
    c->lazy.xy = false;
    int rc = materialize_info(c);  // (the publish kernel reads each QP's status)
    if (rc) return rc;
    auto publish = [c](auto a) {  // (a: the context's AdmmArgs<T>)
        a.img = (decltype(a.img))c->d_img;
        a.paired = c->paired && c->all_ineq && c->lower_free;
        return mpcq::launch_tile_publish(a, c->KN, c->KM, a.paired != 0, c->last);
    };
    rc = c->dims.dtype == MPCQ_F32 ? publish(make_args<float>(c)) : publish(make_args<double>(c));
    return rc ? fail(MPCQ_ERR_HIP, "solution publish kernel failed") : MPCQ_OK;
}

// d_rho of the last tile solve from its warm-state rho (fp64: the same value), once.
int materialize_rho(mpcq_ctx *c)
{
    if (!c->lazy.rho) return MPCQ_OK;
    c->lazy.rho = false;
    HIPCHK(hipMemcpyAsync(c->d_rho, c->d_rhos, 8 * (size_t)c->dims.batch, hipMemcpyDeviceToDevice, c->last));
    return MPCQ_OK;
}

// d_status, d_iter of the last ordered single-launch solve from its list-slot pairs, once.
int materialize_info(mpcq_ctx *c)
{
    if (!c->lazy.info) return MPCQ_OK;
    c->lazy.info = false;
    const int B = c->dims.batch;
    const int *list = c->d_ord + mpcq::OrderBins::kBins + B;
    if (mpcq_internal_order_info(B, list, list + B, c->d_status, c->d_iter, c->last) != 0)
        return fail(MPCQ_ERR_HIP, "status publish kernel failed");
    return MPCQ_OK;
}

extern "C" {

void mpcq_default_settings(mpcq_settings *s)
{
    if (!s) return;
    // osqp constants.h (v0.6) + osqp-eigen setWarmStart(true) (ModelPredictiveControlAPI.cpp:52)
    s->rho = 0.1;
    s->sigma = 1e-6;
    s->alpha = 1.6;
    s->eps_abs = 1e-3;
    s->eps_rel = 1e-3;
    s->eps_prim_inf = 1e-4;
    s->eps_dual_inf = 1e-4;
    s->adaptive_rho_tolerance = 5.0;
    s->adaptive_rho_fraction = 0.4;
    s->max_iter = 4000;
    s->check_termination = 25;
    s->scaling = 10;
    s->adaptive_rho = 1;
    s->adaptive_rho_interval = 0;
    s->warm_start = 1;
    s->scaled_termination = 0;
    s->verbose = 0;
    s->polish = 0;
    s->polish_refine_iter = 3;
    s->delta = 1e-6;
}

const char *mpcq_last_error(void) { return g_err.c_str(); }

int mpcq_create(const mpcq_dims *d, const mpcq_settings *s, mpcq_ctx **out)
{
    if (!d || !out) return fail(MPCQ_ERR_ARG, "null argument");
    *out = nullptr;
    if (d->n <= 0 || d->m < 0 || d->batch <= 0) return fail(MPCQ_ERR_ARG, "n > 0, m >= 0, batch > 0 required");
    if (d->n_plants != 1 && d->n_plants != d->batch) return fail(MPCQ_ERR_ARG, "n_plants must be 1 or batch");
    if (d->dtype != MPCQ_F64 && d->dtype != MPCQ_F32 && d->dtype != MPCQ_F64_MIXED) return fail(MPCQ_ERR_ARG, "dtype");
    mpcq_settings st;
    mpcq_default_settings(&st);
    if (s) st = *s;
    if (st.rho <= 0 || st.sigma <= 0 || st.alpha <= 0 || st.alpha >= 2 || st.max_iter <= 0 ||
        st.eps_abs < 0 || st.eps_rel < 0 || (st.eps_abs == 0 && st.eps_rel == 0) || st.scaling < 0 ||
        st.check_termination < 0 || st.adaptive_rho_tolerance < 1 || st.adaptive_rho_interval < 0 ||
        !(st.delta > 0) || st.polish_refine_iter < 0)
        return fail(MPCQ_ERR_ARG, "invalid settings (osqp validate_settings)");
    if (st.polish && (d->n > 32 || d->m > 64))
        return fail(MPCQ_ERR_ARG, "settings.polish serves n <= 32, m <= 64 (the polish kernel's capacities)");
    int nc = 0, mc = 0;
    const int KN = (d->n + 3) / 4, KM = (std::max(d->m, 1) + 3) / 4;
    const bool tile = d->n_plants == 1 && mpcq_internal_tile_supported(KN, KM) &&
                      std::strcmp(test_hook("MPCQ_KERNEL"), "lane") != 0;
    if (tile) {
        nc = 16 * ((KN + 3) / 4);
        mc = 16 * ((KM + 3) / 4);
    } else if (mpcq_internal_caps(d->n, std::max(d->m, 1), &nc, &mc) != 0) {
        // larger per-plant QPs: only the MIMO condensed-MPC path (mpcq_mimo_*) serves them
        if (!(d->n_plants == d->batch && d->n <= 128 && d->m == 2 * d->n && d->dtype != MPCQ_F32))
            return fail(MPCQ_ERR_ARG, "n/m exceed the compiled kernel capacities (n <= 32, m <= 64; the MIMO "
                                      "MPC path takes per-plant n <= 128, m = 2n, fp64)");
        nc = d->n;
        mc = d->m;
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= d->device || d->device < 0)
        return fail(MPCQ_ERR_HIP, "no HIP device with this ordinal");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, d->device) != hipSuccess)
        return fail(MPCQ_ERR_HIP, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MPCQ_ERR_HIP, std::string("device is ") + prop.gcnArchName + ", gfx950 required");
    HIPCHK(hipSetDevice(d->device));

    mpcq_ctx *c = new mpcq_ctx();
    c->dims = *d;
    c->set = st;
    c->nc = nc;
    c->mc = mc;
    c->cus = prop.multiProcessorCount;
    c->tile = tile;
    c->mimo_only = !tile && (d->n > 32 || d->m > 64);
    c->KN = KN;
    c->KM = KM;
    const mpcq::OpsLayout L = mpcq::OpsLayout::make(nc, mc);
    c->ops_stride = L.total;
    const size_t P = d->n_plants, B = d->batch, n = d->n, m = d->m;
    const size_t es = d->dtype == MPCQ_F32 ? 4 : 8;
    // a shared plant's setup arrays now; per-plant ones at the first setup (ensure_plant_buffers): a
    // one-pass context (mpcq_mpc_plants_step_device, ~1M plants on one GPU) never allocates them
    bool bad = (P == 1 && ensure_plant_buffers(c)) || c->d_setup_status.alloc(4 * P) || c->d_flags.alloc(4) ||
               c->d_q.alloc(8 * B * n) || c->d_u.alloc(8 * B * m) || c->d_l.alloc(8 * B * m) || c->d_x.alloc(8 * B * n) ||
               c->d_y.alloc(8 * B * m) || c->d_rho.alloc(8 * B) || c->d_status.alloc(4 * B) || c->d_iter.alloc(4 * B) ||
               c->d_xs.alloc(es * B * nc) || c->d_zs.alloc(es * B * mc) || c->d_ys.alloc(es * B * mc) ||
               c->d_rhos.alloc(es * B);
    if (tile) {
        const size_t lcap = (size_t)mpcq::ListSeg::kShards * mpcq::ListSeg::cap(B);  // entries per phase list
        bad = bad || c->d_img.alloc(es * mpcq::TileLayout::buffer(KN, KM, (int)(16 / es))) || c->d_list.alloc(4 * 2 * lcap) ||
              c->d_counts.alloc(4 * kMaxPhases * mpcq::ListSeg::kCounters) || c->d_itstate.alloc(4 * B);
    } else if (!c->mimo_only) {
        bad = bad || c->d_snx.alloc(es * B * nc) || c->d_sny.alloc(es * B * mc);
    }
    if (st.polish) bad = bad || c->d_pol_status.alloc(4 * B) || c->d_pol_nact.alloc(4 * B) || c->d_pol_res.alloc(8 * 2 * B);
    if (bad) {
        mpcq_destroy(c);
        return fail(MPCQ_ERR_HIP, "hipMalloc failed");
    }
    c->hD.assign(n, 1.0);
    c->hE.assign(m, 1.0);
    *out = c;
    return MPCQ_OK;
}

int mpcq_destroy(mpcq_ctx *c)
{
    if (!c) return MPCQ_OK;
    (void)hipSetDevice(c->dims.device);
    if (c->order_ev) (void)hipEventDestroy(c->order_ev);
    if (c->gexec) (void)hipGraphExecDestroy(c->gexec);
    if (c->graph) (void)hipGraphDestroy(c->graph);
    delete c;  // (its device buffers go with it)
    return MPCQ_OK;
}

int mpcq_get_solution(mpcq_ctx *c, double *x)
{
    int rc = check_ctx(c, kAnySetup);
    if (rc) return rc;
    if (!x) return fail(MPCQ_ERR_ARG, "null x");
    if ((rc = materialize_xy(c))) return rc;
    return d2h(c, x, c->d_x, 8 * (size_t)c->dims.batch * c->dims.n);
}

int mpcq_get_dual(mpcq_ctx *c, double *y)
{
    int rc = check_ctx(c, kAnySetup);
    if (rc) return rc;
    if (!y && c->dims.m) return fail(MPCQ_ERR_ARG, "null y");
    if ((rc = materialize_xy(c))) return rc;
    return d2h(c, y, c->d_y, 8 * (size_t)c->dims.batch * c->dims.m);
}

int mpcq_get_info(mpcq_ctx *c, int *status, int *iter, double *rho)
{
    int rc = check_ctx(c, kAnySetup);
    if (rc) return rc;
    const size_t B = c->dims.batch;
    if (rho && (rc = materialize_rho(c))) return rc;
    if ((status || iter) && (rc = materialize_info(c))) return rc;
    if ((rc = d2h(c, status, c->d_status, 4 * B))) return rc;
    if ((rc = d2h(c, iter, c->d_iter, 4 * B))) return rc;
    return d2h(c, rho, c->d_rho, 8 * B);
}

int mpcq_get_scaling(mpcq_ctx *c, double *D, double *E, double *cc)
{
    int rc = check_ctx(c, kGeneric);
    if (rc) return rc;
    if (D) std::copy(c->hD.begin(), c->hD.end(), D);
    if (E) std::copy(c->hE.begin(), c->hE.end(), E);
    if (cc) *cc = c->hc;
    return MPCQ_OK;
}

int mpcq_get_polish_info(mpcq_ctx *c, int *status_polish, int *n_active, double *pri_res, double *dua_res)
{
    int rc = check_ctx(c, kAnySetup);
    if (rc) return rc;
    const size_t B = c->dims.batch;
    if (!c->pol_valid) {  // not performed (set only by a polish launch: settings.polish, mpcq_mimo_step_polish_device)
        HIPCHK(hipStreamSynchronize(c->last));
        for (size_t b = 0; b < B; b++) {
            if (status_polish) status_polish[b] = 0;
            if (n_active) n_active[b] = 0;
            if (pri_res) pri_res[b] = std::nan("");
            if (dua_res) dua_res[b] = std::nan("");
        }
        return MPCQ_OK;
    }
    if ((rc = d2h(c, status_polish, c->d_pol_status, 4 * B)) || (rc = d2h(c, n_active, c->d_pol_nact, 4 * B))) return rc;
    if (pri_res || dua_res) {
        std::vector<double> res(2 * B);
        if ((rc = d2h(c, res.data(), c->d_pol_res, 8 * 2 * B))) return rc;
        for (size_t b = 0; b < B; b++) {
            if (pri_res) pri_res[b] = res[2 * b];
            if (dua_res) dua_res[b] = res[2 * b + 1];
        }
    }
    HIPCHK(hipStreamSynchronize(c->last));
    return MPCQ_OK;
}

int mpcq_get_stream_path(mpcq_ctx *c, int *kind)
{
    if (!c || !kind) return fail(MPCQ_ERR_ARG, "null argument");
    *kind = c->stream_path;
    return MPCQ_OK;
}

int mpcq_get_order(mpcq_ctx *c, int *ordered, int *order)
{
    if (!c || !ordered) return fail(MPCQ_ERR_ARG, "null argument");
    *ordered = c->lazy.ord ? 1 : 0;
    if (order) {
        const size_t B = c->dims.batch;
        if (!c->lazy.ord) {
            for (size_t i = 0; i < B; i++) order[i] = (int)i;
        } else {
            HIPCHK(hipMemcpyAsync(order, c->d_ord + mpcq::OrderBins::kBins + B, 4 * B, hipMemcpyDeviceToHost, c->last));
            HIPCHK(hipStreamSynchronize(c->last));
        }
    }
    return MPCQ_OK;
}

int mpcq_get_path(mpcq_ctx *c, int *kind, int *paired)
{
    if (!c) return fail(MPCQ_ERR_ARG, "null context");
    const PathChoice p = choose_path(c);
    if (kind) *kind = p.kind;
    if (paired) *paired = p.paired;
    return MPCQ_OK;
}

int mpcq_device_view_get(mpcq_ctx *c, mpcq_device_view *v)
{
    if (!c || !v) return fail(MPCQ_ERR_ARG, "null argument");
    int rc = materialize_qu(c);  // (enqueued on the context's last stream)
    if (rc || (rc = materialize_xy(c)) || (rc = materialize_rho(c)) || (rc = materialize_info(c))) return rc;
    v->q = c->d_q;
    v->u = c->d_u;
    v->l = c->d_l;
    v->x = c->d_x;
    v->y = c->d_y;
    v->status = c->d_status;
    v->iter = c->d_iter;
    v->rho = c->d_rho;
    return MPCQ_OK;
}

}  // extern "C"

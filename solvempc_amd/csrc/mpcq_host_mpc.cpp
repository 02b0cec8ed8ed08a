// solvempc_amd/csrc/mpcq_host_mpc.cpp — host side of the C ABI declared in include/mpcq.h: the MPC front end's
// operators, the control step and the receding-horizon stream.
#include "mpcq_ctx.h"

// Device buffers of the MPC front-end operators for nx states (per plant) and X/U staging.
int alloc_mpc_ops(mpcq_ctx *c, int nx)
{
    const size_t Pn = c->dims.n_plants, n = c->dims.n, m = c->dims.m, B = c->dims.batch;
    if (c->nx != nx) {
        c->gen++;
        c->d_Fx.release();
        c->d_Sbar.release();
        c->d_X.release();
        c->d_Xs.release();
    }
    int rc = c->d_Fx.alloc(8 * Pn * n * nx);
    if (rc || (rc = c->d_Fu.alloc(8 * Pn * n)) || (rc = c->d_Fr.alloc(8 * Pn * n * n)) ||
        (rc = c->d_Sbar.alloc(8 * Pn * m * nx)) || (rc = c->d_Ku.alloc(8 * Pn * m)) || (rc = c->d_W0.alloc(8 * Pn * m)) ||
        (rc = c->d_X.alloc(8 * B * nx)) || (rc = c->d_U.alloc(8 * B)) || (rc = c->d_Xs.alloc(8 * B * nx)) ||
        (rc = c->d_Us.alloc(8 * B)))
        return rc;
    return MPCQ_OK;
}

namespace {

// The call in progress runs with per-QP references: launch_typed / launch_stream / launch_tile_stream read
// c->cur_ref, which is the scalar xref again when the call returns.
struct RefScope {
    mpcq_ctx *c;
    RefScope(mpcq_ctx *cc, const mpcq::RefArgs &r) : c(cc) { c->cur_ref = r; }
    ~RefScope() { c->cur_ref = mpcq::RefArgs{}; }
};

// The refusals the mpcq_mpc_step* entry points share, in their order (have_xu: X and U are both given)
int step_check(mpcq_ctx *c, bool have_xu)
{
    int rc = check_ctx(c, kGeneric);
    if (rc) return rc;
    if (!c->mpc_ready) return fail(MPCQ_ERR_ORDER, "mpcq_mpc_set_operators has not been called");
    if (!have_xu) return fail(MPCQ_ERR_ARG, "null X/U");
    return MPCQ_OK;
}

// ... and those of the forms with per-QP references
int step_ref_check(mpcq_ctx *c, bool have_xu, const double *ref, long long ref_stride)
{
    int rc = step_check(c, have_xu);
    if (rc) return rc;
    if (!ref) return fail(MPCQ_ERR_ARG, "null ref");
    if (ref_stride != 0 && ref_stride < c->dims.n) return fail(MPCQ_ERR_ARG, "ref_stride must be 0 or >= n");
    return MPCQ_OK;
}

// The stream in one launch (stream_wave_kernel, mpcq_wave.h): the one-QP-per-wave path's control
// steps with the plant update between them, no per-step launches or graph.
template <typename T>
int launch_stream(mpcq_ctx *c, hipStream_t s, double *X, double *U, double xref, const mpcq::StreamArgs &sa,
                         const mpcq::LogArgs *lg)
{
    c->lazy.clear_results();  // (the stream writes every QP's x, y, rho, status and iter at its last step)
    auto a = make_args<T>(c);
    set_mpc_front_end(c, a, X, U, xref);
    a.q_out = c->d_q; a.u_out = c->d_u;
    // (a reference schedule, c->cur_ref: the REF variant slides the window with the step)
    a.stop_iter = c->set.max_iter;
    c->lazy.qu = false;
    // (a record is attached, lg: the REF + LOG variant; a scalar run: the one-entry schedule [xref], mpc_run)
    return mpcq::launch_wave_stream(a, c->nc, c->mc, sa, c->cur_ref.p ? &c->cur_ref : nullptr, lg, s);
}

// The stream in one tile launch (admm_tile_kernel STREAM mode): every MFMA column is one plant that runs
// all its control steps, a wave holding `cpw` plants.  A control step of a column never waits for the
// others', so a wave lives as long as its slowest plant's iterations summed over the steps (not the
// per-step maximum over the batch); with a few thousand plants the chip is latency-bound, so cpw is
// chosen to spread the plants over every SIMD (MPCQ_STREAM_CPW: A/B).  Needs adapt_rho and max_iter
// on check iterations (multiples of check_termination, as OSQP's defaults are).
template <typename T>
int launch_tile_stream(mpcq_ctx *c, hipStream_t s, double *X, double *U, double xref, mpcq::StreamArgs sa,
                              const mpcq::LogArgs *lg)
{
    c->lazy.clear_results();  // (the stream writes every QP's x, y, rho, status and iter at its last step)
    const mpcq_settings &st = c->set;
    const int ct = st.check_termination;
    auto a = make_args<T>(c);
    if (ct <= 0 || st.max_iter % ct || (st.adaptive_rho && a.adaptive_interval % ct)) return -1;
    const char *e = test_hook("MPCQ_STREAM_CPW");
    const long simds = (long)c->cus * 4;
    // plants per wave: one wave per SIMD (f32, 4 at 4,096 plants), twice that for fp64 / mixed, whose waves
    // measured faster at half the SIMDs (config 5: cpw 4 103.7 M QP/s, 6-16 105.5-106.3 M, r04w_*)
    const long per = ((long)c->dims.batch + simds - 1) / simds * (c->dims.dtype == MPCQ_F32 ? 1 : 2);
    sa.cpw = *e ? std::max(1, std::min(16, std::atoi(e))) : (int)std::max<long>(1, std::min<long>(16, per));
    // the kernel compiled for two waves per SIMD (its plant and check code spill outside the hot loop); the
    // variant compiled for one (no spills, MFMA accumulators in AGPRs) measured 2 % slower at config 5
    // (103.7 against 106.0 M QP/s, profiles/r05h_cfg5_occ_ab.jsonl): test hook MPCQ_STREAM_OCC=1 for A/B,
    // taken only when the waves fit one per SIMD
    const long waves = ((long)c->dims.batch + sa.cpw - 1) / sa.cpw;
    sa.occ = (waves <= simds && test_hook("MPCQ_STREAM_OCC")[0] == '1') ? 1 : 2;
    set_mpc_front_end(c, a, X, U, xref);
    a.X_save = c->d_Xs; a.U_save = c->d_Us;  // the last step's X, U: its q, u on demand (materialize_qu)
    if (c->cur_ref.p) {  // a reference schedule: the last step's q, u themselves (its window is not kept)
        a.X_save = a.U_save = nullptr;
        a.q_out = c->d_q; a.u_out = c->d_u;
    }
    a.paired = 1;
    a.img = (const T *)c->d_img;
    a.stop_iter = INT_MAX;
    a.sim = sa;
    // debug build: per-wave stage stamps of the launch (tools/stamps.py format, one phase), written to
    // $MPCQ_TILE_STAMPS after it
    const char *stp = debug_hook("MPCQ_TILE_STAMPS");
    const size_t swaves = (size_t)waves + 8;  // (+ a workgroup's idle waves)
    if (stp && *stp) {
        c->d_stamps.release();
        if (c->d_stamps.alloc(8 * 8 * swaves) != MPCQ_OK || hipMemsetAsync(c->d_stamps, 0, 8 * 8 * swaves, s) != hipSuccess)
            return -2;
        a.stamps = c->d_stamps;
    }
    // (a reference schedule: the REF variant; a record is attached, lg: the scalar or the REF kernel's LOG variant)
    const int rc = mpcq::launch_tile_stream(a, c->KN, c->KM, c->cur_ref.p ? &c->cur_ref : nullptr, lg, s);
    if (rc == 0 && stp && *stp) {
        if (dump_tile_stamps(stp, c->d_stamps, 1, swaves, s)) return -2;
        c->d_stamps.release();
    }
    if (rc == 0) {
        c->lazy.qu = !c->cur_ref.p;
        c->lazy.xref = xref;
    }
    return rc;
}

// mpcq_mpc_run_device (sched == null: the scalar xref) and mpcq_mpc_run_ref_device (the schedule sched_dev,
// sched_len, sched_stride in place of xref).
int mpc_run(mpcq_ctx *c, const char *fn, double *X, double *U, double xref, const double *sched, int sched_len,
                   long long sched_stride, int steps, unsigned long long seed, long long first_qp, long long first_step,
                   double noise_std, void *stream)
{
    int rc = check_ctx(c, kGeneric);
    if (rc) return rc;
    if (c->set.polish) return fail(MPCQ_ERR_ARG, polish_refusal(fn));
    if (!c->mpc_ready || !c->plant_nx) return fail(MPCQ_ERR_ORDER, "mpc operators / plant not set");
    if (c->plant_nx != c->nx) return fail(MPCQ_ERR_ARG, "plant nx differs from the operators' nx");
    if (!X || !U || steps < 0) return fail(MPCQ_ERR_ARG, "null X/U or steps < 0");
    if (!stream) return fail(MPCQ_ERR_ARG, "graph capture needs a non-NULL stream");
    hipStream_t s = (hipStream_t)stream;
    // an attached record (mpcq_mpc_set_stream_log): every row of this run must lie in its buffers, checked before
    // anything is enqueued.  The one-launch kernels index the rows from first_step themselves (lg_launch), the
    // per-step launches from the device step counter (lg_graph), as with the reference window below.
    const bool logged = c->slog_on && steps > 0;
    mpcq::LogArgs lg_launch{}, lg_graph{};
    if (logged) {
        const mpcq_stream_log &L = c->slog;
        if (first_step < L.step0 || first_step - L.step0 > L.rows - steps)
            return fail(MPCQ_ERR_ARG, std::string(fn) + ": control steps outside the attached stream log's rows");
        lg_launch = mpcq::LogArgs{L.U, L.X, L.status, L.iter, first_step - L.step0, nullptr, c->dims.batch};
        lg_graph = mpcq::LogArgs{L.U, L.X, L.status, L.iter, -L.step0, c->d_step, c->dims.batch};
        if (!sched && (rc = c->d_logref.alloc(8))) return rc;
    }
    const mpcq::LogArgs *const lgp = logged ? &lg_launch : nullptr;
    // the one-launch kernels slide the window from first_step themselves; the per-step launches (eager first
    // step, captured graph) take the step from the device counter, as the captured plant simulation does
    mpcq::RefArgs ref_launch{}, ref_graph{};
    if (sched) {
        ref_launch = mpcq::RefArgs{sched, sched_stride, first_step, nullptr, sched_len};
        ref_graph = mpcq::RefArgs{sched, sched_stride, 0, c->d_step, sched_len};
    }
    RefScope scope(c, ref_launch);
    HIPCHK(hipMemsetAsync(c->d_it_acc, 0, 4 * (size_t)c->dims.batch, s));
    HIPCHK(hipMemsetAsync(c->d_uns_acc, 0, 4 * (size_t)c->dims.batch, s));
    if (steps == 0) return MPCQ_OK;
    struct Acc {  // this call's launches (eager and captured) accumulate the stream counters
        mpcq_ctx *c;
        explicit Acc(mpcq_ctx *cc) : c(cc) { c->stream_acc = true; }
        ~Acc() { c->stream_acc = false; }
    } acc(c);
    c->sens_ok = false;  // (the warm state becomes the stream's last step's)
    if (mpcq_internal_set_step(c->d_step, first_step, s)) return fail(MPCQ_ERR_HIP, "set_step launch failed");
    const bool sync_each = debug_hook("MPCQ_DEBUG_SYNC")[0] == '1';  // synchronise every stage
    auto stage = [&](const char *what) -> int {
        if (!sync_each) return MPCQ_OK;
        const hipError_t e = hipStreamSynchronize(s);
        return e == hipSuccess ? MPCQ_OK : fail(MPCQ_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    };
    if ((rc = stage("set_step"))) return rc;
    // one launch for the whole stream: the tile kernel's stream mode for a shared plant of the paired
    // condensed-MPC shape, else one QP per wave (per-plant batches); MPCQ_STREAM=graph: the per-step
    // hipGraph below, MPCQ_STREAM=wave: the one-QP-per-wave launch (A/B and test cross-checks)
    const char *smode = test_hook("MPCQ_STREAM");
    const bool tile_ok = c->tile && c->paired && c->all_ineq && c->lower_free && c->d_Xs && c->d_Us &&
                         std::strcmp(smode, "graph") != 0 && std::strcmp(smode, "wave") != 0 &&
                         std::strcmp(test_hook("MPCQ_KERNEL"), "wave") != 0 && std::strcmp(test_hook("MPCQ_KERNEL"), "lane") != 0;
    if (tile_ok) {
        const mpcq::StreamArgs sa{steps, c->nx, c->dims.n_plants == 1, 0, c->d_Ad, c->d_Bd, seed, first_qp, first_step,
                                  noise_std};
        const int lrc = c->dims.dtype == MPCQ_F32 ? launch_tile_stream<float>(c, s, X, U, xref, sa, lgp)
                                                  : launch_tile_stream<double>(c, s, X, U, xref, sa, lgp);
        if (lrc == -2) return fail(MPCQ_ERR_HIP, std::string("tile stream launch failed: ") + hipGetErrorString(hipGetLastError()));
        if (lrc == 0) {
            if (mpcq_internal_set_step(c->d_step, first_step + steps, s)) return fail(MPCQ_ERR_HIP, "set_step launch failed");
            c->fresh = false;
            c->have_xy = true;  // (the stream's last step wrote d_x, d_y)
            c->last = s;
            c->stream_path = MPCQ_STREAM_TILE;
            return stage("tile stream kernel");
        }
    }
    if (choose_path(c).kind == MPCQ_PATH_WAVE && c->dims.n <= 32 && c->dims.m <= 64 &&
        std::strcmp(smode, "graph") != 0) {
        const mpcq::StreamArgs sa{steps, c->nx, c->dims.n_plants == 1, 1, c->d_Ad, c->d_Bd, seed, first_qp, first_step,
                                  noise_std};
        if (logged && !sched) {
            // a logged scalar run: the wave stream has the REF kernel's LOG variant only, handed the shared
            // one-entry schedule [xref] (a uniform reference reproduces the scalar path bit for bit)
            if (mpcq_internal_fill(c->d_logref, 0, xref, 1, s)) return fail(MPCQ_ERR_HIP, "fill launch failed");
            c->cur_ref = mpcq::RefArgs{c->d_logref, 0, first_step, nullptr, 1};
        }
        const int lrc = c->dims.dtype == MPCQ_F32 ? launch_stream<float>(c, s, X, U, xref, sa, lgp)
                                                  : launch_stream<double>(c, s, X, U, xref, sa, lgp);
        if (lrc) return fail(MPCQ_ERR_HIP, std::string("stream kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
        if (mpcq_internal_set_step(c->d_step, first_step + steps, s)) return fail(MPCQ_ERR_HIP, "set_step launch failed");
        c->fresh = false;
        c->have_xy = true;  // (the stream's last step wrote d_x, d_y)
        c->last = s;
        c->stream_path = MPCQ_STREAM_WAVE;
        return stage("stream kernel");
    }
    int done = 0;
    c->stream_path = MPCQ_STREAM_GRAPH;
    c->cur_ref = ref_graph;
    // the record's row of a per-step launch, after its plant update and ahead of the counter's tick: the kernel
    // reads the published status, iter, so an ordered tile solve's list-slot pairs are permuted first
    // (materialize_info, on the same stream: captured with the step)
    auto log_row = [&]() -> int {
        if (!logged) return MPCQ_OK;
        if (int mrc = materialize_info(c)) return mrc;
        if (mpcq_internal_log_row(c->nx, X, U, c->d_status, c->d_iter, &lg_graph, s))
            return fail(MPCQ_ERR_HIP, "stream log kernel launch failed");
        return MPCQ_OK;
    };
    if (c->fresh) {  // a reset is a one-off (x = z = y = 0): run that step eagerly, capture the rest
        if ((rc = launch_solve(c, s, true, X, U, xref))) return rc;
        if (mpcq_internal_simulate(c->dims.batch, c->nx, c->dims.n_plants == 1, c->d_Ad, c->d_Bd, X, U, seed,
                                   first_qp, c->d_step, 0, noise_std, s))
            return fail(MPCQ_ERR_HIP, "simulate kernel launch failed");
        if ((rc = log_row())) return rc;
        if (mpcq_internal_tick(c->d_step, s)) return fail(MPCQ_ERR_HIP, "simulate kernel launch failed");
        done = 1;
        if ((rc = stage("eager first step"))) return rc;
    }
    const bool same = c->gexec && c->gkey.X == X && c->gkey.U == U && c->gkey.xref == xref &&
                      c->gkey.noise == noise_std && c->gkey.seed == seed && c->gkey.first_qp == first_qp &&
                      c->gkey.s == s && c->gkey.gen == c->gen && c->gkey.sched == sched &&
                      (!sched || (c->gkey.sched_len == sched_len && c->gkey.sched_stride == sched_stride));
    if (!same && done < steps) {
        if (c->gexec) { (void)hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
        if (c->graph) { (void)hipGraphDestroy(c->graph); c->graph = nullptr; }
        HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        int lrc = launch_solve(c, s, true, X, U, xref);
        if (!lrc && mpcq_internal_simulate(c->dims.batch, c->nx, c->dims.n_plants == 1, c->d_Ad, c->d_Bd, X, U,
                                           seed, first_qp, c->d_step, 0, noise_std, s))
            lrc = fail(MPCQ_ERR_HIP, "simulate kernel launch failed");
        if (!lrc) lrc = log_row();
        if (!lrc && mpcq_internal_tick(c->d_step, s)) lrc = fail(MPCQ_ERR_HIP, "simulate kernel launch failed");
        hipGraph_t g = nullptr;
        const hipError_t ec = hipStreamEndCapture(s, &g);
        // a discarded capture ran none of its launches: the phase-list counters are not known clean
        if (lrc || ec != hipSuccess) c->count0_clean = false;
        if (lrc) { if (g) (void)hipGraphDestroy(g); return lrc; }
        if (ec != hipSuccess) return fail(MPCQ_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ec));
        c->graph = g;
        const hipError_t ei = hipGraphInstantiate(&c->gexec, c->graph, nullptr, nullptr, 0);
        if (ei != hipSuccess) {
            c->count0_clean = false;
            c->gexec = nullptr;
            return fail(MPCQ_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
        }
        c->gkey = {X, U, xref, noise_std, seed, first_qp, s, c->gen, sched, sched_len, sched_stride};
        c->glazy = c->lazy;
    }
    for (int k = done; k < steps; k++) {
        const auto t0 = std::chrono::steady_clock::now();
        HIPCHK(hipGraphLaunch(c->gexec, s));
        c->lazy = c->glazy;
        if (sync_each && (rc = stage(("graph replay " + std::to_string(k)).c_str()))) return rc;
        if (c->set.verbose) {  // (the captured solve printed nothing: launch_solve)
            HIPCHK(hipStreamSynchronize(s));
            c->last = s;
            verbose_solve(c, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
    }
    c->last = s;
    return MPCQ_OK;
}

}  // namespace

extern "C" {

int mpcq_mpc_set_operators(mpcq_ctx *c, int nx, const double *Fx, const double *Fu, const double *Fr,
                           const double *Sbar, const double *Ku, const double *W0)
{
    int rc = check_generic_dims(c);
    if (rc) return rc;
    const size_t Pn = c->dims.n_plants, n = c->dims.n, m = c->dims.m;
    if (nx <= 0 || nx > 8) return fail(MPCQ_ERR_ARG, "nx must be in 1..8");
    if (m != 2 * n) return fail(MPCQ_ERR_ARG, "MPC front end needs m == 2n (ModelPredictiveControlAPI.cpp:47-48)");
    if (!Fx || !Fu || !Fr || !Sbar || !Ku || !W0) return fail(MPCQ_ERR_ARG, "null operator");
    if ((rc = materialize_qu(c))) return rc;  // (with the operators the pending step used)
    if ((rc = alloc_mpc_ops(c, nx))) return rc;
    c->nx = nx;
    c->sens_ok = false;  // (the last step's q, u came from the operators being replaced)
    hipStream_t s = c->last;
    if ((rc = h2d(c->d_Fx, Fx, 8 * Pn * n * nx, s)) || (rc = h2d(c->d_Fu, Fu, 8 * Pn * n, s)) ||
        (rc = h2d(c->d_Fr, Fr, 8 * Pn * n * n, s)) || (rc = h2d(c->d_Sbar, Sbar, 8 * Pn * m * nx, s)) ||
        (rc = h2d(c->d_Ku, Ku, 8 * Pn * m, s)) || (rc = h2d(c->d_W0, W0, 8 * Pn * m, s)))
        return rc;
    c->mpc_ready = true;
    return build_order_map(c);
}

int mpcq_mpc_step_device(mpcq_ctx *c, const double *X, double *U, double xref, void *stream)
{
    int rc = step_check(c, X && U);
    if (rc) return rc;
    return launch_solve(c, (hipStream_t)stream, true, X, U, xref);
}

int mpcq_mpc_step(mpcq_ctx *c, const double *X, double *U, double xref)
{
    int rc = step_check(c, true);  // (null X, U: the copies below report them)
    if (rc) return rc;
    const size_t B = c->dims.batch;
    if ((rc = h2d(c->d_X, X, 8 * B * c->nx, c->last)) || (rc = h2d(c->d_U, U, 8 * B, c->last))) return rc;
    if ((rc = launch_solve(c, c->last, true, c->d_X, c->d_U, xref))) return rc;
    return d2h(c, U, c->d_U, 8 * B);
}

int mpcq_mpc_step_ref_device(mpcq_ctx *c, const double *X, double *U, const double *ref, long long ref_stride,
                             void *stream)
{
    int rc = step_ref_check(c, X && U, ref, ref_stride);
    if (rc) return rc;
    RefScope scope(c, mpcq::RefArgs{ref, ref_stride, 0, nullptr, c->dims.n});
    return launch_solve(c, (hipStream_t)stream, true, X, U, 0.0);
}

int mpcq_mpc_step_ref(mpcq_ctx *c, const double *X, double *U, const double *ref, long long ref_stride)
{
    int rc = step_ref_check(c, X && U, ref, ref_stride);
    if (rc) return rc;
    const size_t B = c->dims.batch, n = c->dims.n;
    // the staged copy is packed: B rows of n (or the one shared row)
    const size_t rows = ref_stride ? B : 1;
    if (c->d_ref.cap() < 8 * rows * n && (rc = materialize_qu(c))) return rc;
    if ((rc = c->d_ref.grow(8 * rows * n, c->last))) return rc;  // (no solve still reads a buffer it frees)
    if (ref_stride == 0 || ref_stride == (long long)n) {
        if ((rc = h2d(c->d_ref, ref, 8 * rows * n, c->last))) return rc;
    } else {
        HIPCHK(hipMemcpy2DAsync(c->d_ref, 8 * n, ref, 8 * (size_t)ref_stride, 8 * n, rows, hipMemcpyHostToDevice, c->last));
        HIPCHK(hipStreamSynchronize(c->last));
    }
    if ((rc = h2d(c->d_X, X, 8 * B * c->nx, c->last)) || (rc = h2d(c->d_U, U, 8 * B, c->last))) return rc;
    RefScope scope(c, mpcq::RefArgs{c->d_ref, ref_stride ? (long long)n : 0, 0, nullptr, (int)n});
    if ((rc = launch_solve(c, c->last, true, c->d_X, c->d_U, 0.0))) return rc;
    return d2h(c, U, c->d_U, 8 * B);
}

int mpcq_mpc_set_plant(mpcq_ctx *c, int nx, const double *Ad, const double *Bd)
{
    int rc = check_generic_dims(c);
    if (rc) return rc;
    if (nx <= 0 || nx > 8 || !Ad || !Bd) return fail(MPCQ_ERR_ARG, "set_plant: 1 <= nx <= 8 and Ad, Bd required");
    const size_t Pn = c->dims.n_plants;
    if (c->plant_nx != nx) {
        c->gen++;
        c->d_Ad.release();
        c->d_Bd.release();
    }
    if (!c->d_it_acc) c->gen++;  // (the counters are baked into captured graphs)
    if ((rc = c->d_Ad.alloc(8 * Pn * nx * nx)) || (rc = c->d_Bd.alloc(8 * Pn * nx)) || (rc = c->d_step.alloc(8)) ||
        (rc = c->d_it_acc.alloc(4 * (size_t)c->dims.batch)) || (rc = c->d_uns_acc.alloc(4 * (size_t)c->dims.batch)))
        return rc;
    c->plant_nx = nx;
    if ((rc = h2d(c->d_Ad, Ad, 8 * Pn * nx * nx, c->last)) || (rc = h2d(c->d_Bd, Bd, 8 * Pn * nx, c->last))) return rc;
    return MPCQ_OK;
}

int mpcq_mpc_stream_counters(mpcq_ctx *c, int *iters, int *unsolved)
{
    int rc = check_ctx(c, kGeneric);
    if (rc) return rc;
    if (!c->d_it_acc) return fail(MPCQ_ERR_ORDER, "mpcq_mpc_set_plant has not been called");
    const size_t B = c->dims.batch;
    if ((rc = d2h(c, iters, c->d_it_acc, 4 * B))) return rc;
    return d2h(c, unsolved, c->d_uns_acc, 4 * B);
}

int mpcq_mpc_set_stream_log(mpcq_ctx *c, const mpcq_stream_log *log)
{
    if (!c) return fail(MPCQ_ERR_ARG, "null context");
    const bool on = log && (log->U || log->X || log->status || log->iter);
    if (on && (log->rows < 1 || log->step0 < 0)) return fail(MPCQ_ERR_ARG, "stream log: rows >= 1 and step0 >= 0 required");
    if (on || c->slog_on) c->gen++;  // (the record kernel and its buffers are baked into a captured graph)
    c->slog = on ? *log : mpcq_stream_log{};
    c->slog_on = on;
    return MPCQ_OK;
}

int mpcq_mpc_simulate_device(mpcq_ctx *c, double *X, const double *U, unsigned long long seed, long long first_qp,
                             long long step, double noise_std, void *stream)
{
    int rc = check_generic_dims(c);
    if (rc) return rc;
    if (!c->plant_nx) return fail(MPCQ_ERR_ORDER, "mpcq_mpc_set_plant has not been called");
    if (!X || !U) return fail(MPCQ_ERR_ARG, "null X/U");
    if (mpcq_internal_simulate(c->dims.batch, c->plant_nx, c->dims.n_plants == 1, c->d_Ad, c->d_Bd, X, U, seed,
                               first_qp, nullptr, step, noise_std, (hipStream_t)stream))
        return fail(MPCQ_ERR_HIP, "simulate kernel launch failed");
    c->last = (hipStream_t)stream;
    return MPCQ_OK;
}

int mpcq_mpc_run_device(mpcq_ctx *c, double *X, double *U, double xref, int steps, unsigned long long seed,
                        long long first_qp, long long first_step, double noise_std, void *stream)
{
    return mpc_run(c, "mpcq_mpc_run_device", X, U, xref, nullptr, 0, 0, steps, seed, first_qp, first_step, noise_std,
                   stream);
}

int mpcq_mpc_run_ref_device(mpcq_ctx *c, double *X, double *U, const double *sched, int sched_len,
                            long long sched_stride, int steps, unsigned long long seed, long long first_qp,
                            long long first_step, double noise_std, void *stream)
{
    if (!c) return fail(MPCQ_ERR_ARG, "null context");
    if (!sched) return fail(MPCQ_ERR_ARG, "null schedule");
    if (sched_len < 1) return fail(MPCQ_ERR_ARG, "sched_len must be >= 1");
    if (sched_stride != 0 && sched_stride < sched_len) return fail(MPCQ_ERR_ARG, "sched_stride must be 0 or >= sched_len");
    if (first_step < 0) return fail(MPCQ_ERR_ARG, "first_step must be >= 0");
    return mpc_run(c, "mpcq_mpc_run_ref_device", X, U, 0.0, sched, sched_len, sched_stride, steps, seed, first_qp,
                   first_step, noise_std, stream);
}

}  // extern "C"

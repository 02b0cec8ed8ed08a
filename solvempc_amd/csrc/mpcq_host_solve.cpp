// solvempc_amd/csrc/mpcq_host_solve.cpp — host side of the C ABI declared in include/mpcq.h: the launch surface of
// a solve (kernel path, phase chain, polish, verbose output).
#include "mpcq_ctx.h"

namespace {

template <typename T>
void fill_ops(mpcq::PlantOps<T> &op, const T *base, const mpcq::OpsLayout &L, const int *ctype)
{
    op.lam = base + L.lam;
    op.W = base + L.W;
    op.sWtW = base + L.sWtW;
    op.WtA = base + L.WtA;
    op.PW = base + L.PW;
    op.Winv = base + L.Winv;
    op.Ah = base + L.Ah;
    op.D = base + L.D;
    op.E = base + L.E;
    op.Dinv = base + L.Dinv;
    op.Einv = base + L.Einv;
    op.cs = base + L.cs;
    op.rscale = base + L.rscale;
    op.ctype = ctype;
}

// Phase boundaries of the tile path (multiples of check_termination, then max_iter): QPs still
// running at a boundary are re-packed densely into the waves of the next launch.  Default: stops at
// 4 and 5 check_termination (100 and 125 iterations at the defaults), then the QPs that need more
// (the ~tens of the long tail) finish on the one-QP-per-wave kernel: each runs on its own SIMD at
// ~0.7 us per iteration, where a tile wave holding them runs at its slowest column's pace, ~0.9 us
// per lone-wave iteration (config 2: 347-350 us per solve against 368-371 us for [100, max_iter] on
// tile waves).  When the batch is more than ~1.5 rounds of the chip's tile-wave slots the
// chain is 3, 4 check_termination and max_iter on tile waves, where the re-pack at 75 pays; a tile
// chain forced onto a batch under 8,192 QPs (MPCQ_KERNEL=tile; the default there is the wave kernel)
// stops at 4 check_termination and runs the rest on tile waves.
// *wave_tail: the last launch runs on the wave kernel (test hooks MPCQ_PHASES, MPCQ_TAIL=wave|tile).
constexpr bool kWaveTail = false;  // [100, 125] + wave tail: slower in round 4 (tile tail f32 +2.4 %, mixed +8 %)
// ordered (phase 0 in hardest-first order, mpcq_order.hip): one launch per solve.  Its waves hold QPs of
// like difficulty, so a re-pack saves little, and the slow QPs start first instead of waiting for a
// later phase (config 2 mixed, one box: 0.335 ms against 0.406-0.416 ms for the same order with stops at
// 100 or 125 and 0.446-0.474 ms in index order, profiles/r05a_order_mixed.log).
int phase_stops(const mpcq_settings &st, int batch, int cus, int *stops, bool *wave_tail, bool ordered = false)
{
    const int ct = st.check_termination;
    int np = 0;
    const char *e = test_hook("MPCQ_PHASES");  // "0" = one launch per solve, or check multiples "3,4,5"
    const char *t = test_hook("MPCQ_TAIL");
    const bool many = (long)batch / 16 > (long)cus * 4 * 3 * 3 / 2;  // waves vs 3 waves/SIMD, 4 SIMD/CU
    int mult[kMaxPhases] = {3, 4};
    int nm = 2;
    *wave_tail = false;
    if (ordered) {
        nm = 0;
    } else if (!many && batch < 8192) {  // (a tile chain forced onto a small batch: one stop, tile waves)
        mult[0] = 4;
        nm = 1;
    } else if (!many) {
        mult[0] = 4;
        mult[1] = 5;
        *wave_tail = kWaveTail;
        if (!kWaveTail) nm = 1;
    }
    const int cap = kMaxPhases;
    if (e[0] == '0') nm = 0;
    else if (*e) {
        nm = 0;
        *wave_tail = false;
        for (const char *p = e; *p && nm < cap - 1;) {
            mult[nm++] = std::atoi(p);
            while (*p && *p != ',') p++;
            if (*p == ',') p++;
        }
    }
    if (t[0] == 'w') {  // test hook: [100, 125] (or the MPCQ_PHASES list) + wave tail
        if (!*e && !many && batch >= 8192) {
            mult[1] = 5;
            nm = 2;
        }
        *wave_tail = true;
    }
    if (t[0] == 't') *wave_tail = false;
    if (ct > 0) {
        for (int i = 0; i < nm; i++) {
            const long it = (long)mult[i] * ct;
            if (it >= st.max_iter || np >= cap - 1) break;
            if (np && it <= stops[np - 1]) continue;
            stops[np++] = (int)it;
        }
    }
    stops[np++] = st.max_iter;
    if (np < 2) *wave_tail = false;  // (phase 0 stays on tile waves)
    return np;
}

const char *env_kernel() { return test_hook("MPCQ_KERNEL"); }

template <typename T>
int wave_launch(mpcq_ctx *c, const mpcq::AdmmArgs<T> &a, int grid, hipStream_t s)
{
    // (the reference: for an MPC front end with per-QP references, the REF variant)
    return mpcq::launch_wave(a, c->nc, c->mc, grid, c->cur_ref.p && a.mpc ? &c->cur_ref : nullptr, s);
}

// The phase chain of a tile solve on stream s: phase p's QPs still running at its stop are appended to
// the ListSeg list of phase p + 1 (two alternating lists; each phase its own block of counters).
template <typename T>
int launch_phases(mpcq_ctx *c, mpcq::AdmmArgs<T> &a, hipStream_t s, bool wave_only)
{
    const int B = c->dims.batch;
    int stops[kMaxPhases];
    bool wave_tail = false;
    // an MPC step on the tile waves runs its batch hardest-first (mpcq_order.hip; test hook MPCQ_ORDER=0:
    // index order)
    // (a step with per-QP references: the key's G ref_b term needs the folded G, build_order_map)
    const bool ordered = a.mpc && a.X && a.U && c->ord_ok && !wave_only && test_hook("MPCQ_ORDER")[0] != '0' &&
                         (!c->cur_ref.p || c->ordG_ok);
    const int np = phase_stops(c->set, B, c->cus, stops, &wave_tail, ordered);
    c->lazy.ord = ordered;
    int *const ord_cnt = c->d_ord, *const ord_key = c->d_ord + mpcq::OrderBins::kBins, *const ord_list = ord_key + B;
    if (ordered) {
        // the counters are zero unless the last ordered sort's tile launch did not run (it clears them)
        if (!c->ord_clean && hipMemsetAsync(ord_cnt, 0, 4 * (size_t)mpcq::OrderBins::kBins, s) != hipSuccess) return -2;
        c->ord_clean = false;
        if (c->cur_ref.p) {
            if (mpcq_internal_order_ref(B, c->nx, c->dims.n, c->dims.m, a.X, a.U, c->d_ordmap, c->d_ordG, &c->cur_ref, ord_cnt,
                                        ord_key, ord_list, a.X_save, a.U_save, s) != 0)
                return -2;
        } else if (mpcq_internal_order(B, c->nx, c->dims.m, a.X, a.U, c->d_ordmap, a.xref, ord_cnt, ord_key, ord_list,
                                       a.X_save, a.U_save, s) != 0)
            return -2;
    }
    // (an ordered step's X, U copies are the order kernel's: its phase-0 tile launch skips them)
    double *const X_save = a.X_save, *const U_save = a.U_save;
    const int seg = mpcq::ListSeg::cap(B);
    const size_t lcap = (size_t)mpcq::ListSeg::kShards * seg;
    // Counter blocks: launch p zeroes block p + 1 (its successor's output) and a chain's final launch,
    // when it is at least the third, zeroes block 0 for the next solve; only a chain that could not
    // leave block 0 clean costs a memset here.
    if (!c->count0_clean && hipMemsetAsync(c->d_counts, 0, 4 * (size_t)mpcq::ListSeg::kCounters, s) != hipSuccess)
        return -2;
    c->count0_clean = false;
    const int mpc = a.mpc;
    // one QP per wave: from phase 0 for small batches, else the chain's last launch (phase_stops)
    const int tail_from = wave_only ? 0 : wave_tail ? np - 1 : kMaxPhases;
    int np_run = 0;
    a.list_seg = seg;
    // a chain entirely on tile waves publishes x, y lazily (materialize_xy; test hook MPCQ_LAZY_XY=0: eager)
    const bool lazy_xy = tail_from >= np && test_hook("MPCQ_LAZY_XY")[0] != '0';
    if (lazy_xy) {
        a.x = nullptr;
        a.y = nullptr;
        // fp64 state: the finalize stores rho once, as warm state (materialize_rho reports it)
        if (std::is_same<T, double>::value) a.rho_out = nullptr;
    }
    // ... and one ordered launch its status, iter in list-slot order (materialize_info; test hook
    // MPCQ_LAZY_INFO=0: at the QPs' indices)
    const bool lazy_info = lazy_xy && ordered && np == 1 && test_hook("MPCQ_LAZY_INFO")[0] != '0';
    a.info_slot = lazy_info ? ord_list + B : nullptr;

    // debug build: per-wave stage stamps of every phase launch, written to $MPCQ_TILE_STAMPS after the solve
    const char *stp = debug_hook("MPCQ_TILE_STAMPS");
    const size_t waves = (size_t)(B + 15) / 16 + 4 * mpcq::ListSeg::kShards;
    if (stp && *stp && c->d_stamps.alloc(8 * 8 * waves * kMaxPhases) != MPCQ_OK) return -2;
    if (stp && *stp && hipMemsetAsync(c->d_stamps, 0, 8 * 8 * waves * kMaxPhases, s) != hipSuccess) return -2;
    for (int p = 0; p < np; p++) {
        a.stamps = (stp && *stp) ? c->d_stamps + (size_t)p * 8 * waves : nullptr;
        a.img = (const T *)c->d_img;
        a.list_in = p ? c->d_list + (size_t)(p % 2) * lcap : nullptr;
        a.count_in = p ? c->d_counts + (size_t)(p - 1) * mpcq::ListSeg::kCounters : nullptr;
        a.list_out = c->d_list + (size_t)((p + 1) % 2) * lcap;
        a.count_out = c->d_counts + (size_t)p * mpcq::ListSeg::kCounters;
        a.it_state = c->d_itstate;
        a.ord_list = (ordered && p == 0) ? ord_list : nullptr;
        a.X_save = (ordered && p == 0) ? nullptr : X_save;
        a.U_save = (ordered && p == 0) ? nullptr : U_save;
        a.ord_zero = (ordered && p == 0) ? ord_cnt : nullptr;
        a.stop_iter = stops[p];
        a.resume = p > 0;
        a.mpc = p == 0 ? mpc : 0;  // later phases read q, u from the buffers phase 0 filled
        const bool final_launch = p + 1 == np || (p >= tail_from && c->dims.n <= 32 && c->dims.m <= 64);
        a.zero_cnt = final_launch ? nullptr : c->d_counts + (size_t)(p + 1) * mpcq::ListSeg::kCounters;
        a.zero_cnt0 = (final_launch && p >= 2) ? c->d_counts : nullptr;
        int rc;
        if (p >= tail_from && c->dims.n <= 32 && c->dims.m <= 64) {
            // one QP per wave carries no idle columns: the rest of the solve is one launch (a resumed
            // list: a multiple of ListSeg::kShards blocks)
            a.stop_iter = c->set.max_iter;
            if (p > 0 && mpc && a.X_save) {
                // the wave kernel reads q, u from the buffers, which a lazy phase 0 did not fill: its
                // front end rebuilds them from X, U (the tile prologue's fp64 order) for the QPs it runs
                a.mpc = 1;
                a.q_out = c->d_q;
                a.u_out = c->d_u;
            }
            rc = wave_launch<T>(c, a, p == 0 ? B : 2048, s);
            if (rc) return rc;
            c->count0_clean = a.zero_cnt0 != nullptr;
            np_run = p + (stp && *stp ? 1 : 0);  // (the stamps dump includes the wave launch)
            break;
        }
        // every phase launches the phase-0 grid: list segment s is served by the blocks b % kShards == s
        // (per-QP references: the REF variant, whose every phase re-forms q from X, U and ref)
        rc = mpcq::launch_tile(a, c->KN, c->KM, c->cur_ref.p && a.X ? &c->cur_ref : nullptr, s);
        if (rc) return rc;
        c->count0_clean = a.zero_cnt0 != nullptr;
        if (a.ord_zero) c->ord_clean = true;
        np_run = p + 1;
    }
    c->lazy.xy = lazy_xy;
    c->lazy.rho = lazy_xy && std::is_same<T, double>::value;
    c->lazy.info = lazy_info;
    if (stp && *stp) return dump_tile_stamps(stp, c->d_stamps, np_run, waves, s);
    return 0;
}

template <typename T>
int launch_args(mpcq_ctx *c, mpcq::AdmmArgs<T> &a, hipStream_t s)
{
    const PathChoice p = choose_path(c);
    a.paired = p.paired;
    if (p.kind == MPCQ_PATH_LANE)  // (the reference: for an MPC front end with per-QP references, the REF variant)
        return mpcq::launch_lane(a, c->nc, c->mc, c->cur_ref.p && a.mpc ? &c->cur_ref : nullptr, s);
    if (!c->tile) {  // per-plant batches: one QP per wave (operators in VGPRs)
        a.stop_iter = c->set.max_iter;
        return wave_launch<T>(c, a, c->dims.batch, s);
    }
    return launch_phases<T>(c, a, s, p.kind == MPCQ_PATH_WAVE);
}

template <typename T>
int launch_typed(mpcq_ctx *c, hipStream_t s, bool mpc, const double *X, double *U, double xref)
{
    auto a = make_args<T>(c);
    if (mpc) {
        set_mpc_front_end(c, a, X, U, xref);
        if (c->set.polish) a.mpc_u = 0;  // (the applied move is the polished one: polish_kernel's U += x[0])
        // (a step with per-QP references writes q, u eagerly on every path: q must outlive the caller's
        // reference buffer, and a saved window would need its own copy, buffer and front-end variant)
        const bool lazy = c->tile && choose_path(c).kind == MPCQ_PATH_TILE && c->d_Xs && c->d_Us && !c->cur_ref.p;
        if (lazy) {  // phase 0 saves X, U (40 B/QP) instead of writing q, u (480 B/QP): materialize_qu
            a.X_save = c->d_Xs; a.U_save = c->d_Us;
        } else {
            a.q_out = c->d_q; a.u_out = c->d_u;
        }
        c->lazy.qu = lazy;
        c->lazy.xref = xref;
    }
    return launch_args<T>(c, a, s);
}
// a verbose solve synchronises its stream.
const char *status_name(int st)
{
    switch (st) {
    case MPCQ_SOLVED: return "solved";
    case MPCQ_SOLVED_INACCURATE: return "solved inaccurate";
    case MPCQ_MAX_ITER_REACHED: return "maximum iterations reached";
    case MPCQ_PRIMAL_INFEASIBLE: return "primal infeasible";
    case MPCQ_DUAL_INFEASIBLE: return "dual infeasible";
    case MPCQ_NON_CVX: return "problem non convex";
    case MPCQ_INVALID_BOUNDS: return "invalid bounds (u < l)";
    case MPCQ_TYPE_CHANGED: return "constraint type changed (re-run setup)";
    case MPCQ_UNSOLVED: return "unsolved";
    default: return st == 3 ? "primal infeasible inaccurate" : st == 4 ? "dual infeasible inaccurate" : "unknown";
    }
}


// settings.polish: OSQP's polish of every SOLVED QP of the solve just enqueued on s (mpcq_polish.hip), one
// more launch on the same stream.  Whatever the solve left lazy (q, u of a tile-path controllerStep; x, y,
// rho, status, iter of a tile chain) is published first, on the same stream (c->last == s), so the kernel
// reads this solve's data and results and every later reader finds d_x, d_y, d_status, d_iter complete.
int launch_polish(mpcq_ctx *c, hipStream_t s, double *U)
{
    int rc = materialize_qu(c);
    if (rc || (rc = materialize_info(c)) || (rc = materialize_xy(c)) || (rc = materialize_rho(c))) return rc;
    mpcq::PolishArgs a{};
    a.batch = c->dims.batch;
    a.n = c->dims.n;
    a.m = c->dims.m;
    a.nc = c->nc;
    a.mc = c->mc;
    a.shared = c->dims.n_plants == 1;
    a.is_f32 = c->dims.dtype == MPCQ_F32;
    a.ops_stride = c->ops_stride;
    a.ops = c->d_ops;
    a.P = c->d_P;
    a.A = c->d_A;
    a.q = c->d_q;
    a.l = c->d_l;
    a.u = c->d_u;
    a.xs = c->d_xs;
    a.zs = c->d_zs;
    a.ys = c->d_ys;
    a.status = c->d_status;
    a.x = c->d_x;
    a.y = c->d_y;
    a.U = U;
    a.pol_status = c->d_pol_status;
    a.pol_nact = c->d_pol_nact;
    a.pol_res = c->d_pol_res;
    a.delta = c->set.delta;
    a.refine = c->set.polish_refine_iter;
    a.scaled_termination = c->set.scaled_termination;
    hipError_t err = hipSuccess;
    const int prc = mpcq_internal_polish_launch(&a, c->cus, s, &err);
    if (prc == -1) return fail(MPCQ_ERR_ARG, "polish: the kernel serves n <= 32, m <= 64");
    if (prc) return fail(MPCQ_ERR_HIP, std::string("polish kernel launch failed: ") + hipGetErrorString(err));
    c->pol_valid = true;
    return MPCQ_OK;
}

}  // namespace

mpcq::SolverSettings to_solver(const mpcq_settings &s)
{
    mpcq::SolverSettings o{};
    o.rho = s.rho;
    o.sigma = s.sigma;
    o.alpha = s.alpha;
    o.eps_abs = s.eps_abs;
    o.eps_rel = s.eps_rel;
    o.eps_prim_inf = s.eps_prim_inf;
    o.eps_dual_inf = s.eps_dual_inf;
    o.adaptive_rho_tolerance = s.adaptive_rho_tolerance;
    o.max_iter = s.max_iter;
    o.check_termination = s.check_termination;
    o.adaptive_rho = s.adaptive_rho;
    o.adaptive_rho_interval = s.adaptive_rho_interval;
    o.warm_start = s.warm_start;
    o.scaled_termination = s.scaled_termination;
    o.scaling = s.scaling;
    return o;
}

template <typename T>
mpcq::AdmmArgs<T> make_args(mpcq_ctx *c)
{
    mpcq::AdmmArgs<T> a{};
    const mpcq::OpsLayout L = mpcq::OpsLayout::make(c->nc, c->mc);
    const T *base = std::is_same<T, double>::value ? (const T *)c->d_ops : (const T *)c->d_ops32;
    fill_ops(a.ops, base, L, c->d_ctype);
    a.batch = c->dims.batch;
    a.n = c->dims.n;
    a.m = c->dims.m;
    a.shared = c->dims.n_plants == 1;
    a.ops_stride = c->ops_stride;
    a.ctype = c->d_ctype;
    a.st = to_solver(c->set);
    a.eps10[0] = (T)a.st.eps_abs * T(10);
    a.eps10[1] = (T)a.st.eps_rel * T(10);
    a.eps10[2] = (T)a.st.eps_prim_inf * T(10);
    a.eps10[3] = (T)a.st.eps_dual_inf * T(10);
    const int ct = c->set.check_termination;
    a.adaptive_interval = c->set.adaptive_rho_interval ? c->set.adaptive_rho_interval : (ct ? 4 * ct : 100);
    a.all_ineq = c->all_ineq;
    a.dinf_kappa = c->set.scaled_termination ? c->dinf_ks : c->dinf_ku;
    a.lower_free = c->lower_free;
    a.q = c->d_q;
    a.u = c->d_u;
    a.l = c->d_l;
    a.l_shared = 0;
    a.xs = (T *)c->d_xs;
    a.zs = (T *)c->d_zs;
    a.ys = (T *)c->d_ys;
    a.rhos = (T *)c->d_rhos;
    a.warm = c->set.warm_start;
    a.fresh = c->fresh;
    a.snap_x = (T *)c->d_snx;
    a.snap_y = (T *)c->d_sny;
    a.x = c->d_x;
    a.y = c->d_y;
    a.rho_out = c->d_rho;
    a.status = c->d_status;
    a.iter = c->d_iter;
    a.it_acc = c->stream_acc ? c->d_it_acc : nullptr;
    a.uns_acc = c->stream_acc ? c->d_uns_acc : nullptr;
    {
        const char *o = test_hook("MPCQ_TILE_OCC");  // f32 paired tile kernel: 2 or 3 waves/SIMD (A/B)
        a.tile_occ = *o ? std::atoi(o) : 0;
    }
    if (c->dims.dtype == MPCQ_F64_MIXED) {  // (test hook MPCQ_MIX_R: another fp64 share for A/B)
        const char *r = test_hook("MPCQ_MIX_R");
        a.mix_r = *r ? std::max(1, std::atoi(r)) : MPCQ_MIX_R;
    }
    return a;
}

template mpcq::AdmmArgs<float> make_args<float>(mpcq_ctx *c);
template mpcq::AdmmArgs<double> make_args<double>(mpcq_ctx *c);

// The device path of this context's next solve, decided in one place for launch_args and
// mpcq_get_path: per-plant contexts run one QP per wave (n <= 32, m <= 64) or one QP per lane;
// shared-plant contexts run the MFMA tile kernel's phase chain (its tail one QP per wave), except
// that small batches (under 512 tile waves: latency-bound) run one QP per wave throughout.
PathChoice choose_path(const mpcq_ctx *c)
{
    const char *k = env_kernel();
    const bool fits_wave = c->dims.n <= 32 && c->dims.m <= 64;
    PathChoice p{MPCQ_PATH_LANE, false};
    if (c->inv_ops) return {MPCQ_PATH_WAVE, false};  // direct-inverse operators: the wave kernel's refactorisation
    if (std::strcmp(k, "lane") == 0 || !fits_wave) return p;
    if (!c->tile) return {MPCQ_PATH_WAVE, false};
    const bool small = c->dims.batch < 8192 && std::strcmp(k, "tile") != 0;
    if (small || std::strcmp(k, "wave") == 0) return {MPCQ_PATH_WAVE, false};
    return {MPCQ_PATH_TILE, c->paired && c->all_ineq && c->lower_free};
}

// The debug dump $MPCQ_TILE_STAMPS in the tools/stamps.py format: the header {phases, waves}, then the 8 stamps
// of every wave, phase by phase.  Synchronises s.
int dump_tile_stamps(const char *path, const long long *d_stamps, size_t phases, size_t waves, hipStream_t s)
{
    std::vector<long long> h(8 * waves * phases);
    if (hipMemcpyAsync(h.data(), d_stamps, 8 * h.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return -2;
    if (FILE *f = std::fopen(path, "wb")) {
        const long long hdr[2] = {(long long)phases, (long long)waves};
        std::fwrite(hdr, 8, 2, f);
        std::fwrite(h.data(), 8, h.size(), f);
        std::fclose(f);
    }
    return 0;
}

// `count` stamps of a plant or MIMO kernel's debug build, raw (tools/*stamps*.py read them): MPCQ_OK or MPCQ_ERR_HIP
int dump_stamps(const char *path, const long long *d_stamps, size_t count, hipStream_t s)
{
    std::vector<long long> h(count);
    HIPCHK(hipMemcpyAsync(h.data(), d_stamps, 8 * count, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (FILE *f = std::fopen(path, "wb")) {
        std::fwrite(h.data(), 8, count, f);
        std::fclose(f);
    }
    return MPCQ_OK;
}

// ---- settings.verbose (osqp-eigen setVerbosity, ModelPredictiveControlAPI.cpp:51, solver.cpp:21-25):
// OSQP v0.6's setup header, its iteration summary line and its status footer, for QP 0 of the context
// (the reference's one QP), plus the batch's status counts.  The device keeps no per-iteration record,
// so the summary is the final iterate's line: objective, primal and dual residual of the returned
// (x, y) in the unscaled problem, the final rho, the host-timed solve.  Printed on stdout as OSQP does;

void verbose_header(const mpcq_ctx *c, const char *what)
{
    if (!c->set.verbose) return;
    const mpcq_settings &s = c->set;
    const char *dt = c->dims.dtype == MPCQ_F32 ? "fp32 iterate, fp64 setup"
                     : c->dims.dtype == MPCQ_F64_MIXED ? "fp64 (fp32 plain iterations on the tile path)" : "fp64";
    std::printf("-----------------------------------------------------------------\n"
                "   libmpcq: batched OSQP-v0.6 ADMM on gfx950 (solvempc_amd)\n"
                "-----------------------------------------------------------------\n");
    std::printf("problem:  variables n = %d, constraints m = %d\n", c->dims.n, c->dims.m);
    std::printf("          batch = %d QPs, %s, %s\n", c->dims.batch,
                c->dims.n_plants == 1 ? "one shared (P, A)" : "one (P, A) per QP", dt);
    std::printf("          setup: %s\n", what);
    std::printf("settings: linear system solver = reduced KKT on the device (%s),\n",
                c->tile ? "eigenbasis, MFMA tile kernel" : c->inv_ops ? "direct inverse" : "eigenbasis");
    std::printf("          eps_abs = %.1e, eps_rel = %.1e,\n", s.eps_abs, s.eps_rel);
    std::printf("          eps_prim_inf = %.1e, eps_dual_inf = %.1e,\n", s.eps_prim_inf, s.eps_dual_inf);
    std::printf("          rho = %.2e %s,\n", s.rho, s.adaptive_rho ? "(adaptive)" : "");
    std::printf("          sigma = %.2e, alpha = %.2f, max_iter = %d\n", s.sigma, s.alpha, s.max_iter);
    if (s.check_termination) std::printf("          check_termination: on (interval %d),\n", s.check_termination);
    else std::printf("          check_termination: off,\n");
    std::printf("          scaling: %s, scaled_termination: %s\n", s.scaling ? "on" : "off",
                s.scaled_termination ? "on" : "off");
    std::printf("          warm start: %s, polish: %s, time_limit: off\n\n", s.warm_start ? "on" : "off",
                s.polish ? "on" : "off");
    std::fflush(stdout);
}

void verbose_solve(mpcq_ctx *c, double seconds)
{
    const size_t B = c->dims.batch, n = c->dims.n, m = c->dims.m;
    std::vector<int> st(B), it(B);
    std::vector<double> rho(B), x(n), y(m), q(n), u(m), l(m), P(n * n), A(m * n);
    if (materialize_xy(c) != MPCQ_OK || materialize_rho(c) != MPCQ_OK || materialize_info(c) != MPCQ_OK ||
        hipStreamSynchronize(c->last) != hipSuccess ||
        hipMemcpy(st.data(), c->d_status, 4 * B, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(it.data(), c->d_iter, 4 * B, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(rho.data(), c->d_rho, 8 * B, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(x.data(), c->d_x, 8 * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(y.data(), c->d_y, 8 * m, hipMemcpyDeviceToHost) != hipSuccess)
        return;
    // QP 0's data in the unscaled problem (generic contexts: plant 0's P, A and this solve's q, l, u)
    bool have = c->mode == mpcq_ctx::Mode::Generic && materialize_qu(c) == MPCQ_OK &&
                hipMemcpy(q.data(), c->d_q, 8 * n, hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(u.data(), c->d_u, 8 * m, hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(l.data(), c->d_l, 8 * m, hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(P.data(), c->d_P, 8 * n * n, hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(A.data(), c->d_A, 8 * m * n, hipMemcpyDeviceToHost) == hipSuccess;
    const bool sol = st[0] == MPCQ_SOLVED || st[0] == MPCQ_SOLVED_INACCURATE || st[0] == MPCQ_MAX_ITER_REACHED;
    double obj = 0.0, pri = 0.0, dua = 0.0;
    if (have && sol) {
        std::vector<double> Px(n, 0.0), Aty(n, 0.0);
        for (size_t i = 0; i < n; i++)
            for (size_t k = 0; k < n; k++) Px[i] += P[std::min(i, k) * n + std::max(i, k)] * x[k];  // upper triangle
        for (size_t j = 0; j < m; j++) {
            double ax = 0.0;
            for (size_t k = 0; k < n; k++) {
                ax += A[j * n + k] * x[k];
                Aty[k] += A[j * n + k] * y[j];
            }
            pri = std::max(pri, std::max(ax - u[j], l[j] - ax));
        }
        for (size_t i = 0; i < n; i++) {
            obj += 0.5 * x[i] * Px[i] + q[i] * x[i];
            dua = std::max(dua, std::fabs(Px[i] + q[i] + Aty[i]));
        }
    }
    std::printf("iter   objective    pri res    dua res    rho        time\n");
    if (have && sol) std::printf("%4d  %12.4e  %9.2e  %9.2e  %9.2e  %9.2es\n\n", it[0], obj, pri, dua, rho[0], seconds);
    else std::printf("%4d  %12s  %9s  %9s  %9.2e  %9.2es\n\n", it[0], "-", "-", "-", rho[0], seconds);
    std::vector<int> pst;
    if (c->set.polish && c->pol_valid) {
        pst.resize(B);
        if (hipMemcpy(pst.data(), c->d_pol_status, 4 * B, hipMemcpyDeviceToHost) != hipSuccess) pst.clear();
    }
    std::printf("status:               %s\n", status_name(st[0]));
    if (!pst.empty() && pst[0]) std::printf("solution polish:      %s\n", pst[0] == 1 ? "successful" : "unsuccessful");
    std::printf("number of iterations: %d\n", it[0]);
    if (have && sol) std::printf("optimal objective:    %.4f\n", obj);
    std::printf("run time:             %.2es\n", seconds);
    std::printf("final rho:            %.2e\n", rho[0]);
    if (B > 1) {
        size_t solved = 0;
        long long tot = 0;
        int mn = it[0], mx = it[0];
        for (size_t b = 0; b < B; b++) {
            solved += st[b] == MPCQ_SOLVED;
            tot += it[b];
            mn = std::min(mn, it[b]);
            mx = std::max(mx, it[b]);
        }
        if (pst.empty()) {
            std::printf("batch:                %zu QPs, %zu solved, iterations %d / %.1f / %d (min / mean / max)\n", B,
                        solved, mn, (double)tot / B, mx);
        } else {
            size_t polished = 0;
            for (size_t b = 0; b < B; b++) polished += pst[b] == 1;
            std::printf("batch:                %zu QPs, %zu solved, %zu polished, iterations %d / %.1f / %d (min / mean / "
                        "max)\n", B, solved, polished, mn, (double)tot / B, mx);
        }
    }
    std::printf("\n");
    std::fflush(stdout);
}


int launch_solve(mpcq_ctx *c, hipStream_t s, bool mpc, const double *X, double *U, double xref)
{
    const auto t0 = std::chrono::steady_clock::now();
    c->lazy.ord = false;  // (launch_phases sets it for a hardest-first tile solve)
    // (the solve below writes x, y, rho, status and iter of every QP, or launch_phases leaves them lazy again)
    c->lazy.clear_results();
    const int rc = c->dims.dtype == MPCQ_F32 ? launch_typed<float>(c, s, mpc, X, U, xref)
                                             : launch_typed<double>(c, s, mpc, X, U, xref);
    if (rc) return fail(MPCQ_ERR_HIP, std::string("ADMM kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    c->last = s;
    c->fresh = false;
    c->have_xy = true;
    c->pol_valid = false;
    c->sens_ok = !c->stream_acc;  // (a stream run's per-step solves are not served: mpcq_sensitivity_device)
    if (c->set.polish) {
        if (int prc = launch_polish(c, s, mpc ? U : nullptr)) return prc;
    }
    // settings.verbose: the summary needs the results on the host, so it synchronises the stream, which a
    // stream under capture (mpcq_mpc_run_device's per-step graph) must not do: there the replay loop prints
    // after each replayed step instead
    if (c->set.verbose && !stream_capturing(s)) {
        (void)hipStreamSynchronize(s);
        verbose_solve(c, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    return MPCQ_OK;
}

extern "C" {

int mpcq_reset(mpcq_ctx *c)
{
    int rc = check_ctx(c, kAnySetup);
    if (rc) return rc;
    c->fresh = true;
    c->sens_ok = false;
    return MPCQ_OK;
}

int mpcq_solve(mpcq_ctx *c, void *stream)
{
    int rc = check_ctx(c, kGeneric);
    if (rc) return rc;
    if ((rc = materialize_qu(c))) return rc;
    return launch_solve(c, (hipStream_t)stream, false, nullptr, nullptr, 0.0);
}

}  // extern "C"

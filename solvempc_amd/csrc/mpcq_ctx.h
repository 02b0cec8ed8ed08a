// solvempc_amd/csrc/mpcq_ctx.h — private to the host side of the C ABI (the mpcq_host_*.cpp files; no .hip file
// includes it): the context, the owner of its device buffers, and the helpers that cross the host files.
#pragma once

#include "../../include/mpcq.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "mpcq_internal.h"

// (nothing declared here is an exported symbol of libmpcq.so)
#pragma GCC visibility push(hidden)

// Records msg as the calling thread's mpcq_last_error text and returns code.
int fail(int code, const std::string &msg);

#define HIPCHK(expr)                                                                  \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) return fail(MPCQ_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

constexpr int kMaxPhases = 16;

// Test hooks: the library reads exactly these environment variables, here and nowhere else.  Each
// selects among production code paths so that the tests can cover every path on one device:
//   MPCQ_KERNEL=lane|wave|tile  the ADMM kernel family (mpcq_get_path reports the choice)
//   MPCQ_PHASES=0|k1,k2,..      the tile path's phase stops, in check_termination multiples
//   MPCQ_SETUP=ref              per-plant setup on the workgroup kernel (mpcq_setup.hip)
//   MPCQ_CONDENSE=ref           condensing on the workgroup kernel (mpcq_condense.hip)
//   MPCQ_MIMO_GENERAL_K0=1      the MIMO solve's general-K0 exchange path on a diagonal K0
//   MPCQ_STREAM=graph|wave      mpcq_mpc_run_device's per-step graph or one-QP-per-wave launch
//                               (mpcq_get_stream_path reports the choice)
//   MPCQ_STREAM_CPW=k           plants per wave of the tile stream mode
//   MPCQ_STREAM_OCC=1           the tile stream mode's one-wave-per-SIMD variant (when the waves fit)
//   MPCQ_TAIL=wave|tile         the tile chain's last launch on the one-QP-per-wave / tile kernel
//   MPCQ_MIX_R=r                MPCQ_F64_MIXED: fp64 iterations per check interval (default MPCQ_MIX_R)
//   MPCQ_TILE_OCC=2|3           waves per SIMD of the f32 paired tile kernel (default 3)
//   MPCQ_PLANT_WPE=2|3|4        waves per SIMD of the one-pass per-plant kernel (default f64 3, f32 2)
//   MPCQ_PLANT_LAYOUT=2         the one-pass per-plant kernel with two plants per wave at N 17 .. 20 (default 3)
//   MPCQ_ORDER=0                a shared-plant MPC step's tile solve in index order (default: hardest first)
//   MPCQ_LAZY_XY=0              the tile solve stores x, y at finalize (default: published on demand)
//   MPCQ_LAZY_INFO=0            an ordered one-launch solve stores status, iter at the QPs' indices
//                               (default: in list-slot order, permuted on demand)
// Debug builds (-DMPCQ_DEBUG_HOOKS) add the stamp / profiling dumps (MPCQ_TILE_STAMPS,
// MPCQ_SETUP_PROF, MPCQ_MIMO_SETUP_STAMPS, MPCQ_MIMO_STAMPS) and MPCQ_DEBUG_SYNC.
inline const char *test_hook(const char *name)
{
    const char *v = std::getenv(name);
    return v ? v : "";
}
inline const char *debug_hook(const char *name)
{
#ifdef MPCQ_DEBUG_HOOKS
    const char *v = std::getenv(name);
    return v ? v : "";
#else
    (void)name;
    return "";
#endif
}

// The owner of one device allocation: freed when the owner goes, never copied.  It reads as its element pointer
// (an explicit cast re-types it, as the same cast re-types a pointer), and after a failed allocation it is empty.
template <typename T>
class DevBuf {
    T *p_ = nullptr;
    size_t cap_ = 0;  // bytes the last grow() asked for

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    ~DevBuf() { release(); }
    operator T *() const { return p_; }
    template <typename U>
    explicit operator U *() const { return (U *)p_; }
    size_t cap() const { return cap_; }
    void release()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // Allocates max(bytes, 8) when empty; the failure text is "hipMalloc failed" or "hipMalloc failed (what)".
    int alloc(size_t bytes, const char *what = nullptr)
    {
        if (p_) return MPCQ_OK;
        if (hipMalloc((void **)&p_, std::max<size_t>(bytes, 8)) == hipSuccess) return MPCQ_OK;
        p_ = nullptr;
        return fail(MPCQ_ERR_HIP, what ? std::string("hipMalloc failed (") + what + ")" : std::string("hipMalloc failed"));
    }
    // Room for `bytes`: a smaller buffer is replaced once nothing enqueued on s still reads it.
    int grow(size_t bytes, hipStream_t s, const char *what = nullptr)
    {
        if (bytes <= cap_) return MPCQ_OK;
        HIPCHK(hipStreamSynchronize(s));
        release();
        if (int rc = alloc(bytes, what)) return rc;
        cap_ = bytes;
        return MPCQ_OK;
    }
};

struct mpcq_ctx {
    mpcq_dims dims{};
    mpcq_settings set{};
    int nc = 0, mc = 0;
    size_t ops_stride = 0;
    // The formulation the context was last set up for: the generic / condensed-MPC operators
    // (mpcq_setup, mpcq_mpc_setup_plants_device) or the MIMO operator blocks
    // (mpcq_mimo_setup_plants_device).  Each entry point checks for the one it runs on.
    // OneShot: mpcq_mpc_plants_step_device left this step's results but no operators behind.
    enum class Mode { None, Generic, Mimo, OneShot } mode = Mode::None;
    bool all_ineq = true, mpc_ready = false, lower_free = false, fresh = false;
    double dinf_ks = 0.0, dinf_ku = 0.0;  // dual-infeasibility bounds (AdmmArgs::dinf_kappa), 0: none
    int cus = 256;                        // compute units of the device (phase lists)
    // What the last solve left to be published on demand, and its order flag.
    struct Lazy {
        // a tile solve whose finalize stored only the warm state (x', z, y) and U: d_x, d_y are formed from it by
        // materialize_xy before anything reads them (get_solution / get_dual, the device view, verbose, or a
        // call that overwrites the warm state)
        bool xy = false;
        // the same solve's rho (fp64 contexts): its warm-state rho d_rhos is the reported one; d_rho is copied
        // from it by materialize_rho before anything reads d_rho (get_info, the device view, verbose) or a
        // reset overwrites d_rhos
        bool rho = false;
        // an ordered single-launch solve left status, iter in list-slot order: materialize_info permutes them
        // into d_status, d_iter before anything reads those (get_info, the device view, verbose, the publish
        // kernel of materialize_xy)
        bool info = false;
        // a tile-path controllerStep leaves q, u (the solver's data after updateGradient / updateUpperBound)
        // as the step's saved X, U (d_Xs, d_Us) and its xref: d_q, d_u are filled from them by materialize_qu
        // before anything reads them (a generic solve, the device view, an update, new operators)
        bool qu = false;
        double xref = 0.0;
        bool ord = false;  // the last solve ran in the hardest-first order (mpcq_get_order)
        void clear_results() { xy = rho = info = false; }  // a solve that writes every QP's x, y, rho, status, iter
    } lazy;
    DevBuf<double> d_Xs, d_Us;
    bool paired = false;  // shared plant of the condensed-MPC shape (tile kernel's paired loop)
    bool inv_ops = false; // per-plant operators in the direct-inverse reading (setup_inv_kernel): wave kernel only
    // tile (MFMA) path: shared plant with a compiled (KN, KM) shape
    bool tile = false;
    int KN = 0, KM = 0;
    DevBuf<void> d_img;
    DevBuf<int> d_list, d_counts, d_itstate;
    bool count0_clean = false;    // phase 0's ListSeg counters are zero (the last phase chain's final launch zeroed them)
    DevBuf<long long> d_stamps;  // debug (MPCQ_TILE_STAMPS)
    hipStream_t last = nullptr;
    int nx = 0;
    // setup
    DevBuf<double> d_P, d_q0, d_A, d_l0, d_u0;
    DevBuf<double> d_ops, d_scratch;
    DevBuf<int> d_flags;
    DevBuf<float> d_ops32;
    DevBuf<int> d_ctype, d_setup_status;
    // per QP
    DevBuf<double> d_q, d_u, d_l, d_x, d_y, d_rho;
    DevBuf<int> d_status, d_iter;
    DevBuf<void> d_xs, d_zs, d_ys, d_rhos, d_snx, d_sny;
    // MPC front end
    DevBuf<double> d_Fx, d_Fu, d_Fr, d_Sbar, d_Ku, d_W0;
    DevBuf<double> d_X, d_U;
    // receding-horizon stream: plant, step counter, captured graph of one control step
    DevBuf<double> d_Ad, d_Bd;
    DevBuf<long long> d_step;
    int plant_nx = 0;
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    // gen: bumped whenever buffers baked into the captured graph are reallocated or the kernel
    // variant flags (all_ineq, lower_free) may change; a replay needs the generation it captured
    unsigned long long gen = 1;
    struct { double *X, *U; double xref, noise; unsigned long long seed; long long first_qp; hipStream_t s;
             unsigned long long gen; const double *sched; int sched_len; long long sched_stride; } gkey{};
    // per-QP horizon references (mpcq_mpc_step_ref*, mpcq_mpc_run_ref_device): the reference of the call in
    // progress (p == null: a scalar-xref call), read by launch_typed / launch_stream / launch_tile_stream;
    // d_ref: the host form's staging buffer (grown on demand); d_ordG: G = -A P^-1 Fr (m x n) of the
    // hardest-first order's key (ordG_ok when it matches d_ordmap)
    mpcq::RefArgs cur_ref{};
    DevBuf<double> d_ref;
    DevBuf<double> d_ordG;
    bool ordG_ok = false;
    // what the captured step leaves lazy and its order flag: every replay leaves the same, whatever a reader
    // materialised in between
    Lazy glazy;
    bool mimo_only = false;  // n > 32 or m > 64 per plant: only the MIMO entry points serve it
    // MIMO condensed MPC (mpcq_mimo.hip; the host side is mpcq_host_mimo.cpp): what the last
    // mpcq_mimo_setup_plants_device left and what the mpcq_mimo_* calls keep between them
    struct Mimo {
        DevBuf<double> ops;  // per-plant operator block
        int N = 0, nx = 0, nu = 0, ny = 0, srows = 0, diag_k0 = 0;  // dims
        bool stepped = false;  // a mpcq_mimo_step_device since the last MIMO setup (mpcq_mimo_sensitivity* needs one)
        bool ref_step = false; // that step was a mpcq_mimo_step_ref* (mpcq_mimo_plant_vjp* knows yref only: refused)
        // mpcq_mimo_plant_vjp*: mimo_sens_kernel's (gq, gu, n_active) for the call's g, which mimo_plant_vjp_kernel reads
        // (batch*n, batch*2n doubles, then batch ints; allocated on first use)
        DevBuf<double> pv;
        // closed-loop MIMO runs (mpcq_mimo_set_plant_device, mpcq_mimo_run*_device): the simulated plant
        // of every QP (plant: set, for this block's nx, nu) and the padded tail of a reference schedule (grown by the
        // first run that reaches it)
        DevBuf<double> Ad, Bd, tail;
        bool plant = false;
        DevBuf<double> Uprev;  // mpcq_mimo_step_polish_device: the caller's U from before the step
        // What a setup for these dims invalidates, whether it then succeeds or not: the operator blocks of another
        // shape, the simulated plant of another n_x or n_u (mpcq_mimo_set_plant_device's arrays have these shapes), and
        // every record of a step.
        void invalidate(int N_, int nx_, int nu_, int ny_)
        {
            if (N != N_ || nx != nx_ || nu != nu_ || ny != ny_) ops.release();
            if (nx != nx_ || nu != nu_) {
                Ad.release();
                Bd.release();
                plant = false;
            }
            stepped = ref_step = false;
        }
    } mimo;
    // receding-horizon stream counters (mpcq_mpc_run_device): per-QP iterations and unsolved steps
    DevBuf<int> d_it_acc, d_uns_acc;
    bool stream_acc = false;  // launches made inside mpcq_mpc_run_device accumulate into them
    int stream_path = MPCQ_STREAM_GRAPH;  // how the last mpcq_mpc_run_device call ran
    // per-step record of the stream (mpcq_mpc_set_stream_log): the caller's buffers while one is attached
    // (slog_on), baked into a captured graph (gen); d_logref: the one-entry schedule [xref] a logged scalar run
    // hands the wave stream's REF + LOG kernel
    mpcq_stream_log slog{};
    bool slog_on = false;
    DevBuf<double> d_logref;
    // hardest-first order of a tile-path MPC step (mpcq_order.hip, build_order_map): the m x kStride
    // violation map of plant 0, the bin counters and lists; ord_ok when the map matches the current setup
    // and operators
    DevBuf<double> d_ordmap;
    // OrderBins::kBins counters, then `batch` keys, the list of `batch` QPs, and `batch` (status, iter) pairs in
    // list-slot order (AdmmArgs::info_slot)
    DevBuf<int> d_ord;
    bool ord_ok = false;
    // the same order for a batch of distinct plants (mpcq_mpc_plants_step_device): the map of the batch's first
    // plant, kept while the plant arrays are the same (pord_key); pord_ok when d_ordmap holds it
    bool pord_ok = false;
    struct { const double *Ad, *Bd, *Cd, *K, *Q, *R, *RD; int nx, s_rows; } pord_key{};
    bool ord_clean = false;  // the order's bin counters are zero (an ordered phase-0 launch clears them)
    // settings.polish (mpcq_polish.hip): status_polish and the reduced system's rows per QP, the returned
    // solution's (primal, dual) residual pairs; allocated only when polish is set, or by the first
    // mpcq_mimo_step_polish_device (mpcq_mimo_polish.hip).  pol_valid: the last solve filled them
    // (mpcq_get_polish_info reports "not performed" otherwise)
    DevBuf<int> d_pol_status, d_pol_nact;
    DevBuf<double> d_pol_res;
    bool pol_valid = false;
    // active-set sensitivities (mpcq_sens.hip).  sens_ok: the warm state and d_l, d_u are those of a solve that
    // mpcq_sensitivity* serves (set by launch_solve outside a stream run; cleared by every setup, data update,
    // warm / cold start, reset and stream run).  d_sens: staging of the host forms and the step gains' (gq, gu),
    // allocated on first use (g, gq: batch*n; gl, gu: batch*m; dX: batch*8; dU: batch; dref: batch*n; then
    // batch ints).
    bool sens_ok = false;
    // d_x, d_y hold (or a pending publish will give) the (x, y) that mpcq_update_P_A_device warm-starts from: set by
    // every solve (launch_solve, the one-launch stream runs, whose last step writes them) and by mpcq_warm_start,
    // which stages its arguments there; cleared by every setup and by mpcq_cold_start (the update then starts cold)
    bool have_xy = false;
    DevBuf<double> d_sens;
    // order_ev orders a caller's stream after the context's last stream and back (order_after_last, order_last_after)
    hipEvent_t order_ev = nullptr;
    // mpcq_sensitivity_data*: the shared plant's partial sums, then the host form's gP, gA (grown on demand)
    DevBuf<double> d_sdata;
    // host copies of plant-0 scaling
    std::vector<double> hD, hE;
    double hc = 1.0;
};

// ---- context and results (mpcq_host_context.cpp)
enum Need { kNone, kGeneric, kAnySetup };
int check_ctx(mpcq_ctx *c, Need need);
int check_generic_dims(mpcq_ctx *c);
int ensure_plant_buffers(mpcq_ctx *c);
std::string polish_refusal(const char *fn);
int h2d(void *dst, const void *src, size_t bytes, hipStream_t s);
int d2h(mpcq_ctx *c, void *dst, const void *src, size_t bytes);
bool stream_capturing(hipStream_t s);
int refuse_capture(const char *fn, hipStream_t s);
int order_after_last(mpcq_ctx *c, hipStream_t s);
int order_last_after(mpcq_ctx *c, hipStream_t s);
int materialize_qu(mpcq_ctx *c);
int materialize_xy(mpcq_ctx *c);
int materialize_rho(mpcq_ctx *c);
int materialize_info(mpcq_ctx *c);

// ---- setup and data updates (mpcq_host_setup.cpp)
int reset_state(mpcq_ctx *c, bool reset_rho);
int setup_on_device(mpcq_ctx *c, hipStream_t s);
bool order_map_rows(int n, int m, int nx, const std::vector<double> &P, const std::vector<double> &A,
                    const std::vector<double> &Fx, const std::vector<double> &Fu, const std::vector<double> &Fr,
                    const std::vector<double> &Sb, const std::vector<double> &Ku, const std::vector<double> &W0,
                    std::vector<double> &map, std::vector<double> *G = nullptr);
int upload_order_map(mpcq_ctx *c, const std::vector<double> &map, hipStream_t s);
int build_order_map(mpcq_ctx *c);

// ---- solve (mpcq_host_solve.cpp)
struct PathChoice {
    int kind;    // MPCQ_PATH_*
    bool paired; // the tile kernel's paired loop
};
PathChoice choose_path(const mpcq_ctx *c);
mpcq::SolverSettings to_solver(const mpcq_settings &s);
template <typename T>
mpcq::AdmmArgs<T> make_args(mpcq_ctx *c);  // (instantiated for float and double)
int dump_tile_stamps(const char *path, const long long *d_stamps, size_t phases, size_t waves, hipStream_t s);
int dump_stamps(const char *path, const long long *d_stamps, size_t count, hipStream_t s);
void verbose_header(const mpcq_ctx *c, const char *what);
void verbose_solve(mpcq_ctx *c, double seconds);
int launch_solve(mpcq_ctx *c, hipStream_t s, bool mpc, const double *X, double *U, double xref);

// ---- MPC step and stream (mpcq_host_mpc.cpp)
int alloc_mpc_ops(mpcq_ctx *c, int nx);

// The MPC front end's operators in the context (AdmmArgs reads them, CondenseArgs writes them).
template <typename A>
void set_front_end_ops(const mpcq_ctx *c, A &a)
{
    a.Fx = c->d_Fx; a.Fu = c->d_Fu; a.Fr = c->d_Fr; a.Sbar = c->d_Sbar; a.Ku = c->d_Ku; a.W0 = c->d_W0;
}

// An MPC step's front end (q = Fx X + Fu U + Fr ref, u = W0 + Sbar X + Ku U, then U += x(0)); where q, u or the
// saved X, U go is the caller's choice.
template <typename T>
void set_mpc_front_end(const mpcq_ctx *c, mpcq::AdmmArgs<T> &a, const double *X, double *U, double xref)
{
    a.mpc = 1; a.mpc_u = 1; a.nx = c->nx; a.X = X; a.U = U; a.xref = xref;
    set_front_end_ops(c, a);
}

// ---- MIMO (mpcq_host_mimo.cpp)
// The MIMO setup's dims and operator blocks, on any of the per-QP argument structs (MimoArgs, MimoSensArgs,
// MimoPolishArgs, MimoPlantVjpArgs); those with s_rows add it themselves.
template <typename A>
void set_mimo_ops(const mpcq_ctx *c, A &a)
{
    a.batch = c->dims.batch;
    a.N = c->mimo.N; a.nx = c->mimo.nx; a.nu = c->mimo.nu; a.ny = c->mimo.ny;
    a.ops_stride = (size_t)mpcq::MimoLayout::make(a.N, a.nx, a.nu, a.ny).total;
    a.ops = c->mimo.ops;
}

// The device staging of one host-form call: one allocation handed out as consecutive typed sub-arrays.  The
// stream is waited for, whatever the outcome, before the staging goes away.
class Staging {
    DevBuf<double> d_;
    double *next_ = nullptr;
    hipStream_t s_;

public:
    explicit Staging(hipStream_t s) : s_(s) {}
    ~Staging() { (void)hipStreamSynchronize(s_); }
    int alloc(size_t doubles, const char *what)
    {
        const int rc = d_.alloc(8 * doubles, what);
        next_ = d_;
        return rc;
    }
    // The next `doubles` doubles, read as T (ints: two to a double, an odd count rounded up by the caller)
    template <typename T = double>
    T *take(size_t doubles)
    {
        double *p = next_;
        next_ += doubles;
        return (T *)p;
    }
};

#pragma GCC visibility pop

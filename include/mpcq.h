/*
 * include/mpcq.h — C ABI of the MI355X (gfx950) batched condensed-MPC QP solver.
 *
 * This is the drop-in boundary for the one hot path of LukeSchmitt96/solveMPC: the QP solve that
 * ModelPredictiveControlAPI performs through osqp-eigen (OsqpEigen::Solver, a member at
 * include/ModelPredictiveControlAPI.h:144).  Every entry point names the reference call it
 * replaces.  Conventions:
 *   - plain pointers and sizes; every function returns an int status, 0 == MPCQ_OK;
 *   - host buffers are caller-owned and only read/written during the call; device buffers are
 *     owned by the context;
 *   - matrices are dense, row-major, fp64 (the reference's c_float == double), QP-major across a
 *     batch: element (b, i, j) of a batch of r x c matrices sits at b*r*c + i*c + j;
 *   - one context per host thread; calls on one context are not re-entrant;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *
 * A context holds `batch` independent QPs of identical shape (n variables, m constraints).
 * They either share one plant (n_plants == 1: one P and A, e.g. 65,536 copies of the reference's
 * controller fed different states) or carry one plant each (n_plants == batch).
 */
#ifndef MPCQ_H
#define MPCQ_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes -------------------------------------------------------------------------- */
#define MPCQ_OK 0
#define MPCQ_ERR_ARG (-1)      /* bad argument / unsupported size                              */
#define MPCQ_ERR_HIP (-2)      /* HIP runtime error or no usable gfx950 device                 */
#define MPCQ_ERR_SETUP (-3)    /* setup rejected the data (P not PSD / KKT not quasi-definite) */
#define MPCQ_ERR_ORDER (-4)    /* call order (e.g. solve before setup)                         */
#define MPCQ_ERR_BOUNDS (-5)   /* some u < l (osqp_update_*_bound failure)                     */

/* ---- per-QP status (OSQP v0.6 values; osqp-eigen's solve() is true only for SOLVED) ------- */
#define MPCQ_SOLVED 1
#define MPCQ_SOLVED_INACCURATE 2
#define MPCQ_PRIMAL_INFEASIBLE_INACCURATE 3
#define MPCQ_DUAL_INFEASIBLE_INACCURATE 4
#define MPCQ_MAX_ITER_REACHED (-2)
#define MPCQ_PRIMAL_INFEASIBLE (-3)
#define MPCQ_DUAL_INFEASIBLE (-4)
#define MPCQ_NON_CVX (-7)
#define MPCQ_UNSOLVED (-10)
#define MPCQ_INVALID_BOUNDS (-20) /* this QP's u < l: update rejected, not solved              */
#define MPCQ_TYPE_CHANGED (-21)   /* this QP's bounds changed a row's OSQP constraint type
                                     (equality/inequality/free) away from its plant's setup;
                                     re-run mpcq_setup with these bounds                     */

/* ---- precision of the device iterate ------------------------------------------------------- */
#define MPCQ_F64 0 /* fp64 throughout (the reference's precision)                            */
#define MPCQ_F32 1 /* fp32 ADMM iterate, fp64 setup.  Bound: where OSQP certifies primal
                      infeasibility an fp32 iterate may not (the dual iterate of an infeasible QP
                      grows without bound and its fp32 rounding moves the certificate's
                      ||A' dy|| / ||dy|| past eps_prim_inf), and the QP then runs to max_iter:
                      MPCQ_MAX_ITER_REACHED, or MPCQ_SOLVED_INACCURATE where OSQP's approximate
                      check passes there, instead of MPCQ_PRIMAL_INFEASIBLE (never MPCQ_SOLVED;
                      osqp-eigen's solve() is false either way).  MPCQ_F64 and MPCQ_F64_MIXED
                      return OSQP's status (tests/test_gpu.py test_infeasible_statuses_match_oracle) */
#define MPCQ_F64_MIXED 2 /* fp64 state, checks and solution; on the shared-plant tile path the plain
                            iterations before the last MPCQ_MIX_R of every check interval run in fp32
                            (MFMA f32 products), which the fp64 ones damp; every
                            other path is MPCQ_F64                                               */
#define MPCQ_MIX_R 5

/* OSQP v0.6 settings (osqp constants.h defaults via mpcq_default_settings).  Replaces
 * OsqpEigen::Settings as used at ModelPredictiveControlAPI.cpp:51-52 (setVerbosity,
 * setWarmStart(true)).
 * polish (off by default, as the reference leaves it): OSQP's solution polishing (polish.c) of every QP
 * that ended MPCQ_SOLVED, run on the device after the ADMM in fp64 whatever the context's dtype: the
 * active set is guessed from the final iterate, the delta-regularised reduced KKT system is solved with
 * polish_refine_iter steps of iterative refinement, and the polished (x, y) replaces the ADMM's where it
 * reduces the residuals (mpcq_get_polish_info).  mpcq_solve, mpcq_mpc_step_device and mpcq_mpc_step honour
 * it; the contexts it serves have n <= 32 and m <= 64 (mpcq_create refuses larger ones with polish set),
 * and the single-launch entry points (mpcq_mpc_run_device, mpcq_mpc_plants_step_device, mpcq_mimo_*), which
 * cannot fit a second pass, return MPCQ_ERR_ARG on a context whose polish is set.  With polish == 0 every
 * code path, launch and result is what it is without the setting.  A MIMO context (n up to 128) is polished by an
 * entry point of its own, mpcq_mimo_step_polish_device, on a context whose polish is 0; polish_refine_iter and
 * delta are its settings too. */
typedef struct mpcq_settings {
    double rho, sigma, alpha;
    double eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
    double adaptive_rho_tolerance, adaptive_rho_fraction;
    int max_iter, check_termination, scaling, adaptive_rho, adaptive_rho_interval;
    int warm_start, scaled_termination, verbose;
    int polish;             /* 0 (default) / 1                                                */
    int polish_refine_iter; /* iterative refinement steps of the polish solve (default 3)    */
    double delta;           /* regularisation of the polish KKT system (default 1e-6)        */
} mpcq_settings;

typedef struct mpcq_dims {
    int n;        /* decision variables  (setNumberOfVariables, :54)   */
    int m;        /* constraint rows     (setNumberOfConstraints, :55) */
    int batch;    /* QPs in this context (reference: 1)                */
    int n_plants; /* 1 (shared P, A) or batch (one plant per QP)       */
    int dtype;    /* MPCQ_F64, MPCQ_F32 or MPCQ_F64_MIXED              */
    int device;   /* HIP device ordinal                                */
} mpcq_dims;

typedef struct mpcq_ctx mpcq_ctx;

/* Device-resident views of a context's buffers (fp64, QP-major), for zero-copy callers.
 * The pointers never change, but the OUTPUTS (x, y, status, iter, rho) are published lazily on the
 * shared-plant tile path: a solve leaves them in its warm state and they are formed
 * from it when something reads them.  mpcq_device_view_get is such a read: the output arrays hold the
 * last solve's values only after mpcq_device_view_get has been called AFTER that solve (call it again
 * after every mpcq_solve / mpcq_mpc_step_device / graph replay), and they are written by kernels
 * enqueued on the context's last stream (the stream of its last solve), so a reader on another stream
 * must order itself after that stream (an event) or synchronise it.  A view fetched once and re-read
 * after later solves shows an older solve's outputs.  The inputs (q, u, l) follow the same rule. */
typedef struct mpcq_device_view {
    double *q;     /* batch*n   gradient (input of the next solve)      */
    double *u;     /* batch*m   upper bounds                            */
    double *l;     /* batch*m   lower bounds                            */
    double *x;     /* batch*n   unscaled primal solution (output)       */
    double *y;     /* batch*m   unscaled dual solution (output)         */
    int *status;   /* batch     MPCQ_* status (output)                  */
    int *iter;     /* batch     ADMM iterations (output)                */
    double *rho;   /* batch     rho after the solve (output)            */
} mpcq_device_view;

void mpcq_default_settings(mpcq_settings *s);

/* Allocate a context on dims->device.  Fails with MPCQ_ERR_HIP when no gfx950 device exists. */
int mpcq_create(const mpcq_dims *dims, const mpcq_settings *settings, mpcq_ctx **out);
int mpcq_destroy(mpcq_ctx *ctx);

/* Setup: replaces setHessianMatrix / setGradient / setLinearConstraintsMatrix / setLowerBound /
 * setUpperBound + initSolver (ModelPredictiveControlAPI.cpp:57-64 -> osqp_setup).  Arrays are per
 * plant (n_plants copies): P n*n (upper triangle read, as osqp-eigen does), q0 n, A m*n, l0/u0 m.
 * Ruiz equilibration, cost scaling and the KKT factorisation run on the device.  q0/l0/u0 also
 * become the current q/l/u of every QP of the plant. */
int mpcq_setup(mpcq_ctx *ctx, const double *P, const double *q0, const double *A,
               const double *l0, const double *u0);

/* Per-QP data updates from host memory (batch*n or batch*m).
 * Replace OsqpEigen::Solver::updateGradient (:96 -> osqp_update_lin_cost) and
 * updateUpperBound (:99 -> osqp_update_upper_bound); lower/both-bound forms for completeness.
 * Bounds are validated per QP when the solve runs (status MPCQ_INVALID_BOUNDS). */
int mpcq_update_lin_cost(mpcq_ctx *ctx, const double *q);
int mpcq_update_upper_bound(mpcq_ctx *ctx, const double *u);
int mpcq_update_lower_bound(mpcq_ctx *ctx, const double *l);
int mpcq_update_bounds(mpcq_ctx *ctx, const double *l, const double *u);

/* osqp_warm_start / cold_start for every QP (x batch*n, y batch*m, unscaled). */
int mpcq_warm_start(mpcq_ctx *ctx, const double *x, const double *y);
int mpcq_cold_start(mpcq_ctx *ctx);

/* New matrices for a context that is set up: osqp_update_P / osqp_update_A / osqp_update_P_A (osqp-eigen's
 * updateHessianMatrix / updateLinearConstraintsMatrix), from device memory, with a warm start.
 * P_dev: n_plants*n*n (upper triangle read, as mpcq_setup), A_dev: n_plants*m*n, fp64 device pointers; either may
 * be NULL, which keeps the context's current matrix.  Serves a context set up by mpcq_setup or
 * mpcq_mpc_setup_plants_device: shared-plant and per-plant, every dtype and solve path.  Runs on `stream`, ordered
 * after the context's last stream (an event), and becomes the context's last stream: the next solve is ordered
 * after it.  The only host transfer is the setup's flag word with plant 0's operator block, as in
 * mpcq_mpc_setup_plants_device.
 * Afterwards, for both values of `rescale`:
 *   - every QP keeps its current q, l, u (a tile-path step's lazy q, u are formed first); nothing is re-broadcast
 *     from the setup's q0, l0, u0, which still give the constraint types and the q0 the cost scaling sees;
 *   - the next solve starts from the previous unscaled (x, y) exactly as mpcq_warm_start(x_prev, y_prev) would
 *     install them under the new matrices and scaling (x^ = D^-1 x, y^ = c E^-1 y, z^ = A^ x^); a QP whose previous
 *     x or y holds a non-finite entry (infeasible, non-convex) starts cold (x = z = y = 0).  The previous (x, y)
 *     are those of the context's last solve, a stream run (mpcq_mpc_run*_device: its last control step) included,
 *     or the arguments of a later mpcq_warm_start.  A context that has not solved or been warm-started since its
 *     setup, or since its last mpcq_cold_start, starts cold as a whole: a cold start asked for before the update
 *     stands.  A pending mpcq_reset still applies to the next solve;
 *   - every QP's rho is settings.rho again.  A stated deviation: OSQP keeps rho_vec and leaves its iterates in the
 *     old scaled coordinates, neither of which means anything across a new scaling;
 *   - the outputs (x, y, status, iter, rho) keep the last solve's values until the next solve;
 *     mpcq_get_polish_info reports "not performed", mpcq_sensitivity* return MPCQ_ERR_ORDER until then;
 *   - the MPC operators (Fx .. W0) and the stream plant are kept: a caller whose plant changed calls
 *     mpcq_mpc_set_operators as before.  The hardest-first order map follows the new matrices.
 * rescale = 1 (OSQP's behaviour): scale_data and the KKT basis run again on the new matrices with the setup's q0:
 *   the setup kernels of mpcq_setup on the new data; every generic shape.
 * rescale = 0 (the fast path): D, E, c, the rows' rho scales and constraint types stay bit for bit what the
 *   last setup left (mpcq_get_scaling returns the same bits); only the factor stage is rebuilt (Cholesky, Jacobi
 *   eigen-basis and operator products of a shared plant; M(rho) and its inverse per plant), one wavefront per
 *   plant.  The new matrices are scaled once, each product rounded left to right in fp64:
 *     P^_ij = (D_i * (c * P_ij)) * D_j      (P symmetrised from its upper triangle first)
 *     A^_ij = (E_i * A_ij) * D_j
 *   Needs n <= 32 and m <= 64.
 * MPCQ_ERR_ORDER: no setup yet, or after mpcq_mpc_plants_step_device.  MPCQ_ERR_ARG: both matrices NULL (on a
 * context with m == 0, which has no A: P NULL); a MIMO
 * context; rescale not 0 or 1; rescale = 0 with n > 32 or m > 64; `stream` under graph capture.  A refused call
 * writes nothing.  MPCQ_ERR_SETUP: the new P^ + sigma I (+ rho A^'A^) is not positive definite; the context then
 * needs mpcq_setup (solves return MPCQ_ERR_ORDER), as OSQP's workspace is unusable after a failed update. */
int mpcq_update_P_A_device(mpcq_ctx *ctx, const double *P_dev, const double *A_dev, int rescale, void *stream);
/* Host-memory form (copies in on the context's last stream, synchronises). */
int mpcq_update_P_A(mpcq_ctx *ctx, const double *P, const double *A, int rescale);

/* Return every QP to the state right after setup (x = z = y = 0, rho = settings.rho), as
 * re-running initSolver (:64) would; applied by the next solve at no cost. */
int mpcq_reset(mpcq_ctx *ctx);

/* Solve every QP (replaces OsqpEigen::Solver::solve, :102 -> osqp_solve).  Asynchronous on
 * `stream`; iterates stay on the device (warm start, :52). */
int mpcq_solve(mpcq_ctx *ctx, void *stream);

/* Results (synchronise the context's last stream).  Replace getSolution() (:105). */
int mpcq_get_solution(mpcq_ctx *ctx, double *x);            /* batch*n */
int mpcq_get_dual(mpcq_ctx *ctx, double *y);                /* batch*m */
int mpcq_get_info(mpcq_ctx *ctx, int *status, int *iter, double *rho); /* each batch, may be NULL */
int mpcq_get_scaling(mpcq_ctx *ctx, double *D, double *E, double *c); /* plant 0: n, m, 1 */
/* Polish outcome of the last solve (OSQP info->status_polish and the polished residuals; synchronises).
 * Each argument is a host array of `batch` entries and may be NULL.  status_polish: 1 successful,
 * -1 unsuccessful (the ADMM solution was kept), 0 not performed (settings.polish == 0 and the last step was not
 * a mpcq_mimo_step_polish_device, or the QP did not end MPCQ_SOLVED); n_active: rows of the reduced KKT system
 * (lower-active + upper-active); pri_res,
 * dua_res: residuals of the returned solution in the termination norm (unscaled unless
 * scaled_termination), NaN where status_polish == 0. */
int mpcq_get_polish_info(mpcq_ctx *ctx, int *status_polish, int *n_active, double *pri_res, double *dua_res);

/* Device path the next solve takes (no OSQP counterpart; for benchmarks and tests):
 * *kind = MPCQ_PATH_TILE (shared plant, MFMA tile kernel's phase chain), MPCQ_PATH_WAVE
 * (one QP per wave: per-plant contexts, and shared-plant batches under 8,192 QPs) or MPCQ_PATH_LANE
 * (one QP per lane); *paired = 1 when the tile kernel runs its paired loop (rows n + j of A are the
 * negated rows j: the condensed-MPC constraint matrix). */
#define MPCQ_PATH_TILE 0
#define MPCQ_PATH_WAVE 1
#define MPCQ_PATH_LANE 2
int mpcq_get_path(mpcq_ctx *ctx, int *kind, int *paired);

/* Fill *view and publish the last solve's pending outputs into it (see mpcq_device_view above). */
int mpcq_device_view_get(mpcq_ctx *ctx, mpcq_device_view *view);

/* ---- condensed-MPC front end: ModelPredictiveControlAPI::controllerStep, batched ------------
 * Per-plant operators of the condensed problem (n == N, m == 2N; ModelPredictiveControlAPI.cpp
 * setFVars :303-307, setUpperBound :360-369, setTransformations :185,208): Fx N*nx, Fu N,
 * Fr N*N, Sbar m*nx, Ku m, W0 m (n_plants copies each). */
int mpcq_mpc_set_operators(mpcq_ctx *ctx, int nx, const double *Fx, const double *Fu,
                           const double *Fr, const double *Sbar, const double *Ku,
                           const double *W0);
/* One receding-horizon step for every QP, on device-resident X (batch*nx) and U (batch):
 *   q = Fx X + Fu U + Fr (xref 1)          (setF :372-375, updateRef :378-380)
 *   u = W0 + Sbar X + Ku U                 (:93-99)
 *   solve                                  (:102, warm-started)
 *   U += x[0] where status == SOLVED       (:105)
 * X_dev/U_dev are device pointers (fp64). */
int mpcq_mpc_step_device(mpcq_ctx *ctx, const double *X_dev, double *U_dev, double xref,
                         void *stream);

/* Host-memory convenience form of mpcq_mpc_step_device (copies in/out, synchronises). */
int mpcq_mpc_step(mpcq_ctx *ctx, const double *X, double *U, double xref);

/* ---- per-QP reference trajectories with horizon preview --------------------------------------
 * The reference drives one plant to one set-point (updateRef :378-380, ref = xref 1); a batch of
 * controllers has one set-point each, and a tracking controller wants its horizon to see a set-point
 * change before it arrives.  The condensed QP carries that already (Fr is the full N x N operator), so
 * these twins of the entry points above take the horizon reference itself.
 * One controllerStep for every QP with its own horizon reference:
 *   q_b = Fx X_b + Fu U_b + Fr ref_b,  ref_b[j] = ref_dev[b*ref_stride + j], j = 0..n-1.
 * ref_stride == 0: one n-vector shared by the batch; otherwise ref_stride >= n.
 * ref_dev is read-only for the call and must stay valid and unchanged until the solve has finished
 * on `stream` (later phases of a tile solve re-form q from it, as they do from X).
 * Arithmetic: q_v = s0 + s1 + s2 with s0, s1 as in mpcq_mpc_step_device and s2 = sum_t Fr[v,t] ref[t]
 * accumulated in ascending t in fp64, the form of the scalar entry point's row sum, so a reference whose
 * entries all equal xref reproduces mpcq_mpc_step_device bit for bit on every device path and dtype.
 * Every path of mpcq_mpc_step_device is served (tile kernel, one QP per wave, one QP per lane), with its
 * hardest-first order (the key gains -A P^-1 Fr ref_b: still the key of the QP's actual q) and
 * settings.polish.  q and u are written eagerly on this path (no lazy q/u): mpcq_device_view_get().q and
 * a following mpcq_solve see this step's q even after the caller has overwritten ref_dev.
 * Returns MPCQ_ERR_ARG for a null ref or a non-zero stride < n, otherwise as mpcq_mpc_step_device.
 * Out of scope: mpcq_mpc_plants_step_device.  A MIMO context has twins of its own, mpcq_mimo_step_ref*. */
int mpcq_mpc_step_ref_device(mpcq_ctx *ctx, const double *X_dev, double *U_dev, const double *ref_dev,
                             long long ref_stride, void *stream);
/* Host-memory form (copies in/out, synchronises), as mpcq_mpc_step is to mpcq_mpc_step_device. */
int mpcq_mpc_step_ref(mpcq_ctx *ctx, const double *X, double *U, const double *ref, long long ref_stride);

/* ---- active-set sensitivities of the last solve (no OSQP counterpart) -----------
 * How x* moves with the QP's data at the active set of the last solve's final iterate.  Per QP, with the
 * active rows taken by the polish rule on the scaled iterate (lower-active when z^ - l^ < -y^, otherwise
 * upper-active when u^ - z^ < y^; lower rows first, then upper rows), A_a those rows of A and
 * K = [P, A_a'; A_a, 0] (P symmetrised from its upper triangle): for a cotangent g = dL/dx* (n entries),
 * K [v; w] = [g; 0] and
 *   gq = -v                                    (dL/dq, n entries)
 *   gl[i] = w_k where row i is the k-th reduced row and lower-active, else 0   (dL/dl)
 *   gu[i] = w_k where row i is upper-active, else 0                            (dL/du)
 * the vector-Jacobian product of x*(q, l, u) at a fixed active set.  Solved on the device in fp64 whatever
 * the context's dtype, in the scaled space, with settings.delta and settings.polish_refine_iter as the polish
 * pass uses them; the contract is the solution of the unregularised system.  n_active: rows of the reduced
 * system.  A QP that did not end MPCQ_SOLVED (or whose reduced system could not be factored) gets all-zero
 * gradients and n_active = -1.  With settings.polish the active set is that of the polished iterate.
 * g_dev: batch*n cotangents (device, fp64), or NULL for g = e_0 (the applied move x*[0]) in every QP.  The
 * outputs are device arrays gq batch*n, gl batch*m, gu batch*m, n_active batch; each may be NULL, not all.
 * Serves the last mpcq_solve / mpcq_mpc_step(_device) / mpcq_mpc_step_ref(_device) of shared-plant and
 * per-plant contexts, every dtype and device path.  Read-only on the context: a call between two solves
 * leaves the second solve bit-identical.  The kernel runs on `stream`, ordered after the context's last
 * stream (an event; see mpcq_device_view above), and the context's next solve is ordered after it.
 * MPCQ_ERR_ORDER: no solve since the last setup, data update, warm / cold start or reset; after
 * mpcq_mpc_plants_step_device (no operators are kept); after a stream run (mpcq_mpc_run*_device).
 * MPCQ_ERR_ARG: n > 32 or m > 64; a MIMO context; every output NULL; `stream` under graph capture (nothing
 * is recorded into the capture).  A refused call writes nothing. */
int mpcq_sensitivity_device(mpcq_ctx *ctx, const double *g_dev, double *gq_dev, double *gl_dev, double *gu_dev,
                            int *n_active_dev, void *stream);
/* Host-memory form (copies in/out, synchronises); the same arrays on the host. */
int mpcq_sensitivity(mpcq_ctx *ctx, const double *g, double *gq, double *gl, double *gu, int *n_active);
/* The same call with the gradients with respect to the QP's matrices and the active sets.  With
 * x, y the solution and dual the solve returned (mpcq_get_solution, mpcq_get_dual), y_a = y on the active rows
 * and 0 elsewhere, and w = gl + gu:
 *   gP = 1/2 (gq x' + x gq')    n*n, row-major, symmetric   (dL/dP)
 *   gA = y_a gq' - w x'         m*n, row-major, zero on inactive rows   (dL/dA)
 * gP is the gradient with respect to a symmetric P: a caller who parametrises only the upper triangle that
 * mpcq_setup reads takes gP[i][j] + gP[j][i] for i < j (and gP[i][i] on the diagonal).
 * A context with n_plants == batch gets one pair per QP (gP batch*n*n, gA batch*m*n; zeros where n_active = -1);
 * a shared-plant context gets the sums over the batch (gP n*n, gA m*n).  QPs with n_active = -1 are left out of
 * the sums (their x may be NaN; nothing of them is read).  The sums are formed in a fixed order that depends
 * on the batch alone (chunks of 256 QPs, added in ascending order; no atomics): two calls give identical bits.
 * active: batch*2 words; word 2b holds the lower-active rows of QP b as a bit mask (bit i: row i), word 2b + 1
 * the upper-active rows; both 0 where n_active = -1.
 * Each of the seven outputs may be NULL, not all.  With gP, gA and active all NULL the call is
 * mpcq_sensitivity_device, bit for bit.  Preconditions, refusals, stream ordering and the read-only guarantee
 * are those of mpcq_sensitivity_device; like mpcq_device_view_get the call may first publish the lazily kept
 * x, y of a tile-path solve (on the context's last stream).  Whatever the contraction reads and the caller
 * passed as NULL (gq, gl, gu, the masks, n_active) and the partial sums live in staging owned by the context. */
int mpcq_sensitivity_data_device(mpcq_ctx *ctx, const double *g_dev, double *gq_dev, double *gl_dev, double *gu_dev,
                                 double *gP_dev, double *gA_dev, unsigned long long *active_dev, int *n_active_dev,
                                 void *stream);
/* Host-memory form (copies in/out, synchronises); the same arrays on the host. */
int mpcq_sensitivity_data(mpcq_ctx *ctx, const double *g, double *gq, double *gl, double *gu, double *gP, double *gA,
                          unsigned long long *active, int *n_active);
/* Step gains of the condensed-MPC front end: the gradient of the applied move x*[0] (g = e_0) with respect to
 * the last step's X, previous U and horizon reference, by the chain rule through q = Fx X + Fu U + Fr ref and
 * u = W0 + Sbar X + Ku U:
 *   dX = Fx' gq + Sbar' gu (batch*nx),  dU = Fu' gq + Ku' gu (batch),  dref = Fr' gq (batch*n)
 * from the context's operators (shared or per plant), fp64 sums in ascending row index: the explicit-MPC
 * feedback gain at the current active set.  After a scalar-xref step the gain with respect to xref is the
 * sum of dref's entries.  Outputs are device arrays; each may be NULL, not all.  As mpcq_sensitivity_device
 * otherwise; also MPCQ_ERR_ARG when the context has no MPC operators (mpcq_mpc_set_operators). */
int mpcq_mpc_step_gains_device(mpcq_ctx *ctx, double *dX_dev, double *dU_dev, double *dref_dev, int *n_active_dev,
                               void *stream);
/* Host-memory form (synchronises). */
int mpcq_mpc_step_gains(mpcq_ctx *ctx, double *dX, double *dU, double *dref, int *n_active);

/* ---- receding-horizon stream (BASELINE config 5; the solver.cpp loop, solver.cpp:43-74, with the
 * serial plant replaced by a simulated one) ----------------------------------------------------
 * Plant of every QP: X <- Ad X + Bd U + w,  w ~ N(0, noise_std^2 I) drawn from a counter-based
 * generator keyed by (seed, global QP index first_qp + b, step, component) — the same stream on any
 * sharding of the batch (solvempc_amd/workload.py restates it).  Ad nx*nx, Bd nx per plant. */
int mpcq_mpc_set_plant(mpcq_ctx *ctx, int nx, const double *Ad, const double *Bd);
/* One plant update on device-resident X (batch*nx) / U (batch); `step` selects the noise draw. */
int mpcq_mpc_simulate_device(mpcq_ctx *ctx, double *X_dev, const double *U_dev, unsigned long long seed,
                             long long first_qp, long long step, double noise_std, void *stream);
/* `steps` warm-started control steps  [controllerStep (:81-108) ; plant update]  for every QP
 * (steps first_step .. first_step+steps-1); X_dev/U_dev evolve in place.  One launch runs every
 * step: the tile kernel's stream mode for a shared plant of the condensed-MPC shape (each MFMA
 * column one plant), else one QP per wave; other shapes replay a hipGraph of per-step launches.
 * `stream` must not be the NULL stream (graph capture). */
int mpcq_mpc_run_device(mpcq_ctx *ctx, double *X_dev, double *U_dev, double xref, int steps,
                        unsigned long long seed, long long first_qp, long long first_step,
                        double noise_std, void *stream);
/* mpcq_mpc_run_device with a reference schedule: the control step with absolute index
 * s = first_step + k uses ref_b[j] = sched_dev[b*sched_stride + min(s + j, sched_len - 1)]
 * (the last value is held).  sched_stride == 0: one schedule shared by the batch; else >= sched_len.
 * b is the context's local QP index (a shard passes its own rows).  sched_len >= 1, first_step >= 0.
 * The window slides inside the one-launch stream kernels (a column or wave starting its step k loads
 * the window at first_step + k); the per-step graph takes the step from the context's device step
 * counter, as its captured plant simulation does.  sched_dev must stay valid and unchanged until the
 * stream has finished.  Afterwards q, u are the last step's.  MPCQ_ERR_ARG: null schedule, sched_len < 1,
 * a non-zero stride < sched_len, first_step < 0, or settings.polish set (as mpcq_mpc_run_device). */
int mpcq_mpc_run_ref_device(mpcq_ctx *ctx, double *X_dev, double *U_dev, const double *sched_dev,
                            int sched_len, long long sched_stride, int steps, unsigned long long seed,
                            long long first_qp, long long first_step, double noise_std, void *stream);
/* How the last mpcq_mpc_run_device call ran (benchmarks and tests): MPCQ_STREAM_TILE (one tile-kernel
 * launch), MPCQ_STREAM_WAVE (one one-QP-per-wave launch) or MPCQ_STREAM_GRAPH (per-step launches). */
#define MPCQ_STREAM_GRAPH 0
#define MPCQ_STREAM_WAVE 1
#define MPCQ_STREAM_TILE 2
int mpcq_get_stream_path(mpcq_ctx *ctx, int *kind);
/* Hardest-first order of the last solve (benchmarks and tests): *ordered = 1 when it
 * was a tile-path MPC step or a one-pass distinct-plants step (mpcq_mpc_plants_step_device; the key from the
 * batch's first plant) run in ascending |max_j (A x_u - u)_j| (x_u = -P^-1 q, the QP's unconstrained
 * optimum; binned 16 per octave), else 0; order (batch ints, or NULL) receives that step's QPs in the
 * order it ran them (synchronises).  The order changes no result. */
int mpcq_get_order(mpcq_ctx *ctx, int *ordered, int *order);
/* Per-QP counters of the last mpcq_mpc_run_device call (host arrays of `batch` ints, synchronises):
 * the ADMM iterations of all its control steps, and the steps whose solve did not end SOLVED
 * (controllerStep returning false, :102, where the reference's loop would exit, solver.cpp:50).
 * The per-step values behind these sums: mpcq_mpc_set_stream_log below. */
int mpcq_mpc_stream_counters(mpcq_ctx *ctx, int *iters, int *unsolved);

/* Per-step record of a receding-horizon stream.  Device pointers, caller-owned, fp64/int32, step-major:
 * row r holds what the batch looked like after the control step with absolute index step0 + r:
 *   U      [r*batch + b]            U_b after that step's controllerStep (the control the plant then sees;
 *                                   unchanged from the row before where the step did not end SOLVED)
 *   X      [(r*batch + b)*nx + i]   X_b after that step's plant update (what the next step measures)
 *   status [r*batch + b]            MPCQ_* status of that step's solve
 *   iter   [r*batch + b]            its ADMM iterations
 * Any of the four may be NULL (not recorded).  b is the context's local QP index. */
typedef struct mpcq_stream_log {
    double *U, *X;
    int *status, *iter;
    long long rows;   /* capacity in control steps */
    long long step0;  /* absolute control step stored in row 0 */
} mpcq_stream_log;

/* Attach (or with log == NULL / all four pointers NULL: detach) a record to the context.  It applies to
 * every later mpcq_mpc_run_device / mpcq_mpc_run_ref_device call until it is detached, on all three stream
 * paths (tile stream, one QP per wave, per-step graph) and every dtype: the call's k-th control step fills
 * row first_step + k - step0, so chunked runs (first_step = 0, 7, 12, ...) fill one buffer.  The rows are
 * exactly the X_dev / U_dev / mpcq_get_info values that steps = 1 calls would have shown after each step, bit
 * for bit.  The one-launch stream kernels write them from their once-per-control-step code (additional kernel
 * variants: without a record every launch, kernel and result is what it is otherwise); the per-step graph
 * captures a small record kernel after each plant update.  The buffers are written by the kernels of the
 * run's `stream` and must stay valid until that stream has finished.
 * MPCQ_ERR_ARG: a pointer is set and rows < 1 or step0 < 0.  A run returns MPCQ_ERR_ARG, before anything is
 * enqueued (X_dev, U_dev, the counters and the buffers untouched), when any of its rows would fall outside
 * [0, rows).  Not served: mpcq_mpc_plants_step_device; a MIMO run takes a record of its own as an argument
 * (mpcq_mimo_log, mpcq_mimo_run_device). */
int mpcq_mpc_set_stream_log(mpcq_ctx *ctx, const mpcq_stream_log *log);

/* Condensed-QP construction on device `device` for n_plants SISO plants (ModelPredictiveControlAPI
 * setTransformations / setLL / setLiftedCosts / setH / setFVars / setLinearConstraints /
 * setUpperBound, src/ModelPredictiveControlAPI.cpp:158-369).  Inputs per plant: Ad nx*nx, Bd nx,
 * Cd nx, K nx, Q, R, RD (scalars); N = horizon; s_rows = rows of S filled with K (reference: 10,
 * :185).  Outputs per plant (host memory, caller-allocated): P N*N, A 2N*N, Fx N*nx, Fu N, Fr N*N,
 * Sbar 2N*nx, Ku 2N, W0 2N.  nx <= 8. */
int mpcq_condense(int device, int n_plants, int nx, int N, int s_rows, const double *Ad,
                  const double *Bd, const double *Cd, const double *K, const double *Q,
                  const double *R, const double *RD, double *P, double *A, double *Fx, double *Fu,
                  double *Fr, double *Sbar, double *Ku, double *W0);

/* Reverse of mpcq_condense: cotangents of the condensed operators -> cotangents of the plant
 * data, the vector-Jacobian product of the condensing.  All pointers are device pointers, fp64, plant-major
 * (n_plants copies); Ad .. RD as mpcq_condense reads them, gP .. gKu of the shapes of its outputs P, A, Fx, Fu, Fr,
 * Sbar, Ku (each may be NULL = 0, not all), gAd .. gRD of the shapes of Ad .. RD (each may be NULL, not all).
 * With L the lower-triangular ones, r_k = Cd Ad^k, S(i,j) = sum_(k <= i-j) r_k Bd for j <= i (else 0) and
 * Sx(i) = r_(i+1) as the condensing forms them, and Ps = gP + gP':
 *   gR  = <Ps, L'L> + 2 sum gFu             gRD = tr Ps
 *   gQ  = <Ps, S'S> + 2 gFu.(S(:,0)'S) - 2 <gFr, S'> + 2 <gFx, S'Sx>
 *   GS  = 2Q S Ps + 2Q S(:,0) gFu' - 2Q gFr' + 2Q Sx gFx',  GS(:,0) += 2Q S gFu     (its lower triangle is used)
 *   GSx = 2Q S gFx
 *   Gc_d = sum_(i-j = d) GS(i,j),  GCAB_k = sum_(d >= k) Gc_d,  gBd = sum_(k < N) GCAB_k r_k'
 *   rho_k = GCAB_k Bd' (k < N) + GSx(k-1) (k >= 1);  for k = N .. 1:  gAd += r_(k-1)' rho_k,
 *   rho_(k-1) += rho_k Ad';  gCd = rho_0
 *   gK[c] = sum_(i < min(s_rows, N)) (gSbar(i,c) - gSbar(N+i,c));  gK[0] also receives
 *   sum_(j <= i) (gA(i,j) - gA(N+i,j)) - sum_(i < N) gKu[i] + sum_(i < N) gKu[N+i]
 * W0 is constant and has no cotangent.  gP is the cotangent of the full symmetric P that mpcq_condense writes
 * (the convention of mpcq_sensitivity_data's gP).  Stateless: no context is touched.  One wavefront per plant,
 * fp64, no atomics, sums in a fixed order: two calls give identical bits, and the outputs asked for do not
 * depend on which others are NULL.  The kernel runs on `stream` of device `device`.
 * MPCQ_ERR_ARG, with nothing written: N < 1 or N > 32, nx < 1 or nx > 8, s_rows < 0, n_plants < 1; a NULL plant
 * array; every cotangent NULL or every output NULL; `stream` under graph capture. */
int mpcq_condense_vjp_device(int device, int n_plants, int nx, int N, int s_rows, const double *Ad, const double *Bd,
                             const double *Cd, const double *K, const double *Q, const double *R, const double *RD,
                             const double *gP, const double *gA, const double *gFx, const double *gFu,
                             const double *gFr, const double *gSbar, const double *gKu, double *gAd, double *gBd,
                             double *gCd, double *gK, double *gQ, double *gR, double *gRD, void *stream);
/* Host-memory form (copies in/out, synchronises); the same arrays on the host. */
int mpcq_condense_vjp(int device, int n_plants, int nx, int N, int s_rows, const double *Ad, const double *Bd,
                      const double *Cd, const double *K, const double *Q, const double *R, const double *RD,
                      const double *gP, const double *gA, const double *gFx, const double *gFu, const double *gFr,
                      const double *gSbar, const double *gKu, double *gAd, double *gBd, double *gCd, double *gK,
                      double *gQ, double *gR, double *gRD);

/* Per-plant condensing + setup on the device (BASELINE config 3): every plant of the context
 * (n_plants copies, device pointers, plant-major: Ad nx*nx, Bd nx, Cd nx, K nx, Q, R, RD) is
 * condensed as mpcq_condense does, its front-end operators installed (as mpcq_mpc_set_operators)
 * and the solver set up on the ctor's data (as mpcq_setup with q0 = 0, l0 = -DBL_MAX, u0 = W0:
 * ModelPredictiveControlAPI.cpp:22-23,38-43,51-64), all on `stream`; the only host transfer is
 * the setup's status word.  Needs n == N, m == 2N. */
int mpcq_mpc_setup_plants_device(mpcq_ctx *ctx, int nx, int s_rows, const double *Ad,
                                 const double *Bd, const double *Cd, const double *K,
                                 const double *Q, const double *R, const double *RD, void *stream);

/* Per-plant batch in one pass (BASELINE config 3): for every plant the reference's constructor
 * (condensing + osqp_setup on the ctor's data, X = U = 0: :3-65) and one controllerStep (:81-108) from
 * device-resident X (batch*nx) and U (batch; U += x[0] when SOLVED) — the work of
 * mpcq_mpc_setup_plants_device followed by mpcq_mpc_step_device, with each plant's operators kept on
 * chip instead of written to the context.  Plant arrays as in mpcq_mpc_setup_plants_device.
 * Afterwards the context holds this step's solution, dual, status, iterations and rho; it holds no
 * operators, so further solves need mpcq_mpc_setup_plants_device / mpcq_setup first (MPCQ_ERR_ORDER
 * otherwise).  Asynchronous on `stream`; a plant whose KKT matrix is not positive definite ends
 * MPCQ_NON_CVX.  Needs n == N <= 32, m == 2N, n_plants == batch, nx <= 8. */
int mpcq_mpc_plants_step_device(mpcq_ctx *ctx, int nx, int s_rows, const double *Ad, const double *Bd,
                                const double *Cd, const double *K, const double *Q, const double *R,
                                const double *RD, const double *X, double *U, double xref, void *stream);

/* ---- MIMO condensed MPC (BASELINE config 4: quad-rotor hover linearisations, n_x 12, n_u 4, N 30) --
 * The reference's condensing (ModelPredictiveControlAPI.cpp:158-369) with every SISO scalar a block
 * (oracle/mpc_mimo.h): decision du in R^(N n_u), A = [L (x) K0; -(L (x) K0)], u = W0 + Sbar X + Ku U,
 * l = -DBL_MAX.  The context must have n_plants == batch, n = N n_u (<= 128), m = 2n, dtype MPCQ_F64;
 * n_u in {1, 2, 4}, n_x, n_y <= 12, N <= 32.
 * Setup (replaces the ctor :3-65 + initSolver :64 per plant) from device-resident plant data,
 * plant-major fp64: Ad nx*nx, Bd nx*nu, Cd ny*nx, Q ny*ny (symmetric), R nu*nu, RD nu*nu, K nu*nx,
 * K0 nu*nu, w0 nu; S = K on block rows k < s_rows.  Condensing, Ruiz scaling and P^ on the device;
 * the solver state is reset (x = z = y = 0, rho = settings.rho). */
int mpcq_mimo_setup_plants_device(mpcq_ctx *ctx, int nx, int nu, int ny, int s_rows, const double *Ad,
                                  const double *Bd, const double *Cd, const double *Q, const double *R,
                                  const double *RD, const double *K, const double *K0, const double *w0,
                                  void *stream);
/* One controllerStep (:81-108) for every QP on device-resident X (batch*nx) and U (batch*nu):
 * q = Fx X + Fu U + Fr (1_N (x) yref), u = W0 + Sbar X + Ku U, solve (warm-started after the first
 * step), U += x[0:n_u] where SOLVED.  yref: device pointer to n_y values, or NULL for 0. */
int mpcq_mimo_step_device(mpcq_ctx *ctx, const double *X_dev, double *U_dev, const double *yref_dev,
                          void *stream);
/* One polished controllerStep for every QP: mpcq_mimo_step_device, its kernel, launch and
 * arithmetic unchanged, then OSQP v0.6 polish.c on every QP that ended MPCQ_SOLVED, in one more kernel on the same
 * stream; the context keeps a device-to-device copy of U_dev from before the step.  settings.polish stays 0:
 * settings.delta and settings.polish_refine_iter are read.
 * Where polish succeeds (OSQP's criterion: both residuals reduced, or one reduced and the other already below
 * 1e-10) the published x, y (mpcq_get_solution, mpcq_get_dual, mpcq_device_view_get) become the polished point,
 * the scaled warm state becomes the polished (x^, z^, y^) as OSQP replaces work->x, z, y, and
 * U_b = U_prev_b + x_b[0:n_u], one fp64 add per component.  Where it does not, or the QP did not end
 * MPCQ_SOLVED, x, y, the warm state and U are what the plain step left, bit for bit.  status, iter and rho are
 * always the ADMM's.  A QP with more than n active rows (some bound pair j, n + j both active; a deviation from
 * OSQP: the reduced system is held for at most n rows) or whose factorisation meets a non-positive pivot is
 * reported unsuccessful, n_active being the count.
 * mpcq_get_polish_info serves the call (its buffers are allocated on the first polished step); a plain
 * mpcq_mimo_step_device or a MIMO setup makes it report "not performed" again.  The sensitivities above the
 * step's iterate (mpcq_mimo_sensitivity*, mpcq_mimo_step_*) then read the polished iterate.  No atomics: two
 * calls on equal state give identical bits.
 * MPCQ_ERR_ORDER: no successful mpcq_mimo_setup_plants_device since the last setup.  MPCQ_ERR_ARG: NULL X / U,
 * settings.polish set, or `stream` under graph capture.  A refused call writes nothing. */
int mpcq_mimo_step_polish_device(mpcq_ctx *ctx, const double *X_dev, double *U_dev, const double *yref_dev,
                                 void *stream);
/* One controllerStep for every QP with its own output reference over the horizon, the MIMO twin of
 * mpcq_mpc_step_ref_device:
 *   q_b = Fx X_b + Fu U_b + Fr ref_b,  ref_b[i*n_y + y] = ref_dev[b*ref_stride + i*n_y + y], i < N, y < n_y.
 * ref_stride == 0: one horizon reference shared by the batch; otherwise ref_stride >= N*n_y.  Everything else is
 * mpcq_mimo_step_device's.  Fr is never stored: it is block-Toeplitz, and with F[j] block row j of the operator
 * block's row sums Frs (F[N] = 0) and ref_N = 0,
 *   (Fr ref)_j = sum_{d=0}^{N-1-j} F[N-1-d] (ref_{j+d} - ref_{j+d+1}),
 * accumulated in ascending d, then ascending y, in fp64 FMA.  A horizon-constant reference 1_N (x) yref leaves exact
 * zeros and the last term F[j] yref, so it reproduces mpcq_mimo_step_device(yref) bit for bit.
 * polish = 1 runs the polish pass of mpcq_mimo_step_polish_device afterwards (the same kernel, U_prev copy and
 * mpcq_get_polish_info); polish = 0 is the plain step.
 * ref_dev is read-only and must stay valid and unchanged until the step has finished on `stream`.  q is written
 * eagerly: mpcq_device_view_get().q shows this step's q.
 * Afterwards mpcq_mimo_sensitivity*, mpcq_mimo_step_vjp* and mpcq_mimo_step_gains* serve the step unchanged; their
 * dyref is then the gradient with respect to a uniform shift of the reference (ref_b + 1_N (x) dy), and
 * mpcq_mimo_step_ref_vjp_device gives the gradient with respect to ref_b itself.  mpcq_mimo_plant_vjp* would form gFr
 * from a yref the step did not use: it returns MPCQ_ERR_ORDER until the next mpcq_mimo_step_device or
 * mpcq_mimo_step_polish_device.
 * MPCQ_ERR_ARG, nothing written: NULL X, U or ref; a non-zero ref_stride below N*n_y; polish not 0 or 1;
 * settings.polish set; `stream` under graph capture when polish = 1.  MPCQ_ERR_ORDER as mpcq_mimo_step_device. */
int mpcq_mimo_step_ref_device(mpcq_ctx *ctx, const double *X_dev, double *U_dev, const double *ref_dev,
                              long long ref_stride, int polish, void *stream);
/* Host-memory form (copies in/out, synchronises): X batch*n_x, U batch*n_u (updated), ref as above on the host. */
int mpcq_mimo_step_ref(mpcq_ctx *ctx, const double *X, double *U, const double *ref, long long ref_stride, int polish);

/* ---- closed-loop MIMO runs: simulated plant, reference schedule, record ------------
 * The MIMO twins of mpcq_mpc_set_plant / mpcq_mpc_simulate_device / mpcq_mpc_run_device / mpcq_mpc_run_ref_device /
 * mpcq_mpc_set_stream_log.  The control step stays the kernels of mpcq_mimo_step*_device, launched once per step;
 * between two steps one kernel advances every plant, writes the record row and adds to the totals.  No hipGraph.
 *
 * The simulated plant of every QP: Ad_dev batch*n_x*n_x, Bd_dev batch*n_x*n_u (device, fp64, QP-major, row-major
 * blocks), copied device-to-device on `stream` into buffers the context owns; n_x, n_u are the context's own from
 * mpcq_mimo_setup_plants_device.  It need not be the model the controller was set up with.  A later MIMO setup keeps
 * the plant when n_x and n_u are unchanged and drops it otherwise.  A run on another stream is ordered after the
 * copy by the caller.  MPCQ_ERR_ORDER: no MIMO setup.  MPCQ_ERR_ARG: NULL Ad / Bd, `stream` under graph capture. */
int mpcq_mimo_set_plant_device(mpcq_ctx *ctx, const double *Ad_dev, const double *Bd_dev, void *stream);
/* One plant update in place on device-resident X (batch*n_x) from U (batch*n_u):  X_b <- Ad_b X_b + Bd_b U_b + w.
 * Row i is sum_t Ad[i,t] x_t in ascending t, then sum_j Bd[i,j] u_j in ascending j, then + w_i, in fp64, every
 * product rounded before it is added (no FMA).  w of QP b is the counter-based noise of mpcq_mpc_simulate_device
 * keyed by (seed, first_qp + b, step): Box-Muller pairs from draws step*64 + 2p, 2p + 1, ceil(n_x/2) <= 6 pairs,
 * component i < ceil(n_x/2) the cosine of pair i, the others the sine of pair i - ceil(n_x/2)
 * (workload.plant_noise); noise_std == 0 draws nothing.  Asynchronous on `stream`.
 * MPCQ_ERR_ORDER: no MIMO setup, or no plant.  MPCQ_ERR_ARG: NULL X / U, step < 0. */
int mpcq_mimo_simulate_device(mpcq_ctx *ctx, double *X_dev, const double *U_dev, unsigned long long seed,
                              long long first_qp, long long step, double noise_std, void *stream);

/* Record of a run.  Caller-owned device pointers, any of which may be NULL (not recorded).  The four per-step arrays
 * are step-major as mpcq_stream_log's; row r = s - step0 of control step s holds
 *   U      [(r*batch + b)*n_u + j]  U_b after the step's control step (the row before, or the call's input for row
 *                                   0 of the first call, where the step did not end MPCQ_SOLVED)
 *   X      [(r*batch + b)*n_x + i]  X_b after the step's plant update
 *   status [r*batch + b], iter [r*batch + b]   those of the step's solve
 * and the two totals are batch ints each: the ADMM iterations of the call's steps and the number of them that did
 * not end MPCQ_SOLVED.  A run with steps > 0 zeroes the totals when it starts and accumulates them on the device
 * (each QP is owned by one 16-lane group: no atomics).  rows and step0 are read when one of the four is set. */
typedef struct mpcq_mimo_log {
    double *U, *X;
    int *status, *iter;
    int *iters_total, *unsolved_total;
    long long rows;   /* capacity in control steps */
    long long step0;  /* absolute control step stored in row 0 */
} mpcq_mimo_log;

/* `steps` rounds of [control step; plant update] for the absolute control steps first_step .. first_step+steps-1;
 * X_dev / U_dev evolve in place.  The control step is mpcq_mimo_step_device(yref_dev), or with polish = 1
 * mpcq_mimo_step_polish_device(yref_dev); the plant update of step s is mpcq_mimo_simulate_device(step = s).
 * A run is, bit for bit, that sequence of single calls: X, U, the context's x, y, status, iter, rho, q, warm state
 * and polish info are the last step's, every log row is what the single calls would have shown after the step, and
 * the context is left as the sequence leaves it, so mpcq_mimo_sensitivity*, mpcq_mimo_step_vjp* and
 * mpcq_mimo_step_*gains* serve the run's last control step unchanged.  `log` may be NULL.  steps == 0 enqueues and
 * writes nothing and returns MPCQ_OK.  Asynchronous on `stream`; yref_dev and the log's buffers must stay valid
 * until it has finished.
 * Refused before anything is enqueued or written.  MPCQ_ERR_ORDER: no MIMO setup, or no plant.  MPCQ_ERR_ARG: NULL
 * X / U; steps < 0; first_step < 0; polish not 0 or 1; settings.polish set; one of the log's four per-step pointers
 * set with rows < 1, step0 < 0 or a row of the call outside [0, rows); `stream` under graph capture. */
int mpcq_mimo_run_device(mpcq_ctx *ctx, double *X_dev, double *U_dev, const double *yref_dev, int steps,
                         unsigned long long seed, long long first_qp, long long first_step, double noise_std,
                         int polish, const mpcq_mimo_log *log, void *stream);
/* The same run with a reference schedule of sched_len blocks of n_y values per QP, sched_stride doubles apart
 * (0: one schedule for the batch; otherwise >= sched_len*n_y).  Control step s is
 * mpcq_mimo_step_ref_device(ref, ref_stride, polish) on the window
 *   ref_b[i*n_y + y] = sched_dev[b*sched_stride + min(s + i, sched_len - 1)*n_y + y],  i < N
 * (the last block is held, as in mpcq_mpc_run_ref_device).  While s + N <= sched_len the step reads the schedule in
 * place (ref = sched_dev + s*n_y); a call that goes further first copies, once, 2N-1 blocks per schedule row from
 * block max(sched_len - N, 0) with the last block repeated into staging the context owns (8 (2N-1) n_y bytes per QP,
 * 5.7 KB at n_y 12, N 30; one row for a shared schedule; allocated by the first such call) and its later steps read
 * their windows there.  sched_dev must stay valid and unchanged until `stream` has finished.
 * Also MPCQ_ERR_ARG: NULL schedule, sched_len < 1, a non-zero sched_stride below sched_len*n_y. */
int mpcq_mimo_run_ref_device(mpcq_ctx *ctx, double *X_dev, double *U_dev, const double *sched_dev, int sched_len,
                             long long sched_stride, int steps, unsigned long long seed, long long first_qp,
                             long long first_step, double noise_std, int polish, const mpcq_mimo_log *log,
                             void *stream);

/* ---- active-set sensitivities of the last MIMO step --------------------------------
 * The definition of mpcq_sensitivity_device above, applied to the last mpcq_mimo_step_device of the context:
 * the active rows by the polish rule on the step's final scaled iterate with u^ = E u of the step's bounds
 * (l = -DBL_MAX: no row is lower-active, so there is no gl), and for each right-hand side r < n_rhs
 * (1 <= n_rhs <= 4)  K [v; w] = [g_r; 0],  K = [P, A_a'; A_a, 0]:
 *   gq_r = -v                                   (batch*n_rhs*n, QP-major, then r)
 *   gu_r[i] = w_k where row i is the k-th active row, else 0   (batch*n_rhs*m)
 * g_dev: batch*n_rhs*n cotangents (device, fp64), or NULL for g_r = e_r, the r-th component of the applied move
 * x*[0:n_u] (then n_rhs <= n_u).  Solved in the scaled space with settings.delta and
 * settings.polish_refine_iter, one factorisation per QP for all right-hand sides; the contract is the solution
 * of the unregularised system.  n_active (batch): the active rows.  A QP that did not end MPCQ_SOLVED, whose
 * reduced system could not be factored, or with more than n active rows (some bound pair j, n + j both active)
 * gets all-zero outputs and n_active = -1.  Each output may be NULL, not all.
 * Read-only on the context: a step after the call is bit-identical to the same step without it.  The kernel
 * runs on `stream`, ordered after the context's last stream (an event), and the context's next step is ordered
 * after it.  No atomics: two calls give identical bits.
 * MPCQ_ERR_ORDER: no successful mpcq_mimo_setup_plants_device; no mpcq_mimo_step_device since the last setup.
 * MPCQ_ERR_ARG: n_rhs out of range; NULL g with n_rhs > n_u; every output NULL; `stream` under graph capture
 * (nothing is recorded into the capture).  A refused call writes nothing. */
int mpcq_mimo_sensitivity_device(mpcq_ctx *ctx, const double *g_dev, int n_rhs, double *gq_dev, double *gu_dev,
                                 int *n_active_dev, void *stream);
/* Host-memory form (copies in/out, synchronises); the same arrays on the host. */
int mpcq_mimo_sensitivity(mpcq_ctx *ctx, const double *g, int n_rhs, double *gq, double *gu, int *n_active);
/* The same solve followed by the chain rule through the MIMO front end, q = Fx X + Fu U + Fr (1_N (x) yref) and
 * u = W0 + Sbar X + Ku U: with gu_r = [gt; gb] split into horizon blocks of n_u, per right-hand side
 *   dX = Fx' gq + K' sum_{k < min(s_rows, N)} (gt_k - gb_k)   (batch*n_rhs*n_x)
 *   dU = Fu' gq + K0' sum_k (gb_k - gt_k)                     (batch*n_rhs*n_u)
 *   dyref = Frs' gq                                           (batch*n_rhs*n_y)
 * from the plant's own operator block, fp64 sums in ascending row index.  dyref is per QP: mpcq_mimo_step_device's
 * yref is one vector for the whole batch, so a caller who wants its gradient sums dyref over the QPs (after a
 * mpcq_mimo_step_ref_device, dyref is the gradient with respect to a uniform shift of the QP's reference; the
 * gradient with respect to the reference itself: mpcq_mimo_step_ref_vjp_device).  Each output may be NULL, not
 * all.  Otherwise as mpcq_mimo_sensitivity_device. */
int mpcq_mimo_step_vjp_device(mpcq_ctx *ctx, const double *g_dev, int n_rhs, double *dX_dev, double *dU_dev,
                              double *dyref_dev, int *n_active_dev, void *stream);
/* Step gains: mpcq_mimo_step_vjp_device with g = NULL and n_rhs = n_u, the gradients of the applied move
 * x*[0:n_u] with respect to the step's X, previous U and yref at the current active set: the explicit-MPC
 * feedback gain.  (U_new = U + x*[0:n_u] adds the identity to dU.) */
int mpcq_mimo_step_gains_device(mpcq_ctx *ctx, double *dX_dev, double *dU_dev, double *dyref_dev, int *n_active_dev,
                                void *stream);
/* mpcq_mimo_step_vjp_device with the gradient of the horizon reference in place of dyref:
 *   dref = Fr' gq                                             (batch*n_rhs*N*n_y; block i, then y)
 * from the row sums alone: with w_i = sum_{j<=i} F[N-1-i+j]' gq_j and w_{-1} = 0, dref_i = w_i - w_{i-1}, one thread
 * per output, both sums in ascending j in fp64; sum_i dref_i = Frs' gq, which is dyref.  dX, dU and n_active are
 * mpcq_mimo_step_vjp_device's bit for bit.  Refusals and ordering are those of mpcq_mimo_step_vjp_device; the
 * last step may be a mpcq_mimo_step_device too (dref is then the gradient at ref = 1_N (x) yref).  No atomics: two
 * calls give identical bits; a QP with n_active = -1 gets zeros. */
int mpcq_mimo_step_ref_vjp_device(mpcq_ctx *ctx, const double *g_dev, int n_rhs, double *dX_dev, double *dU_dev,
                                  double *dref_dev, int *n_active_dev, void *stream);
/* Step gains with respect to the horizon reference: mpcq_mimo_step_ref_vjp_device with g = NULL and n_rhs = n_u. */
int mpcq_mimo_step_ref_gains_device(mpcq_ctx *ctx, double *dX_dev, double *dU_dev, double *dref_dev, int *n_active_dev,
                                    void *stream);
/* Host-memory form (copies out, synchronises): dX batch*n_u*n_x, dU batch*n_u*n_u, dref batch*n_u*N*n_y, n_active. */
int mpcq_mimo_step_ref_gains(mpcq_ctx *ctx, double *dX, double *dU, double *dref, int *n_active);

/* ---- the last MIMO step differentiated in the plant model, the weights and the constraint data
 * The nine plant arrays are those mpcq_mimo_setup_plants_device read (device, fp64, plant-major; the caller vouches
 * that they are unchanged); n_x, n_u, n_y, N and s_rows are the context's own from that setup.  X_dev (batch*n_x) is
 * the X of the context's last MIMO step, U_prev_dev (batch*n_u) the U from before that step (which the step
 * overwrites), yref_dev (n_y, or NULL for 0) that step's yref.  g_dev: batch*n cotangents of x*, or NULL for e_0.
 * Per QP, with (gq, w = gu, n_active) what mpcq_mimo_sensitivity_device(g, n_rhs = 1) returns for this step, x and y
 * the published solution and dual, and y_a = y on the rows of the active set that call uses (polish's rule on the
 * step's final scaled iterate), 0 elsewhere, the operator cotangents are
 *   gP = 1/2 (gq x' + x gq')     gA = y_a gq' - w x'
 *   gFx = gq X'    gFu = gq U_prev'    gFr = gq (1_N (x) yref)'    gSbar = w X'    gKu = w U_prev'    gW0 = w
 * and the outputs are these pulled back through the MIMO condensing as oracle/mpc_mimo.c states it
 * (P = (H1 + H1')/2, ...): gAd batch*n_x*n_x, gBd batch*n_x*n_u, gCd batch*n_y*n_x, gQ batch*n_y*n_y, gR, gRD
 * batch*n_u*n_u, gK batch*n_u*n_x, gK0 batch*n_u*n_u, gw0 batch*n_u.  Q, R and RD are treated as general matrices:
 * a caller with a symmetric parametrisation symmetrises.  No n x n object is formed: every term is a sum over the
 * horizon of small outer products (the factored form of DESIGN.md 4.17).  A QP with n_active = -1 gets all-zero
 * outputs.  Each output may be NULL, not all; an output's bits do not depend on which others are NULL.
 * Two kernels on `stream`: the sensitivity solve into staging the context owns (allocated on the first call), then
 * the pull-back.  Read-only on the context, ordered after the context's last stream (an event) with the context's
 * next step ordered after it, as mpcq_mimo_sensitivity_device; after mpcq_mimo_step_polish_device the polished
 * iterate is read.  No atomics, sums in a fixed order: two calls give identical bits.
 * MPCQ_ERR_ORDER: no setup; no mpcq_mimo_step_device since the last MIMO setup; the last step was a
 * mpcq_mimo_step_ref* (its horizon reference is not among the arguments).  MPCQ_ERR_ARG: a context whose last
 * setup is not a MIMO one; a NULL plant array, X or U_prev; every output NULL; `stream` under graph capture.  A
 * refused call writes nothing. */
int mpcq_mimo_plant_vjp_device(mpcq_ctx *ctx, const double *g_dev, const double *Ad, const double *Bd, const double *Cd,
                               const double *Q, const double *R, const double *RD, const double *K, const double *K0,
                               const double *w0, const double *X_dev, const double *U_prev_dev, const double *yref_dev,
                               double *gAd, double *gBd, double *gCd, double *gQ, double *gR, double *gRD, double *gK,
                               double *gK0, double *gw0, int *n_active_dev, void *stream);
/* Host-memory form (copies in/out, synchronises); the same arrays on the host. */
int mpcq_mimo_plant_vjp(mpcq_ctx *ctx, const double *g, const double *Ad, const double *Bd, const double *Cd,
                        const double *Q, const double *R, const double *RD, const double *K, const double *K0,
                        const double *w0, const double *X, const double *U_prev, const double *yref, double *gAd,
                        double *gBd, double *gCd, double *gQ, double *gR, double *gRD, double *gK, double *gK0, double *gw0,
                        int *n_active);

/* Last HIP error string of this thread (static storage). */
const char *mpcq_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MPCQ_H */

// solvempc_amd/csrc/mpcq_internal.h — device data layout shared by the setup and ADMM kernels.
//
// Factorisations used on the device (replace OSQP's QDLDL LDL' of the KKT matrix): for a plant
// with scaled data (P^, A^) and constraint-type pattern s (rho_j = rho*s_j, or RHO_MIN for free
// rows), the reduced KKT matrix is a one-parameter family
//        M(rho) = P~ + rho G,   P~ = P^ + sigma I + RHO_MIN sum_free a_j a_j',  G = sum s_j a_j a_j'.
// * Eigen-basis (shared plants; per-plant shapes beyond one wave): setup computes W' P~ W = I,
//   W' G W = diag(lambda), so that M(rho)^-1 = W diag(1/(1 + rho lambda)) W' for EVERY rho: an
//   adaptive-rho update (OSQP adapt_rho) only rescales a diagonal, and all QPs of a plant share W
//   whatever rho each one has reached.  The iterate keeps x in that basis (x^ = W x').
// * Direct inverse (per-plant batches, n <= 32, m <= 64; setup_inv_kernel): M(rho0)^-1 itself, the
//   iterate in the scaled basis (x' = x^).  The same operator slots then hold W = W^-1 = I,
//   lambda = 0, sigma W'W = sigma M^-1, G = M^-1, Bt = A^ M^-1 (so one iteration is the same code
//   for both), and rho0 = the rho they were built for; a QP whose rho moves away from rho0 rebuilds
//   M^-1 in its kernel (OSQP's refactorisation, mpcq_wave.h).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace mpcq {

// OSQP v0.6 constants (constants.h)
constexpr double kInfty = 1e30;
constexpr double kMinScaling = 1e-4;
constexpr double kMaxScaling = 1e4;
constexpr double kRhoMin = 1e-6;
constexpr double kRhoMax = 1e6;
constexpr double kRhoTol = 1e-4;
constexpr double kRhoEqOverIneq = 1e3;
constexpr double kDivisionTol = 1.0 / kInfty;

// Per-plant operators, padded to the kernel capacity (NC variables, MC rows).  Row-major.
// Every array is [n_plants][...]; padding entries are zero (padded rows: free, E = 1).
template <typename T>
struct PlantOps {
    const T *lam;    // NC          generalised eigenvalues
    const T *W;      // NC x NC     x^ = W x'
    const T *sWtW;   // NC x NC     sigma * W'W   (the sigma x term of the KKT rhs, in W-basis)
    const T *WtA;    // MC x NC     B = A^ W   (row j: b_j)
    const T *PW;     // NC x NC     P^ W       (P x^ for the dual residual)
    const T *Winv;   // NC x NC     W^-1 = V' L'  (osqp_warm_start: x' = W^-1 x^)
    const T *Ah;     // MC x NC     A^         (A' y for the dual residual)
    const T *D;      // NC          Ruiz D     (Dinv = 1/D)
    const T *E;      // MC          Ruiz E
    const T *Dinv;   // NC
    const T *Einv;   // MC
    const T *cs;     // 2           c, 1/c
    const T *rscale; // MC          rho_j = rho * rscale_j  (0 => free row => RHO_MIN)
    const int *ctype;// MC          OSQP constr_type: -1 free, 0 inequality, 1 equality
};
// (G: NC x NC, g = -G' q^; Bt: MC x NC, the x-side product's operator rows; rho0: 1.  Eigen-basis:
// G = W, Bt = A^ W, rho0 = -1.  Direct inverse: G = M^-1, Bt = A^ M^-1, rho0 = the built-for rho.)

// Shapes of one plant's operator block, in elements, for capacities (nc, mc).
struct OpsLayout {
    int nc, mc;
    size_t lam, W, sWtW, WtA, PW, Winv, Ah, D, E, Dinv, Einv, cs, rscale, G, Bt, rho0, total;
    __host__ __device__ static constexpr OpsLayout make(int nc, int mc)
    {
        OpsLayout L{};
        L.nc = nc;
        L.mc = mc;
        size_t o = 0;
        L.lam = o; o += nc;
        L.W = o; o += (size_t)nc * nc;
        L.sWtW = o; o += (size_t)nc * nc;
        L.WtA = o; o += (size_t)mc * nc;
        L.PW = o; o += (size_t)nc * nc;
        L.Winv = o; o += (size_t)nc * nc;
        L.Ah = o; o += (size_t)mc * nc;
        L.D = o; o += nc;
        L.E = o; o += mc;
        L.Dinv = o; o += nc;
        L.Einv = o; o += mc;
        L.cs = o; o += 2;
        L.rscale = o; o += mc;
        L.G = o; o += (size_t)nc * nc;
        L.Bt = o; o += (size_t)mc * nc;
        L.rho0 = o; o += 2;
        L.total = o;
        return L;
    }
};

struct SolverSettings {
    double rho, sigma, alpha;
    double eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
    double adaptive_rho_tolerance;
    int max_iter, check_termination, adaptive_rho, adaptive_rho_interval;
    int warm_start, scaled_termination, scaling;
};

// Status values (mirror include/mpcq.h)
enum : int {
    kSolved = 1,
    kSolvedInaccurate = 2,
    kPrimalInfeasibleInaccurate = 3,
    kDualInfeasibleInaccurate = 4,
    kMaxIterReached = -2,
    kPrimalInfeasible = -3,
    kDualInfeasible = -4,
    kNonCvx = -7,
    kUnsolved = -10,
    kInvalidBounds = -20,
    kTypeChanged = -21,
};

// Arguments of the setup kernel (one 64-lane workgroup per plant).
struct SetupArgs {
    int n, m, nc, mc, n_plants;
    int scaling;       // Ruiz passes
    double sigma, rho;
    double jacobi_tol;  // Jacobi stops at off(C)^2 <= jacobi_tol * diag(C)^2 (fp64 solves 1e-32, fp32 1e-20)
    const double *P, *q0, *A, *l0, *u0;  // [plant] n*n, n, m*n, m, m
    double *ops;       // [plant] OpsLayout(nc, mc).total
    int *ctype;        // [plant] mc
    double *scratch;   // [plant] scratch_len(n, m)
    int *status;       // [plant] 0 ok, else error
    long long *prof;   // debug (MPCQ_SETUP_PROF): [plant][16] stage clock stamps, or null
    int *flags;        // OR over plants: 1 setup failed (non-convex), 2 a row is not an inequality,
                       // 4 the Jacobi eigen-solve hit its sweep cap (inaccurate basis); 8, 16: the checks of
                       // mpcq_update_P_A_device (mpcq_internal_lower_free_check, mpcq_internal_paired_check)
};

// Phase lists of the tile path: the QPs a phase hands on are appended to one of kShards segments
// (the appending workgroup's blockIdx % kShards), each with its own counter on its own 128-B line, so
// the ~3,000 waves reaching a phase boundary together do not serialise on one device-scope counter
// (~11 ns per atomic).  Segment s holds entries [s cap, s cap + count[s * kStride]).  The next phase's
// workgroup b serves segment b % kShards (its 64 G slots at (b / kShards) 64 G): the workgroups of a
// segment are exactly those that can have filled it, so every entry is covered.
struct ListSeg {
    static constexpr int kShards = 32;
    static constexpr int kStride = 32;  // ints per counter line
    static constexpr int kCounters = kShards * kStride;
    __host__ __device__ static constexpr int cap(int batch) { return (batch + kShards - 1) / kShards + 256; }
};

// Hardest-first order of a shared-plant MPC step (mpcq_order.hip): the key v = max_j (A x_u - u)_j of a
// QP (its unconstrained optimum's largest bound violation) falls in bin floor(16 log2|v|) + 256 (16 bins
// per octave, 2^-16 .. 2^16, clamped), |v| = 0 in bin 0, a non-finite |v| in the last; phase 0 runs bin
// 0's QPs first.  The host's map (m rows of kStride doubles): v_j = r[0..nx) . X + r[8] U + r[9] +
// r[10] xref.  A QP's rank inside its bin takes the low kRankBits of its key word.
struct OrderBins {
    static constexpr int kBins = 512;
    static constexpr int kPerOctave = 16;
    static constexpr int kRankBits = 22;  // batches below 4,194,304 QPs
    static constexpr int kStride = 12;
    static constexpr int kMaxRows = 64;
    __host__ __device__ static int bin(double v)
    {
        const double a = v < 0.0 ? -v : v;
        if (!(a < __builtin_inf())) return kBins - 1;  // inf, NaN
        if (a == 0.0) return 0;
        int e = 0;
        const double f = __builtin_frexp(a, &e);  // a = f 2^e, f in [0.5, 1): log2 a = e - 1 + log2(2 f)
        // the fraction's 16 sub-octave steps from its top mantissa bits (a monotone map of a within the
        // octave: ordering only needs monotone bins, not exact logarithms)
        const int sub = (int)((f - 0.5) * 32.0);  // 0 .. 15
        const int i = (e - 1) * kPerOctave + sub + kBins / 2;
        return i < 0 ? 0 : (i > kBins - 2 ? kBins - 2 : i);
    }
};

// Arguments of the ADMM kernel (one QP per lane).
// Persistent receding-horizon stream (config 5): control steps first_step .. first_step + steps - 1 of
// the simulated plant X <- Ad X + Bd U + w (mpcq_plant_sim.h) between the solves.
struct StreamArgs {
    int steps, nx, shared;        // shared: every QP's plant is plant 0
    int cpw;                      // tile stream: plants (columns) per wave
    const double *Ad, *Bd;        // [plant] nx*nx, nx
    unsigned long long seed;
    long long first_qp, first_step;
    double noise_std;
    int occ;                      // tile stream: waves per SIMD the kernel is compiled for (1: at most one
                                  // wave per SIMD, the whole register file, no spills; 2 otherwise)
};

// Per-QP horizon reference of the MPC front end (mpcq_mpc_step_ref*, mpcq_mpc_run_ref_device; read by the
// REF kernel variants only): the control step with absolute index s uses, for QP b,
//     ref_b[j] = p[b stride + min(s + j, len - 1)],   j = 0 .. n - 1
// (stride 0: one row shared by the batch).  One controllerStep: len = n, s = 0 (the row is the window).
// A stream: s = step + k for the launch's k-th control step, the step taken from *step_p where non-null
// (the captured per-step graph: the context's device step counter).  p == null: the scalar xref.
// It is a kernel argument of its own, next to AdmmArgs, so that the scalar kernels' arguments (and code)
// are what they were.
struct RefArgs {
    const double *p;
    long long stride, step;
    const long long *step_p;
    int len;
    // the window's first schedule entry at the launch's k-th control step, and element j of QP row `row`
    __device__ __forceinline__ long long first(int k) const { return (step_p ? *step_p : step) + k; }
    __device__ __forceinline__ const double *row(long long b) const { return p + b * stride; }
    __device__ __forceinline__ double at(const double *row, long long s0, int j) const
    {
        const long long i = s0 + j;
        return row[i < len ? i : len - 1];
    }
};

// Per-step record of a receding-horizon stream (mpcq_mpc_set_stream_log; written by the LOG kernel variants
// and the per-step graph's record kernel only).  Step-major: the launch's k-th control step fills row
//     r = row0 + k (+ *step_p where non-null),   U, status, iter at [r batch + b], X at [(r batch + b) nx + i]
// with row0 = first_step - step0 for a one-launch stream (k = 0 .. steps - 1) and row0 = -step0, k = 0 for the
// per-step graph, whose step is the context's device step counter (step_p).  The host has checked every row of
// the run against the buffers' capacity before anything is enqueued.  A null array is not recorded.
// Like RefArgs it is a kernel argument of its own: the scalar and REF kernels' arguments (and code) are what
// they were.
struct LogArgs {
    double *U, *X;
    int *status, *iter;
    long long row0;
    const long long *step_p;
    int batch;
    __device__ __forceinline__ size_t at(int k, int b) const
    {
        return (size_t)((step_p ? *step_p : 0) + row0 + k) * (size_t)batch + (size_t)b;
    }
};

template <typename T>
struct AdmmArgs {
    int batch, n, m;
    int shared;                 // 1: every QP uses plant 0
    size_t ops_stride;          // elements per plant block (OpsLayout::total)
    PlantOps<T> ops;
    const int *ctype;           // [plant][mc]
    SolverSettings st;
    int adaptive_interval;      // resolved (0 -> 4*check_termination)
    int all_ineq;               // every row of every plant is an inequality (constr_type 0)
    int paired;                 // shared plant with m = 2n, n % 4 == 0, A rows n + j == -rows j (tile kernel)
    int lower_free;             // every l^ of every QP is below -OSQP_INFTY*MIN_SCALING
    // per-QP inputs (fp64, QP-major as in the C ABI)
    const double *q, *u, *l;    // batch*n, batch*m, batch*m (l may be a single shared m-vector)
    int l_shared;
    // state (QP-major [batch][row], T) for warm start
    T *xs, *zs, *ys, *rhos;
    int warm;                   // read xs/zs/ys at entry (settings.warm_start)
    int fresh;                  // ignore stored state: x = z = y = 0, rho = settings.rho (mpcq_reset)
    // snapshots for the infeasibility certificates (QP-major)
    T *snap_x, *snap_y;
    // outputs
    double *x, *y, *rho_out;
    int *status, *iter;
    // receding-horizon stream counters (mpcq_mpc_run_device; null otherwise): per QP, the iterations of
    // every solve and the solves that did not end SOLVED, accumulated at finalize
    int *it_acc, *uns_acc;
    // MPC front end (n = N, m = 2N); null when unused
    int mpc, nx;
    const double *X, *Fx, *Fu, *Fr, *Sbar, *Ku, *W0;
    double *U, *q_out, *u_out;
    double *X_save, *U_save;    // tile path: phase 0 saves X [batch][nx], U [batch] (q, u computed on demand)
    double xref;
    int mpc_u;                  // U += x[0] at termination (the front end may have run in an earlier phase)
    // tile kernel (shared plant): MFMA operand images and the phase machinery (mpcq_tile.h)
    const T *img;               // TileLayout images of the plant
    const int *list_in;         // active QP indices of this phase (null: identity 0..batch-1), ListSeg layout
    const int *count_in;        // ListSeg counters of list_in (null: batch)
    int *list_out, *count_out;  // QPs still running at stop_iter (appended, ListSeg layout)
    // ListSeg counter blocks this launch zeroes on entry (workgroup 0; null: none): the next phase's
    // output counters, and in a chain's last launch the first phase's (for the next solve)
    int *zero_cnt, *zero_cnt0;
    int list_seg;               // ListSeg segment capacity
    int *it_state;              // [batch] iterations done so far in this solve
    int qp0;                    // QP index of identity-list slot 0 (sub-batch parts of a tile solve)
    // phase 0 of a tile solve in hardest-first order (mpcq_order.hip; null: index order): slot i runs QP
    // ord_list[i]; workgroup 0 zeroes the OrderBins::kBins counters ord_zero for the next solve
    const int *ord_list;
    int *ord_zero;
    int stop_iter;              // phase boundary (multiple of check_termination, or max_iter)
    int resume;                 // 1: phase >= 2 (state, rho and iteration count come from the buffers)
    long long *stamps;          // debug build (MPCQ_DEBUG_HOOKS): [wave][8] s_memtime stamps, or null
    StreamArgs sim;             // the tile kernel's stream mode (tile_stream_launch): plants and noise
    // OSQP is_dual_infeasible needs ||P^ dx|| < c eps ||dx|| (norms as the termination mode reads them);
    // with lambda_min(P^) >= mu > 0 the left side is >= kappa ||dx|| (kappa from mu, D and n: host,
    // setup_on_device), so for kappa > 2 c eps the certificate cannot hold and its products are skipped
    // (0: always evaluated)
    double dinf_kappa;
    // mixed precision (MPCQ_F64_MIXED contexts, the tile kernel's paired loop): the last mix_r iterations
    // before every info iteration run in fp64, the earlier plain ones in fp32 (0: all fp64)
    int mix_r;
    // waves per SIMD of the f32 paired tile kernel (0: the default, 3; 2: the OCC-2 variant)
    int tile_occ;
    // (T) eps_abs, eps_rel, eps_prim_inf, eps_dual_inf times T(10), formed on the host in T: the tile
    // kernel's approximate check_termination (OSQP auxil.c, the 10x tolerances after max_iter)
    T eps10[4];
    // a hardest-first solve in one launch: the finalize stores (status, iter) of list slot i at
    // info_slot[2 i], [2 i + 1], one 8-B store per QP into the wave's own 128-B line, instead of two
    // scattered 4-B stores at the QP's index (mpcq_host_context.cpp materialize_info permutes them when read); null:
    // at the QP's index in status, iter
    int *info_slot;
};

// MFMA operand images of one shared plant for the tile kernel (mpcq_tile.h).  A vector of length
// 4*KS is held in "D-layout": lane l = 16 g + c (column c = QP, group g) keeps element 4 s + g of
// its QP in register s.  Image (tile t, k-step s, lane l) = M[16 t + arow(l & 15)][4 s + (l >> 4)],
// stored [t][s / VEC][lane][s % VEC] so one lane reads VEC consecutive k-steps with one 16-B load.
// paired (the tile kernel's paired loop, m = 2n, rows n + j of A = -rows j): only the top halves are
// kept, B~ = B's first n rows and B~' = its transpose, A~' = the first n columns of A^' (KBT = KNP
// k-steps, NT tiles), plus for f64 (VEC 2) BS = [B~; S] stacked (B~ rows 0 .. 4 KN - 1, then S): the
// plain iteration's z~ = B~ eta' and S eta' in one product (ceil(8 KN / 16) tiles instead of 2 NT).
// The buffer holds the generic set (make(.., false)) followed by the paired one (make(.., true)).
struct TileLayout {
    int KN, KM, NT, MT, VEC, KNP, KMP, KBT, NBS;
    bool paired;
    size_t S, Bt, B, PW, AhT, W, Wt, BS, total;
    __host__ __device__ static constexpr TileLayout make(int KN, int KM, int VEC, bool paired = false)
    {
        TileLayout L{};
        L.KN = KN; L.KM = KM; L.VEC = VEC; L.paired = paired;
        L.NT = (KN + 3) / 4; L.MT = (KM + 3) / 4;
        L.KNP = (KN + VEC - 1) / VEC * VEC; L.KMP = (KM + VEC - 1) / VEC * VEC;
        L.KBT = paired ? L.KNP : L.KMP;
        L.NBS = (paired && VEC == 2) ? (8 * KN + 15) / 16 : 0;
        const int BT = paired ? L.NT : L.MT;  // tiles of B
        size_t o = 0;
        L.S = o;   o += (size_t)L.NT * L.KNP * 64;   // sigma W'W       (n x n)
        L.Bt = o;  o += (size_t)L.NT * L.KBT * 64;   // B' = (A^ W)'    (n x m; paired n x n)
        L.B = o;   o += (size_t)BT * L.KNP * 64;     // B = A^ W        (m x n; paired n x n)
        L.PW = o;  o += (size_t)L.NT * L.KNP * 64;   // P^ W            (n x n)
        L.AhT = o; o += (size_t)L.NT * L.KBT * 64;   // A^'             (n x m; paired n x n)
        L.W = o;   o += (size_t)L.NT * L.KNP * 64;   // W               (n x n)
        L.Wt = o;  o += (size_t)L.NT * L.KNP * 64;   // W'              (n x n)
        L.BS = o;  o += (size_t)L.NBS * L.KNP * 64;  // [B~; S]         (8 KN x n; paired f64 only)
        L.total = o;
        return L;
    }
    // elements of the device buffer: both sets
    __host__ __device__ static constexpr size_t buffer(int KN, int KM, int VEC)
    {
        return make(KN, KM, VEC, false).total + make(KN, KM, VEC, true).total;
    }
    __host__ __device__ static constexpr size_t at(int KSP, int VEC, int t, int s, int lane)
    {
        return ((size_t)(t * (KSP / VEC) + s / VEC) * 64 + lane) * VEC + (s % VEC);
    }
};
// A-operand row i of an output tile holds logical row arow(i): the f32 16x16x4 accumulator keeps
// rows 4g + r of a tile in lane group g, register r; the f64 one keeps rows g + 4r.
__host__ __device__ constexpr int tile_arow(int is_f32, int i) { return is_f32 ? 4 * (i & 3) + (i >> 2) : i; }

}  // namespace mpcq

namespace mpcq {
struct CondenseArgs {
    int n_plants, nx, N, s_rows;
    const double *Ad, *Bd, *Cd, *K, *Q, *R, *RD;  // [plant] nx*nx, nx, nx, nx, 1, 1, 1
    double *P, *A, *Fx, *Fu, *Fr, *Sbar, *Ku, *W0;  // [plant] N*N, 2N*N, N*nx, N, N*N, 2N*nx, 2N, 2N
    double *scratch;                                 // [plant] condense_scratch_len (N > 32 only)
    double *q0, *l0, *u0;                            // optional: the ctor's setup data (0, -DBL_MAX, W0)
    int force_ref;                                   // test hook: the workgroup kernel at any N
};
// The reverse of the condensing (mpcq_condense_vjp.hip): N <= 32, nx <= 8, one wavefront per plant.
struct CondenseVjpArgs {
    int n_plants, nx, N, s_rows;
    const double *Ad, *Bd, *Cd, *K, *Q, *R, *RD;          // the plant data, as CondenseArgs
    const double *gP, *gA, *gFx, *gFu, *gFr, *gSbar, *gKu;  // cotangents, shapes of CondenseArgs' outputs; null: 0
    double *gAd, *gBd, *gCd, *gK, *gQ, *gR, *gRD;         // shapes of the plant data; each may be null
};
}  // namespace mpcq

namespace mpcq {
// ---- MIMO condensed MPC (BASELINE config 4; mpcq_mimo.hip) -------------------------------------
// Per-plant operator block (fp64, offsets in doubles) written by mimo_setup_kernel: the scaled Hessian
// P^ = c D P D (row-major n x n), the Ruiz scaling (D: n; E: n, the same for row j and row n + j of
// A = [L (x) K0; -(L (x) K0)]), c and 1/c, the unscaled front-end operators Fx (n x nx), Fu (n x nu),
// Frs = Fr (1_N (x) I_ny) (n x ny), the bound data K (nu x nx), K0 (nu x nu), w0 (nu), and
// SW (N blocks of nu x nu): suffix sums over k >= j of K0' diag(2 E_k^2) K0, so that the constraint
// Gram matrix A^'A^ has block (j1, j2) = D SW[max(j1, j2)] D.
struct MimoLayout {
    int N, nx, nu, ny, n, ldp;
    int Ph, D, E, cs, Fx, Fu, Frs, K, K0, w0, SW, total;  // < 2^31 for n <= 128
    __host__ __device__ static MimoLayout make(int N, int nx, int nu, int ny)
    {
        MimoLayout L{};
        L.N = N; L.nx = nx; L.nu = nu; L.ny = ny; L.n = N * nu;
        const int n = L.n;
        L.ldp = (n + 15) & ~15;  // P^ rows padded (zeros) to 16 columns: aligned, in-bounds 16-column loads
        int o = 0;
        L.Ph = o; o += n * L.ldp;
        L.D = o; o += n;
        L.E = o; o += n;
        L.cs = o; o += 2;
        L.Fx = o; o += n * nx;
        L.Fu = o; o += n * nu;
        L.Frs = o; o += n * ny;
        L.K = o; o += nu * nx;
        L.K0 = o; o += nu * nu;
        L.w0 = o; o += nu;
        L.SW = o; o += N * nu * nu;
        L.total = (o + 1) & ~1;  // 16-B aligned blocks
        return L;
    }
};

// The MIMO shape domain: what mpcq_mimo_setup_plants_device accepts and every MIMO launcher serves.
inline bool mimo_shape_ok(int N, int nx, int nu, int ny)
{
    return (nu == 1 || nu == 2 || nu == 4) && nx >= 1 && nx <= 12 && ny >= 1 && ny <= 12 && N >= 1 && N <= 32 &&
           N * nu <= 128;
}

// f(std::integral_constant<int, n_u>) for the run-time n_u of a shape mimo_shape_ok accepts
template <typename F>
inline auto mimo_with_nu(int nu, F &&f)
{
    if (nu == 1) return f(std::integral_constant<int, 1>{});
    if (nu == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 4>{});
}

// The active set's rule of a MIMO step's row, polish's on the scaled iterate (l = -DBL_MAX: upper-active rows only):
// u the row's unscaled upper bound, E its scaling, (z, y) the step's final scaled iterate.
__host__ __device__ __forceinline__ bool mimo_upper_active(double u, double E, double z, double y)
{
    return u * E - z < y;
}

struct MimoSetupArgs {
    int n_plants, N, nx, nu, ny, s_rows, scaling;
    double sigma;
    const double *Ad, *Bd, *Cd, *Q, *R, *RD, *K, *K0, *w0;  // [plant] nx*nx, nx*nu, ny*nx, ny*ny, nu*nu x2, nu*nx, nu*nu, nu
    double *ops;                                            // [plant] MimoLayout::total
    int *flags;                                             // OR: 1 a diagonal of P^ + sigma I is not positive
                                                            //     (non-convex), 2 a row is not an inequality,
                                                            //     4 some K0 is not diagonal
    long long *stamps;                                      // debug (MPCQ_MIMO_SETUP_STAMPS): 16 per plant, or null
};

struct MimoArgs {
    int batch, N, nx, nu, ny, s_rows;
    size_t ops_stride;
    const double *ops;          // [plant] MimoLayout
    SolverSettings st;
    int adaptive_interval;
    const double *X, *yref;     // batch*nx (device), ny (device)
    double *U;                  // batch*nu (device): U += x[0:nu] when solved (:105)
    double *q_out, *u_out;      // batch*n, batch*2n: this step's q, u (unscaled)
    double *xs, *zs, *ys, *rhos;// scaled state (warm start): batch*n, batch*2n, batch*2n, batch
    int warm, fresh;
    int diag_k0;                // every plant's K0 is diagonal: the A^ products need no cross-component mix
    double *x, *y;              // unscaled solution: batch*n, batch*2n
    int *status, *iter;
    double *rho_out;
    long long *stamps;          // debug (MPCQ_MIMO_STAMPS) or null
};

// Arguments of mimo_sens_kernel (mpcq_mimo_sens.hip): the active-set sensitivities of the last MIMO step and the
// front end's chain rule, one workgroup per QP, fp64.  Everything of the context is read-only.
struct MimoSensArgs {
    int batch, N, nx, nu, ny, s_rows;
    int n_rhs;                  // right-hand sides per QP (1..4), one factorisation for all of them
    size_t ops_stride;
    const double *ops;          // [plant] MimoLayout
    const double *u;            // [batch] 2n: the step's unscaled upper bounds (MimoArgs::u_out)
    const double *zs, *ys;      // [batch] 2n: the step's final scaled iterate
    const int *status;          // [batch] only MPCQ_SOLVED QPs get a sensitivity
    const double *g;            // [batch][n_rhs] n: the cotangents, or null: e_r for right-hand side r
    double *gq, *gu;            // [batch][n_rhs] n, 2n (each may be null)
    double *dX, *dU, *dyref;    // [batch][n_rhs] nx, nu, ny: the chain rule on (gq, gu) (each may be null)
    int *n_active;              // [batch] rows of the reduced system, -1 where no sensitivity exists (or null)
    double delta;
    int refine;
    double *dref;               // [batch][n_rhs] N*ny: Fr' gq, the chain rule on a horizon reference (or null)
};

// Arguments of polish_mimo_kernel (mpcq_mimo_polish.hip): OSQP's polish of the MIMO step just enqueued, one workgroup
// per QP, fp64.  Written where polish succeeds: x, y, the warm state and U; always: the three pol_* arrays.
struct MimoPolishArgs {
    int batch, N, nx, nu, ny;
    size_t ops_stride;
    const double *ops;          // [plant] MimoLayout
    const double *q, *u;        // [batch] n, 2n: the step's unscaled q, u (MimoArgs::q_out, u_out)
    double *xs, *zs, *ys;       // [batch] n, 2n, 2n: the step's final scaled iterate
    const int *status;          // [batch] the ADMM's status: only MPCQ_SOLVED QPs are polished
    double *x, *y;              // [batch] n, 2n: the published solution
    const double *U_prev;       // [batch] nu: the caller's U from before the step
    double *U;                  // [batch] nu: U = U_prev + x[0:nu] where polish succeeds
    int *pol_status, *pol_nact; // [batch] OSQP status_polish (1, -1, 0), rows of the reduced system
    double *pol_res;            // [batch][2] primal, dual residual of the returned solution (NaN: not performed)
    double delta;
    int refine, scaled_termination;
};

// Arguments of mimo_plant_vjp_kernel (mpcq_mimo_plant_vjp.hip): the cotangents of the last MIMO step's QP data
// pulled back through the MIMO condensing to the plant data, one workgroup per plant, fp64.
// Everything of the context is read-only.
struct MimoPlantVjpArgs {
    int batch, N, nx, nu, ny, s_rows;
    size_t ops_stride;
    const double *ops;          // [plant] MimoLayout (E is read: the active set's rule)
    const double *u;            // [batch] 2n: the step's unscaled upper bounds (MimoArgs::u_out)
    const double *zs, *ys;      // [batch] 2n: the step's final scaled iterate
    const double *x, *y;        // [batch] n, 2n: the published solution and dual
    const double *gq, *gu;      // [batch] n, 2n: mimo_sens_kernel's gradients for this call's g (n_rhs = 1)
    const int *nact;            // [batch] its n_active: -1 where no sensitivity exists (all-zero outputs)
    const double *Ad, *Bd, *Cd, *Q;  // [plant] nx*nx, nx*nu, ny*nx, ny*ny (the other plant arrays enter linearly)
    const double *X, *U_prev;   // [batch] nx, nu: the step's X and the U from before it
    const double *yref;         // ny, or null: 0
    double *gAd, *gBd, *gCd, *gQ, *gR, *gRD, *gK, *gK0, *gw0;  // [plant] shapes of the plant data; each may be null
    int *n_active;              // [batch] copy of nact (or null)
};

// Arguments of mimo_plant_kernel (mpcq_mimo_run.hip): one plant update of every QP between two control steps of a
// closed-loop MIMO run, with the step's record row and totals.  A 16-lane group per QP, fp64.
struct MimoPlantArgs {
    int batch, nx, nu;
    const double *Ad, *Bd;      // [batch] nx*nx, nx*nu: the simulated plant (mpcq_mimo_set_plant_device)
    double *X;                  // [batch] nx, updated in place
    const double *U;            // [batch] nu, the control the plant sees
    unsigned long long seed;
    long long first_qp, step;   // the noise of QP b at this control step is keyed by (seed, first_qp + b, step)
    double noise_std;
    // the record (each may be null): this step's row of mpcq_mimo_log, already offset to the row, and its totals
    double *log_U, *log_X;      // [batch] nu, nx
    int *log_status, *log_iter; // [batch]
    int *iters_total, *unsolved_total;  // [batch] += iter, += (status != SOLVED)
    const int *status, *iter;   // [batch] the control step's (read only where the record asks for them)
};

// Arguments of mimo_sched_tail_kernel (mpcq_mimo_run.hip): the padded tail of a reference schedule,
// tail[r][j] = sched[r][min(base + j, len - 1)] for j < blocks, blocks of ny values.
struct MimoTailArgs {
    long long rows;             // schedule rows: batch, or 1 for a shared schedule
    long long stride;           // doubles between two rows of sched (unused when rows == 1)
    long long len, base;        // blocks of the schedule; the first block of the tail
    int blocks, ny;             // 2N - 1 blocks per row
    const double *sched;
    double *tail;               // [rows] blocks*ny
};
}  // namespace mpcq

namespace mpcq {
// Arguments of plant_step_kernel (mpcq_plant.hip): condensing + setup + one controllerStep per SISO plant.
struct PlantStepArgs {
    int n_plants, nx, N, s_rows;
    const double *Ad, *Bd, *Cd, *K, *Q, *R, *RD;  // [plant] nx*nx, nx, nx, nx, 1, 1, 1
    const double *X;                               // [plant] nx (device)
    double *U;                                     // [plant]    (device): U += x0 when solved
    double xref;
    SolverSettings st;
    int adaptive_interval;
    double *x, *y, *rho_out;                       // [plant] n, 2n unscaled solution; final rho
    int *status, *iter;
    int *flags;                                    // OR: 1 a plant's KKT matrix is not positive definite
    int wpe;                                       // waves per SIMD of the kernel variant (2; 3: A/B hook)
    int layout;                                    // plants per wave (0: the default, 3 for 17 <= N <= 20;
                                                   // 2: one per 32-lane half, test hook MPCQ_PLANT_LAYOUT)
    // hardest-first (mpcq_order.hip): slot i of the grid runs plant order[i] (null: plant i); workgroup 0
    // zeroes the OrderBins::kBins counters ord_zero for the next sort
    const int *order;
    int *ord_zero;
    long long *stamps;  // debug builds (-DMPCQ_PLANT_STAMPS): 16 per wave, stage clock stamps
};
}  // namespace mpcq

namespace mpcq {
// Arguments of polish_kernel (mpcq_polish.hip): OSQP's solution polishing, one QP per wave, fp64.
struct PolishArgs {
    int batch, n, m, nc, mc;
    int shared;                 // 1: every QP uses plant 0
    int is_f32;                 // the warm state is float (MPCQ_F32 contexts), else double
    size_t ops_stride;
    const double *ops;          // [plant] OpsLayout(nc, mc): W, Winv, D, E, Dinv, Einv, c
    const double *P, *A;        // [plant] n*n (upper triangle read), m*n: the unscaled setup data
    const double *q, *l, *u;    // [batch] n, m, m: this solve's unscaled data
    void *xs, *zs, *ys;         // warm state [batch][nc], [batch][mc] x 2 (read; written where polish succeeds)
    const int *status;          // [batch] the ADMM's status: only MPCQ_SOLVED QPs are polished
    double *x, *y;              // [batch] n, m: the published ADMM solution, overwritten where polish succeeds
    double *U;                  // MPC step: U += x[0] for every SOLVED QP (null otherwise)
    int *pol_status, *pol_nact; // [batch] OSQP status_polish (1, -1, 0), rows of the reduced system
    double *pol_res;            // [batch][2] primal, dual residual of the returned solution (NaN: not performed)
    double delta;
    int refine, scaled_termination;
};

// Arguments of sens_kernel (mpcq_sens.hip): the active-set sensitivities of the last solve, one QP per wave,
// fp64.  Everything of the context is read-only.
struct SensArgs {
    int batch, n, m, nc, mc;
    int shared;                 // 1: every QP uses plant 0
    int is_f32;                 // the warm state is float (MPCQ_F32 contexts), else double
    size_t ops_stride;
    const double *ops;          // [plant] OpsLayout(nc, mc): D, E, c
    const double *P, *A;        // [plant] n*n (upper triangle read), m*n: the unscaled setup data
    const double *l, *u;        // [batch] m, m: the last solve's unscaled bounds
    const void *zs, *ys;        // warm state [batch][mc] x 2
    const int *status;          // [batch] only MPCQ_SOLVED QPs get a sensitivity
    const double *g;            // [batch] n: the cotangent dL/dx, or null: e_0 for every QP
    double *gq, *gl, *gu;       // [batch] n, m, m: dL/dq, dL/dl, dL/du (each may be null)
    int *n_active;              // [batch] rows of the reduced system, -1 where no sensitivity exists (or null)
    double delta;
    int refine;
    unsigned long long *active; // [batch][2] lower-active, upper-active row bit masks; zeros where n_active = -1 (or null)
};

// Arguments of the data-gradient kernels (mpcq_sensdata.hip): gP, gA from a sens_kernel's outputs and the solve's
// x, y.  A QP with n_active < 0 is skipped (none of its arrays is read).  shared: the sums over the batch, by
// sens_contract_kernel (one partial of n*n + m*n doubles per kSensChunk QPs) and sens_reduce_kernel.
constexpr int kSensChunk = 256;
struct SensDataArgs {
    int batch, n, m;
    int shared;                          // 1: gP n*n, gA m*n summed over the batch; 0: one pair per QP
    const double *gq, *gl, *gu;          // [batch] n, m, m
    const double *x, *y;                 // [batch] n, m: the solve's solution and dual
    const unsigned long long *active;    // [batch][2]
    const int *n_active;                 // [batch]
    double *part;                        // [ceil(batch / kSensChunk)][n*n + m*n] (shared plant)
    double *gP, *gA;                     // each may be null
};

// Arguments of sens_chain_kernel (mpcq_sens.hip): the MPC front end's chain rule on (gq, gu).
struct SensChainArgs {
    int batch, n, m, nx;
    int shared;                          // 1: every QP uses plant 0's operators
    const double *Fx, *Fu, *Fr, *Sbar, *Ku;  // [plant] n*nx, n, n*n, m*nx, m
    const double *gq, *gu;               // [batch] n, m
    double *dX, *dU, *dref;              // [batch] nx, 1, n (each may be null)
};
}  // namespace mpcq

// ---- Launchers of the ADMM kernel families, typed on T.
// Every family's kernels are compiled once per variant and dtype, each pair in a translation unit of its own
// (mpcq_<family>[_ref|_log|_reflog]_f32.hip / _f64.hip; mpcq_tile.h MPCQ_TILE_KERNEL says why the split is per
// unit).  A unit defines its pair's piece of the family: an explicit specialisation of the family's *_unit
// template on (Variant, T).  The launch_* dispatchers pick the piece from the pointers they are handed, so which
// variant a call needs is decided here and nowhere else:
//     a reference with data (ref && ref->p): Ref;  a record (lg): Log;  both: RefLog;  neither: Scalar
// (a null or empty reference never reaches a REF unit).  The callers pass the reference only where the kernel's
// front end reads it (mpcq_host_solve.cpp).  Return codes: 0 launched, -1 the variant or the shape (capacity, (KN, KM),
// the tile stream's paired condensed-MPC shape) is not compiled, -2 HIP error.
namespace mpcq {
enum class Variant { Scalar, Ref, Log, RefLog };
inline Variant variant_of(const RefArgs *ref, const LogArgs *lg = nullptr)
{
    const bool r = ref && ref->p;
    return lg ? (r ? Variant::RefLog : Variant::Log) : (r ? Variant::Ref : Variant::Scalar);
}

// One QP per lane (mpcq_admm.h): capacity (nc, mc) of MPCQ_CAPS.
template <Variant V, typename T>
int lane_unit(const AdmmArgs<T> &a, int nc, int mc, const RefArgs *ref, hipStream_t s);
// One QP per wave (mpcq_wave.h): grid blocks of 64 threads stride over the (listed) QPs; n <= 32, m <= 64.
template <Variant V, typename T>
int wave_unit(const AdmmArgs<T> &a, int nc, int mc, int grid, const RefArgs *ref, hipStream_t s);
// The receding-horizon stream in one launch (mpcq_wave.h stream_wave_kernel): every wave owns one QP for all
// sa.steps control steps (solve, U += x0, plant update).
template <Variant V, typename T>
int wave_stream_unit(const AdmmArgs<T> &a, int nc, int mc, const StreamArgs &sa, const RefArgs *ref, const LogArgs *lg,
                     hipStream_t s);
// Tile (MFMA) path for a shared plant (mpcq_tile.h), shape (KN, KM) of MPCQ_TILE_SHAPES: one phase launch, and
// the receding-horizon stream in one launch (AdmmArgs::sim; every column one plant through all its control steps).
template <Variant V, typename T>
int tile_unit(const AdmmArgs<T> &a, int KN, int KM, const RefArgs *ref, hipStream_t s);
template <Variant V, typename T>
int tile_stream_unit(const AdmmArgs<T> &a, int KN, int KM, const RefArgs *ref, const LogArgs *lg, hipStream_t s);
// osqp_warm_start from the unscaled x, y (mpcq_admm_f32.hip / _f64.hip), and the lazily published x, y of the last
// tile solve from its stored warm state (tile_publish_kernel, mpcq_tile_f32.hip / _f64.hip): no variants.
template <typename T>
int launch_warm_start(const AdmmArgs<T> &a, int nc, int mc, const double *x, const double *y, hipStream_t s);
template <typename T>
int launch_tile_publish(const AdmmArgs<T> &a, int KN, int KM, bool paired, hipStream_t s);

// The compiled pieces (one line per translation unit and family).
#define MPCQ_DECLARE_UNITS(T)                                                                                           \
    template <> int lane_unit<Variant::Scalar, T>(const AdmmArgs<T> &, int, int, const RefArgs *, hipStream_t);         \
    template <> int lane_unit<Variant::Ref, T>(const AdmmArgs<T> &, int, int, const RefArgs *, hipStream_t);            \
    template <> int wave_unit<Variant::Scalar, T>(const AdmmArgs<T> &, int, int, int, const RefArgs *, hipStream_t);    \
    template <> int wave_unit<Variant::Ref, T>(const AdmmArgs<T> &, int, int, int, const RefArgs *, hipStream_t);       \
    template <> int wave_stream_unit<Variant::Scalar, T>(const AdmmArgs<T> &, int, int, const StreamArgs &,             \
                                                         const RefArgs *, const LogArgs *, hipStream_t);                \
    template <> int wave_stream_unit<Variant::Ref, T>(const AdmmArgs<T> &, int, int, const StreamArgs &,                \
                                                      const RefArgs *, const LogArgs *, hipStream_t);                   \
    template <> int wave_stream_unit<Variant::RefLog, T>(const AdmmArgs<T> &, int, int, const StreamArgs &,             \
                                                         const RefArgs *, const LogArgs *, hipStream_t);                \
    template <> int tile_unit<Variant::Scalar, T>(const AdmmArgs<T> &, int, int, const RefArgs *, hipStream_t);         \
    template <> int tile_unit<Variant::Ref, T>(const AdmmArgs<T> &, int, int, const RefArgs *, hipStream_t);            \
    template <> int tile_stream_unit<Variant::Scalar, T>(const AdmmArgs<T> &, int, int, const RefArgs *,                \
                                                         const LogArgs *, hipStream_t);                                 \
    template <> int tile_stream_unit<Variant::Ref, T>(const AdmmArgs<T> &, int, int, const RefArgs *, const LogArgs *,  \
                                                      hipStream_t);                                                     \
    template <> int tile_stream_unit<Variant::Log, T>(const AdmmArgs<T> &, int, int, const RefArgs *, const LogArgs *,  \
                                                      hipStream_t);                                                     \
    template <> int tile_stream_unit<Variant::RefLog, T>(const AdmmArgs<T> &, int, int, const RefArgs *,                \
                                                         const LogArgs *, hipStream_t);                                 \
    template <> int launch_warm_start<T>(const AdmmArgs<T> &, int, int, const double *, const double *, hipStream_t);   \
    template <> int launch_tile_publish<T>(const AdmmArgs<T> &, int, int, bool, hipStream_t);
MPCQ_DECLARE_UNITS(float)
MPCQ_DECLARE_UNITS(double)
#undef MPCQ_DECLARE_UNITS

// (the lane, wave and tile phase kernels have no LOG variants: the record is the streams')
template <typename T>
inline int launch_lane(const AdmmArgs<T> &a, int nc, int mc, const RefArgs *ref, hipStream_t s)
{
    return variant_of(ref) == Variant::Ref ? lane_unit<Variant::Ref, T>(a, nc, mc, ref, s)
                                           : lane_unit<Variant::Scalar, T>(a, nc, mc, ref, s);
}
template <typename T>
inline int launch_wave(const AdmmArgs<T> &a, int nc, int mc, int grid, const RefArgs *ref, hipStream_t s)
{
    return variant_of(ref) == Variant::Ref ? wave_unit<Variant::Ref, T>(a, nc, mc, grid, ref, s)
                                           : wave_unit<Variant::Scalar, T>(a, nc, mc, grid, ref, s);
}
template <typename T>
inline int launch_tile(const AdmmArgs<T> &a, int KN, int KM, const RefArgs *ref, hipStream_t s)
{
    return variant_of(ref) == Variant::Ref ? tile_unit<Variant::Ref, T>(a, KN, KM, ref, s)
                                           : tile_unit<Variant::Scalar, T>(a, KN, KM, ref, s);
}
template <typename T>
inline int launch_wave_stream(const AdmmArgs<T> &a, int nc, int mc, const StreamArgs &sa, const RefArgs *ref,
                              const LogArgs *lg, hipStream_t s)
{
    switch (variant_of(ref, lg)) {
    case Variant::Scalar: return wave_stream_unit<Variant::Scalar, T>(a, nc, mc, sa, ref, lg, s);
    case Variant::Ref: return wave_stream_unit<Variant::Ref, T>(a, nc, mc, sa, ref, lg, s);
    case Variant::RefLog: return wave_stream_unit<Variant::RefLog, T>(a, nc, mc, sa, ref, lg, s);
    case Variant::Log: break;  // not compiled: a logged scalar run hands the one-entry schedule [xref] (mpc_run)
    }
    return -1;
}
template <typename T>
inline int launch_tile_stream(const AdmmArgs<T> &a, int KN, int KM, const RefArgs *ref, const LogArgs *lg, hipStream_t s)
{
    switch (variant_of(ref, lg)) {
    case Variant::Scalar: return tile_stream_unit<Variant::Scalar, T>(a, KN, KM, ref, lg, s);
    case Variant::Ref: return tile_stream_unit<Variant::Ref, T>(a, KN, KM, ref, lg, s);
    case Variant::Log: return tile_stream_unit<Variant::Log, T>(a, KN, KM, ref, lg, s);
    case Variant::RefLog: return tile_stream_unit<Variant::RefLog, T>(a, KN, KM, ref, lg, s);
    }
    return -1;
}

// The smallest of a list of compiled capacities (by NC (NC + MC)) that holds an n x m QP: false when none does
// (*nc, *mc untouched).
struct Cap { int nc, mc; };
#define MPCQ_CAP_ITEM(NC_, MC_) {NC_, MC_},
template <int K>
inline bool smallest_cap(const Cap (&caps)[K], int n, int m, int *nc, int *mc)
{
    int best = -1;
    for (const Cap &c : caps)
        if (n <= c.nc && m <= c.mc && (best < 0 || c.nc * (c.nc + c.mc) < best)) {
            best = c.nc * (c.nc + c.mc);
            *nc = c.nc;
            *mc = c.mc;
        }
    return best >= 0;
}

// Launch of a post-pass with one workgroup per QP and `lds` bytes of dynamic LDS (polish, the sensitivities): as
// many workgroups as the LDS lets a CU hold (at most 8) on each of `cus` CUs, striding over the batch.
// static_lds: the kernel's static LDS, counted with the dynamic part against the CU's 160 KiB.  0 launched,
// -1 the LDS does not fit, -2 HIP error (*err).
template <typename Args>
inline int launch_per_qp(void (*kernel)(Args), const Args &a, int batch, int threads, size_t lds, size_t static_lds,
                         int cus, hipStream_t s, hipError_t *err)
{
    constexpr size_t kCuLds = 160 * 1024;
    if (lds + static_lds > kCuLds) return -1;
    if (lds > 64 * 1024 &&
        (*err = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) != hipSuccess)
        return -2;
    const size_t fit = kCuLds / (lds + static_lds);
    const int per_cu = fit > 8 ? 8 : (int)fit, all = (cus > 1 ? cus : 1) * per_cu;  // (fit >= 1: checked above)
    hipLaunchKernelGGL(kernel, dim3(batch < all ? batch : all), dim3(threads), lds, s, a);
    *err = hipGetLastError();
    return *err == hipSuccess ? 0 : -2;
}
}  // namespace mpcq

// Launchers that are not typed on T (extern "C" so the host library links them without templates).
extern "C" {
// OSQP polish of every SOLVED QP (mpcq_polish.hip; n <= 32, m <= 64): 0 launched, -1 unsupported shape,
// -2 HIP error (*err).  cus: compute units of the device (grid size).
int mpcq_internal_polish_launch(const mpcq::PolishArgs *a, int cus, hipStream_t s, hipError_t *err);
// Active-set sensitivities of every SOLVED QP (mpcq_sens.hip; n <= 32, m <= 64), same return codes; and the MPC
// chain rule of the step gains (0 launched, -2 HIP error).
int mpcq_internal_sens_launch(const mpcq::SensArgs *a, int cus, hipStream_t s, hipError_t *err);
int mpcq_internal_sens_chain_launch(const mpcq::SensChainArgs *a, hipStream_t s);
// gP, gA of a sensitivity call (mpcq_sensdata.hip; n <= 32, m <= 64): 0 launched, -1 unsupported shape, -2 HIP error.
int mpcq_internal_sens_data_launch(const mpcq::SensDataArgs *a, hipStream_t s);
int mpcq_internal_setup_launch(const mpcq::SetupArgs *args, hipStream_t stream);
int mpcq_internal_setup_wave_launch(const mpcq::SetupArgs *args, hipStream_t stream);
// Per-plant setup with the direct inverse M(rho)^-1 (mpcq_setup_wave.hip; n <= 32, m <= 64).
int mpcq_internal_setup_inv_launch(const mpcq::SetupArgs *args, hipStream_t stream);
size_t mpcq_internal_setup_wave_lds(int n, int m);
// mpcq_update_P_A_device (mpcq_setup_wave.hip).  The factor stage alone under the scaling the operator blocks hold
// (inv: the direct-inverse reading); the device-side checks, which OR into the setup's flag word: 8 some QP's lower
// bound is not free under the blocks' E, 16 A's lower half is not its negated upper half; and the cold start of
// the QPs whose previous (x, y) is not finite.  0 launched, -1 unsupported shape, -2 HIP error.
int mpcq_internal_setup_keep_launch(const mpcq::SetupArgs *args, int inv, hipStream_t stream);
int mpcq_internal_lower_free_check(const double *l, const double *E, int m, size_t total, int *flags, hipStream_t stream);
int mpcq_internal_paired_check(const double *A, int nn, int *flags, hipStream_t stream);
int mpcq_internal_cold_nonfinite(const double *x, const double *y, int n, int m, int nc, int mc, int batch, int is_f32,
                                 void *xs, void *zs, void *ys, hipStream_t stream);
int mpcq_internal_f64_to_f32(const double *in, float *out, size_t count, hipStream_t s);
int mpcq_internal_broadcast(const double *src, double *dst, int len, int batch, int per_qp_src, hipStream_t s);
int mpcq_internal_fill(void *p, int is_f32, double v, size_t count, hipStream_t s);
int mpcq_internal_caps(int n, int m, int *nc, int *mc);
int mpcq_internal_condense_launch(const mpcq::CondenseArgs *a, hipStream_t s);
size_t mpcq_internal_condense_scratch(int nx, int N);
// 0 launched, -1 a shape the kernel does not serve (N > 32, nx > 8), -2 the launch failed.
int mpcq_internal_condense_vjp_launch(const mpcq::CondenseVjpArgs *a, hipStream_t s);
// Tile (MFMA) path for a shared plant: 1 when (KN, KM) is compiled.
int mpcq_internal_tile_supported(int KN, int KM);
// One row of the record from the context's buffers (mpcq_log.hip; the per-step graph, after the step's plant
// update): U, X as they stand, status and iter of the step's solve.
int mpcq_internal_log_row(int nx, const double *X, const double *U, const int *status, const int *iter,
                          const mpcq::LogArgs *lg, hipStream_t s);
// Plant update of the receding-horizon stream (mpcq_stream.hip); step from *step_p when non-null.
int mpcq_internal_simulate(int batch, int nx, int shared, const double *Ad, const double *Bd, double *X,
                           const double *U, unsigned long long seed, long long first_qp, const long long *step_p,
                           long long step_v, double noise_std, hipStream_t s);
int mpcq_internal_tick(long long *step, hipStream_t s);
int mpcq_internal_front_end(int batch, int nx, int n, int m, const double *Xs, const double *Us, double xref,
                            const double *Fx, const double *Fu, const double *Fr, const double *Sbar,
                            const double *Ku, const double *W0, double *q, double *u, hipStream_t s);
int mpcq_internal_set_step(long long *step, long long v, hipStream_t s);
// Hardest-first order of a shared-plant MPC step (mpcq_order.hip): per-QP bound-violation key from the
// host's OrderBins map, counting-sorted into list (cnt: OrderBins::kBins counters, zero on entry); Xs, Us
// (or null): copies of X, U for the step's q, u on demand.
int mpcq_internal_order(int batch, int nx, int m, const double *X, const double *U, const double *kmap, double xref,
                        int *cnt, int *key, int *list, double *Xs, double *Us, hipStream_t s);
// The same order for a step with per-QP references: the key gains G ref_b, G = -A P^-1 Fr (gmap: m x n,
// row-major, folded by the host next to kmap; the map's xref column is not used).
int mpcq_internal_order_ref(int batch, int nx, int n, int m, const double *X, const double *U, const double *kmap,
                            const double *gmap, const mpcq::RefArgs *ref, int *cnt, int *key, int *list, double *Xs,
                            double *Us, hipStream_t s);
// status[list[i]], iter[list[i]] = slot[2 i], slot[2 i + 1] (an ordered launch's AdmmArgs::info_slot)
int mpcq_internal_order_info(int batch, const int *list, const int *slot, int *status, int *iter, hipStream_t s);
// MIMO condensed MPC (mpcq_mimo.hip): per-plant condensing + Ruiz + P^, then the per-QP solve
// (one 512-thread workgroup per QP: KKT inverse by Gauss-Jordan in VGPRs, structured A).
int mpcq_internal_mimo_setup_launch(const mpcq::MimoSetupArgs *a, hipStream_t s);
int mpcq_internal_mimo_solve_launch(const mpcq::MimoArgs *a, hipStream_t s);
// The same step with a horizon reference per QP in place of a->yref (mimo_solve_ref_kernel): ref +
// b ref_stride holds N*ny values, ref_stride 0 one horizon for the batch.  Same return codes.
int mpcq_internal_mimo_solve_ref_launch(const mpcq::MimoArgs *a, const double *ref, long long ref_stride, hipStream_t s);
// Sensitivities of the last MIMO step with the chain rule as the kernel's tail (mpcq_mimo_sens.hip; every shape
// the MIMO setup accepts): 0 launched, -1 unsupported shape or n_rhs, -2 HIP error (*err).  The workgroup's
// dynamic LDS bytes for n variables: mpcq_internal_mimo_sens_lds.
int mpcq_internal_mimo_sens_launch(const mpcq::MimoSensArgs *a, int cus, hipStream_t s, hipError_t *err);
size_t mpcq_internal_mimo_sens_lds(int n);
// OSQP polish of every SOLVED QP of the last MIMO step (mpcq_mimo_polish.hip; every shape the MIMO setup accepts),
// same return codes; its dynamic LDS bytes for n variables.
int mpcq_internal_mimo_polish_launch(const mpcq::MimoPolishArgs *a, int cus, hipStream_t s, hipError_t *err);
size_t mpcq_internal_mimo_polish_lds(int n);
// The last MIMO step's cotangents pulled back to the plant data (mpcq_mimo_plant_vjp.hip; every shape the MIMO
// setup accepts), same return codes; its dynamic LDS bytes for the call's N, nx, nu, ny.
int mpcq_internal_mimo_plant_vjp_launch(const mpcq::MimoPlantVjpArgs *a, int cus, hipStream_t s, hipError_t *err);
size_t mpcq_internal_mimo_plant_vjp_lds(int N, int nx, int nu, int ny);
// The plant update, record row and totals of one step of a closed-loop MIMO run, and the padded tail of its
// reference schedule (mpcq_mimo_run.hip): 0 launched, -1 unsupported shape, -2 HIP error.
int mpcq_internal_mimo_plant_launch(const mpcq::MimoPlantArgs *a, hipStream_t s);
int mpcq_internal_mimo_sched_tail_launch(const mpcq::MimoTailArgs *a, hipStream_t s);
// One pass per batch of distinct SISO plants (mpcq_plant.hip): condensing + setup + one
// controllerStep per plant, two plants per wave.  0 launched, -1 unsupported shape, -2 HIP error.
int mpcq_internal_plant_step_launch(const mpcq::PlantStepArgs *a, int is_f32, hipStream_t s);
// Build the TileLayout images (type T = f32 if is_f32) of plant 0 from its fp64 operator block.
int mpcq_internal_tile_images(const double *ops, int nc, int mc, int KN, int KM, int is_f32, void *img,
                              hipStream_t s);
}

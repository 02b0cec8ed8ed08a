"""OSQP solution polishing on the device (settings.polish; solvempc_amd/csrc/mpcq_polish.hip).

The oracle (oracle/) has no polish, so this file carries two CPU fp64 numpy references of its own:

* ``_polish_ref`` restates OSQP v0.6 polish.c on a final ADMM iterate: scaled data, OSQP's active-set rule
  (lower-active when z - l < -y, upper-active when u - z < y), the delta-regularised reduced KKT system by
  a plain ``np.linalg.solve`` plus ``polish_refine_iter`` refinement steps against the unregularised
  matrix, project_normalcone, and OSQP's success criterion.  It is applied to the oracle's iterates and
  scaling (the fp64 device trajectory equals the oracle's to ~1e-12, tests/test_gpu.py), and also reports
  the smallest active-set decision margin min(|z - l + y|, |u - z - y|): where that margin is far above the
  trajectory difference, the device must take the same decisions.
* ``_optimum`` does not depend on OSQP's rule: the oracle run at eps_abs = eps_rel = 1e-10, the active set
  read from its duals, and the exact equality-constrained KKT system solved (least squares, so duplicated
  active rows are fine).  Every use asserts stationarity, feasibility, dual sign and complementarity of
  the result to <= 1e-9.

TOL, the bound on the distance of a polished x from ``_optimum`` relative to max(1, ||x*||_inf), comes from
the references alone: max(1e-10, 100 x the largest error of ``_polish_ref`` against ``_optimum`` on the
same inputs); the x100 covers a different elimination order on the device (Cholesky of H and of the Schur
complement instead of an LU of the whole KKT matrix).  Each family asserts its TOL is below 1e-9.

The Python-loop references run on the first 512 QPs of an MPC batch (the device batches are 4,096 on the
tile path); beyond that prefix the tests assert reference-free properties.  The generic families end with
the two unconstrained solves: a QP none of whose rows is active (c) and an m = 0 context (d), where the
polished x is -P^-1 q.

The residuals of ``polish_info()`` are compared with numpy's to rtol 1e-6 plus an absolute floor for
residuals that are themselves rounding noise: a polished point's residual is a difference of O(1) .. O(1e3)
terms that cancel to ~1e-13, so two correct evaluations agree only to a few ulps of those terms; the floor
is 64 eps times the sum of the absolute terms entering the residual's row (the usual bound of a rounded
dot product, its <= 61 terms each rounded once).
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import workload

LMIN = -np.finfo(np.float64).max
EPS = np.finfo(np.float64).eps
F32_TOL = 1e-5  # tests/test_gpu.py's fp32 bar (_f32_close)
PREFIX = 512    # QPs of a batch that get the Python-loop references


# ----------------------------------------------------------------------------- references
def _sym(P):
    P = np.asarray(P, dtype=np.float64)
    return np.triu(P) + np.triu(P, 1).T


def _residuals(Ph, Ah, qh, D, E, c, x, z, y, scaled_term=False):
    """OSQP's primal / dual residual of a scaled point in the termination norm."""
    pri = Ah @ x - z
    dua = Ph @ x + qh + Ah.T @ y
    if not scaled_term:
        pri = pri / E
        dua = dua / D / c
    return float(np.abs(pri).max(initial=0.0)), float(np.abs(dua).max(initial=0.0))


def _polish_ref(P, A, q, l, u, D, E, c, x, z, y, delta=1e-6, refine=3, scaled_term=False):
    """OSQP v0.6 polish.c on the scaled iterate (x, z, y).  Returns a dict: status (1 / -1), n_active,
    the unscaled x and y it would return, their residuals, the decision margin, the scaled polished
    (x, z, y)."""
    n, m = len(q), len(l)
    Ph = c * D[:, None] * _sym(P) * D[None, :]
    Ah = E[:, None] * np.asarray(A, dtype=np.float64).reshape(m, n) * D[None, :]
    qh = c * D * q
    with np.errstate(over="ignore"):
        lh, uh = E * l, E * u
    low = z - lh < -y
    upp = uh - z < y
    with np.errstate(invalid="ignore"):
        margin = float(np.minimum(np.abs(z - lh + y), np.abs(uh - z - y)).min(initial=np.inf))
    Ared = np.vstack([Ah[low], Ah[upp]])
    mr = Ared.shape[0]
    K = np.block([[Ph, Ared.T], [Ared, np.zeros((mr, mr))]])
    Kreg = K + np.diag(np.r_[np.full(n, delta), np.full(mr, -delta)])
    b = np.r_[-qh, lh[low], uh[upp]]
    s = np.linalg.solve(Kreg, b)
    for _ in range(refine):
        s = s + np.linalg.solve(Kreg, b - K @ s)
    xp = s[:n]
    yp = np.zeros(m)
    yp[low] = s[n:n + int(low.sum())]
    yp[upp] = s[n + int(low.sum()):]
    t = Ah @ xp + yp
    zp = np.clip(t, lh, uh)
    yp = t - zp
    pri_a, dua_a = _residuals(Ph, Ah, qh, D, E, c, x, z, y, scaled_term)
    pri_p, dua_p = _residuals(Ph, Ah, qh, D, E, c, xp, zp, yp, scaled_term)
    ok = (pri_p < pri_a and dua_p < dua_a) or (pri_p < pri_a and dua_a < 1e-10) or (dua_p < dua_a and pri_a < 1e-10)
    xs, zs, ys = (xp, zp, yp) if ok else (x, z, y)
    return dict(status=1 if ok else -1, n_active=mr, x=D * xs, y=E * ys / c, pri=pri_p if ok else pri_a,
                dua=dua_p if ok else dua_a, margin=margin, scaled=(xs, zs, ys))


_TIGHT = dict(eps_abs=1e-10, eps_rel=1e-10, max_iter=200000)


def _optimum(P, A, q, l, u, solver=None):
    """The QP's optimum, independent of OSQP's polish rule: active set from the duals of a 1e-10 oracle solve,
    then the exact equality-constrained KKT system.  Asserts the KKT conditions of the result to 1e-9.
    Returns (x, y)."""
    n, m = len(q), len(l)
    A = np.asarray(A, dtype=np.float64).reshape(m, n)
    if solver is None:
        solver = oracle.Solver(P, q, A, l, u, oracle.default_settings(**_TIGHT))
    assert solver.solve() == oracle.SOLVED
    y0 = solver.y()
    thr = 1e-9 * max(1.0, float(np.abs(y0).max(initial=0.0)))
    up, lo = y0 > thr, y0 < -thr
    act = up | lo
    Aa = A[act]
    ba = np.where(up, u, l)[act]
    k = Aa.shape[0]
    K = np.block([[_sym(P), Aa.T], [Aa, np.zeros((k, k))]])
    s = np.linalg.lstsq(K, np.r_[-q, ba], rcond=None)[0]
    x = s[:n]
    y = np.zeros(m)
    y[act] = s[n:]
    r = oracle.kkt_residuals(P, q, A, l, u, x, y)
    scale = max(1.0, float(np.abs(x).max()), float(np.abs(q).max()))
    assert max(r.values()) <= 1e-9 * scale, r
    # complementarity's missing half: an active multiplier has the sign of its bound
    assert np.all(y[up] >= -1e-9 * scale) and np.all(y[lo] <= 1e-9 * scale)
    return x, y


def _rel_err(x, x_opt):
    return np.abs(x - x_opt).max(axis=-1) / np.maximum(1.0, np.abs(x_opt).max(axis=-1))


def _tol(ref_x, ref_status, x_opt):
    """TOL of a family of inputs from its two references (module docstring); asserted below 1e-9."""
    ok = ref_status == 1
    err = float(_rel_err(ref_x[ok], x_opt[ok]).max(initial=0.0))
    tol = max(1e-10, 100.0 * err)
    assert tol < 1e-9, (err, tol)
    return tol


# ----------------------------------------------------------------------------- the MPC family
def _problem(plant, N, B, seed=1, u_range=1.0, start=0):
    ops = oracle.condense(plant, N)
    X, U = workload.mpc_states(seed, start, B, u_range)
    return ops, X, U, oracle.gradient(ops, X, U), oracle.upper_bound(ops, X, U)


@functools.lru_cache(maxsize=None)
def _mpc_refs(N, seed, count=PREFIX):
    """Both references on the first `count` QPs of _problem(plant, N, ., seed): computed once per session."""
    plant = workload.reference_plant()
    ops, X, U, q, u = _problem(plant, N, count, seed)
    l = np.full(2 * N, LMIN)
    u0 = oracle.upper_bound(ops, np.zeros(4), 0.0)
    ref = oracle.Solver(ops["P"], np.zeros(N), ops["A"], l, u0)
    tight = oracle.Solver(ops["P"], np.zeros(N), ops["A"], l, u0, oracle.default_settings(**_TIGHT))
    D, E, c = ref.scaling()
    out = dict(status=[], n_active=[], x=[], y=[], pri=[], dua=[], margin=[], x_admm=[], y_admm=[], x_opt=[], st=[],
               it=[])
    for b in range(count):
        # (a fresh solver state per QP, as oracle.batch_solve gives every QP its template's)
        ref = oracle.Solver(ops["P"], np.zeros(N), ops["A"], l, u0)
        ref.update_gradient(q[b])
        ref.update_upper_bound(u[b])
        out["st"].append(ref.solve())
        out["it"].append(ref.info().iter)
        out["x_admm"].append(ref.x())
        out["y_admm"].append(ref.y())
        r = _polish_ref(ops["P"], ops["A"], q[b], l, u[b], D, E, c, *ref.iterates())
        for k in ("status", "n_active", "x", "y", "pri", "dua", "margin"):
            out[k].append(r[k])
        tight.update_gradient(q[b])
        tight.update_upper_bound(u[b])
        tight.cold_start()
        out["x_opt"].append(_optimum(ops["P"], ops["A"], q[b], l, u[b], tight)[0])
    out = {k: np.asarray(v) for k, v in out.items()}
    out["tol"] = _tol(out["x"], out["status"], out["x_opt"])
    out.update(ops=ops, q=q, u=u, l=l, D=D, E=E, c=c)
    return out


# ----------------------------------------------------------------------------- generic per-plant families
def _generic_inputs(kind):
    """Seeded per-plant QPs (one (P, A) per QP).  a: n 8, m 12, random A, two-sided bounds, rows 0-1
    equalities, rows 2-3 without a lower bound; b: n 4, m 8, A = [I; I] with duplicated u (both copies of a
    row active: up to 8 > n reduced rows, a rank-deficient reduced system); c: wide bounds, no active row;
    d: no constraint at all (m = 0)."""
    rng = np.random.default_rng({"a": 11, "b": 12, "c": 13, "d": 14}[kind])
    n, m, B = {"a": (8, 12, 128), "b": (4, 8, 64), "c": (4, 8, 32), "d": (4, 0, 32)}[kind]
    P, A, q, l, u = [], [], [], [], []
    for b in range(B):
        M = rng.normal(size=(n, n))
        if kind == "a":
            P.append(M @ M.T + 0.1 * np.eye(n))
            A.append(rng.normal(size=(m, n)))
            q.append(rng.normal(size=n))
            lo, up = -rng.uniform(0.5, 2.0, size=m), rng.uniform(0.5, 2.0, size=m)
            lo[:2] = up[:2] = 0.1 * rng.normal(size=2)
            lo[2:4] = LMIN
        elif kind == "b":
            Pb = np.diag(rng.uniform(1.0, 2.0, size=n)) + 0.05 * (M + M.T)
            P.append(Pb)
            A.append(np.vstack([np.eye(n), np.eye(n)]))
            up = np.tile(rng.uniform(0.2, 1.0, size=n), 2)
            lo = np.full(m, LMIN)
            # even QPs: the unconstrained optimum beyond u in every coordinate (all 2n rows active); odd: random
            q.append(-Pb @ (up[:n] + rng.uniform(0.5, 2.0, size=n)) if b % 2 == 0 else 2.0 * rng.normal(size=n))
        else:  # (c, d)
            P.append(M @ M.T + 0.5 * np.eye(n))
            A.append(rng.normal(size=(m, n)))
            q.append(rng.normal(size=n))
            lo, up = np.full(m, -100.0), np.full(m, 100.0)
        l.append(lo)
        u.append(up)
    return tuple(np.stack(v) for v in (P, A, q, l, u))


@functools.lru_cache(maxsize=None)
def _generic_refs(kind):
    P, A, q, l, u = _generic_inputs(kind)
    B = len(q)
    out = dict(st=[], it=[], status=[], n_active=[], x=[], margin=[], x_opt=[])
    for b in range(B):
        ref = oracle.Solver(P[b], q[b], A[b], l[b], u[b])
        st = ref.solve()
        out["st"].append(st)
        out["it"].append(ref.info().iter)
        if st != oracle.SOLVED:  # (polish not performed)
            out["status"].append(0); out["n_active"].append(0); out["margin"].append(np.inf)
            out["x"].append(np.full(len(q[b]), np.nan)); out["x_opt"].append(np.full(len(q[b]), np.nan))
            continue
        r = _polish_ref(P[b], A[b], q[b], l[b], u[b], *ref.scaling(), *ref.iterates())
        for k in ("status", "n_active", "x", "margin"):
            out[k].append(r[k])
        out["x_opt"].append(_optimum(P[b], A[b], q[b], l[b], u[b])[0])
    out = {k: np.asarray(v) for k, v in out.items()}
    out["tol"] = _tol(out["x"], out["status"], out["x_opt"])
    return out


# ----------------------------------------------------------------------------- CPU tests
def test_default_polish_settings():
    s = sm.default_settings()
    assert (s.polish, s.polish_refine_iter, s.delta) == (0, 3, 1e-6)
    assert sm.default_settings(polish=1).polish == 1


@pytest.mark.parametrize("over", [dict(delta=0.0), dict(delta=-1e-6), dict(polish_refine_iter=-1)])
def test_polish_settings_validated(over):
    with pytest.raises(sm.MpcqError) as e:
        sm.BatchSolver(20, 40, 16, settings=sm.default_settings(polish=1, **over))
    assert e.value.code == sm._capi.MPCQ_ERR_ARG


def test_polish_refuses_shapes_beyond_its_capacity():
    with pytest.raises(sm.MpcqError) as e:
        sm.BatchSolver(40, 80, 4, n_plants=4, settings=sm.default_settings(polish=1))
    assert e.value.code == sm._capi.MPCQ_ERR_ARG


@pytest.mark.parametrize("N,seed", [(20, 1), (15, 3)])
def test_polish_ref_reaches_the_optimum_mpc(N, seed):
    """_polish_ref against _optimum on the GPU tests' MPC inputs: validates the reference and yields TOL.  The
    unpolished iterate is >= 1e-5 away on hundreds of these QPs; (15, 3) holds the one QP of the prefix whose
    polish OSQP's criterion rejects."""
    r = _mpc_refs(N, seed)
    assert np.all(r["st"] == oracle.SOLVED)
    ok = r["status"] == 1
    assert r["tol"] < 1e-9 and _rel_err(r["x"][ok], r["x_opt"][ok]).max() <= 1e-12
    assert (np.abs(r["x_admm"] - r["x_opt"]).max(axis=1) >= 1e-5).sum() >= 200
    assert r["margin"].min() >= 1e-9  # every active-set decision of the prefix is clear of a tie
    if (N, seed) == (15, 3):
        assert (~ok).sum() == 1
    print(f"N={N} seed={seed}: ref err {_rel_err(r['x'][ok], r['x_opt'][ok]).max():.2e}, TOL {r['tol']:.1e}, "
          f"{int((~ok).sum())} unsuccessful, min margin {r['margin'].min():.2e}")


@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
def test_polish_ref_reaches_the_optimum_generic(kind):
    r = _generic_refs(kind)
    ok = r["status"] == 1
    assert r["tol"] < 1e-9 and ok.sum() >= 0.9 * len(ok)
    if kind == "b":
        assert r["n_active"].max() == 8  # more reduced rows than variables
    if kind in "cd":
        assert np.all(r["n_active"][r["status"] != 0] == 0)
    print(f"generic {kind}: {int(ok.sum())} of {len(ok)} successful, TOL {r['tol']:.1e}, n_active "
          f"{r['n_active'].min()}..{r['n_active'].max()}, min margin {r['margin'].min():.2e}")


def test_flops_polish_hand_count():
    """flops_polish counts what mpcq_polish.hip performs.  By hand, with chol(N) = (N-1)N(N+1)/3 (the column
    updates) + N(N-1)/2 (the scalings) + 2N (sqrt, reciprocal), solve(N) = 2N^2 (both triangles):
    factorisation chol(n) + mr n^2 (V = L^-1 A_red') + n mr (mr + 1) (S) + chol(mr);
    one KKT solve 2 solve(n) + solve(mr) + 4 n mr + mr; one refinement step 2n^2 + 4 n mr + n + mr + a solve.
    (4, 0): chol(4) = 20 + 6 + 8 = 34, solve = 64, step = 32 + 4 + 64 = 100: 34 + 64 + 3 * 100 = 398.
    (20, 11): chol(20) = 2660 + 190 + 40 = 2890, chol(11) = 440 + 55 + 22 = 517,
    factorisation 2890 + 4400 + 2640 + 517 = 10447, solve 1600 + 242 + 880 + 11 = 2733,
    step 800 + 880 + 31 + 2733 = 4444: 10447 + 2733 + 3 * 4444 = 26512."""
    assert workload.flops_polish(4, 0, 3) == 398
    assert workload.flops_polish(20, 11, 3) == 26512
    assert workload.flops_polish(20, 11, 0) == 10447 + 2733


def test_polish_kernel_is_listed_once_without_scratch():
    import tools.kernel_resources as kr
    if not os.path.isdir(kr.BUILD) or shutil.which("c++filt") is None or \
            not os.path.exists(f"{kr.LLVM}/clang-offload-bundler"):
        pytest.skip("needs the built objects and the ROCm LLVM tools")
    hit = [r for r in kr.table() if "polish_kernel" in r["kernel"]]
    assert len(hit) == 1, [r["kernel"] for r in hit]
    assert hit[0]["scratch"] == 0 and hit[0]["vgpr_spill"] == 0


EIGEN = "/root/reference/include"  # (tests/test_cpp_surface.py: the only Eigen this project's tests know)


@pytest.mark.skipif(not os.path.exists(os.path.join(EIGEN, "Eigen", "Dense")),
                    reason="needs an Eigen include directory")
def test_osqp_eigen_polish_settings(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "polish_settings.cpp"
    src.write_text('#include <cstdio>\n#include "OsqpEigen/OsqpEigen.h"\n'
                   "int main() {\n  OsqpEigen::Solver s;\n  s.settings()->setPolish(true);\n"
                   "  s.settings()->setDelta(1e-5);\n  s.settings()->setPolishRefineIter(5);\n"
                   "  const mpcq_settings &r = s.settings()->getSettings();\n"
                   '  std::printf("%d %.17g %d %d\\n", r.polish, r.delta, r.polish_refine_iter, s.getPolishStatus());\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "polish_settings"
    lib = os.path.join(root, "solvempc_amd")
    subprocess.run(["g++", "-std=c++11", "-O0", f"-I{EIGEN}", f"-I{os.path.join(root, 'include')}", "-o", str(exe),
                    str(src), f"-L{lib}", "-lmpcq", f"-Wl,-rpath,{lib}"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert (int(out[0]), float(out[1]), int(out[2]), int(out[3])) == (1, 1e-5, 5, 0)


# ----------------------------------------------------------------------------- GPU tests
gpu = pytest.mark.gpu


@pytest.fixture(params=["tile", "wave", "lane"])
def kernel(request, monkeypatch):
    """Every device path, forced through the MPCQ_KERNEL test hook (tests/test_gpu.py's fixture)."""
    monkeypatch.setenv("MPCQ_KERNEL", request.param)
    return request.param


def _setup_mpc(ops, N, B, dtype="f64", settings=None):
    s = sm.BatchSolver(N, 2 * N, B, dtype=dtype, settings=settings)
    s.setup(ops["P"], np.zeros(N), ops["A"], np.full(2 * N, LMIN), oracle.upper_bound(ops, np.zeros(4), 0.0))
    return s


def _gpu_solve(ops, q, u, N, dtype="f64", settings=None):
    s = _setup_mpc(ops, N, q.shape[0], dtype, settings)
    s.update_lin_cost(q)
    s.update_upper_bound(u)
    s.solve()
    return s


def _results(s):
    out = dict(x=s.solution(), y=s.dual())
    out["st"], out["it"], out["rho"] = s.info()
    out["sp"], out["na"], out["pri"], out["dua"] = s.polish_info()
    return out


def _kkt_mpc(ops, q, u, x, y):
    """Largest violation per QP of stationarity, primal feasibility, dual sign and complementarity (l = -inf)."""
    Ax = x @ ops["A"].T
    stat = np.abs(x @ _sym(ops["P"]) + q + y @ ops["A"]).max(axis=1)
    prim = np.maximum(Ax - u, 0).max(axis=1)
    sign = np.maximum(-y, 0).max(axis=1)
    compl = np.abs(y * (u - Ax)).max(axis=1)
    return np.maximum(np.maximum(stat, prim), np.maximum(sign, compl))


def _assert_kkt_where_converged(ops, q, u, r, r0=None):
    """Whole-batch optimality without a reference.  OSQP's criterion accepts a polish that merely reduces
    the ADMM's residuals, so a wrong active-set guess can end "successful" at a point that is not the optimum
    (the CPU reference itself does so on QP 2693 of (N 20, seed 1), returning status 1 with a primal residual
    of 2.9e-3, and on QP 3805 of (15, 3)); such a QP shows in polish_info()'s residuals.  Wherever those say the
    polished point converged (dual residual <= 1e-9, primal residual times max(1, ||y||_inf) <= 1e-9: the
    residual bounds the primal violation, and times |y| the complementarity gap) the returned (x, y) must be a
    KKT point to 1e-8.  The polished QPs that did not converge are at most 0.1 % (at least one allowed): the
    CPU reference's own rate on these inputs is 1 in 4,096 for both seeds.  With the polish-off results r0,
    each of those must still be no worse than the ADMM's answer on a measure that needs no reference: its
    stationarity residual ||P x + q + A' y||_inf, which is OSQP's unscaled dual residual and which the success
    criterion requires to have gone down (the ADMM's is ~1e-4 here, never below 1e-10), and its primal
    violation within the primal residual polish_info() reports (z <= u)."""
    ok = r["sp"] == 1
    conv = ok & (r["dua"] <= 1e-9) & (r["pri"] * np.maximum(1.0, np.abs(r["y"]).max(axis=1)) <= 1e-9)
    left = np.flatnonzero(ok & ~conv)
    assert left.size <= max(1, ok.sum() // 1000), (left, int(ok.sum()))
    if r0 is not None and left.size:
        Ps = _sym(ops["P"])
        stat = lambda x, y: np.abs(x @ Ps + q[left] + y @ ops["A"]).max(axis=1)
        s1, s0 = stat(r["x"][left], r["y"][left]), stat(r0["x"][left], r0["y"][left])
        assert np.all(s1 <= s0), (left, s1, s0)
        viol = np.maximum(r["x"][left] @ ops["A"].T - u[left], 0).max(axis=1)
        assert np.all(viol <= r["pri"][left] * (1 + 1e-6) + 1e-12), (left, viol, r["pri"][left])
    kkt = _kkt_mpc(ops, q[conv], u[conv], r["x"][conv], r["y"][conv])
    assert kkt.max() <= 1e-8, (kkt.max(), np.flatnonzero(conv)[np.argmax(kkt)])
    return int(conv.sum()), float(kkt.max())


def _check_info_residuals(r, ref, P, A, q, l, u, D, E, c, idx):
    """polish_info()'s residuals are those of the returned solution (module docstring for the floor): where
    polish succeeded recomputed from the returned (x, y) with z = clip(A^ x^ + y^, l^, u^); where it did not,
    the ADMM iterate's, whose z the oracle's iterate supplies (ref pri / dua)."""
    Ph = c * D[:, None] * _sym(P) * D[None, :]
    Ah = E[:, None] * A * D[None, :]
    with np.errstate(over="ignore"):
        lh, uh = E * l, E * u
    for b in idx:
        if r["sp"][b] == 1:
            xh, yh, qh = r["x"][b] / D, c * r["y"][b] / E, c * D * q[b]
            zh = np.clip(Ah @ xh + yh, lh, uh[b] if uh.ndim == 2 else uh)
            pri, dua = _residuals(Ph, Ah, qh, D, E, c, xh, zh, yh)
            fl_p = 64 * EPS * ((np.abs(Ah) @ np.abs(xh) + np.abs(zh)) / E).max()
            fl_d = 64 * EPS * ((np.abs(Ph) @ np.abs(xh) + np.abs(qh) + np.abs(Ah).T @ np.abs(yh)) / D / c).max()
        else:
            pri, dua, fl_p, fl_d = ref["pri"][b], ref["dua"][b], 1e-12, 1e-12
        assert abs(r["pri"][b] - pri) <= 1e-6 * pri + fl_p, (b, r["sp"][b], r["pri"][b], pri)
        assert abs(r["dua"][b] - dua) <= 1e-6 * dua + fl_d, (b, r["sp"][b], r["dua"][b], dua)


@gpu
@pytest.mark.parametrize("N,seed", [(20, 1), (15, 3)])
def test_fp64_polish_every_path(plant, kernel, N, seed):
    """fp64 polish on the tile, wave and lane paths: the ADMM's status and iterations unchanged; on the
    reference prefix OSQP's status_polish and active-set size, the optimum within TOL and the KKT conditions
    to 1e-8 on every polished QP; on the whole batch the KKT conditions wherever polish converged
    (_assert_kkt_where_converged); rejected polishes leave the ADMM result bit for bit."""
    B = 4096 if kernel == "tile" else 512
    ref = _mpc_refs(N, seed)
    ops, X, U, q, u = _problem(plant, N, B, seed)
    off = _gpu_solve(ops, q, u, N)
    assert off.path()[0] == kernel
    r0 = _results(off)
    off.close()
    on = _gpu_solve(ops, q, u, N, settings=sm.default_settings(polish=1))
    assert on.path()[0] == kernel
    r = _results(on)
    D, E, c = on.scaling()
    on.close()
    assert np.array_equal(r["st"], r0["st"]) and np.array_equal(r["it"], r0["it"])
    assert np.array_equal(r["st"][:PREFIX], ref["st"]) and np.array_equal(r["it"][:PREFIX], ref["it"])
    clear = ref["margin"] >= 1e-9
    assert np.array_equal(r["sp"][:PREFIX][clear], ref["status"][clear])
    assert np.array_equal(r["na"][:PREFIX][clear], ref["n_active"][clear])
    if (N, seed) == (15, 3):
        assert (r["sp"][:PREFIX] == -1).sum() == 1  # the reference's one rejected polish
    ok = r["sp"] == 1
    err = _rel_err(r["x"][:PREFIX], ref["x_opt"])
    okp = np.flatnonzero(ok[:PREFIX])
    kkt = _kkt_mpc(ops, q[okp], u[okp], r["x"][okp], r["y"][okp])
    print(f"{kernel} N={N} seed={seed}: {int(ok.sum())} of {B} polished, max rel err vs optimum "
          f"{err[okp].max():.2e} (TOL {ref['tol']:.1e}), unpolished {_rel_err(r0['x'][:PREFIX], ref['x_opt']).max():.2e}, "
          f"KKT on the prefix {kkt.max():.2e}")
    assert np.all(r["st"] == sm.SOLVED) and np.all(r["sp"] != 0)
    assert err[okp].max() <= ref["tol"]
    assert kkt.max() <= 1e-8
    print("  whole batch: %d converged, KKT %.2e" % _assert_kkt_where_converged(ops, q, u, r, r0))
    assert np.array_equal(r["x"][~ok], r0["x"][~ok]) and np.array_equal(r["y"][~ok], r0["y"][~ok])
    _check_info_residuals(r, ref, ops["P"], ops["A"], q, ref["l"], u, D, E, c, range(PREFIX))


@gpu
@pytest.mark.parametrize("dtype", ["mixed", "f32"])
@pytest.mark.parametrize("N,seed", [(20, 1), (15, 3)])
def test_reduced_precision_polish_reaches_the_fp64_optimum(plant, monkeypatch, dtype, N, seed):
    """mixed and f32 iterates on the tile path: polish (fp64) turns them into the fp64 optimum.  Counted on the
    reference prefix: the QPs that are not (status_polish == 1 and within TOL of _optimum) are at most 2 %, and
    each of those still meets tests/test_gpu.py's fp32 bar against the oracle's unpolished x."""
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    B = 4096
    ref = _mpc_refs(N, seed)
    ops, X, U, q, u = _problem(plant, N, B, seed)
    s = _gpu_solve(ops, q, u, N, dtype=dtype, settings=sm.default_settings(polish=1))
    assert s.path()[0] == "tile"
    r = _results(s)
    s.close()
    assert np.all(r["st"] == sm.SOLVED)
    err = _rel_err(r["x"][:PREFIX], ref["x_opt"])
    good = (r["sp"][:PREFIX] == 1) & (err <= ref["tol"])
    left = np.flatnonzero(~good)
    print(f"{dtype} N={N} seed={seed}: {left.size} of {PREFIX} not polished to the optimum; polished max rel err "
          f"{err[good].max():.2e}; whole batch {int((r['sp'] == 1).sum())} of {B} polished")
    assert left.size <= 0.02 * PREFIX
    if left.size:
        scale = np.maximum(1.0, np.abs(ref["x_admm"][left]).max(axis=1))
        e = np.abs(r["x"][:PREFIX][left] - ref["x_admm"][left]).max(axis=1) / scale
        assert e.max() < F32_TOL, (left, e)


class _DevArray:
    """A device buffer of the C ABI's device view, wrapped for torch (__cuda_array_interface__)."""

    def __init__(self, ptr, shape, typestr="<f8"):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3}


@gpu
def test_mpc_step_applies_the_polished_move(plant, kernel, monkeypatch):
    """mpc_step and mpc_step_device on every path (the ADMM launch leaves U alone, so the wave and lane front
    ends must still read it for q and u): the applied move is the polished x[0] (U_new = U + x[0]
    in fp64, exactly), the optimum's move within TOL where polish succeeded; get_solution, dual, info and the
    device view agree; lazy and eager publication (MPCQ_LAZY_XY) give the same bits."""
    import torch
    N, B = 20, 4096 if kernel == "tile" else 512
    ref = _mpc_refs(N, 1)
    ops, X, U, q, u = _problem(plant, N, B, 1)

    def run(lazy, device):
        if lazy:
            monkeypatch.delenv("MPCQ_LAZY_XY", raising=False)
        else:
            monkeypatch.setenv("MPCQ_LAZY_XY", "0")
        s = _setup_mpc(ops, N, B, settings=sm.default_settings(polish=1))
        s.mpc_set_operators(ops["Fx"], ops["Fu"], ops["Fr"], ops["Sbar"], ops["Ku"], ops["W0"])
        if device:
            Xd, Ud = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(U.copy()).cuda()
            s.mpc_step_device(Xd.data_ptr(), Ud.data_ptr(), 0.0)
            torch.cuda.synchronize()
            Un = Ud.cpu().numpy()
        else:
            Un = s.mpc_step(X, U)
        assert s.path()[0] == kernel
        r = _results(s)
        v = s.device_view()
        torch.cuda.synchronize()
        r["xv"] = torch.as_tensor(_DevArray(v["x"], (B, N)), device="cuda").cpu().numpy()
        r["yv"] = torch.as_tensor(_DevArray(v["y"], (B, 2 * N)), device="cuda").cpu().numpy()
        r["stv"] = torch.as_tensor(_DevArray(v["status"], (B,), "<i4"), device="cuda").cpu().numpy()
        r["itv"] = torch.as_tensor(_DevArray(v["iter"], (B,), "<i4"), device="cuda").cpu().numpy()
        r["U"] = Un
        s.close()
        return r

    runs = [run(True, True), run(False, True), run(True, False)]
    r = runs[0]
    for o in runs[1:]:
        for k in r:
            assert np.array_equal(r[k], o[k], equal_nan=True), k
    assert np.all(r["st"] == sm.SOLVED)
    assert np.array_equal(r["U"], U + r["x"][:, 0])
    assert np.array_equal(r["xv"], r["x"]) and np.array_equal(r["yv"], r["y"])
    assert np.array_equal(r["stv"], r["st"]) and np.array_equal(r["itv"], r["it"])
    assert np.array_equal(r["st"][:PREFIX], ref["st"]) and np.array_equal(r["it"][:PREFIX], ref["it"])
    ok = r["sp"][:PREFIX] == 1
    assert np.array_equal(r["sp"][:PREFIX], ref["status"]) and ok.all()
    scale = np.maximum(1.0, np.abs(ref["x_opt"]).max(axis=1))
    move = np.abs((r["U"] - U)[:PREFIX] - ref["x_opt"][:, 0]) / scale
    assert move[ok].max() <= ref["tol"] + 4 * EPS * np.abs(U).max()  # (U + x0 - U rounds at U's magnitude)
    _assert_kkt_where_converged(ops, q, u, r)


@gpu
def test_warm_start_after_polish(plant, monkeypatch):
    """The warm state after a successful polish is the polished point, as in OSQP: a second solve() on
    unchanged data follows an oracle solve warm-started with warm_start(x_pol, y_pol) (same status, same
    iteration count), and returns the polish of that solve's iterate to 1e-9."""
    monkeypatch.setenv("MPCQ_KERNEL", "wave")
    N, B = 20, 512
    ref = _mpc_refs(N, 1)
    ops, X, U, q, u = _problem(plant, N, B, 1)
    s = _gpu_solve(ops, q, u, N, settings=sm.default_settings(polish=1))
    assert s.path()[0] == "wave"
    r1 = _results(s)
    s.solve()
    r2 = _results(s)
    s.close()
    assert np.array_equal(r1["sp"], ref["status"])
    l = ref["l"]
    u0 = oracle.upper_bound(ops, np.zeros(4), 0.0)
    for b in range(B):
        o = oracle.Solver(ops["P"], np.zeros(N), ops["A"], l, u0)
        o.update_gradient(q[b])
        o.update_upper_bound(u[b])
        o.solve()
        o.warm_start(r1["x"][b], r1["y"][b])
        st = o.solve()
        assert (st, o.info().iter) == (r2["st"][b], r2["it"][b]), b
        p = _polish_ref(ops["P"], ops["A"], q[b], l, u[b], ref["D"], ref["E"], ref["c"], *o.iterates())
        if p["margin"] >= 1e-9:
            assert p["status"] == r2["sp"][b], b
            assert np.abs(p["x"] - r2["x"][b]).max() <= 1e-9, b


@gpu
@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
def test_generic_shapes_per_plant(kind):
    """Generic QPs on the per-plant one-QP-per-wave path: equalities, rows without a lower bound, two-sided
    rows (a); more active rows than variables, a rank-deficient reduced system held by delta (b); no active
    row, the unconstrained solve (c); an m = 0 context, where every QP must end polished at x = -P^-1 q with
    an empty reduced system and an empty dual (d)."""
    ref = _generic_refs(kind)
    P, A, q, l, u = _generic_inputs(kind)
    B, n = q.shape
    m = l.shape[1]
    s = sm.BatchSolver(n, m, B, n_plants=B, settings=sm.default_settings(polish=1))
    s.setup(P, q, A, l, u)
    s.solve()
    assert s.path()[0] == "wave"
    r = _results(s)
    s.close()
    assert np.array_equal(r["st"], ref["st"]) and np.array_equal(r["it"], ref["it"])
    clear = ref["margin"] >= 1e-9
    assert np.array_equal(r["sp"][clear], ref["status"][clear])
    assert np.array_equal(r["na"][clear], ref["n_active"][clear])
    ok = (r["sp"] == 1) & (ref["status"] == 1)
    err = _rel_err(r["x"][ok], ref["x_opt"][ok])
    print(f"generic {kind}: {int((r['sp'] == 1).sum())} of {B} polished, n_active {r['na'].min()}..{r['na'].max()}, "
          f"max rel err {err.max():.2e} (TOL {ref['tol']:.1e}), {int((~clear).sum())} ties")
    assert err.max() <= ref["tol"]
    nsol = r["st"] != sm.SOLVED
    assert np.all(r["sp"][nsol] == 0) and np.all(np.isnan(r["pri"][nsol]))
    if kind == "d":
        x_unc = np.stack([np.linalg.solve(_sym(P[b]), -q[b]) for b in range(B)])
        assert np.all(r["st"] == sm.SOLVED) and np.all(r["sp"] == 1) and np.all(r["na"] == 0)
        assert _rel_err(r["x"], x_unc).max() <= ref["tol"]
        assert r["y"].shape == (B, 0) and np.all(r["pri"] == 0.0)


def _infeasible_batch(plant, N, B):
    """tests/test_gpu.py test_infeasible_statuses_match_oracle's batch: five primal-infeasible QPs."""
    ops, X, U, q, u = _problem(plant, N, B)
    u = u.copy()
    bad = {7: (slice(None), -1e3), 8: (slice(None), -1e3), 1000: (slice(None), -1.0), 2001: ([3, N + 3], -5.0),
           4090: ([0, N + 0], -0.5)}
    for i, (rows, c) in bad.items():
        u[i, rows] = c
    return ops, q, u, np.array(sorted(bad))


@gpu
def test_unsolved_qps_are_not_polished(plant):
    N, B = 20, 16384
    ops, q, u, bad = _infeasible_batch(plant, N, B)
    off = _gpu_solve(ops, q, u, N)
    assert off.path()[0] == "tile"
    r0 = _results(off)
    off.close()
    on = _gpu_solve(ops, q, u, N, settings=sm.default_settings(polish=1))
    r = _results(on)
    on.close()
    assert np.all(r["st"][bad] == sm.PRIMAL_INFEASIBLE) and np.array_equal(r["st"], r0["st"])
    assert np.array_equal(r["it"], r0["it"])
    assert np.all(r["sp"][bad] == 0) and np.all(r["na"][bad] == 0)
    assert np.all(np.isnan(r["pri"][bad])) and np.all(np.isnan(r["dua"][bad]))
    assert np.array_equal(r["x"][bad], r0["x"][bad], equal_nan=True)
    assert np.array_equal(r["y"][bad], r0["y"][bad], equal_nan=True)
    ok = np.setdiff1d(np.arange(B), bad)
    assert np.all(r["sp"][ok] != 0)


@gpu
def test_single_launch_paths_refuse_polish(plant):
    import torch
    N, B = 20, 64
    ops = oracle.condense(plant, N)
    on = sm.default_settings(polish=1)
    with pytest.raises(sm.MpcqError) as e:
        sm.BatchSolver(40, 80, 4, n_plants=4, settings=on)
    assert e.value.code == sm._capi.MPCQ_ERR_ARG
    X, U = workload.mpc_states(1, 0, B)
    Xd, Ud = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(U.copy()).cuda()
    s = _setup_mpc(ops, N, B, settings=on)
    s.mpc_set_operators(ops["Fx"], ops["Fu"], ops["Fr"], ops["Sbar"], ops["Ku"], ops["W0"])
    s.mpc_set_plant(plant["Ad"], plant["Bd"])
    with pytest.raises(sm.MpcqError) as e:
        s.mpc_run_device(Xd.data_ptr(), Ud.data_ptr(), 0.0, 2, 9, 0, 0, 1e-2, torch.cuda.current_stream().cuda_stream)
    assert e.value.code == sm._capi.MPCQ_ERR_ARG and "polish" in str(e.value)
    s.close()
    p = sm.BatchSolver(N, 2 * N, B, n_plants=B, settings=on)
    z = torch.zeros(B * 16, dtype=torch.float64, device="cuda")
    with pytest.raises(sm.MpcqError) as e:
        p.mpc_plants_step_device(4, 10, *[z.data_ptr()] * 7, Xd.data_ptr(), Ud.data_ptr())
    assert e.value.code == sm._capi.MPCQ_ERR_ARG and "polish" in str(e.value)
    with pytest.raises(sm.MpcqError) as e:
        p.mimo_step_device(Xd.data_ptr(), Ud.data_ptr())
    assert e.value.code == sm._capi.MPCQ_ERR_ARG and "polish" in str(e.value)
    p.close()
    assert np.array_equal(Ud.cpu().numpy(), U)  # (no refused call touched the caller's buffers)


@gpu
def test_polish_off_means_off(plant, kernel):
    N, B = 20, 4096 if kernel == "tile" else 512
    ops, X, U, q, u = _problem(plant, N, B, 1)
    a = _gpu_solve(ops, q, u, N)
    b = _gpu_solve(ops, q, u, N, settings=sm.default_settings(polish=0))
    ra, rb = _results(a), _results(b)
    a.close()
    b.close()
    assert np.all(rb["sp"] == 0) and np.all(rb["na"] == 0)
    assert np.all(np.isnan(rb["pri"])) and np.all(np.isnan(rb["dua"]))
    for k in ("x", "y", "st", "it", "rho"):
        assert np.array_equal(ra[k], rb[k]), k


@gpu
def test_verbose_reports_polish(plant, capfd):
    """settings.verbose with polish: the header says polish: on, the footer carries OSQP's solution-polish line
    for QP 0 and the batch line the count of polished QPs (all 64 here, as on the reference prefix)."""
    N, B = 20, 64
    ops, X, U, q, u = _problem(plant, N, B, 1)
    s = _gpu_solve(ops, q, u, N, settings=sm.default_settings(polish=1, verbose=1))
    sp = s.polish_info()[0]
    s.close()
    out = capfd.readouterr().out
    assert "warm start: on, polish: on" in out
    assert "solution polish:      successful" in out and sp[0] == 1
    assert f"{B} QPs, {B} solved, {int((sp == 1).sum())} polished" in out

"""CPU references of the MIMO active-set sensitivities (solvempc_amd/csrc/mpcq_mimo_sens.hip) and
the tests that pin them, and the fairness of the GPU tests' inputs, without any device code.

Per QP: ``oracle.condense_mimo`` gives the dense P, A and front-end operators; an ``oracle.Solver`` set up with
q0 = 0, l = LMIN, u0 = W0 takes the step's q and u (``update_gradient``, ``update_upper_bound``) and solves; its
``iterates()`` and ``scaling()`` feed tests/test_sensitivity_ref.py's ``_sens_ref`` (the device algorithm in numpy)
and ``_sens_exact`` (the unscaled, unregularised KKT system at the same active set).  The chain rule is applied in
numpy from the dense Fx, Fu, Fr, Sbar, Ku.

Families (``FAMILIES``; the GPU file runs the same ones): R, R-tight, Q, Q-tight, Q32, S, odd -- see ``_inputs``.
What is asserted here:
* every QP ends SOLVED, no bound pair (j, n + j) is active, and n_active covers the stated range (R-tight reaches
  n_active = n: a Schur complement as large as H);
* no QP's rule margin min |(u^ - z^) - y^| is below TIE = 1e-6 (the device's iterate follows the oracle's to about
  1e-7, tests/test_mimo.py), so the reference alone excludes no QP from the GPU comparison of active sets;
* TOL of a family = max(1e-9, 100 x the disagreement of _sens_ref and _sens_exact), tests/test_sensitivity_ref.py's
  rule, with its ceiling of 1e-7 on every family but Q-tight.  Disagreements as printed: R 6.5e-10, R-tight 8.1e-13,
  Q 6.0e-10, Q32 4.8e-10, S 1.2e-15, odd 5.7e-12, and Q-tight 2.55e-6 (up to 64 active rows at n = 120: the
  delta-regularised solve with three refinement steps is that far from the unregularised solution there), so
  Q-tight's TOL is 2.6e-4 by the same rule and its ceiling the next power of ten, 1e-3 (``CEILING``);
* the chain rule's signs against central finite differences of a tight-tolerance optimum in X, U and yref;
* the four new entry points are in the header, the ctypes mirror and the built library, and the new Python names
  exist (these fail without the feature)."""
import functools
import subprocess

import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import _capi, workload

from test_sensitivity_ref import LMIN, ROOT, _cotangents, _declared, _optimum_active, _rel, _rule, _sens_exact, _sens_ref, _tol

TIE = 1e-6
N_RHS = 3
NEW_SYMBOLS = ("mpcq_mimo_sensitivity_device", "mpcq_mimo_sensitivity", "mpcq_mimo_step_vjp_device",
               "mpcq_mimo_step_gains_device")
# family -> (n_active range asserted (lo_max, hi_min) or None, QPs the GPU test may exclude)
FAMILIES = {"R": ((0, 14), 2), "R-tight": ((5, 16), 2), "Q": ((0, 10), 1), "Q-tight": ((11, 64), 1), "Q32": ((0, 8), 0),
            "S": (None, 1), "odd": (None, 0)}


def _random_plants(rng, B, nx, nu):
    Ad = np.empty((B, nx, nx))
    for b in range(B):
        M = rng.normal(size=(nx, nx))
        Ad[b] = 0.9 * M / np.abs(np.linalg.eigvals(M)).max()
    return Ad, rng.normal(size=(B, nx, nu))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """dict(sh, Ad, Bd, X, U, N, s_rows, yref, seed) of a family."""
    if name in ("R", "R-tight"):  # tests/test_mimo.py's random plant: general K0, a state term in the bounds
        N, B, nx, nu, ny = 8, 40, 3, 2, 2
        rng = np.random.default_rng(11)
        Ad, Bd = _random_plants(rng, B, nx, nu)
        sh = {"Cd": rng.normal(size=(ny, nx)), "Q": np.diag([2.0, 0.5]), "R": np.diag([0.3, 0.1]),
              "RD": np.array([[1.0, 0.2], [0.2, 0.8]]), "K": 0.5 * rng.normal(size=(nu, nx)),
              "K0": np.array([[1.0, 0.3], [0.0, 0.8]]), "w0": np.array([0.8, 1.2])}
        X = rng.normal(size=(B, nx))
        U = 0.2 * rng.normal(size=(B, nu))
        if name == "R-tight":
            sh["w0"] = 0.1 * sh["w0"]
        return dict(sh=sh, Ad=Ad, Bd=Bd, X=X, U=U, N=N, s_rows=5, yref=np.array([0.3, -0.2]), seed=11)
    if name in ("Q", "Q-tight", "Q32"):  # the quad-rotor (config 4): n = 120 (no multiple of 16), n = 128 (capacity)
        N, B = (32, 8) if name == "Q32" else (30, 24)
        Ad, Bd = workload.quadrotor_plants(3, 0, B)
        X, U = workload.quadrotor_states(3, 0, B)
        sh = dict(workload.quadrotor_shared())
        if name == "Q-tight":
            sh["w0"] = 0.25 * np.asarray(sh["w0"], dtype=np.float64)
        return dict(sh=sh, Ad=Ad, Bd=Bd, X=X, U=U, N=N, s_rows=N, yref=None, seed=3)
    if name == "S":  # the SISO specialisation of tests/test_mimo.py: n_u = n_y = 1
        plant = workload.reference_plant()
        N, B = 20, 32
        rng = np.random.default_rng(5)
        Ad = plant["Ad"][None] * (1 + 0.02 * rng.normal(size=(B, 4, 4)))
        Bd = (plant["Bd"][None] * (1 + 0.02 * rng.normal(size=(B, 4))))[:, :, None]
        sh = {"Cd": plant["Cd"][None, :], "Q": [[plant["Q"]]], "R": [[plant["R"]]], "RD": [[plant["RD"]]],
              "K": plant["K"][None, :], "K0": [[plant["K"][0]]], "w0": [255.0]}
        X, U = workload.mpc_states(3, 0, B)
        return dict(sh=sh, Ad=Ad, Bd=Bd, X=X, U=U[:, None], N=N, s_rows=10, yref=None, seed=5)
    if name == "odd":  # n = 30 with n_u = 2: padding of P^'s rows
        N, B, nx, nu, ny = 15, 16, 3, 2, 2
        rng = np.random.default_rng(13)
        Ad, Bd = _random_plants(rng, B, nx, nu)
        sh = {"Cd": rng.normal(size=(ny, nx)), "Q": np.diag([2.0, 0.5]), "R": np.diag([0.3, 0.1]),
              "RD": np.array([[1.0, 0.2], [0.2, 0.8]]), "K": 0.5 * rng.normal(size=(nu, nx)),
              "K0": np.array([[1.0, 0.3], [0.0, 0.8]]), "w0": np.array([0.8, 1.2])}
        return dict(sh=sh, Ad=Ad, Bd=Bd, X=rng.normal(size=(B, nx)), U=0.2 * rng.normal(size=(B, nu)), N=N, s_rows=7,
                    yref=np.array([0.3, -0.2]), seed=13)
    raise KeyError(name)


# A family whose own reference disagreement puts the rule's TOL above tests/test_sensitivity_ref.py's ceiling of 1e-7
# keeps the rule; its ceiling is the next power of ten above the rule's value (printed by test_family_references).
CEILING = {"Q-tight": 1e-3}


def _family_tol(name, err):
    """TOL = max(1e-9, 100 x disagreement), _tol's rule; _tol's ceiling unless the family has its own."""
    if name not in CEILING:
        return _tol(err)
    tol = max(1e-9, 100.0 * float(err))
    assert tol < CEILING[name], tol
    return tol


def _frs(ops, ny):
    """Frs = Fr (1_N (x) I_ny): the gradient's operator on yref."""
    n = ops["Fr"].shape[0]
    return ops["Fr"].reshape(n, -1, ny).sum(axis=1)


def _chain(ops, ny, gq, gu):
    """(dX, dU, dyref) from dense operators: q = Fx X + Fu U + Frs yref, u = W0 + Sbar X + Ku U."""
    return ops["Fx"].T @ gq + ops["Sbar"].T @ gu, ops["Fu"].T @ gq + ops["Ku"].T @ gu, _frs(ops, ny).T @ gq


@functools.lru_cache(maxsize=None)
def _refs(name):
    """The oracle side of a family, once per session: per QP the dense operators, status, iterations, the rule's
    active set and margin on the oracle's iterate, and for the cotangents g (B, N_RHS, n) and e_r (r < n_u) the
    gradients of _sens_ref and _sens_exact; TOL from their disagreement."""
    f = _inputs(name)
    B, nx, nu = f["Bd"].shape
    ny = np.asarray(f["sh"]["Cd"]).shape[0]
    N = f["N"]
    n, m = N * nu, 2 * N * nu
    g = _cotangents(f["seed"], B, N_RHS * n).reshape(B, N_RHS, n)
    eye = np.eye(n)
    l = np.full(m, LMIN)
    out = dict(ops=[], st=[], it=[], upp=[], margin=[], n_active=[], q=[], u=[], ref=[], exact=[], ref0=[], exact0=[])
    for b in range(B):
        ops = oracle.condense_mimo(dict(f["sh"], Ad=f["Ad"][b], Bd=f["Bd"][b]), N, f["s_rows"])
        s = oracle.Solver(ops["P"], np.zeros(n), ops["A"], l, ops["W0"])
        D, E, c = s.scaling()
        q = oracle.mimo_gradient(ops, f["X"][b], f["U"][b], f["yref"])
        u = oracle.mimo_upper_bound(ops, f["X"][b], f["U"][b])
        assert s.update_gradient(q) and s.update_upper_bound(u)
        out["st"].append(s.solve())
        out["it"].append(s.info().iter)
        _, z, y = s.iterates()
        per = dict(ref=[], exact=[], ref0=[], exact0=[])
        for key, gs in (("", g[b]), ("0", eye[:nu])):
            for gv in gs:
                r = _sens_ref(ops["P"], ops["A"], l, u, D, E, c, z, y, gv)
                assert not r["low"].any()
                ex = _sens_exact(ops["P"], ops["A"], r["low"], r["upp"], gv)
                per["ref" + key].append(np.r_[r["gq"], r["gu"]])
                per["exact" + key].append(np.r_[ex[0], ex[2]])
        for k, v in per.items():
            out[k].append(np.asarray(v))
        out["ops"].append(ops)
        out["upp"].append(r["upp"])
        out["margin"].append(r["margin"])
        out["n_active"].append(r["n_active"])
        out["q"].append(q)
        out["u"].append(u)
    ops_list = out.pop("ops")
    out = {k: np.asarray(v) for k, v in out.items()}
    err = max(float(_rel(out["ref"], out["exact"]).max()), float(_rel(out["ref0"], out["exact0"]).max()))
    out.update(ops=ops_list, g=g, err=err, tol=_family_tol(name, err), dims=(B, N, nx, nu, ny, n, m), inputs=f)
    return out


# ----------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_family_references(name):
    r = _refs(name)
    B, N, nx, nu, ny, n, m = r["dims"]
    na, upp = r["n_active"], r["upp"]
    pairs = int((upp[:, :n] & upp[:, n:]).any(axis=1).sum())
    print(f"{name}: B {B}, n {n}; n_active {na.min()}..{na.max()} ({int((na == n).sum())} QPs at n), smallest rule margin "
          f"{r['margin'].min():.2e}, ref-vs-exact {r['err']:.2e}, TOL {r['tol']:.1e}, bound pairs active in {pairs} QPs")
    assert np.all(r["st"] == oracle.SOLVED)
    assert pairs == 0 and na.max() <= n
    assert r["margin"].min() >= TIE, r["margin"].min()
    rng_ = FAMILIES[name][0]
    if rng_ is not None:
        assert na.min() <= rng_[0] and na.max() >= rng_[1], (na.min(), na.max())
    if name == "R-tight":
        assert (na == n).sum() >= 1
    assert r["tol"] < CEILING.get(name, 1e-7)
    assert FAMILIES[name][1] <= 0.05 * B  # the GPU file's exclusion cap


def test_chain_rule_signs_match_finite_differences():
    """dX, dU, dyref of _chain on _sens_exact at the optimum's active set against central differences of g . x* with
    x* = _optimum(q(X, U, yref), u(X, U)), on QPs of family R with 0, some and many active rows whose active set
    the step leaves alone (asserted).  x* is affine on such a piece, so the quotient is exact up to rounding: the
    bound is tests/test_sensitivity_ref.py's 1e-7 relative to max(1, |reference|)."""
    r = _refs("R")
    f = r["inputs"]
    B, N, nx, nu, ny, n, m = r["dims"]
    l = np.full(m, LMIN)
    h = 1e-4
    seen = set()
    for b in range(B):
        ops = r["ops"][b]
        X, U, yref = f["X"][b], f["U"][b], f["yref"]

        def xstar(X, U, yref):
            return _optimum_active(ops["P"], ops["A"], oracle.mimo_gradient(ops, X, U, yref), l,
                                   oracle.mimo_upper_bound(ops, X, U))

        x0, low, upp = xstar(X, U, yref)
        k = int(upp.sum())
        if k in seen or len(seen) >= 4:
            continue
        gv = r["g"][b, 0]
        gq, _, gu = _sens_exact(ops["P"], ops["A"], low, upp, gv)
        dX, dU, dy = _chain(ops, ny, gq, gu)
        stable, err = True, 0.0
        scale = max(1.0, float(np.abs(np.r_[dX, dU, dy]).max()))
        for which, size, ref_ in (("X", nx, dX), ("U", nu, dU), ("y", ny, dy)):
            for j in range(size):
                xs = []
                for sgn in (1.0, -1.0):
                    d = sgn * h * np.eye(size)[j]
                    x, lo, up = xstar(X + d if which == "X" else X, U + d if which == "U" else U,
                                      yref + d if which == "y" else yref)
                    stable &= bool(np.array_equal(lo, low) and np.array_equal(up, upp))
                    xs.append(x)
                err = max(err, abs(gv @ (xs[0] - xs[1]) / (2 * h) - ref_[j]))
        if not stable:
            continue
        seen.add(k)
        print(f"R QP {b}: {k} active rows, chain-rule FD error {err / scale:.2e}")
        assert err / scale <= 1e-7, (b, err / scale)
    assert len(seen) >= 3 and max(seen) >= 2, seen


def test_mimo_sensitivity_entry_points_in_header_mirror_and_library():
    declared = _declared()
    lib = sm.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sm.library_path())], check=True, capture_output=True,
                        text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.EXPORTS, name
        assert name in exported, name
        f = getattr(lib, name)
        assert f.restype is not None and f.argtypes, name
    assert len(lib.mpcq_mimo_sensitivity_device.argtypes) == 7 and len(lib.mpcq_mimo_sensitivity.argtypes) == 6
    assert len(lib.mpcq_mimo_step_vjp_device.argtypes) == 8 and len(lib.mpcq_mimo_step_gains_device.argtypes) == 6
    hdr = (ROOT / "include" / "mpcq.h").read_text()
    assert "DESIGN.md 4.15" in hdr


def test_python_names_exist():
    for name in ("mimo_sensitivity", "mimo_sensitivity_device", "mimo_step_gains", "mimo_step_gains_device",
                 "mimo_step_vjp_device"):
        assert callable(getattr(sm.BatchSolver, name)), name
    from solvempc_amd import diff
    assert callable(diff.mimo_solution)

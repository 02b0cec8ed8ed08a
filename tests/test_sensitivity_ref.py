"""CPU references of the active-set sensitivities (solvempc_amd/csrc/mpcq_sens.hip) and the tests
that pin them without any device code.

* ``_sens_ref`` restates the device algorithm in numpy on a scaled final iterate (the oracle's, ``ora_get_iterates``
  and ``ora_get_scaling``): polish's active-set rule (lower-active when z - l < -y, otherwise upper-active when
  u - z < y; lower rows first), the delta-regularised reduced KKT system with the scaled cotangent c D g as its
  right-hand side by a plain ``np.linalg.solve``, ``refine`` steps of refinement against the unregularised matrix,
  and the way back, gq = -D v^, w = E_a w^ / c.  It also reports tests/test_polish.py's decision margin.
* ``_sens_exact`` needs neither the scaling nor delta: the unscaled K = [P, A_a'; A_a, 0] at a given active set,
  solved by least squares (duplicated active rows are fine: v is unique, w the minimum-norm one, which is also
  what the regularised solve tends to).  ``_optimum_active`` supplies the active set of tests/test_polish.py's
  ``_optimum`` (from the duals of a 1e-10 oracle solve).

The tests here check ``_sens_exact`` against central finite differences of ``_optimum``'s x* under perturbations of
q, u (and l where finite) that leave the active set alone, which they assert.  x* is affine in (q, l, u) on such a
piece, so the difference quotient is exact up to rounding: _optimum's KKT solve is good to ~kappa(K) eps ~ 1e-12,
divided by the step 2h = 2e-4 that is ~1e-8 at worst; the bound is 1e-7 relative to max(1, |reference|).  That pins
the sign conventions (gq = -v, gl / gu = +w) independently of the device.  They also yield the GPU tests' TOL
(``_tol``) and the seeds' share of QPs near an active-set tie."""
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import _capi, workload

import test_polish as tp

ROOT = Path(__file__).resolve().parents[1]
LMIN = tp.LMIN
PREFIX = tp.PREFIX
TIE = 1e-8        # a QP whose active-set decision margin is below this is excluded from reference comparisons
MAX_TIES = 0.02   # at most this share of a prefix may be excluded
NEW_SYMBOLS = ("mpcq_sensitivity_device", "mpcq_sensitivity", "mpcq_mpc_step_gains_device", "mpcq_mpc_step_gains")


# ----------------------------------------------------------------------------- references
def _rule(lh, uh, z, y):
    """polish's active-set rule on a scaled iterate: (low, upp, margin)."""
    low = z - lh < -y
    upp = ~low & (uh - z < y)
    with np.errstate(invalid="ignore"):
        margin = float(np.minimum(np.abs(z - lh + y), np.abs(uh - z - y)).min(initial=np.inf))
    return low, upp, margin


def _sens_ref(P, A, l, u, D, E, c, z, y, g, delta=1e-6, refine=3):
    """The device algorithm on the scaled iterate (z, y): dict(gq, gl, gu, n_active, margin, low, upp)."""
    n, m = len(D), len(E)
    Ph = c * D[:, None] * tp._sym(P) * D[None, :]
    Ah = E[:, None] * np.asarray(A, dtype=np.float64).reshape(m, n) * D[None, :]
    with np.errstate(over="ignore"):
        lh, uh = E * l, E * u
    low, upp, margin = _rule(lh, uh, z, y)
    rows = np.r_[np.flatnonzero(low), np.flatnonzero(upp)]
    Ared = Ah[rows]
    mr = len(rows)
    K = np.block([[Ph, Ared.T], [Ared, np.zeros((mr, mr))]])
    Kreg = K + np.diag(np.r_[np.full(n, delta), np.full(mr, -delta)])
    b = np.r_[c * D * g, np.zeros(mr)]
    s = np.linalg.solve(Kreg, b)
    for _ in range(refine):
        s = s + np.linalg.solve(Kreg, b - K @ s)
    w = E[rows] * s[n:] / c
    gl, gu = np.zeros(m), np.zeros(m)
    nl = int(low.sum())
    gl[rows[:nl]] = w[:nl]
    gu[rows[nl:]] = w[nl:]
    return dict(gq=-(D * s[:n]), gl=gl, gu=gu, n_active=mr, margin=margin, low=low, upp=upp)


def _sens_exact(P, A, low, upp, g):
    """(gq, gl, gu) from the unregularised, unscaled KKT system at the active set (low, upp), by least squares."""
    n = len(g)
    A = np.asarray(A, dtype=np.float64).reshape(-1, n)
    rows = np.r_[np.flatnonzero(low), np.flatnonzero(upp)]
    Aa = A[rows]
    k = len(rows)
    K = np.block([[tp._sym(P), Aa.T], [Aa, np.zeros((k, k))]])
    s = np.linalg.lstsq(K, np.r_[g, np.zeros(k)], rcond=None)[0]
    gl, gu = np.zeros(A.shape[0]), np.zeros(A.shape[0])
    nl = int(np.sum(low))
    gl[rows[:nl]] = s[n:][:nl]
    gu[rows[nl:]] = s[n:][nl:]
    return -s[:n], gl, gu


def _optimum_active(P, A, q, l, u, solver=None):
    """(x*, low, upp): tests/test_polish.py's _optimum and the active set its duals show."""
    x, y = tp._optimum(P, A, q, l, u, solver)
    return x, y < 0, y > 0


def _stack(gq, gl, gu):
    return np.concatenate([gq, gl, gu], axis=-1)


def _rel(a, ref):
    """max |a - ref| relative to max(1, |ref|_inf), per QP (last axis)."""
    return np.abs(a - ref).max(axis=-1, initial=0.0) / np.maximum(1.0, np.abs(ref).max(axis=-1, initial=0.0))


def _tol(err):
    """TOL of a family from the references alone: max(1e-9, 100 x the largest error of _sens_ref against
    _sens_exact on the same inputs and active set); the x100 covers the device's elimination order (Cholesky of H
    and of the Schur complement instead of numpy's LU of the whole matrix), as in tests/test_polish.py."""
    tol = max(1e-9, 100.0 * float(np.max(err, initial=0.0)))
    assert tol < 1e-7, tol
    return tol


def _cotangents(seed, B, n):
    return np.random.default_rng(1000 + seed).normal(size=(B, n))


# ----------------------------------------------------------------------------- the MPC family
@functools.lru_cache(maxsize=None)
def _mpc_sens_refs(N, seed, count=PREFIX):
    """_sens_ref for random cotangents (g) and for e_0 on the first `count` QPs of tp._problem(plant, N, ., seed),
    from the oracle's final iterates; _sens_exact at the same active set; TOL; the ties.  Once per session."""
    plant = workload.reference_plant()
    ops, X, U, q, u = tp._problem(plant, N, count, seed)
    l = np.full(2 * N, LMIN)
    u0 = oracle.upper_bound(ops, np.zeros(4), 0.0)
    g = _cotangents(seed, count, N)
    e0 = np.eye(N)[0]
    out = dict(st=[], it=[], ref=[], ref0=[], exact=[], exact0=[], n_active=[], margin=[], low=[], upp=[])
    for b in range(count):
        s = oracle.Solver(ops["P"], np.zeros(N), ops["A"], l, u0)
        D, E, c = s.scaling()
        s.update_gradient(q[b])
        s.update_upper_bound(u[b])
        out["st"].append(s.solve())
        out["it"].append(s.info().iter)
        _, z, y = s.iterates()
        r = _sens_ref(ops["P"], ops["A"], l, u[b], D, E, c, z, y, g[b])
        r0 = _sens_ref(ops["P"], ops["A"], l, u[b], D, E, c, z, y, e0)
        out["ref"].append(_stack(r["gq"], r["gl"], r["gu"]))
        out["ref0"].append(_stack(r0["gq"], r0["gl"], r0["gu"]))
        out["exact"].append(_stack(*_sens_exact(ops["P"], ops["A"], r["low"], r["upp"], g[b])))
        out["exact0"].append(_stack(*_sens_exact(ops["P"], ops["A"], r["low"], r["upp"], e0)))
        for k in ("n_active", "margin", "low", "upp"):
            out[k].append(r[k])
    out = {k: np.asarray(v) for k, v in out.items()}
    out["tol"] = _tol(np.maximum(_rel(out["ref"], out["exact"]), _rel(out["ref0"], out["exact0"])))
    out["clear"] = out["margin"] >= TIE
    out.update(ops=ops, X=X, U=U, q=q, u=u, l=l, g=g, D=D, E=E, c=c)
    return out


# seeds of the GPU tests' MPC families: (N, seed) -> chosen here so that the share of the prefix within TIE of an
# active-set flip stays under MAX_TIES (test_mpc_family_references prints and asserts it)
MPC_SEEDS = {20: 1, 15: 3, 32: 5}


# ----------------------------------------------------------------------------- the generic family
GEN_N, GEN_M, GEN_B = 7, 11, 64


def _generic_inputs():
    """Seeded per-plant QPs, n 7, m 11: rows 0-1 equalities, rows 2-3 without a lower bound, rows 4-5 free on both
    sides, rows 6-10 two-sided.  QP 0 has wide bounds on every row (no active row)."""
    rng = np.random.default_rng(21)
    n, m, B = GEN_N, GEN_M, GEN_B
    P, A, q, l, u = [], [], [], [], []
    for b in range(B):
        M = rng.normal(size=(n, n))
        P.append(M @ M.T + 0.1 * np.eye(n))
        A.append(rng.normal(size=(m, n)))
        q.append(rng.normal(size=n))
        lo, up = -rng.uniform(0.2, 1.0, size=m), rng.uniform(0.2, 1.0, size=m)
        lo[:2] = up[:2] = 0.1 * rng.normal(size=2)
        lo[2:4] = LMIN
        lo[4:6], up[4:6] = LMIN, -LMIN
        if b == 0:
            lo[:], up[:] = -100.0, 100.0
        l.append(lo)
        u.append(up)
    return tuple(np.stack(v) for v in (P, A, q, l, u))


@functools.lru_cache(maxsize=None)
def _generic_sens_refs():
    P, A, q, l, u = _generic_inputs()
    B, n = q.shape
    g = _cotangents(21, B, n)
    e0 = np.eye(n)[0]
    out = dict(st=[], it=[], ref=[], ref0=[], exact=[], exact0=[], n_active=[], margin=[])
    for b in range(B):
        s = oracle.Solver(P[b], q[b], A[b], l[b], u[b])
        out["st"].append(s.solve())
        out["it"].append(s.info().iter)
        _, z, y = s.iterates()
        r = _sens_ref(P[b], A[b], l[b], u[b], *s.scaling(), z, y, g[b])
        r0 = _sens_ref(P[b], A[b], l[b], u[b], *s.scaling(), z, y, e0)
        out["ref"].append(_stack(r["gq"], r["gl"], r["gu"]))
        out["ref0"].append(_stack(r0["gq"], r0["gl"], r0["gu"]))
        out["exact"].append(_stack(*_sens_exact(P[b], A[b], r["low"], r["upp"], g[b])))
        out["exact0"].append(_stack(*_sens_exact(P[b], A[b], r["low"], r["upp"], e0)))
        out["n_active"].append(r["n_active"])
        out["margin"].append(r["margin"])
    out = {k: np.asarray(v) for k, v in out.items()}
    solved = out["st"] == oracle.SOLVED
    out["tol"] = _tol(np.maximum(_rel(out["ref"], out["exact"]), _rel(out["ref0"], out["exact0"]))[solved])
    out["clear"] = (out["margin"] >= TIE) & solved
    out["g"] = g
    return out


# ----------------------------------------------------------------------------- finite differences
def _fd_check(P, A, q, l, u, g, h=1e-4):
    """_sens_exact at _optimum's active set against central differences of _optimum's x* in every entry of q, every
    finite u and l (an equality row's l and u move together and are compared with gl + gu).  Asserts that no
    perturbation changes the active set.  Returns the largest error relative to max(1, |reference|_inf)."""
    n, m = len(q), len(l)
    x0, low, upp = _optimum_active(P, A, q, l, u)
    gq, gl, gu = _sens_exact(P, A, low, upp, g)

    def moved(dq=None, dl=None, du=None):
        xs = []
        for sgn in (1.0, -1.0):
            qq = q + sgn * dq if dq is not None else q
            ll = l + sgn * dl if dl is not None else l
            uu = u + sgn * du if du is not None else u
            x, lo, up = _optimum_active(P, A, qq, ll, uu)
            assert np.array_equal(lo, low) and np.array_equal(up, upp), "the perturbation changed the active set"
            xs.append(x)
        return g @ (xs[0] - xs[1]) / (2 * h)

    scale = max(1.0, float(np.abs(_stack(gq, gl, gu)).max()))
    err = 0.0
    for j in range(n):
        err = max(err, abs(moved(dq=h * np.eye(n)[j]) - gq[j]))
    for i in range(m):
        e = h * np.eye(m)[i]
        if l[i] == u[i]:
            err = max(err, abs(moved(dl=e, du=e) - (gl[i] + gu[i])))
            continue
        if u[i] < 1e20:
            err = max(err, abs(moved(du=e) - gu[i]))
        if l[i] > -1e20:
            err = max(err, abs(moved(dl=e) - gl[i]))
    return err / scale, int(low.sum() + upp.sum())


# ----------------------------------------------------------------------------- CPU tests
def test_sens_exact_matches_finite_differences_mpc(plant):
    """The MPC QP at N = 20 (tp._problem, seed 1): QPs with 0, 1 and several active rows."""
    N = 20
    ops, X, U, q, u = tp._problem(plant, N, 64, 1)
    l = np.full(2 * N, LMIN)
    g = _cotangents(1, 64, N)
    seen = set()
    for b in range(64):
        x, low, upp = _optimum_active(ops["P"], ops["A"], q[b], l, u[b])
        k = int(upp.sum())
        if k in seen or len(seen) >= 4:
            continue
        seen.add(k)
        for gv in (g[b], np.eye(N)[0]):
            err, na = _fd_check(ops["P"], ops["A"], q[b], l, u[b], gv)
            print(f"MPC QP {b}: {na} active rows, FD error {err:.2e}")
            assert err <= 1e-7, (b, err)
    assert 0 in seen and max(seen) >= 2, seen


def test_sens_exact_matches_finite_differences_generic():
    """Generic QPs with equality, one-sided, free and two-sided rows, lower- and upper-active rows among them."""
    P, A, q, l, u = _generic_inputs()
    g = _cotangents(21, len(q), GEN_N)
    lows = upps = 0
    for b in (0, 1, 2, 3, 4, 5):
        x, low, upp = _optimum_active(P[b], A[b], q[b], l[b], u[b])
        lows += int(low[2:].sum())
        upps += int(upp[2:].sum())
        err, na = _fd_check(P[b], A[b], q[b], l[b], u[b], g[b])
        print(f"generic QP {b}: {na} active rows, FD error {err:.2e}")
        assert err <= 1e-7, (b, err)
        assert (na == 0) == (b == 0)
    assert lows >= 1 and upps >= 1, (lows, upps)


@pytest.mark.parametrize("N", sorted(MPC_SEEDS))
def test_mpc_family_references(N):
    """_sens_ref against _sens_exact on the GPU tests' MPC inputs (TOL < 1e-7), the share of the prefix within TIE
    of an active-set flip (<= 2 %), and that the rule's active set on the oracle's iterate is the optimum's on all
    but a few QPs (so "exact" is the sensitivity of the optimum there; checked on the first 64 QPs)."""
    seed = MPC_SEEDS[N]
    r = _mpc_sens_refs(N, seed)
    assert np.all(r["st"] == oracle.SOLVED)
    ties = float((~r["clear"]).mean())
    err = float(np.maximum(_rel(r["ref"], r["exact"]), _rel(r["ref0"], r["exact0"])).max())
    same = 0
    for b in range(64):
        _, low, upp = _optimum_active(r["ops"]["P"], r["ops"]["A"], r["q"][b], r["l"], r["u"][b])
        same += bool(np.array_equal(low, r["low"][b]) and np.array_equal(upp, r["upp"][b]))
    print(f"N={N} seed={seed}: ref-vs-exact {err:.2e}, TOL {r['tol']:.1e}, ties {ties:.4f}, n_active "
          f"{r['n_active'].min()}..{r['n_active'].max()}, rule == optimum's set on {same} of 64")
    assert r["tol"] < 1e-7 and ties <= MAX_TIES
    assert same >= 60
    assert r["n_active"].min() == 0 and r["n_active"].max() >= 2


def test_generic_family_references():
    r = _generic_sens_refs()
    solved = r["st"] == oracle.SOLVED
    ties = float((~r["clear"] & solved).mean())
    print(f"generic: {int(solved.sum())} of {len(solved)} solved, TOL {r['tol']:.1e}, ties {ties:.4f}, n_active "
          f"{r['n_active'].min()}..{r['n_active'].max()}")
    assert r["tol"] < 1e-7 and ties <= MAX_TIES and solved.sum() >= 0.9 * len(solved)
    assert r["n_active"][0] == 0 and r["n_active"].max() >= 4


# ----------------------------------------------------------------------------- ABI
def _declared():
    hdr = (ROOT / "include" / "mpcq.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return set(re.findall(r"\b(mpcq_[a-z_0-9]+)\s*\(", hdr))


def test_sensitivity_entry_points_in_header_mirror_and_library():
    """include/mpcq.h, _capi.py and the built library's dynamic symbol table agree on the four new entry points."""
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
    assert len(lib.mpcq_sensitivity_device.argtypes) == 7 and len(lib.mpcq_sensitivity.argtypes) == 6
    assert len(lib.mpcq_mpc_step_gains_device.argtypes) == 6 and len(lib.mpcq_mpc_step_gains.argtypes) == 5


def test_solve_counter_and_methods_exist():
    for name in ("sensitivity", "sensitivity_device", "mpc_step_gains", "mpc_step_gains_device"):
        assert callable(getattr(sm.BatchSolver, name))
    from solvempc_amd import diff
    assert callable(diff.mpc_solution)

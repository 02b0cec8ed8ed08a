"""CPU reference of the gradients with respect to the QP's matrices (mpcq_sensitivity_data*,
solvempc_amd/csrc/mpcq_sensdata.hip) and the tests that pin it without any device code.

``_data_exact`` applies the contract to the references the project already has: with (gq, gl, gu) from
``test_sensitivity_ref._sens_exact`` at the optimum's active set, x*, y* from ``test_polish._optimum`` (y* is zero
off the active set) and w = gl + gu,

    gP = 1/2 (gq x*' + x* gq')        gA = y* gq' - w x*'

The finite-difference tests compare it with central differences of g . x* in every upper-triangle entry of P
(``_sym`` mirrors that triangle, as mpcq_setup reads it: entry (i, j), i < j, is compared with gP_ij + gP_ji, a
diagonal entry with gP_ii) and in every entry of A, at h = 1e-5, and assert that no perturbation moves the active
set.  The bound is that of tests/test_sensitivity_ref.py's finite-difference tests, 1e-7 relative to
max(1, |reference|_inf).  x* is not affine in P or A, so the quotient carries a truncation error ~h^2: where a QP's
error exceeds the bound the step is halved, the error must fall by about 4x (between 2.5x and 6x: it is truncation,
not a wrong formula), and the halved step must meet the same bound.

``_directional_fd`` is the reference's share of tests/test_sensitivity_data.py's directional check of
``diff.qp_solution``: the same difference quotient along a random (symmetric dP, dA), done with ``_optimum``."""
import functools
import subprocess

import numpy as np

import oracle
import solvempc_amd as sm
from solvempc_amd import _capi

import test_polish as tp
import test_sensitivity_ref as ref

LMIN = tp.LMIN
H = 1e-5
FD_BOUND = 1e-7
NEW_SYMBOLS = ("mpcq_sensitivity_data_device", "mpcq_sensitivity_data")


# ----------------------------------------------------------------------------- the reference
def _formula(gq, w, x, ya):
    """(gP, gA) of one QP from gq, w = gl + gu, the solution x and the dual on the active rows ya."""
    return 0.5 * (np.outer(gq, x) + np.outer(x, gq)), np.outer(ya, gq) - np.outer(w, x)


def _data_exact(P, A, q, l, u, g):
    """dict(gP, gA, gq, gl, gu, x, y, low, upp) at _optimum's x*, y* and active set."""
    x, y = tp._optimum(P, A, q, l, u)
    low, upp = y < 0, y > 0
    gq, gl, gu = ref._sens_exact(P, A, low, upp, g)
    gP, gA = _formula(gq, gl + gu, x, np.where(low | upp, y, 0.0))
    return dict(gP=gP, gA=gA, gq=gq, gl=gl, gu=gu, x=x, y=y, low=low, upp=upp)


def _upper(gP):
    """The gradient with respect to the upper triangle that _sym / mpcq_setup read: gP_ij + gP_ji above the diagonal."""
    return np.triu(gP) + np.triu(gP.T, 1)


def _formula_batch(gq, w, x, ya):
    """_formula on a batch (leading axis)."""
    gP = 0.5 * (gq[:, :, None] * x[:, None, :] + x[:, :, None] * gq[:, None, :])
    return gP, ya[:, :, None] * gq[:, None, :] - w[:, :, None] * x[:, None, :]


@functools.lru_cache(maxsize=None)
def _mpc_oracle_xy(N, seed, count=tp.PREFIX):
    """The oracle's own final (x, y) on the QPs of test_sensitivity_ref._mpc_sens_refs(N, seed)."""
    r = ref._mpc_sens_refs(N, seed, count)
    ops = r["ops"]
    u0 = oracle.upper_bound(ops, np.zeros(4), 0.0)
    xs, ys = [], []
    for b in range(count):
        s = oracle.Solver(ops["P"], np.zeros(N), ops["A"], r["l"], u0)  # (as _mpc_sens_refs: a fresh solver per QP)
        s.update_gradient(r["q"][b])
        s.update_upper_bound(r["u"][b])
        assert s.solve() == r["st"][b] and s.info().iter == r["it"][b]
        xs.append(s.x())
        ys.append(s.y())
    return np.asarray(xs), np.asarray(ys)


@functools.lru_cache(maxsize=None)
def _generic_oracle_xy():
    P, A, q, l, u = ref._generic_inputs()
    xs, ys = [], []
    for b in range(len(q)):
        s = oracle.Solver(P[b], q[b], A[b], l[b], u[b])
        s.solve()
        xs.append(s.x())
        ys.append(s.y())
    return np.asarray(xs), np.asarray(ys)


# ----------------------------------------------------------------------------- finite differences
def _fd_data(P, A, q, l, u, g, h):
    """Largest error of _data_exact against central differences of g . x* over every upper-triangle entry of P and
    every entry of A, relative to max(1, |reference|_inf); asserts that the active set does not move."""
    P, A = tp._sym(P), np.asarray(A, dtype=np.float64).reshape(len(l), len(q))
    e = _data_exact(P, A, q, l, u, g)
    n, m = len(q), len(l)

    def value(Pm, Am):
        x, low, upp = ref._optimum_active(Pm, Am, q, l, u)
        assert np.array_equal(low, e["low"]) and np.array_equal(upp, e["upp"]), "the perturbation changed the active set"
        return g @ x

    def quotient(M, i, j, which):
        vals = []
        for sgn in (1.0, -1.0):
            Mm = M.copy()
            Mm[i, j] += sgn * h
            vals.append(value(Mm, A) if which == "P" else value(P, Mm))
        return (vals[0] - vals[1]) / (2 * h)

    gPu = _upper(e["gP"])
    scale = max(1.0, float(np.abs(gPu).max()), float(np.abs(e["gA"]).max(initial=0.0)))
    err = 0.0
    for i in range(n):
        for j in range(i, n):
            err = max(err, abs(quotient(P, i, j, "P") - gPu[i, j]))
    for r in range(m):
        for j in range(n):
            err = max(err, abs(quotient(A, r, j, "A") - e["gA"][r, j]))
    return err / scale, int(e["low"].sum() + e["upp"].sum())


def _fd_within_bound(name, *qp):
    """The check of the module docstring on one QP; returns its number of active rows."""
    err, na = _fd_data(*qp, H)
    print(f"{name}: {na} active rows, FD error {err:.2e} at h = {H:g}")
    if err > FD_BOUND:
        err2, _ = _fd_data(*qp, H / 2)
        print(f"{name}: FD error {err2:.2e} at h = {H / 2:g} (x{err / err2:.2f} smaller)")
        assert 2.5 <= err / err2 <= 6.0, (name, err, err2)
        err = err2
    assert err <= FD_BOUND, (name, err)
    return na


def test_data_exact_matches_finite_differences_generic():
    """Generic QPs 0-5 of test_sensitivity_ref._generic_inputs (n 7, m 11: equality, one-sided, free and two-sided
    rows; QP 0 has no active row)."""
    P, A, q, l, u = ref._generic_inputs()
    g = ref._cotangents(21, len(q), ref.GEN_N)
    for b in range(6):
        na = _fd_within_bound(f"generic QP {b}", P[b], A[b], q[b], l[b], u[b], g[b])
        assert (na == 0) == (b == 0)


def test_data_exact_matches_finite_differences_mpc(plant):
    """The MPC QP at N = 20 (tp._problem, seed 1) with no, one and several active rows.  The family's states have
    either no active row (QP 3) or ten and more (QP 0: 11, QP 4: 10) -- the input constraint's rows saturate
    together -- so the one-row QP is the state 0.279 (X, U)_3 + 0.721 (X, U)_4, in the middle of the short
    stretch between the two (0.72003 .. 0.72209) where exactly one row is active."""
    N = 20
    ops, X, U, q, u = tp._problem(plant, N, 8, 1)
    l = np.full(2 * N, LMIN)
    g = ref._cotangents(1, 8, N)
    Xm, Um = 0.279 * X[3] + 0.721 * X[4], 0.279 * U[3] + 0.721 * U[4]
    cases = {"none": (q[3], u[3], g[3]), "several": (q[0], u[0], g[0]),
             "one": (oracle.gradient(ops, Xm[None], np.array([Um]))[0],
                     oracle.upper_bound(ops, Xm[None], np.array([Um]))[0], g[1])}
    for kind, (qb, ub, gb) in cases.items():
        na = _fd_within_bound(f"MPC QP ({kind})", ops["P"], ops["A"], qb, l, ub, gb)
        assert {"none": na == 0, "one": na == 1, "several": na >= 2}[kind], (kind, na)


def test_upper_triangle_rule():
    """gP is symmetric; the upper-triangle parametrisation doubles the off-diagonal entries."""
    P, A, q, l, u = ref._generic_inputs()
    e = _data_exact(P[1], A[1], q[1], l[1], u[1], ref._cotangents(21, len(q), ref.GEN_N)[1])
    assert np.array_equal(e["gP"], e["gP"].T)
    up = _upper(e["gP"])
    assert np.array_equal(np.diag(up), np.diag(e["gP"])) and np.array_equal(np.triu(up, 1), 2 * np.triu(e["gP"], 1))
    assert np.all(e["gA"][~(e["low"] | e["upp"])] == 0)


# ----------------------------------------------------------------------------- the directional check's reference
def _directions(seed=77):
    """One random symmetric dP and one random dA per QP of the generic family."""
    rng = np.random.default_rng(seed)
    dP = rng.normal(size=(ref.GEN_B, ref.GEN_N, ref.GEN_N))
    return 0.5 * (dP + dP.transpose(0, 2, 1)), rng.normal(size=(ref.GEN_B, ref.GEN_M, ref.GEN_N))


@functools.lru_cache(maxsize=None)
def _directional_fd():
    """On the clear QPs of the generic family: the derivative of g . x* along (dP, dA) by the formula,
    <gP, dP> + <gA, dA> with _data_exact, and by central differences of _optimum at h = 1e-5.  Returns
    dict(exact, fd, keep, err): per-QP values, the QPs compared (clear, and the active set the same at both ends of
    the difference) and the largest |fd - exact| / max(1, |exact|) over them -- the reference's own error."""
    P, A, q, l, u = ref._generic_inputs()
    r = ref._generic_sens_refs()
    dP, dA = _directions()
    B = len(q)
    exact, fd, keep = np.zeros(B), np.zeros(B), r["clear"].copy()
    for b in np.flatnonzero(r["clear"]):
        Pb = tp._sym(P[b])
        e = _data_exact(Pb, A[b], q[b], l[b], u[b], r["g"][b])
        exact[b] = np.sum(e["gP"] * dP[b]) + np.sum(e["gA"] * dA[b])
        vals = []
        for sgn in (1.0, -1.0):
            x, low, upp = ref._optimum_active(Pb + sgn * H * dP[b], A[b] + sgn * H * dA[b], q[b], l[b], u[b])
            keep[b] &= bool(np.array_equal(low, e["low"]) and np.array_equal(upp, e["upp"]))
            vals.append(r["g"][b] @ x)
        fd[b] = (vals[0] - vals[1]) / (2 * H)
    err = float((np.abs(fd - exact) / np.maximum(1.0, np.abs(exact)))[keep].max())
    return dict(exact=exact, fd=fd, keep=keep, err=err)


def test_directional_difference_reference():
    """The CPU directional difference agrees with the formula within the finite-difference bound on (nearly) every
    clear QP; 100 x its error is the tolerance of test_sensitivity_data.py's qp_solution check."""
    d = _directional_fd()
    clear = ref._generic_sens_refs()["clear"]
    print(f"directional FD on {int(d['keep'].sum())} of {int(clear.sum())} clear QPs: error {d['err']:.2e}")
    assert d["keep"].sum() >= 0.9 * clear.sum()
    assert d["err"] <= FD_BOUND


# ----------------------------------------------------------------------------- ABI
def test_data_entry_points_in_header_mirror_and_library():
    """include/mpcq.h, _capi.py and the built library's dynamic symbol table agree on the two new entry points."""
    declared = ref._declared()
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
    assert len(lib.mpcq_sensitivity_data_device.argtypes) == 10 and len(lib.mpcq_sensitivity_data.argtypes) == 9


def test_methods_exist():
    for name in ("sensitivity_data", "sensitivity_data_device"):
        assert callable(getattr(sm.BatchSolver, name))
    from solvempc_amd import diff
    assert callable(diff.qp_solution) and callable(diff.mpc_solution)

"""CPU references of the MIMO polish (mpcq_mimo_step_polish_device; solvempc_amd/csrc/mpcq_mimo_polish.hip, DESIGN.md
4.16) and the tests that pin them, and the fairness of the GPU tests' inputs, without any device code.

The oracle has no polish.  The references are tests/test_polish.py's ``_polish_ref`` (OSQP v0.6 polish.c in numpy) and
``_optimum`` (independent of OSQP's rule), applied per QP to an ``oracle.Solver``'s ``iterates()`` and ``scaling()``
exactly as tests/test_mimo_sensitivity_ref.py's ``_refs`` does.  Families: that file's (R, R-tight, Q, Q-tight, Q32, S,
odd) and R-pinned, R with w0 x 0 (nearly every QP has a bound pair j, n + j active: more than n reduced rows, the
stated deviation).  Settings: tight (eps_abs = eps_rel = 1e-6) and default.

What is asserted here, with the numbers printed:
* every QP ends SOLVED; at tight every QP polishes successfully; at default R, Q and Q-tight hold at least one
  unsuccessful QP (so the GPU file's "everything kept" comparisons are not empty);
* no rule margin min |(u^ - z^) - y^| is below TIE = 1e-6 and no success decision's margin
  min(|ln(pri_p / pri_a)|, |ln(dua_p / dua_a)|) is below DEC = 0.1, so the reference alone excludes no QP from the GPU
  comparisons;
* n_active stays within n except in R-pinned, and covers tests/test_mimo_sensitivity_ref.py's ranges at default;
* TOL of a family (tight) = max(1e-10, 100 x its _polish_ref-vs-_optimum error), tests/test_polish.py's rule (the x100
  covers the Schur elimination against an LU of the whole matrix), below 1e-7 on every family but Q-tight, whose
  ceiling is the next power of ten above its rule value (``CEILING``, the sensitivity file's pattern);
* the new entry point is in the header, the ctypes mirror and the built library, and the new Python names exist
  (these fail without the feature)."""
import functools
import inspect
import subprocess

import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import _capi

from test_mimo_sensitivity_ref import FAMILIES, _inputs
from test_polish import LMIN, _optimum, _polish_ref, _rel_err, _residuals, _sym
from test_sensitivity_ref import ROOT, _declared

TIE = 1e-6
DEC = 0.1
TIGHT = dict(eps_abs=1e-6, eps_rel=1e-6)
SETTINGS = {"tight": TIGHT, "default": {}}
ALL = sorted(FAMILIES) + ["R-pinned"]
CEILING = {"Q-tight": 1e-4}
# QPs of a family the GPU file may leave out of a comparison with the oracle side (<= 5 %)
CAP = dict({k: v[1] for k, v in FAMILIES.items()}, **{"R-pinned": 0})


def _family_inputs(name):
    if name != "R-pinned":
        return _inputs(name)
    f = dict(_inputs("R"))
    f["sh"] = dict(f["sh"], w0=0.0 * np.asarray(f["sh"]["w0"], dtype=np.float64))
    return f


def _decision(P, A, q, u, D, E, c, x, z, y, delta=1e-6, refine=3):
    """The polished candidate of _polish_ref whatever its fate (l = LMIN) and the margin of OSQP's success decision:
    min(|ln(pri_p / pri_a)|, |ln(dua_p / dua_a)|).  Returns (margin, upper-active rows)."""
    n, m = len(q), len(u)
    Ph = c * D[:, None] * _sym(P) * D[None, :]
    Ah = E[:, None] * np.asarray(A, dtype=np.float64).reshape(m, n) * D[None, :]
    qh, uh = c * D * q, E * u
    upp = uh - z < y
    Ared = Ah[upp]
    mr = Ared.shape[0]
    K = np.block([[Ph, Ared.T], [Ared, np.zeros((mr, mr))]])
    Kreg = K + np.diag(np.r_[np.full(n, delta), np.full(mr, -delta)])
    b = np.r_[-qh, uh[upp]]
    s = np.linalg.solve(Kreg, b)
    for _ in range(refine):
        s = s + np.linalg.solve(Kreg, b - K @ s)
    yp = np.zeros(m)
    yp[upp] = s[n:]
    t = Ah @ s[:n] + yp
    zp = np.minimum(t, uh)
    pri_a, dua_a = _residuals(Ph, Ah, qh, D, E, c, x, z, y)
    pri_p, dua_p = _residuals(Ph, Ah, qh, D, E, c, s[:n], zp, t - zp)
    with np.errstate(divide="ignore"):
        return float(min(abs(np.log(pri_p / pri_a)), abs(np.log(dua_p / dua_a)))), upp


@functools.lru_cache(maxsize=None)
def _prefs(name, setting):
    """The oracle side of (family, setting), once per session: per QP the dense operators, the step's q and u, status,
    iterations and the scaling of the oracle's solve, _polish_ref on its iterate (status, n_active, x, y, residuals,
    rule margin, the scaled polished point), the success decision's margin, the rule's set, and at tight _optimum's x
    and the family's TOL."""
    f = _family_inputs(name)
    B, nx, nu = f["Bd"].shape
    ny = np.asarray(f["sh"]["Cd"]).shape[0]
    N = f["N"]
    n, m = N * nu, 2 * N * nu
    l = np.full(m, LMIN)
    keys = ("st", "it", "q", "u", "D", "E", "c", "status", "n_active", "x", "y", "pri", "dua", "margin", "dec", "upp",
            "x_admm", "y_admm", "x_opt")
    out = {k: [] for k in keys}
    ops_list = []
    for b in range(B):
        ops = oracle.condense_mimo(dict(f["sh"], Ad=f["Ad"][b], Bd=f["Bd"][b]), N, f["s_rows"])
        s = oracle.Solver(ops["P"], np.zeros(n), ops["A"], l, ops["W0"], oracle.default_settings(**SETTINGS[setting]))
        D, E, c = s.scaling()
        q = oracle.mimo_gradient(ops, f["X"][b], f["U"][b], f["yref"])
        u = oracle.mimo_upper_bound(ops, f["X"][b], f["U"][b])
        assert s.update_gradient(q) and s.update_upper_bound(u)
        out["st"].append(s.solve())
        out["it"].append(s.info().iter)
        it = s.iterates()
        r = _polish_ref(ops["P"], ops["A"], q, l, u, D, E, c, *it)
        dec, upp = _decision(ops["P"], ops["A"], q, u, D, E, c, *it)
        for k in ("status", "n_active", "x", "y", "pri", "dua", "margin"):
            out[k].append(r[k])
        for k, v in (("q", q), ("u", u), ("D", D), ("E", E), ("c", c), ("dec", dec), ("upp", upp), ("x_admm", s.x()),
                     ("y_admm", s.y())):
            out[k].append(v)
        out["x_opt"].append(_optimum(ops["P"], ops["A"], q, l, u)[0] if setting == "tight" and name != "R-pinned"
                            else np.full(n, np.nan))
        ops_list.append(ops)
    out = {k: np.asarray(v) for k, v in out.items()}
    out.update(ops=ops_list, dims=(B, N, nx, nu, ny, n, m), inputs=f, l=l)
    if setting == "tight" and name != "R-pinned":
        ok = out["status"] == 1
        out["err"] = float(_rel_err(out["x"][ok], out["x_opt"][ok]).max(initial=0.0))
        out["tol"] = max(1e-10, 100.0 * out["err"])
    return out


# ----------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("setting", ["tight", "default"])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_family_references(name, setting):
    r = _prefs(name, setting)
    B, N, nx, nu, ny, n, m = r["dims"]
    na, bad = r["n_active"], r["status"] != 1
    print(f"{name} / {setting}: B {B}, n {n}; iterations up to {r['it'].max()}, {int(bad.sum())} of {B} unsuccessful, "
          f"n_active {na.min()}..{na.max()}, smallest rule margin {r['margin'].min():.2e}, smallest decision margin "
          f"{r['dec'].min():.3f}")
    assert np.all(r["st"] == oracle.SOLVED)
    assert na.max() <= n
    assert r["margin"].min() >= TIE, r["margin"].min()
    assert r["dec"].min() >= DEC, r["dec"].min()
    assert CAP[name] <= 0.05 * B
    if setting == "tight":
        assert not bad.any(), np.flatnonzero(bad)
        admm = _rel_err(r["x_admm"], r["x_opt"])
        print(f"  _polish_ref against _optimum {r['err']:.2e} (TOL {r['tol']:.1e}); the ADMM point is "
              f"{admm.min():.1e} .. {admm.max():.1e} away")
        assert r["tol"] < CEILING.get(name, 1e-7), r["tol"]
    else:
        if name in ("R", "Q", "Q-tight"):
            assert bad.any()
        rng_ = FAMILIES[name][0]
        if rng_ is not None:
            assert na.min() <= rng_[0] and na.max() >= rng_[1], (na.min(), na.max())


def test_r_pinned_has_more_than_n_active_rows():
    r = _prefs("R-pinned", "default")
    B, N, nx, nu, ny, n, m = r["dims"]
    over = r["n_active"] > n
    print(f"R-pinned / default: {int(over.sum())} of {B} QPs above n = {n} active rows (up to {r['n_active'].max()}), "
          f"smallest rule margin {r['margin'].min():.2e}")
    assert np.all(r["st"] == oracle.SOLVED)
    assert over.sum() >= 1
    # (a pinned pair's rows sit at u^ - z^ = y^ up to the iterate's accuracy: the rule margin is no bar here, and
    # the GPU file compares such a QP with the device's own twin only, never with this count)
    pair = (r["upp"][:, :n] & r["upp"][:, n:]).any(axis=1)
    assert np.all(pair[over])  # (above n rows only through an active bound pair)


def test_entry_point_in_header_mirror_and_library():
    name = "mpcq_mimo_step_polish_device"
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sm.library_path())], check=True, capture_output=True,
                        text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    assert name in _declared() and name in _capi.EXPORTS and name in exported
    f = getattr(sm.lib(), name)
    assert f.restype is not None and len(f.argtypes) == 5
    hdr = (ROOT / "include" / "mpcq.h").read_text()
    assert "DESIGN.md 4.16" in hdr


def test_python_names_exist():
    from solvempc_amd import diff

    assert callable(sm.BatchSolver.mimo_step_polish_device)
    assert "polish" in inspect.signature(diff.mimo_solution).parameters
    assert inspect.signature(diff.mimo_solution).parameters["polish"].default is False

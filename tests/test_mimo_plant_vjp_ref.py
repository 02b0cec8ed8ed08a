"""CPU references of the MIMO step's gradients with respect to the plant data (mpcq_mimo_plant_vjp*,
diff.mimo_plant_solution; solvempc_amd/csrc/mpcq_mimo_plant_vjp.hip) and the tests that pin them
without any device code, in the three-way pinning of tests/test_condense_vjp_ref.py.

* ``_condense_mimo_torch`` restates oracle/mpc_mimo.c's condensing in torch fp64 (r_k = Cd Ad^k by recursion, Su as
  the block-Toeplitz matrix of the running sums of r_k Bd, the operators expression by expression).  It is compared
  with ``oracle.condense_mimo``; the reference of everything else is its autograd vector-Jacobian product,
  ``_vjp_torch``.
* ``_vjp_torch`` is checked against central differences of ``oracle.condense_mimo`` in every entry of the nine plant
  arrays (bound: tests/test_sensitivity_data_ref.py's FD_BOUND with its halve-the-step rule).
* ``_closed_form_factored`` transcribes the factored form of DESIGN.md 4.17 in numpy: the specification of the
  kernel, which forms no n x n object.  It is compared with ``_vjp_torch`` fed the dense cotangents
  (``_dense_cotangents``) built from the same vectors; ``_factored_error`` is the disagreement E_f of a family, from
  which tests/test_mimo_plant_vjp.py takes its tolerance max(1e-12, 100 E_f).
* ``_plant_directional_fd`` is the end-to-end reference: the derivative of g . x* along a random direction in all
  nine arrays by ``_sens_exact`` -> ``_closed_form_factored``, against central differences of
  ``oracle.condense_mimo`` followed by ``_optimum``; its error is the base of the GPU file's layer tolerance.

The shapes are those of the families R, odd, S, Q and Q32 of tests/test_mimo_sensitivity_ref.py (``_inputs``)."""
import functools
import subprocess

import numpy as np
import pytest
import torch

import oracle
import solvempc_amd as sm
from solvempc_amd import _capi

import test_polish as tp
import test_sensitivity_data_ref as dref
import test_sensitivity_ref as ref
from test_mimo_sensitivity_ref import _inputs

LMIN = tp.LMIN
H = dref.H
FD_BOUND = dref.FD_BOUND
PLANT_KEYS = ("Ad", "Bd", "Cd", "Q", "R", "RD", "K", "K0", "w0")
COT_KEYS = ("P", "A", "Fx", "Fu", "Fr", "Sbar", "Ku", "W0")
SHAPE_FAMILIES = ("R", "odd", "S", "Q", "Q32")
NEW_SYMBOLS = ("mpcq_mimo_plant_vjp_device", "mpcq_mimo_plant_vjp")


# ----------------------------------------------------------------------------- the families' plants
def _family_plants(name, B=None):
    """(plants, X, U, yref, N, s_rows) of a family: ``plants`` maps PLANT_KEYS to arrays with a leading plant axis
    (the shared data repeated); yref is an array (zeros where the family has none)."""
    f = _inputs(name)
    B = f["Bd"].shape[0] if B is None else B
    plants = {"Ad": np.array(f["Ad"][:B], dtype=np.float64), "Bd": np.array(f["Bd"][:B], dtype=np.float64)}
    for k in PLANT_KEYS[2:]:
        v = np.asarray(f["sh"][k], dtype=np.float64)
        plants[k] = np.broadcast_to(v, (B,) + v.shape).copy()
    ny = plants["Cd"].shape[1]
    yref = np.zeros(ny) if f["yref"] is None else np.asarray(f["yref"], dtype=np.float64)
    return plants, np.asarray(f["X"][:B], dtype=np.float64), np.asarray(f["U"][:B], dtype=np.float64), yref, f["N"], \
        f["s_rows"]


def _one(plants, p):
    return {k: plants[k][p] for k in PLANT_KEYS}


# ----------------------------------------------------------------------------- the reference
def _condense_mimo_torch(pl, N, s_rows):
    """The MIMO condensed operators (torch fp64) of one plant given as a dict of torch tensors (PLANT_KEYS)."""
    Ad, Bd, Cd, Q, R, RD, K, K0, w0 = (pl[k] for k in PLANT_KEYS)
    f = dict(dtype=torch.float64)
    nx, nu = Bd.shape
    ny = Cd.shape[0]
    r = [Cd]
    for _ in range(N):
        r.append(r[-1] @ Ad)
    r = torch.stack(r)                                    # r_k = Cd Ad^k, k = 0 .. N
    cum = torch.cumsum(r[:N] @ Bd, dim=0)                 # C_d: running sums of CAB_k = r_k Bd
    d = torch.arange(N)[:, None] - torch.arange(N)[None, :]
    blocks = torch.where((d >= 0)[:, :, None, None], cum[d.clamp(min=0)], torch.zeros((), **f))
    Su = blocks.permute(0, 2, 1, 3).reshape(N * ny, N * nu)
    Sx = r[1:].reshape(N * ny, nx)
    L = torch.tril(torch.ones(N, N, **f))
    eyeN = torch.eye(N, **f)
    LL = torch.kron(L, torch.eye(nu, **f))
    Rb, RDb, Qb = torch.kron(eyeN, R), torch.kron(eyeN, RD), torch.kron(eyeN, Q)
    H1 = 2.0 * (LL.T @ Rb @ LL + RDb + Su.T @ Qb @ Su)
    Fu = 2.0 * (R.T.repeat(N, 1) + (Su[:, :nu].T @ Qb @ Su).T)   # (the diagonal blocks of LL' Rbar' are R')
    rows = (torch.arange(N) < s_rows).to(torch.float64)[:, None]
    S = torch.kron(rows, K)
    one = torch.ones(N, 1, **f)
    return {"P": (H1 + H1.T) / 2.0, "A": torch.cat([torch.kron(L, K0), -torch.kron(L, K0)]),
            "Fx": 2.0 * (Sx.T @ Qb @ Su).T, "Fu": Fu, "Fr": -2.0 * (Qb @ Su).T, "Sbar": torch.cat([S, -S]),
            "Ku": torch.cat([-torch.kron(one, K0), torch.kron(one, K0)]), "W0": w0.repeat(2 * N)}


def _as_torch(plant, grad=False):
    return {k: torch.tensor(np.asarray(plant[k], dtype=np.float64)).requires_grad_(grad) for k in PLANT_KEYS}


def _vjp_torch(plant, cots, N, s_rows):
    """Autograd VJP of _condense_mimo_torch for one plant: dict of numpy gradients (zeros for a datum nothing
    reaches); cots: dict of numpy cotangents, any subset of COT_KEYS."""
    pl = _as_torch(plant, grad=True)
    ops = _condense_mimo_torch(pl, N, s_rows)
    loss = sum((ops[k] * torch.from_numpy(np.asarray(c, dtype=np.float64))).sum() for k, c in cots.items())
    grads = torch.autograd.grad(loss, [pl[k] for k in PLANT_KEYS], allow_unused=True)
    return {k: (np.zeros(tuple(pl[k].shape)) if g is None else g.numpy()) for k, g in zip(PLANT_KEYS, grads)}


def _dense_cotangents(gq, w, x, ya, X, U, yref, N):
    """The operator cotangents of include/mpcq.h's contract as dense arrays."""
    return {"P": 0.5 * (np.outer(gq, x) + np.outer(x, gq)), "A": np.outer(ya, gq) - np.outer(w, x),
            "Fx": np.outer(gq, X), "Fu": np.outer(gq, U), "Fr": np.outer(gq, np.tile(yref, N)),
            "Sbar": np.outer(w, X), "Ku": np.outer(w, U), "W0": np.array(w, dtype=np.float64)}


def _closed_form_factored(plant, N, s_rows, gq, w, x, ya, X, U, yref):
    """The factored form of DESIGN.md 4.17, line by line, in numpy: a = gq and b = x in N blocks of n_u, w and ya
    split as [top; bottom] in N blocks each.  No n x n object is formed."""
    Ad, Bd, Cd, Q = (np.asarray(plant[k], dtype=np.float64) for k in ("Ad", "Bd", "Cd", "Q"))
    nx, nu = Bd.shape
    ny = Cd.shape[0]
    n = N * nu
    a, b = np.reshape(gq, (N, nu)), np.reshape(x, (N, nu))
    wt, wb = np.reshape(w[:n], (N, nu)), np.reshape(w[n:], (N, nu))
    yt, yb = np.reshape(ya[:n], (N, nu)), np.reshape(ya[n:], (N, nu))
    pa, pb = np.cumsum(a, axis=0), np.cumsum(b, axis=0)
    r = [Cd]
    for _ in range(N):
        r.append(r[-1] @ Ad)
    r = np.array(r)
    C = np.cumsum(r[:N] @ Bd, axis=0)
    sa = np.array([sum(C[i - j] @ a[j] for j in range(i + 1)) for i in range(N)])
    sb = np.array([sum(C[i - j] @ b[j] for j in range(i + 1)) for i in range(N)])
    e = np.array([r[i + 1] @ X + C[i] @ U - yref for i in range(N)])           # sx_i + cu_i - yref
    gRD = sum(np.outer(a[k], b[k]) + np.outer(b[k], a[k]) for k in range(N))
    gR = sum(np.outer(pa[k], pb[k]) + np.outer(pb[k], pa[k]) for k in range(N)) + 2.0 * np.outer(U, a.sum(axis=0))
    gQ = sum(np.outer(sa[i], sb[i]) + np.outer(sb[i], sa[i]) + 2.0 * np.outer(e[i], sa[i]) for i in range(N))
    v = np.array([(Q + Q.T) @ sb[i] + 2.0 * Q.T @ e[i] for i in range(N)])
    ww = np.array([(Q + Q.T) @ sa[i] for i in range(N)])
    qs = np.array([Q @ sa[i] for i in range(N)])
    Gc = np.array([sum(np.outer(v[i], a[i - d]) + np.outer(ww[i], b[i - d]) for i in range(d, N))
                   + 2.0 * np.outer(qs[d], U) for d in range(N)])
    GCAB = np.cumsum(Gc[::-1], axis=0)[::-1]
    gBd = sum(r[k].T @ GCAB[k] for k in range(N))
    rho = np.zeros((N + 1, ny, nx))
    for k in range(N):
        rho[k] += GCAB[k] @ Bd.T
    for k in range(1, N + 1):
        rho[k] += 2.0 * np.outer(qs[k - 1], X)                                  # GSx_(k-1)
    gAd = np.zeros((nx, nx))
    for k in range(N, 0, -1):
        gAd += r[k - 1].T @ rho[k]
        rho[k - 1] += rho[k] @ Ad.T
    dw = wt - wb
    rows = min(s_rows, N)
    gK = np.outer(dw[:rows].sum(axis=0), X)
    gK0 = sum(np.outer(yt[i] - yb[i], pa[i]) - np.outer(dw[i], pb[i]) for i in range(N)) \
        + np.outer(-dw.sum(axis=0), U)
    return {"Ad": gAd, "Bd": gBd, "Cd": rho[0], "Q": gQ, "R": gR, "RD": gRD, "K": gK, "K0": gK0,
            "w0": (wt + wb).sum(axis=0)}


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max(initial=0.0)) / max(1.0, float(np.abs(b).max(initial=0.0)))


def _random_vectors(seed, n):
    """(gq, w, x, ya): standard-normal stand-ins for the four vectors the cotangents are built from."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=n), rng.normal(size=2 * n), rng.normal(size=n), rng.normal(size=2 * n)


@functools.lru_cache(maxsize=None)
def _factored_error(name, s_rows=None):
    """E_f of a family's shape: the largest disagreement, over the nine arrays, of _closed_form_factored and
    _vjp_torch of the dense cotangents, on the family's first plant and state with random vectors (relative to
    max(1, |autograd|_inf) per array).  s_rows: the family's own unless given."""
    plants, X, U, yref, N, s_fam = _family_plants(name, 1)
    s_rows = s_fam if s_rows is None else s_rows
    pl = _one(plants, 0)
    n = N * pl["Bd"].shape[1]
    gq, w, x, ya = _random_vectors(60 + N + s_rows, n)
    want = _vjp_torch(pl, _dense_cotangents(gq, w, x, ya, X[0], U[0], yref, N), N, s_rows)
    got = _closed_form_factored(pl, N, s_rows, gq, w, x, ya, X[0], U[0], yref)
    return max(_rel(got[k], want[k]) for k in PLANT_KEYS)


def _family_shape(name):
    """The family whose shape (and so whose E_f) a GPU family shares."""
    return {"R-tight": "R", "Q-tight": "Q"}.get(name, name)


# ----------------------------------------------------------------------------- the restated condensing
@pytest.mark.parametrize("name", SHAPE_FAMILIES)
def test_condense_mimo_torch_matches_the_oracle(name):
    plants, _, _, _, N, s_rows = _family_plants(name, 2)
    worst = 0.0
    for p in range(2):
        pl = _one(plants, p)
        want = oracle.condense_mimo(pl, N, s_rows)
        with torch.no_grad():
            got = _condense_mimo_torch(_as_torch(pl), N, s_rows)
        for key in COT_KEYS:
            assert tuple(got[key].shape) == want[key].shape, key
            err = _rel(got[key].numpy(), want[key])
            worst = max(worst, err)
            assert err <= 1e-12, (key, err)
    print(f"{name}: _condense_mimo_torch vs oracle.condense_mimo, worst relative error {worst:.1e}")


# ----------------------------------------------------------------------------- finite differences
def _random_cotangents(seed, N, nx, nu, ny):
    rng = np.random.default_rng(seed)
    n, m = N * nu, 2 * N * nu
    shapes = {"P": (n, n), "A": (m, n), "Fx": (n, nx), "Fu": (n, nu), "Fr": (n, N * ny), "Sbar": (m, nx),
              "Ku": (m, nu), "W0": (m,)}
    return {key: rng.normal(size=s) for key, s in shapes.items()}


def _fd_vjp(plant, N, s_rows, cots, h):
    """Largest error of _vjp_torch against central differences of sum_op <cot, oracle.condense_mimo(.)[op]> in every
    entry of the nine plant arrays (step h max(1, |entry|)), relative to max(1, |gradient|_inf)."""
    grads = _vjp_torch(plant, cots, N, s_rows)

    def value(pl):
        ops = oracle.condense_mimo(pl, N, s_rows)
        return sum(float(np.sum(ops[key] * c)) for key, c in cots.items())

    scale = max(1.0, max(float(np.abs(g).max()) for g in grads.values()))
    err = 0.0
    for key in PLANT_KEYS:
        base = np.array(plant[key], dtype=np.float64)
        for idx in np.ndindex(base.shape):
            step = h * max(1.0, abs(float(base[idx])))
            vals = []
            for sgn in (1.0, -1.0):
                v = base.copy()
                v[idx] += sgn * step
                vals.append(value({**plant, key: v}))
            err = max(err, abs((vals[0] - vals[1]) / (2 * step) - float(grads[key][idx])))
    return err / scale


@pytest.mark.parametrize("name", ["R", "odd", "S"])
def test_vjp_torch_matches_finite_differences(name):
    plants, _, _, _, N, s_rows = _family_plants(name, 1)
    pl = _one(plants, 0)
    nx, nu = pl["Bd"].shape
    cots = _random_cotangents(40 + N, N, nx, nu, pl["Cd"].shape[0])
    err = _fd_vjp(pl, N, s_rows, cots, H)
    print(f"{name}: FD error {err:.2e} at h = {H:g}")
    if err > FD_BOUND:
        err2 = _fd_vjp(pl, N, s_rows, cots, H / 2)
        print(f"{name}: FD error {err2:.2e} at h = {H / 2:g} (x{err / err2:.2f} smaller)")
        assert 2.5 <= err / err2 <= 6.0, (err, err2)
        err = err2
    assert err <= FD_BOUND, err


# ----------------------------------------------------------------------------- the factored form
def _r_shape_cases():
    N = _inputs("R")["N"]
    return [(name, None) for name in SHAPE_FAMILIES] + [("R", 0), ("R", N + 5)]


@pytest.mark.parametrize("name,s_rows", _r_shape_cases())
def test_factored_form_matches_autograd(name, s_rows):
    err = _factored_error(name, s_rows)
    print(f"{name} (s_rows {'own' if s_rows is None else s_rows}): factored form vs autograd of the dense cotangents, "
          f"E_f = {err:.2e}")
    assert err <= 1e-12, err


def test_factored_form_one_cotangent_at_a_time():
    """Each operator's cotangent alone (the others absent): the lines of the factored form are attributed to the
    right operators.  With only gq (w = ya = 0, x = 0 in gP) and so on, on R's shape."""
    plants, X, U, yref, N, s_rows = _family_plants("R", 1)
    pl = _one(plants, 0)
    n = N * pl["Bd"].shape[1]
    gq, w, x, ya = _random_vectors(77, n)
    z, z2 = np.zeros(n), np.zeros(2 * n)
    for label, vec in (("w only", (z, w, x, z2)), ("ya only", (gq, z2, z, ya)), ("gq only", (gq, z2, x, z2))):
        a_, w_, x_, y_ = vec
        want = _vjp_torch(pl, _dense_cotangents(a_, w_, x_, y_, X[0], U[0], yref, N), N, s_rows)
        got = _closed_form_factored(pl, N, s_rows, a_, w_, x_, y_, X[0], U[0], yref)
        for k in PLANT_KEYS:
            assert _rel(got[k], want[k]) <= 1e-12, (label, k)


# ----------------------------------------------------------------------------- end to end
def _plant_directions(plants, seed=88):
    """Per plant, dv = N(0, 1) max(1e-3, |v|) for every entry v of the plant data; Q's direction is symmetrised,
    since mpcq_mimo_setup_plants_device reads Q as a symmetric matrix (include/mpcq.h), so that the device test's
    perturbed plants are ones the device's forward pass is defined for."""
    rng = np.random.default_rng(seed)
    dv = {k: rng.normal(size=plants[k].shape) * np.maximum(1e-3, np.abs(plants[k])) for k in PLANT_KEYS}
    dv["Q"] = 0.5 * (dv["Q"] + np.swapaxes(dv["Q"], -1, -2))
    return dv


DIR_QPS = 8  # QPs of a family the directional check uses: its first ones


@functools.lru_cache(maxsize=None)
def _plant_directional_fd(name):
    """On the first DIR_QPS QPs of a family with random cotangents g: the derivative of g . x* along
    _plant_directions by _optimum -> _sens_exact -> _closed_form_factored, and by central differences at h = H of
    oracle.condense_mimo followed by _optimum_active.  Returns dict(exact, fd, keep, err, n_active, g): per-QP
    values, the QPs whose active set is the same at both ends of the difference, and the largest
    |fd - exact| / max(1, |exact|) over them -- the reference's own error."""
    plants, X, U, yref, N, s_rows = _family_plants(name, DIR_QPS)
    B = DIR_QPS
    nu = plants["Bd"].shape[2]
    n, m = N * nu, 2 * N * nu
    g = ref._cotangents(_inputs(name)["seed"], B, n)
    dv = _plant_directions(plants)
    l = np.full(m, LMIN)
    exact, fd, keep, nact = np.zeros(B), np.zeros(B), np.ones(B, dtype=bool), np.zeros(B, dtype=int)

    def qp(pl, b):
        ops = oracle.condense_mimo(pl, N, s_rows)
        return ops, oracle.mimo_gradient(ops, X[b], U[b], yref), oracle.mimo_upper_bound(ops, X[b], U[b])

    for b in range(B):
        pb = _one(plants, b)
        ops, q, u = qp(pb, b)
        x, y = tp._optimum(ops["P"], ops["A"], q, l, u)
        low, upp = y < 0, y > 0
        assert not low.any()
        gq, _, gu = ref._sens_exact(ops["P"], ops["A"], low, upp, g[b])
        nact[b] = int(upp.sum())
        grads = _closed_form_factored(pb, N, s_rows, gq, gu, x, np.where(upp, y, 0.0), X[b], U[b], yref)
        exact[b] = sum(float(np.sum(grads[k] * dv[k][b])) for k in PLANT_KEYS)
        vals = []
        for sgn in (1.0, -1.0):
            om, qm, um = qp({k: pb[k] + sgn * H * dv[k][b] for k in PLANT_KEYS}, b)
            xm, lo, up = ref._optimum_active(om["P"], om["A"], qm, l, um)
            keep[b] &= bool(np.array_equal(lo, low) and np.array_equal(up, upp))
            vals.append(g[b] @ xm)
        fd[b] = (vals[0] - vals[1]) / (2 * H)
    err = float((np.abs(fd - exact) / np.maximum(1.0, np.abs(exact)))[keep].max())
    return dict(exact=exact, fd=fd, keep=keep, err=err, n_active=nact, g=g)


@pytest.mark.parametrize("name", ["R", "odd"])
def test_plant_directional_difference_reference(name):
    """Every active set stays put, and the difference quotient agrees with the chain of references within the
    finite-difference bound; 100 x R's error is the tolerance of tests/test_mimo_plant_vjp.py's layer check."""
    d = _plant_directional_fd(name)
    print(f"{name}: plant directional FD on {int(d['keep'].sum())} of {len(d['keep'])} QPs (active rows "
          f"{sorted(set(d['n_active'].tolist()))}): error {d['err']:.2e}")
    assert d["keep"].all()
    assert (d["n_active"] > 0).any()
    assert d["err"] <= FD_BOUND


# ----------------------------------------------------------------------------- ABI
def test_plant_vjp_entry_points_in_header_mirror_and_library():
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
    assert len(lib.mpcq_mimo_plant_vjp_device.argtypes) == 25 and len(lib.mpcq_mimo_plant_vjp.argtypes) == 24
    assert "DESIGN.md 4.17" in (ref.ROOT / "include" / "mpcq.h").read_text()


def test_python_names_exist():
    for name in ("mimo_plant_vjp", "mimo_plant_vjp_device"):
        assert callable(getattr(sm.BatchSolver, name)), name
    from solvempc_amd import diff
    assert callable(diff.mimo_plant_solution)

"""CPU references of the condensing's vector-Jacobian product (mpcq_condense_vjp*, diff.mpc_plant_solution;
solvempc_amd/csrc/mpcq_condense_vjp.hip) and the tests that pin them without any device code.

* ``_condense_torch`` restates the condensing in torch fp64 (r_k = Cd Ad^k by recursion, Su as a Toeplitz matrix of
  the running sums of r_k Bd, the operators expression by expression).  It is compared with ``oracle.condense``; the
  reference of everything else is its autograd vector-Jacobian product, ``_vjp_torch``.
* ``_vjp_torch`` is checked against central differences of ``oracle.condense`` in every entry of the plant data
  (bound: tests/test_sensitivity_data_ref.py's FD_BOUND with its halve-the-step rule; the operators are polynomials
  of degree up to 2N + 1 in Ad, so the quotient carries a truncation error ~h^2).
* ``_closed_form`` transcribes include/mpcq.h's contract in numpy: the specification of the kernel, independent of
  autograd.
* ``_plant_directional_fd`` is the end-to-end reference of tests/test_condense_vjp.py's layer test: the derivative
  of g . x* along a random direction in the plant data by tests/test_sensitivity_data_ref.py's ``_data_exact`` ->
  operator cotangents -> ``_vjp_torch``, against central differences of ``oracle.condense`` followed by
  ``_optimum_active``."""
import functools
import subprocess

import numpy as np
import pytest
import torch

import oracle
import solvempc_amd as sm
from solvempc_amd import _capi, workload

import test_polish as tp
import test_sensitivity_data_ref as dref
import test_sensitivity_ref as ref

LMIN = tp.LMIN
H = dref.H
FD_BOUND = dref.FD_BOUND
PLANT_KEYS = ("Ad", "Bd", "Cd", "K", "Q", "R", "RD")
COT_KEYS = ("P", "A", "Fx", "Fu", "Fr", "Sbar", "Ku")
SHAPES = ((20, 10), (5, 10), (17, 3), (32, 10))
NEW_SYMBOLS = ("mpcq_condense_vjp_device", "mpcq_condense_vjp")


# ----------------------------------------------------------------------------- the reference
def _condense_torch(pl, N, s_rows):
    """The condensed operators (torch fp64) of one plant given as a dict of torch tensors Ad (nx, nx), Bd, Cd, K
    (nx) and 0-d Q, R, RD."""
    Ad, Bd, Cd, K, Q, R, RD = (pl[k] for k in PLANT_KEYS)
    f = dict(dtype=torch.float64)
    r = [Cd]
    for _ in range(N):
        r.append(r[-1] @ Ad)
    r = torch.stack(r)                                    # r_k = Cd Ad^k, k = 0 .. N
    cum = torch.cumsum(r[:N] @ Bd, dim=0)                 # running sums of CAB_k = r_k Bd
    d = torch.arange(N)[:, None] - torch.arange(N)[None, :]
    Su = torch.where(d >= 0, cum[d.clamp(min=0)], torch.zeros((), **f))
    Sx = r[1:]
    L = torch.tril(torch.ones(N, N, **f))
    H1 = 2.0 * (R * (L.T @ L) + RD * torch.eye(N, **f) + Q * (Su.T @ Su))
    rows = (torch.arange(N) < s_rows).to(torch.float64)[:, None] * K[None, :]
    one = torch.ones(N, **f)
    return {"P": (H1 + H1.T) / 2.0, "A": torch.cat([K[0] * L, -K[0] * L]), "Fx": 2.0 * Q * (Su.T @ Sx),
            "Fu": 2.0 * (R + Q * (Su[:, 0] @ Su)), "Fr": -2.0 * Q * Su.T, "Sbar": torch.cat([rows, -rows]),
            "Ku": torch.cat([-K[0] * one, K[0] * one]), "W0": torch.full((2 * N,), 255.0, **f)}


def _as_torch(plant, grad=False):
    return {k: torch.tensor(np.asarray(plant[k], dtype=np.float64)).requires_grad_(grad) for k in PLANT_KEYS}


def _vjp_torch(plant, cots, N, s_rows):
    """Autograd VJP of _condense_torch for one plant: dict of numpy gradients (zeros for a datum nothing reaches);
    cots: dict of numpy cotangents, any subset of COT_KEYS."""
    pl = _as_torch(plant, grad=True)
    ops = _condense_torch(pl, N, s_rows)
    loss = sum((ops[k] * torch.from_numpy(np.asarray(c, dtype=np.float64))).sum() for k, c in cots.items()
               if c is not None)
    grads = torch.autograd.grad(loss, [pl[k] for k in PLANT_KEYS], allow_unused=True)
    return {k: (np.zeros(tuple(pl[k].shape)) if g is None else g.numpy()) for k, g in zip(PLANT_KEYS, grads)}


def _vjp_torch_batch(plants, cots, N, s_rows):
    """_vjp_torch plant by plant: ``plants`` and ``cots`` carry a leading plant axis."""
    k = len(plants["Ad"])
    outs = [_vjp_torch({key: plants[key][p] for key in PLANT_KEYS},
                       {key: c[p] for key, c in cots.items() if c is not None}, N, s_rows) for p in range(k)]
    return {key: np.stack([o[key] for o in outs]) for key in PLANT_KEYS}


def _closed_form(plant, cots, N, s_rows):
    """include/mpcq.h's contract, line by line, in numpy."""
    Ad, Bd, Cd = (np.asarray(plant[k], dtype=np.float64) for k in ("Ad", "Bd", "Cd"))
    Q = float(plant["Q"])
    nx = len(Bd)
    z = {"P": (N, N), "A": (2 * N, N), "Fx": (N, nx), "Fu": (N,), "Fr": (N, N), "Sbar": (2 * N, nx), "Ku": (2 * N,)}
    g = {k: (np.zeros(s) if cots.get(k) is None else np.asarray(cots[k], dtype=np.float64)) for k, s in z.items()}
    r = [Cd]
    for _ in range(N):
        r.append(r[-1] @ Ad)
    r = np.array(r)
    cum = np.cumsum(r[:N] @ Bd)
    S = np.array([[cum[i - j] if j <= i else 0.0 for j in range(N)] for i in range(N)])
    Sx = r[1:]
    L = np.tril(np.ones((N, N)))
    Ps = g["P"] + g["P"].T
    gR = np.sum(Ps * (L.T @ L)) + 2.0 * g["Fu"].sum()
    gRD = np.trace(Ps)
    gQ = (np.sum(Ps * (S.T @ S)) + 2.0 * g["Fu"] @ (S[:, 0] @ S) - 2.0 * np.sum(g["Fr"] * S.T)
          + 2.0 * np.sum(g["Fx"] * (S.T @ Sx)))
    GS = 2 * Q * S @ Ps + 2 * Q * np.outer(S[:, 0], g["Fu"]) - 2 * Q * g["Fr"].T + 2 * Q * Sx @ g["Fx"].T
    GS[:, 0] += 2 * Q * S @ g["Fu"]
    GS = np.tril(GS)
    GSx = 2 * Q * S @ g["Fx"]
    Gc = np.array([np.trace(GS, -d) for d in range(N)])
    GCAB = np.cumsum(Gc[::-1])[::-1]
    gBd = GCAB @ r[:N]
    rho = np.zeros((N + 1, nx))
    rho[:N] += GCAB[:, None] * Bd[None, :]
    rho[1:] += GSx
    gAd = np.zeros((nx, nx))
    for k in range(N, 0, -1):
        gAd += np.outer(r[k - 1], rho[k])
        rho[k - 1] += rho[k] @ Ad.T
    rows = min(s_rows, N)
    gK = (g["Sbar"][:rows] - g["Sbar"][N:N + rows]).sum(axis=0)
    gK[0] += np.sum(np.tril(g["A"][:N] - g["A"][N:])) - g["Ku"][:N].sum() + g["Ku"][N:].sum()
    return {"Ad": gAd, "Bd": gBd, "Cd": rho[0], "K": gK, "Q": np.float64(gQ), "R": np.float64(gR),
            "RD": np.float64(gRD)}


def _random_cotangents(seed, N, nx, k=None):
    """One standard-normal cotangent per operator (with a leading plant axis k when given)."""
    rng = np.random.default_rng(seed)
    lead = () if k is None else (k,)
    shapes = {"P": (N, N), "A": (2 * N, N), "Fx": (N, nx), "Fu": (N,), "Fr": (N, N), "Sbar": (2 * N, nx),
              "Ku": (2 * N,)}
    return {key: rng.normal(size=lead + s) for key, s in shapes.items()}


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max(initial=0.0)) / max(1.0, float(np.abs(b).max(initial=0.0)))


# ----------------------------------------------------------------------------- the restated condensing
@pytest.mark.parametrize("N,s_rows", SHAPES)
def test_condense_torch_matches_the_oracle(plant, N, s_rows):
    want = oracle.condense(plant, N, s_rows)
    with torch.no_grad():
        got = _condense_torch(_as_torch(plant), N, s_rows)
    worst = 0.0
    for key in COT_KEYS + ("W0",):
        assert tuple(got[key].shape) == want[key].shape, key
        err = _rel(got[key].numpy(), want[key])
        worst = max(worst, err)
        assert err <= 1e-12, (key, err)
    print(f"N={N} s_rows={s_rows}: _condense_torch vs oracle.condense, worst relative error {worst:.1e}")


# ----------------------------------------------------------------------------- finite differences
def _fd_vjp(plant, N, s_rows, cots, h):
    """Largest error of _vjp_torch against central differences of sum_op <cot, oracle.condense(.)[op]> in every
    entry of the plant data (step h max(1, |entry|)), relative to max(1, |gradient|_inf)."""
    grads = _vjp_torch(plant, cots, N, s_rows)

    def value(pl):
        ops = oracle.condense(pl, N, s_rows)
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
                vals.append(value({**plant, key: v if v.ndim else float(v)}))
            err = max(err, abs((vals[0] - vals[1]) / (2 * step) - float(grads[key][idx])))
    return err / scale


@pytest.mark.parametrize("N,s_rows", SHAPES)
def test_vjp_torch_matches_finite_differences(plant, N, s_rows):
    cots = _random_cotangents(40 + N, N, 4)
    err = _fd_vjp(plant, N, s_rows, cots, H)
    print(f"N={N} s_rows={s_rows}: FD error {err:.2e} at h = {H:g}")
    if err > FD_BOUND:
        err2 = _fd_vjp(plant, N, s_rows, cots, H / 2)
        print(f"N={N} s_rows={s_rows}: FD error {err2:.2e} at h = {H / 2:g} (x{err / err2:.2f} smaller)")
        assert 2.5 <= err / err2 <= 6.0, (err, err2)
        err = err2
    assert err <= FD_BOUND, err


# ----------------------------------------------------------------------------- the closed form
@pytest.mark.parametrize("N,s_rows", SHAPES + ((1, 0), (20, 25)))
def test_closed_form_matches_autograd(plant, N, s_rows):
    cots = _random_cotangents(60 + N, N, 4)
    want, got = _vjp_torch(plant, cots, N, s_rows), _closed_form(plant, cots, N, s_rows)
    worst = max(_rel(got[k], want[k]) for k in PLANT_KEYS)
    print(f"N={N} s_rows={s_rows}: closed form vs autograd, worst relative error {worst:.1e}")
    for k in PLANT_KEYS:
        assert _rel(got[k], want[k]) <= 1e-12, k
    # one cotangent at a time (the others absent)
    for key in COT_KEYS:
        one = {key: cots[key]}
        want, got = _vjp_torch(plant, one, N, s_rows), _closed_form(plant, one, N, s_rows)
        for k in PLANT_KEYS:
            assert _rel(got[k], want[k]) <= 1e-12, (key, k)


# ----------------------------------------------------------------------------- end to end
def _seeded_ref(B, N, seed=5):
    """A horizon reference per QP."""
    return np.random.default_rng(seed).uniform(-0.5, 0.5, size=(B, N))


def _stack_plants(plant, B, Ad=None, Bd=None):
    """B copies of the plant with a leading axis (Ad, Bd replaced when given)."""
    out = {k: np.broadcast_to(np.asarray(plant[k], dtype=np.float64), (B,) + np.shape(plant[k])).copy()
           for k in PLANT_KEYS}
    if Ad is not None:
        out["Ad"], out["Bd"] = np.array(Ad, dtype=np.float64), np.array(Bd, dtype=np.float64)
    return out


def _plant_directions(plants, seed=88):
    """Per plant, dv = N(0, 1) max(1e-3, |v|) for every entry v of the plant data."""
    rng = np.random.default_rng(seed)
    return {k: rng.normal(size=plants[k].shape) * np.maximum(1e-3, np.abs(plants[k])) for k in PLANT_KEYS}


def _operator_cotangents(e, X, U, rf):
    """Cotangents of the operators from those of the QP data, q = Fx X + Fu U + Fr ref, u = W0 + Sbar X + Ku U."""
    return {"P": e["gP"], "A": e["gA"], "Fx": np.outer(e["gq"], X), "Fu": e["gq"] * U, "Fr": np.outer(e["gq"], rf),
            "Sbar": np.outer(e["gu"], X), "Ku": e["gu"] * U}


def _qp(ops, X, U, rf):
    return ops["Fx"] @ X + ops["Fu"] * U + ops["Fr"] @ rf, ops["W0"] + ops["Sbar"] @ X + ops["Ku"] * U


@functools.lru_cache(maxsize=None)
def _plant_directional_fd():
    """On the eight QPs of tp._problem(plant, 20, 8, 1) with a seeded horizon reference: the derivative of g . x*
    along _plant_directions by _data_exact -> _operator_cotangents -> _vjp_torch, and by central differences at
    h = 1e-5 of oracle.condense followed by _optimum_active.  Returns dict(exact, fd, keep, err): per-QP values, the
    QPs whose active set is the same at both ends of the difference, and the largest |fd - exact| / max(1, |exact|)
    over them -- the reference's own error."""
    N, B, s_rows = 20, 8, 10
    plant = workload.reference_plant()
    _, X, U, _, _ = tp._problem(plant, N, B, 1)
    rf = _seeded_ref(B, N)
    g = ref._cotangents(1, B, N)
    plants = _stack_plants(plant, B)
    dv = _plant_directions(plants)
    l = np.full(2 * N, LMIN)
    exact, fd, keep, nact = np.zeros(B), np.zeros(B), np.ones(B, dtype=bool), np.zeros(B, dtype=int)
    for b in range(B):
        pb = {k: plants[k][b] for k in PLANT_KEYS}
        ops = oracle.condense({**pb, "Q": float(pb["Q"]), "R": float(pb["R"]), "RD": float(pb["RD"])}, N, s_rows)
        q, u = _qp(ops, X[b], U[b], rf[b])
        e = dref._data_exact(ops["P"], ops["A"], q, l, u, g[b])
        nact[b] = int(e["low"].sum() + e["upp"].sum())
        grads = _vjp_torch(pb, _operator_cotangents(e, X[b], U[b], rf[b]), N, s_rows)
        exact[b] = sum(float(np.sum(grads[k] * dv[k][b])) for k in PLANT_KEYS)
        vals = []
        for sgn in (1.0, -1.0):
            pm = {k: pb[k] + sgn * H * dv[k][b] for k in PLANT_KEYS}
            om = oracle.condense({**pm, "Q": float(pm["Q"]), "R": float(pm["R"]), "RD": float(pm["RD"])}, N, s_rows)
            qm, um = _qp(om, X[b], U[b], rf[b])
            x, low, upp = ref._optimum_active(om["P"], om["A"], qm, l, um)
            keep[b] &= bool(np.array_equal(low, e["low"]) and np.array_equal(upp, e["upp"]))
            vals.append(g[b] @ x)
        fd[b] = (vals[0] - vals[1]) / (2 * H)
    err = float((np.abs(fd - exact) / np.maximum(1.0, np.abs(exact)))[keep].max())
    return dict(exact=exact, fd=fd, keep=keep, err=err, n_active=nact)


def test_plant_directional_difference_reference():
    """Every active set stays put, and the difference quotient agrees with the chain of references within the
    finite-difference bound; 100 x its error is the tolerance of tests/test_condense_vjp.py's layer check."""
    d = _plant_directional_fd()
    print(f"plant directional FD on {int(d['keep'].sum())} of {len(d['keep'])} QPs (active rows "
          f"{sorted(set(d['n_active'].tolist()))}): error {d['err']:.2e}")
    assert d["keep"].all()
    assert d["err"] <= FD_BOUND


# ----------------------------------------------------------------------------- ABI
def test_vjp_entry_points_in_header_mirror_and_library():
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
    assert len(lib.mpcq_condense_vjp_device.argtypes) == 27 and len(lib.mpcq_condense_vjp.argtypes) == 26


def test_argument_refusals_need_no_device(plant):
    """The argument checks come before any device call: MPCQ_ERR_ARG with the outputs untouched."""
    pl = _stack_plants(plant, 2)
    for N, cots in ((33, {"Fu": np.zeros((2, 33))}), (0, {"Fu": np.zeros((2, 0))}), (20, {})):
        with pytest.raises(sm.MpcqError) as e:
            sm.condense_vjp(pl, cots, N)
        assert e.value.code == _capi.MPCQ_ERR_ARG, str(e.value)
    with pytest.raises(sm.MpcqError) as e:
        sm.condense_vjp(pl, {"Fu": np.zeros((2, 20))}, 20, s_rows=-1)
    assert e.value.code == _capi.MPCQ_ERR_ARG
    with pytest.raises(ValueError):
        sm.condense_vjp(pl, {"W0": np.zeros((2, 40))}, 20)


def test_vjp_kernel_is_listed_once_without_scratch():
    import os
    import shutil

    import tools.kernel_resources as kr
    if not os.path.isdir(kr.BUILD) or shutil.which("c++filt") is None or \
            not os.path.exists(f"{kr.LLVM}/clang-offload-bundler"):
        pytest.skip("needs the built objects and the ROCm LLVM tools")
    hit = [r for r in kr.table() if "condense_vjp_kernel" in r["kernel"]]
    assert len(hit) == 1, [r["kernel"] for r in hit]
    assert hit[0]["scratch"] == 0 and hit[0]["vgpr_spill"] == 0


def test_functions_exist():
    from solvempc_amd import diff
    assert callable(sm.condense_vjp) and callable(sm.condense_vjp_device) and callable(sm.condense)
    assert callable(diff.mpc_plant_solution)

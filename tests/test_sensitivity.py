"""Active-set sensitivities on the device (mpcq_sensitivity*, mpcq_mpc_step_gains*, solvempc_amd.diff;
solvempc_amd/csrc/mpcq_sens.hip) against the CPU references of tests/test_sensitivity_ref.py.

fp64 contexts follow the oracle's trajectory to ~1e-12 (tests/test_gpu.py), so on the first 512 QPs of a batch
(tests/test_polish.py's Python-loop prefix) the device must take ``_sens_ref``'s active-set decisions wherever
the decision margin is clear of a tie (>= 1e-8; at most 2 % of the prefix may be excluded, asserted) and return
its gradients within TOL relative to max(1, |reference|_inf).  TOL = max(1e-9, 100 x the references' own
disagreement) and is asserted below 1e-7 (test_sensitivity_ref._tol).  Seeds and observed shares of ties, from
test_sensitivity_ref.test_mpc_family_references: (N 20, seed 1) 0 of 512, (N 15, seed 3) 0 of 512, (N 32, seed 5)
0 of 512; the generic family (seed 21) 0 of 64.

Beyond the prefix and on every dtype the tests assert properties that need no reference (``_check_properties``):
with v = -gq, w = gl + gu the KKT rows P v + A' w = g and (A v)_i = 0 on the support of w, gl gu = 0, n_active the
support's size, zeros and -1 where the QP did not end SOLVED.  A solution with relative error TOL in (v, w) leaves
a row residual of at most TOL times the sum of the absolute terms of that row, so that sum (at least 1) is the
scale of each bound.

f32 and mixed contexts run with settings.polish = 1: where polish succeeded the warm state is the fp64 polished
point, whose active set is the optimum's, so those QPs are compared with ``_sens_exact`` at ``_optimum``'s active
set, excluding QPs whose optimum is within 1e-8 of violating strict complementarity (same cap)."""
import functools

import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import workload

import test_polish as tp
import test_sensitivity_ref as ref

pytestmark = pytest.mark.gpu

LMIN = tp.LMIN
PREFIX = tp.PREFIX
ERR_ARG, ERR_ORDER = sm._capi.MPCQ_ERR_ARG, sm._capi.MPCQ_ERR_ORDER


def _mpc_solver(ops, N, B, dtype="f64", settings=None, n_plants=1, operators=False):
    s = sm.BatchSolver(N, 2 * N, B, n_plants=n_plants, dtype=dtype, settings=settings)
    t = (lambda a: np.broadcast_to(a, (n_plants,) + np.shape(a)).copy()) if n_plants > 1 else (lambda a: a)
    s.setup(t(ops["P"]), t(np.zeros(N)), t(ops["A"]), t(np.full(2 * N, LMIN)), t(oracle.upper_bound(ops, np.zeros(4), 0.0)))
    if operators:
        s.mpc_set_operators(*[t(ops[k]) for k in ("Fx", "Fu", "Fr", "Sbar", "Ku", "W0")])
    return s


def _solve(ops, q, u, N, **kw):
    s = _mpc_solver(ops, N, q.shape[0], **kw)
    s.update_lin_cost(q)
    s.update_upper_bound(u)
    s.solve()
    return s


def _check_properties(P, A, g, gq, gl, gu, na, st, tol):
    """The reference-free properties of the module docstring on a whole batch.  P (n, n) / A (m, n) shared, or one
    per QP with a leading batch axis."""
    B, n = gq.shape
    P = np.broadcast_to(tp._sym(P) if np.ndim(P) == 2 else np.stack([tp._sym(p) for p in P]), (B, n, n))
    A = np.broadcast_to(A, (B,) + np.shape(A)[-2:])
    solved = st == sm.SOLVED
    assert np.all(gq[~solved] == 0) and np.all(gl[~solved] == 0) and np.all(gu[~solved] == 0)
    assert np.all(na[~solved] == -1) and np.all(na[solved] >= 0)
    assert np.all(gl * gu == 0)
    v, w = -gq, gl + gu
    supp = w != 0
    assert np.array_equal(supp.sum(axis=1)[solved], na[solved])
    res = np.einsum("bij,bj->bi", P, v) + np.einsum("bji,bj->bi", A, w) - g
    scale = np.maximum(1.0, (np.einsum("bij,bj->bi", np.abs(P), np.abs(v)) + np.einsum("bji,bj->bi", np.abs(A), np.abs(w))
                             + np.abs(g)).max(axis=1))
    r1 = (np.abs(res).max(axis=1) / scale)[solved]
    Av = np.einsum("bij,bj->bi", A, v)
    scale2 = np.maximum(1.0, np.einsum("bij,bj->bi", np.abs(A), np.abs(v)).max(axis=1, initial=0.0))
    r2 = (np.where(supp, np.abs(Av), 0.0).max(axis=1, initial=0.0) / scale2)[solved]
    print(f"  properties on {int(solved.sum())} of {B} QPs: stationarity {r1.max(initial=0):.2e}, A_a v {r2.max(initial=0):.2e}")
    assert r1.max(initial=0) <= tol and r2.max(initial=0) <= tol
    return solved


def _compare_prefix(r, out, out0, na, st, it, count=PREFIX):
    """Device results (cotangents g, and e_0) against _sens_ref on the reference prefix."""
    assert np.array_equal(st[:count], r["st"][:count]) and np.array_equal(it[:count], r["it"][:count])
    clear = r["clear"][:count]
    assert (~clear).mean() <= ref.MAX_TIES
    assert np.array_equal(na[:count][clear], r["n_active"][:count][clear])
    e = ref._rel(ref._stack(*out)[:count], r["ref"][:count])[clear]
    e0 = ref._rel(ref._stack(*out0)[:count], r["ref0"][:count])[clear]
    print(f"  prefix: max rel err {e.max():.2e} (g), {e0.max():.2e} (e_0), TOL {r['tol']:.1e}, {int((~clear).sum())} ties")
    assert e.max() <= r["tol"] and e0.max() <= r["tol"]


def _g_batch(r, B, n, seed):
    """The prefix's reference cotangents followed by seeded ones for the rest of the batch."""
    g = ref._cotangents(100 + seed, B, n)
    g[:min(B, len(r["g"]))] = r["g"][:B]
    return g


@pytest.mark.parametrize("kern,N", [("tile", 20), ("tile", 15), ("wave", 20), ("wave", 15), ("wave", 32), ("lane", 20)])
def test_f64_matches_reference_shared_plant(plant, monkeypatch, kern, N):
    """Shared plant on the tile path (4,096 QPs), on the wave path (under 8,192 QPs) and on the lane path: N = 20
    (the bench shape, remainder rows), N = 15 (odd horizon), N = 32 (m = 64 fills the wave)."""
    monkeypatch.setenv("MPCQ_KERNEL", kern)
    seed = ref.MPC_SEEDS[N]
    B = 4096 if kern == "tile" else 512
    r = ref._mpc_sens_refs(N, seed)
    ops, X, U, q, u = tp._problem(plant, N, B, seed)
    s = _solve(ops, q, u, N)
    assert s.path()[0] == kern
    g = _g_batch(r, B, N, seed)
    gq, gl, gu, na = s.sensitivity(g)
    gq0, gl0, gu0, na0 = s.sensitivity()
    st, it, _ = s.info()
    s.close()
    print(f"{kern} N={N}: n_active {na.min()}..{na.max()}")
    assert np.array_equal(na, na0)
    _compare_prefix(r, (gq, gl, gu), (gq0, gl0, gu0), na, st, it)
    _check_properties(ops["P"], ops["A"], g, gq, gl, gu, na, st, r["tol"])
    _check_properties(ops["P"], ops["A"], np.tile(np.eye(N)[0], (B, 1)), gq0, gl0, gu0, na0, st, r["tol"])
    assert np.all(gl == 0)  # (no lower bound in the MPC QP)


def test_f64_matches_reference_per_plant(plant):
    """A per-plant context (every QP its own copy of the plant: the per-QP factorisation and Schur complement)."""
    N, B = 20, PREFIX
    r = ref._mpc_sens_refs(N, ref.MPC_SEEDS[N])
    ops, X, U, q, u = tp._problem(plant, N, B, ref.MPC_SEEDS[N])
    s = _solve(ops, q, u, N, n_plants=B)
    assert s.path()[0] == "wave"
    gq, gl, gu, na = s.sensitivity(r["g"])
    gq0, gl0, gu0, na0 = s.sensitivity()
    st, it, _ = s.info()
    s.close()
    _compare_prefix(r, (gq, gl, gu), (gq0, gl0, gu0), na, st, it)
    _check_properties(ops["P"], ops["A"], r["g"], gq, gl, gu, na, st, r["tol"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_generic_family(dtype):
    """n = 7, m = 11 per-plant QPs with equality, one-sided, free and two-sided rows; QP 0 has no active row; one
    QP is given u < l after setup and ends MPCQ_INVALID_BOUNDS (zeros, -1).  f64 against _sens_ref, both dtypes
    the properties."""
    r = ref._generic_sens_refs()
    P, A, q, l, u = ref._generic_inputs()
    B, n = q.shape
    bad = 5
    l2, u2 = l.copy(), u.copy()
    l2[bad, 7], u2[bad, 7] = 1.0, -1.0
    s = sm.BatchSolver(n, ref.GEN_M, B, n_plants=B, dtype=dtype)
    s.setup(P, q, A, l, u)
    s.update_bounds(l2, u2)
    s.solve()
    assert s.path()[0] == "wave"
    out = s.sensitivity(r["g"])
    out0 = s.sensitivity()
    st, it, _ = s.info()
    s.close()
    assert st[bad] == sm.INVALID_BOUNDS and out[3][bad] == -1 and np.all(out[0][bad] == 0)
    keep = np.arange(B) != bad
    solved = _check_properties(P, A, r["g"], *out, st, r["tol"])
    _check_properties(P, A, np.tile(np.eye(n)[0], (B, 1)), *out0, st, r["tol"])
    assert solved[keep].sum() >= 0.9 * B
    if dtype == "f64":
        assert np.array_equal(st[keep], r["st"][keep]) and np.array_equal(it[keep], r["it"][keep])
        clear = r["clear"] & keep
        assert (~r["clear"]).mean() <= ref.MAX_TIES
        assert np.array_equal(out[3][clear], r["n_active"][clear]) and out[3][0] == 0
        e = ref._rel(ref._stack(*out[:3]), r["ref"])[clear]
        e0 = ref._rel(ref._stack(*out0[:3]), r["ref0"])[clear]
        print(f"generic: max rel err {e.max():.2e} (g), {e0.max():.2e} (e_0), TOL {r['tol']:.1e}")
        assert e.max() <= r["tol"] and e0.max() <= r["tol"]
        assert (out[1] != 0).any() and (out[2] != 0).any()  # lower- and upper-active rows both occur


def test_unconstrained_context():
    """m = 0: gq = -P^-1 g, n_active = 0, empty gl and gu."""
    rng = np.random.default_rng(31)
    n, B = 7, 8
    M = rng.normal(size=(B, n, n))
    P = M @ M.transpose(0, 2, 1) + 0.5 * np.eye(n)
    q, g = rng.normal(size=(B, n)), rng.normal(size=(B, n))
    e = np.zeros((B, 0))
    s = sm.BatchSolver(n, 0, B, n_plants=B)
    s.setup(P, q, np.zeros((B, 0, n)), e, e)
    s.solve()
    gq, gl, gu, na = s.sensitivity(g)
    st = s.info()[0]
    s.close()
    assert np.all(st == sm.SOLVED) and np.all(na == 0) and gl.shape == gu.shape == (B, 0)
    exact = np.stack([-np.linalg.solve(tp._sym(P[b]), g[b]) for b in range(B)])
    assert ref._rel(gq, exact).max() <= 1e-9


@functools.lru_cache(maxsize=None)
def _optimum_sets(N, seed, count=PREFIX):
    """_sens_exact at _optimum's active set on the prefix (cotangents of _mpc_sens_refs), and the optimum's
    strict-complementarity margin in the scaled space, min_i |u^_i - (A^ x^)_i - y^_i|."""
    r = ref._mpc_sens_refs(N, seed)
    ops, l = r["ops"], r["l"]
    u0 = oracle.upper_bound(ops, np.zeros(4), 0.0)
    tight = oracle.Solver(ops["P"], np.zeros(N), ops["A"], l, u0, oracle.default_settings(**tp._TIGHT))
    exact, margin, nact = [], [], []
    for b in range(count):
        tight.update_gradient(r["q"][b])
        tight.update_upper_bound(r["u"][b])
        tight.cold_start()
        x, y = tp._optimum(ops["P"], ops["A"], r["q"][b], l, r["u"][b], tight)
        low, upp = y < 0, y > 0
        exact.append(ref._stack(*ref._sens_exact(ops["P"], ops["A"], low, upp, r["g"][b])))
        margin.append(np.abs(r["E"] * (r["u"][b] - ops["A"] @ x) - r["c"] * y / r["E"]).min())
        nact.append(int(upp.sum()))
    return np.asarray(exact), np.asarray(margin), np.asarray(nact)


@pytest.mark.parametrize("dtype", ["mixed", "f32"])
def test_reduced_precision_with_polish(plant, monkeypatch, dtype):
    """mixed and f32 iterates on the tile path with settings.polish = 1: the sensitivities at the polished point
    are the optimum's (module docstring); the properties on the whole batch, with two primal-infeasible QPs."""
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    N, B = 20, 4096
    seed = ref.MPC_SEEDS[N]
    r = ref._mpc_sens_refs(N, seed)
    exact, margin, nact = _optimum_sets(N, seed)
    ops, X, U, q, u = tp._problem(plant, N, B, seed)
    u = u.copy()
    u[[1000, 2001]] = -1e3
    s = _solve(ops, q, u, N, dtype=dtype, settings=sm.default_settings(polish=1))
    assert s.path()[0] == "tile"
    g = _g_batch(r, B, N, seed)
    gq, gl, gu, na = s.sensitivity(g)
    st = s.info()[0]
    sp = s.polish_info()[0]
    s.close()
    assert st[1000] != sm.SOLVED and st[2001] != sm.SOLVED
    _check_properties(ops["P"], ops["A"], g, gq, gl, gu, na, st, r["tol"])
    clear = margin >= ref.TIE
    assert (~clear).mean() <= ref.MAX_TIES
    cmp = clear & (sp[:PREFIX] == 1)
    e = ref._rel(ref._stack(gq, gl, gu)[:PREFIX], exact)[cmp]
    print(f"{dtype}: {int(cmp.sum())} of {PREFIX} compared with the optimum's sensitivities, max rel err {e.max():.2e} "
          f"(TOL {r['tol']:.1e}), {int((~clear).sum())} ties")
    assert cmp.sum() >= 0.96 * PREFIX  # (tests/test_polish.py: at most 2 % unpolished; at most 2 % ties)
    assert np.array_equal(na[:PREFIX][cmp], nact[cmp])
    assert e.max() <= r["tol"]


# ----------------------------------------------------------------------------- step gains
def _chain(ops, gq, gu):
    """dX = Fx' gq + Sbar' gu, dU = Fu' gq + Ku' gu, dref = Fr' gq, summed in ascending row index as the device
    does (a BLAS product's own order would differ from it by rounding of the order of the 1e-12 bound)."""
    B = gq.shape[0]
    dX, dU, dref = np.zeros((B, ops["Fx"].shape[1])), np.zeros(B), np.zeros((B, gq.shape[1]))
    for i in range(gq.shape[1]):
        dX += gq[:, i, None] * ops["Fx"][i]
        dU += gq[:, i] * ops["Fu"][i]
        dref += gq[:, i, None] * ops["Fr"][i]
    for j in range(gu.shape[1]):
        dX += gu[:, j, None] * ops["Sbar"][j]
        dU += gu[:, j] * ops["Ku"][j]
    return dX, dU, dref


@pytest.mark.parametrize("n_plants", [1, 64])
def test_step_gains_equal_the_chain_rule(plant, n_plants):
    N, B = 20, 64
    ops, X, U, _, _ = tp._problem(plant, N, B, 1)
    s = _mpc_solver(ops, N, B, n_plants=n_plants, operators=True)
    s.mpc_step(X, U, 0.3)
    dX, dU, dref, na = s.mpc_step_gains()
    gq, gl, gu, na2 = s.sensitivity()
    s.close()
    cX, cU, cref = _chain(ops, gq, gu)
    assert np.array_equal(na, na2) and (na > 0).any() and (na == 0).any()
    for a, b in ((dX, cX), (dU[:, None], cU[:, None]), (dref, cref)):
        assert ref._rel(a, b).max() <= 1e-12


def test_step_gains_match_finite_differences(plant, monkeypatch):
    """mpc_step_gains() against central differences of _optimum's x*[0] through q(X, U, ref) and u(X, U) on 8 QPs
    of the prefix: the 4 with the largest strict-complementarity margin among those with an active row, and the 4
    among those with none.  Bound: the device against the exact sensitivities (TOL) plus the difference quotient's
    own error (1e-7, tests/test_sensitivity_ref.py), relative to max(1, |gains|_inf)."""
    monkeypatch.setenv("MPCQ_KERNEL", "wave")
    N, B, h = 20, PREFIX, 1e-4
    seed = ref.MPC_SEEDS[N]
    r = ref._mpc_sens_refs(N, seed)
    _, margin, nact = _optimum_sets(N, seed)
    ops, X, U, l = r["ops"], r["X"], r["U"], r["l"]
    order = np.argsort(-margin)
    pick = [b for b in order if nact[b] > 0][:4] + [b for b in order if nact[b] == 0][:4]
    refs = np.zeros((B, N))
    s = _mpc_solver(ops, N, B, operators=True)
    s.mpc_step_ref(X, U, refs)
    dX, dU, dref, na = s.mpc_step_gains()
    s.close()

    def x0(Xb, Ub, rb):
        q = ops["Fx"] @ Xb + ops["Fu"] * Ub + ops["Fr"] @ rb
        x, low, upp = ref._optimum_active(ops["P"], ops["A"], q, l, oracle.upper_bound(ops, Xb, Ub))
        return x[0], upp

    for b in pick:
        assert na[b] == nact[b]
        _, upp = x0(X[b], U[b], refs[b])
        fd = []
        for d in np.eye(4 + 1 + N):
            vals = []
            for sgn in (1.0, -1.0):
                v, up = x0(X[b] + sgn * h * d[:4], U[b] + sgn * h * d[4], refs[b] + sgn * h * d[5:])
                assert np.array_equal(up, upp), "the perturbation changed the active set"
                vals.append(v)
            fd.append((vals[0] - vals[1]) / (2 * h))
        fd = np.asarray(fd)
        dev = np.r_[dX[b], dU[b], dref[b]]
        err = np.abs(dev - fd).max() / max(1.0, np.abs(fd).max())
        print(f"QP {b}: n_active {na[b]}, gains vs finite differences {err:.2e}")
        assert err <= r["tol"] + 1e-7, (b, err)


# ----------------------------------------------------------------------------- transparency
@pytest.mark.parametrize("kern", ["tile", "wave"])
def test_a_sensitivity_call_changes_no_later_solve(plant, monkeypatch, kern):
    """solve, sensitivity, warm-started second step == the same two steps without the call, bit for bit (x, U,
    status, iter, rho): the tile path with its lazily published outputs, and the wave path with the call on a side
    stream."""
    import torch
    monkeypatch.setenv("MPCQ_KERNEL", kern)
    N, B = 20, 4096 if kern == "tile" else 512
    ops, X, U, _, _ = tp._problem(plant, N, B, 1)
    X2 = X * 0.9 + 0.01

    def run(call):
        s = _mpc_solver(ops, N, B, operators=True)
        Xd, X2d, Ud = (torch.from_numpy(a.copy()).cuda() for a in (X, X2, U))
        s.mpc_step_device(Xd.data_ptr(), Ud.data_ptr(), 0.0)
        assert s.path()[0] == kern
        keep = None
        if call:
            gq = torch.zeros(B, N, dtype=torch.float64, device="cuda")
            gu = torch.zeros(B, 2 * N, dtype=torch.float64, device="cuda")
            nat = torch.zeros(B, dtype=torch.int32, device="cuda")
            side = torch.cuda.Stream() if kern == "wave" else None
            s.sensitivity_device(0, gq.data_ptr(), 0, gu.data_ptr(), nat.data_ptr(), side.cuda_stream if side else None)
            keep = (gq, gu, nat, side)
        s.mpc_step_device(X2d.data_ptr(), Ud.data_ptr(), 0.0)
        torch.cuda.synchronize()
        out = [Ud.cpu().numpy(), s.solution(), *s.info()]
        if call:
            assert (keep[2].cpu().numpy() >= 0).all() and (keep[0].cpu().numpy()[:, 0] != 0).all()
        s.close()
        return out

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ----------------------------------------------------------------------------- autograd
def test_autograd_backward_matches_reference(plant, monkeypatch):
    import torch
    from solvempc_amd import diff
    N, B = 20, 64
    seed = ref.MPC_SEEDS[N]
    r = ref._mpc_sens_refs(N, seed)
    ops = r["ops"]
    s = _mpc_solver(ops, N, B, operators=True)
    assert s.path()[0] == "wave"
    X = torch.from_numpy(r["X"][:B].copy()).cuda().requires_grad_()
    U = torch.from_numpy(r["U"][:B].copy()).cuda().requires_grad_()
    R = torch.zeros(B, N, dtype=torch.float64, device="cuda", requires_grad=True)
    G = torch.from_numpy(r["g"][:B].copy()).cuda()
    x, status = diff.mpc_solution(s, X, U, R)
    assert np.array_equal(status.cpu().numpy(), r["st"][:B]) and np.array_equal(U.detach().cpu().numpy(), r["U"][:B])
    assert np.array_equal(x.detach().cpu().numpy(), s.solution())
    (x * G).sum().backward()
    n = N
    cX, cU, cref = _chain(ops, r["ref"][:B, :n], r["ref"][:B, n + 2 * N:])
    clear = r["clear"][:B]
    for t, c in ((X.grad, cX), (U.grad[:, None], cU[:, None]), (R.grad, cref)):
        assert ref._rel(t.cpu().numpy(), c)[clear].max() <= r["tol"]
    # backward after an intervening solve
    x, status = diff.mpc_solution(s, X, U, R)
    s.solve()
    with pytest.raises(RuntimeError, match="solved again"):
        (x * G).sum().backward()
    s.close()


# ----------------------------------------------------------------------------- refusals
def _raises(code, fn, *a, **kw):
    with pytest.raises(sm.MpcqError) as e:
        fn(*a, **kw)
    assert e.value.code == code, str(e.value)


def test_refusals(plant):
    import torch
    N, B = 20, 64
    ops, X, U, q, u = tp._problem(plant, N, B, 1)
    out = [torch.full((B, k), 7.0, dtype=torch.float64, device="cuda") for k in (N, 2 * N, 2 * N, 4, 1)]
    nat = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    gq, gl, gu, dX, dU = out
    sens = lambda s, st=None: s.sensitivity_device(0, gq.data_ptr(), gl.data_ptr(), gu.data_ptr(), nat.data_ptr(), st)
    gains = lambda s: s.mpc_step_gains_device(dX.data_ptr(), dU.data_ptr(), gq.data_ptr(), nat.data_ptr())
    Xd, Ud = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(U.copy()).cuda()

    # before a first solve; gains without operators; every output NULL
    s = _mpc_solver(ops, N, B)
    _raises(ERR_ORDER, sens, s)
    _raises(ERR_ORDER, s.sensitivity)
    s.update_lin_cost(q)
    s.update_upper_bound(u)
    s.solve()
    _raises(ERR_ARG, gains, s)
    _raises(ERR_ARG, s.mpc_step_gains)
    _raises(ERR_ARG, s.sensitivity_device)
    _raises(ERR_ARG, s.mpc_step_gains_device)
    # a stream under graph capture: refused, nothing recorded
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        _raises(ERR_ARG, sens, s, side.cuda_stream)
    torch.cuda.synchronize()
    sens(s)  # (and served afterwards)
    torch.cuda.synchronize()
    assert (nat.cpu().numpy() >= 0).all()
    nat.fill_(7)
    gq.fill_(7.0); gl.fill_(7.0); gu.fill_(7.0)
    # new data since the solve
    s.update_upper_bound(u)
    _raises(ERR_ORDER, sens, s)
    s.close()

    # after a stream run
    s = _mpc_solver(ops, N, B, operators=True)
    s.mpc_set_plant(plant["Ad"], plant["Bd"])
    s.mpc_step_device(Xd.data_ptr(), Ud.data_ptr(), 0.0)
    torch.cuda.synchronize()
    s.mpc_run_device(Xd.data_ptr(), Ud.data_ptr(), 0.0, 2, 9, 0, 0, 1e-2, side.cuda_stream)
    torch.cuda.synchronize()
    _raises(ERR_ORDER, sens, s)
    _raises(ERR_ORDER, gains, s)
    s.close()

    # after mpcq_mpc_plants_step_device (no operators kept)
    Ad, Bd = workload.randomized_plants(plant, 3, 0, B)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
    keep = [dev(Ad), dev(Bd), dev(np.tile(plant["Cd"], (B, 1))), dev(np.tile(plant["K"], (B, 1))),
            dev(np.full(B, plant["Q"])), dev(np.full(B, plant["R"])), dev(np.full(B, plant["RD"]))]
    p = sm.BatchSolver(N, 2 * N, B, n_plants=B)
    p.mpc_plants_step_device(4, 10, *[k.data_ptr() for k in keep], Xd.data_ptr(), Ud.data_ptr())
    torch.cuda.synchronize()
    _raises(ERR_ORDER, sens, p)
    _raises(ERR_ORDER, gains, p)
    p.close()

    # n > 32 or m > 64; a MIMO context (the SISO specialisation, n = 20: within the kernel's capacity)
    big = sm.BatchSolver(40, 80, 4, n_plants=4)
    _raises(ERR_ARG, sens, big)
    _raises(ERR_ARG, gains, big)
    big.close()
    sh = {"Cd": plant["Cd"][None, :], "Q": [[plant["Q"]]], "R": [[plant["R"]]], "RD": [[plant["RD"]]],
          "K": plant["K"][None, :], "K0": [[plant["K"][0]]], "w0": [255.0]}
    mk = [dev(Ad), dev(Bd[:, :, None])] + [dev(np.broadcast_to(np.asarray(sh[k], dtype=np.float64),
                                                               (B,) + np.asarray(sh[k]).shape).copy())
                                            for k in ("Cd", "Q", "R", "RD", "K", "K0", "w0")]
    mi = sm.BatchSolver(N, 2 * N, B, n_plants=B)
    mi.mimo_setup_plants_device(4, 1, 1, 10, *[k.data_ptr() for k in mk])
    Um = Ud.clone()
    mi.mimo_step_device(Xd.data_ptr(), Um.data_ptr())
    torch.cuda.synchronize()
    _raises(ERR_ARG, sens, mi)
    _raises(ERR_ARG, gains, mi)
    mi.close()

    torch.cuda.synchronize()
    for t in out:
        assert (t == 7.0).all()
    assert (nat == 7).all()

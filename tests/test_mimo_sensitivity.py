"""Active-set sensitivities and step gains of MIMO contexts on the device (mpcq_mimo_sensitivity*,
mpcq_mimo_step_vjp_device, mpcq_mimo_step_gains_device; solvempc_amd/csrc/mpcq_mimo_sens.hip)
against the CPU references of tests/test_mimo_sensitivity_ref.py, on that file's families.

* Exact at the reported set, every SOLVED QP: the support of gu under a random cotangent is the device's active set;
  n_active is its size, all right-hand sides of a call share it, and (gq, gu) match ``_sens_exact`` at that set
  within the family's TOL (from the references alone), relative to max(1, |ref|_inf).
* Reference-free: P v + A' w = g and (A v)_i = 0 on the support, scaled as tests/test_sensitivity.py's
  ``_check_properties``.
* The set is the oracle's (polish's rule on the oracle's iterate) on every QP whose iteration count is the oracle's
  (tests/test_mimo.py's termination tie) and whose rule margin is at least TIE; at most 5 % of a family may be
  excluded (the CPU file shows that the reference alone excludes none).
* Gains = the numpy chain rule of the device's own gq, gu (1e-12 relative: the same sums, fp64, another order), the
  oracle-side chain within TOL, and mimo_step_vjp_device with an explicit g = e_r bit for bit.
* Determinism, read-only, n_rhs consistency, unsolved QPs, refusals (outputs untouched), autograd, and the old
  entry point's refusal of MIMO contexts."""
import functools

import numpy as np
import pytest

import solvempc_amd as sm

from test_mimo_sensitivity_ref import FAMILIES, N_RHS, TIE, _chain, _inputs, _refs
from test_sensitivity import _check_properties
from test_sensitivity_ref import _rel, _sens_exact

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_ORDER = sm._capi.MPCQ_ERR_ARG, sm._capi.MPCQ_ERR_ORDER


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")


class _Ctx:
    """A MIMO solver set up for a family, with the device arrays it reads kept alive."""

    def __init__(self, name, settings=None, B=None):
        import torch

        f = _inputs(name)
        B = f["Bd"].shape[0] if B is None else B
        _, nx, nu = f["Bd"].shape
        ny = np.asarray(f["sh"]["Cd"]).shape[0]
        N = f["N"]
        self.dims = (B, N, nx, nu, ny, N * nu, 2 * N * nu)
        self.keep = [_dev(f["Ad"][:B]), _dev(f["Bd"][:B])] + [
            _dev(np.broadcast_to(np.asarray(f["sh"][k], dtype=np.float64), (B,) + np.asarray(f["sh"][k]).shape).copy())
            for k in ("Cd", "Q", "R", "RD", "K", "K0", "w0")]
        self.s = sm.BatchSolver(N * nu, 2 * N * nu, B, n_plants=B, dtype="f64", settings=settings)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.s.mimo_setup_plants_device(nx, nu, ny, f["s_rows"], *[k.data_ptr() for k in self.keep], stream=self.stream)
        self.X, self.U0 = _dev(f["X"][:B]), _dev(f["U"][:B])
        self.yref = _dev(f["yref"]) if f["yref"] is not None else None

    def step(self, U=None):
        import torch

        U = self.U0.clone() if U is None else U
        self.s.mimo_step_device(self.X.data_ptr(), U.data_ptr(), self.yref.data_ptr() if self.yref is not None else 0,
                                self.stream)
        torch.cuda.synchronize()
        return U

    def vjp(self, g, n_rhs):
        """mimo_step_vjp_device on a host cotangent (or None): numpy (dX, dU, dyref, n_active)."""
        import torch

        B, N, nx, nu, ny, n, m = self.dims
        new = lambda k: torch.full((B, n_rhs, k), np.nan, dtype=torch.float64, device="cuda:0")
        dX, dU, dy = new(nx), new(nu), new(ny)
        na = torch.full((B,), -7, dtype=torch.int32, device="cuda:0")
        gd = _dev(g) if g is not None else None
        self.s.mimo_step_vjp_device(gd.data_ptr() if gd is not None else 0, n_rhs, dX.data_ptr(), dU.data_ptr(),
                                    dy.data_ptr(), na.data_ptr(), self.stream)
        torch.cuda.synchronize()
        return dX.cpu().numpy(), dU.cpu().numpy(), dy.cpu().numpy(), na.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _device(name):
    """One setup and step of a family and every call the tests compare, once per session."""
    c = _Ctx(name)
    B, N, nx, nu, ny, n, m = c.dims
    c.step()
    r = _refs(name)
    nr = 1 if nu == 1 else N_RHS
    g = r["g"][:, :nr]
    out = dict(c=c, g=g, nr=nr)
    out["st"], out["it"], _ = c.s.info()
    out["multi"] = c.s.mimo_sensitivity(g)
    out["multi2"] = c.s.mimo_sensitivity(g)
    out["single"] = [c.s.mimo_sensitivity(g[:, k]) for k in range(nr)]
    out["unit"] = c.s.mimo_sensitivity(None, nu)
    out["gains"] = c.s.mimo_step_gains()
    out["gains2"] = c.s.mimo_step_gains()
    eye = np.broadcast_to(np.eye(n)[:nu], (B, nu, n)).copy()
    out["vjp_unit"] = c.vjp(eye, nu)
    return out


def _dense(r):
    return np.stack([o["P"] for o in r["ops"]]), np.stack([o["A"] for o in r["ops"]])


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_exact_at_the_reported_set_and_properties(name):
    d, r = _device(name), _refs(name)
    B, N, nx, nu, ny, n, m = d["c"].dims
    gq, gu, na = d["multi"]
    st = d["st"]
    assert np.all(st == sm.SOLVED)  # (every QP of these families: none is left out below)
    supp = gu[:, 0] != 0
    assert np.array_equal(na, supp.sum(axis=1))
    for k in range(d["nr"]):
        assert np.array_equal(gu[:, k] != 0, supp), k
    P, A = _dense(r)
    worst = 0.0
    for b in range(B):
        for k in range(d["nr"]):
            ex = _sens_exact(P[b], A[b], np.zeros(m, bool), supp[b], d["g"][b, k])
            worst = max(worst, float(_rel(np.r_[gq[b, k], gu[b, k]], np.r_[ex[0], ex[2]])))
    print(f"{name}: device against _sens_exact at its own set {worst:.2e} (TOL {r['tol']:.1e}), n_active "
          f"{na.min()}..{na.max()}")
    assert worst <= r["tol"]
    for k in range(d["nr"]):
        _check_properties(P, A, d["g"][:, k], gq[:, k], np.zeros_like(gu[:, k]), gu[:, k], na, st, r["tol"])


def _clear(name, d, r):
    """QPs compared with the oracle side: same status and iteration count, rule margin >= TIE; the cap asserted."""
    assert np.array_equal(d["st"], r["st"])
    clear = (d["it"] == r["it"]) & (r["margin"] >= TIE)
    assert (~clear).sum() <= FAMILIES[name][1], (np.flatnonzero(~clear), FAMILIES[name][1])
    return clear


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_active_set_is_the_oracles(name):
    d, r = _device(name), _refs(name)
    clear = _clear(name, d, r)
    gq, gu, na = d["multi"]
    assert np.array_equal(na[clear], r["n_active"][clear])
    assert np.array_equal((gu[:, 0] != 0)[clear], r["upp"][clear])
    print(f"{name}: {int(clear.sum())} of {len(clear)} QPs compared with the oracle's set")


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_gains_and_vjp(name):
    d, r = _device(name), _refs(name)
    c = d["c"]
    B, N, nx, nu, ny, n, m = c.dims
    gq, gu, na = d["unit"]
    dX, dU, dy, na2 = d["gains"]
    assert np.array_equal(na, na2)
    clear = _clear(name, d, r)
    worst = worst_o = 0.0
    for b in range(B):
        for k in range(nu):
            own = np.r_[_chain(r["ops"][b], ny, gq[b, k], gu[b, k])]
            got = np.r_[dX[b, k], dU[b, k], dy[b, k]]
            worst = max(worst, float(_rel(got, own)))
            if clear[b]:
                ex = r["exact0"][b, k]
                worst_o = max(worst_o, float(_rel(got, np.r_[_chain(r["ops"][b], ny, ex[:n], ex[n:])])))
    print(f"{name}: gains against the chain of the device's own gq, gu {worst:.2e}; against the oracle side {worst_o:.2e}")
    # (the device's operators Fx, Fu, Frs come from its own condensing: they follow the oracle's to ~1e-13 relative,
    # tests/test_mimo.py; 1e-12 is the issue's bound for "the same sums")
    assert worst <= 1e-12
    assert worst_o <= r["tol"]
    for a, b_ in zip(d["gains"], d["vjp_unit"]):
        assert np.array_equal(a, b_)


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_deterministic_and_n_rhs_consistent(name):
    d = _device(name)
    for a, b in zip(d["multi"], d["multi2"]):
        assert np.array_equal(a, b)
    for a, b in zip(d["gains"], d["gains2"]):
        assert np.array_equal(a, b)
    gq, gu, na = d["multi"]
    for k in range(d["nr"]):
        gq1, gu1, na1 = d["single"][k]
        assert np.array_equal(gq1[:, 0], gq[:, k]) and np.array_equal(gu1[:, 0], gu[:, k]) and np.array_equal(na1, na)


@pytest.mark.parametrize("name", ["R", "Q"])
def test_read_only_on_a_warm_started_context(name):
    res = []
    for call in (False, True):
        c = _Ctx(name, settings=sm.default_settings(warm_start=1))
        U = c.step()
        if call:
            c.s.mimo_sensitivity(None, 1)
            c.s.mimo_step_gains()
        U = c.step(U)
        st, it, rho = c.s.info()
        res.append((U.cpu().numpy(), c.s.solution(), c.s.dual(), st, it, rho))
    for a, b in zip(*res):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("max_iter", [15, 100])
def test_unsolved_qps_get_zeros(max_iter):
    """Family Q with max_iter = 15: every QP ends MAX_ITER_REACHED or SOLVED_INACCURATE (the oracle: 5 and 19), none
    SOLVED, and all get zeros and -1.  max_iter = 100 mixes SOLVED QPs (the oracle: 8) with SOLVED_INACCURATE ones:
    the unsolved get zeros and -1, the others are still correct at their own set."""
    name = "Q"
    c = _Ctx(name, settings=sm.default_settings(max_iter=max_iter))
    B, N, nx, nu, ny, n, m = c.dims
    c.step()
    st, it, _ = c.s.info()
    r = _refs(name)
    g = r["g"][:, :1]
    gq, gu, na = c.s.mimo_sensitivity(g)
    dX, dU, dy, na2 = c.s.mimo_step_gains()
    bad = st != sm.SOLVED
    print(f"max_iter {max_iter}: statuses {sorted(set(st.tolist()))}, {int(bad.sum())} of {B} QPs did not end SOLVED")
    if max_iter == 15:
        assert (st == sm.MAX_ITER_REACHED).any() and bad.all()
    else:
        assert bad.any() and (~bad).any()
    assert np.all(na[bad] == -1) and np.all(na2[bad] == -1) and np.all(na[~bad] >= 0) and np.all(na2[~bad] >= 0)
    for a in (gq, gu, dX, dU, dy):
        assert np.all(a[bad] == 0)
    P, A = _dense(r)
    worst = 0.0
    for b in np.flatnonzero(~bad):
        supp = gu[b, 0] != 0
        assert na[b] == supp.sum()
        ex = _sens_exact(P[b], A[b], np.zeros(m, bool), supp, g[b, 0])
        worst = max(worst, float(_rel(np.r_[gq[b, 0], gu[b, 0]], np.r_[ex[0], ex[2]])))
    assert worst <= r["tol"], worst


def _rc(fn, *args):
    with pytest.raises(sm.MpcqError) as e:
        fn(*args)
    return e.value.code


def test_refusals_write_nothing():
    import torch

    c = _Ctx("R")
    B, N, nx, nu, ny, n, m = c.dims
    sent = lambda *shape: torch.full(shape, 12345.0, dtype=torch.float64, device="cuda:0")
    gq, gu, dX, dU, dy = sent(B, 4, n), sent(B, 4, m), sent(B, 4, nx), sent(B, 4, nu), sent(B, 4, ny)
    na = torch.full((B,), 77, dtype=torch.int32, device="cuda:0")
    g = sent(B, 4, n)
    s, p = c.s, lambda t: t.data_ptr()
    # no step since the setup
    assert _rc(s.mimo_sensitivity_device, 0, 1, p(gq), p(gu), p(na), c.stream) == ERR_ORDER
    assert _rc(s.mimo_step_vjp_device, p(g), 1, p(dX), p(dU), p(dy), p(na), c.stream) == ERR_ORDER
    assert _rc(s.mimo_step_gains_device, p(dX), p(dU), p(dy), p(na), c.stream) == ERR_ORDER
    # no MIMO setup at all
    with sm.BatchSolver(n, m, B, n_plants=B) as fresh:
        assert _rc(fresh.mimo_sensitivity_device, 0, 1, p(gq), p(gu), p(na), c.stream) == ERR_ORDER
    c.step()
    for bad in (0, 5, -1):
        assert _rc(s.mimo_sensitivity_device, p(g), bad, p(gq), p(gu), p(na), c.stream) == ERR_ARG
        assert _rc(s.mimo_step_vjp_device, p(g), bad, p(dX), p(dU), p(dy), p(na), c.stream) == ERR_ARG
    assert _rc(s.mimo_sensitivity_device, 0, nu + 1, p(gq), p(gu), p(na), c.stream) == ERR_ARG  # NULL g, n_rhs > n_u
    assert _rc(s.mimo_step_vjp_device, 0, nu + 1, p(dX), p(dU), p(dy), p(na), c.stream) == ERR_ARG
    assert _rc(s.mimo_sensitivity_device, p(g), 1, 0, 0, 0, c.stream) == ERR_ARG                # every output NULL
    assert _rc(s.mimo_step_vjp_device, p(g), 1, 0, 0, 0, 0, c.stream) == ERR_ARG
    assert _rc(s.mimo_step_gains_device, 0, 0, 0, 0, c.stream) == ERR_ARG
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):  # refused, nothing recorded
        assert _rc(s.mimo_sensitivity_device, p(g), 1, p(gq), p(gu), p(na), side.cuda_stream) == ERR_ARG
        assert _rc(s.mimo_step_gains_device, p(dX), p(dU), p(dy), p(na), side.cuda_stream) == ERR_ARG
    torch.cuda.synchronize()
    for t in (gq, gu, dX, dU, dy):
        assert bool((t == 12345.0).all())
    assert bool((na == 77).all())
    # and the context still serves a call afterwards
    s.mimo_sensitivity_device(0, 1, p(gq), p(gu), p(na), c.stream)
    torch.cuda.synchronize()
    assert bool((na >= 0).all())


def test_old_entry_points_still_refuse_mimo_contexts():
    import torch

    c = _Ctx("R")
    B, N, nx, nu, ny, n, m = c.dims
    c.step()
    gq = torch.zeros(B, n, dtype=torch.float64, device="cuda:0")
    assert _rc(c.s.sensitivity_device, 0, gq.data_ptr(), 0, 0, 0, c.stream) == ERR_ARG
    assert _rc(c.s.mpc_step_gains_device, gq.data_ptr(), 0, 0, 0, c.stream) == ERR_ARG


def test_autograd_mimo_solution():
    import torch

    from solvempc_amd import diff

    c = _Ctx("R")
    B, N, nx, nu, ny, n, m = c.dims
    X = c.X.clone().requires_grad_(True)
    U = c.U0.clone().requires_grad_(True)
    yref = c.yref.clone().requires_grad_(True)
    x, status = diff.mimo_solution(c.s, X, U, yref)
    assert bool((status == sm.SOLVED).all()) and not status.requires_grad
    w = _dev(np.random.default_rng(7).normal(size=(B, n)))
    gX, gU, gy = torch.autograd.grad((x * w).sum(), (X, U, yref), retain_graph=True)
    dX, dU, dy, na = c.vjp(w.cpu().numpy()[:, None, :], 1)
    assert np.array_equal(gX.cpu().numpy(), dX[:, 0]) and np.array_equal(gU.cpu().numpy(), dU[:, 0])
    ysum = dy[:, 0].sum(axis=0)  # (the batch sum: another order than torch's, so not bit for bit)
    np.testing.assert_allclose(gy.cpu().numpy(), ysum, rtol=0, atol=1e-12 * max(1.0, float(np.abs(dy).sum(axis=0).max())))
    assert torch.equal(U.detach(), c.U0)  # the caller's U is left alone
    c.step()
    with pytest.raises(RuntimeError, match="solved again"):
        torch.autograd.grad((x * w).sum(), (X, U, yref))

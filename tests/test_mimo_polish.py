"""MIMO polish on the device (mpcq_mimo_step_polish_device; solvempc_amd/csrc/mpcq_mimo_polish.hip)
against the CPU references of tests/test_mimo_polish_ref.py, on that file's families and settings.

A QP is "clear" when its device iteration count equals the oracle's (tests/test_mimo.py's termination tie), its rule
margin is at least TIE and its success decision's margin at least DEC; at most CAP[family] QPs may be unclear
(asserted; the CPU file shows that the reference alone excludes none).  Every (family, setting) runs three contexts
once per session (``_run``): a polished one, a second polished one on equal inputs, and a twin that runs the plain
``mimo_step_device``; each then takes one more plain step from the state and the U it was left with.

Measured on the device: the figures each test prints; none of the bounds below was taken from them."""
import functools

import numpy as np
import pytest

import oracle
import solvempc_amd as sm

from test_mimo_polish_ref import ALL, CAP, DEC, SETTINGS, TIE, _family_inputs, _prefs
from test_mimo_sensitivity_ref import FAMILIES
from test_polish import EPS, _rel_err, _residuals, _sym
from test_sensitivity_ref import _cotangents, _rel, _sens_exact

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_ORDER = sm._capi.MPCQ_ERR_ARG, sm._capi.MPCQ_ERR_ORDER
RESULT_KEYS = ("x", "y", "st", "it", "rho", "U")


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")


class _Ctx:
    """A MIMO solver set up for a family, with the device arrays it reads kept alive."""

    def __init__(self, name, **settings):
        import torch

        f = _family_inputs(name)
        B, nx, nu = f["Bd"].shape
        ny = np.asarray(f["sh"]["Cd"]).shape[0]
        N = f["N"]
        self.dims = (B, N, nx, nu, ny, N * nu, 2 * N * nu)
        self.keep = [_dev(f["Ad"]), _dev(f["Bd"])] + [
            _dev(np.broadcast_to(np.asarray(f["sh"][k], dtype=np.float64), (B,) + np.asarray(f["sh"][k]).shape).copy())
            for k in ("Cd", "Q", "R", "RD", "K", "K0", "w0")]
        self.s = sm.BatchSolver(N * nu, 2 * N * nu, B, n_plants=B, dtype="f64", settings=sm.default_settings(**settings))
        self.stream = torch.cuda.current_stream().cuda_stream
        self.s.mimo_setup_plants_device(nx, nu, ny, f["s_rows"], *[k.data_ptr() for k in self.keep], stream=self.stream)
        self.X, self.U = _dev(f["X"]), _dev(f["U"])
        self.yref = _dev(f["yref"]) if f["yref"] is not None else None

    def step(self, polish):
        """One step on the context's own U (evolving); the results as numpy."""
        import torch

        fn = self.s.mimo_step_polish_device if polish else self.s.mimo_step_device
        fn(self.X.data_ptr(), self.U.data_ptr(), self.yref.data_ptr() if self.yref is not None else 0, self.stream)
        torch.cuda.synchronize()
        r = dict(x=self.s.solution(), y=self.s.dual(), U=self.U.cpu().numpy())
        r["st"], r["it"], r["rho"] = self.s.info()
        r["sp"], r["na"], r["pri"], r["dua"] = self.s.polish_info()
        return r


@functools.lru_cache(maxsize=None)
def _run(name, setting):
    """{p, p2: the polished step on two contexts; w: the twin's plain step; sens: mimo_sensitivity after p's polished
    step; p_next, w_next: a plain step after each; U0}."""
    out = {}
    ctxs = {k: _Ctx(name, **SETTINGS[setting]) for k in ("p", "p2", "w")}
    out["U0"] = ctxs["p"].U.cpu().numpy()
    for k, c in ctxs.items():
        out[k] = c.step(polish=k != "w")
    c = ctxs["p"]
    B, N, nx, nu, ny, n, m = c.dims
    if name in FAMILIES:
        out["g"] = _cotangents(17, B, n).reshape(B, 1, n)
        out["sens"] = c.s.mimo_sensitivity(out["g"])
    out["p_next"] = c.step(polish=False)
    out["w_next"] = ctxs["w"].step(polish=False)
    out["dims"] = c.dims
    for c in ctxs.values():
        c.s.close()
    return out


def _clear(name, d, r):
    assert np.array_equal(d["p"]["st"], r["st"])
    clear = (d["p"]["it"] == r["it"]) & (r["margin"] >= TIE) & (r["dec"] >= DEC)
    assert (~clear).sum() <= CAP[name], (np.flatnonzero(~clear), CAP[name])
    return clear


def _same_rows(a, b, rows, keys=RESULT_KEYS):
    for k in keys:
        assert np.array_equal(a[k][rows], b[k][rows], equal_nan=True), k


def _info_residuals(r, b, x, y):
    """numpy's residuals of a returned (x, y) of QP b with z = min(A^ x^ + y^, u^), and the rounded-dot-product floor
    of each: 2 (n + m + 1) eps x the largest row sum of absolute terms (two summation orders at this shape)."""
    ops, D, E, c = r["ops"][b], r["D"][b], r["E"][b], r["c"][b]
    n, m = len(D), len(E)
    Ph = c * D[:, None] * _sym(np.asarray(ops["P"]).reshape(n, n)) * D[None, :]
    Ah = E[:, None] * np.asarray(ops["A"]).reshape(m, n) * D[None, :]
    xh, yh, qh, uh = x / D, c * y / E, c * D * r["q"][b], E * r["u"][b]
    zh = np.minimum(Ah @ xh + yh, uh)
    pri, dua = _residuals(Ph, Ah, qh, D, E, c, xh, zh, yh)
    k = 2 * (n + m + 1) * EPS
    fl_p = k * ((np.abs(Ah) @ np.abs(xh) + np.abs(zh)) / E).max()
    fl_d = k * ((np.abs(Ph) @ np.abs(xh) + np.abs(qh) + np.abs(Ah).T @ np.abs(yh)) / D / c).max()
    return pri, dua, fl_p, fl_d


# ----------------------------------------------------------------------------- 1. tight
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_tight_reaches_the_optimum(name):
    d, r = _run(name, "tight"), _prefs(name, "tight")
    B, N, nx, nu, ny, n, m = d["dims"]
    p = d["p"]
    clear = _clear(name, d, r)
    assert np.all(p["st"] == sm.SOLVED) and np.all(p["sp"] == 1)
    err = _rel_err(p["x"], r["x_opt"])
    kkt = np.empty(B)
    worst_p = worst_d = 0.0
    for b in range(B):
        ops = r["ops"][b]
        res = oracle.kkt_residuals(ops["P"], r["q"][b], ops["A"], r["l"], r["u"][b], p["x"][b], p["y"][b])
        kkt[b] = max(res.values()) / max(1.0, float(np.abs(p["x"][b]).max()), float(np.abs(r["q"][b]).max()))
        pri, dua, fl_p, fl_d = _info_residuals(r, b, p["x"][b], p["y"][b])
        worst_p, worst_d = max(worst_p, abs(p["pri"][b] - pri)), max(worst_d, abs(p["dua"][b] - dua))
        assert abs(p["pri"][b] - pri) <= 1e-6 * pri + fl_p, (b, p["pri"][b], pri, fl_p)
        assert abs(p["dua"][b] - dua) <= 1e-6 * dua + fl_d, (b, p["dua"][b], dua, fl_d)
    print(f"{name} / tight: polished x against _optimum {err.max():.2e} (TOL {r['tol']:.1e}; the plain step "
          f"{_rel_err(d['w']['x'], r['x_opt']).max():.2e}), KKT {kkt.max():.2e}, n_active {p['na'].min()}..{p['na'].max()}, "
          f"polish_info residuals up to {p['pri'].max():.1e} / {p['dua'].max():.1e} (off numpy's by {worst_p:.1e} / "
          f"{worst_d:.1e}), {int(clear.sum())} of {B} clear")
    assert err.max() <= r["tol"]
    assert kkt.max() <= 1e-9
    assert np.array_equal(p["na"][clear], r["n_active"][clear])
    assert np.array_equal((p["y"] > 0)[clear], (r["y"] > 0)[clear])


# ----------------------------------------------------------------------------- 2. default, 3. the applied move
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_default_follows_the_reference_and_keeps_the_rest(name):
    d, r = _run(name, "default"), _prefs(name, "default")
    p, w = d["p"], d["w"]
    clear = _clear(name, d, r)
    assert np.array_equal(p["sp"][clear], r["status"][clear])
    assert np.array_equal(p["na"][clear], r["n_active"][clear])
    ok = p["sp"] == 1
    both = ok & clear & (r["status"] == 1)
    err = _rel_err(p["x"][both], r["x"][both]).max(initial=0.0)
    print(f"{name} / default: {int(ok.sum())} of {len(ok)} polished, {int((p['sp'] == -1).sum())} unsuccessful, polished x "
          f"against _polish_ref {err:.2e}, {int(clear.sum())} clear")
    assert err <= 1e-9
    for k in ("st", "it", "rho"):  # always the ADMM's
        assert np.array_equal(p[k], w[k]), k
    _same_rows(p, w, ~ok)
    _same_rows(d["p_next"], d["w_next"], ~ok)
    if name in ("R", "Q", "Q-tight"):
        assert (~ok).any()


@pytest.mark.parametrize("setting", ["tight", "default"])
@pytest.mark.parametrize("name", ALL)
def test_applied_move(name, setting):
    d = _run(name, setting)
    B, N, nx, nu, ny, n, m = d["dims"]
    p, w = d["p"], d["w"]
    ok = p["sp"] == 1
    assert np.array_equal(p["U"][ok], (d["U0"] + p["x"][:, :nu])[ok])
    assert np.array_equal(p["U"][~ok], w["U"][~ok])
    solved = w["st"] == sm.SOLVED
    assert np.array_equal(w["U"][solved], (d["U0"] + w["x"][:, :nu])[solved])  # (the plain step's own move)


# ----------------------------------------------------------------------------- 4. more than n active rows
def test_more_than_n_active_rows_are_reported_and_kept():
    """R-pinned's pinned rows sit at the rule's tie (tests/test_mimo_polish_ref.py), so the count is the device's own:
    such a QP is compared with the twin only."""
    d = _run("R-pinned", "default")
    B, N, nx, nu, ny, n, m = d["dims"]
    p, w = d["p"], d["w"]
    assert np.all(p["st"] == sm.SOLVED)
    over = p["na"] > n
    print(f"R-pinned: {int(over.sum())} of {B} QPs above n = {n} active rows (up to {p['na'].max()})")
    assert over.sum() >= 1 and np.all(p["sp"][over] == -1)
    _same_rows(p, w, over)
    _same_rows(d["p_next"], d["w_next"], over)
    # (the ADMM iterate's residuals, as the unsuccessful case reports them: met the step's termination test)
    assert np.all(np.isfinite(p["pri"][over])) and np.all(np.isfinite(p["dua"][over]))


# ----------------------------------------------------------------------------- 5. warm start
@pytest.mark.parametrize("name", ["S", "R-tight", "Q"])
def test_next_step_is_warm_started_from_the_polished_point(name):
    """The plain step after the polished one follows an oracle.Solver that solved the first step, took
    warm_start(x_pol, y_pol) where polish succeeded (OSQP replaces work->x, z, y; elsewhere its own iterate stays),
    then the evolved U's q and u."""
    d, r = _run(name, "default"), _prefs(name, "default")
    B, N, nx, nu, ny, n, m = d["dims"]
    f, p, nxt = r["inputs"], d["p"], d["p_next"]
    unclear, worst = 0, 0.0
    for b in range(B):
        ops = r["ops"][b]
        o = oracle.Solver(ops["P"], np.zeros(n), ops["A"], r["l"], ops["W0"])
        assert o.update_gradient(r["q"][b]) and o.update_upper_bound(r["u"][b])
        assert o.solve() == p["st"][b]
        if o.info().iter != p["it"][b]:
            unclear += 1
            continue
        if p["sp"][b] == 1:
            o.warm_start(p["x"][b], p["y"][b])
        assert o.update_gradient(oracle.mimo_gradient(ops, f["X"][b], p["U"][b], f["yref"]))
        assert o.update_upper_bound(oracle.mimo_upper_bound(ops, f["X"][b], p["U"][b]))
        st = o.solve()
        info = o.info()
        if info.margin < 1e-6:
            unclear += 1
            continue
        assert (st, info.iter) == (nxt["st"][b], nxt["it"][b]), (b, st, info.iter, nxt["st"][b], nxt["it"][b])
        worst = max(worst, float(_rel_err(nxt["x"][b], o.x())))
    print(f"{name}: next step against the warm-started oracle {worst:.2e}, {unclear} of {B} QPs not compared")
    assert unclear <= CAP[name]
    assert worst <= 1e-7


# ----------------------------------------------------------------------------- 6. sensitivities follow
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_sensitivities_read_the_polished_iterate(name):
    from test_mimo_sensitivity_ref import _refs

    d = _run(name, "tight")
    r = _prefs(name, "tight")
    B, N, nx, nu, ny, n, m = d["dims"]
    tol = _refs(name)["tol"]
    gq, gu, na = d["sens"]
    supp = d["p"]["y"] > 0
    assert np.array_equal(gu[:, 0] != 0, supp)
    assert np.array_equal(na, supp.sum(axis=1))
    worst = 0.0
    for b in range(B):
        ops = r["ops"][b]
        ex = _sens_exact(ops["P"], ops["A"], np.zeros(m, bool), supp[b], d["g"][b, 0])
        worst = max(worst, float(_rel(np.r_[gq[b, 0], gu[b, 0]], np.r_[ex[0], ex[2]])))
    print(f"{name}: sensitivities after the polished step against _sens_exact at dual() > 0: {worst:.2e} (TOL {tol:.1e})")
    assert worst <= tol


# ----------------------------------------------------------------------------- 7. other properties
@pytest.mark.parametrize("setting", ["tight", "default"])
@pytest.mark.parametrize("name", ALL)
def test_deterministic_and_plain_step_clears_the_info(name, setting):
    d = _run(name, setting)
    for k in RESULT_KEYS + ("sp", "na", "pri", "dua"):
        assert np.array_equal(d["p"][k], d["p2"][k], equal_nan=True), k
    for r in (d["w"], d["p_next"], d["w_next"]):  # "not performed"
        assert np.all(r["sp"] == 0) and np.all(r["na"] == 0)
        assert np.all(np.isnan(r["pri"])) and np.all(np.isnan(r["dua"]))


def test_no_solved_qp_means_nothing_is_polished():
    p, w = _Ctx("Q", max_iter=15), _Ctx("Q", max_iter=15)
    rp, rw = p.step(polish=True), w.step(polish=False)
    assert not (rp["st"] == sm.SOLVED).any()
    assert np.all(rp["sp"] == 0) and np.all(rp["na"] == 0)
    assert np.all(np.isnan(rp["pri"])) and np.all(np.isnan(rp["dua"]))
    _same_rows(rp, rw, slice(None))
    _same_rows(p.step(polish=False), w.step(polish=False), slice(None))
    p.s.close()
    w.s.close()


def _rc(fn, *args):
    with pytest.raises(sm.MpcqError) as e:
        fn(*args)
    return e.value.code


def test_refusals_write_nothing():
    import torch

    c = _Ctx("R")
    B, N, nx, nu, ny, n, m = c.dims
    U0 = c.U.cpu().numpy()
    X, U, y = c.X.data_ptr(), c.U.data_ptr(), c.yref.data_ptr()
    with sm.BatchSolver(n, m, B, n_plants=B) as fresh:  # no MIMO setup
        assert _rc(fresh.mimo_step_polish_device, X, U, y, c.stream) == ERR_ORDER
    assert _rc(c.s.mimo_step_polish_device, 0, U, y, c.stream) == ERR_ARG
    assert _rc(c.s.mimo_step_polish_device, X, 0, y, c.stream) == ERR_ARG
    with sm.BatchSolver(16, 32, B, n_plants=B, settings=sm.default_settings(polish=1)) as on:
        with pytest.raises(sm.MpcqError) as e:
            on.mimo_step_polish_device(X, U, y, c.stream)
        assert e.value.code == ERR_ARG and "polish" in str(e.value)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):  # refused, nothing recorded
        assert _rc(c.s.mimo_step_polish_device, X, U, y, side.cuda_stream) == ERR_ARG
    torch.cuda.synchronize()
    assert np.array_equal(c.U.cpu().numpy(), U0)
    sp = c.s.polish_info()[0]
    assert np.all(sp == 0)
    r = c.step(polish=True)  # and the context still serves a call afterwards
    assert np.all(r["sp"] != 0) and np.array_equal(r["sp"], _run("R", "default")["p"]["sp"])
    c.s.close()


def test_autograd_mimo_solution_polished():
    import torch

    from solvempc_amd import diff

    d = _run("R", "tight")
    c = _Ctx("R", **SETTINGS["tight"])
    B, N, nx, nu, ny, n, m = c.dims
    X = c.X.clone().requires_grad_(True)
    U = c.U.clone().requires_grad_(True)
    yref = c.yref.clone().requires_grad_(True)
    x, status = diff.mimo_solution(c.s, X, U, yref, polish=True)
    assert bool((status == sm.SOLVED).all())
    assert np.array_equal(x.detach().cpu().numpy(), d["p"]["x"])  # the polished x
    assert np.all(c.s.polish_info()[0] == 1)
    w = _dev(np.random.default_rng(7).normal(size=(B, n)))
    gX, gU, gy = torch.autograd.grad((x * w).sum(), (X, U, yref))
    new = lambda k: torch.full((B, 1, k), np.nan, dtype=torch.float64, device="cuda:0")
    dX, dU, dy = new(nx), new(nu), new(ny)
    c.s.mimo_step_vjp_device(w.data_ptr(), 1, dX.data_ptr(), dU.data_ptr(), dy.data_ptr(), 0, c.stream)
    torch.cuda.synchronize()
    assert torch.equal(gX, dX[:, 0]) and torch.equal(gU, dU[:, 0])
    assert torch.equal(gy, dy[:, 0].sum(dim=0))
    assert torch.equal(U.detach(), c.U)  # the caller's U is left alone
    c.s.close()

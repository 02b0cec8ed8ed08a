"""Per-QP reference trajectories with horizon preview (mpcq_mpc_step_ref*, mpcq_mpc_run_ref_device):

    q_b = Fx X_b + Fu U_b + Fr ref_b,   ref_b in R^N (one controllerStep), or the window
    ref_b[j] = sched_b[min(s + j, len - 1)] of a schedule at control step s (a stream).

Inputs (``_inputs``): the config-2 states ``workload.mpc_states(1, 0, .)`` and, per QP, a set-point step of
its own size at its own point of the horizon, drawn once for 65,536 QPs (``default_rng(7)``); a test takes the
first B.  The oracle's q is formed in numpy and solved by ``oracle.batch_solve`` / ``oracle.Solver``.

Bars: fp64 against the oracle as tests/test_gpu.py (status, iterations, rho 1e-9 relative, x and the applied
move 1e-9); fp32 its ``F32_TOL`` bar with the tie rule; mixed its ``_mixed_parity`` bar.  A uniform reference
must reproduce the scalar entry point bit for bit on every path and dtype (same expression form).
The helpers are restated from tests/test_gpu.py.
"""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import _capi, workload

ROOT = Path(__file__).resolve().parents[1]
LMIN = -np.finfo(np.float64).max
F32_TOL = 1e-5
TIE_MARGIN = 2e-3
MIXED_TOL = 1e-5
MIXED_OFF_SCHEDULE = 1e-4
NEW = ("mpcq_mpc_step_ref_device", "mpcq_mpc_step_ref", "mpcq_mpc_run_ref_device")
DTYPES = ["f64", "f32", "mixed"]


# ---- 1. CPU: the surface exists (fails on the parent) ----------------------------------------------
def test_symbols_declared_exported_and_bound():
    hdr = (ROOT / "include" / "mpcq.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mpcq_[a-z_0-9]+)\s*\(", hdr))
    lib = sm.lib()
    for name in NEW:
        assert name in declared, name
        assert name in _capi.EXPORTS, name
        f = getattr(lib, name)
        assert f.restype is C.c_int and f.argtypes, name  # bound with a prototype
    assert len(lib.mpcq_mpc_step_ref_device.argtypes) == 6
    assert len(lib.mpcq_mpc_step_ref.argtypes) == 5
    assert len(lib.mpcq_mpc_run_ref_device.argtypes) == 12
    for meth in ("mpc_step_ref", "mpc_step_ref_device", "mpc_run_ref_device"):
        assert callable(getattr(sm.BatchSolver, meth))
    assert callable(getattr(sm.ModelPredictiveControlAPI, "setRefTrajectory"))


# ---- helpers (restated from tests/test_gpu.py) -----------------------------------------------------
class _DevArray:
    def __init__(self, ptr, shape, typestr="<f8"):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3}


@pytest.fixture(params=["tile", "wave", "lane"])
def kernel(request, monkeypatch):
    monkeypatch.setenv("MPCQ_KERNEL", request.param)
    return request.param


def _osqp_terminated(x, y, q, u, ops, slack=1.5):
    Ax = x @ ops["A"].T
    prim = np.maximum(Ax - u, 0).max(axis=1)
    tol_p = 1e-3 + 1e-3 * np.maximum(np.abs(Ax).max(axis=1), np.abs(u).max(axis=1))
    assert np.all(prim <= slack * tol_p)
    Px, Aty = x @ ops["P"], y @ ops["A"]
    dual = np.abs(Px + q + Aty).max(axis=1)
    tol_d = 1e-3 + 1e-3 * np.maximum(np.abs(q).max(axis=1), np.maximum(np.abs(Aty).max(axis=1), np.abs(Px).max(axis=1)))
    assert np.all(dual <= slack * tol_d)


def _f32_close(x, x_ref, what=""):
    scale = np.maximum(1.0, np.abs(x_ref).max(axis=1))
    e0 = np.abs(x[:, 0] - x_ref[:, 0]) / scale
    ev = np.abs(x - x_ref).max(axis=1) / scale
    print(f"{what}: fp32 max rel |dx0| {e0.max():.2e}, |dx| {ev.max():.2e}")
    assert e0.max() < F32_TOL and ev.max() < F32_TOL, (what, e0.max(), ev.max(), int(np.argmax(ev)))


def _f32_parity(s, x, st, it, x_ref, st_ref, it_ref, margin, q, u, ops, what=""):
    assert np.array_equal(st, st_ref), what
    tie = margin < TIE_MARGIN
    off = it != it_ref
    assert not np.any(off & ~tie), (what, np.flatnonzero(off & ~tie)[:8], margin[off & ~tie][:8])
    _f32_close(x[~off], x_ref[~off], what)
    if off.any():
        _osqp_terminated(x[off], s.dual()[off], q[off], u[off], ops)
    return int(off.sum())


def _mixed_parity(x, y, st, it, x_ref, st_ref, it_ref, q, u, ops, what=""):
    assert np.array_equal(st, st_ref), what
    off = it != it_ref
    e0 = np.abs(x[:, 0] - x_ref[:, 0])
    print(f"{what}: mixed max |dx0| {e0.max():.2e}, {int(off.sum())} QPs off the oracle's schedule")
    assert off.mean() <= MIXED_OFF_SCHEDULE, (what, int(off.sum()))
    assert e0.max() < MIXED_TOL, (what, e0.max(), int(np.argmax(e0)))
    ev = np.abs(x - x_ref).max(axis=1) / np.maximum(1.0, np.abs(x_ref).max(axis=1))
    assert ev[~off].max() < MIXED_TOL, (what, ev[~off].max())
    if off.any():
        _osqp_terminated(x[off], y[off], q[off], u[off], ops)


def _order_bin(v):
    a = np.abs(v)
    out = np.full(a.shape, 511, dtype=np.int64)
    fin = np.isfinite(a)
    f, e = np.frexp(a[fin])
    i = np.clip((e - 1) * 16 + ((f - 0.5) * 32.0).astype(np.int64) + 256, 0, 510)
    out[fin] = np.where(a[fin] == 0.0, 0, i)
    return out


# ---- inputs and oracle references, computed once ---------------------------------------------------
_CACHE = {}


def _ops(plant, N):
    if ("ops", N) not in _CACHE:
        _CACHE["ops", N] = oracle.condense(plant, N)
    return _CACHE["ops", N]


def _inputs(N, B):
    """X, U, ref of the first B of the 65,536 QPs: a set-point step of a per-QP size at a per-QP point."""
    if ("in", N) not in _CACHE:
        full = 65536
        X, U = workload.mpc_states(1, 0, full)
        rng = np.random.default_rng(7)
        lvl = rng.uniform(-5, 5, (full, 1))
        ref = lvl * (np.arange(N) >= rng.integers(0, N, (full, 1)))
        _CACHE["in", N] = (X, U, ref)
    X, U, ref = _CACHE["in", N]
    return X[:B].copy(), U[:B].copy(), ref[:B].copy()


def _qu(ops, X, U, ref):
    q = X @ ops["Fx"].T + U[:, None] * ops["Fu"] + ref @ ops["Fr"].T
    return q, oracle.upper_bound(ops, X, U)


def _u0(ops):
    return oracle.upper_bound(ops, np.zeros(4), 0.0)


def _oracle(plant, N, B):
    """(q, u, x, status, iter, rho, margin) of the oracle on the first B inputs, cold."""
    if ("ora", N, B) not in _CACHE:
        ops = _ops(plant, N)
        X, U, ref = _inputs(N, B)
        q, u = _qu(ops, X, U, ref)
        x, st, it, rho, mg = oracle.batch_solve(ops["P"], ops["A"], np.zeros(N), np.full(2 * N, LMIN), _u0(ops), q, u,
                                                margins=True)
        _CACHE["ora", N, B] = (q, u, x, st, it, rho, mg)
    return _CACHE["ora", N, B]


def _ctx(ops, N, B, dtype="f64", settings=None, operators=True):
    s = sm.BatchSolver(N, 2 * N, B, dtype=dtype, settings=settings)
    s.setup(ops["P"], np.zeros(N), ops["A"], np.full(2 * N, LMIN), _u0(ops))
    if operators:
        s.mpc_set_operators(ops["Fx"], ops["Fu"], ops["Fr"], ops["Sbar"], ops["Ku"], ops["W0"])
    return s


def _outputs(s, U):
    return (U, s.solution(), s.dual(), *s.info())


def _schedules(B, L, seed=11):
    """Per-QP schedules of L values: a set-point step of a per-QP size at a per-QP step."""
    rng = np.random.default_rng(seed)
    lvl = rng.uniform(-5, 5, (B, 1))
    return lvl * (np.arange(L) >= rng.integers(0, L, (B, 1)))


def _window(sched, s, N):
    """ref_b[j] = sched_b[min(s + j, L - 1)]"""
    return sched[:, np.minimum(s + np.arange(N), sched.shape[1] - 1)]


# ---- 2. a uniform reference is the scalar path, bit for bit ----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", [20, 15])
@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform_reference_is_the_scalar_path(plant, kernel, dtype, N):
    B = 512
    ops = _ops(plant, N)
    X, U, _ = _inputs(N, B)
    X2 = X * 1.01  # the second, warm-started step's states
    runs = []
    for form in ("scalar", "per_qp", "shared"):
        s = _ctx(ops, N, B, dtype)
        assert s.path()[0] == kernel
        outs, Uk = [], U
        for Xk in (X, X2):
            if form == "scalar":
                Uk = s.mpc_step(Xk, Uk, 0.7)
            elif form == "per_qp":
                Uk = s.mpc_step_ref(Xk, Uk, np.full((B, N), 0.7))
            else:
                Uk = s.mpc_step_ref(Xk, Uk, np.full(N, 0.7))
            outs.append(_outputs(s, Uk))
        s.close()
        runs.append(outs)
    for form, outs in zip(("per_qp", "shared"), runs[1:]):
        for step in range(2):
            for name, a, b in zip(("U", "x", "y", "status", "iter", "rho"), runs[0][step], outs[step]):
                assert np.array_equal(a, b, equal_nan=True), (form, step, name)


# ---- 3. per-QP references against the oracle, one cold step, every kernel --------------------------
def _device_step(s, X, U, ref, B, N):
    """One mpc_step_ref_device on torch buffers; the reference buffer is overwritten with NaN after the
    solve, then the device view's q is read.  Returns (U, q_view)."""
    import torch
    Xd, Ud = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(U.copy()).cuda()
    Rd = torch.from_numpy(ref.copy()).cuda()
    s.mpc_step_ref_device(Xd.data_ptr(), Ud.data_ptr(), Rd.data_ptr(), N)
    torch.cuda.synchronize()
    Rd.fill_(float("nan"))
    torch.cuda.synchronize()
    v = s.device_view()
    torch.cuda.synchronize()
    qd = torch.as_tensor(_DevArray(v["q"], (B, N)), device="cuda").cpu().numpy().copy()
    return Ud.cpu().numpy(), qd


@pytest.mark.gpu
@pytest.mark.parametrize("N", [20, 15])
def test_per_qp_reference_f64_matches_oracle(plant, kernel, N):
    B = 512
    ops = _ops(plant, N)
    X, U, ref = _inputs(N, B)
    q, u, x_ref, st_ref, it_ref, rho_ref, _ = _oracle(plant, N, B)
    assert np.all(st_ref == oracle.SOLVED)
    s = _ctx(ops, N, B)
    Ug, qd = _device_step(s, X, U, ref, B, N)
    assert s.path()[0] == kernel
    if kernel == "tile":
        assert s.order()[0]  # the ordered single launch
    x, (st, it, rho) = s.solution(), s.info()
    assert np.array_equal(st, st_ref) and np.array_equal(it, it_ref)
    np.testing.assert_allclose(rho, rho_ref, rtol=1e-9)
    print(f"f64 {kernel} N={N}: max |x - x_oracle| {np.abs(x - x_ref).max():.2e}")
    assert np.abs(x - x_ref).max() < 1e-9
    np.testing.assert_allclose(Ug, U + x_ref[:, 0], rtol=0, atol=1e-9)
    # q was written for good: the caller's buffer is NaN by now
    assert np.all(np.abs(qd - q) <= 1e-12 * np.maximum(1.0, np.abs(q)))
    # and a following generic solve sees that q: from the post-setup state it is the oracle's cold solve again
    s.reset_state()
    s.solve()
    st2, it2, _ = s.info()
    assert np.array_equal(st2, st_ref) and np.array_equal(it2, it_ref)
    assert np.abs(s.solution() - x_ref).max() < 1e-9
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [20, 15])
def test_per_qp_reference_f32_matches_oracle(plant, kernel, N):
    B = 512
    ops = _ops(plant, N)
    X, U, ref = _inputs(N, B)
    q, u, x_ref, st_ref, it_ref, _, margin = _oracle(plant, N, B)
    s = _ctx(ops, N, B, "f32")
    Ug = s.mpc_step_ref(X, U, ref)
    assert s.path()[0] == kernel
    x, (st, it, _) = s.solution(), s.info()
    ties = _f32_parity(s, x, st, it, x_ref, st_ref, it_ref, margin, q, u, ops, f"f32 {kernel} N={N}")
    print(f"f32 {kernel} N={N}: {ties} of {B} QPs took a tie's other branch")
    np.testing.assert_allclose(Ug, U + x[:, 0], rtol=0, atol=1e-12)


@pytest.mark.gpu
def test_per_qp_reference_mixed_tile_matches_oracle(plant, monkeypatch):
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    N, B = 20, 8192
    ops = _ops(plant, N)
    X, U, ref = _inputs(N, B)
    q, u, x_ref, st_ref, it_ref, _, margin = _oracle(plant, N, B)
    assert margin.min() >= 1e-4  # no schedule tie in reach of the fp32 stretches: none may be off-schedule
    s = _ctx(ops, N, B, "mixed")
    Ug = s.mpc_step_ref(X, U, ref)
    assert s.path() == ("tile", True)
    x, (st, it, _) = s.solution(), s.info()
    _mixed_parity(x, s.dual(), st, it, x_ref, st_ref, it_ref, q, u, ops, f"mixed N={N} B={B}")
    assert np.abs(Ug - (U + x_ref[:, 0])).max() < MIXED_TOL


# ---- 4. the hardest-first order with references -----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "mixed"])
def test_order_with_references_is_transparent(plant, dtype, monkeypatch):
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    N, B = 20, 8192
    ops = _ops(plant, N)
    X, U, ref = _inputs(N, B)
    q, u = _oracle(plant, N, B)[:2]

    def run(order):
        if order:
            monkeypatch.delenv("MPCQ_ORDER", raising=False)
        else:
            monkeypatch.setenv("MPCQ_ORDER", "0")
        s = _ctx(ops, N, B, dtype)
        Ug = s.mpc_step_ref(X, U, ref)
        o, lst = s.order()
        out = _outputs(s, Ug)
        s.close()
        return o, lst, out

    o1, order, got = run(True)
    o0, order0, ref_out = run(False)
    assert o1 and not o0 and np.array_equal(order0, np.arange(B))
    for name, a, b in zip(("U", "x", "y", "status", "iter", "rho"), got, ref_out):
        assert np.array_equal(a, b, equal_nan=True), name
    assert np.array_equal(np.sort(order), np.arange(B))  # a permutation of the batch
    xu = -np.linalg.solve(ops["P"], q.T).T  # the key of the QP's actual (reference-carrying) q
    key = (xu @ ops["A"].T - u).max(axis=1)
    bins = _order_bin(key)[order]
    inv = int((np.diff(bins) < 0).sum())
    print(f"order {dtype}: {inv} bin inversions along the device's order (allowed {2e-3 * B:.0f})")
    assert inv <= 2e-3 * B
    # without the G ref_b term the key would be that of another q: the order then is far from sorted
    key0 = ((-np.linalg.solve(ops["P"], oracle.gradient(ops, X, U).T).T) @ ops["A"].T - u).max(axis=1)
    assert (np.diff(_order_bin(key0)[order]) < 0).sum() > 2e-3 * B


# ---- 5. receding horizon, warm-started, host loop ----------------------------------------------------
@pytest.mark.gpu
def test_receding_horizon_with_sliding_window(plant, kernel):
    N, B, steps = 20, 512, 3
    ops = _ops(plant, N)
    X, U, _ = _inputs(N, B)
    sched = _schedules(B, N + steps)
    l, u0 = np.full(2 * N, LMIN), _u0(ops)
    s = _ctx(ops, N, B)
    refs = [oracle.Solver(ops["P"], np.zeros(N), ops["A"], l, u0) for _ in range(16)]
    U_ref, Ug = U[:16].copy(), U.copy()
    for k in range(steps):
        win = _window(sched, k, N)
        Ug = s.mpc_step_ref(X, Ug, win)
        q, u = _qu(ops, X[:16], U_ref, win[:16])
        for b, r in enumerate(refs):
            assert r.update_gradient(q[b])
            assert r.update_upper_bound(u[b])
            if r.solve() == sm.SOLVED:
                U_ref[b] += r.x()[0]
        print(f"{kernel} step {k}: max |U - U_oracle| {np.abs(Ug[:16] - U_ref).max():.2e}")
        np.testing.assert_allclose(Ug[:16], U_ref, rtol=0, atol=1e-9)
    s.close()


# ---- 6. streams --------------------------------------------------------------------------------------
STREAMS = {"tile": {}, "wave": {"MPCQ_STREAM": "wave"}, "graph": {"MPCQ_STREAM": "graph"}}


def _stream_ctx(plant, ops, N, B, dtype):
    s = _ctx(ops, N, B, dtype)
    s.mpc_set_plant(plant["Ad"], plant["Bd"])
    return s


def _run_ref(s, X, U, sched, stride, steps, first_step, path, each=None):
    """steps control steps in calls of `each` (default: one call); returns X, U and the summed counters."""
    import torch
    Xd, Ud = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(U.copy()).cuda()
    Sd = torch.from_numpy(np.ascontiguousarray(sched)).cuda()
    st = torch.cuda.Stream()
    each = each or steps
    its, uns, trace = 0, 0, []
    for k in range(0, steps, each):
        with torch.cuda.stream(st):
            s.mpc_run_ref_device(Xd.data_ptr(), Ud.data_ptr(), Sd.data_ptr(), sched.shape[-1], stride, each, 9, 0,
                                 first_step + k, 1e-2, st.cuda_stream)
        st.synchronize()
        assert s.stream_path() == path
        a, b = s.stream_counters()
        its, uns = its + a, uns + b
        trace.append((Xd.cpu().numpy().copy(), Ud.cpu().numpy().copy()))
    return Xd.cpu().numpy(), Ud.cpu().numpy(), its, uns, trace


def _run_scalar(s, X, U, xref, steps, path):
    import torch
    Xd, Ud = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(U.copy()).cuda()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        s.mpc_run_device(Xd.data_ptr(), Ud.data_ptr(), xref, steps, 9, 0, 0, 1e-2, st.cuda_stream)
    st.synchronize()
    assert s.stream_path() == path
    return (Xd.cpu().numpy(), Ud.cpu().numpy(), *s.stream_counters())


def _stream_a_and_c(plant, path, dtype, monkeypatch):
    """(a) one call of 10 steps == ten calls of one step; (c) a shared schedule of 0.7 == xref 0.7.
    Returns what (b) needs: the inputs, the schedule and the per-step trace."""
    for k, v in STREAMS[path].items():
        monkeypatch.setenv(k, v)
    N, B, steps, L = 20, 512, 10, 8
    ops = _ops(plant, N)
    X, U, _ = _inputs(N, B)
    sched = _schedules(B, L)
    s = _stream_ctx(plant, ops, N, B, dtype)
    one = _run_ref(s, X, U, sched, L, steps, 0, path)
    s.close()
    s = _stream_ctx(plant, ops, N, B, dtype)
    ten = _run_ref(s, X, U, sched, L, steps, 0, path, each=1)
    s.close()
    for name, a, b in zip(("X", "U", "iterations", "unsolved"), one[:4], ten[:4]):
        assert np.array_equal(a, b), (path, dtype, name)
    assert one[3].sum() == 0  # every step of every plant ended SOLVED
    # (c)
    s = _stream_ctx(plant, ops, N, B, dtype)
    shared = _run_ref(s, X, U, np.full(L, 0.7), 0, steps, 0, path)
    s.close()
    s = _stream_ctx(plant, ops, N, B, dtype)
    scalar = _run_scalar(s, X, U, 0.7, steps, path)
    s.close()
    for name, a, b in zip(("X", "U", "iterations", "unsolved"), shared[:4], scalar):
        assert np.array_equal(a, b), (path, dtype, name)
    return ops, X, U, sched, ten[4]


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["tile", "wave", "graph"])
def test_stream_with_reference_schedule(plant, path, monkeypatch):
    N, nref = 20, 16
    ops, X, U, sched, trace = _stream_a_and_c(plant, path, "f64", monkeypatch)
    B = X.shape[0]
    # (b) a host loop over the first 16 plants: warm-started oracle, simulated plant, the same noise
    l, u0 = np.full(2 * N, LMIN), _u0(ops)
    refs = [oracle.Solver(ops["P"], np.zeros(N), ops["A"], l, u0) for _ in range(nref)]
    Xk, Uk = X[:nref].copy(), U[:nref].copy()
    for k, (Xg, Ug) in enumerate(trace):
        q, u = _qu(ops, Xk, Uk, _window(sched[:nref], k, N))
        for b, r in enumerate(refs):
            assert r.update_gradient(q[b])
            assert r.update_upper_bound(u[b])
            if r.solve() == oracle.SOLVED:
                Uk[b] += r.x()[0]
        np.testing.assert_allclose(Ug[:nref], Uk, rtol=0, atol=1e-9, err_msg=f"{path} step {k}")
        Xk = workload.simulate(plant["Ad"], plant["Bd"], Xk, Uk, workload.plant_noise(9, 0, B, k, 4, 1e-2)[:nref])
        np.testing.assert_allclose(Xg[:nref], Xk, rtol=1e-11, atol=1e-12, err_msg=f"{path} step {k}")
        Xk = Xg[:nref].copy()  # keep the oracle on the device's trajectory (libm vs device math)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "mixed"])
def test_tile_stream_with_reference_schedule_low_precision(plant, dtype, monkeypatch):
    _stream_a_and_c(plant, "tile", dtype, monkeypatch)


@pytest.mark.gpu
def test_stream_leaves_the_last_steps_q(plant):
    """After a stream the device view's q is the last step's window's, the schedule buffer overwritten."""
    import torch
    N, B, steps, L = 20, 512, 4, 8
    ops = _ops(plant, N)
    X, U, _ = _inputs(N, B)
    sched = _schedules(B, L)
    s = _stream_ctx(plant, ops, N, B, "f64")
    Xd, Ud = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(U.copy()).cuda()
    Sd = torch.from_numpy(sched.copy()).cuda()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        s.mpc_run_ref_device(Xd.data_ptr(), Ud.data_ptr(), Sd.data_ptr(), L, L, steps - 1, 9, 0, 0, 0.0, st.cuda_stream)
    st.synchronize()
    Xl, Ul = Xd.cpu().numpy(), Ud.cpu().numpy()  # the state the last step starts from
    with torch.cuda.stream(st):
        s.mpc_run_ref_device(Xd.data_ptr(), Ud.data_ptr(), Sd.data_ptr(), L, L, 1, 9, 0, steps - 1, 0.0, st.cuda_stream)
    st.synchronize()
    assert s.stream_path() == "tile"
    Sd.fill_(float("nan"))
    torch.cuda.synchronize()
    v = s.device_view()
    torch.cuda.synchronize()
    qd = torch.as_tensor(_DevArray(v["q"], (B, N)), device="cuda").cpu().numpy()
    q = _qu(ops, Xl, Ul, _window(sched, steps - 1, N))[0]
    assert np.all(np.abs(qd - q) <= 1e-12 * np.maximum(1.0, np.abs(q)))


# ---- 7. errors and polish ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_and_order_errors(plant):
    import torch
    N, B = 20, 64
    ops = _ops(plant, N)
    X, U, ref = _inputs(N, B)
    Xd, Ud = torch.from_numpy(X).cuda(), torch.from_numpy(U).cuda()
    Rd = torch.from_numpy(np.ascontiguousarray(np.hstack([ref, ref]))).cuda()  # rows of 2 N: any stride N .. 2 N
    st = torch.cuda.Stream()

    def code(fn, *a):
        with pytest.raises(sm.MpcqError) as e:
            fn(*a)
        return e.value.code

    s = _ctx(ops, N, B, operators=False)
    assert code(s.mpc_step_ref_device, Xd.data_ptr(), Ud.data_ptr(), Rd.data_ptr(), N) == _capi.MPCQ_ERR_ORDER
    s.nx = 4
    assert code(s.mpc_step_ref, X, U, ref) == _capi.MPCQ_ERR_ORDER
    s.close()

    s = _ctx(ops, N, B)
    s.mpc_set_plant(plant["Ad"], plant["Bd"])
    assert code(s.mpc_step_ref_device, Xd.data_ptr(), Ud.data_ptr(), 0, N) == _capi.MPCQ_ERR_ARG
    assert code(s.mpc_step_ref_device, Xd.data_ptr(), Ud.data_ptr(), Rd.data_ptr(), N - 1) == _capi.MPCQ_ERR_ARG
    assert code(s.mpc_step_ref_device, 0, Ud.data_ptr(), Rd.data_ptr(), N) == _capi.MPCQ_ERR_ARG
    null = C.POINTER(C.c_double)()
    Xh, Uh = np.ascontiguousarray(X), np.ascontiguousarray(U)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    assert sm.lib().mpcq_mpc_step_ref(s._ctx, dp(Xh), dp(Uh), null, N) == _capi.MPCQ_ERR_ARG
    assert sm.lib().mpcq_mpc_step_ref(s._ctx, dp(Xh), dp(Uh), dp(ref), N - 1) == _capi.MPCQ_ERR_ARG
    run = lambda sched, L, stride, first: code(s.mpc_run_ref_device, Xd.data_ptr(), Ud.data_ptr(), sched, L, stride,  # noqa: E731
                                               2, 9, 0, first, 0.0, st.cuda_stream)
    assert run(0, 8, 8, 0) == _capi.MPCQ_ERR_ARG              # null schedule
    assert run(Rd.data_ptr(), 0, 8, 0) == _capi.MPCQ_ERR_ARG  # sched_len < 1
    assert run(Rd.data_ptr(), 8, 7, 0) == _capi.MPCQ_ERR_ARG  # stride below the length
    assert run(Rd.data_ptr(), 8, 8, -1) == _capi.MPCQ_ERR_ARG  # negative first step
    # the valid forms still run afterwards (a wider stride, a shared row)
    s.mpc_step_ref_device(Xd.data_ptr(), Ud.data_ptr(), Rd.data_ptr(), 2 * N)
    s.mpc_step_ref_device(Xd.data_ptr(), Ud.data_ptr(), Rd.data_ptr(), 0)
    torch.cuda.synchronize()
    assert np.all(s.info()[0] == sm.SOLVED)
    s.close()

    s = _ctx(ops, N, B, settings=sm.default_settings(polish=1))
    s.mpc_set_plant(plant["Ad"], plant["Bd"])
    assert code(s.mpc_run_ref_device, Xd.data_ptr(), Ud.data_ptr(), Rd.data_ptr(), 8, 2 * N, 2, 9, 0, 0, 0.0,
                st.cuda_stream) == _capi.MPCQ_ERR_ARG
    s.close()


@pytest.mark.gpu
def test_wider_stride_reads_the_right_rows(plant, kernel):
    """ref_stride > n: QP b's reference starts at b * ref_stride."""
    import torch
    N, B = 20, 512
    ops = _ops(plant, N)
    X, U, ref = _inputs(N, B)
    x_ref = _oracle(plant, N, B)[2]
    wide = np.full((B, N + 3), np.nan)
    wide[:, :N] = ref
    s = _ctx(ops, N, B)
    Xd, Ud, Rd = (torch.from_numpy(a.copy()).cuda() for a in (X, U, wide))
    s.mpc_step_ref_device(Xd.data_ptr(), Ud.data_ptr(), Rd.data_ptr(), N + 3)
    torch.cuda.synchronize()
    assert np.abs(s.solution() - x_ref).max() < 1e-9
    s.close()


@pytest.mark.gpu
def test_step_ref_honours_polish(plant):
    N, B = 20, 512
    ops = _ops(plant, N)
    X, U, ref = _inputs(N, B)
    q, u = _oracle(plant, N, B)[:2]
    tight = oracle.batch_solve(ops["P"], ops["A"], np.zeros(N), np.full(2 * N, LMIN), _u0(ops), q, u,
                               settings=oracle.default_settings(eps_abs=1e-10, eps_rel=1e-10, max_iter=200000))[0]
    err = {}
    for polish in (0, 1):
        s = _ctx(ops, N, B, "f32", settings=sm.default_settings(polish=polish))
        Ug = s.mpc_step_ref(X, U, ref)
        err[polish] = np.abs(Ug - (U + tight[:, 0]))
        if polish:
            sp = s.polish_info()[0]
            assert (sp == 1).sum() > B // 2, (sp == 1).sum()
        s.close()
    print(f"f32 applied move vs the tight oracle: mean {err[0].mean():.2e} without polish, {err[1].mean():.2e} with")
    assert err[1].mean() < err[0].mean() and err[1].max() < err[0].max()


# ---- 8. the Python and C++ surfaces --------------------------------------------------------------------
@pytest.mark.gpu
def test_python_api_reference_trajectory(golden_dir):
    cfg = golden_dir / "plant_mpc_api.json"
    N, B = sm.mpc.MPC_WINDOW, 4
    X = workload.mpc_states(3, 0, B)[0]
    ref = _schedules(B, N, seed=5)
    a = sm.ModelPredictiveControlAPI(config=cfg, batch=B)
    b = sm.ModelPredictiveControlAPI(config=cfg, batch=B)
    assert a.solverFlag and b.solverFlag
    a.X = X.copy()
    a.setRefTrajectory(ref)
    a.setF()
    np.testing.assert_allclose(a.f, X @ a.Fx.T + ref @ a.Fr.T, rtol=0, atol=1e-12)
    assert a.controllerStep()
    U1 = b.solver.mpc_step_ref(X, np.zeros(B), ref)
    assert np.array_equal(a.U, U1) and np.abs(U1).max() > 0
    a.setRefTrajectory(ref[0])  # one trajectory shared by the copies
    assert a.controllerStep()
    U2 = b.solver.mpc_step_ref(X, U1, ref[0])
    assert np.array_equal(a.U, U2)
    a.setRefTrajectory(None)  # back on the scalar path
    assert a.controllerStep()
    U3 = b.solver.mpc_step(X, U2, b.xref)
    assert np.array_equal(a.U, U3)
    with pytest.raises(ValueError):
        a.setRefTrajectory(np.zeros(N + 1))


@pytest.mark.gpu
def test_cpp_api_reference_trajectory(golden_dir):
    """A caller of the C++ class: updateRef(std::vector<double>) makes controllerStep step through
    mpcq_mpc_step_ref; two steps with a ramp reference equal the Python class's."""
    cpp = ROOT / "tests" / "cpp"
    exe = cpp / "build" / "ref_trajectory_caller"
    (cpp / "build").mkdir(exist_ok=True)
    # the compiler line of the from_json_check rule of tests/cpp/Makefile
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-o", str(exe), "ref_trajectory_caller.cpp",
                    "../../solvempc_amd/cpp/mpc_api.cpp", "../../solvempc_amd/cpp/mpcq_solver.cpp", "-L../../solvempc_amd",
                    "-lmpcq", "-Wl,-rpath,$ORIGIN/../../../solvempc_amd"], cwd=cpp, check=True)
    cfg = golden_dir / "plant_mpc_api.json"
    r = subprocess.run([str(exe), str(cfg)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [float(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("U ")]
    assert len(got) == 3
    N = sm.mpc.MPC_WINDOW
    a = sm.ModelPredictiveControlAPI(config=cfg, batch=1)
    a.X = np.array([[0.05, -0.02, 0.01, 0.1]])
    want = []
    a.setRefTrajectory(0.1 * np.arange(N))
    for _ in range(2):
        assert a.controllerStep()
        want.append(a.U[0])
    a.setRefTrajectory(None)  # updateRef(double) in the caller: the scalar path again
    assert a.controllerStep()
    want.append(a.U[0])
    print("C++ U", got, "Python U", want)
    np.testing.assert_allclose(got[:2], want[:2], rtol=0, atol=1e-12)
    # (the third step ran on the scalar path again; there the C++ class forms q on the host as the reference
    # does and the Python class on the device, so only its having moved U is checked)
    assert np.isfinite(got[2]) and got[2] != got[1]

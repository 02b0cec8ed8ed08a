"""The tile kernel's fp64 remainder rows (n = 20: rows 16-19 of every n-row product and rows 32-39 of the
stacked [B~; S] product run on v_mfma_f64_4x4x4_4b_f64 chains instead of a padded 16x16x4 tile, mpcq_tile.h
MPCQ_REM4D) against the CPU oracle, at the smallest batches that cover one column, one full wave and one
workgroup plus a one-wave second workgroup.  The bars are test_gpu.py's: fp64 the oracle's trajectory (status,
iterations, rho to 1e-9 relative, |x - x_oracle| < 1e-9), mixed test_mixed_tile_parity's.  The remainder rows
are asserted on their own (x[16:20]; the duals of rows 16-19 and 36-39, which are the rows of A that the
remainder rows of B~ eta' feed), so that a wrong remainder row is named in the failure."""
import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import workload

pytestmark = pytest.mark.gpu
LMIN = -np.finfo(np.float64).max
N20 = 20
BATCHES = (1, 16, 80)
MIXED_TOL = 1e-5  # test_gpu.py: north_star's bound on the applied move, absolute
_REF = {}


def _problem(plant, N, B, u_range=1.0):
    ops = oracle.condense(plant, N)
    X, U = workload.mpc_states(1, 0, B, u_range)
    return ops, X, U, oracle.gradient(ops, X, U), oracle.upper_bound(ops, X, U)


def _reference(plant, N, B, u_range=1.0):
    """The oracle's solve of the case, computed once: x, status, iterations, rho (batch_solve) and the duals
    (one oracle.Solver per QP: batch_solve does not return them)."""
    key = (N, B, u_range)
    if key not in _REF:
        ops, X, U, q, u = _problem(plant, N, B, u_range)
        l = np.full(2 * N, LMIN)
        u0 = oracle.upper_bound(ops, np.zeros(4), 0.0)
        x, st, it, rho = oracle.batch_solve(ops["P"], ops["A"], np.zeros(N), l, u0, q, u)
        y = np.empty((B, 2 * N))
        for b in range(B):
            r = oracle.Solver(ops["P"], np.zeros(N), ops["A"], l, u0, oracle.default_settings())
            assert r.update_gradient(q[b]) and r.update_upper_bound(u[b])
            r.solve()
            assert r.info().status == st[b] and r.info().iter == it[b]
            y[b] = r.y()
        for v in (x, st, it, rho, y):
            v.setflags(write=False)
        _REF[key] = (ops, X, U, q, u, x, st, it, rho, y)
    return _REF[key]


def _solve(ops, q, u, N, dtype):
    s = sm.BatchSolver(N, 2 * N, q.shape[0], dtype=dtype)
    s.setup(ops["P"], np.zeros(N), ops["A"], np.full(2 * N, LMIN), oracle.upper_bound(ops, np.zeros(4), 0.0))
    s.update_lin_cost(q)
    s.update_upper_bound(u)
    s.solve()
    return s


def _f64_bars(x, y, st, it, rho, ref, what):
    x_ref, st_ref, it_ref, rho_ref, y_ref = ref
    assert np.array_equal(st, st_ref), what
    assert np.array_equal(it, it_ref), what
    np.testing.assert_allclose(rho, rho_ref, rtol=1e-9)
    ex, ey = np.abs(x - x_ref), np.abs(y - y_ref)
    print(f"{what}: max |dx| {ex.max():.2e} (rows 16-19 {ex[:, 16:20].max():.2e}), max |dy| {ey.max():.2e} "
          f"(rows 16-19 {ey[:, 16:20].max():.2e}, rows 36-39 {ey[:, 36:40].max():.2e})")
    assert ex[:, 16:20].max() < 1e-9, (what, "x rows 16-19", ex[:, 16:20].max())
    assert ey[:, 16:20].max() < 1e-9, (what, "y rows 16-19", ey[:, 16:20].max())
    assert ey[:, 36:40].max() < 1e-9, (what, "y rows 36-39", ey[:, 36:40].max())
    assert ex.max() < 1e-9, (what, ex.max())


@pytest.mark.parametrize("B", BATCHES)
def test_f64_remainder_rows_match_oracle(plant, B, monkeypatch):
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    ops, X, U, q, u, *ref = _reference(plant, N20, B)
    s = _solve(ops, q, u, N20, "f64")
    assert s.path()[0] == "tile"
    _f64_bars(s.solution(), s.dual(), *s.info(), ref, f"f64 N=20 B={B}")
    s.close()


@pytest.mark.parametrize("B", BATCHES)
def test_mixed_remainder_rows_match_oracle(plant, B, monkeypatch):
    """test_mixed_tile_parity's bar (test_gpu.py _mixed_parity; at these batch sizes its allowance of 1e-4 of
    the QPs off the oracle's schedule is no QP), with the bound on rows 16-19 of the solution on its own."""
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    ops, X, U, q, u, x_ref, st_ref, it_ref, _, _ = _reference(plant, N20, B)
    s = _solve(ops, q, u, N20, "mixed")
    assert s.path()[0] == "tile"
    x, (st, it, _) = s.solution(), s.info()
    s.close()
    assert np.array_equal(st, st_ref)
    assert np.array_equal(it, it_ref)
    scale = np.maximum(1.0, np.abs(x_ref).max(axis=1))
    e0 = np.abs(x[:, 0] - x_ref[:, 0])
    ev = np.abs(x - x_ref) / scale[:, None]
    print(f"mixed N=20 B={B}: max |dx0| {e0.max():.2e}, max rel |dx| {ev.max():.2e} (rows 16-19 {ev[:, 16:20].max():.2e})")
    assert e0.max() < MIXED_TOL
    assert ev[:, 16:20].max() < MIXED_TOL, ("x rows 16-19", ev[:, 16:20].max())
    assert ev.max() < MIXED_TOL


def test_f64_mpc_step_publish_matches_oracle(plant, monkeypatch):
    """One hardest-first MPC step (mpc_step_device, lazy publish) at B = 80: U and solution() against the
    oracle, with solution() read after get_info and before it (the finalize / tile_publish_kernel pair)."""
    import torch
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    B = 80
    ops, X, U, q, u, x_ref, st_ref, it_ref, rho_ref, y_ref = _reference(plant, N20, B)
    U_ref = U + np.where(st_ref == sm.SOLVED, x_ref[:, 0], 0.0)

    def run(info_first):
        s = sm.BatchSolver(N20, 2 * N20, B, dtype="f64")
        s.setup(ops["P"], np.zeros(N20), ops["A"], np.full(2 * N20, LMIN), oracle.upper_bound(ops, np.zeros(4), 0.0))
        s.mpc_set_operators(ops["Fx"], ops["Fu"], ops["Fr"], ops["Sbar"], ops["Ku"], ops["W0"])
        Xd, Ud = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(U.copy()).cuda()
        s.mpc_step_device(Xd.data_ptr(), Ud.data_ptr(), 0.0)
        if info_first:
            info, x = s.info(), s.solution()
        else:
            x, info = s.solution(), s.info()
        torch.cuda.synchronize()
        assert s.path()[0] == "tile" and s.order()[0]
        out = (Ud.cpu().numpy(), x, s.dual(), *info)
        s.close()
        return out

    a_, b_ = run(True), run(False)
    for v, w in zip(a_, b_):
        assert np.array_equal(v, w, equal_nan=True)
    Ug, x, y, st, it, rho = a_
    _f64_bars(x, y, st, it, rho, (x_ref, st_ref, it_ref, rho_ref, y_ref), "f64 MPC step B=80")
    assert np.abs(Ug - U_ref).max() < 1e-9


def test_f64_n15_unchanged(plant, monkeypatch):
    """N = 15 has no remainder tile (n = 15 pads to one 16-row tile): the oracle's trajectory as before."""
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    N, B = 15, 16
    ops, X, U, q, u, x_ref, st_ref, it_ref, rho_ref, _ = _reference(plant, N, B, 0.0)
    s = _solve(ops, q, u, N, "f64")
    assert s.path()[0] == "tile"
    x, (st, it, rho) = s.solution(), s.info()
    s.close()
    assert np.array_equal(st, st_ref) and np.array_equal(it, it_ref)
    np.testing.assert_allclose(rho, rho_ref, rtol=1e-9)
    assert np.abs(x - x_ref).max() < 1e-9

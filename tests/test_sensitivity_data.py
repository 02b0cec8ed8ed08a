"""Gradients with respect to the QP's matrices on the device (mpcq_sensitivity_data*, diff.qp_solution;
solvempc_amd/csrc/mpcq_sensdata.hip) against the CPU references of tests/test_sensitivity_data_ref.py.

Two kinds of checks.  The contraction (a shared plant's sums over the batch) is compared with a numpy contraction
of the same call's per-QP outputs within the standard summation bound, 2 (B + 8) 2^-53 times the sum of the
absolute terms of each element: that covers the matrix core's fused products and numpy's own order.  What the
per-QP terms are is checked end to end on per-plant contexts and, for reduced precision, through the per-QP
formula applied to the call's own outputs, against references that share no code with the device."""
import re
from pathlib import Path

import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import workload

import test_gpu as tg
import test_polish as tp
import test_sensitivity as ts
import test_sensitivity_data_ref as dref
import test_sensitivity_ref as ref

pytestmark = pytest.mark.gpu

LMIN = tp.LMIN
PREFIX = tp.PREFIX
ERR_ARG, ERR_ORDER = sm._capi.MPCQ_ERR_ARG, sm._capi.MPCQ_ERR_ORDER
XY_TOL = 1e-9  # the device's x, y against the oracle's (tests/test_gpu.py test_fp64_trajectory_parity)
CHUNK = int(re.search(r"kSensChunk = (\d+);", (Path(__file__).resolve().parents[1] / "solvempc_amd" / "csrc" /
                                                "mpcq_internal.h").read_text()).group(1))


def _bits(words, m):
    """(B,) uint64 bit masks -> (B, m) booleans."""
    return ((words[:, None] >> np.arange(m, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def _check_masks(gl, gu, act, na):
    m = gl.shape[1]
    low, upp = _bits(act[:, 0], m), _bits(act[:, 1], m)
    ok = na >= 0
    assert np.array_equal((low.sum(axis=1) + upp.sum(axis=1))[ok], na[ok])
    assert not (low & upp).any() and not low[~ok].any() and not upp[~ok].any()
    assert not ((gl != 0) & ~low).any() and not ((gu != 0) & ~upp).any()
    if m < 64:
        assert not (act >> np.uint64(m)).any()
    return low, upp


def _check_contraction(out, x, y, label=""):
    """gP, gA of a shared-plant call against the numpy contraction of the same call's outputs (module docstring)."""
    gq, gl, gu, gP, gA, act, na = out
    B, m = gl.shape
    low, upp = _check_masks(gl, gu, act, na)
    keep = na >= 0
    gqk, xk, wk = gq[keep], x[keep], (gl + gu)[keep]
    yk = np.where(low | upp, y, 0.0)[keep]
    assert np.isfinite(xk).all() and np.isfinite(yk).all()
    S, aS = gqk.T @ xk, np.abs(gqk).T @ np.abs(xk)
    eP, aP = 0.5 * (S + S.T), 0.5 * (aS + aS.T)
    eA, aA = yk.T @ gqk - wk.T @ xk, np.abs(yk).T @ np.abs(gqk) + np.abs(wk).T @ np.abs(xk)
    f = 2.0 * (B + 8) * 2.0 ** -53
    assert np.isfinite(gP).all() and np.isfinite(gA).all()
    assert np.array_equal(gP, gP.T)
    rP = np.abs(gP - eP) / np.maximum(f * aP, np.finfo(float).tiny)
    rA = np.abs(gA - eA) / np.maximum(f * aA, np.finfo(float).tiny)
    print(f"  {label}contraction over {int(keep.sum())} of {B} QPs: worst error / bound {rP.max():.1e} (gP), "
          f"{rA.max(initial=0):.1e} (gA); |gP| {np.abs(gP).max():.2e}, |gA| {np.abs(gA).max(initial=0):.2e}")
    assert np.all(np.abs(gP - eP) <= f * aP) and np.all(np.abs(gA - eA) <= f * aA)
    assert np.all(gA[~(low | upp)[keep].any(axis=0)] == 0)  # a row active in no QP


# ----------------------------------------------------------------------------- 1. the contraction
@pytest.mark.parametrize("kern,N,B", [("tile", 20, 4096), ("wave", 15, 512), ("wave", 32, 512), ("wave", 20, 1),
                                      ("wave", 20, 5), ("wave", 20, CHUNK + 3)])
def test_shared_plant_contraction(plant, monkeypatch, kern, N, B):
    """16 + 4 rows (N 20), under 16 rows (N 15), two full tiles and m = 64 (N 32); a K tail below 4 (B 1), off a
    multiple of 4 (B 5) and across a chunk boundary (B = chunk + 3); 16 chunks on the tile path."""
    monkeypatch.setenv("MPCQ_KERNEL", kern)
    seed = ref.MPC_SEEDS[N]
    ops, X, U, q, u = tp._problem(plant, N, B, seed)
    s = ts._solve(ops, q, u, N)
    assert s.path()[0] == kern
    g = ref._cotangents(300 + seed, B, N)
    out = s.sensitivity_data(g)
    x, y = s.solution(), s.dual()
    base = s.sensitivity(g)
    s.close()
    assert out[3].shape == (N, N) and out[4].shape == (2 * N, N) and (out[6] >= 0).all()
    for a, b in zip((out[0], out[1], out[2], out[6]), base):
        assert np.array_equal(a, b)
    _check_contraction(out, x, y, f"{kern} N={N} B={B}: ")
    if B >= 512:
        assert (out[6] > 0).any() and (out[6] == 0).any() and np.abs(out[4]).max() > 0


# ----------------------------------------------------------------------------- 2. per plant, end to end
def _product_rule(tol, sens_ref, x, y, gq, w, xy_tol=XY_TOL):
    """The bound of a product of two factors known to (tol relative to max(1, |ref|_inf)) and (xy_tol absolute):
    tol max(1, |ref|) (|x|_inf + |y|_inf) + xy_tol (|gq|_inf + |w|_inf), per QP."""
    inf = lambda a: np.abs(a).max(axis=1, initial=0.0)
    return tol * np.maximum(1.0, inf(sens_ref)) * (inf(x) + inf(y)) + xy_tol * (inf(gq) + inf(w))


def _compare_per_plant(r, xo, yo, out, low, upp, clear, label):
    gq, gl, gu, gP, gA, act, na = out
    n = gq.shape[1]
    m = gl.shape[1]
    rgq, rw = r["ref"][:, :n], r["ref"][:, n:n + m] + r["ref"][:, n + m:]
    eP, eA = dref._formula_batch(rgq, rw, xo, np.where(low | upp, yo, 0.0))
    bound = _product_rule(r["tol"], r["ref"], xo, yo, rgq, rw)
    err = np.maximum(np.abs(gP - eP).max(axis=(1, 2)), np.abs(gA - eA).max(axis=(1, 2)))
    print(f"  {label}: worst error / bound {(err / bound)[clear].max():.1e} on {int(clear.sum())} QPs "
          f"(bound {bound[clear].min():.1e} .. {bound[clear].max():.1e})")
    assert (~clear).mean() <= ref.MAX_TIES
    assert np.all(err[clear] <= bound[clear])
    assert np.array_equal(gP, gP.transpose(0, 2, 1))
    dl, du = _check_masks(gl, gu, act, na)
    assert np.array_equal(dl[clear], low[clear]) and np.array_equal(du[clear], upp[clear])


def test_per_plant_mpc_matches_reference(plant):
    """N = 20, one copy of the plant per QP: each QP's gP, gA against the formula on _sens_ref's outputs and the
    oracle's own final x, y, within the product rule's bound."""
    N, B = 20, PREFIX
    seed = ref.MPC_SEEDS[N]
    r = ref._mpc_sens_refs(N, seed)
    xo, yo = dref._mpc_oracle_xy(N, seed)
    ops, X, U, q, u = tp._problem(plant, N, B, seed)
    s = ts._solve(ops, q, u, N, n_plants=B)
    out = s.sensitivity_data(r["g"])
    st = s.info()[0]
    s.close()
    assert out[3].shape == (B, N, N) and out[4].shape == (B, 2 * N, N) and np.array_equal(st, r["st"])
    _compare_per_plant(r, xo, yo, out, r["low"], r["upp"], r["clear"], "per-plant MPC N=20")


def test_per_plant_generic_matches_reference():
    """n = 7, m = 11 (lower- and upper-active rows, equalities); one QP ends MPCQ_INVALID_BOUNDS: zeros for it."""
    r = ref._generic_sens_refs()
    xo, yo = dref._generic_oracle_xy()
    P, A, q, l, u = ref._generic_inputs()
    B, n = q.shape
    bad = 5
    l2, u2 = l.copy(), u.copy()
    l2[bad, 7], u2[bad, 7] = 1.0, -1.0
    s = sm.BatchSolver(n, ref.GEN_M, B, n_plants=B)
    s.setup(P, q, A, l, u)
    s.update_bounds(l2, u2)
    s.solve()
    out = s.sensitivity_data(r["g"])
    st = s.info()[0]
    s.close()
    assert st[bad] == sm.INVALID_BOUNDS and out[6][bad] == -1
    assert np.all(out[3][bad] == 0) and np.all(out[4][bad] == 0) and np.all(out[5][bad] == 0)
    low, upp = np.zeros((B, ref.GEN_M), bool), np.zeros((B, ref.GEN_M), bool)
    for b in range(B):  # the rule's sets on the oracle's iterate, as _generic_sens_refs took them
        so = oracle.Solver(P[b], q[b], A[b], l[b], u[b])
        so.solve()
        _, z, yy = so.iterates()
        D, E, c = so.scaling()
        with np.errstate(over="ignore"):
            low[b], upp[b], _ = ref._rule(E * l[b], E * u[b], z, yy)
    clear = r["clear"] & (np.arange(B) != bad)
    _compare_per_plant(r, xo, yo, out, low, upp, clear, "per-plant generic")
    assert (out[1] != 0).any() and (out[2] != 0).any()


# ----------------------------------------------------------------------------- 3. polished, reduced precision
@pytest.mark.parametrize("dtype", ["mixed", "f32"])
def test_reduced_precision_with_polish(plant, monkeypatch, dtype):
    """mixed and f32 on the tile path with settings.polish = 1 (mirrors test_sensitivity.py's test of that name):
    where polish succeeded, the per-QP terms of the call -- the formula on its gq, gl + gu, masks and the returned
    x, y -- are those of _data_exact at the optimum's active set, within the product rule's bound from the
    sensitivity TOL and XY_TOL on the polished x, y (tests/test_polish.py's TOL is below 1e-9).  The sums themselves
    (4,096 QPs, two of them primal infeasible) meet the contraction bound."""
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    N, B = 20, 4096
    seed = ref.MPC_SEEDS[N]
    r = ref._mpc_sens_refs(N, seed)
    exact, margin, nact = ts._optimum_sets(N, seed)
    ops, X, U, q, u = tp._problem(plant, N, B, seed)
    u = u.copy()
    u[[1000, 2001]] = -1e3
    s = ts._solve(ops, q, u, N, dtype=dtype, settings=sm.default_settings(polish=1))
    assert s.path()[0] == "tile"
    g = ts._g_batch(r, B, N, seed)
    out = s.sensitivity_data(g)
    x, y = s.solution(), s.dual()
    st = s.info()[0]
    sp = s.polish_info()[0]
    s.close()
    gq, gl, gu, gP, gA, act, na = out
    assert st[1000] != sm.SOLVED and st[2001] != sm.SOLVED and na[1000] == -1 and na[2001] == -1
    _check_contraction(out, x, y, f"{dtype}: ")
    clear = margin >= ref.TIE
    cmp = clear & (sp[:PREFIX] == 1)
    assert (~clear).mean() <= ref.MAX_TIES and cmp.sum() >= 0.96 * PREFIX
    idx = np.flatnonzero(cmp)
    l = r["l"]
    ex = [dref._data_exact(ops["P"], ops["A"], r["q"][b], l, r["u"][b], r["g"][b]) for b in idx]
    low, upp = _bits(act[:, 0], 2 * N)[idx], _bits(act[:, 1], 2 * N)[idx]
    assert np.array_equal(low, np.array([e["low"] for e in ex])) and np.array_equal(upp, np.array([e["upp"] for e in ex]))
    dP, dA = dref._formula_batch(gq[idx], (gl + gu)[idx], x[idx], np.where(low | upp, y[idx], 0.0))
    eP, eA = np.array([e["gP"] for e in ex]), np.array([e["gA"] for e in ex])
    xs, ys = np.array([e["x"] for e in ex]), np.array([e["y"] for e in ex])
    # (the polished x, y are known relative to max(1, |x*|_inf, |y*|_inf): one solve of the reduced KKT system)
    xy_tol = XY_TOL * np.maximum(1.0, np.maximum(np.abs(xs).max(axis=1), np.abs(ys).max(axis=1)))
    bound = _product_rule(r["tol"], exact[idx], xs, ys, exact[idx][:, :N], exact[idx][:, N:3 * N] + exact[idx][:, 3 * N:],
                          xy_tol)
    err = np.maximum(np.abs(dP - eP).max(axis=(1, 2)), np.abs(dA - eA).max(axis=(1, 2)))
    print(f"{dtype}: {idx.size} of {PREFIX} compared with _data_exact, worst error / bound {(err / bound).max():.1e}")
    assert np.all(err <= bound)


# ----------------------------------------------------------------------------- 4. an infeasible QP in the batch
def test_infeasible_qps_are_left_out_of_the_sums(plant, monkeypatch):
    """tests/test_gpu.py's _infeasible_batch (test_infeasible_statuses_match_oracle): the infeasible QPs' x is NaN;
    the sums are finite and are the contraction without them."""
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    N, B = 20, 4096
    ops, q, u, bad = tg._infeasible_batch(plant, N, B)
    s = tg._gpu_solve(ops, q, u, N)
    assert s.path()[0] == "tile"
    out = s.sensitivity_data(ref._cotangents(400, B, N))
    x, y = s.solution(), s.dual()
    st = s.info()[0]
    s.close()
    assert np.all(st[bad] == sm.PRIMAL_INFEASIBLE) and np.all(np.isnan(x[bad])) and np.all(out[6][bad] == -1)
    assert np.all(out[5][bad] == 0)
    _check_contraction(out, x, y, "infeasible batch: ")


# ----------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("n_plants", [1, 600])
def test_two_calls_give_identical_bits(plant, n_plants):
    """Two calls, bit for bit (a shared plant's 600 QPs span three chunks); with gP, gA and active NULL the call
    writes exactly what sensitivity_device writes."""
    import torch
    N, B = 20, 600
    ops, X, U, q, u = tp._problem(plant, N, B, 1)
    s = ts._solve(ops, q, u, N, n_plants=n_plants)
    k = (B,) if n_plants > 1 else ()
    G = torch.from_numpy(ref._cotangents(500, B, N)).cuda()

    def call(data, full=True):
        t = dict(gq=(B, N), gl=(B, 2 * N), gu=(B, 2 * N), gP=k + (N, N), gA=k + (2 * N, N))
        t = {name: torch.full(shape, 7.0, dtype=torch.float64, device="cuda") for name, shape in t.items()}
        act = torch.full((B, 2), 7, dtype=torch.int64, device="cuda")
        na = torch.full((B,), 7, dtype=torch.int32, device="cuda")
        p = lambda v: v.data_ptr()
        if not data:
            s.sensitivity_device(p(G), p(t["gq"]), p(t["gl"]), p(t["gu"]), p(na))
        elif full:
            s.sensitivity_data_device(p(G), p(t["gq"]), p(t["gl"]), p(t["gu"]), p(t["gP"]), p(t["gA"]), p(act), p(na))
        else:
            s.sensitivity_data_device(p(G), p(t["gq"]), p(t["gl"]), p(t["gu"]), 0, 0, 0, p(na))
        torch.cuda.synchronize()
        return {**{name: v.cpu().numpy() for name, v in t.items()}, "act": act.cpu().numpy(), "na": na.cpu().numpy()}

    a, b, plain, thin = call(True), call(True), call(False), call(True, full=False)
    # a call that asks for gP, gA alone (everything else from the context's staging)
    gP = torch.full(k + (N, N), 7.0, dtype=torch.float64, device="cuda")
    gA = torch.full(k + (2 * N, N), 7.0, dtype=torch.float64, device="cuda")
    s.sensitivity_data_device(G.data_ptr(), 0, 0, 0, gP.data_ptr(), gA.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    s.close()
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    assert np.abs(a["gP"]).max() > 0 and np.abs(a["gA"]).max() > 0 and not (a["gP"] == 7.0).any()
    for name in ("gq", "gl", "gu", "na"):
        assert np.array_equal(plain[name], thin[name]) and np.array_equal(plain[name], a[name]), name
    assert (thin["gP"] == 7.0).all() and (thin["gA"] == 7.0).all() and (thin["act"] == 7).all()
    assert np.array_equal(gP.cpu().numpy(), a["gP"]) and np.array_equal(gA.cpu().numpy(), a["gA"])


# ----------------------------------------------------------------------------- 6. transparency
@pytest.mark.parametrize("kern", ["tile", "wave"])
def test_a_data_call_changes_no_later_solve(plant, monkeypatch, kern):
    """solve, sensitivity_data_device, warm-started second step == the same two steps without the call, bit for
    bit (U, x, status, iter, rho): the tile path, whose lazily kept x, y the call publishes, and the wave path with
    the call on a side stream."""
    import torch
    monkeypatch.setenv("MPCQ_KERNEL", kern)
    N, B = 20, 4096 if kern == "tile" else 512
    ops, X, U, _, _ = tp._problem(plant, N, B, 1)
    X2 = X * 0.9 + 0.01

    def run(call):
        s = ts._mpc_solver(ops, N, B, operators=True)
        Xd, X2d, Ud = (torch.from_numpy(a.copy()).cuda() for a in (X, X2, U))
        s.mpc_step_device(Xd.data_ptr(), Ud.data_ptr(), 0.0)
        assert s.path()[0] == kern
        keep = None
        if call:
            gP = torch.zeros(N, N, dtype=torch.float64, device="cuda")
            gA = torch.zeros(2 * N, N, dtype=torch.float64, device="cuda")
            side = torch.cuda.Stream() if kern == "wave" else None
            s.sensitivity_data_device(0, 0, 0, 0, gP.data_ptr(), gA.data_ptr(), 0, 0, side.cuda_stream if side else None)
            keep = (gP, gA, side)
        s.mpc_step_device(X2d.data_ptr(), Ud.data_ptr(), 0.0)
        torch.cuda.synchronize()
        out = [Ud.cpu().numpy(), s.solution(), *s.info()]
        if call:
            assert np.abs(keep[0].cpu().numpy()).max() > 0 and np.abs(keep[1].cpu().numpy()).max() > 0
        s.close()
        return out

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


# ----------------------------------------------------------------------------- 7. refusals
def test_refusals(plant):
    import torch
    N, B = 20, 64
    ops, X, U, q, u = tp._problem(plant, N, B, 1)
    out = [torch.full(shape, 7.0, dtype=torch.float64, device="cuda")
           for shape in ((B, N), (B, 2 * N), (B, 2 * N), (B, N, N), (B, 2 * N, N))]
    act = torch.full((B, 2), 7, dtype=torch.int64, device="cuda")
    nat = torch.full((B,), 7, dtype=torch.int32, device="cuda")
    data = lambda s: s.sensitivity_data_device(0, *[t.data_ptr() for t in out], act.data_ptr(), nat.data_ptr())

    s = ts._mpc_solver(ops, N, B)
    ts._raises(ERR_ORDER, data, s)              # before any solve
    ts._raises(ERR_ORDER, s.sensitivity_data)
    s.update_lin_cost(q)
    s.update_upper_bound(u)
    s.solve()
    ts._raises(ERR_ARG, s.sensitivity_data_device)  # every output NULL
    s.update_upper_bound(u)                      # new data since the solve
    ts._raises(ERR_ORDER, data, s)
    ts._raises(ERR_ORDER, s.sensitivity_data)
    s.close()

    big = sm.BatchSolver(33, 66, 4, n_plants=4)  # n = 33 (a context of that size exists only as per-plant, m = 2n)
    ts._raises(ERR_ARG, data, big)
    big.close()

    # a MIMO context (the SISO specialisation, n = 20: within the kernel's capacity)
    Ad, Bd = workload.randomized_plants(plant, 3, 0, B)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
    sh = {"Cd": plant["Cd"][None, :], "Q": [[plant["Q"]]], "R": [[plant["R"]]], "RD": [[plant["RD"]]],
          "K": plant["K"][None, :], "K0": [[plant["K"][0]]], "w0": [255.0]}
    mk = [dev(Ad), dev(Bd[:, :, None])] + [dev(np.broadcast_to(np.asarray(sh[k], dtype=np.float64),
                                                               (B,) + np.asarray(sh[k]).shape).copy())
                                            for k in ("Cd", "Q", "R", "RD", "K", "K0", "w0")]
    Xd, Ud = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(U.copy()).cuda()
    mi = sm.BatchSolver(N, 2 * N, B, n_plants=B)
    mi.mimo_setup_plants_device(4, 1, 1, 10, *[k.data_ptr() for k in mk])
    mi.mimo_step_device(Xd.data_ptr(), Ud.data_ptr())
    torch.cuda.synchronize()
    ts._raises(ERR_ARG, data, mi)
    mi.close()

    torch.cuda.synchronize()
    for t in out:
        assert (t == 7.0).all()
    assert (act == 7).all() and (nat == 7).all()


# ----------------------------------------------------------------------------- 8. qp_solution
def _tensors(*arrays, grad=True):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda().requires_grad_(grad) for a in arrays]


def test_qp_solution_backward_is_sensitivity_data_shared(plant):
    """Shared plant (MPC N = 20): the five gradients of one backward pass are one sensitivity_data call's, bit for
    bit; backward after a later solve is refused."""
    import torch
    from solvempc_amd import diff
    N, B = 20, 64
    ops, X, U, q, u = tp._problem(plant, N, B, 1)
    l = np.full((B, 2 * N), LMIN)
    s = sm.BatchSolver(N, 2 * N, B)
    P, A, qt, lt, ut = _tensors(ops["P"], ops["A"], q, l, u)
    G = torch.from_numpy(ref._cotangents(600, B, N)).cuda()
    x, status = diff.qp_solution(s, P, A, qt, lt, ut)
    assert np.array_equal(x.detach().cpu().numpy(), s.solution()) and (status.cpu().numpy() == sm.SOLVED).all()
    (x * G).sum().backward()
    gq, gl, gu, gP, gA, act, na = s.sensitivity_data(G.cpu().numpy())
    for t, e in ((P, gP), (A, gA), (qt, gq), (lt, gl), (ut, gu)):
        assert t.grad.shape == t.shape and np.array_equal(t.grad.cpu().numpy(), e)
    assert np.abs(gP).max() > 0 and np.abs(gA).max() > 0 and (na > 0).any()
    # the same data without a new setup; then backward after an intervening solve
    x2, st2 = diff.qp_solution(s, P, A, qt, lt, ut, setup=False)
    assert (st2.cpu().numpy() == sm.SOLVED).all() and x2.shape == x.shape
    s.solve()
    with pytest.raises(RuntimeError, match="solved again"):
        (x2 * G).sum().backward()
    s.close()


def test_qp_solution_per_plant_and_directional_differences():
    """Per-plant context, the generic family, settings.polish = 1.  Backward equals sensitivity_data on the same
    solve, bit for bit.  Then the derivative of sum_b g_b . x_b along a random symmetric dP and a random dA,
    <gP, dP> + <gA, dA> per QP, against central differences (h = 1e-5) of two more polished device solves, on the
    clear QPs the CPU reference kept.  Tolerance: 100 x the error of the same difference quotient done on the CPU
    with _optimum against _data_exact (test_sensitivity_data_ref._directional_fd: 9.1e-9, so 9.1e-7), relative to
    max(1, |derivative|): the reference's own error, nothing the device returns."""
    import torch
    from solvempc_amd import diff
    P, A, q, l, u = ref._generic_inputs()
    r = ref._generic_sens_refs()
    d = dref._directional_fd()
    dP, dA = dref._directions()
    B, n = q.shape
    h = dref.H
    G = torch.from_numpy(r["g"].copy()).cuda()

    def solve(Pm, Am):
        s = sm.BatchSolver(n, ref.GEN_M, B, n_plants=B, settings=sm.default_settings(polish=1))
        t = _tensors(Pm, Am, q, l, u)
        x, status = diff.qp_solution(s, *t)
        return s, t, x, status

    s, t, x, status = solve(P, A)
    (x * G).sum().backward()
    out = s.sensitivity_data(r["g"])
    sp0 = s.polish_info()[0]
    s.close()
    for tt, e in zip(t, (out[3], out[4], out[0], out[1], out[2])):
        assert np.array_equal(tt.grad.cpu().numpy(), e)
    deriv = (out[3] * dP).sum(axis=(1, 2)) + (out[4] * dA).sum(axis=(1, 2))
    vals, ok = [], (status.cpu().numpy() == sm.SOLVED) & (sp0 == 1)
    for sgn in (1.0, -1.0):
        s2, _, x2, st2 = solve(P + sgn * h * dP, A + sgn * h * dA)
        ok &= (st2.cpu().numpy() == sm.SOLVED) & (s2.polish_info()[0] == 1)
        s2.close()
        vals.append((x2.detach() * G).sum(dim=1).cpu().numpy())
    fd = (vals[0] - vals[1]) / (2 * h)
    keep = d["keep"] & ok
    tol = 100.0 * d["err"]
    err = np.abs(deriv - fd) / np.maximum(1.0, np.abs(fd))
    print(f"qp_solution: directional derivative vs device differences on {int(keep.sum())} of {B} QPs: "
          f"{err[keep].max():.2e} (tolerance {tol:.1e}); vs the CPU formula {np.abs(deriv - d['exact'])[keep].max():.2e}")
    assert keep.sum() >= 0.9 * d["keep"].sum()
    assert err[keep].max() <= tol

"""GPU tests of mpcq_update_P_A / mpcq_update_P_A_device (include/mpcq.h): new P and A for a context
that is set up, with every QP's q, l, u kept and the next solve warm-started from the previous (x, y).

Inputs and oracle references: tests/test_update_P_A_ref.py (which also shows that every QP of them ends SOLVED in
the oracle on every route).  The warm start handed to the oracle is the device's own first solution()/dual(), so
both sides start the second solve from identical bits.

Bars:
* against the oracle, fp64: status, iterations and rho equal (rho to rtol 1e-9), |dx| < 1e-9 -- the bars of
  test_gpu.test_fp64_trajectory_parity; f32 and mixed at the project's F32_TOL / 1e-5 bars with the tie rule;
* kept scaling with scaled_termination: the oracle iterates on the pre-scaled problem, formed in the header's
  rounding order, so the same bars apply.  A QP may leave the oracle's schedule only where the oracle's own decision
  margin is within fp64 rounding of flipping, FP64_TIE = 1e-9: the two sides' residuals differ by accumulated fp64
  rounding alone, far below the 1e-9 bar on x that the same accumulation has to meet;
* kept scaling with the default (unscaled) termination: OSQP's two termination inequalities on the returned
  (x, y) in numpy fp64 (oracle.kkt_residuals), slack (1 + 1e-9) and 1e-12 for summation order.  The primal one is
  taken in the form that needs no z: with r = ||Ax - z||_inf >= dist_inf(Ax, [l, u]) and ||z|| <= ||Ax|| + r,
  r <= eps_abs + eps_rel max(||Ax||, ||z||) implies dist_inf(Ax, [l, u]) <= (eps_abs + eps_rel ||Ax||) / (1 - eps_rel);
* device against device: bit for bit.
"""
import subprocess

import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import _capi
from solvempc_amd.diff import _DevArray, qp_solution

import test_gpu as tg
import test_update_P_A_ref as ref

pytestmark = pytest.mark.gpu
B, BP = ref.B_SHARED, ref.B_PLANTS
FP64_TIE = 1e-9
EPS = 1e-3  # eps_abs = eps_rel of the default settings


@pytest.fixture(params=["tile", "wave", "lane"])
def kernel(request, monkeypatch):
    monkeypatch.setenv("MPCQ_KERNEL", request.param)
    return request.param


_CASES = {}


def shared(plant, N):
    if N not in _CASES:
        _CASES[N] = ref.shared_case(plant, N)
    return _CASES[N]


def plants(plant):
    if "pp" not in _CASES:
        _CASES["pp"] = ref.plants_case(plant)
    return _CASES["pp"]


def solved_shared(cs, dtype="f64", settings=None, which="old", q=None, u=None):
    """A shared-plant context set up on the case's old (or new) matrices, with the QPs' data, after one solve."""
    N = cs["N"]
    s = sm.BatchSolver(N, 2 * N, len(cs["q"]), dtype=dtype, settings=settings)
    s.setup(cs[which]["P"], cs["q0"], cs[which]["A"], cs["l0"], cs["u0"])
    s.update_lin_cost(cs["q"] if q is None else q)
    s.update_bounds(cs["l"], cs["u"] if u is None else u)
    if which == "old":
        s.solve()
    return s


def solved_plants(cs, dtype="f64", which="old", settings=None):
    N = cs["N"]
    s = sm.BatchSolver(N, 2 * N, BP, n_plants=BP, dtype=dtype, settings=settings)
    s.setup(cs[f"P_{which}"], cs["q0"], cs[f"A_{which}"], cs["l0"], cs["u0"])
    s.update_lin_cost(cs["q"])
    s.update_bounds(cs["l"], cs["u"])
    if which == "old":
        s.solve()
    return s


def results(s):
    return (s.solution(), s.dual(), *s.info())


def same_bits(got, want, what=""):
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b, equal_nan=True), (what, k, np.argwhere(~((a == b) | (a != a)))[:4])


def oracle_rescale(cs, x1, y1, b, per_plant=False):
    if per_plant:
        return ref.ref_rescale(cs["P_new"][b], cs["A_new"][b], cs["q0"][b], cs["l0"][b], cs["u0"][b], cs["q"][b],
                               cs["u"][b], x1[b], y1[b])
    return ref.ref_rescale(cs["new"]["P"], cs["new"]["A"], cs["q0"], cs["l0"], cs["u0"], cs["q"][b], cs["u"][b], x1[b],
                           y1[b])


def fp64_parity(s, refs, what=""):
    x, _, st, it, rho = results(s)
    xr = np.stack([r[0] for r in refs])
    str_, itr, rhor = (np.array([r[k] for r in refs]) for k in (2, 3, 4))
    err = np.abs(x - xr).max()
    print(f"{what}: iterations {it.min()}..{it.max()} (mean {it.mean():.1f}), max|dx| = {err:.3e}")
    assert np.array_equal(st, str_) and np.all(st == sm.SOLVED), what
    assert np.array_equal(it, itr), (what, np.flatnonzero(it != itr)[:8])
    np.testing.assert_allclose(rho, rhor, rtol=1e-9)
    assert err < 1e-9, what


# ---- 1. rescale = 1 against the oracle, fp64, every kernel; per plant
@pytest.mark.parametrize("N", [20, 15])
def test_rescale_trajectory_parity(plant, N, kernel):
    cs = shared(plant, N)
    s = solved_shared(cs)
    x1, y1 = s.solution(), s.dual()
    s.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=True)
    s.solve()
    fp64_parity(s, [oracle_rescale(cs, x1, y1, b) for b in range(B)], f"rescale=1 N={N} {kernel} path {s.path()}")


def test_rescale_trajectory_parity_per_plant(plant):
    cs = plants(plant)
    s = solved_plants(cs)
    x1, y1 = s.solution(), s.dual()
    s.update_P_A(cs["P_new"], cs["A_new"], rescale=True)
    s.solve()
    fp64_parity(s, [oracle_rescale(cs, x1, y1, b, True) for b in range(BP)], "rescale=1 per plant")


# ---- 2. rescale = 0 against the oracle on the pre-scaled problem (scaled_termination = 1), shared plant
@pytest.mark.parametrize("N", [20, 15])
def test_keep_scaling_trajectory_parity(plant, N, kernel):
    cs = shared(plant, N)
    s = solved_shared(cs, settings=sm.default_settings(scaled_termination=1))
    x1, y1 = s.solution(), s.dual()
    D, E, c = s.scaling()
    s.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=False)
    D2, E2, c2 = s.scaling()
    assert np.array_equal(D, D2) and np.array_equal(E, E2) and c == c2
    s.solve()
    x, _, st, it, _ = results(s)
    refs = [ref.ref_keep(cs["new"]["P"], cs["new"]["A"], D, E, c, cs["l0"], cs["u0"], cs["q"][b], cs["l"][b], cs["u"][b],
                         x1[b], y1[b]) for b in range(B)]
    xr = D * np.stack([r[0] for r in refs])
    str_, itr, margin = (np.array([r[k] for r in refs]) for k in (2, 3, 5))
    off = it != itr
    err = np.abs(x - xr)[~off].max()
    print(f"rescale=0 N={N} {kernel}: iterations {it.min()}..{it.max()} (mean {it.mean():.1f}), max|x - D x'| = {err:.3e}, "
          f"{int(off.sum())} off schedule, smallest margin {margin.min():.2e}")
    assert np.array_equal(st, str_) and np.all(st == sm.SOLVED)
    assert not np.any(off & ~(margin < FP64_TIE)), (np.flatnonzero(off)[:8], margin[off][:8])
    assert err < 1e-9


# ---- 3. rescale = 0 with the default termination: OSQP's own criteria on the returned (x, y)
def osqp_terminated(P, A, q, l, u, x, y):
    r = oracle.kkt_residuals(P, q, A, l, u, x, y)
    Pf = ref.sym_upper(P)
    ax, px, aty = np.abs(A @ x).max(), np.abs(Pf @ x).max(), np.abs(A.T @ y).max()
    pri_tol = (EPS + EPS * ax) / (1.0 - EPS)
    dua_tol = EPS + EPS * max(px, aty, np.abs(q).max())
    return r["primal"] <= pri_tol * (1 + 1e-9) + 1e-12 and r["stationarity"] <= dua_tol * (1 + 1e-9) + 1e-12


@pytest.mark.parametrize("N", [20, 15])
def test_keep_scaling_default_termination(plant, N, kernel):
    cs = shared(plant, N)
    s = solved_shared(cs)
    it1 = s.info()[1]
    s.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=False)
    s.solve()
    x, y, st, it, _ = results(s)
    print(f"rescale=0 N={N} {kernel}: mean iterations {it.mean():.1f} warm (first solve, cold: {it1.mean():.1f})")
    assert np.all(st == sm.SOLVED)
    bad = [b for b in range(B) if not osqp_terminated(cs["new"]["P"], cs["new"]["A"], cs["q"][b], cs["l"][b], cs["u"][b],
                                                      x[b], y[b])]
    assert not bad, bad[:8]


def test_keep_scaling_default_termination_per_plant(plant):
    cs = plants(plant)
    s = solved_plants(cs)
    s.update_P_A(cs["P_new"], cs["A_new"], rescale=False)
    s.solve()
    x, y, st, it, _ = results(s)
    assert np.all(st == sm.SOLVED)
    bad = [b for b in range(BP) if not osqp_terminated(cs["P_new"][b], cs["A_new"][b], cs["q"][b], cs["l"][b],
                                                       cs["u"][b], x[b], y[b])]
    assert not bad, bad[:8]


# ---- 4. path equivalence, bit for bit: update = setup on the new matrices + data + warm start
def zero_nonfinite(x, y):
    bad = ~(np.isfinite(x).all(axis=1) & np.isfinite(y).all(axis=1))
    x, y = x.copy(), y.copy()
    x[bad], y[bad] = 0.0, 0.0
    return x, y, bad


@pytest.mark.parametrize("dtype", ["f64", "f32", "mixed"])
def test_update_equals_setup_and_warm_start(plant, dtype, kernel):
    cs = shared(plant, 20)
    N = 20
    u = cs["u"].copy()
    u[5, [3, N + 3]] = -5.0  # rows 3 and N + 3 are negations: A_3 x <= -5 and A_3 x >= 5, infeasible
    a = solved_shared(cs, dtype, u=u)
    x1, y1, st1, _, _ = results(a)
    assert st1[5] != sm.SOLVED and np.all(np.delete(st1, 5) == sm.SOLVED)
    a.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=True)
    a.solve()
    b = solved_shared(cs, dtype, which="new", u=u)
    xz, yz, bad = zero_nonfinite(x1, y1)
    b.warm_start(xz, yz)
    b.solve()
    print(f"{dtype} {kernel}: {int(bad.sum())} QP(s) started cold, status of QP 5: {st1[5]}")
    # the infeasible QP's x, y are NaN (OSQP's certificate status) and it is the one cold start.  An fp32 iterate may
    # miss the certificate and end with a finite x (include/mpcq.h, MPCQ_F32): then QP 5 is warm-started like the
    # rest, and test_nonfinite_previous_solution_starts_cold covers the cold start in that precision
    assert bad.sum() == int(bad[5]) and bad[5] == (st1[5] == sm.PRIMAL_INFEASIBLE)
    if dtype != "f32":
        assert bad[5]
    same_bits(results(a), results(b), f"{dtype} {kernel}")


@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("dtype", ["f64", "f32", "mixed"])
def test_nonfinite_previous_solution_starts_cold(plant, dtype, rescale, kernel):
    """Rows of the previous (x, y) that hold a NaN or an infinity, here installed through mpcq_warm_start (NaN in x
    of QP 7, inf in y of QP 9), start cold in every precision; every other QP is warm-started."""
    cs = shared(plant, 20)
    first = solved_shared(cs, dtype)
    xn, yn = first.solution(), first.dual()
    xn[7, 3], yn[9, 0] = np.nan, np.inf
    xz, yz, bad = zero_nonfinite(xn, yn)
    assert list(np.flatnonzero(bad)) == [7, 9]
    runs = []
    for x, y in ((xn, yn), (xz, yz)):
        s = solved_shared(cs, dtype)
        s.warm_start(x, y)
        s.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=rescale)
        s.solve()
        runs.append(results(s))
    assert np.all(runs[0][2] == sm.SOLVED)
    same_bits(runs[0], runs[1], f"{dtype} {kernel} rescale={rescale}")
    if rescale:  # and both are a setup on the new matrices warm-started at the zeroed rows
        b = solved_shared(cs, dtype, which="new")
        b.warm_start(xz, yz)
        b.solve()
        same_bits(runs[0], results(b), f"{dtype} {kernel} against setup")


def test_cold_start_before_the_update_stands(plant, kernel):
    """mpcq_cold_start, then the update: the next solve starts cold (as a setup on the new matrices + data)."""
    cs = shared(plant, 20)
    a = solved_shared(cs)
    a.cold_start()
    a.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=True)
    a.solve()
    b = solved_shared(cs, which="new")
    b.solve()
    same_bits(results(a), results(b), "cold start kept")
    fresh = solved_shared(cs, which="new")  # (set up, never solved: an update starts it cold too)
    fresh.update_P_A(cs["new"]["P"], None, rescale=True)
    fresh.solve()
    same_bits(results(fresh), results(b), "never solved")


@pytest.mark.parametrize("family", ["tile", "wave"])
def test_update_after_a_stream_run_warm_starts_from_its_last_step(plant, family, monkeypatch):
    """A one-launch stream run (tile stream mode / one QP per wave) is a solve: its last step's (x, y) are the
    update's warm start, on a context that never called mpcq_solve."""
    import torch
    monkeypatch.setenv("MPCQ_KERNEL", family)
    cs = shared(plant, 20)
    old = cs["old"]
    side = torch.cuda.Stream()
    a = sm.BatchSolver(20, 40, B)
    a.setup(old["P"], cs["q0"], old["A"], cs["l0"], cs["u0"])
    a.mpc_set_operators(*(old[k] for k in ("Fx", "Fu", "Fr", "Sbar", "Ku", "W0")))
    a.mpc_set_plant(plant["Ad"], plant["Bd"])
    from solvempc_amd import workload
    X, U = workload.stream_states(4, 0, B)  # (the stream workload's states: every step of it ends SOLVED)
    Xd, Ud = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(U.copy()).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        a.mpc_run_device(Xd.data_ptr(), Ud.data_ptr(), 0.0, 3, 9, 0, 0, 1e-2, side.cuda_stream)
    side.synchronize()
    assert a.stream_path() == family
    x1, y1 = a.solution(), a.dual()
    q1, l1, u1 = view(a)
    assert np.all(a.info()[0] == sm.SOLVED) and np.isfinite(x1).all() and np.isfinite(y1).all()
    a.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=True)
    a.solve()
    b = sm.BatchSolver(20, 40, B)
    b.setup(cs["new"]["P"], cs["q0"], cs["new"]["A"], cs["l0"], cs["u0"])
    b.update_lin_cost(q1)
    b.update_bounds(l1, u1)
    b.warm_start(x1, y1)
    b.solve()
    same_bits(results(a), results(b), f"after a {family} stream run")


@pytest.mark.parametrize("rescale", [True, False])
def test_update_equals_setup_and_warm_start_per_plant(plant, rescale):
    """Per plant (the direct-inverse reading).  rescale = 0 against rescale = 1 cannot be bit-equal (another
    scaling), so the kept-scaling run is compared with itself through the device form instead."""
    import torch
    cs = plants(plant)
    a = solved_plants(cs)
    x1, y1 = a.solution(), a.dual()
    a.update_P_A(cs["P_new"], cs["A_new"], rescale=rescale)
    a.solve()
    if rescale:
        b = solved_plants(cs, which="new")
        b.warm_start(x1, y1)
    else:
        b = solved_plants(cs)
        Pd, Ad = torch.from_numpy(cs["P_new"]).cuda(), torch.from_numpy(cs["A_new"]).cuda()
        b.update_P_A_device(Pd.data_ptr(), Ad.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    b.solve()
    same_bits(results(a), results(b), f"per plant rescale={rescale}")


@pytest.mark.parametrize("per_plant", [False, True])
def test_update_on_the_workgroup_setup_kernel(plant, per_plant, monkeypatch):
    """MPCQ_SETUP=ref: the context is built by the workgroup setup kernel (mpcq_setup.hip).  rescale = 1 runs that
    kernel again (bit for bit a setup + warm start); rescale = 0 rebuilds such a block's factors with the wave keep
    kernel, and lands on the wave-built context's trajectory (the two kernels' blocks differ by rounding alone)."""
    cs = plants(plant) if per_plant else shared(plant, 20)
    make = solved_plants if per_plant else solved_shared
    new = (cs["P_new"], cs["A_new"]) if per_plant else (cs["new"]["P"], cs["new"]["A"])
    wave = make(cs)
    wave.update_P_A(*new, rescale=False)
    wave.solve()
    monkeypatch.setenv("MPCQ_SETUP", "ref")
    a = make(cs)
    x1, y1 = a.solution(), a.dual()
    a.update_P_A(*new, rescale=True)
    a.solve()
    b = make(cs, which="new")
    b.warm_start(x1, y1)
    b.solve()
    same_bits(results(a), results(b), "workgroup kernel, rescale=1")
    k = make(cs)
    k.update_P_A(*new, rescale=False)
    k.solve()
    (xk, _, stk, itk, _), (xw, _, stw, itw, _) = results(k), results(wave)
    assert np.array_equal(stk, stw) and np.all(stk == sm.SOLVED) and np.array_equal(itk, itw)
    assert np.abs(xk - xw).max() < 1e-9


def test_update_then_mpc_step_on_the_tile_path(plant, monkeypatch):
    import torch
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    cs = shared(plant, 20)
    old = cs["old"]
    X2 = torch.from_numpy(cs["X"] * 0.9).cuda()

    def front(s):
        s.mpc_set_operators(*(old[k] for k in ("Fx", "Fu", "Fr", "Sbar", "Ku", "W0")))

    a = sm.BatchSolver(20, 40, B)
    a.setup(old["P"], cs["q0"], old["A"], cs["l0"], cs["u0"])
    front(a)
    Xd, Ud = torch.from_numpy(cs["X"].copy()).cuda(), torch.from_numpy(cs["U"].copy()).cuda()
    a.mpc_step_device(Xd.data_ptr(), Ud.data_ptr(), 0.0)
    x1, y1 = a.solution(), a.dual()
    U1 = Ud.cpu().numpy()
    a.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=True)
    a.mpc_step_device(X2.data_ptr(), Ud.data_ptr(), 0.0)
    torch.cuda.synchronize()
    assert a.path() == ("tile", True) and a.order()[0]

    b = sm.BatchSolver(20, 40, B)
    b.setup(cs["new"]["P"], cs["q0"], cs["new"]["A"], cs["l0"], cs["u0"])
    front(b)
    b.warm_start(x1, y1)  # (q, u are the step's own: no data update stands between setup and step on either side)
    Ub = torch.from_numpy(U1.copy()).cuda()
    b.mpc_step_device(X2.data_ptr(), Ub.data_ptr(), 0.0)
    torch.cuda.synchronize()
    assert b.order()[0]
    assert np.array_equal(Ud.cpu().numpy(), Ub.cpu().numpy())
    same_bits(results(a), results(b), "mpc step")
    same_bits(a.sensitivity(), b.sensitivity(), "sensitivity")


# ---- 5. unchanged matrices and data
def view(s, names=("q", "l", "u")):
    import torch
    v = s.device_view()
    torch.cuda.synchronize()
    shape = {"q": (s.batch, s.n), "l": (s.batch, s.m), "u": (s.batch, s.m)}
    return [torch.as_tensor(_DevArray(v[k], shape[k], "<f8"), device="cuda").cpu().numpy() for k in names]


@pytest.mark.parametrize("rescale", [True, False])
def test_null_matrix_keeps_the_current_one(plant, rescale, kernel):
    cs = shared(plant, 20)
    new, old = cs["new"], cs["old"]
    runs = []
    for P, A in ((new["P"], None), (new["P"], old["A"]), (None, new["A"]), (old["P"], new["A"])):
        s = solved_shared(cs)
        s.update_P_A(P, A, rescale=rescale)
        s.solve()
        runs.append(results(s))
    same_bits(runs[0], runs[1], "A = NULL")
    same_bits(runs[2], runs[3], "P = NULL")


def test_data_and_outputs_are_kept(plant, kernel):
    cs = shared(plant, 20)
    s = solved_shared(cs, settings=sm.default_settings(polish=1))
    before, out = view(s), results(s)
    assert np.any(s.polish_info()[0] != 0)
    s.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=False)
    same_bits(view(s), before, "q, l, u")
    same_bits(results(s), out, "outputs until the next solve")
    assert np.all(s.polish_info()[0] == 0)
    with pytest.raises(sm.MpcqError) as e:
        s.sensitivity()
    assert e.value.code == _capi.MPCQ_ERR_ORDER
    s.solve()
    assert np.all(s.info()[0] == sm.SOLVED) and np.any(s.polish_info()[0] != 0)


def test_lazy_step_data_are_kept(plant, monkeypatch):
    """After a tile-path step q, u are lazy (the step's saved X, U): the update materialises them first."""
    import torch
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    cs = shared(plant, 20)
    old = cs["old"]

    def stepped():
        s = sm.BatchSolver(20, 40, B)
        s.setup(old["P"], cs["q0"], old["A"], cs["l0"], cs["u0"])
        s.mpc_set_operators(*(old[k] for k in ("Fx", "Fu", "Fr", "Sbar", "Ku", "W0")))
        Xd, Ud = torch.from_numpy(cs["X"].copy()).cuda(), torch.from_numpy(cs["U"].copy()).cuda()
        s.mpc_step_device(Xd.data_ptr(), Ud.data_ptr(), 0.0)
        torch.cuda.synchronize()
        return s

    want = view(stepped())  # (published right after the step)
    s = stepped()
    s.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=False)
    same_bits(view(s), want, "lazy q, u")
    assert np.abs(want[0] - cs["q"]).max() <= 1e-12 * np.abs(cs["q"]).max()


# ---- 6. f32 and mixed against the oracle
@pytest.mark.parametrize("N", [20, 15])
def test_rescale_parity_f32(plant, N, kernel):
    cs = shared(plant, N)
    s = solved_shared(cs, "f32")
    x1, y1 = s.solution(), s.dual()
    s.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=True)
    s.solve()
    x, _, st, it, _ = results(s)
    refs = [oracle_rescale(cs, x1, y1, b) for b in range(B)]
    xr = np.stack([r[0] for r in refs])
    str_, itr, margin = (np.array([r[k] for r in refs]) for k in (2, 3, 5))
    assert np.all(st == sm.SOLVED)
    ties = tg._f32_parity(s, x, st, it, xr, str_, itr, margin, cs["q"], cs["u"], cs["new"])
    print(f"f32 N={N} {kernel}: {ties} of {B} QPs took a tie's other branch")


@pytest.mark.parametrize("N", [20, 15])
def test_rescale_parity_mixed(plant, N, monkeypatch):
    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    cs = shared(plant, N)
    s = solved_shared(cs, "mixed")
    x1, y1 = s.solution(), s.dual()
    s.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=True)
    s.solve()
    x, y, st, it, _ = results(s)
    refs = [oracle_rescale(cs, x1, y1, b) for b in range(B)]
    xr = np.stack([r[0] for r in refs])
    str_, itr = (np.array([r[k] for r in refs]) for k in (2, 3))
    # the mixed bar: the oracle's status and the applied move within 1e-5 absolute on EVERY QP; the whole vector at
    # the same bar where the QP kept the oracle's schedule, OSQP's own criteria where an fp32 stretch tipped a tie
    off = it != itr
    e0 = np.abs(x[:, 0] - xr[:, 0])
    print(f"mixed N={N}: max |dx0| {e0.max():.2e}, {int(off.sum())} of {B} QPs off the oracle's schedule")
    assert np.array_equal(st, str_) and np.all(st == sm.SOLVED)
    assert e0.max() < tg.MIXED_TOL
    ev = np.abs(x - xr).max(axis=1) / np.maximum(1.0, np.abs(xr).max(axis=1))
    assert ev[~off].max() < tg.MIXED_TOL
    if off.any():
        tg._osqp_terminated(x[off], y[off], cs["q"][off], cs["u"][off], cs["new"])


# ---- 7. refusals
def test_refusals_write_nothing(plant):
    import torch
    cs = shared(plant, 20)
    new = cs["new"]
    code = lambda f, *a, **k: pytest.raises(sm.MpcqError, f, *a, **k).value.code

    fresh = sm.BatchSolver(20, 40, B)
    assert code(fresh.update_P_A, new["P"], new["A"]) == _capi.MPCQ_ERR_ORDER  # no setup yet

    s = solved_shared(cs)
    twin = solved_shared(cs)
    assert code(s.update_P_A) == _capi.MPCQ_ERR_ARG  # both NULL
    Pd, Ad = torch.from_numpy(new["P"]).cuda(), torch.from_numpy(new["A"]).cuda()
    assert code(s.update_P_A_device, Pd.data_ptr(), Ad.data_ptr(), 2) == _capi.MPCQ_ERR_ARG  # rescale not 0 / 1
    assert code(s.update_P_A_device, Pd.data_ptr(), Ad.data_ptr(), -1) == _capi.MPCQ_ERR_ARG
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):  # (as test_sensitivity's refusal case)
        assert code(s.update_P_A_device, Pd.data_ptr(), Ad.data_ptr(), 1, side.cuda_stream) == _capi.MPCQ_ERR_ARG
        assert code(s.update_P_A_device, Pd.data_ptr(), Ad.data_ptr(), 0, side.cuda_stream) == _capi.MPCQ_ERR_ARG
    torch.cuda.synchronize()
    s.solve()
    twin.solve()
    same_bits(results(s), results(twin), "after the refused calls")


def test_refusal_one_shot_and_mimo_contexts(plant):
    import torch
    from solvempc_amd import workload
    N, Bq = 20, 64
    Ad, Bd = workload.randomized_plants(plant, 3, 0, Bq)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    rep = lambda v: dev(np.broadcast_to(np.asarray(v, dtype=np.float64), (Bq,) + np.shape(v)))
    arrs = [dev(Ad), dev(Bd), rep(plant["Cd"]), rep(plant["K"]), rep(plant["Q"]), rep(plant["R"]), rep(plant["RD"])]
    X, U = workload.mpc_states(1, 0, Bq)
    Xd, Ud = dev(X), dev(U)
    s = sm.BatchSolver(N, 2 * N, Bq, n_plants=Bq)
    s.mpc_plants_step_device(4, 10, *[t.data_ptr() for t in arrs], Xd.data_ptr(), Ud.data_ptr())
    torch.cuda.synchronize()
    P = np.zeros((Bq, N, N))
    with pytest.raises(sm.MpcqError) as e:
        s.update_P_A(P, None)
    assert e.value.code == _capi.MPCQ_ERR_ORDER  # a OneShot context keeps no operators
    big = sm.BatchSolver(120, 240, 4, n_plants=4)  # n > 32: served by the MIMO entry points only
    for rescale in (True, False):
        with pytest.raises(sm.MpcqError) as e:
            big.update_P_A(np.zeros((4, 120, 120)), None, rescale=rescale)
        assert e.value.code == _capi.MPCQ_ERR_ARG


def test_keep_scaling_serves_the_largest_generic_shape():
    """rescale = 0 needs n <= 32, m <= 64.  mpcq_create gives larger plants to the MIMO entry points only, so a
    context beyond the limit is always a MIMO one (refused with MPCQ_ERR_ARG for both values of rescale:
    test_refusal_one_shot_and_mimo_contexts); here the limit itself, n = 32, m = 64 on a generic QP, is served."""
    rng = np.random.default_rng(0)
    n, m, Bq = 32, 64, 8
    G = rng.normal(size=(n, n))
    P = G @ G.T + n * np.eye(n)
    A = rng.normal(size=(m, n))
    l0, u0 = np.full(m, -1.0), np.full(m, 1.0)
    s = sm.BatchSolver(n, m, Bq)
    s.setup(P, np.zeros(n), A, l0, u0)
    s.update_lin_cost(rng.normal(size=(Bq, n)))
    s.solve()
    s.update_P_A(1.1 * P, None, rescale=False)  # the largest shape the keep-scaling kernels take
    s.solve()
    assert np.all(s.info()[0] == sm.SOLVED)


def test_unconstrained_context_has_no_A_to_update():
    """m = 0: an A alone is nothing to update (MPCQ_ERR_ARG, nothing written); a new P is served."""
    rng = np.random.default_rng(31)
    n, Bq = 7, 8
    M = rng.normal(size=(Bq, n, n))
    P = M @ M.transpose(0, 2, 1) + 0.5 * np.eye(n)
    q, e, A = rng.normal(size=(Bq, n)), np.zeros((Bq, 0)), np.zeros((Bq, 0, n))

    def ctx(Pm):
        s = sm.BatchSolver(n, 0, Bq, n_plants=Bq)
        s.setup(Pm, q, A, e, e)
        return s

    a, twin = ctx(P), ctx(P)
    a.solve()
    twin.solve()
    # (a pointer that is not NULL, whatever numpy hands out for an empty array)
    spare = np.zeros(1)
    rc = sm.lib().mpcq_update_P_A(a._ctx, None, spare.ctypes.data_as(sm.C.POINTER(sm.C.c_double)), 1)
    assert rc == _capi.MPCQ_ERR_ARG
    a.solve()
    twin.solve()
    same_bits(results(a), results(twin), "after the refused call")
    x1, y1 = a.solution(), a.dual()
    P2 = 1.3 * P
    a.update_P_A(P2, None, rescale=True)
    a.solve()
    b = ctx(P2)
    b.warm_start(x1, y1)
    b.solve()
    same_bits(results(a), results(b), "m = 0, rescale=1")
    twin.update_P_A(P2, None, rescale=False)
    twin.solve()
    x = twin.solution()
    assert np.all(twin.info()[0] == sm.SOLVED)
    for k in range(Bq):  # OSQP's dual inequality (the only one without constraints)
        px = P2[k] @ x[k]
        tol = EPS + EPS * max(np.abs(px).max(), np.abs(q[k]).max())
        assert np.abs(px + q[k]).max() <= tol * (1 + 1e-9) + 1e-12


def test_non_psd_update_leaves_the_context_needing_setup(plant):
    cs = shared(plant, 20)
    for rescale in (True, False):
        s = solved_shared(cs)
        with pytest.raises(sm.MpcqError) as e:
            s.update_P_A(-cs["new"]["P"], None, rescale=rescale)
        assert e.value.code == _capi.MPCQ_ERR_SETUP
        with pytest.raises(sm.MpcqError) as e:
            s.solve()
        assert e.value.code == _capi.MPCQ_ERR_ORDER
        s.setup(cs["old"]["P"], cs["q0"], cs["old"]["A"], cs["l0"], cs["u0"])  # mpcq_setup recovers it
        s.update_lin_cost(cs["q"])
        s.update_bounds(cs["l"], cs["u"])
        s.solve()
        assert np.all(s.info()[0] == sm.SOLVED)


# ---- 8. upper layers
def test_osqp_eigen_updates_match_the_oracle(plant, tmp_path):
    exe = ref.build_update_caller()
    if exe is None:
        pytest.skip("build() compiles update_caller where an Eigen include directory exists; this tree's build had "
                    "none (it has no reference_caller either)")
    cs = shared(plant, 15)
    b = 3
    ref.caller_input(cs, b, tmp_path / "in.txt")
    r = subprocess.run([str(exe), str(tmp_path / "in.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    N = 15
    rows = [np.array([float(v) for v in line.split()]) for line in r.stdout.strip().split("\n")]
    assert len(rows) == 3
    got = [(int(v[0]), int(v[1]), v[2:2 + N], v[2 + N:]) for v in rows]
    q, l, u = cs["q"][b], cs["l"][b], cs["u"][b]
    first = oracle.Solver(cs["old"]["P"], q, cs["old"]["A"], l, u)
    first.solve()
    want = [(first.info().status, first.info().iter, first.x())]
    for P, A, (_, _, x, y) in ((cs["new"]["P"], cs["old"]["A"], got[0]), (cs["new"]["P"], cs["new"]["A"], got[1])):
        o = oracle.Solver(P, q, A, l, u)  # (initSolver's q is the setup's q0, as in the caller)
        o.warm_start(x, y)
        o.solve()
        want.append((o.info().status, o.info().iter, o.x()))
    for k, ((st, it, x, _), (st_r, it_r, x_r)) in enumerate(zip(got, want)):
        assert st == st_r == oracle.SOLVED and it == it_r and np.abs(x - x_r).max() < 1e-9, (k, st, it, it_r)


@pytest.mark.parametrize("mode,rescale", [("update", True), ("update_keep", False)])
def test_qp_solution_update_modes(plant, mode, rescale):
    import torch
    cs = shared(plant, 20)
    dev = lambda a, g=False: torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(g)
    P0, A0 = dev(cs["old"]["P"]), dev(cs["old"]["A"])
    q, l, u = dev(cs["q"]), dev(cs["l"]), dev(cs["u"])
    gx = dev(np.random.default_rng(2).normal(size=(B, 20)))

    def grads(solver, setup):
        P, A = dev(cs["new"]["P"], True), dev(cs["new"]["A"], True)
        x, st = qp_solution(solver, P, A, q, l, u, setup=setup)
        (x * gx).sum().backward()
        return x.detach().cpu().numpy(), st.cpu().numpy(), P.grad.cpu().numpy(), A.grad.cpu().numpy()

    a = sm.BatchSolver(20, 40, B)
    x1, _ = qp_solution(a, P0, A0, q, l, u, setup=True)
    y1 = a.dual()
    got = grads(a, mode)
    if mode == "update":  # the same as setup=True followed by the same warm start
        b = sm.BatchSolver(20, 40, B)
        b.setup(cs["new"]["P"], cs["q0"], cs["new"]["A"], cs["l"][0], cs["u"][0])
        b.warm_start(x1.detach().cpu().numpy(), y1)
        want = grads(b, False)
    else:  # the same as the C ABI's kept-scaling update
        b = sm.BatchSolver(20, 40, B)
        qp_solution(b, P0, A0, q, l, u, setup=True)
        b.update_P_A(cs["new"]["P"], cs["new"]["A"], rescale=False)
        want = grads(b, False)
    assert np.array_equal(got[1], want[1]) and np.all(got[1] == sm.SOLVED)
    assert np.abs(got[0] - want[0]).max() < 1e-9
    for g, w in zip(got[2:], want[2:]):
        assert np.abs(g - w).max() <= 1e-9 * max(1.0, np.abs(w).max())

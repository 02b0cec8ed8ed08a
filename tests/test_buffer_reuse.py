"""GPU tests of the context's device buffers across calls that release, reallocate or grow them: a context taken
through a first shape or size and then a second must give, bit for bit, what a fresh context created directly
in the second state gives (x, y, status, iter, rho, U, as tests/test_update_P_A.py same_bits compares them), and a
destroyed context must give all its device memory back.

Shapes are the smallest that take each path: batch 8, horizon N = 4 unless the path needs otherwise, fp64.
Inputs: the reference plant and its leading 2-state block, condensed on the device (solvempc_amd.mpc.condense).
"""
import numpy as np
import pytest

import solvempc_amd as sm
from solvempc_amd import mpc, workload

pytestmark = pytest.mark.gpu
B, N = 8, 4
S_ROWS = 2
LOWER = -np.finfo(np.float64).max


def _dev(a, dtype=np.float64):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda:0")


def same_bits(got, want, what=""):
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b, equal_nan=True), (what, k, np.argwhere(~((a == b) | (a != a)))[:4])


def results(s):
    return (s.solution(), s.dual(), *s.info())


def sub_plant(plant, nx):
    """The plant's leading nx states, with a plant axis of one (mpc.condense's layout)."""
    p = {k: np.asarray(plant[k], dtype=np.float64)[None, :nx] for k in ("Bd", "Cd", "K")}
    p["Ad"] = plant["Ad"][None, :nx, :nx]
    p.update({k: np.array([plant[k]]) for k in ("Q", "R", "RD")})
    return p


_CASES = {}


def case(plant, nx, n_plants=1, horizon=N):
    """Condensed operators of ``n_plants`` plants of nx states (perturbed by +-2 % when more than one), with states X,
    previous moves U and the QP data (q, u) of one control step from them."""
    key = (nx, n_plants, horizon)
    if key not in _CASES:
        p = sub_plant(plant, nx)
        if n_plants > 1:
            rng = np.random.default_rng(17)
            p = {k: np.repeat(v, n_plants, axis=0) for k, v in p.items()}
            p["Ad"] = p["Ad"] * (1 + 0.02 * rng.uniform(-1, 1, p["Ad"].shape))
            p["Bd"] = p["Bd"] * (1 + 0.02 * rng.uniform(-1, 1, p["Bd"].shape))
        ops = mpc.condense(p, horizon, s_rows=S_ROWS)
        X, U = workload.mpc_states(5, 0, B)
        X = np.ascontiguousarray(X[:, :nx])
        k = (lambda a: a) if n_plants > 1 else (lambda a: np.broadcast_to(a, (B,) + a.shape[1:]))
        q = np.einsum("bij,bj->bi", k(ops["Fx"]), X) + k(ops["Fu"]) * U[:, None] + 0.5 * k(ops["Fr"]).sum(axis=2)
        u = k(ops["W0"]) + np.einsum("bij,bj->bi", k(ops["Sbar"]), X) + k(ops["Ku"]) * U[:, None]
        _CASES[key] = dict(plant=p, ops=ops, X=X, U=U, q=q, u=u, nx=nx, n=horizon, k=n_plants)
    return _CASES[key]


def set_up(s, cs, operators=True):
    """mpcq_setup on the case's P, A with the X = U = 0 data, then its MPC operators."""
    o, k, n = cs["ops"], cs["k"], cs["n"]
    s.setup(o["P"], np.zeros((k, n)), o["A"], np.full((k, 2 * n), LOWER), o["W0"])
    if operators:
        s.mpc_set_operators(*[o[key] for key in ("Fx", "Fu", "Fr", "Sbar", "Ku", "W0")])


def solved(cs, settings=None):
    s = sm.BatchSolver(cs["n"], 2 * cs["n"], B, n_plants=cs["k"], settings=settings)
    set_up(s, cs, operators=False)
    s.update_lin_cost(cs["q"])
    s.update_upper_bound(cs["u"])
    s.solve()
    return s


def run2(s, cs):
    """Two control steps of the receding-horizon stream from the case's X, U; returns the final (X, U)."""
    import torch

    Xd, Ud = _dev(cs["X"]), _dev(cs["U"])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    s.mpc_run_device(Xd.data_ptr(), Ud.data_ptr(), 0.5, 2, 7, 0, 0, 0.01, side.cuda_stream)
    side.synchronize()
    return Xd.cpu().numpy(), Ud.cpu().numpy()


def step_and_run(s, cs):
    """Operators and plant of the case, one control step, then a 2-step run: everything a caller can read."""
    set_up(s, cs)
    s.mpc_set_plant(cs["plant"]["Ad"][0], cs["plant"]["Bd"][0])
    U1 = s.mpc_step(cs["X"], cs["U"], 0.5)
    step = (U1, *results(s))
    Xr, Ur = run2(s, cs)
    return step + (Xr, Ur, *results(s), *s.stream_counters())


@pytest.mark.parametrize("stream", ["graph", "default"])
def test_operators_and_plant_of_another_nx(plant, stream, monkeypatch):
    """mpcq_mpc_set_operators and mpcq_mpc_set_plant with nx = 2, a step and a 2-step run, then the same with
    nx = 4 on the same context: the operator, X staging and plant buffers are freed and allocated again.  With
    MPCQ_STREAM=graph the run replays a captured step, which must be captured again on the new buffers."""
    if stream == "graph":
        monkeypatch.setenv("MPCQ_STREAM", "graph")
    c2, c4 = case(plant, 2), case(plant, 4)
    s = sm.BatchSolver(N, 2 * N, B)
    first = step_and_run(s, c2)
    assert stream != "graph" or s.stream_path() == "graph"
    got = step_and_run(s, c4)
    fresh = sm.BatchSolver(N, 2 * N, B)
    want = step_and_run(fresh, c4)
    same_bits(got, want, f"nx 2 -> 4, {stream}")
    assert np.all(want[3] == sm.SOLVED) and np.all(first[3] == sm.SOLVED)  # (the step's status)
    assert not np.array_equal(first[0], want[0])  # (the two plants' moves differ: the comparison can fail)


def test_step_reference_buffer_grows(plant):
    """mpcq_mpc_step_ref (host form) with ref_stride = 0, then with ref_stride = n: the staging buffer grows from
    one row to B rows between two warm-started steps."""
    cs = case(plant, 4)
    rng = np.random.default_rng(3)
    shared_ref, refs = rng.uniform(0.2, 0.8, N), rng.uniform(0.2, 0.8, (B, N))
    s, fresh = sm.BatchSolver(N, 2 * N, B), sm.BatchSolver(N, 2 * N, B)
    set_up(s, cs)
    set_up(fresh, cs)
    U1 = s.mpc_step_ref(cs["X"], cs["U"], shared_ref)  # one row
    W1 = fresh.mpc_step_ref(cs["X"], cs["U"], np.tile(shared_ref, (B, 1)))  # B rows from the start
    same_bits((U1, *results(s)), (W1, *results(fresh)), "first step")
    U2 = s.mpc_step_ref(cs["X"], U1, refs)  # grows
    W2 = fresh.mpc_step_ref(cs["X"], W1, refs)
    same_bits((U2, *results(s)), (W2, *results(fresh)), "second step")
    assert not np.array_equal(U1, U2)


@pytest.mark.parametrize("n_plants", [1, B])
def test_data_gradient_staging_grows(plant, n_plants):
    """mpcq_sensitivity_data_device asking for gP (the shared plant's partial sums, or nothing, in the context's
    staging), then mpcq_sensitivity_data (host form) asking for gP and gA as well: the staging grows."""
    cs = case(plant, 4, n_plants)
    s, fresh = solved(cs), solved(cs)
    gP = _dev(np.zeros((n_plants, N, N) if n_plants > 1 else (N, N)))
    s.sensitivity_data_device(gP_ptr=gP.data_ptr())
    got, want = s.sensitivity_data(), fresh.sensitivity_data()
    same_bits(got, want, "host form after the device form")
    same_bits([gP.cpu().numpy()], [want[3]], "gP of the device form")
    same_bits(results(s), results(fresh), "results")
    assert np.all(want[6] >= 0) and np.abs(want[3]).max() > 0  # (every QP SOLVED, a gradient to compare)


def _mimo_plants(nu, seed):
    """B random stable plants of 3 states, nu inputs, 2 outputs, their shared weights, states and previous moves."""
    nx, ny = 3, 2
    rng = np.random.default_rng(seed)
    Ad = np.empty((B, nx, nx))
    for b in range(B):
        M = rng.normal(size=(nx, nx))
        Ad[b] = 0.9 * M / np.abs(np.linalg.eigvals(M)).max()
    sh = {"Cd": rng.normal(size=(ny, nx)), "Q": np.diag([2.0, 0.5]), "R": np.diag(np.linspace(0.3, 0.1, nu)),
          "RD": np.diag(np.linspace(1.0, 0.8, nu)), "K": 0.5 * rng.normal(size=(nu, nx)), "K0": np.eye(nu),
          "w0": np.linspace(0.8, 1.2, nu)}
    arrays = [Ad, rng.normal(size=(B, nx, nu))] + [np.broadcast_to(sh[k], (B,) + sh[k].shape)
                                                     for k in ("Cd", "Q", "R", "RD", "K", "K0", "w0")]
    return dict(nx=nx, nu=nu, ny=ny, arrays=[_dev(a) for a in arrays], X=rng.normal(size=(B, nx)),
                U=0.2 * rng.normal(size=(B, nu)))


def _mimo_step(s, p, horizon):
    import torch

    stream = torch.cuda.current_stream().cuda_stream
    s.mimo_setup_plants_device(p["nx"], p["nu"], p["ny"], horizon, *[a.data_ptr() for a in p["arrays"]], stream=stream)
    Xd, Ud = _dev(p["X"]), _dev(p["U"])
    s.mimo_step_device(Xd.data_ptr(), Ud.data_ptr(), 0, stream)
    torch.cuda.synchronize()
    return (Ud.cpu().numpy(), *results(s))


def test_mimo_blocks_of_another_shape():
    """mpcq_mimo_setup_plants_device twice on one context, (N, n_u) = (4, 2) then (2, 4) of the same n = 8, a step
    after each: the operator blocks are released and allocated again."""
    p2, p4 = _mimo_plants(2, 21), _mimo_plants(4, 22)
    s, fresh = sm.BatchSolver(8, 16, B, n_plants=B), sm.BatchSolver(8, 16, B, n_plants=B)
    first = _mimo_step(s, p2, 4)
    got, want = _mimo_step(s, p4, 2), _mimo_step(fresh, p4, 2)
    same_bits(got, want, "(4, 2) -> (2, 4)")
    assert np.all(first[3] == sm.SOLVED) and np.all(want[3] == sm.SOLVED)


def test_destroyed_contexts_give_their_memory_back(plant, monkeypatch):
    """200 contexts of batch 8, created, taken through one solve and destroyed: a shared plant on the tile path, one
    plant per QP, a MIMO-only shape (n = 36) and a shared plant with settings.polish.  The device's free memory
    (torch.cuda.mem_get_info) afterwards is within one allocator granule (2 MiB) of what it was before: a buffer
    that mpcq_destroy forgot would cost 200 (or 50) times its size.  One context of each kind runs first, so that
    the runtime's own one-off allocations (code objects, staging) are not counted.  Measured on an MI355X: 0 B lost,
    and 0 B as well on the commit before the buffers had an owner (its hand-kept free list was complete)."""
    import torch

    monkeypatch.setenv("MPCQ_KERNEL", "tile")
    tile, per, small, mimo = case(plant, 4, 1, 20), case(plant, 4, B), case(plant, 4), _mimo_plants(4, 23)
    polish = sm.default_settings(polish=1)

    def one(kind):
        if kind == 0:
            s = solved(tile)
            assert s.path()[0] == "tile"
        elif kind == 1:
            s = solved(per)
        elif kind == 2:
            s = sm.BatchSolver(36, 72, B, n_plants=B)
            _mimo_step(s, mimo, 9)
        else:
            s = solved(small, settings=polish)
            assert np.all(s.polish_info()[0] != 0)
        assert np.all(s.info()[0] == sm.SOLVED), kind
        s.close()

    for kind in range(4):
        one(kind)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for i in range(200):
        one(i % 4)
    torch.cuda.synchronize()
    lost = before - torch.cuda.mem_get_info()[0]
    print(f"free device memory: {before} B before, {lost} B fewer after 200 contexts")
    assert lost <= 2 << 20, lost

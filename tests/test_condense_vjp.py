"""The condensing's vector-Jacobian product on the device (mpcq_condense_vjp*, solvempc_amd/csrc/mpcq_condense_vjp.hip)
and the layer built on it (diff.mpc_plant_solution), against the CPU references of
tests/test_condense_vjp_ref.py.

The kernel is compared with the autograd VJP of the restated condensing within 1e-12 of max(1, |reference|_inf) per
array: the condensing's own tolerance (the sums are O(N^2) fp64 terms).  The layer's plant gradients are compared
with that reference applied to the same solver's ``sensitivity_data`` outputs, and end to end with central
differences of further device solves within 100 x the error the CPU reference shows for the same quotient."""
import functools
import itertools

import numpy as np
import pytest
import torch

import solvempc_amd as sm
from solvempc_amd import diff, workload

import test_condense_vjp_ref as cref
import test_polish as tp
import test_sensitivity as ts
import test_sensitivity_data_ref as dref
import test_sensitivity_ref as ref

pytestmark = pytest.mark.gpu

PLANT_KEYS, COT_KEYS = cref.PLANT_KEYS, cref.COT_KEYS
ERR_ARG = sm._capi.MPCQ_ERR_ARG
TOL = 1e-12
KMAX = 67
N_PLANTS = (1, 3, 64, 67)
HORIZONS = (1, 5, 17, 20, 32)


def _s_rows(N):
    return (0, 3, 10, N + 5)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _device_vjp(plants, cots, N, s_rows, k, outputs=PLANT_KEYS, stream=None):
    """mpcq_condense_vjp_device on the first k plants; returns {key: numpy} for ``outputs`` and the sentinel-filled
    buffers of the others (which the call must leave alone)."""
    nx = plants["Ad"].shape[1]
    pl = [_cuda(plants[key][:k]) for key in PLANT_KEYS]
    ct = [None if cots.get(key) is None else _cuda(cots[key][:k]) for key in COT_KEYS]
    out = {key: torch.full(tuple(np.shape(plants[key][:k])), 7.0, dtype=torch.float64, device="cuda")
           for key in PLANT_KEYS}
    sm.condense_vjp_device(k, nx, N, s_rows, [t.data_ptr() for t in pl], [0 if t is None else t.data_ptr() for t in ct],
                           [out[key].data_ptr() if key in outputs else 0 for key in PLANT_KEYS], stream)
    torch.cuda.synchronize()
    res = {key: v.cpu().numpy() for key, v in out.items()}
    for key in PLANT_KEYS:
        if key not in outputs:
            assert (res[key] == 7.0).all(), key
    return res


def _assert_close(got, want, label, keys=PLANT_KEYS):
    worst = 0.0
    for key in keys:
        err = cref._rel(got[key], want[key])
        worst = max(worst, err)
        assert np.isfinite(got[key]).all() and err <= TOL, (label, key, err)
    return worst


# ----------------------------------------------------------------------------- 1. the kernel against the reference
@functools.lru_cache(maxsize=None)
def _golden_family():
    """The golden plant and KMAX - 1 seeded relative perturbations of it (workload.randomized_plants, as config 3
    draws them)."""
    plant = workload.reference_plant()
    Ad, Bd = workload.randomized_plants(plant, 3, 0, KMAX - 1)
    return cref._stack_plants(plant, KMAX, np.concatenate([plant["Ad"][None], Ad]), np.concatenate([plant["Bd"][None], Bd]))


@functools.lru_cache(maxsize=None)
def _synthetic_family(nx, k=3):
    rng = np.random.default_rng(900 + nx)
    return {"Ad": rng.normal(size=(k, nx, nx)) * 0.5 / np.sqrt(nx), "Bd": rng.normal(size=(k, nx)),
            "Cd": rng.normal(size=(k, nx)), "K": rng.normal(size=(k, nx)), "Q": rng.uniform(0.5, 2.0, size=k),
            "R": rng.uniform(0.5, 2.0, size=k), "RD": rng.uniform(0.5, 2.0, size=k)}


@functools.lru_cache(maxsize=None)
def _family_reference(nx, N, s_rows):
    """(plants, cotangents, reference VJP) of a family at one (N, s_rows): computed once, shared, left unchanged."""
    plants = _golden_family() if nx == 4 else _synthetic_family(nx)
    k = len(plants["Ad"])
    cots = cref._random_cotangents(7000 + 100 * N + s_rows + nx, N, nx, k)
    return plants, cots, cref._vjp_torch_batch(plants, cots, N, s_rows)


@pytest.mark.parametrize("N", HORIZONS)
def test_kernel_matches_reference_golden_family(N):
    """n_plants 1, 3, 64 (one full wave of blocks' worth), 67; every horizon from 1 to the kernel's capacity 32; no K
    row, a few, the reference's 10, and more rows than the horizon."""
    for s_rows in _s_rows(N):
        plants, cots, want = _family_reference(4, N, s_rows)
        for k in N_PLANTS:
            got = _device_vjp(plants, cots, N, s_rows, k)
            worst = _assert_close(got, {key: want[key][:k] for key in PLANT_KEYS}, (N, s_rows, k))
            print(f"N={N} s_rows={s_rows} n_plants={k}: worst relative error {worst:.1e}")


@pytest.mark.parametrize("nx", [1, 8])
def test_kernel_matches_reference_other_state_dimensions(nx):
    for N in HORIZONS:
        for s_rows in _s_rows(N)[1::2]:
            plants, cots, want = _family_reference(nx, N, s_rows)
            worst = _assert_close(_device_vjp(plants, cots, N, s_rows, 3), want, (nx, N, s_rows))
            print(f"nx={nx} N={N} s_rows={s_rows}: worst relative error {worst:.1e}")


# ----------------------------------------------------------------------------- 2. NULL handling, determinism
def test_null_cotangents_and_outputs_and_host_form():
    N, s_rows, k = 17, 3, 3
    plants, cots, _ = _family_reference(4, N, s_rows)
    full = _device_vjp(plants, cots, N, s_rows, k)
    again = _device_vjp(plants, cots, N, s_rows, k)
    for key in PLANT_KEYS:
        assert np.array_equal(full[key], again[key]), key
    # each cotangent alone
    sub = {key: plants[key][:k] for key in PLANT_KEYS}
    for key in COT_KEYS:
        one = {key: cots[key][:k]}
        _assert_close(_device_vjp(plants, one, N, s_rows, k), cref._vjp_torch_batch(sub, one, N, s_rows), key)
    # any subset of the outputs
    for r in range(1, len(PLANT_KEYS)):
        for outputs in itertools.combinations(PLANT_KEYS, r):
            got = _device_vjp(plants, cots, N, s_rows, k, outputs)
            for key in outputs:
                assert np.array_equal(got[key], full[key]), (outputs, key)
    # the host form
    host = sm.condense_vjp(sub, {key: cots[key][:k] for key in COT_KEYS}, N, s_rows)
    for key in PLANT_KEYS:
        assert host[key].shape == full[key].shape and np.array_equal(host[key], full[key]), key
    one = sm.condense_vjp(sub, {"Fr": cots["Fr"][:k], "P": None}, N, s_rows)
    got = _device_vjp(plants, {"Fr": cots["Fr"]}, N, s_rows, k)
    for key in PLANT_KEYS:
        assert np.array_equal(one[key], got[key]), key


# ----------------------------------------------------------------------------- 3. refusals
def test_refusals():
    k, nx, N = 3, 4, 20
    big = dict(N=33, nx=9)  # (every buffer has room for the largest shape a call below names)
    pl = [torch.full((k * big["nx"] * big["nx"],), 0.5, dtype=torch.float64, device="cuda") for _ in PLANT_KEYS]
    ct = [torch.full((k * 2 * big["N"] * big["N"],), 1.0, dtype=torch.float64, device="cuda") for _ in COT_KEYS]
    out = [torch.full((k * big["nx"] * big["nx"],), 7.0, dtype=torch.float64, device="cuda") for _ in PLANT_KEYS]
    ptr = lambda ts_, drop=(): [0 if i in drop else t.data_ptr() for i, t in enumerate(ts_)]

    def call(k=k, nx=nx, N=N, s_rows=10, pdrop=(), cdrop=(), odrop=(), stream=None):
        sm.condense_vjp_device(k, nx, N, s_rows, ptr(pl, pdrop), ptr(ct, cdrop), ptr(out, odrop), stream)

    every = tuple(range(7))
    for kw in (dict(N=0), dict(N=33), dict(nx=0), dict(nx=9), dict(s_rows=-1), dict(k=0), dict(cdrop=every),
               dict(odrop=every)) + tuple(dict(pdrop=(i,)) for i in every):
        ts._raises(ERR_ARG, call, **kw)
    host = {key: np.zeros(s) for key, s in zip(PLANT_KEYS, ((k, nx, nx), (k, nx), (k, nx), (k, nx), (k,), (k,), (k,)))}
    with pytest.raises(sm.MpcqError) as e:
        sm.condense_vjp(host, {}, N)
    assert e.value.code == ERR_ARG
    with pytest.raises(sm.MpcqError) as e:
        sm.condense_vjp(host, {"Fu": np.zeros((k, 33))}, 33)
    assert e.value.code == ERR_ARG
    # a stream under graph capture: refused, nothing recorded
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        ts._raises(ERR_ARG, call, stream=side.cuda_stream)
    torch.cuda.synchronize()
    for t in out:
        assert (t == 7.0).all()
    call()  # (and served afterwards)
    torch.cuda.synchronize()
    for t, cnt in zip(out, (k * nx * nx, k * nx, k * nx, k * nx, k, k, k)):
        assert not (t[:cnt] == 7.0).any() and (t[cnt:] == 7.0).all()


# ----------------------------------------------------------------------------- 4. the layer, one plant per QP
def _plant_tensors(plants, grad=True):
    return [_cuda(plants[key]).requires_grad_(grad) for key in PLANT_KEYS]


def _layer_problem(B=8, N=20):
    plant = workload.reference_plant()
    _, X, U, _, _ = tp._problem(plant, N, B, 1)
    return plant, X, U, cref._seeded_ref(B, N), ref._cotangents(1, B, N)


def _bits(words, m):
    return ((words[:, None] >> np.arange(m, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def _per_qp_cotangents(out, x, y, X, U, rf):
    """Per-QP operator cotangents from one sensitivity_data call's per-QP outputs: gq, gu, the masks and the
    returned x, y (gP, gA by tests/test_sensitivity_data_ref.py's formula; QPs with n_active = -1 contribute zeros)."""
    gq, gl, gu, _, _, act, na = out
    m = gl.shape[1]
    keep = (na >= 0)[:, None]
    active = _bits(act[:, 0], m) | _bits(act[:, 1], m)
    xk, yk = np.where(keep, x, 0.0), np.where(keep & active, y, 0.0)
    gP, gA = dref._formula_batch(gq, gl + gu, xk, yk)
    return {"P": gP, "A": gA, "Fx": gq[:, :, None] * X[:, None, :], "Fu": gq * U[:, None],
            "Fr": gq[:, :, None] * rf[:, None, :], "Sbar": gu[:, :, None] * X[:, None, :], "Ku": gu * U[:, None]}


def test_per_plant_layer_matches_reference_and_device_differences():
    """N = 20, eight distinct plants, settings.polish = 1.  The seven plant gradients of one backward pass against
    the reference VJP applied to the same solver's sensitivity_data outputs and the test's own operator cotangents
    (TOL).  Then the derivative along cref._plant_directions against central differences (h = 1e-5) of two more
    polished device solves, on the QPs the CPU reference kept that are SOLVED and polished at both ends.  Tolerance:
    100 x cref._plant_directional_fd()["err"] (1.3e-9, so 1.3e-7) relative to max(1, |derivative|): the reference's
    own error, nothing the device returns."""
    B, N, s_rows = 8, 20, 10
    plant, X, U, rf, g = _layer_problem(B, N)
    Ad, Bd = workload.randomized_plants(plant, 3, 0, B)
    plants = cref._stack_plants(plant, B, Ad, Bd)
    d = cref._plant_directional_fd()
    dv = cref._plant_directions(plants)
    h = cref.H
    G, Xd, Ud, rd = _cuda(g), _cuda(X), _cuda(U), _cuda(rf)

    def solve(pl, grad):
        s = sm.BatchSolver(N, 2 * N, B, n_plants=B, settings=sm.default_settings(polish=1))
        t = _plant_tensors(pl, grad)
        x, status = diff.mpc_plant_solution(s, *t, Xd, Ud, rd, s_rows=s_rows)
        return s, t, x, status

    s, t, x, status = solve(plants, True)
    assert np.array_equal(Ud.cpu().numpy(), U)  # (the caller's U is left alone)
    (x * G).sum().backward()
    out = s.sensitivity_data(g)
    xs, ys = s.solution(), s.dual()
    sp0 = s.polish_info()[0]
    assert np.array_equal(x.detach().cpu().numpy(), xs)
    want = cref._vjp_torch_batch(plants, _per_qp_cotangents(out, xs, ys, X, U, rf), N, s_rows)
    got = {key: tt.grad.cpu().numpy() for key, tt in zip(PLANT_KEYS, t)}
    for key in PLANT_KEYS:
        assert got[key].shape == plants[key].shape, key
    worst = _assert_close(got, want, "per-plant layer")
    print(f"per-plant layer: plant gradients vs the reference VJP of the call's own cotangents {worst:.1e}; "
          f"active rows {sorted(set(out[6].tolist()))}")
    assert (out[6] > 0).any() and all(np.abs(got[key]).max() > 0 for key in PLANT_KEYS)
    # backward after a later solve is refused
    x2, _ = diff.mpc_plant_solution(s, *t, Xd, Ud, rd, s_rows=s_rows, setup=False)
    s.solve()
    with pytest.raises(RuntimeError, match="solved again"):
        (x2 * G).sum().backward()
    s.close()

    deriv = sum((got[key] * dv[key]).reshape(B, -1).sum(axis=1) for key in PLANT_KEYS)
    vals, ok = [], (status.cpu().numpy() == sm.SOLVED) & (sp0 == 1)
    for sgn in (1.0, -1.0):
        s2, _, xm, st2 = solve({key: plants[key] + sgn * h * dv[key] for key in PLANT_KEYS}, False)
        ok &= (st2.cpu().numpy() == sm.SOLVED) & (s2.polish_info()[0] == 1)
        s2.close()
        vals.append((xm * G).sum(dim=1).cpu().numpy())
    fd = (vals[0] - vals[1]) / (2 * h)
    keep = d["keep"] & ok
    tol = 100.0 * d["err"]
    err = np.abs(deriv - fd) / np.maximum(1.0, np.abs(deriv))
    print(f"per-plant layer: directional derivative vs device differences on {int(keep.sum())} of {B} QPs: "
          f"{err[keep].max():.2e} (tolerance {tol:.1e}); per QP {np.array2string(err, precision=1)}; "
          f"|derivative| {np.array2string(np.abs(deriv), precision=2)}")
    assert keep.sum() >= 0.9 * d["keep"].sum()
    assert err[keep].max() <= tol


@pytest.mark.parametrize("n_plants", [1, 8])
def test_layer_gradients_of_the_step_data(n_plants):
    """X, U and ref: mpc_solution's chain rule, with the operators of solvempc_amd.condense, on the same solver's
    sensitivity outputs (TOL); only the gradients asked for are returned."""
    B, N, s_rows = 8, 20, 10
    plant, X, U, rf, g = _layer_problem(B, N)
    Ad, Bd = workload.randomized_plants(plant, 3, 0, n_plants)
    plants = cref._stack_plants(plant, n_plants, Ad, Bd)
    s = sm.BatchSolver(N, 2 * N, B, n_plants=n_plants)
    t = _plant_tensors(plants, False)
    t[0].requires_grad_(True)
    Xd, Ud, rd = (_cuda(v).requires_grad_(True) for v in (X, U, rf))
    x, _ = diff.mpc_plant_solution(s, *t, Xd, Ud, rd, s_rows=s_rows)
    (x * _cuda(g)).sum().backward()
    gq, _, gu, _ = s.sensitivity(g)
    s.close()
    ops = sm.condense(plants, N, s_rows)
    ops = {key: np.broadcast_to(v, (B,) + v.shape[1:]) for key, v in ops.items()}
    want = {"X": np.einsum("bij,bi->bj", ops["Fx"], gq) + np.einsum("bij,bi->bj", ops["Sbar"], gu),
            "U": (ops["Fu"] * gq).sum(axis=1) + (ops["Ku"] * gu).sum(axis=1), "ref": np.einsum("bit,bi->bt", ops["Fr"], gq)}
    got = {"X": Xd.grad.cpu().numpy(), "U": Ud.grad.cpu().numpy(), "ref": rd.grad.cpu().numpy()}
    _assert_close(got, want, "step data", ("X", "U", "ref"))
    assert t[0].grad is not None and all(v.grad is None for v in t[1:])


# ----------------------------------------------------------------------------- 5. the layer, a shared plant
def _batched_vjp(plant, cots, N, s_rows, chunk=1024):
    """The reference VJP of every QP's cotangents at one plant: torch autograd of cref._condense_torch with batched
    cotangents (is_grads_batched), {key: (B, ...)}."""
    pl = cref._as_torch(plant, grad=True)
    ops = cref._condense_torch(pl, N, s_rows)
    B = len(cots["P"])
    res = {key: [] for key in PLANT_KEYS}
    for lo in range(0, B, chunk):
        grads = torch.autograd.grad([ops[key] for key in COT_KEYS], [pl[key] for key in PLANT_KEYS],
                                    grad_outputs=[torch.from_numpy(np.ascontiguousarray(cots[key][lo:lo + chunk]))
                                                  for key in COT_KEYS], is_grads_batched=True, retain_graph=True)
        for key, gr in zip(PLANT_KEYS, grads):
            res[key].append(gr.numpy())
    return {key: np.concatenate(v) for key, v in res.items()}


@pytest.mark.parametrize("kern,B,dtype,polish", [("wave", 64, "f64", 0), ("tile", 8192, "f64", 0),
                                                  ("tile", 8192, "mixed", 1)])
def test_shared_plant_layer_is_the_sum_over_the_batch(plant, monkeypatch, kern, B, dtype, polish):
    """One plant shared by the batch: the plant gradients equal the sum over the QPs of the reference VJP of each
    QP's cotangents (from the same solver's sensitivity_data outputs).  Tolerance: 100 x the error the CPU reference
    shows for the same comparison, the numpy sum of the per-QP torch VJPs against the torch VJP of the summed
    cotangents, relative to max(1, |.|_inf) per array."""
    monkeypatch.setenv("MPCQ_KERNEL", kern)
    N, s_rows = 20, 10
    _, X, U, _, _ = tp._problem(plant, N, B, 1)
    rf, g = cref._seeded_ref(B, N), ref._cotangents(1, B, N)
    plants = cref._stack_plants(plant, 1)
    s = sm.BatchSolver(N, 2 * N, B, dtype=dtype, settings=sm.default_settings(polish=polish))
    t = _plant_tensors(plants)
    x, status = diff.mpc_plant_solution(s, *t, _cuda(X), _cuda(U), _cuda(rf), s_rows=s_rows)
    assert s.path()[0] == kern
    (x * _cuda(g)).sum().backward()
    out = s.sensitivity_data(g)
    xs, ys = s.solution(), s.dual()
    s.close()
    got = {key: tt.grad.cpu().numpy()[0] for key, tt in zip(PLANT_KEYS, t)}
    cots = _per_qp_cotangents(out, xs, ys, X, U, rf)
    per_qp = _batched_vjp(plant, cots, N, s_rows)
    want = {key: per_qp[key].sum(axis=0) for key in PLANT_KEYS}
    summed = cref._vjp_torch(plant, {key: cots[key].sum(axis=0) for key in COT_KEYS}, N, s_rows)
    ref_err = max(cref._rel(want[key], summed[key]) for key in PLANT_KEYS)
    err = {key: cref._rel(got[key], want[key]) for key in PLANT_KEYS}
    print(f"{kern} B={B} {dtype} polish={polish}: {int((out[6] >= 0).sum())} QPs in the sums; CPU reference's own error "
          f"{ref_err:.2e} (tolerance {100 * ref_err:.1e}); device vs sum of per-QP VJPs "
          + ", ".join(f"{key} {e:.1e}" for key, e in err.items()))
    assert (status.cpu().numpy() == sm.SOLVED).mean() > 0.9 and (out[6] > 0).any()
    for key in PLANT_KEYS:
        assert np.isfinite(got[key]).all() and np.abs(got[key]).max() > 0, key
        assert err[key] <= 100.0 * ref_err, (key, err[key], ref_err)


# ----------------------------------------------------------------------------- 6. side effects
def test_setup_false_after_a_setup_gives_the_same_solution():
    B, N, s_rows = 8, 20, 10
    plant, X, U, rf, _ = _layer_problem(B, N)
    Ad, Bd = workload.randomized_plants(plant, 3, 0, B)
    plants = cref._stack_plants(plant, B, Ad, Bd)
    Xd, Ud, rd = _cuda(X), _cuda(U), _cuda(rf)
    a = sm.BatchSolver(N, 2 * N, B, n_plants=B)
    xa, sa = diff.mpc_plant_solution(a, *_plant_tensors(plants, False), Xd, Ud, rd, s_rows=s_rows)
    b = sm.BatchSolver(N, 2 * N, B, n_plants=B)
    t = _plant_tensors(plants, False)
    b.mpc_setup_plants_device(4, s_rows, *[v.data_ptr() for v in t])
    xb, sb = diff.mpc_plant_solution(b, *t, Xd, Ud, rd, s_rows=s_rows, setup=False)
    assert torch.equal(xa, xb) and torch.equal(sa, sb) and (sa.cpu().numpy() == sm.SOLVED).all()
    a.close()
    b.close()


def test_a_vjp_call_changes_no_later_solve(plant):
    """step, condense_vjp_device, warm-started second step == the same two steps without the call, bit for bit: the
    call is stateless and touches no context."""
    N, B, s_rows = 20, 512, 10
    ops, X, U, _, _ = tp._problem(plant, N, B, 1)
    X2 = X * 0.9 + 0.01
    plants, cots, _ = _family_reference(4, N, s_rows)

    def run(call):
        s = ts._mpc_solver(ops, N, B, operators=True)
        Xd, X2d, Ud = (torch.from_numpy(a.copy()).cuda() for a in (X, X2, U))
        s.mpc_step_device(Xd.data_ptr(), Ud.data_ptr(), 0.0)
        if call:
            got = _device_vjp(plants, cots, N, s_rows, 3)
            assert all(np.abs(got[key]).max() > 0 for key in PLANT_KEYS)
        s.mpc_step_device(X2d.data_ptr(), Ud.data_ptr(), 0.0)
        torch.cuda.synchronize()
        res = [Ud.cpu().numpy(), s.solution(), *s.info()]
        s.close()
        return res

    for p, q in zip(run(False), run(True)):
        assert np.array_equal(p, q)

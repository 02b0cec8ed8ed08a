"""The MIMO step's gradients with respect to the plant data on the device (mpcq_mimo_plant_vjp*,
diff.mimo_plant_solution; solvempc_amd/csrc/mpcq_mimo_plant_vjp.hip) against the CPU references of
tests/test_mimo_plant_vjp_ref.py, on the families of tests/test_mimo_sensitivity_ref.py and the cached device
results of tests/test_mimo_sensitivity.py.

* Against the reference: the nine outputs equal ``_closed_form_factored`` applied to the device's own gq, gu, x, y,
  with the active set taken as the support of gu under a random g, within max(1e-12, 100 E_f) relative to
  max(1, |reference|_inf) per array (E_f: the factored form's disagreement with autograd, from the CPU file).
* g = NULL is g = e_0 bit for bit; two calls give identical bits; the host-memory form has the device form's bits;
  each output asked for alone has the bits of the all-outputs call; a step after the call is bit-identical to the
  same step without it.
* After mimo_step_polish_device the reference at the polished x, y; unsolved QPs get zeros and n_active = -1; every
  refusal leaves the outputs untouched.
* diff.mimo_plant_solution: plant gradients bit for bit the direct call's, dX, dU, dyref those of
  diff.mimo_solution, setup=False, the solve_count guard, and the directional derivative of polished solves
  against central differences of two more device solves within 100 x the CPU file's own quotient error."""
import functools

import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import workload

import test_mimo_plant_vjp_ref as pref
from test_mimo_sensitivity import _Ctx, _dev, _device
from test_mimo_sensitivity_ref import _inputs

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_ORDER = sm._capi.MPCQ_ERR_ARG, sm._capi.MPCQ_ERR_ORDER
KEYS = pref.PLANT_KEYS
FAMILIES = ("R", "R-tight", "odd", "S", "Q", "Q32")


def _shapes(c):
    B, N, nx, nu, ny, n, m = c.dims
    return {"Ad": (B, nx, nx), "Bd": (B, nx, nu), "Cd": (B, ny, nx), "Q": (B, ny, ny), "R": (B, nu, nu),
            "RD": (B, nu, nu), "K": (B, nu, nx), "K0": (B, nu, nu), "w0": (B, nu)}


def _outputs(c, only=None):
    """Nine NaN-filled device outputs (None for those not in ``only``) and n_active filled with -7."""
    import torch

    outs = {k: (torch.full(s, np.nan, dtype=torch.float64, device="cuda:0") if only is None or k in only else None)
            for k, s in _shapes(c).items()}
    return outs, torch.full((c.dims[0],), -7, dtype=torch.int32, device="cuda:0")


def _call(c, g, U_prev=None, only=None, want_na=True):
    """mimo_plant_vjp_device on a host cotangent (or None): dict of numpy outputs (those asked for) and n_active."""
    import torch

    outs, na = _outputs(c, only)
    gd = _dev(g) if g is not None else None
    U_prev = c.U0 if U_prev is None else U_prev
    c.s.mimo_plant_vjp_device(gd.data_ptr() if gd is not None else 0, [k.data_ptr() for k in c.keep], c.X.data_ptr(),
                              U_prev.data_ptr(), c.yref.data_ptr() if c.yref is not None else 0,
                              [outs[k].data_ptr() if outs[k] is not None else 0 for k in KEYS],
                              na.data_ptr() if want_na else 0, c.stream)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in outs.items() if v is not None}
    res["n_active"] = na.cpu().numpy()
    return res


def _host_plants(c):
    return {k: t.cpu().numpy() for k, t in zip(KEYS, c.keep)}


def _reference(c, s_rows, gq, gu, x, y, U_prev=None):
    """_closed_form_factored per QP on the device's own gq, gu, x, y; the active set is the support of gu."""
    B, N, nx, nu, ny, n, m = c.dims
    plants = _host_plants(c)
    X, U = c.X.cpu().numpy(), (c.U0 if U_prev is None else U_prev).cpu().numpy()
    yref = c.yref.cpu().numpy() if c.yref is not None else np.zeros(ny)
    per = [pref._closed_form_factored(pref._one(plants, b), N, s_rows, gq[b], gu[b], x[b], np.where(gu[b] != 0, y[b], 0.0),
                                      X[b], U[b], yref) for b in range(B)]
    return {k: np.stack([p[k] for p in per]) for k in KEYS}


def _compare(label, got, want, tol):
    """Per array: max |got - want| relative to max(1, |want|_inf), asserted; the worst per-QP figure is printed too."""
    worst = worst_qp = 0.0
    for k in KEYS:
        err = pref._rel(got[k], want[k])
        B = len(want[k])
        per_qp = max(pref._rel(got[k][b], want[k][b]) for b in range(B))
        worst, worst_qp = max(worst, err), max(worst_qp, per_qp)
        assert got[k].shape == want[k].shape, k
        assert err <= tol, (label, k, err, tol)
    print(f"{label}: device against the factored reference, worst per array {worst:.2e} (per QP {worst_qp:.2e}), "
          f"tolerance {tol:.1e}")


def _tol(name, s_rows=None):
    return max(1e-12, 100.0 * pref._factored_error(pref._family_shape(name), s_rows))


@functools.lru_cache(maxsize=None)
def _family_call(name):
    """The cached context of tests/test_mimo_sensitivity.py's ``_device`` and the calls the tests below compare."""
    d = _device(name)
    c = d["c"]
    g = np.ascontiguousarray(d["g"][:, 0])
    return dict(c=c, g=g, full=_call(c, g), full2=_call(c, g), e0=_call(c, None),
                e0x=_call(c, np.broadcast_to(np.eye(c.dims[5])[0], (c.dims[0], c.dims[5])).copy()))


@pytest.mark.parametrize("name", FAMILIES)
def test_against_the_factored_reference(name):
    d, f = _device(name), _family_call(name)
    c = f["c"]
    gq, gu, na = d["multi"]
    assert np.all(d["st"] == sm.SOLVED)
    got = f["full"]
    assert np.array_equal(got["n_active"], na) and np.all(na >= 0)
    want = _reference(c, _inputs(name)["s_rows"], gq[:, 0], gu[:, 0], c.s.solution(), c.s.dual())
    _compare(f"{name} (n_active {na.min()}..{na.max()})", got, want, _tol(name))
    # every gradient is exercised somewhere (K is zero for the quad-rotor and its gradient need not be)
    assert all(np.abs(got[k]).max() > 0 for k in ("Ad", "Bd", "Cd", "Q", "R", "RD"))
    if na.max() > 0:
        assert all(np.abs(got[k]).max() > 0 for k in ("K0", "w0"))


@pytest.mark.parametrize("case", ["s_rows 0", "s_rows N+5", "batch 1"])
def test_r_shape_variants(case):
    name = "R"
    f = _inputs(name)
    N = f["N"]
    s_rows = {"s_rows 0": 0, "s_rows N+5": N + 5}.get(case, f["s_rows"])
    c = _Ctx(name, B=1 if case == "batch 1" else None)
    B, N, nx, nu, ny, n, m = c.dims
    if s_rows != f["s_rows"]:
        c.s.mimo_setup_plants_device(nx, nu, ny, s_rows, *[k.data_ptr() for k in c.keep], stream=c.stream)
    c.step()
    g = np.random.default_rng(21).normal(size=(B, n))
    gq, gu, na = c.s.mimo_sensitivity(g)
    got = _call(c, g)
    assert np.array_equal(got["n_active"], na) and np.all(na >= 0)
    want = _reference(c, s_rows, gq[:, 0], gu[:, 0], c.s.solution(), c.s.dual())
    _compare(f"R, {case}", got, want, _tol(name, None if case == "batch 1" else s_rows))
    if case == "s_rows 0":
        assert np.all(got["K"] == 0)


@pytest.mark.parametrize("name", FAMILIES)
def test_null_g_is_e0_and_two_calls_give_identical_bits(name):
    f = _family_call(name)
    for k in KEYS + ("n_active",):
        assert np.array_equal(f["e0"][k], f["e0x"][k]), k
        assert np.array_equal(f["full"][k], f["full2"][k]), k
        assert not np.isnan(f["full"][k]).any(), k


@pytest.mark.parametrize("name", ["R", "S"])
def test_host_form_has_the_bits_of_the_device_form(name):
    """mpcq_mimo_plant_vjp (host arrays in and out) against the device form, with a cotangent and with g = NULL;
    family S has no yref (NULL)."""
    f = _family_call(name)
    c = f["c"]
    yref = c.yref.cpu().numpy() if c.yref is not None else None
    for g, want in ((f["g"], f["full"]), (None, f["e0"])):
        got = c.s.mimo_plant_vjp(_host_plants(c), c.X.cpu().numpy(), c.U0.cpu().numpy(), yref, g)
        assert set(got) == set(KEYS) | {"n_active"}
        for k in KEYS + ("n_active",):
            assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("name", ["R", "Q"])
def test_each_output_alone_has_the_bits_of_the_full_call(name):
    f = _family_call(name)
    c = f["c"]
    for k in KEYS:
        one = _call(c, f["g"], only=(k,), want_na=False)
        assert set(one) == {k, "n_active"}
        assert np.array_equal(one[k], f["full"][k]), k
        assert np.all(one["n_active"] == -7)  # (not asked for: untouched)
    na = _call(c, f["g"], only=(), want_na=True)
    assert np.array_equal(na["n_active"], f["full"]["n_active"])


@pytest.mark.parametrize("name", ["R", "Q"])
def test_read_only_on_a_warm_started_context(name):
    res = []
    for call in (False, True):
        c = _Ctx(name, settings=sm.default_settings(warm_start=1))
        U = c.step()
        if call:
            _call(c, None)
            _call(c, np.random.default_rng(3).normal(size=(c.dims[0], c.dims[5])))
        U = c.step(U)
        st, it, rho = c.s.info()
        res.append((U.cpu().numpy(), c.s.solution(), c.s.dual(), st, it, rho))
    for a, b in zip(*res):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["R-tight", "Q"])
def test_after_a_polished_step(name):
    import torch

    c = _Ctx(name)
    B, N, nx, nu, ny, n, m = c.dims
    U = c.U0.clone()
    c.s.mimo_step_polish_device(c.X.data_ptr(), U.data_ptr(), c.yref.data_ptr() if c.yref is not None else 0, c.stream)
    torch.cuda.synchronize()
    sp = c.s.polish_info()[0]
    assert (sp == 1).any()
    g = np.random.default_rng(22).normal(size=(B, n))
    gq, gu, na = c.s.mimo_sensitivity(g)
    got = _call(c, g)
    assert np.array_equal(got["n_active"], na)
    want = _reference(c, _inputs(name)["s_rows"], gq[:, 0], gu[:, 0], c.s.solution(), c.s.dual())
    _compare(f"{name} after polish ({int((sp == 1).sum())} of {B} polished)", got, want, _tol(name))


@pytest.mark.parametrize("max_iter", [15, 100])
def test_unsolved_qps_get_zeros(max_iter):
    """Family Q as tests/test_mimo_sensitivity.py makes its unsolved QPs: max_iter = 15 leaves none SOLVED, max_iter =
    100 mixes SOLVED and SOLVED_INACCURATE ones; the unsolved get zeros and -1, the others their reference."""
    name = "Q"
    c = _Ctx(name, settings=sm.default_settings(max_iter=max_iter))
    B, N, nx, nu, ny, n, m = c.dims
    c.step()
    st, _, _ = c.s.info()
    g = np.random.default_rng(23).normal(size=(B, n))
    gq, gu, na = c.s.mimo_sensitivity(g)
    got = _call(c, g)
    bad = st != sm.SOLVED
    assert bad.all() if max_iter == 15 else (bad.any() and (~bad).any())
    assert np.array_equal(got["n_active"], na) and np.all(na[bad] == -1) and np.all(na[~bad] >= 0)
    for k in KEYS:
        assert np.all(got[k][bad] == 0), k
    if (~bad).any():
        want = _reference(c, _inputs(name)["s_rows"], gq[:, 0], gu[:, 0], c.s.solution(), c.s.dual())
        ok = np.flatnonzero(~bad)
        _compare(f"Q, max_iter {max_iter}: the {len(ok)} SOLVED QPs", {k: got[k][ok] for k in KEYS},
                 {k: want[k][ok] for k in KEYS}, _tol(name))


def _rc(fn, *args):
    with pytest.raises(sm.MpcqError) as e:
        fn(*args)
    return e.value.code


def test_refusals_write_nothing():
    import torch

    c = _Ctx("R")
    B, N, nx, nu, ny, n, m = c.dims
    outs, na = _outputs(c)
    g = _dev(np.ones((B, n)))
    plant = [k.data_ptr() for k in c.keep]
    grads = [outs[k].data_ptr() for k in KEYS]
    X, U, y = c.X.data_ptr(), c.U0.data_ptr(), c.yref.data_ptr()
    fn = c.s.mimo_plant_vjp_device
    # no step since the setup; no setup at all
    assert _rc(fn, g.data_ptr(), plant, X, U, y, grads, na.data_ptr(), c.stream) == ERR_ORDER
    with sm.BatchSolver(n, m, B, n_plants=B) as fresh:
        assert _rc(fresh.mimo_plant_vjp_device, g.data_ptr(), plant, X, U, y, grads, na.data_ptr(), c.stream) == ERR_ORDER
    # a context whose setup is not a MIMO one
    sp = workload.reference_plant()
    ops = oracle.condense(sp, n)
    with sm.BatchSolver(n, m, B) as gen:
        gen.setup(ops["P"], np.zeros(n), ops["A"], np.full(m, -np.finfo(np.float64).max),
                  oracle.upper_bound(ops, np.zeros(4), 0.0))
        assert _rc(gen.mimo_plant_vjp_device, g.data_ptr(), plant, X, U, y, grads, na.data_ptr(), c.stream) == ERR_ARG
    c.step()
    for k in range(9):  # a NULL plant array
        assert _rc(fn, g.data_ptr(), plant[:k] + [0] + plant[k + 1:], X, U, y, grads, na.data_ptr(), c.stream) == ERR_ARG
    assert _rc(fn, g.data_ptr(), plant, 0, U, y, grads, na.data_ptr(), c.stream) == ERR_ARG   # NULL X
    assert _rc(fn, g.data_ptr(), plant, X, 0, y, grads, na.data_ptr(), c.stream) == ERR_ARG   # NULL U_prev
    assert _rc(fn, g.data_ptr(), plant, X, U, y, [0] * 9, 0, c.stream) == ERR_ARG             # every output NULL
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):  # refused, nothing recorded
        assert _rc(fn, g.data_ptr(), plant, X, U, y, grads, na.data_ptr(), side.cuda_stream) == ERR_ARG
    torch.cuda.synchronize()
    for k in KEYS:
        assert bool(torch.isnan(outs[k]).all()), k
    assert bool((na == -7).all())
    # and the context still serves a call afterwards
    fn(g.data_ptr(), plant, X, U, y, grads, na.data_ptr(), c.stream)
    torch.cuda.synchronize()
    assert bool((na >= 0).all()) and not any(bool(torch.isnan(outs[k]).any()) for k in KEYS)


# ----------------------------------------------------------------------------- the layer
def _plant_tensors(plants, grad):
    return [_dev(plants[k]).requires_grad_(grad) for k in KEYS]


def test_layer_gradients():
    import torch

    from solvempc_amd import diff

    name = "R"
    c = _Ctx(name)  # (the direct call's context, and the dimensions)
    B, N, nx, nu, ny, n, m = c.dims
    s_rows = _inputs(name)["s_rows"]
    plants = _host_plants(c)
    w = _dev(np.random.default_rng(7).normal(size=(B, n)))
    with sm.BatchSolver(n, m, B, n_plants=B) as s:
        t = _plant_tensors(plants, True)
        X, U, yref = (v.clone().requires_grad_(True) for v in (c.X, c.U0, c.yref))
        x, status = diff.mimo_plant_solution(s, *t, X, U, yref, s_rows)
        assert bool((status == sm.SOLVED).all()) and not status.requires_grad
        assert torch.equal(U.detach(), c.U0)  # the caller's U is left alone
        grads = torch.autograd.grad((x * w).sum(), t + [X, U, yref], retain_graph=True)
        # the plant gradients are the direct call's, bit for bit
        c.step()
        assert np.array_equal(c.s.solution(), x.detach().cpu().numpy())
        direct = _call(c, w.cpu().numpy())
        for k, gk in zip(KEYS, grads[:9]):
            assert np.array_equal(gk.cpu().numpy(), direct[k]), k
        # dX, dU, dyref are mimo_solution's
        X2, U2, y2 = (v.clone().requires_grad_(True) for v in (c.X, c.U0, c.yref))
        c2 = _Ctx(name)
        x2, _ = diff.mimo_solution(c2.s, X2, U2, y2)
        want = torch.autograd.grad((x2 * w).sum(), (X2, U2, y2))
        assert torch.equal(x2, x)
        for a, b in zip(grads[9:], want):
            assert torch.equal(a, b)
        # only the gradients asked for: the plant ones alone
        only = torch.autograd.grad((x * w).sum(), t[:3], retain_graph=True)
        for a, b in zip(only, grads[:3]):
            assert torch.equal(a, b)
        # backward after another solve raises
        x3, _ = diff.mimo_plant_solution(s, *t, X, U, yref, s_rows, setup=False)
        Uc = c.U0.clone()
        s.mimo_step_device(c.X.data_ptr(), Uc.data_ptr(), c.yref.data_ptr(), c.stream)
        with pytest.raises(RuntimeError, match="solved again"):
            torch.autograd.grad((x3 * w).sum(), t)
        torch.cuda.synchronize()
    # setup=False on a solver that already holds the plants: a bit-identical x
    with sm.BatchSolver(n, m, B, n_plants=B) as s2:
        keep = [v.detach() for v in t]
        s2.mimo_setup_plants_device(nx, nu, ny, s_rows, *[v.data_ptr() for v in keep], stream=c.stream)
        x4, _ = diff.mimo_plant_solution(s2, *t, X, U, yref, s_rows, setup=False)
        assert torch.equal(x4, x)


def test_layer_end_to_end_against_device_differences():
    """Family R's first DIR_QPS plants, polished solves at eps 1e-7: the derivative of g . x along
    pref._plant_directions from one backward pass against central differences (h = pref.H) of two more polished
    device solves, on the QPs the CPU reference kept that are SOLVED and polished at all three solves.  Tolerance:
    100 x pref._plant_directional_fd("R")["err"] (2.7e-8, so 2.7e-6) relative to max(1, |derivative|): the
    reference's own error for the same quotient, nothing the device returns (tests/test_condense_vjp.py's rule).
    The direction keeps Q symmetric (pref._plant_directions): the device's setup is defined for a symmetric Q only.
    polish_refine_iter = 10: the quotient divides the solves' own error by 2h = 2e-5, and with the default delta =
    1e-6 and three refinement steps a polished point may be as far from the optimum as
    tests/test_mimo_polish_ref.py's TOL (below 1e-7), which the quotient would magnify beyond the tolerance; each
    refinement step gains a factor delta |K^-1|, so ten leave rounding error alone."""
    import torch

    from solvempc_amd import diff

    name = "R"
    d = pref._plant_directional_fd(name)
    B = pref.DIR_QPS
    plants, X, U, yref, N, s_rows = pref._family_plants(name, B)
    dv = pref._plant_directions(plants)
    nu = plants["Bd"].shape[2]
    n, m = N * nu, 2 * N * nu
    G, Xd, Ud, yd = _dev(d["g"]), _dev(X), _dev(U), _dev(yref)
    h = pref.H

    def solve(pl, grad):
        s = sm.BatchSolver(n, m, B, n_plants=B, settings=sm.default_settings(eps_abs=1e-7, eps_rel=1e-7, polish_refine_iter=10))
        t = _plant_tensors(pl, grad)
        x, status = diff.mimo_plant_solution(s, *t, Xd, Ud, yd, s_rows, polish=True)
        ok = (status.cpu().numpy() == sm.SOLVED) & (s.polish_info()[0] == 1)
        return s, t, x, ok

    s, t, x, ok = solve(plants, True)
    (x * G).sum().backward()
    got = {k: v.grad.cpu().numpy() for k, v in zip(KEYS, t)}
    s.close()
    deriv = sum((got[k] * dv[k]).reshape(B, -1).sum(axis=1) for k in KEYS)
    vals = []
    for sgn in (1.0, -1.0):
        s2, _, xm, ok2 = solve({k: plants[k] + sgn * h * dv[k] for k in KEYS}, False)
        ok &= ok2
        s2.close()
        vals.append((xm * G).sum(dim=1).cpu().numpy())
    fd = (vals[0] - vals[1]) / (2 * h)
    keep = d["keep"] & ok
    tol = 100.0 * d["err"]
    err = np.abs(deriv - fd) / np.maximum(1.0, np.abs(deriv))
    print(f"layer: directional derivative vs device differences on {int(keep.sum())} of {B} QPs: "
          f"{err[keep].max():.2e} (tolerance {tol:.1e}); per QP {np.array2string(err, precision=1)}; against the CPU "
          f"reference's derivative {np.abs(deriv - d['exact'])[keep].max():.2e}")
    assert keep.sum() >= 0.9 * d["keep"].sum()
    assert err[keep].max() <= tol

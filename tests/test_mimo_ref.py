"""MIMO steps with a per-plant output reference over the horizon on the device (mpcq_mimo_step_ref*,
mpcq_mimo_step_ref_vjp_device, mpcq_mimo_step_ref_gains*, diff.mimo_ref_solution) against the full
Fr of ``oracle.condense_mimo`` and one ``oracle.Solver`` per plant, on the families of tests/test_mimo_ref_ref.py:
(A) the random n_x 3 / n_u 2 / n_y 2 / N 8 plants with a general K0 (B 40), (B) the quad-rotor at N 30 (B 24), (C) the
SISO specialisation at N 20 (B 32) -- all three n_u and both K0 variants of the solve kernel.

Bounds: q and dref within 1e-12 of the scales stated at each test (the rounding bound of the sums is 2e-14 of them,
tests/test_mimo_ref_ref.py); the solve under tests/test_mimo.py's ``_check`` rule (copied below) with the oracle's own
decision margin; a horizon-constant reference, a padded stride and a second call bit for bit.  None of the bounds was
taken from the device's figures, which each test prints."""
import functools

import numpy as np
import pytest

import oracle
import solvempc_amd as sm

from test_mimo_ref_ref import FAM, _dims, _ops, _references, _yref
from test_mimo_sensitivity import _Ctx, _dev, _rc
from test_mimo_sensitivity_ref import _frs, _inputs
from test_sensitivity_ref import LMIN, _optimum_active

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_ORDER = sm._capi.MPCQ_ERR_ARG, sm._capi.MPCQ_ERR_ORDER
TIE_MARGIN = 1e-6  # tests/test_mimo.py's
TIE_X_REL = 5e-2
KEYS = ("x", "y", "U", "st", "it", "rho", "q")


def _check(x, st, it, U1, x_ref, st_ref, it_ref, U_ref, margin, tol=1e-7):
    """tests/test_mimo.py's rule, copied: the oracle's status on every QP; its iteration count, x and U to `tol` on
    every QP but those whose schedule decision the oracle takes within TIE_MARGIN of its threshold."""
    assert np.array_equal(st, st_ref), (st, st_ref)
    same = it == it_ref
    assert np.all(same | (margin < TIE_MARGIN)), (np.flatnonzero(~same), it[~same], it_ref[~same], margin[~same])
    if not same.all():
        print(f"{int((~same).sum())} of {len(same)} QPs took a tie's other branch (margins {margin[~same]})")
    rel = np.abs(x[same] - x_ref[same]).max(axis=1) / np.maximum(1.0, np.abs(x_ref[same]).max(axis=1))
    assert rel.max() < tol, rel.max()
    assert np.abs(U1[same] - U_ref[same]).max() < tol
    if not same.all():  # a tie stops one check earlier or later: both iterates met eps 1e-3, so they agree loosely
        rt = np.abs(x[~same] - x_ref[~same]).max(axis=1) / np.maximum(1.0, np.abs(x_ref[~same]).max(axis=1))
        assert rt.max() < TIE_X_REL, rt.max()


class _RefCtx(_Ctx):
    """tests/test_mimo_sensitivity.py's context of a family, with the reference steps; U evolves in ``self.U``."""

    def __init__(self, fam, settings=None, B=None):
        super().__init__(FAM[fam], settings, B)
        self.fam, self.U = fam, self.U0.clone()

    def results(self):
        import torch

        from solvempc_amd.diff import _DevArray

        torch.cuda.synchronize()
        B, n = self.dims[0], self.dims[5]
        r = dict(x=self.s.solution(), y=self.s.dual(), U=self.U.cpu().numpy())
        r["st"], r["it"], r["rho"] = self.s.info()
        v = self.s.device_view()
        torch.cuda.synchronize()
        r["q"] = torch.as_tensor(_DevArray(v["q"], (B, n), "<f8"), device="cuda:0").cpu().numpy().copy()
        return r

    def step_ref(self, ref, polish=False):
        """One reference step: ref (N n_y,) is shared by the batch (stride 0), ref (B, w) has stride w."""
        rd = _dev(ref)
        self.s.mimo_step_ref_device(self.X.data_ptr(), self.U.data_ptr(), rd.data_ptr(),
                                    0 if ref.ndim == 1 else ref.shape[1], polish, self.stream)
        r = self.results()
        rd.fill_(float("nan"))  # (the step has finished: nothing reads the reference any more)
        if polish:
            r["pol"] = self.s.polish_info()
        return r

    def step_plain(self, yref, polish=False):
        yd = _dev(yref)
        fn = self.s.mimo_step_polish_device if polish else self.s.mimo_step_device
        fn(self.X.data_ptr(), self.U.data_ptr(), yd.data_ptr(), self.stream)
        r = self.results()
        if polish:
            r["pol"] = self.s.polish_info()
        return r


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    if "pol" in a:
        for u, v in zip(a["pol"], b["pol"]):
            assert np.array_equal(u, v, equal_nan=True)


def _oracle_steps(fam, refs, B=None):
    """One oracle.Solver per plant, built as tests/test_mimo.py's test_second_step_is_warm_started builds it and kept
    across the steps, with the gradient formed in numpy from the full Fr: per step dict(x, st, it, margin, U)."""
    f = _inputs(FAM[fam])
    B0, N, nx, nu, ny = _dims(fam)
    B = B0 if B is None else B
    n, m = N * nu, 2 * N * nu
    out = [dict(x=np.zeros((B, n)), st=np.zeros(B, np.int32), it=np.zeros(B, np.int32), margin=np.zeros(B),
                U=np.zeros((B, nu))) for _ in refs]
    for b in range(B):
        ops = _ops(fam)[b]
        r = oracle.Solver(ops["P"], np.zeros(n), ops["A"], np.full(m, -np.finfo(float).max), ops["W0"])
        u_cur = f["U"][b].copy()
        for k, ref in enumerate(refs):
            q = ops["Fx"] @ f["X"][b] + ops["Fu"] @ u_cur + ops["Fr"] @ ref[b]
            assert r.update_gradient(q)
            assert r.update_upper_bound(oracle.mimo_upper_bound(ops, f["X"][b], u_cur))
            st = r.solve()
            if st == oracle.SOLVED:
                u_cur = u_cur + r.x()[:nu]
            info = r.info()
            o = out[k]
            o["x"][b], o["st"][b], o["it"][b], o["margin"][b], o["U"][b] = r.x(), st, info.iter, info.margin, u_cur
    return out


@functools.lru_cache(maxsize=None)
def _stepped(fam, kind):
    """One context of a family after one reference step of a kind of tests/test_mimo_ref_ref.py's references."""
    c = _RefCtx(fam)
    return c, c.step_ref(_references(fam)[kind])


# ----------------------------------------------------------------------------- 1. the device's q
@pytest.mark.parametrize("fam", sorted(FAM))
def test_q_matches_the_full_operator(fam):
    f = _inputs(FAM[fam])
    B, N, nx, nu, ny = _dims(fam)
    ref = _references(fam)["random"]
    _, r = _stepped(fam, "random")
    worst = 0.0
    for b, ops in enumerate(_ops(fam)):
        q = ops["Fx"] @ f["X"][b] + ops["Fu"] @ f["U"][b] + ops["Fr"] @ ref[b]
        scale = max(1.0, np.abs(ops["Fx"]).max() * np.abs(f["X"][b]).sum() + np.abs(ops["Fu"]).max() * np.abs(f["U"][b]).sum()
                    + np.abs(_frs(ops, ny)).max() * np.abs(ref[b]).sum())
        err = np.abs(r["q"][b] - q).max()
        worst = max(worst, err / scale)
        assert err <= 1e-12 * scale, (b, err, scale)
    print(f"family {fam}: q against Fx X + Fu U + Fr ref {worst:.1e} of the scale (bound 1e-12)")


# ----------------------------------------------------------------------------- 2. the solve against the oracle
@pytest.mark.parametrize("fam", sorted(FAM))
def test_step_references_match_oracle(fam):
    """Every plant's reference steps at a horizon index of its own, so the preview matters."""
    _, r = _stepped(fam, "step")
    o = _oracle_steps(fam, [_references(fam)["step"]])[0]
    print(f"family {fam}: statuses {sorted(set(r['st'].tolist()))}, iterations {r['it'].min()}..{r['it'].max()}")
    _check(r["x"], r["st"], r["it"], r["U"], o["x"], o["st"], o["it"], o["U"], o["margin"])


# ----------------------------------------------------------------------------- 3. a sliding window
def test_sliding_window_is_warm_started():
    """Two steps on family (B), B = 8: the second step's window is the first's shifted by one block with the last
    value held, and the step warm-starts from the first as an oracle solver that keeps its state does."""
    fam, B = "B", 8
    _, N, nx, nu, ny = _dims(fam)
    ref = _references(fam)["step"][:B]
    nxt = np.concatenate([ref[:, ny:], ref[:, -ny:]], axis=1)
    c = _RefCtx(fam, B=B)
    rs = [c.step_ref(ref.copy()), c.step_ref(nxt.copy())]
    os_ = _oracle_steps(fam, [ref, nxt], B)
    for k in range(2):  # (tests/test_mimo.py's test_second_step_is_warm_started: the applied U to 1e-7, the status)
        assert np.array_equal(rs[k]["st"], os_[k]["st"])
        np.testing.assert_allclose(rs[k]["U"], os_[k]["U"], rtol=0, atol=1e-7)
    assert not np.array_equal(rs[0]["U"], rs[1]["U"])


# ----------------------------------------------------------------------------- 4. a uniform reference
@pytest.mark.parametrize("polish", [False, True], ids=["plain", "polish"])
@pytest.mark.parametrize("fam", ["A", "B"])
def test_uniform_reference_is_the_yref_step_bit_for_bit(fam, polish):
    B, N, nx, nu, ny = _dims(fam)
    uni = _references(fam)["uniform"]
    twin = _RefCtx(fam).step_plain(_yref(fam), polish)
    assert (twin["st"] == sm.SOLVED).any()
    if polish:
        assert (twin["pol"][0] == 1).any()
    _same(_RefCtx(fam).step_ref(uni[0].copy(), polish), twin)  # ref_stride = 0
    _same(_RefCtx(fam).step_ref(uni.copy(), polish), twin)     # ref_stride = N n_y


# ----------------------------------------------------------------------------- 5. padding
def test_padded_stride_reads_no_padding():
    fam = "A"
    B, N, nx, nu, ny = _dims(fam)
    ref = _references(fam)["random"]
    padded = np.full((B, N * ny + 3), np.nan)
    padded[:, :N * ny] = ref
    _, packed = _stepped(fam, "random")
    r = _RefCtx(fam).step_ref(padded)
    assert np.isfinite(r["x"]).all()
    _same(r, packed)


# ----------------------------------------------------------------------------- 6. dref
@functools.lru_cache(maxsize=None)
def _gains(fam):
    c, _ = _stepped(fam, "random")
    import torch

    B, N, nx, nu, ny, n, m = c.dims
    new = lambda *shape: torch.full(shape, np.nan, dtype=torch.float64, device="cuda:0")
    dX, dU, dr, na = new(B, nu, nx), new(B, nu, nu), new(B, nu, N * ny), torch.full((B,), -7, dtype=torch.int32,
                                                                                    device="cuda:0")
    c.s.mimo_step_ref_gains_device(dX.data_ptr(), dU.data_ptr(), dr.data_ptr(), na.data_ptr(), c.stream)
    torch.cuda.synchronize()
    dev = tuple(t.cpu().numpy() for t in (dX, dU, dr, na))
    return dict(dev=dev, host=c.s.mimo_step_ref_gains(), plain=c.s.mimo_step_gains(), sens=c.s.mimo_sensitivity(None, nu))


@pytest.mark.parametrize("fam", ["A", "B"])
def test_dref_is_the_transposed_operator(fam):
    g = _gains(fam)
    B, N, nx, nu, ny = _dims(fam)
    dX, dU, dr, na = g["dev"]
    gq = g["sens"][0]
    pX, pU, py, pna = g["plain"]
    assert (na >= 0).all() and np.abs(gq).max() > 0
    worst = worst_s = 0.0
    for b, ops in enumerate(_ops(fam)):
        fmax = np.abs(_frs(ops, ny)).max()
        for k in range(nu):
            scale = max(1.0, fmax * np.abs(gq[b, k]).sum())
            err = np.abs(dr[b, k] - ops["Fr"].T @ gq[b, k]).max()
            err_s = np.abs(dr[b, k].reshape(N, ny).sum(axis=0) - py[b, k]).max()
            worst, worst_s = max(worst, err / scale), max(worst_s, err_s / scale)
            assert err <= 1e-12 * scale and err_s <= 1e-12 * scale, (b, k, err, err_s, scale)
    print(f"family {fam}: dref against Fr' gq {worst:.1e}, its horizon sum against dyref {worst_s:.1e} of the scale "
          f"(bound 1e-12)")
    assert np.array_equal(dX, pX) and np.array_equal(dU, pU) and np.array_equal(na, pna)
    for a, b_ in zip(g["dev"], g["host"]):  # (a second call, through the host form)
        assert np.array_equal(a, b_)


def test_dref_of_unsolved_qps_is_zero():
    fam, B = "B", 8
    c = _RefCtx(fam, settings=sm.default_settings(max_iter=15), B=B)
    r = c.step_ref(_references(fam)["random"][:B].copy())
    assert (r["st"] != sm.SOLVED).all()
    dX, dU, dr, na = c.s.mimo_step_ref_gains()
    assert (na == -1).all() and (dr == 0).all() and (dX == 0).all() and (dU == 0).all()


# ----------------------------------------------------------------------------- 7. autograd
def test_autograd_mimo_ref_solution_and_central_differences():
    """``diff.mimo_ref_solution``'s gradients are mpcq_mimo_step_ref_vjp_device's for the same cotangent, bit for bit.
    Then d(w . x*)/d ref on family (A) against central differences as tests/test_mimo_sensitivity_ref.py's
    test_chain_rule_signs_match_finite_differences takes them for yref: step h = 1e-4 in every entry of the QP's
    reference, x* = ``_optimum_active``, only QPs whose active set no perturbation moves (and whose set on the device,
    the support of gu, is the optimum's: the derivative is that of the optimum's affine piece), bound 1e-7 relative to
    max(1, |dref_b|_inf).  At most a quarter of the QPs may be left out."""
    import torch

    from solvempc_amd import diff

    fam = "A"
    f = _inputs(FAM[fam])
    B, N, nx, nu, ny = _dims(fam)
    n, m, nr = N * nu, 2 * N * nu, N * ny
    ref0 = _references(fam)["random"]
    c = _RefCtx(fam)
    X, U, ref = (t.clone().requires_grad_(True) for t in (c.X, c.U0, _dev(ref0)))
    x, status = diff.mimo_ref_solution(c.s, X, U, ref)
    assert bool((status == sm.SOLVED).all()) and not status.requires_grad
    w = np.random.default_rng(7).normal(size=(B, n))
    wd = _dev(w)
    gX, gU, gr = torch.autograd.grad((x * wd).sum(), (X, U, ref), retain_graph=True)
    new = lambda k: torch.full((B, 1, k), np.nan, dtype=torch.float64, device="cuda:0")
    dX, dU, dr = new(nx), new(nu), new(nr)
    c.s.mimo_step_ref_vjp_device(wd.data_ptr(), 1, dX.data_ptr(), dU.data_ptr(), dr.data_ptr(), 0, c.stream)
    torch.cuda.synchronize()
    assert torch.equal(gX, dX[:, 0]) and torch.equal(gU, dU[:, 0]) and torch.equal(gr, dr[:, 0])
    assert torch.equal(U.detach(), c.U0)  # the caller's U is left alone
    supp = c.s.mimo_sensitivity(w)[1][:, 0] != 0
    dref = gr.cpu().numpy()
    c.step()
    with pytest.raises(RuntimeError, match="solved again"):
        torch.autograd.grad((x * wd).sum(), (X, U, ref))

    h, l = 1e-4, np.full(m, LMIN)
    kept, worst = 0, 0.0
    for b, ops in enumerate(_ops(fam)):
        u = oracle.mimo_upper_bound(ops, f["X"][b], f["U"][b])
        q0 = ops["Fx"] @ f["X"][b] + ops["Fu"] @ f["U"][b]

        def xstar(r):
            return _optimum_active(ops["P"], ops["A"], q0 + ops["Fr"] @ r, l, u)

        _, low, upp = xstar(ref0[b])
        stable = not low.any() and np.array_equal(upp, supp[b])
        fd = np.zeros(nr)
        for j in range(nr):
            xs = []
            for sgn in (1.0, -1.0):
                xj, lo, up = xstar(ref0[b] + sgn * h * np.eye(nr)[j])
                stable = stable and np.array_equal(lo, low) and np.array_equal(up, upp)
                xs.append(xj)
            if not stable:
                break
            fd[j] = w[b] @ (xs[0] - xs[1]) / (2 * h)
        if not stable:
            continue
        kept += 1
        err = np.abs(fd - dref[b]).max() / max(1.0, np.abs(dref[b]).max())
        worst = max(worst, err)
        assert err <= 1e-7, (b, err)
    print(f"family A: {kept} of {B} QPs compared with central differences, worst {worst:.2e} (bound 1e-7)")
    assert B - kept <= B // 4, (kept, B)


# ----------------------------------------------------------------------------- 8. refusals
def test_refused_reference_steps_write_nothing():
    fam = "A"
    B, N, nx, nu, ny = _dims(fam)
    ref = _dev(_references(fam)["random"])
    yref = _yref(fam)
    res = []
    for refuse in (False, True):
        c = _RefCtx(fam)
        if refuse:
            p = lambda t: t.data_ptr()
            step = c.s.mimo_step_ref_device
            assert _rc(step, p(c.X), p(c.U), 0, N * ny, False, c.stream) == ERR_ARG          # NULL ref
            assert _rc(step, p(c.X), p(c.U), p(ref), N * ny - 1, False, c.stream) == ERR_ARG  # a stride below N n_y
            assert _rc(step, p(c.X), p(c.U), p(ref), N * ny, 2, c.stream) == ERR_ARG          # polish = 2
            assert _rc(step, 0, p(c.U), p(ref), N * ny, False, c.stream) == ERR_ARG
        res.append(c.step_plain(yref))
    _same(*res)


def test_plant_vjp_is_refused_after_a_reference_step():
    fam = "A"
    f = _inputs(FAM[fam])
    B, N, nx, nu, ny = _dims(fam)
    c = _RefCtx(fam)
    plant = dict(Ad=f["Ad"], Bd=f["Bd"])
    for k in ("Cd", "Q", "R", "RD", "K", "K0", "w0"):
        a = np.asarray(f["sh"][k], dtype=np.float64)
        plant[k] = np.broadcast_to(a, (B,) + a.shape).copy()
    c.step_ref(_references(fam)["random"].copy())
    assert _rc(c.s.mimo_plant_vjp, plant, f["X"], f["U"], _yref(fam)) == ERR_ORDER
    c.s.mimo_sensitivity(None, 1)  # (the sensitivities serve the reference step)
    c.U = c.U0.clone()
    c.step_plain(_yref(fam))
    out = c.s.mimo_plant_vjp(plant, f["X"], f["U"], _yref(fam))
    assert (out["n_active"] >= 0).all() and np.isfinite(out["Ad"]).all()

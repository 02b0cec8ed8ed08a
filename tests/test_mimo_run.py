"""Closed-loop MIMO runs on the device (mpcq_mimo_set_plant_device, mpcq_mimo_simulate_device, mpcq_mimo_run_device,
mpcq_mimo_run_ref_device, BatchSolver.mimo_rollout; solvempc_amd/csrc/mpcq_mimo_run.hip) on the families
of tests/test_mimo_ref.py: (A) random n_x 3 / n_u 2 / n_y 2 / N 8 plants with a general K0 (B 40), (B) the quad-rotor
at N 30 (the first 8 plants), (C) the SISO specialisation at N 20 (B 32).

The standard run is K = 5 steps, seed 7, noise 0.01, a schedule of L = N + 2 blocks per plant
(tests/test_mimo_run_ref.py's ``_schedule``): steps 0-2 read the schedule in place, steps 3-4 the padded tail.

* A run is the single calls bit for bit: ``mimo_step_ref_device`` on the host-built hold-last window, then
  ``mimo_simulate_device``, K times -- X, U, solution, dual, info, q, polish info and every logged row; the totals
  are the column sums of the logged rows.  The same for chunked calls, log offsets, a padded stride, a shared
  schedule, L = 1 (against ``mimo_run_device``), L = 3 < N, and a run with unsolved steps.
* The plant row against numpy within 1e-12 max(1, sum|Ad_i||x| + sum|Bd_i||u| + |w_i|) per entry: the rounding bound is
  (n_x + n_u + 2) eps = 2e-15 of that scale plus a few ulp of libm in w.
* The closed loop against one warm-started ``oracle.Solver`` per plant, teacher-forced with the device's logged
  X_{k-1}, U_{k-1}, under tests/test_mimo.py's ``_check`` rule (1e-7); the oracle's margins are asserted to lie above
  the tie threshold, so no QP is left out.
* Refusals write nothing.

None of the bounds was taken from the device's figures, which the tests print."""
import functools

import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import workload

from test_mimo_ref import TIE_MARGIN, _RefCtx, _check, _same
from test_mimo_ref_ref import FAM, _dims, _ops, _yref
from test_mimo_run_ref import _schedule, _window
from test_mimo_sensitivity import _dev, _rc
from test_mimo_sensitivity_ref import _inputs

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_ORDER = sm._capi.MPCQ_ERR_ARG, sm._capi.MPCQ_ERR_ORDER
K, SEED, STD = 5, 7, 0.01
BATCH = {"A": None, "B": 8, "C": None}  # (None: the family's own)
ROWS = ("U", "X", "status", "iter")
STATE = ("x", "y", "U", "st", "it", "rho", "q", "X")


def _sched(fam, L=None):
    B, N, nx, nu, ny = _dims(fam)
    return _schedule(fam, N + 2 if L is None else L)[:BATCH[fam] or B]


class _RunCtx(_RefCtx):
    """tests/test_mimo_ref.py's context with a simulated plant (``scale`` Ad: a plant that is not the model); X and U
    evolve in ``self.X``, ``self.U``."""

    def __init__(self, fam, settings=None, scale=1.0, plant=True):
        super().__init__(fam, settings, BATCH[fam])
        B = self.dims[0]
        f = _inputs(FAM[fam])
        self.Ad, self.Bd = scale * f["Ad"][:B], f["Bd"][:B].copy()
        self.X0, self.U0h = f["X"][:B].copy(), f["U"][:B].copy()
        self.plant = [_dev(self.Ad), _dev(self.Bd)]
        if plant:
            self.s.mimo_set_plant_device(self.plant[0].data_ptr(), self.plant[1].data_ptr(), self.stream)

    def log(self, rows=K, step0=0):
        """A record of `rows` rows filled with sentinels: (the device tensors, the mpcq_mimo_log argument)."""
        import torch

        B, N, nx, nu, ny, n, m = self.dims
        f64 = lambda *s: torch.full(s, np.nan, dtype=torch.float64, device="cuda:0")
        i32 = lambda *s: torch.full(s, -99, dtype=torch.int32, device="cuda:0")
        t = dict(U=f64(rows, B, nu), X=f64(rows, B, nx), status=i32(rows, B), iter=i32(rows, B), iters_total=i32(B),
                 unsolved_total=i32(B))
        return t, self.s.mimo_log(*[t[k].data_ptr() for k in ROWS + ("iters_total", "unsolved_total")], rows, step0)

    def run_ref(self, sched, steps=K, first_step=0, polish=False, log=None, first_qp=0, std=STD):
        """mimo_run_ref_device on a host schedule (L, n_y) (shared, stride 0) or (B, L, n_y) (stride L n_y)."""
        import torch

        ny = self.dims[4]
        sd = _dev(sched)
        L, stride = sched.shape[-2], 0 if sched.ndim == 2 else sched.shape[-2] * ny
        self.s.mimo_run_ref_device(self.X.data_ptr(), self.U.data_ptr(), sd.data_ptr(), L, stride, steps, SEED, first_qp,
                                   first_step, std, polish, log, self.stream)
        torch.cuda.synchronize()
        sd.fill_(float("nan"))  # (the run has finished: nothing reads the schedule any more)

    def singles(self, sched, steps=K, first_step=0, polish=False, first_qp=0, std=STD):
        """The sequence a run stands for: per step the hold-last window built here, mimo_step_ref_device, then
        mimo_simulate_device; the rows a log would hold."""
        import torch

        N = self.dims[1]
        rows = {k: [] for k in ROWS}
        for s in range(first_step, first_step + steps):
            r = self.step_ref(_window(sched, s, N), polish)
            self.s.mimo_simulate_device(self.X.data_ptr(), self.U.data_ptr(), SEED, first_qp, s, std, self.stream)
            torch.cuda.synchronize()
            for k, v in zip(ROWS, (r["U"], self.X.cpu().numpy(), r["st"], r["it"])):
                rows[k].append(v)
        return {k: np.stack(v) for k, v in rows.items()}

    def state(self, polish=False):
        r = self.results()
        r["X"] = self.X.cpu().numpy()
        if polish:
            r["pol"] = self.s.polish_info()
        return r


def _host(t):
    import torch

    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in t.items()}


def _same_rows(a, b, rows=slice(None)):
    for k in ROWS:
        assert np.array_equal(a[k][rows], b[k], equal_nan=True), k


def _totals_match(lg, rows=slice(None)):
    assert np.array_equal(lg["iters_total"], lg["iter"][rows].sum(axis=0))
    assert np.array_equal(lg["unsolved_total"], (lg["status"][rows] != sm.SOLVED).sum(axis=0))


def _standard(fam, polish=False, max_iter=None):
    """The standard run of a family and the single calls it stands for, once per session: the run's log and final
    state, the single calls' rows and final state."""
    return _standard_once(fam, polish, max_iter)


@functools.lru_cache(maxsize=None)
def _standard_once(fam, polish, max_iter):
    st =sm.default_settings(max_iter=max_iter) if max_iter else None
    sched = _sched(fam)
    run = _RunCtx(fam, st)
    t, log = run.log()
    run.run_ref(sched, polish=polish, log=log)
    one = _RunCtx(fam, st)
    rows = one.singles(sched, polish=polish)
    return dict(log=_host(t), state=run.state(polish), rows=rows, one_state=one.state(polish), ctx=run, sched=sched)


# ----------------------------------------------------------------------------- 1. a run is the single calls
@pytest.mark.parametrize("fam,polish", [("A", False), ("A", True), ("B", False), ("C", False)],
                         ids=["A", "A-polish", "B", "C"])
def test_run_is_the_single_calls_bit_for_bit(fam, polish):
    d = _standard(fam, polish)
    lg = d["log"]
    print(f"family {fam}: statuses {sorted(set(lg['status'].ravel().tolist()))}, iterations {lg['iter'].min()}.."
          f"{lg['iter'].max()}, |X| up to {np.abs(lg['X']).max():.3g}")
    assert np.isfinite(lg["X"]).all() and np.isfinite(lg["U"]).all() and (lg["status"] == sm.SOLVED).any()
    if polish:
        assert (d["state"]["pol"][0] == 1).any()
    _same(d["state"], d["one_state"], STATE)
    _same_rows(lg, d["rows"])
    assert np.array_equal(lg["X"][-1], d["state"]["X"]) and np.array_equal(lg["U"][-1], d["state"]["U"])
    assert not np.array_equal(lg["U"][0], lg["U"][-1])
    _totals_match(lg)


# ----------------------------------------------------------------------------- 2. chunks and offsets
def test_two_chunks_fill_one_log():
    d = _standard("A")
    c = _RunCtx("A")
    t, log = c.log()
    c.run_ref(d["sched"], steps=3, first_step=0, log=log)
    c.run_ref(d["sched"], steps=2, first_step=3, log=log)
    lg = _host(t)
    _same_rows(lg, d["log"])
    _same(c.state(), d["state"], STATE)
    _totals_match(lg, slice(3, 5))  # (the totals are the second call's)


def test_log_offset_is_checked_and_used():
    d = _standard("A")
    c = _RunCtx("A")
    t, log = c.log(rows=3, step0=2)
    X0, U0 = c.X.cpu().numpy(), c.U.cpu().numpy()
    sd = _dev(d["sched"])
    B, N, nx, nu, ny, n, m = c.dims
    args = lambda first, steps: (c.X.data_ptr(), c.U.data_ptr(), sd.data_ptr(), N + 2, (N + 2) * ny, steps, SEED, 0,
                                 first, STD, False, log, c.stream)
    assert _rc(c.s.mimo_run_ref_device, *args(0, K)) == ERR_ARG   # rows -2 .. 2
    assert _rc(c.s.mimo_run_ref_device, *args(2, 4)) == ERR_ARG   # rows 0 .. 3
    lg = _host(t)
    assert np.isnan(lg["U"]).all() and np.isnan(lg["X"]).all() and (lg["status"] == -99).all()
    assert (lg["iters_total"] == -99).all() and (lg["unsolved_total"] == -99).all()
    assert np.array_equal(c.X.cpu().numpy(), X0) and np.array_equal(c.U.cpu().numpy(), U0)
    c.run_ref(d["sched"], steps=2, first_step=0)          # no record
    c.run_ref(d["sched"], steps=3, first_step=2, log=log)  # rows 0 .. 2
    lg = _host(t)
    _same_rows(d["log"], lg, slice(2, 5))
    _same(c.state(), d["state"], STATE)
    _totals_match(lg)


def test_padded_stride_reads_no_padding():
    d = _standard("A")
    c = _RunCtx("A")
    B, N, nx, nu, ny, n, m = c.dims
    L = N + 2
    padded = np.full((B, L * ny + 3), np.nan)
    padded[:, :L * ny] = d["sched"].reshape(B, -1)
    t, log = c.log()
    import torch

    sd = _dev(padded)
    c.s.mimo_run_ref_device(c.X.data_ptr(), c.U.data_ptr(), sd.data_ptr(), L, L * ny + 3, K, SEED, 0, 0, STD, False, log,
                            c.stream)
    torch.cuda.synchronize()
    lg = _host(t)
    assert np.isfinite(lg["X"]).all()
    _same_rows(lg, d["log"])
    _same(c.state(), d["state"], STATE)


def test_shared_schedule_is_the_schedule_repeated():
    fam = "A"
    B, N, nx, nu, ny = _dims(fam)
    one = _sched(fam)[0]  # (L, n_y)
    res = []
    for sched in (one, np.broadcast_to(one, (B,) + one.shape).copy()):
        c = _RunCtx(fam)
        t, log = c.log()
        c.run_ref(sched, log=log)
        res.append((_host(t), c.state()))
    _same_rows(res[0][0], res[1][0])
    _same(res[0][1], res[1][1], STATE)
    rows = _RunCtx(fam).singles(one)
    _same_rows(res[0][0], rows)


# ----------------------------------------------------------------------------- 3. degenerate schedules
@pytest.mark.parametrize("polish", [False, True], ids=["plain", "polish"])
def test_one_block_schedule_is_the_yref_run(polish):
    import torch

    fam = "A"
    y = _yref(fam)
    a = _RunCtx(fam)
    ta, la = a.log()
    a.run_ref(y[None, :].copy(), polish=polish, log=la)
    b = _RunCtx(fam)
    tb, lb = b.log()
    yd = _dev(y)
    b.s.mimo_run_device(b.X.data_ptr(), b.U.data_ptr(), yd.data_ptr(), K, SEED, 0, 0, STD, polish, lb, b.stream)
    torch.cuda.synchronize()
    ha, hb = _host(ta), _host(tb)
    assert (hb["status"] == sm.SOLVED).any()
    _same_rows(ha, hb)
    _same(a.state(polish), b.state(polish), STATE)
    _totals_match(hb)
    # and the yref run is its own single calls
    c = _RunCtx(fam)
    rows = {k: [] for k in ROWS}
    for s in range(K):
        r = c.step_plain(y, polish)
        c.s.mimo_simulate_device(c.X.data_ptr(), c.U.data_ptr(), SEED, 0, s, STD, c.stream)
        torch.cuda.synchronize()
        for k, v in zip(ROWS, (r["U"], c.X.cpu().numpy(), r["st"], r["it"])):
            rows[k].append(v)
    _same_rows(hb, {k: np.stack(v) for k, v in rows.items()})
    _same(b.state(polish), c.state(polish), STATE)


def test_schedule_shorter_than_the_horizon():
    fam = "A"
    sched = _sched(fam, 3)
    assert sched.shape[1] == 3 < _dims(fam)[1]
    c = _RunCtx(fam)
    t, log = c.log()
    c.run_ref(sched, log=log)
    one = _RunCtx(fam)
    rows = one.singles(sched)
    _same_rows(_host(t), rows)
    _same(c.state(), one.state(), STATE)


# ----------------------------------------------------------------------------- 4. the plant row
def _row_check(c, lg, Ad, first_qp, std, what):
    B, N, nx, nu, ny, n, m = c.dims
    worst = 0.0
    for k in range(K):
        Xp = c.X0 if k == 0 else lg["X"][k - 1]
        w = workload.plant_noise(SEED, first_qp, B, k, nx, std) if std else np.zeros((B, nx))
        want = workload.simulate_mimo(Ad, c.Bd, Xp, lg["U"][k], w)
        scale = np.maximum(1.0, np.einsum("bit,bt->bi", np.abs(Ad), np.abs(Xp)) +
                           np.einsum("bij,bj->bi", np.abs(c.Bd), np.abs(lg["U"][k])) + np.abs(w))
        ratio = np.abs(lg["X"][k] - want) / scale
        worst = max(worst, ratio.max())
        assert np.all(ratio <= 1e-12), (what, k, ratio.max())
    print(f"{what}: worst |X - (Ad X + Bd U + w)| = {worst:.2e} of the scale (bound 1e-12)")
    return worst


@pytest.mark.parametrize("fam", sorted(FAM))
def test_plant_row_matches_numpy(fam):
    c = _RunCtx(fam)
    t, log = c.log()
    c.run_ref(_sched(fam), log=log, first_qp=1000)
    lg = _host(t)
    _row_check(c, lg, c.Ad, 1000, STD, f"family {fam}, first_qp 1000")
    assert not np.array_equal(lg["X"], _standard(fam)["log"]["X"])  # (first_qp keys the noise)


def test_plant_row_without_noise_and_with_another_plant():
    fam = "A"
    c = _RunCtx(fam)
    t, log = c.log()
    c.run_ref(_sched(fam), log=log, std=0.0)
    _row_check(c, _host(t), c.Ad, 0, 0.0, "family A, noise_std 0")
    c = _RunCtx(fam, scale=1.01)
    model = _inputs(FAM[fam])["Ad"][:c.dims[0]]
    assert np.array_equal(c.Ad, 1.01 * model)
    t, log = c.log()
    c.run_ref(_sched(fam), log=log)
    lg = _host(t)
    _row_check(c, lg, c.Ad, 0, STD, "family A, simulated plant 1.01 Ad")
    with pytest.raises(AssertionError):  # (the controller's model is not the plant that ran)
        _row_check(c, lg, model, 0, STD, "family A, the model in the plant's place")


# ----------------------------------------------------------------------------- 5. the oracle, teacher-forced
@pytest.mark.parametrize("fam", sorted(FAM))
def test_closed_loop_matches_oracle_teacher_forced(fam):
    d = _standard(fam)
    lg, c, sched = d["log"], d["ctx"], d["sched"]
    B, N, nx, nu, ny, n, m = c.dims
    o = [dict(x=np.zeros((B, n)), st=np.zeros(B, np.int32), it=np.zeros(B, np.int32), margin=np.zeros(B),
              U=np.zeros((B, nu))) for _ in range(K)]
    for b in range(B):
        ops = _ops(fam)[b]
        r = oracle.Solver(ops["P"], np.zeros(n), ops["A"], np.full(m, -np.finfo(float).max), ops["W0"])
        for k in range(K):
            Xin = c.X0[b] if k == 0 else lg["X"][k - 1][b]
            Uin = c.U0h[b] if k == 0 else lg["U"][k - 1][b]
            q = ops["Fx"] @ Xin + ops["Fu"] @ Uin + ops["Fr"] @ _window(sched[b], k, N)
            assert r.update_gradient(q)
            assert r.update_upper_bound(oracle.mimo_upper_bound(ops, Xin, Uin))
            st = r.solve()
            info = r.info()
            u_new = Uin + r.x()[:nu] if st == oracle.SOLVED else Uin
            o[k]["x"][b], o[k]["st"][b], o[k]["it"][b], o[k]["margin"][b], o[k]["U"][b] = r.x(), st, info.iter, info.margin, u_new
    margin = np.stack([s["margin"] for s in o])
    print(f"family {fam}: oracle statuses {sorted(set(np.stack([s['st'] for s in o]).ravel().tolist()))}, smallest "
          f"margin {margin.min():.2e} (tie threshold {TIE_MARGIN:.0e})")
    for k in range(K):
        assert np.all(o[k]["st"] == oracle.SOLVED), k
        assert margin[k].min() >= TIE_MARGIN, (k, margin[k].min())  # (no QP is left out)
        assert np.array_equal(lg["status"][k], o[k]["st"]), k
        assert np.array_equal(lg["iter"][k], o[k]["it"]), (k, np.flatnonzero(lg["iter"][k] != o[k]["it"]))
        errU = np.abs(lg["U"][k] - o[k]["U"]).max()
        print(f"  step {k}: max|U - U_oracle| = {errU:.2e} (bound 1e-7)")
        assert errU < 1e-7, (k, errU)
    last = o[-1]
    _check(d["state"]["x"], lg["status"][-1], lg["iter"][-1], lg["U"][-1], last["x"], last["st"], last["it"], last["U"],
           last["margin"])


# ----------------------------------------------------------------------------- 6. unsolved steps
def test_unsolved_steps_hold_u_and_are_counted():
    d = _standard("A", False, 50)
    lg = d["log"]
    bad = lg["status"] != sm.SOLVED
    print(f"family A, max_iter 50: {bad.sum(axis=1).tolist()} of {bad.shape[1]} QPs not SOLVED per step, statuses "
          f"{sorted(set(lg['status'].ravel().tolist()))}")
    assert bad.any() and (~bad).any()
    before = np.concatenate([d["ctx"].U0h[None], lg["U"][:-1]])
    assert np.array_equal(lg["U"][bad], before[bad])
    assert not np.array_equal(lg["U"][~bad], before[~bad])
    _totals_match(lg)
    assert lg["unsolved_total"].sum() == bad.sum()
    _same_rows(lg, d["rows"])
    _same(d["state"], d["one_state"], STATE)


# ----------------------------------------------------------------------------- 7. refusals
def test_refusals_write_nothing_and_runs_repeat():
    import torch

    fam = "A"
    d = _standard(fam)
    c = _RunCtx(fam)
    B, N, nx, nu, ny, n, m = c.dims
    L = N + 2
    sd, yd = _dev(d["sched"]), _dev(_yref(fam))
    t, log = c.log()
    X, U, S = c.X.data_ptr(), c.U.data_ptr(), sd.data_ptr()
    X0, U0 = c.X.cpu().numpy(), c.U.cpu().numpy()
    ref = lambda **o: c.s.mimo_run_ref_device(*[{**dict(X=X, U=U, S=S, L=L, stride=L * ny, steps=K, seed=SEED, fq=0, fs=0,
                                                       std=STD, polish=False, log=log, stream=c.stream), **o}[k]
                                                for k in ("X", "U", "S", "L", "stride", "steps", "seed", "fq", "fs", "std",
                                                          "polish", "log", "stream")])
    run = lambda **o: c.s.mimo_run_device(*[{**dict(X=X, U=U, y=yd.data_ptr(), steps=K, seed=SEED, fq=0, fs=0, std=STD,
                                                   polish=False, log=log, stream=c.stream), **o}[k]
                                            for k in ("X", "U", "y", "steps", "seed", "fq", "fs", "std", "polish", "log",
                                                      "stream")])
    mk = lambda rows, step0: c.s.mimo_log(*[t[k].data_ptr() for k in ROWS + ("iters_total", "unsolved_total")], rows, step0)
    for fn in (ref, run):
        assert _rc(lambda: fn(X=0)) == ERR_ARG
        assert _rc(lambda: fn(U=0)) == ERR_ARG
        assert _rc(lambda: fn(steps=-1)) == ERR_ARG
        assert _rc(lambda: fn(fs=-1)) == ERR_ARG
        assert _rc(lambda: fn(polish=2)) == ERR_ARG
        assert _rc(lambda: fn(log=mk(0, 0))) == ERR_ARG        # rows < 1
        assert _rc(lambda: fn(log=mk(K, -1))) == ERR_ARG       # step0 < 0
        assert _rc(lambda: fn(log=mk(K - 1, 0))) == ERR_ARG    # the last row outside
        assert _rc(lambda: fn(log=mk(K, 1))) == ERR_ARG        # the first row outside
    assert _rc(lambda: ref(S=0)) == ERR_ARG
    assert _rc(lambda: ref(L=0)) == ERR_ARG
    assert _rc(lambda: ref(stride=L * ny - 1)) == ERR_ARG
    assert _rc(c.s.mimo_set_plant_device, 0, c.plant[1].data_ptr(), c.stream) == ERR_ARG
    assert _rc(c.s.mimo_set_plant_device, c.plant[0].data_ptr(), 0, c.stream) == ERR_ARG
    assert _rc(c.s.mimo_simulate_device, 0, U, SEED, 0, 0, STD, c.stream) == ERR_ARG
    assert _rc(c.s.mimo_simulate_device, X, 0, SEED, 0, 0, STD, c.stream) == ERR_ARG
    assert _rc(c.s.mimo_simulate_device, X, U, SEED, 0, -1, STD, c.stream) == ERR_ARG
    # no MIMO setup; a MIMO setup without a plant; settings.polish
    with sm.BatchSolver(n, m, B, n_plants=B) as fresh:
        assert _rc(fresh.mimo_set_plant_device, c.plant[0].data_ptr(), c.plant[1].data_ptr(), c.stream) == ERR_ORDER
        assert _rc(fresh.mimo_simulate_device, X, U, SEED, 0, 0, STD, c.stream) == ERR_ORDER
        assert _rc(fresh.mimo_run_device, X, U, yd.data_ptr(), K, SEED, 0, 0, STD, False, log, c.stream) == ERR_ORDER
        assert _rc(fresh.mimo_run_ref_device, X, U, S, L, L * ny, K, SEED, 0, 0, STD, False, log, c.stream) == ERR_ORDER
    bare = _RunCtx(fam, plant=False)
    assert _rc(bare.s.mimo_simulate_device, X, U, SEED, 0, 0, STD, c.stream) == ERR_ORDER
    assert _rc(bare.s.mimo_run_device, X, U, yd.data_ptr(), K, SEED, 0, 0, STD, False, log, c.stream) == ERR_ORDER
    assert _rc(bare.s.mimo_run_ref_device, X, U, S, L, L * ny, K, SEED, 0, 0, STD, False, log, c.stream) == ERR_ORDER
    with sm.BatchSolver(16, 32, B, n_plants=B, settings=sm.default_settings(polish=1)) as on:
        assert _rc(on.mimo_run_device, X, U, yd.data_ptr(), K, SEED, 0, 0, STD, False, log, c.stream) == ERR_ARG
        assert _rc(on.mimo_run_ref_device, X, U, S, L, L * ny, K, SEED, 0, 0, STD, False, log, c.stream) == ERR_ARG
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):  # refused, nothing recorded
        assert _rc(lambda: ref(stream=side.cuda_stream)) == ERR_ARG
        assert _rc(lambda: run(stream=side.cuda_stream)) == ERR_ARG
        assert _rc(c.s.mimo_set_plant_device, c.plant[0].data_ptr(), c.plant[1].data_ptr(), side.cuda_stream) == ERR_ARG
    torch.cuda.synchronize()
    lg = _host(t)
    assert np.isnan(lg["U"]).all() and np.isnan(lg["X"]).all() and (lg["status"] == -99).all() and (lg["iter"] == -99).all()
    assert (lg["iters_total"] == -99).all() and (lg["unsolved_total"] == -99).all()
    assert np.array_equal(c.X.cpu().numpy(), X0) and np.array_equal(c.U.cpu().numpy(), U0)
    ref(steps=0)  # a no-op
    lg = _host(t)
    assert np.isnan(lg["U"]).all() and (lg["iters_total"] == -99).all()
    assert np.array_equal(c.X.cpu().numpy(), X0) and np.array_equal(c.U.cpu().numpy(), U0)
    # the run after the refused calls is the run without them, and a run from equal state repeats its bits
    ref()
    torch.cuda.synchronize()
    lg = _host(t)
    _same_rows(lg, d["log"])
    _same(c.state(), d["state"], STATE)
    assert np.array_equal(lg["iters_total"], d["log"]["iters_total"])
    assert np.array_equal(lg["unsolved_total"], d["log"]["unsolved_total"])


# ----------------------------------------------------------------------------- 8. the host form
def test_mimo_rollout_returns_the_run():
    fam = "A"
    d = _standard(fam)
    c = _RunCtx(fam, plant=False)
    out = c.s.mimo_rollout(c.X0, c.U0h, K, SEED, STD, sched=d["sched"], Ad=c.Ad, Bd=c.Bd)
    for k in ROWS + ("iters_total", "unsolved_total"):
        assert np.array_equal(out[k], d["log"][k]), k
    assert out["U"].shape == (K,) + c.U0h.shape and out["X"].shape == (K,) + c.X0.shape
    assert np.array_equal(out["X_final"], d["state"]["X"]) and np.array_equal(out["U_final"], d["state"]["U"])
    dX, dU, dref, na = c.s.mimo_step_ref_gains()  # (the sensitivities serve the run's last control step)
    assert (na >= 0).all() and np.isfinite(dref).all() and np.abs(dref).max() > 0
    ref = _standard(fam)["ctx"].s.mimo_step_ref_gains()
    for a, b in zip((dX, dU, dref, na), ref):
        assert np.array_equal(a, b)
    shared = c.s.mimo_rollout(c.X0, c.U0h, 2, SEED, STD, sched=d["sched"][0])
    assert shared["U"].shape == (2,) + c.U0h.shape and np.isfinite(shared["X"]).all()
    with pytest.raises(ValueError):
        c.s.mimo_rollout(c.X0, c.U0h, 2, SEED, STD, sched=d["sched"][:, :, :1])

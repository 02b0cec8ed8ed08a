"""The per-step record of a receding-horizon stream (mpcq_mpc_set_stream_log, BatchSolver.mpc_rollout).

A logged run of K control steps must leave, in row r of the caller's buffers, exactly what K unlogged calls of
one step each show after their r-th call: U_dev, X_dev and mpcq_get_info's status and iter, bit for bit, on
the tile stream, the one-QP-per-wave stream and the per-step graph, and must perturb nothing else.

Unless a test says otherwise: N = 20 (the tile kernel's remainder rows 16-19 are live), B = 50 (three full
16-column groups and a ragged one), 9 steps, noise 1e-2, ``workload.stream_states``, seed 9, xref 0.3 (a
non-zero set-point, so that the one-entry schedule a logged scalar run hands the kernels carries a value).
Every record buffer has two sentinel rows before and after the rows handed to the library; they are checked
after every run.  The helpers are this file's own.
"""
import contextlib
import ctypes as C
import os
import re
from pathlib import Path

import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import _capi, workload

ROOT = Path(__file__).resolve().parents[1]
LMIN = -np.finfo(np.float64).max
N0, B0, K0, NOISE, SEED, XREF = 20, 50, 9, 1e-2, 9, 0.3
PAD = 2
SENT_F, SENT_I = -1234.5, -77
PATHS = {"tile": {}, "wave": {"MPCQ_STREAM": "wave"}, "graph": {"MPCQ_STREAM": "graph"}}
NAMES = ("U", "X", "status", "iter")


# ---- CPU: the surface exists (fails on the parent) -------------------------------------------------
def test_symbol_exported_and_struct_layout():
    hdr = (ROOT / "include" / "mpcq.h").read_text()
    body = re.search(r"typedef struct mpcq_stream_log \{(.*?)\} mpcq_stream_log;", hdr, flags=re.S)
    assert body, "mpcq_stream_log not declared"
    fields = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    assert re.sub(r"\s+", " ", fields).strip() == "double *U, *X; int *status, *iter; long long rows; long long step0;"
    assert "mpcq_mpc_set_stream_log" in _capi.EXPORTS
    f = sm.lib().mpcq_mpc_set_stream_log  # AttributeError where the library does not export it
    assert f.restype is C.c_int and len(f.argtypes) == 2
    # 4 pointers + 2 long long
    assert C.sizeof(_capi.StreamLog) == 4 * C.sizeof(C.c_void_p) + 2 * C.sizeof(C.c_longlong) == 48
    assert [n for n, _ in _capi.StreamLog._fields_] == ["U", "X", "status", "iter", "rows", "step0"]
    assert callable(sm.BatchSolver.mpc_set_stream_log) and callable(sm.BatchSolver.mpc_rollout)


# ---- helpers ---------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(**kv):
    hooks = ("MPCQ_STREAM", "MPCQ_KERNEL", "MPCQ_STREAM_CPW")
    old = {k: os.environ.get(k) for k in hooks}
    for k in hooks:
        os.environ.pop(k, None)
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


_CACHE = {}


def _ops(plant, N):
    if ("ops", N) not in _CACHE:
        _CACHE["ops", N] = oracle.condense(plant, N)
    return _CACHE["ops", N]


def _ctx(plant, N, B, dtype="f64"):
    ops = _ops(plant, N)
    s = sm.BatchSolver(N, 2 * N, B, dtype=dtype)
    s.setup(ops["P"], np.zeros(N), ops["A"], np.full(2 * N, LMIN), oracle.upper_bound(ops, np.zeros(4), 0.0))
    s.mpc_set_operators(ops["Fx"], ops["Fu"], ops["Fr"], ops["Sbar"], ops["Ku"], ops["W0"])
    s.mpc_set_plant(plant["Ad"], plant["Bd"])
    return s


def _plants_ctx(plant, N, B):
    """A per-plant context (n_plants == batch) of B perturbed plants, condensed on the host."""
    Ad, Bd = workload.randomized_plants(plant, 2, 100, B)
    o = [oracle.condense(dict(plant, Ad=Ad[b], Bd=Bd[b]), N) for b in range(B)]
    st = lambda k: np.stack([p[k] for p in o])  # noqa: E731
    s = sm.BatchSolver(N, 2 * N, B, n_plants=B)
    u0 = np.stack([oracle.upper_bound(p, np.zeros(4), 0.0) for p in o])
    s.setup(st("P"), np.zeros((B, N)), st("A"), np.full((B, 2 * N), LMIN), u0)
    s.mpc_set_operators(st("Fx"), st("Fu"), st("Fr"), st("Sbar"), st("Ku"), st("W0"))
    s.mpc_set_plant(Ad, Bd)
    return s


class _Log:
    """Device buffers of a record of `rows` control steps, with PAD sentinel rows on either side."""

    def __init__(self, rows, B, nx=4, which=NAMES):
        import torch
        self.rows, self.B, self.nx, self.which = rows, B, nx, which
        shape = {"U": (B,), "X": (B, nx), "status": (B,), "iter": (B,)}
        self.t = {}
        for k in NAMES:
            f = k in ("U", "X")
            self.t[k] = torch.full((rows + 2 * PAD, *shape[k]), SENT_F if f else SENT_I,
                                   dtype=torch.float64 if f else torch.int32, device="cuda")

    def ptr(self, k):
        t = self.t[k]
        return t.data_ptr() + PAD * t[0].numel() * t.element_size() if k in self.which else 0

    def attach(self, s, step0=0):
        s.mpc_set_stream_log(self.ptr("U"), self.ptr("X"), self.ptr("status"), self.ptr("iter"), self.rows, step0)

    def read(self):
        """The record's rows (numpy), after checking that nothing else was written."""
        out = {}
        for k in NAMES:
            a = self.t[k].cpu().numpy()
            sent = SENT_F if k in ("U", "X") else SENT_I
            assert np.all(a[:PAD] == sent) and np.all(a[-PAD:] == sent), f"{k}: a sentinel row was written"
            if k not in self.which:
                assert np.all(a == sent), f"{k}: written though not attached"
            out[k] = a[PAD:-PAD].copy()
        return out

    def untouched(self):
        return all(np.all(v == (SENT_F if k in ("U", "X") else SENT_I)) for k, v in self.read().items())


def _call(s, Xd, Ud, st, first, steps, xref=XREF, sched=None, first_qp=0):
    """One mpc_run_device / mpc_run_ref_device call (sched: a device tensor, (L,) shared or (B, L) per QP)."""
    if sched is None:
        s.mpc_run_device(Xd.data_ptr(), Ud.data_ptr(), xref, steps, SEED, first_qp, first, NOISE, st.cuda_stream)
    else:
        stride = 0 if sched.dim() == 1 else sched.shape[1]
        s.mpc_run_ref_device(Xd.data_ptr(), Ud.data_ptr(), sched.data_ptr(), sched.shape[-1], stride, steps, SEED,
                             first_qp, first, NOISE, st.cuda_stream)
    st.synchronize()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _trace(s, X, U, steps, path, sched=None, first=0):
    """`steps` unlogged calls of one control step: what X_dev, U_dev and info() show after each."""
    import torch
    Xd, Ud, st = _dev(X.copy()), _dev(U.copy()), torch.cuda.Stream()
    sd = None if sched is None else _dev(sched)
    out = {k: [] for k in NAMES}
    for k in range(steps):
        _call(s, Xd, Ud, st, first + k, 1, sched=sd)
        assert s.stream_path() == path
        stat, it, _ = s.info()
        for name, v in zip(NAMES, (Ud.cpu().numpy(), Xd.cpu().numpy(), stat, it)):
            out[name].append(v.copy())
    return {k: np.stack(v) for k, v in out.items()}


def _logged(s, X, U, steps, path, sched=None, first=0, which=NAMES):
    """One logged call of `steps` control steps; the record, the final X and U, and the log object."""
    import torch
    Xd, Ud, st = _dev(X.copy()), _dev(U.copy()), torch.cuda.Stream()
    sd = None if sched is None else _dev(sched)
    log = _Log(steps, X.shape[0], X.shape[1], which)
    log.attach(s, first)
    _call(s, Xd, Ud, st, first, steps, sched=sd)
    assert s.stream_path() == path
    return log.read(), Xd.cpu().numpy(), Ud.cpu().numpy(), log


def _same(rec, trace, what=""):
    for k in NAMES:
        assert rec[k].shape == trace[k].shape, (what, k, rec[k].shape, trace[k].shape)
        assert np.array_equal(rec[k], trace[k]), (what, k, np.argwhere(rec[k] != trace[k])[:4])


def _schedules(B, L, seed=11):
    """Per-QP schedules of L values: a set-point step of a per-QP size at a per-QP step."""
    rng = np.random.default_rng(seed)
    lvl = rng.uniform(-5, 5, (B, 1))
    return lvl * (np.arange(L) >= rng.integers(0, L, (B, 1)))


def _record(plant, path, dtype):
    """Test 1's logged run (cached: the oracle and rollout tests compare against the same record)."""
    key = ("rec", path, dtype)
    if key not in _CACHE:
        X, U = workload.stream_states(4, 0, B0)
        with _env(**PATHS[path]):
            s = _ctx(plant, N0, B0, dtype)
            rec, Xf, Uf, _ = _logged(s, X, U, K0, path)
            extra = (Xf, Uf, *s.stream_counters(), s.solution(), s.dual())
            s.close()
        _CACHE[key] = (X, U, rec, extra)
    return _CACHE[key]


# ---- 1. the record is the per-step trace, bit for bit; logging perturbs nothing --------------------
@pytest.mark.gpu
@pytest.mark.parametrize("path,dtype", [("tile", "f64"), ("wave", "f64"), ("graph", "f64"), ("tile", "f32"),
                                        ("tile", "mixed")])
def test_record_is_the_per_step_trace(plant, path, dtype):
    import torch
    X, U, rec, extra = _record(plant, path, dtype)
    with _env(**PATHS[path]):
        s = _ctx(plant, N0, B0, dtype)
        trace = _trace(s, X, U, K0, path)
        s.close()
        _same(rec, trace, f"{path} {dtype}")
        # an unlogged call of all nine steps ends where the logged one did
        s = _ctx(plant, N0, B0, dtype)
        Xd, Ud, st = _dev(X.copy()), _dev(U.copy()), torch.cuda.Stream()
        _call(s, Xd, Ud, st, 0, K0)
        assert s.stream_path() == path
        plain = (Xd.cpu().numpy(), Ud.cpu().numpy(), *s.stream_counters(), s.solution(), s.dual())
        s.close()
    for name, a, b in zip(("X", "U", "iterations", "unsolved", "x", "y"), extra, plain):
        assert np.array_equal(a, b, equal_nan=True), (path, dtype, name)
    # the record agrees with the end point and the counters it details
    assert np.array_equal(rec["X"][-1], extra[0]) and np.array_equal(rec["U"][-1], extra[1])
    assert np.array_equal(rec["iter"].sum(axis=0), extra[2])
    assert np.array_equal((rec["status"] != sm.SOLVED).sum(axis=0), extra[3])


# ---- 2. against the oracle --------------------------------------------------------------------------
@pytest.mark.gpu
def test_record_matches_the_oracle_loop(plant):
    """The host loop of tests/test_gpu.py test_receding_horizon_stream over the first 16 plants: a warm-started
    oracle.Solver per plant, workload.simulate + plant_noise, re-synchronised to the device's X after each step;
    that test's tolerances."""
    nref = 16
    ops = _ops(plant, N0)
    X, U, rec, _ = _record(plant, "tile", "f64")
    l, u0 = np.full(2 * N0, LMIN), oracle.upper_bound(ops, np.zeros(4), 0.0)
    refs = [oracle.Solver(ops["P"], np.zeros(N0), ops["A"], l, u0) for _ in range(nref)]
    Xk, Uk = X[:nref].copy(), U[:nref].copy()
    for k in range(K0):
        its = np.zeros(nref, dtype=np.int32)
        for b, r in enumerate(refs):
            assert r.update_gradient(oracle.gradient(ops, Xk[b], Uk[b], XREF))
            assert r.update_upper_bound(oracle.upper_bound(ops, Xk[b], Uk[b]))
            if r.solve() == oracle.SOLVED:
                Uk[b] += r.x()[0]
            its[b] = r.info().iter
        np.testing.assert_allclose(rec["U"][k, :nref], Uk, rtol=0, atol=1e-9, err_msg=f"step {k}")
        Xk = workload.simulate(plant["Ad"], plant["Bd"], Xk, Uk, workload.plant_noise(SEED, 0, B0, k, 4, NOISE)[:nref])
        np.testing.assert_allclose(rec["X"][k, :nref], Xk, rtol=1e-11, atol=1e-12, err_msg=f"step {k}")
        assert np.all(rec["status"][k, :nref] == sm.SOLVED), k
        assert np.array_equal(rec["iter"][k, :nref], its), (k, rec["iter"][k, :nref], its)
        Xk = rec["X"][k, :nref].copy()  # keep the oracle on the device's trajectory (libm vs device math)


# ---- 3. with a reference schedule -------------------------------------------------------------------
def _sched_record(plant, path):
    key = ("sched", path)
    if key not in _CACHE:
        X, U = workload.stream_states(4, 0, B0)
        sched = _schedules(B0, 8)
        with _env(**PATHS[path]):
            s = _ctx(plant, N0, B0)
            rec = _logged(s, X, U, K0, path, sched=sched)[0]
            s.close()
        _CACHE[key] = (X, U, sched, rec)
    return _CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["tile", "graph"])
def test_record_with_a_reference_schedule(plant, path):
    X, U, sched, rec = _sched_record(plant, path)
    with _env(**PATHS[path]):
        s = _ctx(plant, N0, B0)
        trace = _trace(s, X, U, K0, path, sched=sched)
        s.close()
    _same(rec, trace, path)
    assert np.all(rec["status"] == sm.SOLVED)


# ---- 4. failing steps -------------------------------------------------------------------------------
def _failing_records(plant):
    """The set-up of tests/test_gpu.py test_stream_failed_steps_advance (B = 8, four plants per wave, the first
    wave's states scaled by 1e29, 5 steps, f32), logged on the tile stream and on the per-step graph."""
    if "failing" not in _CACHE:
        B, steps = 8, 5
        X, U = workload.stream_states(4, 0, B)
        X[:4] *= 1e29
        recs = {}
        for path in ("tile", "graph"):
            with _env(MPCQ_KERNEL="tile", MPCQ_STREAM_CPW="4", **PATHS[path]):
                s = _ctx(plant, N0, B, "f32")
                recs[path] = _logged(s, X, U, steps, path)[0]
                s.close()
        _CACHE["failing"] = (X, U, steps, recs)
    return _CACHE["failing"]


@pytest.mark.gpu
def test_record_of_failing_steps(plant):
    """The first wave's four plants fail OSQP's bound update at every step (U unchanged) and still advance their
    plant; the tile stream's record equals the per-step graph's."""
    X, U, steps, recs = _failing_records(plant)
    t = recs["tile"]
    print("status rows of the failing plants:\n", t["status"][:, :4])
    _same(t, recs["graph"], "tile against graph")
    assert np.all(t["status"][:, 4:] == sm.SOLVED) and not np.any(t["status"][:, :4] == sm.SOLVED)
    assert np.all(t["U"][:, :4] == U[:4])  # constant: no step applied a move
    for k in range(1, steps):
        assert not np.any(np.all(t["X"][k, :4] == t["X"][k - 1, :4], axis=1))  # the failing plants still move


@pytest.mark.gpu
def test_failing_steps_are_type_changed_at_every_step(plant):
    """The same record: the status rows of the first four plants are TYPE_CHANGED at every step.

    The record first showed plants 2 and 3 ending their first one or two steps INVALID_BOUNDS: the tile kernel's
    free-lower-bound path compared u^ with -OSQP_INFTY in place of the row's l^, so a state scaled by 1e29, which
    drives some u^ below -1e30, was rejected as u < l although l = -DBL_MAX.  The wave and lane kernels compare
    with l itself and say TYPE_CHANGED; the tile kernel now re-reads the row's l in that case and agrees."""
    _, _, _, recs = _failing_records(plant)
    assert np.all(recs["tile"]["status"][:, :4] == sm.TYPE_CHANGED), recs["tile"]["status"][:, :4]


# ---- 5. other shapes --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_record_on_an_unpaired_shape(plant):
    """N = 15 is not a multiple of four: not the tile stream.  The record equals the trace on the path it takes."""
    N, B = 15, 7
    X, U = workload.stream_states(4, 0, B)
    with _env():
        s = _ctx(plant, N, B)
        Xd, Ud = _dev(X.copy()), _dev(U.copy())
        import torch
        _call(s, Xd, Ud, torch.cuda.Stream(), 0, 1)
        path = s.stream_path()
        s.close()
        assert path != "tile"
        s = _ctx(plant, N, B)
        rec = _logged(s, X, U, K0, path)[0]
        s.close()
        s = _ctx(plant, N, B)
        trace = _trace(s, X, U, K0, path)
        s.close()
    _same(rec, trace, f"N 15 on {path}")


@pytest.mark.gpu
def test_record_of_a_per_plant_context(plant):
    B = 5
    X, U = workload.stream_states(4, 0, B)
    with _env():
        s = _plants_ctx(plant, N0, B)
        rec = _logged(s, X, U, K0, "wave")[0]
        s.close()
        s = _plants_ctx(plant, N0, B)
        trace = _trace(s, X, U, K0, "wave")
        s.close()
    _same(rec, trace, "per-plant wave")


# ---- 6. chunking and bounds -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["tile", "graph"])
def test_chunked_runs_fill_one_buffer(plant, path):
    import torch
    B, rows = 20, 12
    X, U = workload.stream_states(4, 0, B)
    with _env(**PATHS[path]):
        s = _ctx(plant, N0, B)
        whole = _logged(s, X, U, rows, path)[0]
        s.close()
        s = _ctx(plant, N0, B)
        Xd, Ud, st = _dev(X.copy()), _dev(U.copy()), torch.cuda.Stream()
        log = _Log(rows, B)
        log.attach(s, 0)
        _call(s, Xd, Ud, st, 0, 7)
        part = log.read()
        assert np.all(part["U"][7:] == SENT_F) and np.all(part["iter"][7:] == SENT_I)  # rows 7.. not yet written
        _call(s, Xd, Ud, st, 7, 5)
        _same(log.read(), whole, f"{path} chunks 7 + 5")
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["tile", "wave", "graph"])
def test_step0_and_row_bounds(plant, path):
    import torch
    B = 20
    X, U = workload.stream_states(4, 0, B)
    with _env(**PATHS[path]):
        # a record whose row 0 is step 3: a run from first_step 3 lands in row 0
        s = _ctx(plant, N0, B)
        rec = _logged(s, X, U, 4, path, first=3)[0]
        s.close()
        s = _ctx(plant, N0, B)
        _same(rec, _trace(s, X, U, 4, path, first=3), f"{path} step0 3")
        s.close()
        # runs that would leave the buffer: refused before anything is enqueued
        s = _ctx(plant, N0, B)
        Xd, Ud, st = _dev(X.copy()), _dev(U.copy()), torch.cuda.Stream()
        log = _Log(4, B)
        log.attach(s, 3)
        for first, steps in ((2, 2), (0, 1), (3, 5), (6, 2), (7, 1)):
            with pytest.raises(sm.MpcqError) as e:
                _call(s, Xd, Ud, st, first, steps)
            assert e.value.code == _capi.MPCQ_ERR_ARG, (first, steps)
            torch.cuda.synchronize()
            assert np.array_equal(Xd.cpu().numpy(), X) and np.array_equal(Ud.cpu().numpy(), U)
            assert log.untouched(), (first, steps)
        _call(s, Xd, Ud, st, 6, 1)  # the last row alone fits
        got = log.read()
        assert np.all(got["U"][:3] == SENT_F) and not np.any(got["U"][3] == SENT_F)
        s.close()


@pytest.mark.gpu
def test_set_stream_log_rejects_bad_capacity(plant):
    s = _ctx(plant, N0, 4)
    log = _Log(2, 4)
    for rows, step0 in ((0, 0), (-1, 0), (2, -1)):
        with pytest.raises(sm.MpcqError) as e:
            s.mpc_set_stream_log(log.ptr("U"), 0, 0, 0, rows, step0)
        assert e.value.code == _capi.MPCQ_ERR_ARG
    s.mpc_set_stream_log(0, 0, 0, 0, 0, -5)  # all pointers null: a detach, whatever the rest says
    s.close()


# ---- 7. partial and detached ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["tile", "wave", "graph"])
def test_partial_record_and_detach(plant, path):
    import torch
    X, U, full, extra = _record(plant, path, "f64")
    with _env(**PATHS[path]):
        s = _ctx(plant, N0, B0)
        Xd, Ud, st = _dev(X.copy()), _dev(U.copy()), torch.cuda.Stream()
        log = _Log(K0, B0, which=("U",))
        log.attach(s, 0)
        _call(s, Xd, Ud, st, 0, K0)
        assert s.stream_path() == path
        got = log.read()  # (asserts X, status, iter stayed sentinels)
        assert np.array_equal(got["U"], full["U"])
        assert np.array_equal(Xd.cpu().numpy(), extra[0]) and np.array_equal(Ud.cpu().numpy(), extra[1])
        # detached: a further run of the same steps (the graph path: the same captured key) writes nothing
        s.mpc_set_stream_log()
        log2 = _Log(K0, B0)
        keep = {k: v.clone() for k, v in log.t.items()}
        _call(s, Xd, Ud, st, 0, K0)
        assert s.stream_path() == path
        assert log2.untouched()
        for k in NAMES:
            assert torch.equal(log.t[k], keep[k]), k
        s.close()


# ---- 8. the host convenience ------------------------------------------------------------------------
@pytest.mark.gpu
def test_rollout_scalar_reference(plant):
    X, U, rec, extra = _record(plant, "tile", "f64")
    with _env():
        s = _ctx(plant, N0, B0)
        out = s.mpc_rollout(X, U, K0, SEED, NOISE, xref=XREF)
        assert s.stream_path() == "tile"
        _same({k: out[k] for k in NAMES}, rec, "rollout xref")
        assert out["U"].shape == (K0, B0) and out["X"].shape == (K0, B0, 4)
        assert np.array_equal(out["X_final"], extra[0]) and np.array_equal(out["U_final"], extra[1])
        # the record is detached again: a plain run afterwards is a plain run
        import torch
        Xd, Ud, st = _dev(X.copy()), _dev(U.copy()), torch.cuda.Stream()
        s.reset_state()
        _call(s, Xd, Ud, st, 0, 2)
        s.close()


@pytest.mark.gpu
def test_rollout_schedules(plant):
    X, U, sched, rec = _sched_record(plant, "tile")
    with _env():
        s = _ctx(plant, N0, B0)
        out = s.mpc_rollout(X, U, K0, SEED, NOISE, sched=sched)
        s.close()
        _same({k: out[k] for k in NAMES}, rec, "rollout per-QP schedule")
        shared = sched[3]
        s = _ctx(plant, N0, B0)
        out = s.mpc_rollout(X, U, K0, SEED, NOISE, sched=shared)
        s.close()
        s = _ctx(plant, N0, B0)
        trace = _trace(s, X, U, K0, "tile", sched=shared)
        s.close()
        _same({k: out[k] for k in NAMES}, trace, "rollout shared schedule")
        with pytest.raises(ValueError):
            _ctx(plant, N0, B0).mpc_rollout(X, U, K0, SEED, NOISE, sched=sched[:7])

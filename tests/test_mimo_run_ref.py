"""CPU statement of the closed-loop MIMO run (mpcq_mimo_set_plant_device, mpcq_mimo_simulate_device,
mpcq_mimo_run_device, mpcq_mimo_run_ref_device), without any device code.

* The sliding window.  Control step s of a run reads ref[i] = sched[min(s + i, L - 1)], i < N.  The host passes the
  schedule itself (offset s) while s + N <= L and otherwise a window of the padded tail
  tail[j] = sched[min(base + j, L - 1)], j < 2N - 1, base = max(L - N, 0), at offset min(s - base, N - 1).  Both are
  compared with the hold-last window for every N in 1..6, L in 1..2N+1, s in 0..L+N and n_y in {1, 2}; no index
  leaves the schedule or the tail.
* ``workload.simulate_mimo`` against a per-QP loop that states the row in scalars, bit for bit, and against the
  matrix products within 1e-12 of sum|Ad_i||x| + sum|Bd_i||u| + |w_i| (the rounding bound of a row is (n_x + n_u + 2) eps
  = 2e-15 of that scale for n_x <= 12, n_u <= 4).
* The schedules and windows the GPU tests (tests/test_mimo_run.py) use.

The last two tests fail without the feature: the entry points in the header, the ctypes mirror and the built library,
and the Python names."""
import subprocess

import numpy as np

import solvempc_amd as sm
from solvempc_amd import _capi, workload

from test_mimo_ref_ref import _dims, _yref
from test_sensitivity_ref import ROOT, _declared

NEW_SYMBOLS = ("mpcq_mimo_set_plant_device", "mpcq_mimo_simulate_device", "mpcq_mimo_run_device",
               "mpcq_mimo_run_ref_device")


def _schedule(fam, L):
    """(B, L, n_y): every plant's reference steps between two random levels at a block of its own (1 .. L-1)."""
    B, N, nx, nu, ny = _dims(fam)
    rng = np.random.default_rng(2025)
    scale = np.abs(_yref(fam)).max()
    lo, hi = scale * rng.normal(size=(B, 1, ny)), scale * rng.normal(size=(B, 1, ny))
    at = (N // 2 + np.arange(B) - 1) % (L - 1) + 1
    return np.where(np.arange(L)[None, :, None] < at[:, None, None], lo, hi)


def _window(sched, s, N):
    """The hold-last window of control step s: (..., N n_y) from a schedule (..., L, n_y)."""
    L = sched.shape[-2]
    w = sched[..., np.minimum(s + np.arange(N), L - 1), :]
    return np.ascontiguousarray(w.reshape(w.shape[:-2] + (-1,)))


def _run_window(sched, s, N):
    """The window as mpcq_mimo_run_ref_device forms it for one schedule row (L, n_y): in place, or from the tail."""
    L, ny = sched.shape
    flat = sched.reshape(-1)
    if s + N <= L:
        lo = s * ny
        assert lo + N * ny <= flat.size
        return flat[lo:lo + N * ny]
    base = max(L - N, 0)
    idx = np.minimum(base + np.arange(2 * N - 1), L - 1)
    assert idx.min() >= 0
    tail = sched[idx].reshape(-1)
    lo = min(s - base, N - 1) * ny
    assert 0 <= lo and lo + N * ny <= tail.size
    return tail[lo:lo + N * ny]


def test_tail_window_is_the_hold_last_window():
    rng = np.random.default_rng(5)
    cases = 0
    for N in range(1, 7):
        for L in range(1, 2 * N + 2):
            for ny in (1, 2):
                sched = rng.normal(size=(L, ny))
                for s in range(L + N + 1):
                    assert np.array_equal(_run_window(sched, s, N), _window(sched, s, N)), (N, L, ny, s)
                    cases += 1
    print(f"{cases} windows")


def test_standard_schedule_reads_in_place_then_the_tail():
    """L = N + 2 and five steps: steps 0-2 read the schedule in place, steps 3-4 the tail; the switching blocks differ
    between neighbouring plants and lie inside the schedule."""
    for fam in "ABC":
        B, N, nx, nu, ny = _dims(fam)
        L = N + 2
        sched = _schedule(fam, L)
        assert sched.shape == (B, L, ny)
        assert [s + N <= L for s in range(5)] == [True, True, True, False, False]
        at = np.array([int(np.flatnonzero((sched[b, 1:] != sched[b, :-1]).any(axis=1))[0]) + 1 for b in range(B)])
        assert at.min() >= 1 and at.max() <= L - 1 and np.all(at[1:] != at[:-1])


def test_simulate_mimo_is_the_row_in_scalars():
    rng = np.random.default_rng(11)
    worst = 0.0
    for B, nx, nu in ((5, 3, 2), (4, 12, 4), (6, 4, 1), (3, 1, 1)):
        Ad, Bd = rng.normal(size=(B, nx, nx)), rng.normal(size=(B, nx, nu))
        X, U, w = rng.normal(size=(B, nx)), rng.normal(size=(B, nu)), 0.01 * rng.normal(size=(B, nx))
        got = workload.simulate_mimo(Ad, Bd, X, U, w)
        assert got.shape == (B, nx)
        for b in range(B):
            for i in range(nx):
                s = 0.0
                for t in range(nx):
                    s += Ad[b, i, t] * X[b, t]
                for j in range(nu):
                    s += Bd[b, i, j] * U[b, j]
                assert got[b, i] == s + w[b, i], (b, i)
            scale = np.abs(Ad[b]) @ np.abs(X[b]) + np.abs(Bd[b]) @ np.abs(U[b]) + np.abs(w[b])
            err = np.abs(got[b] - (Ad[b] @ X[b] + Bd[b] @ U[b] + w[b]))
            worst = max(worst, (err / np.maximum(1.0, scale)).max())
            assert np.all(err <= 1e-12 * np.maximum(1.0, scale))
    print(f"simulate_mimo against the matrix products: {worst:.1e} of the scale (bound 1e-12)")


def test_mimo_run_entry_points_in_header_mirror_and_library():
    declared = _declared()
    lib = sm.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sm.library_path())], check=True, capture_output=True,
                        text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.EXPORTS, name
        assert name in exported, name
        f = getattr(lib, name)
        assert f.restype is not None and f.argtypes, name
    assert len(lib.mpcq_mimo_set_plant_device.argtypes) == 4 and len(lib.mpcq_mimo_simulate_device.argtypes) == 8
    assert len(lib.mpcq_mimo_run_device.argtypes) == 12 and len(lib.mpcq_mimo_run_ref_device.argtypes) == 14
    hdr = (ROOT / "include" / "mpcq.h").read_text()
    assert "typedef struct mpcq_mimo_log" in hdr and "DESIGN.md 4.19" in hdr
    assert [k for k, _ in _capi.MimoLog._fields_] == ["U", "X", "status", "iter", "iters_total", "unsolved_total",
                                                      "rows", "step0"]
    assert "MIMO (no stream)" not in hdr


def test_python_names_exist():
    for name in ("mimo_set_plant_device", "mimo_simulate_device", "mimo_run_device", "mimo_run_ref_device",
                 "mimo_rollout", "mimo_log"):
        assert callable(getattr(sm.BatchSolver, name)), name
    assert callable(workload.simulate_mimo)

"""solvempc_amd — MI355X-native batched condensed-MPC QP solver (drop-in for the QP solve path of
LukeSchmitt96/solveMPC).

Python mirror of the C ABI in ``include/mpcq.h`` (library ``solvempc_amd/libmpcq.so``, built for
gfx950).  Names follow the reference's solver interface as it is used in
src/ModelPredictiveControlAPI.cpp (osqp-eigen: ``updateGradient`` / ``updateUpperBound`` /
``solve`` / ``getSolution``; OSQP settings and status values).  There is no CPU path: importing works
anywhere the library exists, but creating a solver needs a gfx950 device and fails loudly otherwise.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import _capi
from ._capi import (  # noqa: F401
    MPCQ_F32, MPCQ_F64, MPCQ_F64_MIXED, MPCQ_MIX_R, SOLVED, SOLVED_INACCURATE, MAX_ITER_REACHED, PRIMAL_INFEASIBLE,
    PRIMAL_INFEASIBLE_INACCURATE, DUAL_INFEASIBLE, DUAL_INFEASIBLE_INACCURATE, NON_CVX, UNSOLVED,
    INVALID_BOUNDS, TYPE_CHANGED, MpcqError, Settings, lib, library_path,
)

__all__ = ["BatchSolver", "Settings", "default_settings", "lib", "library_path", "MpcqError"]


def default_settings(**over) -> Settings:
    """OSQP v0.6 defaults + warm start (ModelPredictiveControlAPI.cpp:51-52)."""
    s = Settings()
    lib().mpcq_default_settings(C.byref(s))
    for k, v in over.items():
        if not hasattr(s, k):
            raise AttributeError(f"unknown setting {k}")
        setattr(s, k, v)
    return s


def _c64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class BatchSolver:
    """A batch of independent QPs  min 1/2 x'Px + q'x  s.t. l <= Ax <= u  on one gfx950 device.

    ``n_plants == 1``: all QPs share P and A (the reference's controller replicated over many
    states).  ``n_plants == batch``: one (P, A) per QP.
    """

    def __init__(self, n: int, m: int, batch: int, n_plants: int = 1, dtype: str = "f64",
                 device: int = 0, settings: Settings | None = None):
        self.n, self.m, self.batch, self.n_plants = int(n), int(m), int(batch), int(n_plants)
        self.dtype = dtype
        self.settings = settings or default_settings()
        codes = {"f64": MPCQ_F64, "f32": MPCQ_F32, "mixed": MPCQ_F64_MIXED}
        if dtype not in codes:
            raise ValueError(f"dtype {dtype!r}: one of {sorted(codes)}")
        dims = _capi.Dims(self.n, self.m, self.batch, self.n_plants, codes[dtype], int(device))
        ctx = C.c_void_p()
        _capi.check(lib().mpcq_create(C.byref(dims), C.byref(self.settings), C.byref(ctx)), "mpcq_create")
        self._ctx = ctx
        self.device = int(device)
        self.nx = 0
        self.solve_count = 0  # bumped by every solving method (diff.mpc_solution's backward checks it)

    def close(self):
        ctx = getattr(self, "_ctx", None)
        if ctx:
            self._ctx = None
            try:
                lib().mpcq_destroy(ctx)
            except TypeError:  # interpreter shutdown: module globals already torn down
                pass

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- setup: setHessianMatrix / setGradient / setLinearConstraintsMatrix / set*Bound + initSolver
    def setup(self, P, q0, A, l0, u0) -> None:
        k = self.n_plants
        P = _c64(P).reshape(k, self.n, self.n)
        q0 = _c64(q0).reshape(k, self.n)
        A = _c64(A).reshape(k, self.m, self.n)
        l0 = _c64(l0).reshape(k, self.m)
        u0 = _c64(u0).reshape(k, self.m)
        _capi.check(lib().mpcq_setup(self._ctx, _dp(P), _dp(q0), _dp(A), _dp(l0), _dp(u0)), "mpcq_setup")

    # -- per-step updates (updateGradient :96, updateUpperBound :99)
    def update_lin_cost(self, q) -> None:
        q = _c64(q).reshape(self.batch, self.n)
        _capi.check(lib().mpcq_update_lin_cost(self._ctx, _dp(q)), "mpcq_update_lin_cost")

    update_gradient = update_lin_cost

    def update_upper_bound(self, u) -> None:
        u = _c64(u).reshape(self.batch, self.m)
        _capi.check(lib().mpcq_update_upper_bound(self._ctx, _dp(u)), "mpcq_update_upper_bound")

    def update_lower_bound(self, l) -> None:
        l = _c64(l).reshape(self.batch, self.m)
        _capi.check(lib().mpcq_update_lower_bound(self._ctx, _dp(l)), "mpcq_update_lower_bound")

    def update_bounds(self, l, u) -> None:
        l = _c64(l).reshape(self.batch, self.m)
        u = _c64(u).reshape(self.batch, self.m)
        _capi.check(lib().mpcq_update_bounds(self._ctx, _dp(l), _dp(u)), "mpcq_update_bounds")

    def warm_start(self, x, y) -> None:
        x = _c64(x).reshape(self.batch, self.n)
        y = _c64(y).reshape(self.batch, self.m)
        _capi.check(lib().mpcq_warm_start(self._ctx, _dp(x), _dp(y)), "mpcq_warm_start")

    def cold_start(self) -> None:
        _capi.check(lib().mpcq_cold_start(self._ctx), "mpcq_cold_start")

    # -- new matrices with a warm start (osqp_update_P_A; updateHessianMatrix / updateLinearConstraintsMatrix)
    def update_P_A(self, P=None, A=None, rescale: bool = True) -> None:
        """New P (n_plants, n, n; upper triangle read) and / or A (n_plants, m, n) for a solver that is set up;
        None keeps the current matrix.  Every QP keeps its q, l, u and the next solve is warm-started from the
        previous (x, y); rho returns to settings.rho.  ``rescale=True`` equilibrates again (OSQP's behaviour),
        ``rescale=False`` keeps the scaling of the last setup and rebuilds the factors alone (n <= 32, m <= 64)."""
        k = self.n_plants
        Pp = Ap = None
        if P is not None:
            P = _c64(P).reshape(k, self.n, self.n)
            Pp = _dp(P)
        if A is not None:
            A = _c64(A).reshape(k, self.m, self.n)
            Ap = _dp(A)
        _capi.check(lib().mpcq_update_P_A(self._ctx, Pp, Ap, int(bool(rescale))), "mpcq_update_P_A")

    def update_P_A_device(self, P_ptr: int = 0, A_ptr: int = 0, rescale: int = 1, stream: int | None = None) -> None:
        """Same from device-resident fp64 buffers (0 keeps the current matrix); asynchronous on ``stream``, ordered
        after the solver's last stream, and the next solve is ordered after it."""
        _capi.check(lib().mpcq_update_P_A_device(self._ctx, C.c_void_p(P_ptr or 0), C.c_void_p(A_ptr or 0), int(rescale),
                                                 C.c_void_p(stream or 0)), "mpcq_update_P_A_device")

    def reset_state(self) -> None:
        """Back to the post-setup state (x = z = y = 0, rho = settings.rho) for the next solve."""
        _capi.check(lib().mpcq_reset(self._ctx), "mpcq_reset")

    # -- solve (:102) and results (:105)
    def solve(self, stream: int | None = None) -> None:
        self.solve_count += 1
        _capi.check(lib().mpcq_solve(self._ctx, C.c_void_p(stream or 0)), "mpcq_solve")

    def solution(self) -> np.ndarray:
        x = np.empty((self.batch, self.n))
        _capi.check(lib().mpcq_get_solution(self._ctx, _dp(x)), "mpcq_get_solution")
        return x

    def dual(self) -> np.ndarray:
        y = np.empty((self.batch, self.m))
        _capi.check(lib().mpcq_get_dual(self._ctx, _dp(y)), "mpcq_get_dual")
        return y

    def info(self):
        st = np.empty(self.batch, dtype=np.int32)
        it = np.empty(self.batch, dtype=np.int32)
        rho = np.empty(self.batch)
        _capi.check(lib().mpcq_get_info(self._ctx, st.ctypes.data_as(C.POINTER(C.c_int)),
                                        it.ctypes.data_as(C.POINTER(C.c_int)), _dp(rho)), "mpcq_get_info")
        return st, it, rho

    # -- active-set sensitivities of the last solve (mpcq_sensitivity*, mpcq_mpc_step_gains*)
    def sensitivity(self, g=None):
        """(gq, gl, gu, n_active) of the last solve for the cotangent ``g`` = dL/dx of shape (batch, n), or None
        for e_0 in every QP (the applied move x[0]): the vector-Jacobian product of x*(q, l, u) at the active set
        of the solve's final iterate, gq = dL/dq (batch, n), gl = dL/dl and gu = dL/du (batch, m); n_active the
        rows of the reduced system, -1 (and zero gradients) where the QP did not end SOLVED."""
        gp = None
        if g is not None:
            g = _c64(g).reshape(self.batch, self.n)
            gp = _dp(g)
        gq = np.empty((self.batch, self.n))
        gl, gu = np.empty((self.batch, self.m)), np.empty((self.batch, self.m))
        na = np.empty(self.batch, dtype=np.int32)
        _capi.check(lib().mpcq_sensitivity(self._ctx, gp, _dp(gq), _dp(gl), _dp(gu),
                                           na.ctypes.data_as(C.POINTER(C.c_int))), "mpcq_sensitivity")
        return gq, gl, gu, na

    def sensitivity_device(self, g_ptr: int = 0, gq_ptr: int = 0, gl_ptr: int = 0, gu_ptr: int = 0,
                           n_active_ptr: int = 0, stream: int | None = None) -> None:
        """Same on device-resident buffers (fp64; n_active int32); g_ptr 0: g = e_0; any output may be 0, not all.
        Asynchronous on ``stream``, ordered after the solver's last stream."""
        ptrs = [C.c_void_p(p or 0) for p in (g_ptr, gq_ptr, gl_ptr, gu_ptr, n_active_ptr)]
        _capi.check(lib().mpcq_sensitivity_device(self._ctx, *ptrs, C.c_void_p(stream or 0)),
                    "mpcq_sensitivity_device")

    def sensitivity_data(self, g=None):
        """(gq, gl, gu, gP, gA, active, n_active) of the last solve (mpcq_sensitivity_data): ``sensitivity`` plus
        the gradients with respect to the matrices, gP = 1/2 (gq x' + x gq') and gA = y_a gq' - (gl + gu) x' -- of
        shape (batch, n, n) and (batch, m, n) for a per-plant solver, summed over the batch to (n, n) and (m, n) for
        a shared plant -- and the active sets as bit masks, active[b] = (lower-active rows, upper-active rows) of
        QP b (uint64; bit i: row i).  gP is the gradient with respect to a symmetric P; for the upper triangle
        that ``setup`` reads take gP[i, j] + gP[j, i], i < j.  QPs with n_active = -1 contribute nothing."""
        gp = None
        if g is not None:
            g = _c64(g).reshape(self.batch, self.n)
            gp = _dp(g)
        k = (self.batch,) if self.n_plants != 1 else ()
        gq = np.empty((self.batch, self.n))
        gl, gu = np.empty((self.batch, self.m)), np.empty((self.batch, self.m))
        gP, gA = np.empty(k + (self.n, self.n)), np.empty(k + (self.m, self.n))
        act = np.empty((self.batch, 2), dtype=np.uint64)
        na = np.empty(self.batch, dtype=np.int32)
        _capi.check(lib().mpcq_sensitivity_data(self._ctx, gp, _dp(gq), _dp(gl), _dp(gu), _dp(gP), _dp(gA),
                                                act.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                                na.ctypes.data_as(C.POINTER(C.c_int))), "mpcq_sensitivity_data")
        return gq, gl, gu, gP, gA, act, na

    def sensitivity_data_device(self, g_ptr: int = 0, gq_ptr: int = 0, gl_ptr: int = 0, gu_ptr: int = 0,
                                gP_ptr: int = 0, gA_ptr: int = 0, active_ptr: int = 0, n_active_ptr: int = 0,
                                stream: int | None = None) -> None:
        """Same on device-resident buffers (fp64; active uint64 (batch, 2); n_active int32); g_ptr 0: g = e_0; any
        output may be 0, not all.  Asynchronous on ``stream``, ordered after the solver's last stream."""
        ptrs = [C.c_void_p(p or 0) for p in (g_ptr, gq_ptr, gl_ptr, gu_ptr, gP_ptr, gA_ptr, active_ptr, n_active_ptr)]
        _capi.check(lib().mpcq_sensitivity_data_device(self._ctx, *ptrs, C.c_void_p(stream or 0)),
                    "mpcq_sensitivity_data_device")

    def mpc_step_gains(self):
        """(dX, dU, dref, n_active) of the last MPC step: the gradient of the applied move x[0] with respect to
        the step's X (batch, nx), previous U (batch) and horizon reference (batch, n) at the current active set
        (after a scalar-xref step the gain with respect to xref is dref.sum(axis=1))."""
        dX, dU, dref = np.empty((self.batch, self.nx)), np.empty(self.batch), np.empty((self.batch, self.n))
        na = np.empty(self.batch, dtype=np.int32)
        _capi.check(lib().mpcq_mpc_step_gains(self._ctx, _dp(dX), _dp(dU), _dp(dref),
                                              na.ctypes.data_as(C.POINTER(C.c_int))), "mpcq_mpc_step_gains")
        return dX, dU, dref, na

    def mpc_step_gains_device(self, dX_ptr: int = 0, dU_ptr: int = 0, dref_ptr: int = 0, n_active_ptr: int = 0,
                              stream: int | None = None) -> None:
        """Same on device-resident buffers; asynchronous on ``stream``."""
        ptrs = [C.c_void_p(p or 0) for p in (dX_ptr, dU_ptr, dref_ptr, n_active_ptr)]
        _capi.check(lib().mpcq_mpc_step_gains_device(self._ctx, *ptrs, C.c_void_p(stream or 0)),
                    "mpcq_mpc_step_gains_device")

    def polish_info(self):
        """(status_polish, n_active, pri_res, dua_res) of the last solve (mpcq_get_polish_info): OSQP's
        status_polish per QP (1 successful, -1 unsuccessful, 0 not performed), the rows of its reduced KKT
        system, and the returned solution's residuals (NaN where polish was not performed)."""
        sp = np.empty(self.batch, dtype=np.int32)
        na = np.empty(self.batch, dtype=np.int32)
        pri, dua = np.empty(self.batch), np.empty(self.batch)
        ip = C.POINTER(C.c_int)
        _capi.check(lib().mpcq_get_polish_info(self._ctx, sp.ctypes.data_as(ip), na.ctypes.data_as(ip), _dp(pri),
                                               _dp(dua)), "mpcq_get_polish_info")
        return sp, na, pri, dua

    def scaling(self):
        D, E, c = np.empty(self.n), np.empty(self.m), C.c_double()
        _capi.check(lib().mpcq_get_scaling(self._ctx, _dp(D), _dp(E), C.byref(c)), "mpcq_get_scaling")
        return D, E, c.value

    def path(self) -> tuple[str, bool]:
        """(kernel family of the next solve: "tile" / "wave" / "lane", paired tile loop)."""
        k, p = C.c_int(), C.c_int()
        _capi.check(lib().mpcq_get_path(self._ctx, C.byref(k), C.byref(p)), "mpcq_get_path")
        return ("tile", "wave", "lane")[k.value], bool(p.value)

    def stream_path(self) -> str:
        """How the last mpc_run_device call ran: "tile" / "wave" (one launch) or "graph" (per-step)."""
        k = C.c_int()
        _capi.check(lib().mpcq_get_stream_path(self._ctx, C.byref(k)), "mpcq_get_stream_path")
        return ("graph", "wave", "tile")[k.value]

    def order(self) -> tuple[bool, np.ndarray]:
        """(whether the last solve ran hardest-first, the QPs in the order phase 0 ran them: mpcq_get_order)."""
        o, lst = C.c_int(), np.zeros(self.batch, dtype=np.int32)
        _capi.check(lib().mpcq_get_order(self._ctx, C.byref(o), lst.ctypes.data_as(C.POINTER(C.c_int))),
                    "mpcq_get_order")
        return bool(o.value), lst

    def device_view(self) -> dict:
        v = _capi.DeviceView()
        _capi.check(lib().mpcq_device_view_get(self._ctx, C.byref(v)), "mpcq_device_view_get")
        return {k: int(getattr(v, k) or 0) for k, _ in _capi.DeviceView._fields_}

    # -- condensed-MPC front end (controllerStep, :81-108)
    def mpc_set_operators(self, Fx, Fu, Fr, Sbar, Ku, W0) -> None:
        k = self.n_plants
        Fx = _c64(Fx).reshape(k, self.n, -1)
        self.nx = Fx.shape[2]
        args = [Fx, _c64(Fu).reshape(k, self.n), _c64(Fr).reshape(k, self.n, self.n),
                _c64(Sbar).reshape(k, self.m, self.nx), _c64(Ku).reshape(k, self.m), _c64(W0).reshape(k, self.m)]
        _capi.check(lib().mpcq_mpc_set_operators(self._ctx, self.nx, *[_dp(a) for a in args]),
                    "mpcq_mpc_set_operators")
        # (kept for solvempc_amd.diff, whose backward pass applies the front end's chain rule in torch)
        self._mpc_ops = dict(zip(("Fx", "Fu", "Fr", "Sbar", "Ku"), args[:5]))

    def mpc_step(self, X, U, xref: float = 0.0) -> np.ndarray:
        """One receding-horizon step for every QP from host X (batch, nx), U (batch); returns new U."""
        self.solve_count += 1
        X = _c64(X).reshape(self.batch, self.nx)
        U = _c64(U).reshape(self.batch).copy()
        _capi.check(lib().mpcq_mpc_step(self._ctx, _dp(X), _dp(U), float(xref)), "mpcq_mpc_step")
        return U

    # -- per-QP reference trajectories with horizon preview (mpcq_mpc_step_ref*, mpcq_mpc_run_ref_device)
    def mpc_step_ref(self, X, U, ref) -> np.ndarray:
        """mpc_step with a horizon reference: ``ref`` of shape (n,) is shared by the batch, (batch, n) is
        one per QP (q_b = Fx X_b + Fu U_b + Fr ref_b); returns new U."""
        self.solve_count += 1
        X = _c64(X).reshape(self.batch, self.nx)
        U = _c64(U).reshape(self.batch).copy()
        ref = _c64(ref)
        if ref.shape == (self.n,):
            stride = 0
        elif ref.shape == (self.batch, self.n):
            stride = self.n
        else:
            raise ValueError(f"ref of shape {ref.shape}: ({self.n},) or ({self.batch}, {self.n})")
        _capi.check(lib().mpcq_mpc_step_ref(self._ctx, _dp(X), _dp(U), _dp(ref), stride), "mpcq_mpc_step_ref")
        return U

    def mpc_step_ref_device(self, X_ptr: int, U_ptr: int, ref_ptr: int, ref_stride: int,
                            stream: int | None = None) -> None:
        """Same on device-resident fp64 buffers: QP b reads ref[b * ref_stride + j], j < n (ref_stride 0: one
        shared n-vector); the buffer must stay unchanged until the solve has finished.  Asynchronous."""
        self.solve_count += 1
        _capi.check(lib().mpcq_mpc_step_ref_device(self._ctx, C.c_void_p(X_ptr), C.c_void_p(U_ptr),
                                                   C.c_void_p(ref_ptr or 0), int(ref_stride),
                                                   C.c_void_p(stream or 0)), "mpcq_mpc_step_ref_device")

    def mpc_run_ref_device(self, X_ptr: int, U_ptr: int, sched_ptr: int, sched_len: int, sched_stride: int,
                           steps: int, seed: int, first_qp: int, first_step: int, noise_std: float,
                           stream: int) -> None:
        """mpc_run_device with a reference schedule: control step s = first_step + k of QP b uses
        ref[j] = sched[b * sched_stride + min(s + j, sched_len - 1)] (sched_stride 0: one shared schedule)."""
        self.solve_count += 1
        _capi.check(lib().mpcq_mpc_run_ref_device(self._ctx, C.c_void_p(X_ptr), C.c_void_p(U_ptr),
                                                  C.c_void_p(sched_ptr or 0), int(sched_len), int(sched_stride),
                                                  int(steps), seed, first_qp, first_step, float(noise_std),
                                                  C.c_void_p(stream)), "mpcq_mpc_run_ref_device")

    # -- receding-horizon stream (BASELINE config 5): simulated plant + graph-captured control steps
    def mpc_set_plant(self, Ad, Bd) -> None:
        k = self.n_plants
        Ad = _c64(Ad).reshape(k, -1)
        nx = int(round(np.sqrt(Ad.shape[1])))
        Bd = _c64(Bd).reshape(k, nx)
        _capi.check(lib().mpcq_mpc_set_plant(self._ctx, nx, _dp(Ad), _dp(Bd)), "mpcq_mpc_set_plant")

    def mpc_simulate_device(self, X_ptr: int, U_ptr: int, seed: int, first_qp: int, step: int,
                            noise_std: float, stream: int | None = None) -> None:
        _capi.check(lib().mpcq_mpc_simulate_device(self._ctx, C.c_void_p(X_ptr), C.c_void_p(U_ptr), seed, first_qp,
                                                   step, float(noise_std), C.c_void_p(stream or 0)),
                    "mpcq_mpc_simulate_device")

    def mpc_run_device(self, X_ptr: int, U_ptr: int, xref: float, steps: int, seed: int, first_qp: int,
                       first_step: int, noise_std: float, stream: int) -> None:
        """``steps`` warm-started [controllerStep; plant update] rounds: one persistent launch on the
        one-QP-per-wave path (every wave runs its QP through all the steps), else replayed from a
        hipGraph."""
        self.solve_count += 1
        _capi.check(lib().mpcq_mpc_run_device(self._ctx, C.c_void_p(X_ptr), C.c_void_p(U_ptr), float(xref),
                                              int(steps), seed, first_qp, first_step, float(noise_std),
                                              C.c_void_p(stream)), "mpcq_mpc_run_device")

    def stream_counters(self):
        """Per-QP (iterations, unsolved steps) accumulated over the last mpc_run_device call."""
        it = np.empty(self.batch, dtype=np.int32)
        un = np.empty(self.batch, dtype=np.int32)
        _capi.check(lib().mpcq_mpc_stream_counters(self._ctx, it.ctypes.data_as(C.POINTER(C.c_int)),
                                                   un.ctypes.data_as(C.POINTER(C.c_int))), "mpcq_mpc_stream_counters")
        return it, un

    def mpc_set_stream_log(self, U_ptr: int = 0, X_ptr: int = 0, status_ptr: int = 0, iter_ptr: int = 0,
                           rows: int = 0, step0: int = 0) -> None:
        """Attach a per-step record to every later mpc_run_device / mpc_run_ref_device call (mpcq_mpc_set_stream_log):
        device buffers, step-major, U (rows, batch) and X (rows, batch, nx) fp64, status and iter (rows, batch)
        int32; any may be 0 (not recorded).  The control step with absolute index ``step0 + r`` fills row r.  All
        zeros detaches."""
        log = _capi.StreamLog(U_ptr or None, X_ptr or None, status_ptr or None, iter_ptr or None, int(rows), int(step0))
        _capi.check(lib().mpcq_mpc_set_stream_log(self._ctx, C.byref(log)), "mpcq_mpc_set_stream_log")

    def mpc_rollout(self, X, U, steps: int, seed: int, noise_std: float, xref: float = 0.0, sched=None,
                    first_qp: int = 0, first_step: int = 0) -> dict:
        """One logged receding-horizon stream from host X (batch, nx), U (batch): ``steps`` control steps in one
        call, the whole closed-loop trajectory back.  ``sched`` (None: the scalar ``xref``) of shape (L,) is one
        reference schedule shared by the batch, (batch, L) one per QP (mpc_run_ref_device).  Returns numpy arrays
        ``U`` (steps, batch), ``X`` (steps, batch, nx), ``status``, ``iter`` (steps, batch) — row k: after control
        step first_step + k — and the final state ``X_final`` (batch, nx), ``U_final`` (batch).  The record is
        detached again on return."""
        import torch

        B, nx, steps = self.batch, self.nx, int(steps)
        dev = torch.device("cuda", self.device)
        Xd = torch.from_numpy(_c64(X).reshape(B, nx).copy()).to(dev)
        Ud = torch.from_numpy(_c64(U).reshape(B).copy()).to(dev)
        rows = max(steps, 1)
        lU = torch.zeros(rows, B, dtype=torch.float64, device=dev)
        lX = torch.zeros(rows, B, nx, dtype=torch.float64, device=dev)
        lS = torch.zeros(rows, B, dtype=torch.int32, device=dev)
        lI = torch.zeros(rows, B, dtype=torch.int32, device=dev)
        sd = None
        if sched is not None:
            sc = _c64(sched)
            if sc.ndim == 1:
                stride = 0
            elif sc.ndim == 2 and sc.shape[0] == B:
                stride = sc.shape[1]
            else:
                raise ValueError(f"sched of shape {sc.shape}: (L,) or ({B}, L)")
            sd = torch.from_numpy(sc.copy()).to(dev)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize(dev)
        self.mpc_set_stream_log(lU.data_ptr(), lX.data_ptr(), lS.data_ptr(), lI.data_ptr(), rows, first_step)
        try:
            if sd is None:
                self.mpc_run_device(Xd.data_ptr(), Ud.data_ptr(), xref, steps, seed, first_qp, first_step, noise_std,
                                    side.cuda_stream)
            else:
                self.mpc_run_ref_device(Xd.data_ptr(), Ud.data_ptr(), sd.data_ptr(), sc.shape[-1], stride, steps, seed,
                                        first_qp, first_step, noise_std, side.cuda_stream)
            side.synchronize()
        finally:
            self.mpc_set_stream_log()
        return {"U": lU[:steps].cpu().numpy(), "X": lX[:steps].cpu().numpy(), "status": lS[:steps].cpu().numpy(),
                "iter": lI[:steps].cpu().numpy(), "X_final": Xd.cpu().numpy(), "U_final": Ud.cpu().numpy()}

    def stream_iterations(self) -> np.ndarray:
        return self.stream_counters()[0]

    def stream_unsolved(self) -> int:
        return int(self.stream_counters()[1].sum())

    def mpc_setup_plants_device(self, nx: int, s_rows: int, Ad_ptr: int, Bd_ptr: int, Cd_ptr: int, K_ptr: int,
                                Q_ptr: int, R_ptr: int, RD_ptr: int, stream: int | None = None) -> None:
        """Condense and set up every plant on the device from device-resident plant data (fp64,
        plant-major; BASELINE config 3): the per-plant form of mpc.condense + setup +
        mpc_set_operators, with the ctor's X = U = 0 setup data."""
        ptrs = [C.c_void_p(p) for p in (Ad_ptr, Bd_ptr, Cd_ptr, K_ptr, Q_ptr, R_ptr, RD_ptr)]
        _capi.check(lib().mpcq_mpc_setup_plants_device(self._ctx, int(nx), int(s_rows), *ptrs,
                                                       C.c_void_p(stream or 0)), "mpcq_mpc_setup_plants_device")
        self.nx = int(nx)

    def mpc_plants_step_device(self, nx: int, s_rows: int, Ad_ptr: int, Bd_ptr: int, Cd_ptr: int, K_ptr: int,
                               Q_ptr: int, R_ptr: int, RD_ptr: int, X_ptr: int, U_ptr: int, xref: float = 0.0,
                               stream: int | None = None) -> None:
        """BASELINE config 3 in one pass: every plant's condensing + setup + one controllerStep (device
        pointers, plant-major fp64), operators kept on chip (the context keeps results only)."""
        self.solve_count += 1
        ptrs = [C.c_void_p(p) for p in (Ad_ptr, Bd_ptr, Cd_ptr, K_ptr, Q_ptr, R_ptr, RD_ptr, X_ptr, U_ptr)]
        _capi.check(lib().mpcq_mpc_plants_step_device(self._ctx, int(nx), int(s_rows), *ptrs, float(xref),
                                                      C.c_void_p(stream or 0)), "mpcq_mpc_plants_step_device")

    # -- MIMO condensed MPC (BASELINE config 4; oracle/mpc_mimo.h formulation)
    def mimo_setup_plants_device(self, nx: int, nu: int, ny: int, s_rows: int, Ad_ptr: int, Bd_ptr: int, Cd_ptr: int,
                                 Q_ptr: int, R_ptr: int, RD_ptr: int, K_ptr: int, K0_ptr: int, w0_ptr: int,
                                 stream: int | None = None) -> None:
        """Condense and set up every plant on the device from device-resident, plant-major fp64 data
        (Ad nx*nx, Bd nx*nu, Cd ny*nx, Q ny*ny, R, RD nu*nu, K nu*nx, K0 nu*nu, w0 nu)."""
        ptrs = [C.c_void_p(p) for p in (Ad_ptr, Bd_ptr, Cd_ptr, Q_ptr, R_ptr, RD_ptr, K_ptr, K0_ptr, w0_ptr)]
        _capi.check(lib().mpcq_mimo_setup_plants_device(self._ctx, int(nx), int(nu), int(ny), int(s_rows), *ptrs,
                                                        C.c_void_p(stream or 0)), "mpcq_mimo_setup_plants_device")
        self.nx, self.nu, self.ny = int(nx), int(nu), int(ny)

    def mimo_step_device(self, X_ptr: int, U_ptr: int, yref_ptr: int = 0, stream: int | None = None) -> None:
        """One controllerStep for every QP on device-resident X (batch, nx), U (batch, nu); asynchronous."""
        self.solve_count += 1
        _capi.check(lib().mpcq_mimo_step_device(self._ctx, C.c_void_p(X_ptr), C.c_void_p(U_ptr),
                                                C.c_void_p(yref_ptr or 0), C.c_void_p(stream or 0)),
                    "mpcq_mimo_step_device")

    def mimo_step_polish_device(self, X_ptr: int, U_ptr: int, yref_ptr: int = 0, stream: int | None = None) -> None:
        """``mimo_step_device`` followed by OSQP's polish of every SOLVED QP on the same stream (DESIGN.md 4.16;
        ``settings.polish`` stays 0): where polish succeeds the solution, the dual, the warm state and the applied
        move U = U_prev + x[:, :nu] are the polished point's, elsewhere the plain step's.  ``polish_info()`` reports
        the outcome; asynchronous."""
        self.solve_count += 1
        _capi.check(lib().mpcq_mimo_step_polish_device(self._ctx, C.c_void_p(X_ptr), C.c_void_p(U_ptr),
                                                       C.c_void_p(yref_ptr or 0), C.c_void_p(stream or 0)),
                    "mpcq_mimo_step_polish_device")

    # -- MIMO steps with a horizon reference per plant (mpcq_mimo_step_ref*)
    def mimo_step_ref_device(self, X_ptr: int, U_ptr: int, ref_ptr: int, ref_stride: int, polish: bool = False,
                             stream: int | None = None) -> None:
        """``mimo_step_device`` with an output reference over the horizon per QP: ``ref_ptr`` holds N*ny doubles
        (block i, then y) per QP, ``ref_stride`` doubles apart (0: one horizon reference for the batch), and must
        stay valid until the step has finished.  ``polish``: ``mimo_step_polish_device``'s pass afterwards.
        Asynchronous."""
        self.solve_count += 1
        _capi.check(lib().mpcq_mimo_step_ref_device(self._ctx, C.c_void_p(X_ptr), C.c_void_p(U_ptr),
                                                    C.c_void_p(ref_ptr or 0), int(ref_stride), int(polish),
                                                    C.c_void_p(stream or 0)), "mpcq_mimo_step_ref_device")

    def _mimo_ref_len(self) -> int:
        """N*ny, the doubles of one QP's horizon reference."""
        nu, ny = getattr(self, "nu", 0), getattr(self, "ny", 0)
        if not (nu and ny):
            raise RuntimeError("the solver has no MIMO plants (BatchSolver.mimo_setup_plants_device)")
        return self.n // nu * ny

    def mimo_step_ref(self, X, U, ref, polish: bool = False) -> np.ndarray:
        """Host arrays: X (batch, nx), U (batch, nu), ref (batch, N*ny), or (N*ny,) for one horizon reference shared
        by the batch.  Returns the new U (batch, nu)."""
        X, U, ref = _c64(X), _c64(U).copy(), _c64(ref)
        nr = self._mimo_ref_len()
        if X.shape != (self.batch, self.nx) or U.shape != (self.batch, self.nu) or \
                ref.shape not in ((nr,), (self.batch, nr)):
            raise ValueError(f"mimo_step_ref: X (batch, {self.nx}), U (batch, {self.nu}), ref (batch, {nr}) or ({nr},)")
        self.solve_count += 1
        _capi.check(lib().mpcq_mimo_step_ref(self._ctx, _dp(X), _dp(U), _dp(ref), nr if ref.ndim == 2 else 0,
                                             int(polish)), "mpcq_mimo_step_ref")
        return U

    def mimo_step_ref_vjp_device(self, g_ptr: int = 0, n_rhs: int = 1, dX_ptr: int = 0, dU_ptr: int = 0,
                                 dref_ptr: int = 0, n_active_ptr: int = 0, stream: int | None = None) -> None:
        """``mimo_step_vjp_device`` with the gradient of the horizon reference, dref (batch, n_rhs, N*ny), in place
        of dyref; asynchronous on ``stream``."""
        ptrs = [C.c_void_p(p or 0) for p in (dX_ptr, dU_ptr, dref_ptr, n_active_ptr)]
        _capi.check(lib().mpcq_mimo_step_ref_vjp_device(self._ctx, C.c_void_p(g_ptr or 0), int(n_rhs), *ptrs,
                                                        C.c_void_p(stream or 0)), "mpcq_mimo_step_ref_vjp_device")

    def mimo_step_ref_gains_device(self, dX_ptr: int = 0, dU_ptr: int = 0, dref_ptr: int = 0, n_active_ptr: int = 0,
                                   stream: int | None = None) -> None:
        """The gradients of the applied move x[0:n_u] with respect to X, the previous U and the horizon reference
        (``mimo_step_ref_vjp_device`` with g = e_r, n_rhs = n_u) on device-resident buffers; asynchronous."""
        ptrs = [C.c_void_p(p or 0) for p in (dX_ptr, dU_ptr, dref_ptr, n_active_ptr)]
        _capi.check(lib().mpcq_mimo_step_ref_gains_device(self._ctx, *ptrs, C.c_void_p(stream or 0)),
                    "mpcq_mimo_step_ref_gains_device")

    def mimo_step_ref_gains(self):
        """(dX, dU, dref, n_active) of the last MIMO step as numpy arrays: the gradient of component r of the applied
        move with respect to X (batch, nu, nx), the previous U (batch, nu, nu) and the QP's horizon reference
        (batch, nu, N*ny) at the current active set."""
        nr = self._mimo_ref_len()
        dX, dU = np.empty((self.batch, self.nu, self.nx)), np.empty((self.batch, self.nu, self.nu))
        dref, na = np.empty((self.batch, self.nu, nr)), np.empty(self.batch, dtype=np.int32)
        _capi.check(lib().mpcq_mimo_step_ref_gains(self._ctx, _dp(dX), _dp(dU), _dp(dref),
                                                   na.ctypes.data_as(C.POINTER(C.c_int))), "mpcq_mimo_step_ref_gains")
        return dX, dU, dref, na

    # -- closed-loop MIMO runs: simulated plant, reference schedule, record (mpcq_mimo_run*)
    def mimo_set_plant_device(self, Ad_ptr: int, Bd_ptr: int, stream: int | None = None) -> None:
        """The simulated plant of every QP, copied device-to-device from Ad (batch, nx, nx) and Bd (batch, nx, nu);
        it need not be the model the controller was set up with."""
        _capi.check(lib().mpcq_mimo_set_plant_device(self._ctx, C.c_void_p(Ad_ptr or 0), C.c_void_p(Bd_ptr or 0),
                                                     C.c_void_p(stream or 0)), "mpcq_mimo_set_plant_device")

    def mimo_simulate_device(self, X_ptr: int, U_ptr: int, seed: int, first_qp: int, step: int, noise_std: float,
                             stream: int | None = None) -> None:
        """One plant update in place, X_b <- Ad_b X_b + Bd_b U_b + workload.plant_noise(seed, first_qp + b, 1, step,
        nx, noise_std); asynchronous."""
        _capi.check(lib().mpcq_mimo_simulate_device(self._ctx, C.c_void_p(X_ptr or 0), C.c_void_p(U_ptr or 0), seed,
                                                    first_qp, step, float(noise_std), C.c_void_p(stream or 0)),
                    "mpcq_mimo_simulate_device")

    @staticmethod
    def mimo_log(U_ptr: int = 0, X_ptr: int = 0, status_ptr: int = 0, iter_ptr: int = 0, iters_total_ptr: int = 0,
                 unsolved_total_ptr: int = 0, rows: int = 0, step0: int = 0) -> _capi.MimoLog:
        """The record argument of ``mimo_run_device`` / ``mimo_run_ref_device`` (mpcq_mimo_log): device buffers,
        step-major U (rows, batch, nu) and X (rows, batch, nx) fp64, status and iter (rows, batch) int32, the totals
        (batch,) int32; any may be 0.  Control step ``step0 + r`` fills row r."""
        return _capi.MimoLog(U_ptr or None, X_ptr or None, status_ptr or None, iter_ptr or None,
                             iters_total_ptr or None, unsolved_total_ptr or None, int(rows), int(step0))

    def mimo_run_device(self, X_ptr: int, U_ptr: int, yref_ptr: int, steps: int, seed: int, first_qp: int,
                        first_step: int, noise_std: float, polish: bool = False, log: _capi.MimoLog | None = None,
                        stream: int | None = None) -> None:
        """``steps`` rounds of [``mimo_step_device`` (``polish``: ``mimo_step_polish_device``); ``mimo_simulate_device``]
        for the control steps first_step .. first_step+steps-1, bit for bit those calls; X, U evolve in place.
        Asynchronous."""
        self.solve_count += 1
        _capi.check(lib().mpcq_mimo_run_device(self._ctx, C.c_void_p(X_ptr or 0), C.c_void_p(U_ptr or 0),
                                               C.c_void_p(yref_ptr or 0), int(steps), seed, first_qp, first_step,
                                               float(noise_std), int(polish), C.byref(log) if log is not None else None,
                                               C.c_void_p(stream or 0)), "mpcq_mimo_run_device")

    def mimo_run_ref_device(self, X_ptr: int, U_ptr: int, sched_ptr: int, sched_len: int, sched_stride: int,
                            steps: int, seed: int, first_qp: int, first_step: int, noise_std: float,
                            polish: bool = False, log: _capi.MimoLog | None = None, stream: int | None = None) -> None:
        """``mimo_run_device`` with a reference schedule of ``sched_len`` blocks of ny values per QP, ``sched_stride``
        doubles apart (0: one for the batch): control step s is ``mimo_step_ref_device`` on the window
        ref[i] = sched[min(s + i, sched_len - 1)], i < N."""
        self.solve_count += 1
        _capi.check(lib().mpcq_mimo_run_ref_device(self._ctx, C.c_void_p(X_ptr or 0), C.c_void_p(U_ptr or 0),
                                                   C.c_void_p(sched_ptr or 0), int(sched_len), int(sched_stride),
                                                   int(steps), seed, first_qp, first_step, float(noise_std),
                                                   int(polish), C.byref(log) if log is not None else None,
                                                   C.c_void_p(stream or 0)), "mpcq_mimo_run_ref_device")

    def mimo_rollout(self, X, U, steps: int, seed: int, noise_std: float, yref=None, sched=None, polish: bool = False,
                     first_qp: int = 0, first_step: int = 0, Ad=None, Bd=None) -> dict:
        """One recorded closed-loop MIMO run from host X (batch, nx), U (batch, nu).  ``sched`` of shape (L, ny) is one
        reference schedule shared by the batch, (batch, L, ny) one per QP (``mimo_run_ref_device``); without it every
        step uses ``yref`` (ny values, None: 0; ``mimo_run_device``).  ``Ad`` (batch, nx, nx) and ``Bd`` (batch, nx, nu),
        when given, set the simulated plant first.  Returns numpy arrays ``U`` (steps, batch, nu), ``X`` (steps, batch,
        nx), ``status``, ``iter`` (steps, batch) -- row k: control step first_step + k -- ``iters_total``,
        ``unsolved_total`` (batch,), and the final ``X_final`` (batch, nx), ``U_final`` (batch, nu)."""
        import torch

        self._mimo_ref_len()  # (refuses a solver without MIMO plants)
        B, nx, nu, ny, steps = self.batch, self.nx, self.nu, self.ny, int(steps)
        if (Ad is None) != (Bd is None):
            raise ValueError("mimo_rollout: Ad and Bd are given together")
        if sched is not None and yref is not None:
            raise ValueError("mimo_rollout: yref or sched, not both")
        dev = torch.device("cuda", self.device)
        put = lambda a, shape: torch.from_numpy(_c64(a).reshape(shape).copy()).to(dev)
        Xd, Ud = put(X, (B, nx)), put(U, (B, nu))
        rows = max(steps, 1)
        lU = torch.zeros(rows, B, nu, dtype=torch.float64, device=dev)
        lX = torch.zeros(rows, B, nx, dtype=torch.float64, device=dev)
        lS, lI = (torch.zeros(rows, B, dtype=torch.int32, device=dev) for _ in range(2))
        tI, tU = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
        log = self.mimo_log(lU.data_ptr(), lX.data_ptr(), lS.data_ptr(), lI.data_ptr(), tI.data_ptr(), tU.data_ptr(),
                            rows, first_step)
        stream = torch.cuda.current_stream(dev).cuda_stream
        if Ad is not None:
            plant = put(Ad, (B, nx, nx)), put(Bd, (B, nx, nu))
            self.mimo_set_plant_device(plant[0].data_ptr(), plant[1].data_ptr(), stream)
        if sched is not None:
            sc = _c64(sched)
            if sc.ndim == 2 and sc.shape[1] == ny:
                stride = 0
            elif sc.ndim == 3 and sc.shape[0] == B and sc.shape[2] == ny:
                stride = sc.shape[1] * ny
            else:
                raise ValueError(f"sched of shape {sc.shape}: (L, {ny}) or ({B}, L, {ny})")
            sd = torch.from_numpy(sc.copy()).to(dev)
            self.mimo_run_ref_device(Xd.data_ptr(), Ud.data_ptr(), sd.data_ptr(), sc.shape[-2], stride, steps, seed,
                                     first_qp, first_step, noise_std, polish, log, stream)
        else:
            yd = put(yref, (ny,)) if yref is not None else None
            self.mimo_run_device(Xd.data_ptr(), Ud.data_ptr(), yd.data_ptr() if yd is not None else 0, steps, seed,
                                 first_qp, first_step, noise_std, polish, log, stream)
        torch.cuda.synchronize(dev)
        host = lambda t: t.cpu().numpy()
        return {"U": host(lU[:steps]), "X": host(lX[:steps]), "status": host(lS[:steps]), "iter": host(lI[:steps]),
                "iters_total": host(tI), "unsolved_total": host(tU), "X_final": host(Xd), "U_final": host(Ud)}

    # -- active-set sensitivities of the last MIMO step (mpcq_mimo_sensitivity*, mpcq_mimo_step_*)
    def mimo_sensitivity(self, g=None, n_rhs: int | None = None):
        """(gq, gu, n_active) of the last ``mimo_step_device``: ``g`` of shape (batch, n_rhs, n) (or (batch, n) for one
        right-hand side) holds the cotangents dL/dx; None stands for e_r, r < n_rhs (default n_u): the components
        of the applied move x[0:n_u].  gq (batch, n_rhs, n), gu (batch, n_rhs, m), n_active (batch), -1 (and zero
        gradients) where the QP did not end SOLVED."""
        gp = None
        if g is not None:
            g = _c64(g)
            if g.ndim == 2:
                g = g[:, None, :]
            n_rhs = g.shape[1] if n_rhs is None else int(n_rhs)
            g = np.ascontiguousarray(g.reshape(self.batch, n_rhs, self.n))
            gp = _dp(g)
        elif n_rhs is None:
            n_rhs = self.nu
        n_rhs = int(n_rhs)
        gq, gu = np.empty((self.batch, max(n_rhs, 0), self.n)), np.empty((self.batch, max(n_rhs, 0), self.m))
        na = np.empty(self.batch, dtype=np.int32)
        _capi.check(lib().mpcq_mimo_sensitivity(self._ctx, gp, n_rhs, _dp(gq), _dp(gu),
                                                na.ctypes.data_as(C.POINTER(C.c_int))), "mpcq_mimo_sensitivity")
        return gq, gu, na

    def mimo_sensitivity_device(self, g_ptr: int = 0, n_rhs: int = 1, gq_ptr: int = 0, gu_ptr: int = 0,
                                n_active_ptr: int = 0, stream: int | None = None) -> None:
        """Same on device-resident buffers (fp64; n_active int32); g_ptr 0: g_r = e_r; any output may be 0, not
        all.  Asynchronous on ``stream``, ordered after the solver's last stream."""
        _capi.check(lib().mpcq_mimo_sensitivity_device(self._ctx, C.c_void_p(g_ptr or 0), int(n_rhs),
                                                       C.c_void_p(gq_ptr or 0), C.c_void_p(gu_ptr or 0),
                                                       C.c_void_p(n_active_ptr or 0), C.c_void_p(stream or 0)),
                    "mpcq_mimo_sensitivity_device")

    def mimo_step_vjp_device(self, g_ptr: int = 0, n_rhs: int = 1, dX_ptr: int = 0, dU_ptr: int = 0,
                             dyref_ptr: int = 0, n_active_ptr: int = 0, stream: int | None = None) -> None:
        """The vector-Jacobian products of the last MIMO step with respect to X (batch, n_rhs, nx), U
        (batch, n_rhs, nu) and yref (batch, n_rhs, ny; per QP) for the cotangents at g_ptr (batch, n_rhs, n), on
        device-resident buffers; asynchronous on ``stream``."""
        ptrs = [C.c_void_p(p or 0) for p in (dX_ptr, dU_ptr, dyref_ptr, n_active_ptr)]
        _capi.check(lib().mpcq_mimo_step_vjp_device(self._ctx, C.c_void_p(g_ptr or 0), int(n_rhs), *ptrs,
                                                    C.c_void_p(stream or 0)), "mpcq_mimo_step_vjp_device")

    def mimo_step_gains_device(self, dX_ptr: int = 0, dU_ptr: int = 0, dyref_ptr: int = 0, n_active_ptr: int = 0,
                               stream: int | None = None) -> None:
        """The gradients of the applied move x[0:n_u] (``mimo_step_vjp_device`` with g = e_r, n_rhs = n_u) on
        device-resident buffers; asynchronous on ``stream``."""
        ptrs = [C.c_void_p(p or 0) for p in (dX_ptr, dU_ptr, dyref_ptr, n_active_ptr)]
        _capi.check(lib().mpcq_mimo_step_gains_device(self._ctx, *ptrs, C.c_void_p(stream or 0)),
                    "mpcq_mimo_step_gains_device")

    def mimo_step_gains(self):
        """(dX, dU, dyref, n_active) of the last MIMO step as numpy arrays: the gradient of component r of the
        applied move with respect to X (batch, nu, nx), the previous U (batch, nu, nu) and yref (batch, nu, ny; per
        QP) at the current active set."""
        import torch

        dev = torch.device("cuda", self.device)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
        dX, dU, dy = new(self.batch, self.nu, self.nx), new(self.batch, self.nu, self.nu), new(self.batch, self.nu, self.ny)
        na = torch.empty(self.batch, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev)
        self.mimo_step_gains_device(dX.data_ptr(), dU.data_ptr(), dy.data_ptr(), na.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        return dX.cpu().numpy(), dU.cpu().numpy(), dy.cpu().numpy(), na.cpu().numpy()

    # -- the last MIMO step differentiated in the plant data (mpcq_mimo_plant_vjp*)
    MIMO_PLANT_KEYS = ("Ad", "Bd", "Cd", "Q", "R", "RD", "K", "K0", "w0")

    def mimo_plant_vjp_device(self, g_ptr: int, plant_ptrs, X_ptr: int, U_prev_ptr: int, yref_ptr: int, grad_ptrs,
                              n_active_ptr: int = 0, stream: int | None = None) -> None:
        """The cotangent at g_ptr (batch, n; 0: e_0) of the last MIMO step's solution pulled back to the plant data,
        on device-resident fp64 buffers: ``plant_ptrs`` are the nine arrays ``mimo_setup_plants_device`` read, in
        its order (``MIMO_PLANT_KEYS``), ``grad_ptrs`` nine outputs of the same shapes (any may be 0, not all);
        X_ptr is the step's X, U_prev_ptr the U from before the step, yref_ptr its yref (0: none).  Asynchronous on
        ``stream``, ordered after the solver's last stream."""
        plant_ptrs, grad_ptrs = list(plant_ptrs), list(grad_ptrs)
        if len(plant_ptrs) != 9 or len(grad_ptrs) != 9:
            raise ValueError("mimo_plant_vjp_device: nine plant pointers and nine gradient pointers (MIMO_PLANT_KEYS)")
        ptrs = [C.c_void_p(p or 0) for p in [g_ptr] + plant_ptrs + [X_ptr, U_prev_ptr, yref_ptr] + grad_ptrs
                + [n_active_ptr]]
        _capi.check(lib().mpcq_mimo_plant_vjp_device(self._ctx, *ptrs, C.c_void_p(stream or 0)),
                    "mpcq_mimo_plant_vjp_device")

    def mimo_plant_vjp(self, plant: dict, X, U_prev, yref=None, g=None) -> dict:
        """Host-memory form: ``plant`` maps ``MIMO_PLANT_KEYS`` to arrays with a leading batch axis, X (batch, nx),
        U_prev (batch, nu), yref (ny) or None, g (batch, n) or None for e_0.  Returns a dict of the nine gradients
        under the same keys and ``n_active`` (batch; -1 and zero gradients where no sensitivity exists)."""
        keep = [np.ascontiguousarray(_c64(plant[k])) for k in self.MIMO_PLANT_KEYS]
        X, U_prev = np.ascontiguousarray(_c64(X)), np.ascontiguousarray(_c64(U_prev))
        yref = None if yref is None else np.ascontiguousarray(_c64(yref))
        g = None if g is None else np.ascontiguousarray(_c64(g).reshape(self.batch, self.n))
        for a in keep + [X, U_prev]:
            if a.shape[0] != self.batch:
                raise ValueError("mimo_plant_vjp: every array carries a leading batch axis")
        out = [np.empty_like(a) for a in keep]
        na = np.empty(self.batch, dtype=np.int32)
        opt = lambda a: None if a is None else _dp(a)
        _capi.check(lib().mpcq_mimo_plant_vjp(self._ctx, opt(g), *[_dp(a) for a in keep], _dp(X), _dp(U_prev), opt(yref),
                                              *[_dp(a) for a in out], na.ctypes.data_as(C.POINTER(C.c_int))),
                    "mpcq_mimo_plant_vjp")
        res = dict(zip(self.MIMO_PLANT_KEYS, out))
        res["n_active"] = na
        return res

    def mpc_step_device(self, X_ptr: int, U_ptr: int, xref: float = 0.0, stream: int | None = None) -> None:
        """Same on device-resident fp64 buffers (e.g. torch tensors' data_ptr()); asynchronous."""
        self.solve_count += 1
        _capi.check(lib().mpcq_mpc_step_device(self._ctx, C.c_void_p(X_ptr), C.c_void_p(U_ptr),
                                               float(xref), C.c_void_p(stream or 0)), "mpcq_mpc_step_device")


from .mpc import ModelPredictiveControlAPI, condense, condense_vjp, condense_vjp_device, from_json  # noqa: E402,F401

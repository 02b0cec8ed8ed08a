"""A differentiable MPC step for PyTorch: ``mpc_solution`` wraps ``BatchSolver.mpc_step_ref_device`` in a
``torch.autograd.Function`` whose backward pass is the solver's active-set sensitivity
(``BatchSolver.sensitivity_device``, solvempc_amd/csrc/mpcq_sens.hip) followed by the chain rule
through the front end's  q = Fx X + Fu U + Fr ref,  u = W0 + Sbar X + Ku U.

The gradient is that of the QP's optimum at the active set of the solve's final iterate; it is exact where the
active set does not change under an infinitesimal perturbation (strict complementarity), and zero for a QP that
did not end SOLVED.

``qp_solution`` is the QP itself as a layer: x*(P, A, q, l, u), with the gradients with respect to the matrices
from ``BatchSolver.sensitivity_data_device`` (solvempc_amd/csrc/mpcq_sensdata.hip).  Gradients with
respect to the front end's operators follow from it by autograd when q and u are formed from operator tensors in
torch; gradients through the condensing to the plant's Ad, Bd, Q, R are out of scope."""
from __future__ import annotations

import torch

__all__ = ["mpc_solution", "qp_solution"]


class _DevArray:
    """A device buffer of the solver's device view, wrapped for torch (__cuda_array_interface__)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3}


def _device_ops(solver) -> dict:
    """Device copies of the front-end operators the solver was given (mpc_set_operators), made once."""
    host = getattr(solver, "_mpc_ops", None)
    if host is None:
        raise RuntimeError("mpc_solution: the solver has no host-side MPC operators (BatchSolver.mpc_set_operators)")
    cached = getattr(solver, "_diff_ops", None)
    if cached is None or cached[0] is not host:
        dev = torch.device("cuda", solver.device)
        cached = (host, {k: torch.from_numpy(v).to(dev) for k, v in host.items()})
        solver._diff_ops = cached
    return cached[1]


class _MpcSolution(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, X, U, ref):
        B, n = solver.batch, solver.n
        _device_ops(solver)
        for name, t, shape in (("X", X, (B, solver.nx)), ("U", U, (B,)), ("ref", ref, (B, n))):
            if not (t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape):
                raise ValueError(f"mpc_solution: {name} must be a device fp64 tensor of shape {shape}")
        Xc, Uc, rc = X.detach().contiguous(), U.detach().clone().contiguous(), ref.detach().contiguous()
        stream = torch.cuda.current_stream(X.device).cuda_stream
        solver.mpc_step_ref_device(Xc.data_ptr(), Uc.data_ptr(), rc.data_ptr(), n, stream)
        view = solver.device_view()  # (publishes x and status on the same stream)
        x = torch.as_tensor(_DevArray(view["x"], (B, n), "<f8"), device=X.device).clone()
        status = torch.as_tensor(_DevArray(view["status"], (B,), "<i4"), device=X.device).clone()
        # (Xc, rc stay alive until the solve has finished: later phases of a tile solve re-form q from them)
        ctx.keep = (Xc, Uc, rc)
        ctx.solver, ctx.count = solver, solver.solve_count
        ctx.mark_non_differentiable(status)
        return x, status

    @staticmethod
    def backward(ctx, gx, _gstatus):
        solver = ctx.solver
        if solver.solve_count != ctx.count:
            raise RuntimeError("mpc_solution.backward: the solver has solved again since this forward pass, so its "
                               "state is no longer this solve's; run backward before the next solve")
        B, n, m = solver.batch, solver.n, solver.m
        g = gx.contiguous()
        gq = torch.empty(B, n, dtype=torch.float64, device=g.device)
        gu = torch.empty(B, m, dtype=torch.float64, device=g.device)
        stream = torch.cuda.current_stream(g.device).cuda_stream
        solver.sensitivity_device(g.data_ptr(), gq.data_ptr(), 0, gu.data_ptr(), 0, stream)
        ops = _device_ops(solver)
        p = "k" if solver.n_plants == 1 else "b"  # (one plant: its operators serve the whole batch)
        dX = torch.einsum(f"{p}ij,bi->bj", ops["Fx"], gq) + torch.einsum(f"{p}ij,bi->bj", ops["Sbar"], gu)
        dU = (ops["Fu"] * gq).sum(dim=1) + (ops["Ku"] * gu).sum(dim=1)
        dref = torch.einsum(f"{p}it,bi->bt", ops["Fr"], gq)
        return None, dX, dU, dref


class _QpSolution(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, P, A, q, l, u, setup):
        B, n, m = solver.batch, solver.n, solver.m
        k = () if solver.n_plants == 1 else (B,)
        if k and solver.n_plants != B:
            raise ValueError("qp_solution: the solver must have n_plants == 1 or n_plants == batch")
        for name, t, shape in (("P", P, k + (n, n)), ("A", A, k + (m, n)), ("q", q, (B, n)), ("l", l, (B, m)),
                               ("u", u, (B, m))):
            if not (t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape):
                raise ValueError(f"qp_solution: {name} must be a device fp64 tensor of shape {shape}")
        host = lambda t: t.detach().cpu().numpy()
        lh, uh, kp = host(l), host(u), solver.n_plants
        if setup:  # (each plant's first QP supplies the setup's bounds; every QP's own follow below)
            solver.setup(host(P), torch.zeros(kp, n, dtype=torch.float64).numpy(), host(A), lh[:kp], uh[:kp])
        solver.update_lin_cost(host(q))
        solver.update_bounds(lh, uh)
        solver.solve(torch.cuda.current_stream(q.device).cuda_stream)
        view = solver.device_view()  # (publishes x and status on the same stream)
        x =torch.as_tensor(_DevArray(view["x"], (B, n), "<f8"), device=q.device).clone()
        status = torch.as_tensor(_DevArray(view["status"], (B,), "<i4"), device=q.device).clone()
        ctx.solver, ctx.count, ctx.shapes = solver, solver.solve_count, (k + (n, n), k + (m, n))
        ctx.mark_non_differentiable(status)
        return x, status

    @staticmethod
    def backward(ctx, gx, _gstatus):
        solver = ctx.solver
        if solver.solve_count != ctx.count:
            raise RuntimeError("qp_solution.backward: the solver has solved again since this forward pass, so its "
                               "state is no longer this solve's; run backward before the next solve")
        B, n, m = solver.batch, solver.n, solver.m
        g = gx.contiguous()
        new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=g.device)
        gq, gl, gu, gP, gA = new(B, n), new(B, m), new(B, m), new(ctx.shapes[0]), new(ctx.shapes[1])
        stream = torch.cuda.current_stream(g.device).cuda_stream
        solver.sensitivity_data_device(g.data_ptr(), gq.data_ptr(), gl.data_ptr(), gu.data_ptr(), gP.data_ptr(),
                                       gA.data_ptr(), 0, 0, stream)
        return None, gP, gA, gq, gl, gu, None


def qp_solution(solver, P, A, q, l, u, setup=True):
    """The solutions of the batch of QPs  min 1/2 x'Px + q'x, l <= Ax <= u  as a differentiable function of all
    five tensors (device fp64): P (n, n) and A (m, n) for a shared-plant solver, (batch, n, n) and (batch, m, n)
    for a per-plant one; q (batch, n); l, u (batch, m).  Returns ``(x, status)`` as ``mpc_solution`` does.

    Forward: ``solver.setup(P, 0, A, l0, u0)`` with each plant's first QP's bounds, then ``update_lin_cost``,
    ``update_bounds`` and ``solve`` (host-side data updates).  With ``setup=False`` the caller vouches that the
    solver already holds P and A, and only q, l, u are updated.  Backward is one
    ``BatchSolver.sensitivity_data_device`` call: the gradient with respect to P is that of a
    symmetric P (``setup`` reads the upper triangle: a caller who parametrises that takes gP[i, j] + gP[j, i]);
    a shared plant's gP, gA are the sums over the batch.  ``backward`` must run before the solver solves again.
    Operator gradients (Fx, Fr, Sbar, ...) need no code: form q and u from operator tensors in torch."""
    return _QpSolution.apply(solver, P, A, q, l, u, setup)


def mpc_solution(solver, X, U, ref):
    """One MPC step ``solver.mpc_step_ref_device`` on device fp64 tensors X (batch, nx), U (batch), ref
    (batch, n), differentiable with respect to all three.  Returns ``(x, status)``: the QP solutions
    (batch, n) and the per-QP status (int32, not differentiable).  The caller's U is left alone (the step runs
    on a private copy; the applied move is x[:, 0]).  ``backward`` must run before the solver solves again."""
    return _MpcSolution.apply(solver, X, U, ref)

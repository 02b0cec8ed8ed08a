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
torch.

``mpc_plant_solution`` is the MPC step as a function of the plant model and the cost weights themselves: the
condensing and the setup run on the device from the plant tensors (``BatchSolver.mpc_setup_plants_device``), and
the backward pass chains ``sensitivity_data_device`` with the condensing's vector-Jacobian product
(``solvempc_amd.condense_vjp_device``, solvempc_amd/csrc/mpcq_condense_vjp.hip).

``mimo_solution`` is the MIMO step (``BatchSolver.mimo_step_device``; n up to 128) as a function of X, U and yref:
its backward pass is ``BatchSolver.mimo_step_vjp_device`` (solvempc_amd/csrc/mpcq_mimo_sens.hip)."""
from __future__ import annotations

import torch

__all__ = ["mpc_solution", "qp_solution", "mpc_plant_solution", "mimo_solution"]


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
        stream = torch.cuda.current_stream(q.device).cuda_stream
        if isinstance(setup, str):  # (new matrices from the tensors' own memory, warm-started: mpcq_update_P_A_device)
            if setup not in ("update", "update_keep"):
                raise ValueError(f"qp_solution: setup={setup!r}: True, False, 'update' or 'update_keep'")
            Pc, Ac = P.detach().contiguous(), A.detach().contiguous()
            solver.update_P_A_device(Pc.data_ptr(), Ac.data_ptr(), 0 if setup == "update_keep" else 1, stream)
            ctx.keep = (Pc, Ac)  # (alive until the copies enqueued on the stream have run)
        elif setup:  # (each plant's first QP supplies the setup's bounds; every QP's own follow below)
            solver.setup(host(P), torch.zeros(kp, n, dtype=torch.float64).numpy(), host(A), lh[:kp], uh[:kp])
        solver.update_lin_cost(host(q))
        solver.update_bounds(lh, uh)
        solver.solve(stream)
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


class _MimoSolution(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, polish, X, U, yref):
        B, n = solver.batch, solver.n
        nx, nu, ny = solver.nx, getattr(solver, "nu", 0), getattr(solver, "ny", 0)
        if not (nu and ny):
            raise RuntimeError("mimo_solution: the solver has no MIMO plants (BatchSolver.mimo_setup_plants_device)")
        for name, t, shape in (("X", X, (B, nx)), ("U", U, (B, nu)), ("yref", yref, (ny,))):
            if not (t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape):
                raise ValueError(f"mimo_solution: {name} must be a device fp64 tensor of shape {shape}")
        Xc, Uc, yc = X.detach().contiguous(), U.detach().clone().contiguous(), yref.detach().contiguous()
        stream = torch.cuda.current_stream(X.device).cuda_stream
        step = solver.mimo_step_polish_device if polish else solver.mimo_step_device
        step(Xc.data_ptr(), Uc.data_ptr(), yc.data_ptr(), stream)
        view = solver.device_view()
        x = torch.as_tensor(_DevArray(view["x"], (B, n), "<f8"), device=X.device).clone()
        status = torch.as_tensor(_DevArray(view["status"], (B,), "<i4"), device=X.device).clone()
        ctx.keep = (Xc, Uc, yc)
        ctx.solver, ctx.count, ctx.dims = solver, solver.solve_count, (nx, nu, ny)
        ctx.mark_non_differentiable(status)
        return x, status

    @staticmethod
    def backward(ctx, gx, _gstatus):
        solver = ctx.solver
        if solver.solve_count != ctx.count:
            raise RuntimeError("mimo_solution.backward: the solver has solved again since this forward pass, so its "
                               "state is no longer this solve's; run backward before the next solve")
        B, (nx, nu, ny) = solver.batch, ctx.dims
        g = gx.contiguous()
        new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=g.device)
        dX, dU, dy = new(B, nx), new(B, nu), new(B, ny)
        stream = torch.cuda.current_stream(g.device).cuda_stream
        solver.mimo_step_vjp_device(g.data_ptr(), 1, dX.data_ptr(), dU.data_ptr(), dy.data_ptr(), 0, stream)
        return None, None, dX, dU, dy.sum(dim=0)  # (yref is one vector for the whole batch)


class _MimoRefSolution(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, polish, X, U, ref):
        B, n = solver.batch, solver.n
        nx, nu, ny = solver.nx, getattr(solver, "nu", 0), getattr(solver, "ny", 0)
        if not (nu and ny):
            raise RuntimeError("mimo_ref_solution: the solver has no MIMO plants (BatchSolver.mimo_setup_plants_device)")
        nr = n // nu * ny
        for name, t, shape in (("X", X, (B, nx)), ("U", U, (B, nu)), ("ref", ref, (B, nr))):
            if not (t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shape):
                raise ValueError(f"mimo_ref_solution: {name} must be a device fp64 tensor of shape {shape}")
        Xc, Uc, rc = X.detach().contiguous(), U.detach().clone().contiguous(), ref.detach().contiguous()
        stream = torch.cuda.current_stream(X.device).cuda_stream
        solver.mimo_step_ref_device(Xc.data_ptr(), Uc.data_ptr(), rc.data_ptr(), nr, polish, stream)
        view = solver.device_view()
        x = torch.as_tensor(_DevArray(view["x"], (B, n), "<f8"), device=X.device).clone()
        status = torch.as_tensor(_DevArray(view["status"], (B,), "<i4"), device=X.device).clone()
        ctx.keep = (Xc, Uc, rc)  # (rc stays alive until the step has finished)
        ctx.solver, ctx.count, ctx.dims = solver, solver.solve_count, (nx, nu, nr)
        ctx.mark_non_differentiable(status)
        return x, status

    @staticmethod
    def backward(ctx, gx, _gstatus):
        solver = ctx.solver
        if solver.solve_count != ctx.count:
            raise RuntimeError("mimo_ref_solution.backward: the solver has solved again since this forward pass, so "
                               "its state is no longer this solve's; run backward before the next solve")
        B, (nx, nu, nr) = solver.batch, ctx.dims
        g = gx.contiguous()
        new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=g.device)
        dX, dU, dref = new(B, nx), new(B, nu), new(B, nr)
        stream = torch.cuda.current_stream(g.device).cuda_stream
        solver.mimo_step_ref_vjp_device(g.data_ptr(), 1, dX.data_ptr(), dU.data_ptr(), dref.data_ptr(), 0, stream)
        return None, None, dX, dU, dref


_MIMO_PLANT = ("Ad", "Bd", "Cd", "Q", "R", "RD", "K", "K0", "w0")


class _MimoPlantSolution(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, s_rows, polish, setup, Ad, Bd, Cd, Q, R, RD, K, K0, w0, X, U, yref):
        B, n, m = solver.batch, solver.n, solver.m
        if solver.n_plants != B or m != 2 * n:
            raise ValueError("mimo_plant_solution: the solver must have n_plants == batch and m == 2 n (the MIMO shape)")
        nx, nu = (int(Bd.shape[1]), int(Bd.shape[2])) if Bd.dim() == 3 else (0, 0)
        ny = int(Cd.shape[1]) if Cd.dim() == 3 else 0
        shapes = {"Ad": (B, nx, nx), "Bd": (B, nx, nu), "Cd": (B, ny, nx), "Q": (B, ny, ny), "R": (B, nu, nu),
                  "RD": (B, nu, nu), "K": (B, nu, nx), "K0": (B, nu, nu), "w0": (B, nu), "X": (B, nx), "U": (B, nu),
                  "yref": (ny,)}
        given = dict(zip(_MIMO_PLANT + ("X", "U", "yref"), (Ad, Bd, Cd, Q, R, RD, K, K0, w0, X, U, yref)))
        for name, t in given.items():
            if not (t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shapes[name]):
                raise ValueError(f"mimo_plant_solution: {name} must be a device fp64 tensor of shape {shapes[name]}")
        plant = [given[k].detach().contiguous() for k in _MIMO_PLANT]
        Xc, U0, yc = X.detach().contiguous(), U.detach().contiguous(), yref.detach().contiguous()
        Uc = U0.clone()  # (the step adds the applied move to its U)
        stream = torch.cuda.current_stream(X.device).cuda_stream
        if setup:
            solver.mimo_setup_plants_device(nx, nu, ny, int(s_rows), *[t.data_ptr() for t in plant], stream=stream)
        elif (solver.nx, getattr(solver, "nu", 0), getattr(solver, "ny", 0)) != (nx, nu, ny):
            raise ValueError("mimo_plant_solution: setup=False, but the solver holds no MIMO plants of these dimensions")
        step = solver.mimo_step_polish_device if polish else solver.mimo_step_device
        step(Xc.data_ptr(), Uc.data_ptr(), yc.data_ptr(), stream)
        view = solver.device_view()
        x = torch.as_tensor(_DevArray(view["x"], (B, n), "<f8"), device=X.device).clone()
        status = torch.as_tensor(_DevArray(view["status"], (B,), "<i4"), device=X.device).clone()
        ctx.keep = (plant, Xc, U0, yc, Uc)
        ctx.solver, ctx.count, ctx.dims = solver, solver.solve_count, (nx, nu, ny)
        ctx.mark_non_differentiable(status)
        return x, status

    @staticmethod
    def backward(ctx, gx, _gstatus):
        solver = ctx.solver
        if solver.solve_count != ctx.count:
            raise RuntimeError("mimo_plant_solution.backward: the solver has solved again since this forward pass, so "
                               "its state is no longer this solve's; run backward before the next solve")
        B, (nx, nu, ny), (plant, X, U0, yref, _) = solver.batch, ctx.dims, ctx.keep
        g = gx.contiguous()
        stream = torch.cuda.current_stream(g.device).cuda_stream
        grads = [None] * 9
        if any(ctx.needs_input_grad[4:13]):
            grads = [torch.empty_like(t) for t in plant]
            solver.mimo_plant_vjp_device(g.data_ptr(), [t.data_ptr() for t in plant], X.data_ptr(), U0.data_ptr(),
                                         yref.data_ptr(), [t.data_ptr() for t in grads], 0, stream)
            grads = [t if need else None for t, need in zip(grads, ctx.needs_input_grad[4:13])]
        dX = dU = dy = None
        if any(ctx.needs_input_grad[13:16]):
            new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=g.device)
            dX, dU, dy = new(B, nx), new(B, nu), new(B, ny)
            solver.mimo_step_vjp_device(g.data_ptr(), 1, dX.data_ptr(), dU.data_ptr(), dy.data_ptr(), 0, stream)
            dy = dy.sum(dim=0)  # (yref is one vector for the whole batch)
        return (None, None, None, None, *grads, dX, dU, dy)


_PLANT = ("Ad", "Bd", "Cd", "K", "Q", "R", "RD")


class _MpcPlantSolution(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, s_rows, setup, Ad, Bd, Cd, K, Q, R, RD, X, U, ref):
        from .mpc import condense
        B, n, m, kp = solver.batch, solver.n, solver.m, solver.n_plants
        if kp not in (1, B):
            raise ValueError("mpc_plant_solution: the solver must have n_plants == 1 or n_plants == batch")
        if m != 2 * n or n > 32:
            raise ValueError("mpc_plant_solution: the solver must have m == 2 n and n <= 32 (the condensed-MPC shape)")
        nx = int(Ad.shape[-1]) if Ad.dim() == 3 else 0
        shapes = {"Ad": (kp, nx, nx), "Bd": (kp, nx), "Cd": (kp, nx), "K": (kp, nx), "Q": (kp,), "R": (kp,),
                  "RD": (kp,), "X": (B, nx), "U": (B,), "ref": (B, n)}
        given = dict(zip(_PLANT + ("X", "U", "ref"), (Ad, Bd, Cd, K, Q, R, RD, X, U, ref)))
        for name, t in given.items():
            if not (t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == shapes[name]):
                raise ValueError(f"mpc_plant_solution: {name} must be a device fp64 tensor of shape {shapes[name]}")
        plant = [given[k].detach().contiguous() for k in _PLANT]
        Xc, U0, rc = X.detach().contiguous(), U.detach().contiguous(), ref.detach().contiguous()
        Uc = U0.clone()  # (the step adds the applied move to its U)
        stream = torch.cuda.current_stream(X.device).cuda_stream
        if setup:
            solver.mpc_setup_plants_device(nx, int(s_rows), *[t.data_ptr() for t in plant], stream)
        elif solver.nx != nx:
            raise ValueError(f"mpc_plant_solution: setup=False, but the solver holds plants of nx = {solver.nx}")
        solver.mpc_step_ref_device(Xc.data_ptr(), Uc.data_ptr(), rc.data_ptr(), n, stream)
        view = solver.device_view()  # (publishes x and status on the same stream)
        x = torch.as_tensor(_DevArray(view["x"], (B, n), "<f8"), device=X.device).clone()
        status = torch.as_tensor(_DevArray(view["status"], (B,), "<i4"), device=X.device).clone()
        ctx.ops = None
        if X.requires_grad or U.requires_grad or ref.requires_grad:  # (the chain rule of mpc_solution: via the host)
            host = condense({k: t.cpu().numpy() for k, t in zip(_PLANT, plant)}, n, int(s_rows), solver.device)
            ctx.ops = {k: torch.from_numpy(host[k]).to(X.device) for k in ("Fx", "Fu", "Fr", "Sbar", "Ku")}
        # (Xc, rc stay alive until the solve has finished: later phases of a tile solve re-form q from them)
        ctx.keep = (plant, Xc, U0, rc, Uc)
        ctx.solver, ctx.count, ctx.dims = solver, solver.solve_count, (nx, int(s_rows))
        ctx.mark_non_differentiable(status)
        return x, status

    @staticmethod
    def backward(ctx, gx, _gstatus):
        from .mpc import condense_vjp_device
        solver = ctx.solver
        if solver.solve_count != ctx.count:
            raise RuntimeError("mpc_plant_solution.backward: the solver has solved again since this forward pass, so "
                               "its state is no longer this solve's; run backward before the next solve")
        B, n, m, kp = solver.batch, solver.n, solver.m, solver.n_plants
        (nx, s_rows), (plant, X, U, ref, _) = ctx.dims, ctx.keep
        g = gx.contiguous()
        new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=g.device)
        gq, gu, gP, gA = new(B, n), new(B, m), new(kp, n, n), new(kp, m, n)
        stream = torch.cuda.current_stream(g.device).cuda_stream
        solver.sensitivity_data_device(g.data_ptr(), gq.data_ptr(), 0, gu.data_ptr(), gP.data_ptr(), gA.data_ptr(), 0, 0,
                                       stream)
        grads = [None] * 7
        if any(ctx.needs_input_grad[3:10]):
            # cotangents of the front end's operators: q = Fx X + Fu U + Fr ref, u = W0 + Sbar X + Ku U
            if kp == 1:
                cots = [gP, gA, gq.t() @ X, gq.t() @ U, gq.t() @ ref, gu.t() @ X, gu.t() @ U]
            else:
                cots = [gP, gA, gq[:, :, None] * X[:, None, :], gq * U[:, None], gq[:, :, None] * ref[:, None, :],
                        gu[:, :, None] * X[:, None, :], gu * U[:, None]]
            cots = [c.contiguous() for c in cots]
            grads = [torch.empty_like(t) for t in plant]
            condense_vjp_device(kp, nx, n, s_rows, [t.data_ptr() for t in plant], [c.data_ptr() for c in cots],
                                [t.data_ptr() for t in grads], stream, solver.device)
            grads = [t if need else None for t, need in zip(grads, ctx.needs_input_grad[3:10])]
        dX = dU = dref = None
        if ctx.ops is not None:
            ops = ctx.ops
            p = "k" if kp == 1 else "b"
            dX = torch.einsum(f"{p}ij,bi->bj", ops["Fx"], gq) + torch.einsum(f"{p}ij,bi->bj", ops["Sbar"], gu)
            dU = (ops["Fu"] * gq).sum(dim=1) + (ops["Ku"] * gu).sum(dim=1)
            dref = torch.einsum(f"{p}it,bi->bt", ops["Fr"], gq)
        return (None, None, None, *grads, dX, dU, dref)


def mpc_plant_solution(solver, Ad, Bd, Cd, K, Q, R, RD, X, U, ref, s_rows=10, setup=True):
    """One MPC step as a differentiable function of the plant model, the cost weights and the constraint row as
    well as of the step's data: device fp64 tensors Ad (k, nx, nx), Bd, Cd, K (k, nx), Q, R, RD (k,) with
    k = ``solver.n_plants`` (1: one plant shared by the batch, or batch: one per QP), X (batch, nx), U (batch),
    ref (batch, n); ``solver.n`` is the horizon N and ``solver.m == 2 N``.  Returns ``(x, status)`` as
    ``mpc_solution`` does; the caller's U is left alone.

    Forward: ``solver.mpc_setup_plants_device`` on the tensors' own memory (condensing and setup on the device, no
    host copy of the plant or the operators), then ``mpc_step_ref_device``.  With ``setup=False`` the caller
    vouches that the solver already holds these plants (a second step on the same model) and only the step runs.
    Backward: one ``sensitivity_data_device`` call (gq, gu, gP, gA), the operator cotangents gFx = gq X', gFu = gq U,
    gFr = gq ref', gSbar = gu X', gKu = gu U in torch, and one ``condense_vjp_device`` call.  A
    shared plant receives the sums over the batch.  A per-plant solver's backward pass materialises per-QP operator
    cotangents, O(batch N^2) doubles (gP, gA, gFr and their kin).  The gradient is that of the QP's optimum at the
    active set of the solve's final iterate: exact under strict complementarity, and zero for every QP that did not
    end SOLVED.  Gradients with respect to X, U and ref are ``mpc_solution``'s chain rule; they need the condensed
    operators, which are then fetched once per forward pass through the host (``solvempc_amd.condense``), only when
    one of the three requires a gradient.  ``backward`` must run before the solver solves again."""
    return _MpcPlantSolution.apply(solver, s_rows, setup, Ad, Bd, Cd, K, Q, R, RD, X, U, ref)


def mimo_solution(solver, X, U, yref, polish=False):
    """One MIMO MPC step ``solver.mimo_step_device`` (after ``mimo_setup_plants_device``) on device fp64 tensors
    X (batch, nx), U (batch, nu), yref (ny,), differentiable with respect to all three.  Returns ``(x, status)`` as
    ``mpc_solution`` does; the caller's U is left alone (the applied move is x[:, :nu]).  Backward is one
    ``BatchSolver.mimo_step_vjp_device`` call on the incoming cotangent (solvempc_amd/csrc/mpcq_mimo_sens.hip;
    DESIGN.md 4.15), the per-QP gradients of yref summed over the batch: the gradient of the QP's optimum at the
    active set of the step's final iterate, zero for a QP that did not end SOLVED.  With ``polish`` the forward pass
    is ``solver.mimo_step_polish_device``: x is the polished point where polish succeeds, and the
    unchanged backward pass then reads the polished iterate.  ``backward`` must run before the solver solves
    again."""
    return _MimoSolution.apply(solver, bool(polish), X, U, yref)


def mimo_ref_solution(solver, X, U, ref, polish=False):
    """``mimo_solution`` with an output reference over the horizon per QP (trajectory tracking with preview):
    ``solver.mimo_step_ref_device`` on device fp64 tensors X (batch, nx), U (batch, nu), ref (batch, N*ny; block i of
    the horizon, then y), differentiable with respect to all three.  Returns ``(x, status)``; the caller's U is left
    alone.  Backward is one ``BatchSolver.mimo_step_ref_vjp_device`` call on the incoming cotangent:
    every QP's own gradient of its reference, nothing summed over the batch, zero for a QP that did not end SOLVED.
    ``polish`` as in ``mimo_solution``.  ``backward`` must run before the solver solves again."""
    return _MimoRefSolution.apply(solver, bool(polish), X, U, ref)


def mimo_plant_solution(solver, Ad, Bd, Cd, Q, R, RD, K, K0, w0, X, U, yref, s_rows, polish=False, setup=True):
    """One MIMO MPC step as a differentiable function of the plant model (Ad, Bd, Cd), the weights (Q, R, RD) and
    the constraint data (K, K0, w0) as well as of the step's data: per-plant device fp64 tensors Ad (batch, nx, nx),
    Bd (batch, nx, nu), Cd (batch, ny, nx), Q (batch, ny, ny), R, RD (batch, nu, nu), K (batch, nu, nx), K0
    (batch, nu, nu), w0 (batch, nu), and X (batch, nx), U (batch, nu), yref (ny,).  Returns ``(x, status)`` as
    ``mimo_solution`` does; the caller's U is left alone.

    Forward: ``solver.mimo_setup_plants_device`` on the tensors' own memory (with ``setup=False`` the caller vouches
    that the solver already holds these plants, and only the step runs), then ``mimo_step_device``, or
    ``mimo_step_polish_device`` with ``polish``, on a private copy of U.  Backward: one
    ``BatchSolver.mimo_plant_vjp_device`` call for the nine plant gradients (no operator cotangent
    is materialised), and ``mimo_step_vjp_device`` for X, U and yref only where one of them requires a gradient.
    Q, R and RD are differentiated as general matrices: parametrise them symmetrically in torch and autograd
    symmetrises.  The gradient is that of the QP's optimum at the active set of the step's final iterate, zero for
    a QP that did not end SOLVED.  ``backward`` must run before the solver solves again."""
    return _MimoPlantSolution.apply(solver, s_rows, bool(polish), setup, Ad, Bd, Cd, Q, R, RD, K, K0, w0, X, U, yref)


def qp_solution(solver, P, A, q, l, u, setup=True):
    """The solutions of the batch of QPs  min 1/2 x'Px + q'x, l <= Ax <= u  as a differentiable function of all
    five tensors (device fp64): P (n, n) and A (m, n) for a shared-plant solver, (batch, n, n) and (batch, m, n)
    for a per-plant one; q (batch, n); l, u (batch, m).  Returns ``(x, status)`` as ``mpc_solution`` does.

    Forward: ``solver.setup(P, 0, A, l0, u0)`` with each plant's first QP's bounds, then ``update_lin_cost``,
    ``update_bounds`` and ``solve`` (host-side data updates).  With ``setup=False`` the caller vouches that the
    solver already holds P and A, and only q, l, u are updated.  ``setup="update"`` and ``setup="update_keep"`` hand
    P and A to a solver that is already set up through ``update_P_A_device`` on the tensors' own memory (no host
    copy of the matrices), equilibrated again or with the last setup's scaling kept (n <= 32, m <= 64): the QPs
    are warm-started from the previous solve's (x, y).  Backward is one
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

"""Cost of the MIMO step's plant gradients on config 4's plants (dev tool, needs the GPU): quad-rotor hover
linearisations, n_x 12, n_u 4, N = 30 (n = 120, m = 240), fp64, after the plants' first control step.

Method: one process; per round the setup (not timed: it resets the solver, so every round's step is the same cold
step), then each between two device events on the solver's stream, with the stream idle before the first event:
  mpcq_mimo_step_device                                          (the baseline: one solve with its factorisations)
  mpcq_mimo_sensitivity_device(g = NULL, n_rhs = 1; gq, gu, n_active)
  mpcq_mimo_plant_vjp_device(g = NULL; all nine gradients, n_active)
after `--warmup` such rounds, `--runs` of them.  The plant-gradient call is the sensitivity kernel (the same launch,
into the context's staging) followed by mimo_plant_vjp_kernel, so the new kernel alone is the difference of the two
calls; a kernel trace of this tool (rocprofv3 --kernel-trace --stats -- python tools/mimo_plant_vjp_cost.py ...)
gives it directly.  Reports the median and the range in ms, the plant-gradient call's ratio to the sensitivity
call, the difference of the medians, and one raw line per timed call.

usage: python tools/mimo_plant_vjp_cost.py [--batch 4096] [--horizon 30] [--runs 5] [--warmup 3] [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()

    import torch

    import solvempc_amd as sm
    from solvempc_amd import workload

    N, B, nu = a.horizon, a.batch, 4
    dev = torch.device("cuda:0")
    Ad, Bd = workload.quadrotor_plants(a.seed, 0, B)
    sh = workload.quadrotor_shared()
    X, U = workload.quadrotor_states(a.seed, 0, B)
    nx, ny = Ad.shape[1], np.asarray(sh["Cd"]).shape[0]
    tdev = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).to(dev)  # noqa: E731
    plant_d = [tdev(Ad), tdev(Bd)] + [
        torch.as_tensor(np.asarray(sh[k], dtype=np.float64)).to(dev).expand((B,) + np.asarray(sh[k]).shape).contiguous()
        for k in ("Cd", "Q", "R", "RD", "K", "K0", "w0")]
    s = sm.BatchSolver(N * nu, 2 * N * nu, B, B, "f64", 0, sm.default_settings())
    X_d, U0_d = tdev(X), tdev(U)
    U_d = U0_d.clone()
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream

    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)  # noqa: E731
    gq, gu = f64(B, N * nu), f64(B, 2 * N * nu)
    grads = [torch.zeros_like(t) for t in plant_d]
    na = torch.zeros(B, dtype=torch.int32, device=dev)
    plant_p, grad_p = [t.data_ptr() for t in plant_d], [t.data_ptr() for t in grads]
    calls = {
        "mimo_step": lambda: s.mimo_step_device(X_d.data_ptr(), U_d.data_ptr(), 0, sp),
        "sensitivity": lambda: s.mimo_sensitivity_device(0, 1, gq.data_ptr(), gu.data_ptr(), na.data_ptr(), sp),
        "plant_vjp": lambda: s.mimo_plant_vjp_device(0, plant_p, X_d.data_ptr(), U0_d.data_ptr(), 0, grad_p,
                                                     na.data_ptr(), sp),
    }

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms = {k: [] for k in calls}
    for i in range(a.warmup + a.runs):
        U_d.copy_(U0_d)
        s.mimo_setup_plants_device(nx, nu, ny, N, *plant_p, stream=sp)
        for k, fn in calls.items():  # (the step first: the other two read it)
            t = timed(fn)
            if i >= a.warmup:
                ms[k].append(t)
                print(f"raw run {i - a.warmup} {k} {t:.4f} ms")
    nact = na.cpu().numpy()
    st, it, _ = s.info()
    s.close()
    mean_na = float(nact[nact >= 0].mean()) if (nact >= 0).any() else float("nan")
    print(f"config-4 plants: {B} QPs, N = {N} (n = {N * nu}), {int((st == sm.SOLVED).sum())} solved, mean iterations "
          f"{it.mean():.1f}, mean n_active {mean_na:.2f}, max n_active {int(nact.max())}")
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rows = []
    for k, v in ms.items():
        v = np.asarray(v)
        rows.append(dict(call=k, batch=B, horizon=N, ms_median=med[k], ms_min=float(v.min()), ms_max=float(v.max()),
                         runs=int(v.size), ratio_to_sensitivity=med[k] / med["sensitivity"], n_active_mean=mean_na))
        print(f"{k:>12}: median {med[k]:.3f} ms, range {v.min():.3f} .. {v.max():.3f} ms over {v.size} runs, "
              f"{med[k] / med['sensitivity']:.3f} x the sensitivity call")
    alone = med["plant_vjp"] - med["sensitivity"]
    print(f"mimo_plant_vjp_kernel alone (difference of the medians): {alone:.3f} ms, "
          f"{alone / med['sensitivity']:.3f} x the sensitivity call")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

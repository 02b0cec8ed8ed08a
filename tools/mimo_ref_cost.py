"""Cost of the MIMO step's per-plant horizon reference on config 4's plants (dev tool, needs the GPU): quad-rotor
hover linearisations, n_x 12, n_u 4, N = 30 (n = 120, m = 240), fp64, the plants' first control step.

Method: one process; per round the setup (not timed: it resets the solver, so every round's step is the same cold
step) and U reset, then each between two device events on the solver's stream, with the stream idle before the first
event, alternating:
  mpcq_mimo_step_device(yref)                                    (the baseline step)
  mpcq_mimo_step_gains_device(dX, dU, dyref, n_active)           (the baseline gains, on that step)
then the setup and U reset again and
  mpcq_mimo_step_ref_device(1_N (x) yref, ref_stride = N n_y)    (the baseline's QPs bit for bit: the front end's cost alone)
the setup and U reset again and
  mpcq_mimo_step_ref_device(ref, ref_stride = N n_y)             (a reference per plant: 1_N (x) yref + noise)
  mpcq_mimo_step_ref_gains_device(dX, dU, dref, n_active)        (the gains with dref, on that step)
after `--warmup` such rounds, `--runs` of them.  Reports the median and the range in ms and the ratio of each
reference call to its baseline (by medians), and one raw line per timed call.

usage: python tools/mimo_ref_cost.py [--batch 4096] [--horizon 30] [--runs 5] [--warmup 2] [--json PATH]"""
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
    ap.add_argument("--warmup", type=int, default=2)
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
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    yref = 0.05 * torch.randn(ny, dtype=torch.float64, device=dev, generator=gen)
    ref = (yref.repeat(N)[None, :] + 0.01 * torch.randn(B, N * ny, dtype=torch.float64, device=dev, generator=gen))
    ref = ref.contiguous()
    uni = yref.repeat(N)[None, :].expand(B, N * ny).contiguous()
    new = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)  # noqa: E731
    dX, dU, dy, dr = new(B, nu, nx), new(B, nu, nu), new(B, nu, ny), new(B, nu, N * ny)
    na = torch.zeros(B, dtype=torch.int32, device=dev)
    calls = {
        "mimo_step": lambda: s.mimo_step_device(X_d.data_ptr(), U_d.data_ptr(), yref.data_ptr(), sp),
        "mimo_step_gains": lambda: s.mimo_step_gains_device(dX.data_ptr(), dU.data_ptr(), dy.data_ptr(), na.data_ptr(), sp),
        "mimo_step_ref_uniform": lambda: s.mimo_step_ref_device(X_d.data_ptr(), U_d.data_ptr(), uni.data_ptr(), N * ny, False,
                                                                sp),
        "mimo_step_ref": lambda: s.mimo_step_ref_device(X_d.data_ptr(), U_d.data_ptr(), ref.data_ptr(), N * ny, False, sp),
        "mimo_step_ref_gains": lambda: s.mimo_step_ref_gains_device(dX.data_ptr(), dU.data_ptr(), dr.data_ptr(),
                                                                    na.data_ptr(), sp),
    }

    def fresh():
        U_d.copy_(U0_d)
        s.mimo_setup_plants_device(nx, nu, ny, N, *[t.data_ptr() for t in plant_d], stream=sp)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms = {k: [] for k in calls}
    info = {}
    for i in range(a.warmup + a.runs):
        for k, fn in calls.items():  # (each step first: the gains read it)
            if not k.endswith("gains"):
                fresh()
            t = timed(fn)
            if i >= a.warmup:
                ms[k].append(t)
                print(f"raw run {i - a.warmup} {k} {t:.4f} ms")
            if not k.endswith("gains"):
                st, it, _ = s.info()
                info[k] = (int((st == sm.SOLVED).sum()), float(it.mean()))
    s.close()
    for k, (ns, mi) in info.items():
        print(f"{k}: {B} QPs, N = {N} (n = {N * nu}, n_y = {ny}), {ns} solved, mean iterations {mi:.1f}")
    rows = []
    for k, v in ms.items():
        v = np.asarray(v)
        base = float(np.median(ms[k.replace("_ref", "").replace("_uniform", "")]))
        rows.append(dict(call=k, batch=B, horizon=N, ms_median=float(np.median(v)), ms_min=float(v.min()),
                         ms_max=float(v.max()), runs=int(v.size), ratio_to_baseline=float(np.median(v)) / base))
        print(f"{k:>22}: median {np.median(v):.3f} ms, range {v.min():.3f} .. {v.max():.3f} ms over {v.size} runs, "
              f"{np.median(v) / base:.3f} x {k.replace('_ref', '').replace('_uniform', '')}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

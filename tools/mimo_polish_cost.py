"""Cost of the MIMO polish on config 4's plants (dev tool, needs the GPU): quad-rotor hover linearisations, n_x 12,
n_u 4, N = 30 (n = 120, m = 240), fp64, the plants' first control step.

Method: one process; per round the setup (not timed: it resets the solver, so every round's step is the same cold
step) and U reset, then each between two device events on the solver's stream, with the stream idle before the first
event:
  mpcq_mimo_step_device                                          (the baseline)
  mpcq_mimo_sensitivity_device(g = NULL, n_rhs = 1; gq, gu, n_active)   (the same factorisations, read-only)
then the setup and U reset again and
  mpcq_mimo_step_polish_device                                   (the copy of U, the same step, the polish kernel)
after `--warmup` such rounds, `--runs` of them.  Reports the median and the range in ms, each call's ratio to the
step, the polish's added cost (polished step - step, by medians), the polish outcome, and one raw line per timed call.

usage: python tools/mimo_polish_cost.py [--batch 4096] [--horizon 30] [--runs 5] [--warmup 3] [--json PATH]"""
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
    gq = torch.zeros(B, N * nu, dtype=torch.float64, device=dev)
    gu = torch.zeros(B, 2 * N * nu, dtype=torch.float64, device=dev)
    na = torch.zeros(B, dtype=torch.int32, device=dev)
    calls = {
        "mimo_step": lambda: s.mimo_step_device(X_d.data_ptr(), U_d.data_ptr(), 0, sp),
        "sensitivity": lambda: s.mimo_sensitivity_device(0, 1, gq.data_ptr(), gu.data_ptr(), na.data_ptr(), sp),
        "mimo_step_polish": lambda: s.mimo_step_polish_device(X_d.data_ptr(), U_d.data_ptr(), 0, sp),
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
    for i in range(a.warmup + a.runs):
        for k, fn in calls.items():  # (the step first: the sensitivity reads it)
            if k != "sensitivity":
                fresh()
            t = timed(fn)
            if i >= a.warmup:
                ms[k].append(t)
                print(f"raw run {i - a.warmup} {k} {t:.4f} ms")
    st, it, _ = s.info()
    pst, pna, _, _ = s.polish_info()
    s.close()
    print(f"config-4 plants: {B} QPs, N = {N} (n = {N * nu}), {int((st == sm.SOLVED).sum())} solved, mean iterations "
          f"{it.mean():.1f}; polish: {int((pst == 1).sum())} successful, {int((pst == -1).sum())} unsuccessful, "
          f"{int((pst == 0).sum())} not performed, mean n_active {pna[pst != 0].mean():.2f}, max {int(pna.max())}")
    base = float(np.median(ms["mimo_step"]))
    rows = []
    for k, v in ms.items():
        v = np.asarray(v)
        rows.append(dict(call=k, batch=B, horizon=N, ms_median=float(np.median(v)), ms_min=float(v.min()),
                         ms_max=float(v.max()), runs=int(v.size), ratio_to_step=float(np.median(v)) / base))
        print(f"{k:>16}: median {np.median(v):.3f} ms, range {v.min():.3f} .. {v.max():.3f} ms over {v.size} runs, "
              f"{np.median(v) / base:.2f} x the step")
    added = float(np.median(ms["mimo_step_polish"])) - base
    print(f"polish adds {added:.3f} ms to the step; the n_rhs = 1 sensitivity call takes "
          f"{float(np.median(ms['sensitivity'])):.3f} ms")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows + [dict(call="polish_added", batch=B, horizon=N, ms_median=added)], f, indent=1)


if __name__ == "__main__":
    main()

"""Cost of a closed-loop MIMO run on config 4's plants (dev tool, needs the GPU): quad-rotor hover linearisations,
n_x 12, n_u 4, N = 30 (n = 120, m = 240), fp64, `--steps` control steps from the plants' first, a reference schedule
per plant of `--sched-len` blocks (so the run reads the schedule in place first and the padded tail afterwards).

Method: one process; per round the setup (not timed: it resets the solver, so every round starts from the same cold
state) and X, U reset, then each of the following between two device events on the solver's stream, with the stream
idle before the first event, alternating:
  run    mpcq_mimo_run_ref_device(sched, steps)                      
  loop   what a caller could do before it: per step the hold-last window gathered by torch indexing,
         mpcq_mimo_step_ref_device(window), the plant updated by torch.baddbmm (+ torch.randn noise)
  plant  `steps` mpcq_mimo_simulate_device calls back to back           (mimo_plant_kernel alone)
after `--warmup` such rounds, `--runs` of them.  Reports the median and the range in ms, the loop's ratio to the run
and the plant kernel's share of a run step (by medians), and one raw line per timed call.

usage: python tools/mimo_run_cost.py [--batch 4096] [--steps 50] [--sched-len 40] [--runs 5] [--warmup 2] [--json PATH]"""
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--sched-len", type=int, default=40)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()

    import torch

    import solvempc_amd as sm
    from solvempc_amd import workload

    N, B, nu, K, L = a.horizon, a.batch, 4, a.steps, a.sched_len
    dev = torch.device("cuda:0")
    Ad, Bd = workload.quadrotor_plants(a.seed, 0, B)
    sh = workload.quadrotor_shared()
    X, U = workload.quadrotor_states(a.seed, 0, B)
    nx, ny = Ad.shape[1], np.asarray(sh["Cd"]).shape[0]
    tdev = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).to(dev)  # noqa: E731
    plant_d = [tdev(Ad), tdev(Bd)] + [
        torch.as_tensor(np.asarray(sh[k], dtype=np.float64)).to(dev).expand((B,) + np.asarray(sh[k]).shape).contiguous()
        for k in ("Cd", "Q", "R", "RD", "K", "K0", "w0")]
    Ad_d, Bd_d = plant_d[0], plant_d[1]
    s = sm.BatchSolver(N * nu, 2 * N * nu, B, B, "f64", 0, sm.default_settings())
    X0_d, U0_d = tdev(X), tdev(U)
    X_d, U_d = X0_d.clone(), U0_d.clone()
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    yref = 0.05 * torch.randn(ny, dtype=torch.float64, device=dev, generator=gen)
    sched = (yref[None, None, :] + 0.01 * torch.randn(B, L, ny, dtype=torch.float64, device=dev, generator=gen)).contiguous()
    tI, tU = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
    log = s.mimo_log(iters_total_ptr=tI.data_ptr(), unsolved_total_ptr=tU.data_ptr())

    def fresh():
        X_d.copy_(X0_d)
        U_d.copy_(U0_d)
        s.mimo_setup_plants_device(nx, nu, ny, N, *[t.data_ptr() for t in plant_d], stream=sp)
        s.mimo_set_plant_device(Ad_d.data_ptr(), Bd_d.data_ptr(), sp)

    def run():
        s.mimo_run_ref_device(X_d.data_ptr(), U_d.data_ptr(), sched.data_ptr(), L, L * ny, K, a.seed, 0, 0, a.noise, False,
                              log, sp)

    def loop():
        keep = []
        Xc = X_d
        for k in range(K):
            idx = torch.clamp(k + torch.arange(N, device=dev), max=L - 1)
            win = sched[:, idx, :].reshape(B, N * ny).contiguous()
            s.mimo_step_ref_device(Xc.data_ptr(), U_d.data_ptr(), win.data_ptr(), N * ny, False, sp)
            w = a.noise * torch.randn(B, nx, 1, dtype=torch.float64, device=dev, generator=gen)
            Xc = torch.baddbmm(torch.baddbmm(w, Bd_d, U_d[:, :, None]), Ad_d, Xc[:, :, None])[:, :, 0].contiguous()
            keep.append((win, Xc))  # (the step reads them asynchronously)
        return keep

    def plant():
        for k in range(K):
            s.mimo_simulate_device(X_d.data_ptr(), U_d.data_ptr(), a.seed, 0, k, a.noise, sp)

    calls = {"run": run, "loop": loop, "plant": plant}

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        held = fn()
        e1.record(stream)
        torch.cuda.synchronize()
        del held
        return e0.elapsed_time(e1)

    ms = {k: [] for k in calls}
    info = {}
    for i in range(a.warmup + a.runs):
        for k, fn in calls.items():
            fresh()
            t = timed(fn)
            if i >= a.warmup:
                ms[k].append(t)
                print(f"raw run {i - a.warmup} {k} {t:.4f} ms", flush=True)
            if k == "run":
                info[k] = (float(tI.sum().item()) / (B * K), int(tU.sum().item()))
            elif k == "loop":
                st, it, _ = s.info()
                info[k] = (float(it.mean()), int((st != sm.SOLVED).sum()))
    s.close()
    print(f"{B} plants, N = {N} (n = {N * nu}, n_y = {ny}), {K} steps, schedule of {L} blocks per plant")
    print(f"run: mean iterations per step {info['run'][0]:.1f}, unsolved steps {info['run'][1]}; "
          f"loop's last step: mean iterations {info['loop'][0]:.1f}, unsolved {info['loop'][1]}")
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rows = []
    for k, v in ms.items():
        v = np.asarray(v)
        rows.append(dict(call=k, batch=B, horizon=N, steps=K, sched_len=L, ms_median=med[k], ms_min=float(v.min()),
                         ms_max=float(v.max()), runs=int(v.size), ms_per_step=med[k] / K, ratio_to_run=med[k] / med["run"]))
        print(f"{k:>6}: median {med[k]:.3f} ms, range {v.min():.3f} .. {v.max():.3f} ms over {v.size} runs, "
              f"{med[k] / K:.4f} ms per step, {med[k] / med['run']:.4f} x run")
    print(f"plant kernel: {100 * med['plant'] / med['run']:.3f} % of a run step; host loop / run = {med['loop'] / med['run']:.4f}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

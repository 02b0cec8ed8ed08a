"""Cost of the backward pass of diff.mpc_plant_solution on config 3's shape (dev tool, needs the GPU): a per-plant
context, N = 20, nx = 4, randomised plants, after one forward pass of the layer (condensing + setup + one step).

Method (as tools/sens_data_cost.py): one process; after a warm-up, `--runs` alternating rounds of
  the layer's backward pass (torch.autograd.grad of x with a random cotangent: mpcq_sensitivity_data_device, the
      operator cotangents in torch, mpcq_condense_vjp_device),
  mpcq_sensitivity_data_device alone (g, outputs gq, gu, gP, gA: what the backward pass asks of it)   and
  mpcq_condense_vjp_device alone (the kernel's own time, on per-QP cotangents prepared beforehand),
each between two device events on torch's current stream, with the stream idle before the first event.  All three
read the same solve.  Reports the median and the range in ms of each, the ratio backward / sensitivity_data and the
kernel's share of the sensitivity call, and one raw line per timed call.

usage: python tools/condense_vjp_cost.py [--batch 65536] [--horizon 20] [--runs 5] [--warmup 3] [--dtype f64]
       [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

KEYS = ("Ad", "Bd", "Cd", "K", "Q", "R", "RD")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")

    import torch

    import solvempc_amd as sm
    from solvempc_amd import diff, workload

    plant = workload.reference_plant()
    N, B, nx, s_rows = a.horizon, a.batch, 4, 10
    Ad, Bd = workload.randomized_plants(plant, 2, 0, B)
    X, U = workload.mpc_states(2, 0, B)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    cuda = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
    tile = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (B,) + np.shape(v)).copy()
    pl = [cuda(v).requires_grad_(True) for v in (Ad, Bd, tile(plant["Cd"]), tile(plant["K"]), tile(plant["Q"]),
                                                 tile(plant["R"]), tile(plant["RD"]))]
    Xd, Ud, ref = cuda(X), cuda(U), cuda(np.full((B, N), plant["xref"]))
    G = cuda(rng.normal(size=(B, N)))
    stream = torch.cuda.current_stream(dev)

    s = sm.BatchSolver(N, 2 * N, B, n_plants=B, dtype=a.dtype)
    x, status = diff.mpc_plant_solution(s, *pl, Xd, Ud, ref, s_rows=s_rows)
    path = s.path()[0]

    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
    gq, gu, gP, gA = f64(B, N), f64(B, 2 * N), f64(B, N, N), f64(B, 2 * N, N)
    na = torch.zeros(B, dtype=torch.int32, device=dev)
    sens = lambda: s.sensitivity_data_device(G.data_ptr(), gq.data_ptr(), 0, gu.data_ptr(), gP.data_ptr(), gA.data_ptr(),
                                             0, na.data_ptr(), stream.cuda_stream)
    sens()
    cots = [gP, gA, gq[:, :, None] * Xd[:, None, :], gq * Ud[:, None], gq[:, :, None] * ref[:, None, :],
            gu[:, :, None] * Xd[:, None, :], gu * Ud[:, None]]
    cots = [c.contiguous() for c in cots]
    outs = [torch.zeros_like(t) for t in pl]
    plant_ptrs = [t.data_ptr() for t in pl]
    calls = {
        "backward": lambda: torch.autograd.grad((x,), pl, grad_outputs=(G,), retain_graph=True),
        "sensitivity_data": sens,
        "condense_vjp": lambda: sm.condense_vjp_device(B, nx, N, s_rows, plant_ptrs, [c.data_ptr() for c in cots],
                                                       [t.data_ptr() for t in outs], stream.cuda_stream),
    }

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        for fn in calls.values():
            timed(fn)
    ms = {k: [] for k in calls}
    for i in range(a.runs):
        for k, fn in calls.items():  # alternated: drift of the device's clocks spreads over all alike
            ms[k].append(timed(fn))
            print(f"raw run {i} {k} {ms[k][-1]:.4f} ms")
    grads = calls["backward"]()
    torch.cuda.synchronize()
    same = all(torch.equal(g_, o) for g_, o in zip(grads, outs))
    nact = na.cpu().numpy()
    st = status.cpu().numpy()
    s.close()
    print(f"config-3 shape: {B} plants, N = {N}, nx = {nx}, dtype {a.dtype}, path {path}, "
          f"{int((st == sm.SOLVED).sum())} solved, mean n_active {nact[nact >= 0].mean():.2f}, "
          f"|gAd| {float(grads[0].abs().max()):.3e}; backward's gradients equal the lone kernel call's: {same}")
    rows = []
    for k, v in ms.items():
        v = np.asarray(v)
        rows.append(dict(call=k, dtype=a.dtype, batch=B, horizon=N, ms_median=float(np.median(v)), ms_min=float(v.min()),
                         ms_max=float(v.max()), runs=int(v.size)))
        print(f"{k:>17}: median {np.median(v):.3f} ms, range {v.min():.3f} .. {v.max():.3f} ms over {v.size} runs")
    med = {k: float(np.median(v)) for k, v in ms.items()}
    ratios = np.asarray(ms["backward"]) / np.asarray(ms["sensitivity_data"])
    shares = np.asarray(ms["condense_vjp"]) / np.asarray(ms["sensitivity_data"])
    rows.append(dict(call="ratio", backward_over_sensitivity_data=med["backward"] / med["sensitivity_data"],
                     ratio_min=float(ratios.min()), ratio_max=float(ratios.max()),
                     kernel_over_sensitivity_data=med["condense_vjp"] / med["sensitivity_data"],
                     share_min=float(shares.min()), share_max=float(shares.max())))
    print(f"backward / sensitivity_data: x{med['backward'] / med['sensitivity_data']:.3f} (medians), per-round "
          f"x{ratios.min():.3f} .. x{ratios.max():.3f}")
    print(f"condense_vjp kernel / sensitivity_data: {med['condense_vjp'] / med['sensitivity_data']:.3f} (medians), "
          f"per-round {shares.min():.3f} .. {shares.max():.3f}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

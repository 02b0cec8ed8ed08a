"""Cost of the gradients with respect to P and A on the config-2 shape (dev tool, needs the GPU): 65,536 QPs, N = 20,
shared plant, after one mpc_step_device of a mixed (default), f64 or f32 context.

Method (as tools/sens_cost.py): one process; after a warm-up, `--runs` alternating rounds of
  mpcq_sensitivity_device(g = NULL, outputs gq, gl, gu, n_active)   and
  mpcq_sensitivity_data_device(g = NULL, the same outputs plus gP, gA; the masks from the context's staging),
each between two device events on the solver's stream, with the stream idle before the first event.  Both read the
same solve, so every round measures the same work; the second adds the mask stores, the contraction
(sens_contract_kernel) and the reduction of its partial sums.  Reports the median and the range in ms
of each, the ratio of the medians and the range of the per-round ratios, and one raw line per timed call.

usage: python tools/sens_data_cost.py [--batch 65536] [--horizon 20] [--runs 5] [--warmup 3] [--dtype mixed]
       [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

LMIN = -np.finfo(np.float64).max


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="mixed")
    ap.add_argument("--json", default="")
    a = ap.parse_args()

    import torch

    import oracle
    import solvempc_amd as sm
    from solvempc_amd import workload

    plant = workload.reference_plant()
    N, B = a.horizon, a.batch
    ops = oracle.condense(plant, N)
    X, U = workload.mpc_states(1, 0, B)
    dev = torch.device("cuda:0")
    X_d, U_d = torch.from_numpy(X).to(dev), torch.from_numpy(U).to(dev)
    stream = torch.cuda.current_stream(dev)

    s = sm.BatchSolver(N, 2 * N, B, dtype=a.dtype)
    s.setup(ops["P"], np.zeros(N), ops["A"], np.full(2 * N, LMIN), oracle.upper_bound(ops, np.zeros(4), 0.0))
    s.mpc_set_operators(ops["Fx"], ops["Fu"], ops["Fr"], ops["Sbar"], ops["Ku"], ops["W0"])
    s.mpc_step_device(X_d.data_ptr(), U_d.data_ptr(), plant["xref"], stream.cuda_stream)
    path = s.path()[0]

    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=dev)
    gq, gl, gu, gP, gA = f64(B, N), f64(B, 2 * N), f64(B, 2 * N), f64(N, N), f64(2 * N, N)
    na = torch.zeros(B, dtype=torch.int32, device=dev)
    calls = {
        "sensitivity": lambda: s.sensitivity_device(0, gq.data_ptr(), gl.data_ptr(), gu.data_ptr(), na.data_ptr(),
                                                    stream.cuda_stream),
        "sensitivity_data": lambda: s.sensitivity_data_device(0, gq.data_ptr(), gl.data_ptr(), gu.data_ptr(),
                                                              gP.data_ptr(), gA.data_ptr(), 0, na.data_ptr(),
                                                              stream.cuda_stream),
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
        for k, fn in calls.items():  # alternated: drift of the device's clocks spreads over both alike
            ms[k].append(timed(fn))
            print(f"raw run {i} {k} {ms[k][-1]:.4f} ms")
    nact = na.cpu().numpy()
    st = s.info()[0]
    s.close()
    print(f"config-2 shape: {B} QPs, N = {N}, dtype {a.dtype}, path {path}, {int((st == sm.SOLVED).sum())} solved, "
          f"mean n_active {nact[nact >= 0].mean():.2f}, |gP| {float(gP.abs().max()):.3e}, |gA| {float(gA.abs().max()):.3e}")
    rows = []
    for k, v in ms.items():
        v = np.asarray(v)
        rows.append(dict(call=k, dtype=a.dtype, batch=B, horizon=N, ms_median=float(np.median(v)), ms_min=float(v.min()),
                         ms_max=float(v.max()), runs=int(v.size)))
        print(f"{k:>17}: median {np.median(v):.3f} ms, range {v.min():.3f} .. {v.max():.3f} ms over {v.size} runs")
    ratios = np.asarray(ms["sensitivity_data"]) / np.asarray(ms["sensitivity"])
    ratio = float(np.median(ms["sensitivity_data"]) / np.median(ms["sensitivity"]))
    rows.append(dict(call="ratio", ratio_of_medians=ratio, ratio_min=float(ratios.min()), ratio_max=float(ratios.max())))
    print(f"sensitivity_data / sensitivity: x{ratio:.3f} (medians), per-round x{ratios.min():.3f} .. x{ratios.max():.3f}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

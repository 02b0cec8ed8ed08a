"""Cost and accuracy of settings.polish on the config-2 shape (dev tool, needs the GPU): 65,536 QPs, N = 20,
through mpc_step_device with polish on and off, for f64, mixed and f32 contexts.

Method: one process, the six variants alternated step by step after
a warm-up, >= 20 timed steps each, device events around the step alone (every step the reference's first
control step: U and the solver state reset outside the timed span).  Reports the median ms per step, the
difference polish makes, the mean n_active, and the accuracy of the applied move: max |x0 - x0*| on a prefix
of the batch against the QP's optimum (the oracle at 1e-10, its active set, the exact KKT system; restated
from tests/test_polish.py), unpolished next to polished.

The polish kernel's own time comes from a separate run under
    rocprofv3 --kernel-trace --stats -- python tools/polish_cost.py --steps 5 --dtypes f32
(polish_kernel's row of the stats); with workload.flops_polish that gives its share of the fp64 VALU peak.

usage: python tools/polish_cost.py [--batch 65536] [--steps 20] [--warmup 3] [--prefix 4096] [--dtypes f64,mixed,f32]
       [--json PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

LMIN = -np.finfo(np.float64).max


def optimum(oracle, P, A, q, l, u, solver):
    """x* of one QP: active set from the duals of a 1e-10 oracle solve, then the exact KKT system."""
    solver.update_gradient(q)
    solver.update_upper_bound(u)
    solver.cold_start()
    if solver.solve() != oracle.SOLVED:
        return np.full(len(q), np.nan)
    y = solver.y()
    thr = 1e-9 * max(1.0, float(np.abs(y).max(initial=0.0)))
    up, lo = y > thr, y < -thr
    act = up | lo
    Aa, ba = A[act], np.where(up, u, l)[act]
    k = Aa.shape[0]
    Pf = np.triu(P) + np.triu(P, 1).T
    K = np.block([[Pf, Aa.T], [Aa, np.zeros((k, k))]])
    return np.linalg.lstsq(K, np.r_[-q, ba], rcond=None)[0][:len(q)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prefix", type=int, default=4096)
    ap.add_argument("--dtypes", default="f64,mixed,f32")
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
    l = np.full(2 * N, LMIN)
    u0 = oracle.upper_bound(ops, np.zeros(4), 0.0)
    dev = torch.device("cuda:0")
    X_d, U0_d = torch.from_numpy(X).to(dev), torch.from_numpy(U).to(dev)
    U_d = U0_d.clone()
    stream = torch.cuda.current_stream(dev)

    variants = []
    for dt in a.dtypes.split(","):
        for pol in (0, 1):
            s = sm.BatchSolver(N, 2 * N, B, dtype=dt, settings=sm.default_settings(polish=pol))
            s.setup(ops["P"], np.zeros(N), ops["A"], l, u0)
            s.mpc_set_operators(ops["Fx"], ops["Fu"], ops["Fr"], ops["Sbar"], ops["Ku"], ops["W0"])
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
            variants.append(dict(dtype=dt, polish=pol, solver=s, ev=ev))

    def step(v, i=None):
        U_d.copy_(U0_d)
        v["solver"].reset_state()
        if i is not None:
            v["ev"][i][0].record(stream)
        v["solver"].mpc_step_device(X_d.data_ptr(), U_d.data_ptr(), plant["xref"], stream.cuda_stream)
        if i is not None:
            v["ev"][i][1].record(stream)

    for _ in range(a.warmup):
        for v in variants:
            step(v)
    for i in range(a.steps):
        for v in variants:  # alternated: drift of the device's clocks spreads over every variant alike
            step(v, i)
    torch.cuda.synchronize()

    # accuracy of the applied move on a prefix (every variant's last step is the same first control step)
    K = min(a.prefix, B)
    q = oracle.gradient(ops, X[:K], U[:K], plant["xref"])
    u = oracle.upper_bound(ops, X[:K], U[:K])
    tight = oracle.Solver(ops["P"], np.zeros(N), ops["A"], l, u0,
                          oracle.default_settings(eps_abs=1e-10, eps_rel=1e-10, max_iter=200000))
    x_opt = np.stack([optimum(oracle, ops["P"], ops["A"], q[b], l, u[b], tight) for b in range(K)])

    rows = []
    for v in variants:
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in v["ev"]])
        st = v["solver"].info()[0]
        x = v["solver"].solution()[:K]
        sp, na, _, _ = v["solver"].polish_info()
        good = (st[:K] == sm.SOLVED) & ~np.isnan(x_opt[:, 0])
        rows.append(dict(dtype=v["dtype"], polish=v["polish"], ms_median=float(np.median(ms)), ms_min=float(ms.min()),
                         ms_max=float(ms.max()), solved=int((st == sm.SOLVED).sum()),
                         polished=int((sp == 1).sum()), rejected=int((sp == -1).sum()),
                         n_active_mean=float(na[sp != 0].mean()) if (sp != 0).any() else 0.0,
                         dx0_max=float(np.abs(x[good, 0] - x_opt[good, 0]).max()),
                         dx_max=float(np.abs(x[good] - x_opt[good]).max()), prefix=int(good.sum())))
        v["solver"].close()
    by = {(r["dtype"], r["polish"]): r for r in rows}
    print(f"config-2 shape: {B} QPs, N = {N}, {a.steps} timed steps per variant (median ms per step)")
    print(f"{'dtype':>6} {'off':>8} {'on':>8} {'polish':>8} {'n_active':>8} {'polished':>9} {'rejected':>8} "
          f"{'max|dx0| off':>13} {'max|dx0| on':>12}")
    for dt in a.dtypes.split(","):
        o, p = by[(dt, 0)], by[(dt, 1)]
        print(f"{dt:>6} {o['ms_median']:8.3f} {p['ms_median']:8.3f} {p['ms_median'] - o['ms_median']:8.3f} "
              f"{p['n_active_mean']:8.2f} {p['polished']:9d} {p['rejected']:8d} {o['dx0_max']:13.3e} {p['dx0_max']:12.3e}")
    na = by[(a.dtypes.split(",")[0], 1)]["n_active_mean"]
    print(f"flops_polish(n = {N}, n_active = {round(na)}, refine = 3) = {workload.flops_polish(N, round(na), 3)} per QP")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

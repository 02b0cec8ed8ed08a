"""Cost of new matrices for a context that is set up (dev tool, needs the GPU): mpcq_update_P_A_device with
rescale = 1 and rescale = 0 against the route that existed before it, host mpcq_setup + mpcq_update_lin_cost +
mpcq_update_bounds + mpcq_warm_start, on two shapes:
  cfg2: 65,536 QPs sharing one plant, N = 20, mixed (config 2's shape)
  cfg3: 65,536 distinct plants, N = 20, f64 (config 3's shape)

Method: one process per shape; the context is set up on the plant's matrices, given its per-QP data and solved
once.  Then, after a warm-up, `--runs` alternating rounds of the three routes, each handed the other one of the two
matrix sets (the plant's, and the retuned plant's: Q x 1.5, R x 0.6, Ad x 1.002, K x 1.1), so every call does the
work of a real change.  Each call is timed on the host clock between two device synchronisations (the host route
and the flag word of the device route both wait for the device, so wall time is the cost a caller sees).  Reports
median and range in ms and one raw line per call, and the mean iterations of the solve that follows an update
(warm) against a from-scratch setup on the new matrices (cold).

usage: python tools/update_cost.py [--shape cfg2|cfg3] [--batch 65536] [--horizon 20] [--runs 5] [--warmup 2] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

LMIN = -np.finfo(np.float64).max


def retuned(pl):
    out = dict(pl)
    out["Q"], out["R"] = pl["Q"] * 1.5, pl["R"] * 0.6
    out["Ad"], out["K"] = np.asarray(pl["Ad"]) * 1.002, np.asarray(pl["K"]) * 1.1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="cfg2", choices=["cfg2", "cfg3"])
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default="")
    a = ap.parse_args()

    import torch

    import solvempc_amd as sm
    from solvempc_amd import workload

    plant = workload.reference_plant()
    N, B = a.horizon, a.batch
    per_plant = a.shape == "cfg3"
    k = B if per_plant else 1
    dtype = "f64" if per_plant else "mixed"
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)

    rep = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (k,) + np.shape(v)).copy()
    base = {key: rep(plant[key]) for key in ("Ad", "Bd", "Cd", "K", "Q", "R", "RD")}
    if per_plant:  # config 3's perturbed plants
        base["Ad"], base["Bd"] = workload.randomized_plants(plant, 11, 0, B)
    mats = [sm.condense(pl, N) for pl in (base, retuned(base))]
    old = mats[0]
    X, U = workload.mpc_states(1, 0, B, 1.0)
    if per_plant:
        q = np.einsum("bij,bj->bi", old["Fx"], X) + old["Fu"] * U[:, None]
        u = old["W0"] + np.einsum("bij,bj->bi", old["Sbar"], X) + old["Ku"] * U[:, None]
    else:
        q = X @ old["Fx"][0].T + U[:, None] * old["Fu"][0]
        u = old["W0"][0] + X @ old["Sbar"][0].T + U[:, None] * old["Ku"][0]
    l = np.full((B, 2 * N), LMIN)
    q0, l0, u0 = np.zeros((k, N)), np.full((k, 2 * N), LMIN), old["W0"].copy()
    dmats = [(torch.from_numpy(m["P"]).to(dev), torch.from_numpy(m["A"]).to(dev)) for m in mats]

    def fresh(m):
        s = sm.BatchSolver(N, 2 * N, B, n_plants=k, dtype=dtype)
        s.setup(m["P"], q0, m["A"], l0, u0)
        s.update_lin_cost(q)
        s.update_bounds(l, u)
        return s

    s = fresh(old)
    s.solve()
    x1, y1 = s.solution(), s.dual()
    cold_first = s.info()[1].mean()

    def host_route(i):
        m = mats[i]
        s.setup(m["P"], q0, m["A"], l0, u0)
        s.update_lin_cost(q)
        s.update_bounds(l, u)
        s.warm_start(x1, y1)

    def device_route(rescale):
        return lambda i: s.update_P_A_device(dmats[i][0].data_ptr(), dmats[i][1].data_ptr(), rescale, stream.cuda_stream)

    routes = {"host setup + data + warm start": host_route, "update_P_A_device rescale=1": device_route(1),
              "update_P_A_device rescale=0": device_route(0)}

    def timed(fn, i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(i)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    turn = 0
    for _ in range(a.warmup):
        for fn in routes.values():
            turn ^= 1
            timed(fn, turn)
    ms = {name: [] for name in routes}
    for r in range(a.runs):
        for name, fn in routes.items():  # alternated: drift of the device's clocks spreads over all three alike
            turn ^= 1
            ms[name].append(timed(fn, turn))
            print(f"raw run {r} {name} {ms[name][-1]:.4f} ms")
    s.close()

    # iterations of the solve that follows: warm (after an update of a solved context) against cold (from scratch)
    iters = {}
    for name, rescale in (("warm, rescale=1", 1), ("warm, rescale=0", 0)):
        w = fresh(old)
        w.solve()
        w.update_P_A_device(dmats[1][0].data_ptr(), dmats[1][1].data_ptr(), rescale, stream.cuda_stream)
        w.solve()
        st, it, _ = w.info()
        iters[name] = (float(it.mean()), int((st == sm.SOLVED).sum()))
        w.close()
    c = fresh(mats[1])
    c.solve()
    st, it, _ = c.info()
    iters["cold"] = (float(it.mean()), int((st == sm.SOLVED).sum()))
    c.close()

    print(f"{a.shape}: {B} QPs, {k} plant(s), N = {N}, dtype {dtype}; first solve {cold_first:.1f} iterations (mean)")
    rows = []
    for name, v in ms.items():
        v = np.asarray(v)
        rows.append(dict(shape=a.shape, route=name, batch=B, horizon=N, dtype=dtype, ms_median=float(np.median(v)),
                         ms_min=float(v.min()), ms_max=float(v.max()), runs=int(v.size)))
        print(f"{name:>32}: median {np.median(v):.3f} ms, range {v.min():.3f} .. {v.max():.3f} ms over {v.size} runs")
    for name, (mean_it, solved) in iters.items():
        rows.append(dict(shape=a.shape, following_solve=name, mean_iterations=mean_it, solved=solved))
        print(f"following solve, {name:>16}: {mean_it:.1f} iterations (mean), {solved} of {B} SOLVED")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

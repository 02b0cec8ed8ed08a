"""Cost of the per-step stream record (mpcq_mpc_set_stream_log) on config 5's shape (dev tool, needs a gfx950 device):
4,096 plants x 1,000 warm-started control steps, N = 20, the tile stream, as `bench.py --workload stream` runs
it (workload.stream_states, the plant's xref, noise 1e-2, the state reset before every run).  One process times
the variants of one tree in turn, every run one JSON line:

    unlogged   no record attached
    log4       U, X, status and iter recorded (48 B per plant-step)
    logU       U only (8 B per plant-step)

--root picks the tree whose solvempc_amd (and libmpcq.so) is imported, so the same script times a checkout of
the parent commit (which has no record: only `unlogged` runs there).  Alternate the trees from a shell loop:

    for i in 1 2 3 4 5; do
      python tools/stream_log_ab.py --root ../parent --tag parent --rep $i
      python tools/stream_log_ab.py --tag branch --rep $i
    done
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--tag", default="branch")
    ap.add_argument("--rep", type=int, default=0)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--plants", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--inner", type=int, default=2, help="timed runs of every variant per process (round-robin)")
    a = ap.parse_args()
    here = str(Path(__file__).resolve().parents[1])
    sys.path[:0] = [a.root, here] if a.root != here else [here]
    import torch

    import oracle
    import solvempc_amd as sm
    from solvempc_amd import workload

    N, B, K = a.horizon, a.plants, a.steps
    plant = workload.reference_plant()
    ops = oracle.condense(plant, N)
    X, U = workload.stream_states(1, 0, B)
    can_log = hasattr(sm.BatchSolver, "mpc_set_stream_log")
    variants = ["unlogged"] + (["log4", "logU"] if can_log else [])
    dev = torch.device("cuda", 0)
    for dtype in a.dtypes.split(","):
        s = sm.BatchSolver(N, 2 * N, B, dtype=dtype)
        s.setup(ops["P"], np.zeros(N), ops["A"], np.full(2 * N, -np.finfo(np.float64).max), ops["W0"].copy())
        s.mpc_set_operators(ops["Fx"], ops["Fu"], ops["Fr"], ops["Sbar"], ops["Ku"], ops["W0"])
        s.mpc_set_plant(plant["Ad"], plant["Bd"])
        X0, U0 = torch.from_numpy(X).to(dev), torch.from_numpy(U).to(dev)
        Xd, Ud = X0.clone(), U0.clone()
        st = torch.cuda.Stream(device=dev)
        if can_log:
            lU = torch.zeros(K, B, dtype=torch.float64, device=dev)
            lX = torch.zeros(K, B, 4, dtype=torch.float64, device=dev)
            lS = torch.zeros(K, B, dtype=torch.int32, device=dev)
            lI = torch.zeros(K, B, dtype=torch.int32, device=dev)

        def run(variant):
            Xd.copy_(X0)
            Ud.copy_(U0)
            s.reset_state()
            if variant == "log4":
                s.mpc_set_stream_log(lU.data_ptr(), lX.data_ptr(), lS.data_ptr(), lI.data_ptr(), K, 0)
            elif variant == "logU":
                s.mpc_set_stream_log(lU.data_ptr(), 0, 0, 0, K, 0)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            s.mpc_run_device(Xd.data_ptr(), Ud.data_ptr(), plant["xref"], K, 1, 0, 0, 1e-2, st.cuda_stream)
            st.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if variant != "unlogged":
                s.mpc_set_stream_log()
            return ms

        for v in variants:  # warm-up: code objects loaded, buffers touched
            run(v)
        for i in range(a.inner):
            for v in variants:
                ms = run(v)
                it, uns = s.stream_counters()
                print(json.dumps({"tag": a.tag, "rep": a.rep, "inner": i, "dtype": dtype, "variant": v,
                                  "path": s.stream_path(), "plants": B, "steps": K, "ms": round(ms, 4),
                                  "mqps": round(B * K / ms / 1e3, 2), "iters": int(it.sum()), "unsolved": int(uns.sum()),
                                  "U_sum": float(Ud.sum().item())}), flush=True)
        s.close()


if __name__ == "__main__":
    main()

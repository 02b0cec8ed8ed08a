"""CPU side of the mpcq_update_P_A tests (no device needed): the inputs tests/test_update_P_A.py runs on the GPU,
the two oracle references it compares against, and the check that every QP of those inputs ends SOLVED in the
oracle on all three routes -- the first solve on the old matrices, the re-equilibrated update (rescale = 1) and the
kept-scaling update (rescale = 0) -- so that the GPU tests compare SOLVED trajectories and nothing else.

Inputs: the golden plant at N = 20 (paired, tile remainder rows 16-19) and N = 15 (unpaired), 256 QPs from
workload.mpc_states(1, 0, B, 1.0); 64 distinct plants from workload.randomized_plants at N = 20.  The old matrices
are condensed from the plant, the new ones from Q x 1.5, R x 0.6, Ad x 1.002, K x 1.1.  Every QP keeps the q, u
that the OLD operators gave it (an update leaves the per-QP data alone).

The references (oracle/ has no update call; both build a fresh workspace on the new matrices):
* rescale = 1: Solver(P_new, q0, A_new, l0, u0), update_gradient(q_b), update_upper_bound(u_b),
  warm_start(x_b, y_b), solve;
* kept scaling: the same on the pre-scaled problem c D P_new D (symmetrised from the upper triangle), c D q,
  E A_new D, E l and E u clipped to +-DBL_MAX, with scaling = 0 and scaled_termination = 1, warm-started at
  (x / D, c y / E); its solution x' is the scaled one, x = D x'.
"""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle
from solvempc_amd import _capi, workload

ROOT = Path(__file__).resolve().parents[1]
LMIN = -np.finfo(np.float64).max
DMAX = np.finfo(np.float64).max
B_SHARED, B_PLANTS = 256, 64


def new_plant(pl):
    """The retuned plant of every update test: Q x 1.5, R x 0.6, Ad x 1.002, K x 1.1."""
    out = dict(pl)
    out["Q"], out["R"] = pl["Q"] * 1.5, pl["R"] * 0.6
    out["Ad"], out["K"] = np.asarray(pl["Ad"]) * 1.002, np.asarray(pl["K"]) * 1.1
    return out


def shared_case(plant, N, B=B_SHARED):
    """One plant, B QPs: old / new operators, the setup data and the per-QP q, l, u (from the old operators)."""
    old, new = oracle.condense(plant, N), oracle.condense(new_plant(plant), N)
    X, U = workload.mpc_states(1, 0, B, 1.0)
    return {"N": N, "old": old, "new": new, "X": X, "U": U, "q0": np.zeros(N), "l0": np.full(2 * N, LMIN),
            "u0": oracle.upper_bound(old, np.zeros(4), 0.0), "q": oracle.gradient(old, X, U),
            "l": np.full((B, 2 * N), LMIN), "u": oracle.upper_bound(old, X, U)}


def plants_case(plant, N=20, B=B_PLANTS):
    """B distinct plants (config 3's perturbations of the golden plant), one QP each."""
    Ad, Bd = workload.randomized_plants(plant, 7, 0, B)
    X, U = workload.mpc_states(1, 0, B, 1.0)
    olds, news = [], []
    for b in range(B):
        pl = dict(plant)
        pl["Ad"], pl["Bd"] = Ad[b], Bd[b]
        olds.append(oracle.condense(pl, N))
        news.append(oracle.condense(new_plant(pl), N))
    stack = lambda ops, k: np.stack([o[k] for o in ops])
    return {"N": N, "olds": olds, "news": news, "P_old": stack(olds, "P"), "A_old": stack(olds, "A"),
            "P_new": stack(news, "P"), "A_new": stack(news, "A"), "q0": np.zeros((B, N)),
            "l0": np.full((B, 2 * N), LMIN), "u0": np.stack([oracle.upper_bound(o, np.zeros(4), 0.0) for o in olds]),
            "q": np.stack([oracle.gradient(o, X[b], U[b]) for b, o in enumerate(olds)]),
            "l": np.full((B, 2 * N), LMIN),
            "u": np.stack([oracle.upper_bound(o, X[b], U[b]) for b, o in enumerate(olds)])}


def _collect(s):
    i = s.info()
    return s.x(), s.y(), i.status, i.iter, i.rho, i.margin


def first_solve(P, A, q0, l0, u0, q, u, settings=None):
    """The solve before the update (fresh workspace, cold): (x, y, status, iter, rho, margin) of one QP."""
    s = oracle.Solver(P, q0, A, l0, u0, settings=settings)
    assert s.update_gradient(q) and s.update_upper_bound(u)
    s.solve()
    return _collect(s)


def ref_rescale(P_new, A_new, q0, l0, u0, q, u, x, y, settings=None):
    """rescale = 1: a fresh workspace on the new matrices, the QP's own q, u, warm-started at (x, y)."""
    s = oracle.Solver(P_new, q0, A_new, l0, u0, settings=settings)
    assert s.update_gradient(q) and s.update_upper_bound(u)
    s.warm_start(x, y)
    s.solve()
    return _collect(s)


def sym_upper(P):
    return np.triu(P) + np.triu(P, 1).T


def ref_keep(P_new, A_new, D, E, c, l0, u0, q, l, u, x, y, **over):
    """Kept scaling: the pre-scaled problem with scaling = 0, scaled_termination = 1 (module docstring).  Returns
    the collect tuple with the SCALED solution and dual (x', y'): x = D x', y = E y' / c."""
    st = oracle.default_settings(scaling=0, scaled_termination=1, **over)
    # (the rounding order include/mpcq.h states for rescale = 0, so that both sides iterate on the same bits)
    Ps = (D[:, None] * (c * sym_upper(P_new))) * D[None, :]
    As = (E[:, None] * A_new) * D[None, :]
    clip = lambda v: np.clip(E * v, -DMAX, DMAX)
    s = oracle.Solver(Ps, np.zeros(len(D)), As, clip(l0), clip(u0), settings=st)
    assert s.update_gradient(c * D * q) and s.update_bounds(clip(l), clip(u))
    s.warm_start(x / D, c * y / E)
    s.solve()
    return _collect(s)


def _routes(P_old, A_old, P_new, A_new, q0, l0, u0, q, l, u):
    """(status of the first solve, of the rescale = 1 route, of the kept-scaling route, their iterations)."""
    D, E, c = oracle.Solver(P_old, q0, A_old, l0, u0).scaling()
    x, y, st0, it0, _, _ = first_solve(P_old, A_old, q0, l0, u0, q, u)
    _, _, st1, it1, _, _ = ref_rescale(P_new, A_new, q0, l0, u0, q, u, x, y)
    _, _, st2, it2, _, _ = ref_keep(P_new, A_new, D, E, c, l0, u0, q, l, u, x, y)
    return (st0, st1, st2), (it0, it1, it2)


@pytest.mark.parametrize("N", [20, 15])
def test_shared_inputs_end_solved_on_every_route(plant, N):
    cs = shared_case(plant, N)
    sts, its = zip(*[_routes(cs["old"]["P"], cs["old"]["A"], cs["new"]["P"], cs["new"]["A"], cs["q0"], cs["l0"],
                             cs["u0"], cs["q"][b], cs["l"][b], cs["u"][b]) for b in range(B_SHARED)])
    sts, its = np.array(sts), np.array(its)
    print(f"N={N}: mean iterations first {its[:, 0].mean():.1f}, rescale=1 {its[:, 1].mean():.1f}, "
          f"kept scaling {its[:, 2].mean():.1f}")
    assert np.all(sts == oracle.SOLVED), np.argwhere(sts != oracle.SOLVED)[:8]


def test_per_plant_inputs_end_solved_on_every_route(plant):
    cs = plants_case(plant)
    sts = np.array([_routes(cs["P_old"][b], cs["A_old"][b], cs["P_new"][b], cs["A_new"][b], cs["q0"][b], cs["l0"][b],
                            cs["u0"][b], cs["q"][b], cs["l"][b], cs["u"][b])[0] for b in range(B_PLANTS)])
    assert np.all(sts == oracle.SOLVED), np.argwhere(sts != oracle.SOLVED)[:8]


def test_new_matrices_differ_and_pairing_is_as_stated(plant):
    """What the shapes are chosen for: N = 20 keeps A's halves negated bit for bit and n % 4 == 0 (the paired
    tile loop, remainder rows 16-19), N = 15 does not qualify; the update changes both matrices."""
    for N, paired in ((20, True), (15, False)):
        cs = shared_case(plant, N)
        for ops in (cs["old"], cs["new"]):
            assert np.array_equal(ops["A"][N:], -ops["A"][:N])
        assert (N % 4 == 0) == paired
        assert not np.allclose(cs["old"]["P"], cs["new"]["P"]) and not np.allclose(cs["old"]["A"], cs["new"]["A"])


EIGEN = Path("/root/reference/include")  # (the one Eigen tests/test_cpp_surface.py compiles against, where readable)


def build_update_caller():
    """tests/cpp/build/update_caller: compiled by build()'s own recipe (__graft_entry__.build_update_caller, the
    flags of tests/cpp/Makefile's reference_caller) where an Eigen include directory is readable; elsewhere the
    program that build() left on such a machine.  None only in a tree whose build had no Eigen at all, which is a
    tree without reference_caller: a tree that has reference_caller and lacks update_caller is a broken build."""
    import __graft_entry__ as entry
    build_dir = ROOT / "tests" / "cpp" / "build"
    exe = build_dir / "update_caller"
    if os.path.exists(EIGEN / "Eigen" / "Dense"):
        return entry.build_update_caller(EIGEN)
    if exe.exists():
        return exe
    assert not (build_dir / "reference_caller").exists(), \
        "the build had an Eigen include directory (reference_caller is there) but left no update_caller"
    return None


def caller_input(cs, b, path):
    """The update caller's input file for QP b of a shared case."""
    rows = [cs["old"]["P"], cs["old"]["A"], cs["q"][b], cs["l"][b], cs["u"][b], cs["new"]["P"], cs["new"]["A"]]
    path.write_text(f"{cs['N']} {2 * cs['N']}\n" + "\n".join(" ".join(f"{v:.17g}" for v in np.ravel(r)) for r in rows) + "\n")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(not os.path.exists(EIGEN / "Eigen" / "Dense"),  # (unreadable counts as absent)
                    reason="needs an Eigen include directory, and this machine has none that this user can read")
def test_update_caller_compiles_against_adapter(tmp_path, plant):
    """updateHessianMatrix / updateLinearConstraintsMatrix compile in the reference's C++11 setting; with no gfx950
    device the caller fails at initSolver() as osqp-eigen reports a failed setup."""
    exe = build_update_caller()
    if _has_gpu():
        return
    caller_input(shared_case(plant, 15, 4), 0, tmp_path / "in.txt")
    r = subprocess.run([str(exe), str(tmp_path / "in.txt")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and r.stdout.startswith("initSolver failed"), (r.returncode, r.stdout)


def test_header_and_mirror_carry_the_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mpcq.h").read_text(), flags=re.S)
    src = (ROOT / "solvempc_amd" / "_capi.py").read_text()
    for name in ("mpcq_update_P_A_device", "mpcq_update_P_A"):
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert f'"{name}": (C.c_int' in src, name
        assert name in _capi.EXPORTS_OSQP_CASE
    lib = _capi.lib()
    assert all(hasattr(lib, n) for n in _capi.EXPORTS_OSQP_CASE)

"""CPU statement of the MIMO step's per-plant horizon reference (mpcq_mimo_step_ref_device and
mpcq_mimo_step_ref_vjp_device), without any device code.

Fr = -2 (Qbar Su)' is block-Toeplitz and upper triangular in blocks, so with F[j] block row j of the stored row sums
Frs = Fr (1_N (x) I_ny) (n_u x n_y, F[N] = 0) and ref_N = 0, summation by parts gives

    (Fr ref)_j = sum_{d=0}^{N-1-j} F[N-1-d] (ref_{j+d} - ref_{j+d+1})
    (Fr' gq)_i = w_i - w_{i-1},   w_i = sum_{j<=i} F[N-1-i+j]' gq_j,   w_{-1} = 0

which is what the two kernels evaluate (``_sbp_forward``, ``_sbp_transposed``: the same sums in the same order).
Both are compared with ``oracle.condense_mimo``'s full Fr and Fr' on the three families of tests/test_mimo_ref.py --
(A) the random n_x 3 / n_u 2 / n_y 2 / N 8 plants with a general K0, (B) the quad-rotor at N 30, (C) the SISO
specialisation at N 20: tests/test_mimo_sensitivity_ref.py's R, Q and S -- under random, mid-horizon step and uniform
references.  Tolerance 1e-12 max|Frs| |ref_b|_1 forward and 1e-12 max|Frs| |gq|_1 transposed: the rounding bound
of the sums is (n + N + 2) eps = 2e-14 of these scales for n <= 128, the measured error at most 4e-17 of them (printed).
A uniform reference must give Frs yref within the same tolerance, and the transposed form summed over the horizon
Frs' gq.

The last two tests fail without the feature: the entry points in the header, the ctypes mirror and the built library,
and the Python names."""
import functools
import subprocess

import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import _capi

from test_mimo_sensitivity_ref import _frs, _inputs
from test_sensitivity_ref import ROOT, _declared

FAM = {"A": "R", "B": "Q", "C": "S"}  # this file's families in tests/test_mimo_sensitivity_ref.py's names
KINDS = ("random", "step", "uniform")
NEW_SYMBOLS = ("mpcq_mimo_step_ref_device", "mpcq_mimo_step_ref", "mpcq_mimo_step_ref_vjp_device",
               "mpcq_mimo_step_ref_gains_device", "mpcq_mimo_step_ref_gains")


def _dims(fam):
    f = _inputs(FAM[fam])
    B, nx, nu = f["Bd"].shape
    ny = np.asarray(f["sh"]["Cd"]).shape[0]
    return B, f["N"], nx, nu, ny


@functools.lru_cache(maxsize=None)
def _ops(fam):
    """oracle.condense_mimo of every plant of a family, once per session."""
    f = _inputs(FAM[fam])
    return [oracle.condense_mimo(dict(f["sh"], Ad=f["Ad"][b], Bd=f["Bd"][b]), f["N"], f["s_rows"])
            for b in range(f["Bd"].shape[0])]


def _yref(fam):
    """The n_y values of a family's uniform reference (family A: tests/test_mimo.py's)."""
    f = _inputs(FAM[fam])
    ny = _dims(fam)[4]
    return np.asarray(f["yref"], dtype=np.float64) if f["yref"] is not None else \
        0.1 * np.random.default_rng(101).normal(size=ny)


@functools.lru_cache(maxsize=None)
def _references(fam):
    """kind -> (B, N n_y): a random reference per plant; one that steps between two random levels at a horizon index
    of its own per plant (1 .. N-1, mid-horizon first), so the preview matters; the uniform 1_N (x) yref."""
    B, N, nx, nu, ny = _dims(fam)
    rng = np.random.default_rng(2024)
    scale = np.abs(_yref(fam)).max()
    rnd = scale * rng.normal(size=(B, N, ny))
    lo, hi = scale * rng.normal(size=(B, 1, ny)), scale * rng.normal(size=(B, 1, ny))
    at = (N // 2 + np.arange(B) - 1) % (N - 1) + 1
    step = np.where(np.arange(N)[None, :, None] < at[:, None, None], lo, hi)
    uni = np.broadcast_to(_yref(fam), (B, N, ny))
    return {"random": rnd.reshape(B, -1).copy(), "step": step.reshape(B, -1).copy(), "uniform": uni.reshape(B, -1).copy()}


def _sbp_forward(Frs, ref, N, nu, ny):
    """Fr ref by summation by parts from the row sums alone: ascending d, then ascending y, as the kernel."""
    F = Frs.reshape(N, nu, ny)
    r = np.vstack([ref.reshape(N, ny), np.zeros((1, ny))])
    out = np.zeros((N, nu))
    for j in range(N):
        for d in range(N - j):
            for y in range(ny):
                out[j] += F[N - 1 - d][:, y] * (r[j + d, y] - r[j + d + 1, y])
    return out.reshape(-1)


def _sbp_transposed(Frs, gq, N, nu, ny):
    """Fr' gq from the row sums alone: w_i and w_{i-1} in ascending j, then their difference, as the kernel."""
    F = Frs.reshape(N, nu, ny)
    g = gq.reshape(N, nu)
    out = np.zeros((N, ny))
    for i in range(N):
        w1, w0 = np.zeros(ny), np.zeros(ny)
        for j in range(i + 1):
            w1 += F[N - 1 - i + j].T @ g[j]
        for j in range(i):
            w0 += F[N - i + j].T @ g[j]
        out[i] = w1 - w0
    return out.reshape(-1)


@pytest.mark.parametrize("fam", sorted(FAM))
def test_summation_by_parts_matches_the_full_operator(fam):
    B, N, nx, nu, ny = _dims(fam)
    refs = _references(fam)
    gqs = np.random.default_rng(77).normal(size=(B, N * nu))
    worst_f = worst_t = worst_u = 0.0
    for b, ops in enumerate(_ops(fam)):
        Fr, Frs = ops["Fr"], _frs(ops, ny)
        fmax = np.abs(Frs).max()
        for kind in KINDS:
            ref = refs[kind][b]
            err = np.abs(_sbp_forward(Frs, ref, N, nu, ny) - Fr @ ref).max()
            scale = fmax * np.abs(ref).sum()
            worst_f = max(worst_f, err / scale)
            assert err <= 1e-12 * scale, (fam, b, kind, err, scale)
        uni = refs["uniform"][b]
        err = np.abs(_sbp_forward(Frs, uni, N, nu, ny) - Frs @ _yref(fam)).max()
        worst_u = max(worst_u, err / (fmax * np.abs(uni).sum()))
        assert err <= 1e-12 * fmax * np.abs(uni).sum(), (fam, b, err)
        gq = gqs[b]
        dref = _sbp_transposed(Frs, gq, N, nu, ny)
        scale = fmax * np.abs(gq).sum()
        err = np.abs(dref - Fr.T @ gq).max()
        worst_t = max(worst_t, err / scale)
        assert err <= 1e-12 * scale, (fam, b, err, scale)
        assert np.abs(dref.reshape(N, ny).sum(axis=0) - Frs.T @ gq).max() <= 1e-12 * scale
    print(f"family {fam}: forward {worst_f:.1e}, uniform against Frs yref {worst_u:.1e}, transposed {worst_t:.1e} "
          f"of the scales (bound 1e-12)")


def test_step_references_differ_per_plant():
    """The step references' switching indices cover the horizon's interior and differ between neighbouring plants."""
    for fam in sorted(FAM):
        B, N, nx, nu, ny = _dims(fam)
        r = _references(fam)["step"].reshape(B, N, ny)
        at = np.array([int(np.flatnonzero((r[b, 1:] != r[b, :-1]).any(axis=1))[0]) + 1 for b in range(B)])
        assert at[0] == N // 2 and at.min() >= 1 and at.max() <= N - 1 and np.all(at[1:] != at[:-1])


def test_mimo_ref_entry_points_in_header_mirror_and_library():
    declared = _declared()
    lib = sm.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(sm.library_path())], check=True, capture_output=True,
                        text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.EXPORTS, name
        assert name in exported, name
        f = getattr(lib, name)
        assert f.restype is not None and f.argtypes, name
    assert len(lib.mpcq_mimo_step_ref_device.argtypes) == 7 and len(lib.mpcq_mimo_step_ref.argtypes) == 6
    assert len(lib.mpcq_mimo_step_ref_vjp_device.argtypes) == 8
    assert len(lib.mpcq_mimo_step_ref_gains_device.argtypes) == 6 and len(lib.mpcq_mimo_step_ref_gains.argtypes) == 5
    assert "DESIGN.md 4.18" in (ROOT / "include" / "mpcq.h").read_text()


def test_python_names_exist():
    for name in ("mimo_step_ref_device", "mimo_step_ref", "mimo_step_ref_vjp_device", "mimo_step_ref_gains",
                 "mimo_step_ref_gains_device"):
        assert callable(getattr(sm.BatchSolver, name)), name
    from solvempc_amd import diff
    assert callable(diff.mimo_ref_solution)

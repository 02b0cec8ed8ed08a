"""BASELINE config 3 in one pass (mpcq_mpc_plants_step_device, solvempc_amd/csrc/mpcq_plant.hip):
every plant condensed, set up and stepped once with its operators kept on chip, against the oracle's
reference constructor + controllerStep per plant (oracle/mpc_batch.c) on the same plants and states.

Bar (every plant): fp64 — the oracle's status and iteration count, the applied U and the whole
solution to 1e-9; fp32 — the oracle's status, its iteration count except on the oracle's own
schedule ties (decision margin < TIE_MARGIN, see test_gpu.py), the applied move and the solution
within 1e-5 * max(1, ||x||_inf).  Plus: agreement with the two-stage path (setup_plants + step), odd
batch sizes (a half-empty last wave), other horizons, and the one-shot context contract."""
import numpy as np
import pytest

import oracle
import solvempc_amd as sm
from solvempc_amd import workload

pytestmark = pytest.mark.gpu
TIE_MARGIN = 2e-3


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")


def _plants(plant, B, seed):
    Ad, Bd = workload.randomized_plants(plant, seed, 0, B)
    X, U = workload.mpc_states(seed, 0, B)
    return Ad, Bd, X, U


def _plant_arrays(plant, Ad, Bd):
    B = Ad.shape[0]
    return [_dev(Ad), _dev(Bd), _dev(np.tile(plant["Cd"], (B, 1))), _dev(np.tile(plant["K"], (B, 1))),
            _dev(np.full(B, plant["Q"])), _dev(np.full(B, plant["R"])), _dev(np.full(B, plant["RD"]))]


def _fused(plant, Ad, Bd, X, U, N, dtype):
    import torch

    B = Ad.shape[0]
    keep = _plant_arrays(plant, Ad, Bd)
    Xd, Ud = _dev(X), _dev(U)
    s = sm.BatchSolver(N, 2 * N, B, n_plants=B, dtype=dtype)
    s.mpc_plants_step_device(4, 10, *[k.data_ptr() for k in keep], Xd.data_ptr(), Ud.data_ptr())
    torch.cuda.synchronize()
    return s, Ud.cpu().numpy()


@pytest.mark.parametrize("N,B", [(20, 257), (15, 64), (32, 33)])
def test_fp64_matches_oracle(plant, N, B):
    Ad, Bd, X, U = _plants(plant, B, 2)
    s, Ug = _fused(plant, Ad, Bd, X, U, N, "f64")
    st, it, rho = s.info()
    U_ref, st_ref, it_ref, x_ref, _ = oracle.plants_step(plant, Ad, Bd, X, U, N, full=True)
    assert np.array_equal(st, st_ref) and np.all(st == sm.SOLVED)
    assert np.array_equal(it, it_ref)
    assert np.abs(Ug - U_ref).max() < 1e-9
    assert np.abs(s.solution() - x_ref).max() < 1e-9


def test_fp32_matches_oracle(plant):
    N, B = 20, 2048
    Ad, Bd, X, U = _plants(plant, B, 2)
    s, Ug = _fused(plant, Ad, Bd, X, U, N, "f32")
    st, it, _ = s.info()
    U_ref, st_ref, it_ref, x_ref, margin = oracle.plants_step(plant, Ad, Bd, X, U, N, full=True)
    assert np.array_equal(st, st_ref)
    off = it != it_ref
    assert not np.any(off & (margin >= TIE_MARGIN)), (np.flatnonzero(off)[:8], margin[off][:8])
    scale = np.maximum(1.0, np.abs(x_ref).max(axis=1))
    x = s.solution()
    assert (np.abs(x - x_ref).max(axis=1)[~off] / scale[~off]).max() < 1e-5
    assert (np.abs(Ug - U_ref)[~off] / scale[~off]).max() < 1e-5


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("N,B", [(20, 301), (17, 98)])
def test_three_plants_per_wave_match_two(plant, dtype, N, B, monkeypatch):
    """At 17 <= N <= 20 the kernel runs three plants per wave (rows plus interleaved tails, lay3_* in
    mpcq_plant.hip) with the association of the two-plants-per-wave layout: every output bit for bit the
    same as MPCQ_PLANT_LAYOUT=2, and each plant's result independent of its slot (0, 1, 2) in the wave."""
    Ad, Bd, X, U = _plants(plant, B, 3)
    out = {}
    for lay in ("2", None):
        if lay:
            monkeypatch.setenv("MPCQ_PLANT_LAYOUT", lay)
        else:
            monkeypatch.delenv("MPCQ_PLANT_LAYOUT", raising=False)
        s, Ug = _fused(plant, Ad, Bd, X, U, N, dtype)
        out[lay] = (s.solution(), s.dual(), Ug, *s.info())
        s.close()
    for a_, b_ in zip(out["2"], out[None]):
        assert np.array_equal(a_, b_, equal_nan=True)
    # the same plants shifted by one slot (a leading copy of plant 0): identical results
    sh = lambda v: np.concatenate([v[:1], v])  # noqa: E731
    s, Ug = _fused(plant, sh(Ad), sh(Bd), sh(X), sh(U), N, dtype)
    assert np.array_equal(s.solution()[1:], out[None][0]) and np.array_equal(Ug[1:], out[None][2])
    assert np.array_equal(s.info()[1][1:], out[None][4])
    s.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_plant_result_independent_of_wave_partner(plant, dtype):
    """Two plants share a wave (one per 32-lane half) and a refactorisation is wave-uniform: a plant
    whose rho never moves must give the same bits whether its partner half adapts rho or not
    (each half rebuilds M at its own rho, rho0 in fp64 until adapt_rho moves it)."""
    N, B = 20, 512
    Ad, Bd, X, U = _plants(plant, B, 2)
    s, _ = _fused(plant, Ad, Bd, X, U, N, dtype)
    st, it, rho = s.info()
    moved = np.abs(rho - 0.1) > 1e-6  # (settings.rho = 0.1; an fp32 rho0 reads 0.1 to 1.5e-9)
    keep = np.flatnonzero(~moved & (st == sm.SOLVED))
    adapt = np.flatnonzero(moved & (st == sm.SOLVED))
    assert keep.size and adapt.size
    i, j = int(keep[0]), int(adapt[0])
    res = []
    for partner in (i, j):
        idx = np.array([i, partner])
        sp, Up = _fused(plant, Ad[idx], Bd[idx], X[idx], U[idx], N, dtype)
        res.append((sp.solution()[0], sp.info()[1][0], Up[0], sp.info()[2][0]))
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1] and res[0][2] == res[1][2]
    assert res[0][3] == res[1][3]


def test_agrees_with_two_stage_path(plant):
    """The same plants through mpcq_mpc_setup_plants_device + mpcq_mpc_step_device (operators in HBM)."""
    import torch

    N, B = 20, 130
    Ad, Bd, X, U = _plants(plant, B, 5)
    sf, Uf = _fused(plant, Ad, Bd, X, U, N, "f64")
    keep = _plant_arrays(plant, Ad, Bd)
    Xd, Ud = _dev(X), _dev(U)
    s2 = sm.BatchSolver(N, 2 * N, B, n_plants=B)
    stream = torch.cuda.current_stream().cuda_stream
    s2.mpc_setup_plants_device(4, 10, *[k.data_ptr() for k in keep], stream)
    s2.mpc_step_device(Xd.data_ptr(), Ud.data_ptr(), 0.0, stream)
    torch.cuda.synchronize()
    assert np.array_equal(sf.info()[0], s2.info()[0]) and np.array_equal(sf.info()[1], s2.info()[1])
    assert np.abs(Uf - Ud.cpu().numpy()).max() < 1e-10
    assert np.abs(sf.solution() - s2.solution()).max() < 1e-10
    assert np.abs(sf.dual() - s2.dual()).max() < 1e-8


def test_one_shot_context_contract(plant):
    """After the one-pass step the context serves its results but no further solves until set up."""
    from solvempc_amd import _capi

    N, B = 20, 8
    Ad, Bd, X, U = _plants(plant, B, 3)
    s, _ = _fused(plant, Ad, Bd, X, U, N, "f64")
    assert s.solution().shape == (B, N) and s.dual().shape == (B, 2 * N)
    with pytest.raises(sm.MpcqError) as e:
        s.solve()
    assert e.value.code == _capi.MPCQ_ERR_ORDER


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_full_config3_batch_every_plant(plant, dtype):
    """The bench's config-3 batch at its size (131,072 randomised plants, seed 2) against the oracle on
    every plant (OpenMP over the host cores, ~2 s on the GPU box), under the module's bar."""
    N, B = 20, 131072
    Ad, Bd, X, U = _plants(plant, B, 2)
    s, Ug = _fused(plant, Ad, Bd, X, U, N, dtype)
    st, it, _ = s.info()
    U_ref, st_ref, it_ref, x_ref, margin = oracle.plants_step(plant, Ad, Bd, X, U, N, full=True)
    assert np.array_equal(st, st_ref) and np.all(st == sm.SOLVED)
    x = s.solution()
    if dtype == "f64":
        assert np.array_equal(it, it_ref)
        assert np.abs(Ug - U_ref).max() < 1e-9 and np.abs(x - x_ref).max() < 1e-9
        return
    off = it != it_ref
    assert not np.any(off & (margin >= TIE_MARGIN)), (np.flatnonzero(off)[:8], margin[off][:8])
    scale = np.maximum(1.0, np.abs(x_ref).max(axis=1))
    assert (np.abs(x - x_ref).max(axis=1)[~off] / scale[~off]).max() < 1e-5
    assert (np.abs(Ug - U_ref)[~off] / scale[~off]).max() < 1e-5
    # a tie's other branch stops one check earlier or later: an OSQP answer at eps_abs = eps_rel = 1e-3
    # of its own, within the eps-level gap of the oracle's (up to ~2e-2)
    assert (np.abs(x - x_ref).max(axis=1)[off] / scale[off]).max(initial=0.0) < 5e-2
    print(f"fp32 config 3: {int(off.sum())} of {B} plants took a tie's other branch")


@pytest.mark.parametrize("dtype,N,B", [("f32", 20, 3001), ("f64", 20, 3001), ("f64", 32, 500), ("f64", 15, 777)])
def test_hardest_first_plants_are_transparent(plant, dtype, N, B, monkeypatch):
    """The one-pass step runs its batch hardest-first (the first plant's order map, mpcq_host_plants.cpp
    plants_order_map, and mpcq_order.hip's counting sort; slot i of the grid runs plant list[i]): every
    output bit-identical to index order (MPCQ_PLANT_ORDER=0) on a ragged batch, the list a permutation of
    it, and the plants that need the most iterations in its first part.  A second step with the same plant
    arrays reuses the map (and the bin counters the first step's kernel cleared).  N = 32 fills the order's
    64 map rows (m = 2N) and runs two plants per wave; N = 15 a short row per plant."""
    Ad, Bd, X, U = _plants(plant, B, 4)

    def run(order):
        if order:
            monkeypatch.delenv("MPCQ_PLANT_ORDER", raising=False)
        else:
            monkeypatch.setenv("MPCQ_PLANT_ORDER", "0")
        import torch

        keep = _plant_arrays(plant, Ad, Bd)
        Xd, Ud = _dev(X), _dev(U)
        s = sm.BatchSolver(N, 2 * N, B, n_plants=B, dtype=dtype)
        out = []
        for _ in range(2):
            s.mpc_plants_step_device(4, 10, *[k.data_ptr() for k in keep], Xd.data_ptr(), Ud.data_ptr())
            torch.cuda.synchronize()
            out += [Ud.cpu().numpy().copy(), s.solution(), s.dual(), *s.info()]
        o, lst = s.order()
        s.close()
        return o, lst, out

    o1, lst, got = run(True)
    o0, _, ref = run(False)
    assert o1 and not o0
    for a_, b_ in zip(got, ref):
        assert np.array_equal(a_, b_, equal_nan=True)
    assert np.array_equal(np.sort(lst), np.arange(B))
    it = ref[4]  # (status, iter, rho of the first step)
    pos = np.empty(B, dtype=np.int64)
    pos[lst] = np.arange(B)
    if N == 20:  # (the bench horizon, where the ranking was measured: DESIGN.md §4.3b)
        assert np.median(pos[it >= np.percentile(it, 95)]) < 0.35 * B


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("poison", ["X", "Ad"])
def test_nonfinite_plant_stays_in_its_own_lanes(plant, dtype, poison, monkeypatch):
    """Every QP is independent, as in OSQP: a plant with a NaN state (X) or non-finite plant data (Ad) must
    leave every other plant's results bit for bit unchanged.  In the three-plants-per-wave layout the lanes of
    no plant (51, 55, 59, 63) belong to plant 2's slot and lane 63 is the zero every other plant's scan carry
    reads, so slot 2 is poisoned: plants 0 and 1 of its wave must not see it (index order, plant i in slot i;
    both layouts; then the hardest-first default, where a NaN key sorts last).  The poisoned plant itself
    gets the same bits in both layouts and: NaN X -> the oracle's (OSQP's) answer, SOLVED with a NaN move
    (OSQP's norms skip NaN); non-finite Ad -> NON_CVX and no move (a documented deviation, include/mpcq.h:
    OSQP would factor the NaN KKT matrix and report SOLVED with NaN)."""
    N, B = 20, 7
    Ad, Bd, X, U = _plants(plant, B, 6)
    Ad2, X2 = Ad.copy(), X.copy()
    if poison == "X":
        X2[2, 1] = np.nan
    else:
        Ad2[2, 0, 0] = np.inf
    poisoned = {}
    for layout, order in (("3", "0"), ("2", "0"), ("3", None)):
        monkeypatch.setenv("MPCQ_PLANT_LAYOUT", layout)
        if order:
            monkeypatch.setenv("MPCQ_PLANT_ORDER", order)
        else:
            monkeypatch.delenv("MPCQ_PLANT_ORDER", raising=False)
        res = []
        for a_, x_ in ((Ad, X), (Ad2, X2)):
            s, Ug = _fused(plant, a_, Bd, x_, U, N, dtype)
            res.append((s.solution(), s.dual(), Ug, *s.info()))
            s.close()
        ok = np.arange(B) != 2
        for a_, b_ in zip(res[0], res[1]):
            assert np.array_equal(a_[ok], b_[ok], equal_nan=True)
        assert np.all(res[0][3] == sm.SOLVED)
        poisoned[layout] = [v[2] for v in res[1]]
        st2, U2 = res[1][3][2], res[1][2][2]
        if poison == "X":
            _, st_ref, it_ref, _, _ = oracle.plants_step(plant, Ad2, Bd, X2, U, N, full=True)
            assert st2 == st_ref[2] == sm.SOLVED and np.isnan(U2), (st2, st_ref[2])
            if dtype == "f64":
                assert res[1][4][2] == it_ref[2]
        else:
            assert st2 == sm.NON_CVX and U2 == U[2]
    for a_, b_ in zip(poisoned["3"], poisoned["2"]):
        assert np.array_equal(a_, b_, equal_nan=True)

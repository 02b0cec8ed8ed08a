"""Static budget of the closed-loop MIMO run's kernels (CPU only: the gfx950 code objects' metadata,
tools/kernel_resources.py; skipped as tests/test_kernel_resources.py is).  mimo_plant_kernel keeps a QP's row in a
handful of registers and mimo_sched_tail_kernel copies one value per thread: neither may use scratch or LDS.  The run
adds no instantiation of the control step's kernels: exactly the twelve mimo_solve* rows remain."""
import os
import shutil

import pytest

import tools.kernel_resources as kr

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.BUILD) or shutil.which("c++filt") is None
                                or not os.path.exists(f"{kr.LLVM}/clang-offload-bundler"),
                                reason="needs the built objects and the ROCm LLVM tools")


def _one(rows, name):
    hit = [r for r in rows if r["kernel"].startswith(name)]
    assert len(hit) == 1, (name, [r["kernel"] for r in rows])
    return hit[0]


def test_plant_and_tail_kernels_use_no_scratch():
    plant = _one(kr.table("mimo_plant_kernel"), "mpcq::mimo_plant_kernel(")
    tail = _one(kr.table("mimo_sched_tail_kernel"), "mpcq::mimo_sched_tail_kernel(")
    for r in (plant, tail):
        print(f"{r['kernel']}: {r['vgpr']} VGPRs, scratch {r['scratch']} B, LDS {r['lds']} B")
        assert r["object"] == "mpcq_mimo_run"
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0
    assert plant["vgpr"] <= 64  # (256 threads per workgroup at full occupancy)


def test_the_twelve_mimo_solve_kernels_are_still_there():
    got = sorted(r["kernel"] for r in kr.table("mimo_solve"))
    want = sorted(f"void mpcq::mimo_solve{ref}_kernel<{nu}, {k0}>(mpcq::Mimo{arg}Args)"
                  for ref, arg in (("", ""), ("_ref", "Ref")) for nu in (1, 2, 4) for k0 in ("false", "true"))
    assert got == want, got

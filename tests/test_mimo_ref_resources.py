"""Static budget of the MIMO reference step's kernel (CPU only: the gfx950 code objects' metadata,
tools/kernel_resources.py; skipped as tests/test_kernel_resources.py is).  The reference term is prologue: the
benched shape's kernel keeps the solve kernel's register budget and spills no more than it."""
import os
import shutil

import pytest

import tools.kernel_resources as kr

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.BUILD) or shutil.which("c++filt") is None
                                or not os.path.exists(f"{kr.LLVM}/clang-offload-bundler"),
                                reason="needs the built objects and the ROCm LLVM tools")


def _one(rows, prefix):
    hit = [r for k, r in rows.items() if k.startswith(prefix)]
    assert len(hit) == 1, (prefix, [r["kernel"] for r in hit])
    return hit[0]


def test_config4_mimo_solve_ref_budget():
    rows = {r["kernel"]: r for r in kr.table("mimo_solve")}
    ref = _one(rows, "void mpcq::mimo_solve_ref_kernel<4, true>")
    plain = _one(rows, "void mpcq::mimo_solve_kernel<4, true>")
    print(f"mimo_solve_ref_kernel<4, true>: {ref['vgpr']} VGPRs, scratch {ref['scratch']} B "
          f"(mimo_solve_kernel<4, true>: {plain['scratch']} B)")
    assert ref["vgpr"] <= 256
    assert ref["scratch"] <= plain["scratch"]

"""Static resources of mimo_plant_vjp_kernel (solvempc_amd/csrc/mpcq_mimo_plant_vjp.hip) against what DESIGN.md 4.17
states (CPU only: the gfx950 code objects' metadata, tools/kernel_resources.py, and the launcher's LDS carve-up)."""
import ctypes as C
import os
import re
import shutil
from pathlib import Path

import pytest

import solvempc_amd as sm
import tools.kernel_resources as kr

pytestmark = pytest.mark.skipif(not os.path.isdir(kr.BUILD) or shutil.which("c++filt") is None
                                or not os.path.exists(f"{kr.LLVM}/clang-offload-bundler"),
                                reason="needs the built objects and the ROCm LLVM tools")
ROOT = Path(__file__).resolve().parents[1]
LDS_CU = 160 * 1024
# (N, nx, nu, ny) of the table: families R, odd, S, Q (config 4), Q32 and the largest shape the setup accepts
SHAPES = ((8, 3, 2, 2), (15, 3, 2, 2), (20, 4, 1, 1), (30, 12, 4, 12), (32, 12, 4, 12))


@pytest.fixture(scope="module")
def section():
    doc = (ROOT / "DESIGN.md").read_text()
    m = re.search(r"^### 4\.17 .*?(?=^### |^## )", doc, flags=re.S | re.M)
    assert m, "DESIGN.md has no section 4.17"
    return m.group(0)


def _lds(N, nx, nu, ny):
    f = sm.lib().mpcq_internal_mimo_plant_vjp_lds
    f.restype, f.argtypes = C.c_size_t, [C.c_int] * 4
    return int(f(N, nx, nu, ny))


def test_registers_scratch_and_static_lds_are_the_documented_ones(section):
    rows = {r["kernel"]: r for r in kr.table("mimo_plant_vjp_kernel")}
    assert len(rows) == 3, sorted(rows)
    for nu in (1, 2, 4):
        r = rows[f"void mpcq::mimo_plant_vjp_kernel<{nu}>(mpcq::MimoPlantVjpArgs)"]
        line = (f"| `mimo_plant_vjp_kernel<{nu}>` | {r['vgpr']} | {r['agpr']} | {r['scratch']} | {r['vgpr_spill']} | "
                f"{r['lds']} |")
        assert line in section, line
        # nothing of the kernel lives in scratch, and two 4-wave workgroups fit a CU's registers (2 waves per SIMD)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["vgpr"] + r["agpr"] <= 256


def test_lds_carve_up_is_the_documented_one_and_fits(section):
    static = max(r["lds"] for r in kr.table("mimo_plant_vjp_kernel"))
    for shape in SHAPES:
        b = _lds(*shape)
        per_cu = min(8, LDS_CU // (b + static))
        assert f"| {' | '.join(str(v) for v in shape)} | {b:,} | {per_cu} |" in section, (shape, b, per_cu)
        assert per_cu >= 1
    # sized by the call's shape, not by the capacity: config 4 and the capacity itself leave room for two plants per CU
    assert LDS_CU // (_lds(30, 12, 4, 12) + static) == 2 and LDS_CU // (_lds(32, 12, 4, 12) + static) == 2

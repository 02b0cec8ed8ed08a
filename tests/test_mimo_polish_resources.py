"""Static resources of polish_mimo_kernel (solvempc_amd/csrc/mpcq_mimo_polish.hip) against what DESIGN.md 4.16 states
(CPU only: the gfx950 code objects' metadata, tools/kernel_resources.py, and the launcher's LDS carve-up)."""
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


@pytest.fixture(scope="module")
def section():
    doc = (ROOT / "DESIGN.md").read_text()
    m = re.search(r"^### 4\.16 .*?(?=^### |^## )", doc, flags=re.S | re.M)
    assert m, "DESIGN.md has no section 4.16"
    return m.group(0)


def _lds(n):
    f = sm.lib().mpcq_internal_mimo_polish_lds
    f.restype, f.argtypes = C.c_size_t, [C.c_int]
    return int(f(n))


def test_variants_are_listed_once_without_scratch_or_spills(section):
    rows = {r["kernel"]: r for r in kr.table("polish_mimo_kernel")}
    assert len(rows) == 3 and len(kr.table("polish_mimo_kernel")) == 3, sorted(rows)
    for nu in (1, 2, 4):
        r = rows[f"void mpcq::polish_mimo_kernel<{nu}>(mpcq::MimoPolishArgs)"]
        line = f"| `polish_mimo_kernel<{nu}>` | {r['vgpr']} | {r['agpr']} | {r['scratch']} | {r['vgpr_spill']} | {r['lds']} |"
        assert line in section, line
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["vgpr"] + r["agpr"] <= 512


def test_lds_carve_up_is_the_documented_one_and_fits(section):
    static = max(r["lds"] for r in kr.table("polish_mimo_kernel"))
    for n in (16, 20, 30, 120, 128):
        b = _lds(n)
        assert f"| {n} | {b:,} |" in section, (n, b)
        assert b + static <= LDS_CU
    assert _lds(128) <= 163840 and _lds(128) > 2 * 8 * (128 * 129 // 2)  # two packed triangles and the vectors

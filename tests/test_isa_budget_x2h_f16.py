"""Register / scratch / LDS budget and MFMA mix of the split-f16 x2h edge kernel (edge_x2h_f16.hip), read from the gfx950 ISA that
hipcc emits (no GPU needed; the recipe of tests/test_isa_budget.py)."""
import os
import re

import pytest

from tests.test_isa_budget import HIPCC, find, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_x2h_f16_kernels_fit_their_budget_and_run_no_fp32_mfma(tmp_path):
    res, text = kernel_resources("edge_x2h_f16.hip", tmp_path)
    assert not [k for k in res if "edge_x2h_dual_kernel" in k or "edge_mfma_kernel" in k]
    for inst in ("ILi8ELb1E", "ILi8ELb0E"):            # <WAVES = 8, FULL_LAYER>: full-layer and listed launches
        k = find(res, "edge_x2h_f16_kernel" + inst)
        assert k["scratch"] == 0 and k["vgpr"] <= 256, k        # 8 waves per CU = 2 per SIMD; a spill's reload drains the gathers
        assert k["lds"] <= 160 * 1024, k
        start = re.search(r"^_ZN4cbgx19edge_x2h_f16_kernel" + inst + r"\S*:", text, flags=re.M).start()
        body = text[start:text.index(".end_amdhsa_kernel", start)]
        mfma32 = len(re.findall(r"^\s+v_mfma_f32_16x16x4", body, flags=re.M))
        mfma16 = len(re.findall(r"^\s+v_mfma_f32_16x16x16_f16", body, flags=re.M))
        mfma16k32 = len(re.findall(r"^\s+v_mfma_f32_16x16x32_f16", body, flags=re.M))
        # both roles inlined.  rbf pre-activation as in edge_x2h_dual_kernel: 128 (protein-only role, one source-class pass) + 256
        # (general role) = 384 K = 16 MFMAs; scores and aggregation each add 8 tiles x 2 halves x 3 products = 48 per role; no
        # exact-fp32 MFMA is left, and no K = 32 f16 MFMA (measured not reproducible from launch to launch in this kernel)
        assert mfma32 == 0, mfma32
        assert mfma16 == 384 + 2 * 48 + 2 * 48, mfma16
        assert mfma16k32 == 0, mfma16k32


def test_shared_body_reads_the_lds_tables_as_the_pack_kernels_write_them():
    """tests/test_lds_layouts.py pins the addressing of the fold table and of the h2x head rows by the text of edge_mfma.hip, where the pack kernel lives; the reading
    side moved to edge_body.h with the body: the same two expressions, as code, there"""
    from tests.test_isa_budget import CSRC
    code = [l.split("//")[0] for l in open(os.path.join(CSRC, "edge_body.h"))]
    for expr in ("wf + 2048 * t + 256 * d", "lds + PP_WFOLD + 4 * lane", "lds + IMG_WBV + 4 * lane", "ld4(lds_brow + 256 * t)"):
        assert any(expr in l for l in code), expr

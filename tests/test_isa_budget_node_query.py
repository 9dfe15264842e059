"""Budget of node_query_kernel (cbgbench_amd/csrc/node_mfma.hip), read from the gfx950 ISA that hipcc emits (no GPU needed): one
8-wave workgroup per CU with both 64 KB tables resident in LDS = two waves per SIMD, which need <= 256 registers, and no spill -- a
scratch reload's wait would drain the next tile's rows, which are in flight across the whole MFMA block."""
import os
import re

import pytest

from tests.test_isa_budget import HIPCC, find, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_node_query_kernel_fits_its_budget(tmp_path):
    res, text = kernel_resources("node_mfma.hip", tmp_path)
    k = find(res, "node_query_kernel")
    assert k["scratch"] == 0 and k["vgpr"] <= 256 and k["lds"] <= 160 * 1024, k
    assert k["lds"] >= 128 * 1024, k          # both tables resident
    # both products on the K = 32 f16 instruction: 2 x 8 output tiles x 4 K chunks x 3 split-f16 terms
    start = re.search(r"^_ZN4cbgx17node_query_kernel\S*:", text, flags=re.M).start()
    body = text[start:text.index(".end_amdhsa_kernel", start)]
    assert len(re.findall(r"^\s+v_mfma_f32_16x16x32_f16", body, flags=re.M)) == 192
    assert "scratch_" not in body and "ds_bpermute" in body
    # the names test_isa_budget.py looks kernels up by still match exactly one kernel each
    for name in ("node_proj_kernelILb0E", "node_proj_kernelILb1E", "node_qmlp_kernel", "node_qfold_kernelILi4E",
                 "node_qfold_kernelILi16E"):
        find(res, name)

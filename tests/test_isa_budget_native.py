"""Scratch, LDS and register budget of the two kernels of the comparison with a native ligand (csrc/native.hip), read from the gfx950 ISA
that hipcc emits (no GPU needed), on the recipe of tests/test_isa_budget_diversity.py: the float64 distance and the sequential centroid
sum stay in registers, the staged ligand of 1024 atoms stays inside the LDS of a workgroup.  Resource numbers only."""
import os

import pytest

from tests.test_isa_budget import HIPCC, find, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("kernel", ["pocket_contacts_kernel", "native_compare_kernel"])
def test_native_kernels_do_not_spill(kernel, tmp_path):
    res, _ = kernel_resources("native.hip", tmp_path)
    k = find(res, kernel)
    assert k["scratch"] == 0 and k["lds"] <= 64 * 1024 and k["vgpr"] <= 256, k

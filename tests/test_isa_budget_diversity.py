"""Scratch, LDS and register budget of the two diversity kernels (csrc/diversity.hip), read from the gfx950 ISA that hipcc emits (no GPU
needed), on the recipe of tests/test_isa_budget_groups.py: the 64-bit products of the refinement stay in registers, the staged graph and
the per-graph keys of a group of 1024 stay inside the LDS of a workgroup.  Resource numbers only."""
import os

import pytest

from tests.test_isa_budget import HIPCC, find, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("kernel", ["ligand_fingerprints_kernel", "group_diversity_kernel"])
def test_diversity_kernels_do_not_spill(kernel, tmp_path):
    res, _ = kernel_resources("diversity.hip", tmp_path)
    k = find(res, kernel)
    assert k["scratch"] == 0 and k["lds"] <= 64 * 1024 and k["vgpr"] <= 256, k

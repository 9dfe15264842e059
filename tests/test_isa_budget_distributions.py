"""Scratch and LDS budgets of the two distributions kernels (csrc/distributions.hip), read from the gfx950 ISA that hipcc emits (no GPU
needed), on the recipe of tests/test_isa_budget.py: both compile without scratch, and their static LDS -- the staged ligand, the edge
tables, the histograms or the per-centre ranges -- leaves room for more than one workgroup per CU."""
import os

import pytest

from tests.test_isa_budget import HIPCC, find, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_distributions_kernels_do_not_spill(tmp_path):
    res, text = kernel_resources("distributions.hip", tmp_path)
    for name in ("ligand_pair_hist_kernel", "ligand_angles_kernel"):
        k = find(res, name)
        assert k["scratch"] == 0 and k["lds"] <= 64 * 1024 and k["vgpr"] <= 128, (name, k)
    # the bin decisions are comparisons against staged tables: nothing here calls an inverse trigonometric routine
    assert "acos" not in text and "atan" not in text

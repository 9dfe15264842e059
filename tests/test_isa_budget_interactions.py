"""Scratch, LDS and register budget of the two interaction kernels (csrc/interactions.hip), read from the gfx950 ISA that hipcc emits (no
GPU needed), on the recipe of tests/test_isa_budget.py: the five fp64 accumulators of a ligand atom and the software exp stay in
registers, and the staged ligand with its pocket tile stays inside the LDS of a workgroup."""
import os

import pytest

from tests.test_isa_budget import HIPCC, find, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_interaction_kernels_do_not_spill(tmp_path):
    res, _ = kernel_resources("interactions.hip", tmp_path)
    for name in ("pocket_types_kernel", "ligand_interactions_kernel"):
        k = find(res, name)
        assert k["scratch"] == 0 and k["lds"] <= 64 * 1024 and k["vgpr"] <= 256, (name, k)

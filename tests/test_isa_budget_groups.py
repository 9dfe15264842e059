"""Scratch, LDS and register budget of the functional-group kernel (csrc/groups.hip), read from the gfx950 ISA that hipcc emits (no GPU
needed), on the recipe of tests/test_isa_budget_valence.py: the isomorphism test keeps its partial map and the group's labels in 64-bit
registers -- no recursion, no scratch --, and the staged graph with the per-lane bond-type matrices stays inside the LDS of a workgroup.
Resource numbers only."""
import os

import pytest

from tests.test_isa_budget import HIPCC, find, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_groups_kernel_does_not_spill(tmp_path):
    res, _ = kernel_resources("groups.hip", tmp_path)
    k = find(res, "ligand_groups_kernel")
    assert k["scratch"] == 0 and k["lds"] <= 64 * 1024 and k["vgpr"] <= 256, k

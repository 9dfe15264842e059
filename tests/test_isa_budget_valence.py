"""Scratch and LDS budget of the valence kernel (csrc/valence.hip), read from the gfx950 ISA that hipcc emits (no GPU needed), on the
recipe of tests/test_isa_budget.py: the backtracking search keeps its matched atoms and its decisions in 64-bit registers -- no recursion,
no scratch --, and the staged graph with the per-lane lists of eligible bonds stays inside the LDS of a workgroup."""
import os

import pytest

from tests.test_isa_budget import HIPCC, find, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_valence_kernel_does_not_spill(tmp_path):
    res, _ = kernel_resources("valence.hip", tmp_path)
    k = find(res, "ligand_valence_kernel")
    assert k["scratch"] == 0 and k["lds"] <= 64 * 1024 and k["vgpr"] <= 256, k

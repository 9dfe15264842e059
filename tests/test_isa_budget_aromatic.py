"""Scratch and LDS budget of the aromatic kernel (csrc/aromatic.hip), read from the gfx950 ISA that hipcc emits (no GPU needed), on the
recipe of tests/test_isa_budget.py: the walk over induced paths keeps its atoms in registers -- no scratch --, and the staged graph with
its adjacency bit matrix leaves room for several one-wave workgroups per CU."""
import os

import pytest

from tests.test_isa_budget import HIPCC, find, kernel_resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_aromatic_kernel_does_not_spill(tmp_path):
    res, _ = kernel_resources("aromatic.hip", tmp_path)
    k = find(res, "ligand_aromatic_kernel")
    assert k["scratch"] == 0 and k["lds"] <= 64 * 1024 and k["vgpr"] <= 256, k

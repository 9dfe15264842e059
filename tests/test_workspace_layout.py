"""The byte layout of the forward workspace, the training workspace and the two tapes is pinned: pure address arithmetic of the host
code (csrc/api.hip carve, csrc/api_train.hip), no device needed.

tests/golden/workspace_layout.json holds what the library returned before the node lists of the forward workspace got names (recorded
results of cbgx_workspace_bytes, cbgx_train_workspace_bytes, cbgx_train_tape_bytes, cbgx_h2x_stack_tape_bytes and of
cbgx_debug_forward_view on a made-up base address).  Node counts 1, 255, 256, 257 cross the 256-byte alignment of the per-node flag
arrays, 8 192 / 8 193 the two list regimes; the training sizes are taken at two layer counts."""
import ctypes
import json
import os

import pytest

from cbgbench_amd import _native, stages

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_layout.json")) as _f:
    GOLDEN = json.load(_f)
NS = GOLDEN["n_nodes"]
N_PTRS = 5 + 2 * len(stages.FORWARD_LISTS)


def test_golden_covers_the_boundaries():
    assert NS == [1, 255, 256, 257, 8192, 8193] and len(GOLDEN["num_layers"]) == 2 and N_PTRS == 37
    assert all(len(GOLDEN["forward_view_offsets"][str(n)]) == N_PTRS for n in NS)


@pytest.mark.parametrize("n", NS)
def test_byte_sizes_are_unchanged(n):
    lib = _native.lib()
    for g in GOLDEN["n_graphs"]:
        assert lib.cbgx_workspace_bytes(n, g) == GOLDEN["workspace_bytes"][str(n)][str(g)]
    assert lib.cbgx_train_workspace_bytes(n) == GOLDEN["train_workspace_bytes"][str(n)]
    for L in GOLDEN["num_layers"]:
        assert lib.cbgx_train_tape_bytes(n, L) == GOLDEN["train_tape_bytes"][str(L)][str(n)]
        assert lib.cbgx_h2x_stack_tape_bytes(n, L) == GOLDEN["h2x_stack_tape_bytes"][str(L)][str(n)]


@pytest.mark.parametrize("n", NS)
def test_forward_view_offsets_are_unchanged(n):
    base = GOLDEN["base"]
    out = (ctypes.c_void_p * N_PTRS)()
    with _native.first_generation_kernels(0) as xlib:
        assert xlib.cbgx_debug_forward_view(ctypes.c_void_p(base), n, out) == 0
        total = xlib.cbgx_workspace_bytes(n, 1)
    assert total == GOLDEN["workspace_bytes"][str(n)]["1"]
    ptrs = [int(p) for p in out]
    assert [p - base for p in ptrs] == GOLDEN["forward_view_offsets"][str(n)]
    assert len(set(ptrs)) == N_PTRS and all(base <= p < base + total for p in ptrs)
    counts = sorted(ptrs[6 + 2 * k] for k in range(len(stages.FORWARD_LISTS)))
    assert len(counts) == 16 and all(b - a >= 64 for a, b in zip(counts, counts[1:]))

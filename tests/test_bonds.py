"""Bond list, fragments and connectivity (cbgbench_amd/geometry.py: ligand_bonds, summarise_bonds; csrc/geometry.hip), host side: the numpy
model (tests/bonds_model.py) against the reference's get_bond_order / check_stability and against independent component searches,
``summarise_bonds`` against hand-computed counts, the C ABI of the two entries without a device, and the driver's refusal of a CPU device.
The kernels themselves are compared with the model in tests/test_gpu_bonds.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from cbgbench_amd import _native, geometry as G
from tests import bonds_model as BM
from tests.test_geometry import SYMBOLS, _load, molecules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref_stability():
    return _load("eval_stability")


# ---- the model against the reference -------------------------------------------------------------------------------------------------
def test_model_bonds_equal_get_bond_order(ref_stability):
    """on the 50 seeded molecules: every pair i < j has the model's order equal to get_bond_order(symbol_i, symbol_j, dist), dist as
    check_stability computes it; the list holds exactly the pairs with order > 0, in (i, j) order; per-atom sums of the list's orders
    equal check_stability's nr_bonds"""
    symbol = {z: s for z, s in zip((1, 6, 7, 8, 9, 15, 16, 17), SYMBOLS)}
    orders, frag_seen = set(), set()
    for x, z, _, _ in molecules():
        n = len(z)
        r = BM.graph_bonds(x, z)
        got = np.zeros((n, n), np.int64)
        got[r["bond_index"][0], r["bond_index"][1]] = r["bond_order"]
        xd = x.astype(np.float64)
        for i in range(n):
            for j in range(i + 1, n):
                dist = np.sqrt(np.sum((xd[i] - xd[j]) ** 2))
                assert got[i, j] == ref_stability.get_bond_order(symbol[int(z[i])], symbol[int(z[j])], dist), (n, i, j)
        pairs = list(zip(*r["bond_index"].tolist()))
        assert pairs == sorted(set(pairs)) and all(i < j for i, j in pairs) and (r["bond_order"] > 0).all()
        nr = np.zeros(n, np.int64)
        np.add.at(nr, r["bond_index"][0], r["bond_order"])
        np.add.at(nr, r["bond_index"][1], r["bond_order"])
        nr_ref = ref_stability.check_stability(xd, z, hs=False, return_nr_bonds=True)[3]
        assert np.array_equal(nr, nr_ref)
        assert r["counts"].tolist()[:3] == [n, len(pairs), int(r["bond_order"].sum())]
        assert np.array_equal(r["deg_up"], np.bincount(r["bond_index"][0], minlength=n))
        orders |= set(r["bond_order"].tolist())
        frag_seen.add(int(r["counts"][3]) == 1)
    assert orders == {1, 2, 3} and frag_seen == {True, False}


def _bfs_labels(n, pairs):
    adj = [[] for _ in range(n)]
    for i, j in pairs:
        adj[i].append(j)
        adj[j].append(i)
    label = [-1] * n
    for s in range(n):                    # ascending: the first atom to reach a component is its smallest
        if label[s] >= 0:
            continue
        label[s], queue = s, [s]
        while queue:
            a = queue.pop()
            for b in adj[a]:
                if label[b] < 0:
                    label[b] = s
                    queue.append(b)
    return label


def test_model_components_equal_an_independent_search():
    mols = [(x, z) for x, z, _, _ in molecules()]
    # and two shapes a chain recipe does not make: a scrambled straight chain, and rings with a lone atom
    perm = np.random.default_rng(5).permutation(200)
    mols.append((np.stack([1.5 * perm, 0 * perm, 0 * perm], 1).astype(np.float32), np.full(200, 6)))
    ang = np.arange(6) * np.pi / 3
    hexagon = 1.5 * np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)
    mols.append((np.concatenate([hexagon, hexagon + [20, 0, 0], [[0, 40, 0]]]).astype(np.float32), np.full(13, 6)))
    for x, z in mols:
        n = len(z)
        r = BM.graph_bonds(x, z)
        pairs = list(zip(*r["bond_index"].tolist()))
        want = _bfs_labels(n, pairs)
        assert r["fragment"].tolist() == want
        sizes = np.bincount(want, minlength=n)
        n_frag = len(set(want))
        assert r["counts"].tolist() == [n, len(pairs), int(r["bond_order"].sum()), n_frag, int(sizes.max()), len(pairs) - n + n_frag]
        try:
            from scipy.sparse import coo_matrix
            from scipy.sparse.csgraph import connected_components
        except ImportError:
            continue
        i, j = r["bond_index"]
        nc, lab = connected_components(coo_matrix((np.ones(len(i)), (i, j)), shape=(n, n)), directed=False)
        first = np.full(nc, n)
        np.minimum.at(first, lab, np.arange(n))
        assert nc == n_frag and first[lab].tolist() == want
    assert BM.graph_bonds(*mols[-2])["counts"].tolist() == [200, 199, 199, 1, 200, 0]
    assert BM.graph_bonds(*mols[-1])["counts"].tolist() == [13, 12, 12, 3, 6, 2]


def test_model_single_atom_and_empty():
    r = BM.graph_bonds(np.zeros((1, 3), np.float32), [6])
    assert r["fragment"].tolist() == [0] and r["counts"].tolist() == [1, 0, 0, 1, 1, 0] and r["bond_index"].shape == (2, 0)
    r = BM.graph_bonds(np.zeros((0, 3), np.float32), [])
    assert r["fragment"].shape == (0,) and r["counts"].tolist() == [0] * 6
    # Br 1.5 A from a carbon: no bond, its own fragment
    r = BM.graph_bonds(np.array([[0, 0, 0], [1.5, 0, 0]], np.float32), [6, 35])
    assert r["fragment"].tolist() == [0, 1] and r["counts"].tolist() == [2, 0, 0, 2, 1, 0]


# ---- summarise_bonds -----------------------------------------------------------------------------------------------------------------
def test_summarise_bonds_against_hand_computed_counts():
    #      n_atoms n_bonds order_sum n_fragments largest n_cycles
    gc = [[10, 11, 14, 1, 10, 2],
          [20, 15, 15, 5, 9, 0],
          [1, 0, 0, 1, 1, 0],
          [0, 0, 0, 0, 0, 0],
          [9, 7, 9, 2, 5, 0]]
    s = G.summarise_bonds(gc)
    assert s["counts"] == {"n_mol": 5, "n_atoms": 40, "n_bonds": 33, "n_connected_mol": 2, "n_largest_fragment_atoms": 25,
                           "n_fragments": 9, "n_cycles": 2}
    assert s["connected_mol_ratio"] == 2 / 5 and s["largest_fragment_atom_ratio"] == 25 / 40 and s["fragments_per_mol"] == 9 / 5
    assert s["cycles_per_mol"] == 2 / 5 and s["bonds_per_atom"] == 33 / 40
    assert set(s) == set(G.BOND_RATIOS) | {"counts"} and tuple(s["counts"]) == G.BOND_COUNT_KEYS
    assert G.BOND_GRAPH_COLUMNS == ("n_atoms", "n_bonds", "bond_order_sum", "n_fragments", "largest_fragment", "n_cycles")
    whole = G.bond_totals(gc)
    parts = [a + b for a, b in zip(G.bond_totals(gc[:2]), G.bond_totals(gc[2:]))]
    assert whole == parts == [5, 40, 33, 2, 25, 9, 2] and G.summarise_bond_totals(parts) == s
    import torch
    assert G.summarise_bonds(torch.tensor(gc, dtype=torch.int32)) == s
    empty = G.summarise_bonds(np.zeros((0, 6), np.int32))
    assert empty["counts"]["n_mol"] == 0 and all(np.isnan(empty[k]) for k in G.BOND_RATIOS)
    # the geometry report's names are what they were
    assert len(G.GRAPH_COLUMNS) == 6 and len(G.COUNT_KEYS) == 8 and len(G.RATIOS) == 5


def test_cpu_tensors_raise():
    import torch
    x, z, b = torch.zeros(2, 3), torch.tensor([6, 6]), torch.zeros(2, dtype=torch.long)
    with pytest.raises(_native.NativeError):
        G.ligand_bonds(x, z, b, 1)
    with pytest.raises(_native.NativeError):
        G.batch_bonds({"num_graphs": 1}, x, torch.zeros(2, dtype=torch.long), b, "basic")


def test_sample_cli_bonds_needs_the_gpu():
    from cbgbench_amd import sample_cli
    cfg = os.path.join(ROOT, "tests", "fixtures", "targetdiff_T20.yml")
    with pytest.raises(SystemExit, match="--bonds runs on the GPU"):
        sample_cli.main(["--config", cfg, "--device", "cpu", "--bonds", "--random_init", "--synthetic", "1"])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("cbgx_ligand_bonds_count", "cbgx_ligand_bonds_fill")


def test_entries_are_declared_bound_and_exported():
    from cbgbench_amd.build import LIBPATH, XCHECK_LIBPATH
    hdr = open(os.path.join(ROOT, "include", "cbgx.h")).read()
    lib = _native.lib()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", hdr) and name in _native.EXPORTS and hasattr(lib, name)
    for path in (LIBPATH, XCHECK_LIBPATH):
        sym = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        for name in ENTRIES:
            assert f" {name}\n" in sym, (path, name)
    assert lib.cbgx_abi_version() == _native.ABI_VERSION == 6
    assert f"#define CBGX_BONDS_GRAPH_COLS {len(G.BOND_GRAPH_COLUMNS)}" in hdr


ONE = ctypes.c_void_p(16)       # a pointer that is never dereferenced: argument checks come first


def _count(lig_ptr, n_lig, B, x_lig=ONE, z_lig=ONE, deg_up=ONE, fragment=ONE, graph_out=ONE):
    lp = np.asarray([] if lig_ptr is None else lig_ptr, np.int32)
    lptr = ctypes.c_void_p(lp.ctypes.data) if lig_ptr is not None else None
    return _native.lib().cbgx_ligand_bonds_count(x_lig, z_lig, lptr, n_lig, B, deg_up, fragment, graph_out, None)


def _fill(lig_ptr, n_lig, B, n_bonds, x_lig=ONE, z_lig=ONE, bond_ptr=ONE, bond_index=ONE, bond_order=ONE, bond_length=ONE):
    lp = np.asarray([] if lig_ptr is None else lig_ptr, np.int32)
    lptr = ctypes.c_void_p(lp.ctypes.data) if lig_ptr is not None else None
    return _native.lib().cbgx_ligand_bonds_fill(x_lig, z_lig, lptr, n_lig, B, bond_ptr, n_bonds, bond_index, bond_order, bond_length, None)


def test_argument_errors_are_returned_without_a_gpu():
    lib = _native.lib()
    ok = [0, 2, 4]
    bad = [_count(ok, 4, -1), _count(ok, -1, 2), _count(None, 4, 2), _count(ok, 4, 2, x_lig=None), _count(ok, 4, 2, z_lig=None),
           _count(ok, 4, 2, deg_up=None), _count(ok, 4, 2, fragment=None), _count(ok, 4, 2, graph_out=None)]
    assert bad == [-1] * len(bad), bad
    assert _count(ok, 4, 2, fragment=None) == -1 and b"NULL" in lib.cbgx_last_error()
    assert _count(ok, -1, 2) == -1 and b"negative" in lib.cbgx_last_error()
    assert _count(None, 0, 0, x_lig=None, z_lig=None, deg_up=None, fragment=None, graph_out=None) == 0
    assert _count(None, 7, 0, graph_out=None) == 0
    bad = [_fill(ok, 4, -1, 3), _fill(ok, -1, 2, 3), _fill(ok, 4, 2, -1), _fill(None, 4, 2, 3), _fill(ok, 4, 2, 3, x_lig=None),
           _fill(ok, 4, 2, 3, z_lig=None), _fill(ok, 4, 2, 3, bond_ptr=None), _fill(ok, 4, 2, 3, bond_index=None),
           _fill(ok, 4, 2, 3, bond_order=None), _fill(ok, 4, 2, 3, bond_length=None)]
    assert bad == [-1] * len(bad), bad
    assert _fill(ok, 4, 2, 3, bond_order=None) == -1 and b"NULL" in lib.cbgx_last_error()
    assert _fill(ok, 4, 2, -1) == -1 and b"negative" in lib.cbgx_last_error()
    assert _fill(None, 0, 0, 0, x_lig=None, z_lig=None, bond_ptr=None, bond_index=None, bond_order=None, bond_length=None) == 0
    # no bonds: nothing to write, no launch, the lists may be NULL
    assert _fill(ok, 4, 2, 0, bond_index=None, bond_order=None, bond_length=None) == 0


def test_a_ligand_above_1024_atoms_is_refused():
    lib = _native.lib()
    for call in (_count, lambda p, n, B: _fill(p, n, B, 5)):
        assert call([0, 3, 1028, 1030], 1030, 3) == -1
        msg = lib.cbgx_last_error().decode()
        assert "graph 1" in msg and "1025" in msg and "1024" in msg
        # exactly 1024 passes the size check; what then refuses this call is the host memory lig_ptr points to, which no kernel could read
        assert call([0, 3, 1027, 1030], 1030, 3) == -1
        msg = lib.cbgx_last_error().decode()
        assert "1024" not in msg and "lig_ptr" in msg
        # CSR entries are clamped to the array like in the kernels
        assert call([-5, 2000], 1000, 1) == -1 and "lig_ptr" in lib.cbgx_last_error().decode()
        assert call([-5, 2000], 1025, 1) == -1 and "1025" in lib.cbgx_last_error().decode()

"""Geometry report (cbgbench_amd/geometry.py, csrc/geometry.hip), host side: the library's constant tables and the numpy model
(tests/geometry_model.py) against the reference's own functions, ``summarise`` against hand-computed counts, and the C ABI of the two
entries without a device.  The kernel itself is compared with the model in tests/test_gpu_geometry.py."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from cbgbench_amd import _native, geometry as G
from tests import geometry_model as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
REF_GEOMETRY = os.path.join(REF, "repo", "tools", "geometry")
SYMBOLS = ("H", "C", "N", "O", "F", "P", "S", "Cl")


def _load(name, stand_ins=()):
    """a module of the reference's geometry tools by file path; ``stand_ins``: module names that get an empty throwaway module for the
    duration of the load (their contents are not used by the functions under test).  Skips when the tree or an import is missing."""
    path = os.path.join(REF_GEOMETRY, name + ".py")
    if not os.path.exists(path):
        pytest.skip("needs the reference tree at " + REF)
    saved = {}
    for full in stand_ins:
        parts = full.split(".")
        for k in range(1, len(parts) + 1):
            key = ".".join(parts[:k])
            if key in saved:
                continue
            saved[key] = sys.modules.get(key)
            mod = types.ModuleType(key)
            mod.__path__ = []
            sys.modules[key] = mod
    if "rdkit" in saved:
        sys.modules["rdkit"].Chem = types.ModuleType("rdkit.Chem")
    if "repo.datasets.parsers.protein_parser" in saved:
        sys.modules["repo.datasets.parsers.protein_parser"].PDBProteinFA = object
    try:
        spec = importlib.util.spec_from_file_location("_reference_" + name, path)
        mod = importlib.util.module_from_spec(spec)
        try:
            spec.loader.exec_module(mod)
        except ImportError as e:
            pytest.skip(f"the reference's {name}.py does not import here: {e}")
        return mod
    finally:
        for key, old in saved.items():
            if old is None:
                sys.modules.pop(key, None)
            else:
                sys.modules[key] = old


@pytest.fixture(scope="module")
def ref_stability():
    return _load("eval_stability")


@pytest.fixture(scope="module")
def ref_clash():
    return _load("eval_steric_clash", stand_ins=("rdkit", "repo.datasets.parsers.protein_parser"))


# ---- tables --------------------------------------------------------------------------------------------------------------------------
def test_tables_are_self_consistent():
    T = G.tables()
    assert T["elements"].tolist() == [1, 6, 7, 8, 9, 15, 16, 17]
    # the model (and the kernel) use one code space: the eight bond-table elements are the first eight radius codes
    assert T["vdw_z"][:8].tolist() == T["elements"].tolist() and T["vdw_z"][8] == 35
    assert T["bond_pm"].shape == (3, 8, 8)
    for o in range(3):
        assert np.array_equal(T["bond_pm"][o], T["bond_pm"][o].T)
    assert (T["bond_pm"][0] > 0).all() and T["tolerance"] == 0.4


def test_tables_equal_the_reference(ref_stability, ref_clash):
    T = G.tables()
    assert [ref_stability.atom_encoder[s] for s in SYMBOLS] == T["elements"].tolist()
    assert len(ref_stability.atom_encoder) == 8
    for o, ref in enumerate((ref_stability.bonds1, ref_stability.bonds2, ref_stability.bonds3)):
        assert sorted(ref) == sorted(SYMBOLS)
        for a, sa in enumerate(SYMBOLS):
            assert sorted(ref[sa]) == sorted(SYMBOLS)
            for b, sb in enumerate(SYMBOLS):
                assert T["bond_pm"][o, a, b] == ref[sa][sb], (o, sa, sb)
    assert T["margins"].tolist() == [ref_stability.margin1, ref_stability.margin2, ref_stability.margin3]
    assert T["allowed"].tolist() == [ref_stability.allowed_bonds[s] for s in SYMBOLS] and len(ref_stability.allowed_bonds) == 8
    assert dict(zip(T["vdw_z"].tolist(), T["vdw_r"].tolist())) == ref_clash.default_vdw_radii
    import inspect
    assert inspect.signature(ref_clash.detect_clash).parameters["tolerance"].default == T["tolerance"]


# ---- the model against the reference's functions -------------------------------------------------------------------------------------
SIZES = list(range(1, 41)) + list(range(42, 61, 2))      # 50 molecules of 1, 2, 3, ... 60 atoms


def molecules():
    """seeded chains with 0.7-1.6 A steps in random directions, float32 coordinates, elements over all eight; and a cloud of protein
    atoms (elements that have a radius) around each"""
    rng = np.random.default_rng(20240611)
    out = []
    for n in SIZES:
        step = rng.uniform(0.7, 1.6, size=(n, 1))
        u = rng.normal(size=(n, 3))
        x = np.cumsum(step * u / np.linalg.norm(u, axis=1, keepdims=True), axis=0).astype(np.float32)
        z = np.array([1, 6, 7, 8, 9, 15, 16, 17])[rng.choice(8, size=n, p=[.1, .4, .15, .15, .05, .05, .05, .05])]
        m = n + 2
        x_rec = (x[rng.integers(0, n, size=m)] + rng.normal(scale=3.0, size=(m, 3))).astype(np.float32)
        z_rec = np.array([1, 6, 7, 8, 16, 35])[rng.integers(0, 6, size=m)]
        out.append((x, z, x_rec, z_rec))
    return out


def test_model_equals_check_stability_and_detect_clash(ref_stability, ref_clash):
    orders, stable_seen, mol_seen, inter_seen = set(), set(), set(), set()
    for x, z, x_rec, z_rec in molecules():
        nr, flags, counts = GM.graph_geometry(x, z, x_rec, z_rec)
        mol_stable, n_stable, n_atoms, nr_ref = ref_stability.check_stability(x.astype(np.float64), z, hs=False, return_nr_bonds=True)
        assert np.array_equal(nr, nr_ref), (len(z), nr, nr_ref)
        assert counts[0] == n_atoms == len(z) and counts[1] == n_stable and bool(counts[2]) == bool(mol_stable)
        assert int(((flags & GM.STABLE) != 0).sum()) == n_stable
        _, info = ref_clash.detect_clash(x.astype(np.float64), x_rec.astype(np.float64), z, z_rec, pair_mask=None)
        clashed = np.flatnonzero(flags & GM.INTER)
        assert np.array_equal(clashed, np.unique(info["clashed_indices"])) and counts[3] == info["clash_atom_num"]
        assert counts[5] == 0 and not (flags & GM.UNKNOWN).any()
        orders |= set(np.unique(GM.bond_orders(x, z)[0]).tolist())
        stable_seen |= set(((flags & GM.STABLE) != 0).tolist())
        mol_seen.add(bool(counts[2]))
        inter_seen |= set(((flags & GM.INTER) != 0).tolist())
    # the cases reach every branch: all bond orders, stable and unstable atoms and molecules, clashing and free atoms
    assert orders == {0, 1, 2, 3} and stable_seen == {True, False} and mol_seen == {True, False} and inter_seen == {True, False}


def test_model_single_atom_and_empty():
    nr, flags, counts = GM.graph_geometry(np.zeros((1, 3), np.float32), [6], np.zeros((0, 3), np.float32), [])
    assert nr.tolist() == [0] and flags.tolist() == [0] and counts.tolist() == [1, 0, 0, 0, 0, 0]
    nr, flags, counts = GM.graph_geometry(np.zeros((0, 3), np.float32), [], np.zeros((2, 3), np.float32), [6, 34])
    assert nr.shape == (0,) and counts.tolist() == [0, 0, 0, 0, 0, 1]


# ---- summarise -----------------------------------------------------------------------------------------------------------------------
def test_summarise_against_hand_computed_counts():
    #      n_atoms n_stable mol_stable n_inter n_intra n_no_radius
    gc = [[10, 10, 1, 0, 0, 0],
          [20, 15, 0, 3, 2, 1],
          [1, 0, 0, 1, 0, 1],
          [9, 9, 1, 0, 4, 0]]
    s = G.summarise(gc)
    assert s["mol_stable"] == 2 / 4 and s["atm_stable"] == 34 / 40
    assert s["inter_clash_atom_ratio"] == 4 / 40 and s["intra_clash_atom_ratio"] == 6 / 40 and s["clash_mol_ratio"] == 2 / 4
    assert s["counts"] == {"n_mol": 4, "n_atoms": 40, "n_stable": 34, "n_mol_stable": 2, "n_inter_clash_atoms": 4,
                           "n_intra_clash_atoms": 6, "n_clash_mol": 2, "n_protein_atoms_without_radius": 2}
    assert set(s) == set(G.RATIOS) | {"counts"}
    # totals of two shards add up to the totals of the whole: what sample_cli sums over ranks
    whole = G.job_totals(gc)
    parts = [a + b for a, b in zip(G.job_totals(gc[:1]), G.job_totals(gc[1:]))]
    assert whole == parts and G.summarise_totals(parts) == s
    import torch
    assert G.summarise(torch.tensor(gc, dtype=torch.int32)) == s
    empty = G.summarise(np.zeros((0, 6), np.int32))
    assert empty["counts"]["n_mol"] == 0 and all(np.isnan(empty[k]) for k in G.RATIOS)


def test_cpu_tensors_raise():
    import torch
    x, z, b = torch.zeros(2, 3), torch.tensor([6, 6]), torch.zeros(2, dtype=torch.long)
    with pytest.raises(_native.NativeError):
        G.ligand_geometry(x, z, b, x, z, b, 1)


def test_csr_refuses_ungrouped_indices():
    import torch
    with pytest.raises(ValueError, match="not grouped"):
        G._csr(torch.tensor([0, 1, 0]), 2, "lig_batch")
    with pytest.raises(ValueError, match="outside"):
        G._csr(torch.tensor([0, 2]), 2, "lig_batch")
    assert G._csr(torch.tensor([0, 0, 2]), 4, "lig_batch").tolist() == [0, 2, 2, 3, 3]
    assert G._csr(torch.zeros(0, dtype=torch.long), 2, "lig_batch").tolist() == [0, 0, 0]


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("cbgx_ligand_geometry", "cbgx_ligand_geometry_tables")


def test_entries_are_declared_bound_and_exported():
    from cbgbench_amd.build import LIBPATH, XCHECK_LIBPATH, sources
    hdr = open(os.path.join(ROOT, "include", "cbgx.h")).read()
    lib = _native.lib()
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", hdr) and name in _native.EXPORTS and hasattr(lib, name)
    for path in (LIBPATH, XCHECK_LIBPATH):
        sym = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        for name in ENTRIES:
            assert f" {name}\n" in sym, (path, name)
    for xcheck in (False, True):
        names = [os.path.basename(s) for s in sources(xcheck)]
        assert "geometry.hip" in names and "api_geometry.hip" in names
    assert lib.cbgx_abi_version() == _native.ABI_VERSION == 6
    assert f"#define CBGX_GEOMETRY_MAX_LIGAND {G.MAX_LIGAND_ATOMS}" in hdr
    assert f"#define CBGX_GEOMETRY_GRAPH_COLS {len(G.GRAPH_COLUMNS)}" in hdr
    for name, bit in (("STABLE", G.STABLE), ("INTER_CLASH", G.INTER_CLASH), ("INTRA_CLASH", G.INTRA_CLASH),
                      ("UNKNOWN_ELEMENT", G.UNKNOWN_ELEMENT)):
        assert re.search(rf"#define CBGX_GEOM_{name} {bit}u\b", hdr)


def _call(lig_ptr, n_lig, B, x_lig="one", z_lig="one", x_rec="one", z_rec="one", rec_ptr="same", n_rec=4, nr_bonds="one",
          flags="one", graph_out="one"):
    """cbgx_ligand_geometry with a host lig_ptr; ``one``: a pointer that is never dereferenced (argument checks come first)"""
    one = ctypes.c_void_p(16)
    lp = np.asarray([] if lig_ptr is None else lig_ptr, np.int32)
    P = lambda a: one if isinstance(a, str) and a == "one" else a
    lptr = ctypes.c_void_p(lp.ctypes.data) if lig_ptr is not None else None
    rptr = lptr if isinstance(rec_ptr, str) else rec_ptr
    return _native.lib().cbgx_ligand_geometry(P(x_lig), P(z_lig), lptr, n_lig, P(x_rec), P(z_rec), rptr, n_rec, B, P(nr_bonds), P(flags),
                                              P(graph_out), None)


def test_argument_errors_are_returned_without_a_gpu():
    lib = _native.lib()
    ok_ptr = [0, 2, 4]
    bad = [_call(ok_ptr, 4, -1), _call(ok_ptr, -1, 2), _call(ok_ptr, 4, 2, n_rec=-1), _call(None, 4, 2), _call(ok_ptr, 4, 2, rec_ptr=None),
           _call(ok_ptr, 4, 2, x_lig=None), _call(ok_ptr, 4, 2, z_lig=None), _call(ok_ptr, 4, 2, x_rec=None), _call(ok_ptr, 4, 2, z_rec=None),
           _call(ok_ptr, 4, 2, nr_bonds=None), _call(ok_ptr, 4, 2, flags=None), _call(ok_ptr, 4, 2, graph_out=None)]
    assert bad == [-1] * len(bad), bad
    assert _call(ok_ptr, 4, 2, flags=None) == -1 and b"NULL" in lib.cbgx_last_error()
    assert _call(ok_ptr, -1, 2) == -1 and b"negative" in lib.cbgx_last_error()
    # a NULL array that has no elements is fine: no ligand atoms, no protein atoms, no graphs -> nothing to do, no launch, no error
    assert _call(None, 0, 0, x_lig=None, z_lig=None, x_rec=None, z_rec=None, rec_ptr=None, n_rec=0, nr_bonds=None, flags=None,
                 graph_out=None) == 0
    assert _call(None, 7, 0, rec_ptr=None, graph_out=None) == 0


def test_a_ligand_above_1024_atoms_is_refused():
    lib = _native.lib()
    assert _call([0, 3, 1028, 1030], 1030, 3) == -1
    msg = lib.cbgx_last_error().decode()
    assert "graph 1" in msg and "1025" in msg and "1024" in msg
    # exactly 1024 passes the size check; what then refuses this call is the host memory lig_ptr points to, which no kernel could read
    assert _call([0, 3, 1027, 1030], 1030, 3) == -1
    msg = lib.cbgx_last_error().decode()
    assert "1024" not in msg and "lig_ptr" in msg
    # CSR entries are clamped to the array like in the kernel: [-5, 2000) over 1000 atoms is a 1000-atom ligand
    assert _call([-5, 2000], 1000, 1) == -1 and "lig_ptr" in lib.cbgx_last_error().decode()
    assert _call([-5, 2000], 1025, 1) == -1 and "1025" in lib.cbgx_last_error().decode()


# ---- job totals over ranks -----------------------------------------------------------------------------------------------------------
SUM_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
import torch.distributed as dist
from cbgbench_amd import geometry, sharding
rank, world, local = sharding.init_process_group("gloo")
mine = [[10, 10, 1, 0, 0, 0], [20, 15, 0, 3, 2, 1]] if rank == 0 else [[1, 0, 0, 1, 0, 1], [9, 9, 1, 0, 4, 0]]
total = sharding.sum_counts(geometry.job_totals(mine))
if rank == 0:
    print("TOTAL", total, flush=True)
dist.destroy_process_group()
"""


def test_sum_counts_adds_the_ranks_totals(tmp_path):
    """two gloo ranks, each with half of the molecules of test_summarise_against_hand_computed_counts: every rank gets the whole job's
    integer totals; without a process group the helper returns its input"""
    from cbgbench_amd import sharding
    assert sharding.sum_counts([3, 0, 7]) == [3, 0, 7]
    script = tmp_path / "sum_script.py"
    script.write_text(SUM_SCRIPT.format(root=ROOT))
    env = dict(os.environ)
    for k in ("MASTER_ADDR", "MASTER_PORT", "CBGX_RDZV_FILE", "RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "cbgbench_amd.launch", "--nproc", "2", str(script)], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "TOTAL [4, 40, 34, 2, 4, 6, 2, 2]" in p.stdout

"""Geometry report of sampled ligands, on the device the samples live on: atom / molecule stability and protein-ligand steric clash,
the two metrics of the reference's quality path (``evaluate_scripts/evaluate_geom_single.py``) that need coordinates and elements only --
``check_stability(..., hs=False)`` of ``repo/tools/geometry/eval_stability.py`` and ``detect_clash`` of
``repo/tools/geometry/eval_steric_clash.py`` -- as ONE libcbgx launch per batch (``cbgx_ligand_geometry``, csrc/geometry.hip; the
definition is in include/cbgx.h).  No RDKit, no OpenBabel.

Two stated deviations from the reference:
  * intra-ligand clashes exclude the pairs that have a TABLE bond (the bond order the stability metric derives from the distance); the
    reference excludes RDKit's bond adjacency.  Hence the names ``intra_clash_table_bonds`` / ``n_intra_clash_atoms``.
  * a protein atom whose element has no van der Waals radius (Se) takes no part in the clash test and is counted
    (``n_protein_atoms_without_radius``); the reference raises ``KeyError``.

The constants (bond lengths, margins, valences, radii, tolerance) live in the kernel's translation unit; ``tables()`` reads them from the
library.

``ligand_bonds`` / ``batch_bonds`` / ``summarise_bonds`` keep what the stability metric throws away: the TABLE-bond graph itself -- the bond
list in (i, j) order with orders and float64 lengths, the connected components (``fragment``) and six integer facts per molecule
(BOND_GRAPH_COLUMNS) -- in two launches with a prefix sum between (``cbgx_ligand_bonds_count`` / ``cbgx_ligand_bonds_fill``).  These are
table bonds, not RDKit's: no aromaticity, no valence repair.  A molecule is ``connected`` iff it has one fragment: the table-bond
counterpart of the reference's ``'.' not in smiles`` (repo/tools/rdkit_utils.py:597-640).

``ligand_rings`` / ``batch_rings`` / ``summarise_rings`` answer what rings that graph holds: the number of rings of every size 3 ... 9 in a
minimum cycle basis, the rings above 9, and the shortest ring through every atom, in one launch on the bond list (``cbgx_ligand_rings``,
csrc/rings.hip) -- the RDKit-free counterpart of the ring statistics of ``evaluate_geom_single.py:27-33`` (``print_ring_ratio``) and
``repo/tools/eval_ring_type.py``, which read the sizes of RDKit's ``AtomRings()``.  Deviations: table bonds; RDKit's SSSR is a heuristic
that can differ from a minimum cycle basis on cage-like graphs."""
import ctypes

import numpy as np
import torch

from . import _native
from .config import _ATOMIC_NUMBER

MAX_LIGAND_ATOMS = 1024       # include/cbgx.h CBGX_GEOMETRY_MAX_LIGAND
# flags bits (include/cbgx.h CBGX_GEOM_*)
STABLE, INTER_CLASH, INTRA_CLASH, UNKNOWN_ELEMENT = 1, 2, 4, 8
# columns of graph_counts (include/cbgx.h)
GRAPH_COLUMNS = ("n_atoms", "n_stable", "mol_stable", "n_inter_clash_atoms", "n_intra_clash_atoms", "n_protein_atoms_without_radius")
# columns of ligand_bonds' graph_counts (include/cbgx.h CBGX_BONDS_GRAPH_COLS)
BOND_GRAPH_COLUMNS = ("n_atoms", "n_bonds", "bond_order_sum", "n_fragments", "largest_fragment", "n_cycles")


def tables():
    """the constants the library's kernel was built with (``cbgx_ligand_geometry_tables``; host only): ``bond_pm`` [3, 8, 8] int32
    (order - 1, element code, element code; -1: no such bond), ``margins`` [3] pm, ``allowed`` [8] valences, ``elements`` [8] atomic
    numbers of the element codes, ``vdw_z`` [9] / ``vdw_r`` [9] atomic numbers with a radius and the radii, ``tolerance``"""
    out = {"bond_pm": np.zeros((3, 8, 8), np.int32), "margins": np.zeros(3, np.int32), "allowed": np.zeros(8, np.int32),
           "elements": np.zeros(8, np.uint8), "vdw_z": np.zeros(9, np.uint8), "vdw_r": np.zeros(9, np.float64),
           "tolerance": np.zeros(1, np.float64)}
    _native.check(_native.lib().cbgx_ligand_geometry_tables(*[ctypes.c_void_p(a.ctypes.data) for a in out.values()]),
                  "cbgx_ligand_geometry_tables")
    out["tolerance"] = float(out["tolerance"][0])
    return out


def _csr(index, n_graphs, what):
    """[B + 1] int32 CSR of a graph-index vector that must be grouped by graph (ascending: the collated layout)"""
    index = index.to(torch.long)
    if index.numel():
        if bool((index[1:] < index[:-1]).any()):
            raise ValueError(f"{what} is not grouped by graph (graph indices must not decrease)")
        if int(index[0]) < 0 or int(index[-1]) >= n_graphs:
            raise ValueError(f"{what} holds graph indices outside [0, {n_graphs})")
    counts = torch.bincount(index, minlength=n_graphs)
    return torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32).contiguous()


def ligand_geometry(x_lig, z_lig, lig_batch, x_rec, z_rec, rec_batch, n_graphs):
    """Stability and clash report of ``n_graphs`` ligands in their pockets, one launch on the tensors' current stream.

    ``x_lig`` [n_lig, 3] / ``x_rec`` [n_rec, 3] coordinates (evaluated as float32), ``z_lig`` / ``z_rec`` atomic numbers, ``lig_batch`` /
    ``rec_batch`` the graph index of every atom, grouped by graph.  Returns device tensors: ``nr_bonds`` [n_lig] int32, ``flags`` [n_lig]
    uint8 (STABLE, INTER_CLASH, INTRA_CLASH -- against ligand atoms without a TABLE bond, not RDKit's bonds --, UNKNOWN_ELEMENT) and
    ``graph_counts`` [n_graphs, 6] int32 (GRAPH_COLUMNS).  A ligand of more than MAX_LIGAND_ATOMS atoms raises ValueError.  There is no CPU
    path."""
    dev = x_lig.device
    if dev.type != "cuda":
        raise _native.NativeError("ligand_geometry runs on the GPU (cbgx_ligand_geometry): there is no CPU fallback")
    n_graphs = int(n_graphs)
    for name, t in (("z_lig", z_lig), ("lig_batch", lig_batch), ("x_rec", x_rec), ("z_rec", z_rec), ("rec_batch", rec_batch)):
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, x_lig on {dev}")
    n_lig, n_rec = int(x_lig.shape[0]), int(x_rec.shape[0])
    if tuple(x_lig.shape) != (n_lig, 3) or tuple(x_rec.shape) != (n_rec, 3):
        raise ValueError("coordinates must be [n, 3]")
    if z_lig.shape != (n_lig,) or lig_batch.shape != (n_lig,) or z_rec.shape != (n_rec,) or rec_batch.shape != (n_rec,):
        raise ValueError("one atomic number and one graph index per atom")
    lig_ptr, rec_ptr = _csr(lig_batch, n_graphs, "lig_batch"), _csr(rec_batch, n_graphs, "rec_batch")
    x_lig, x_rec = x_lig.to(torch.float32).contiguous(), x_rec.to(torch.float32).contiguous()
    # atomic numbers as bytes; anything outside a byte is no element the tables know: 0
    as_z = lambda z: torch.where((z >= 0) & (z <= 255), z, torch.zeros_like(z)).to(torch.uint8).contiguous()
    z_lig, z_rec = as_z(z_lig), as_z(z_rec)
    nr_bonds = torch.empty(n_lig, dtype=torch.int32, device=dev)
    flags = torch.empty(n_lig, dtype=torch.uint8, device=dev)
    graph_counts = torch.empty(n_graphs, len(GRAPH_COLUMNS), dtype=torch.int32, device=dev)
    p = _native.ptr
    _native.check(_native.lib().cbgx_ligand_geometry(p(x_lig), p(z_lig), p(lig_ptr), n_lig, p(x_rec), p(z_rec), p(rec_ptr), n_rec, n_graphs,
                                                     p(nr_bonds), p(flags), p(graph_counts), _native.current_stream(dev)),
                  "cbgx_ligand_geometry")
    return {"nr_bonds": nr_bonds, "flags": flags, "graph_counts": graph_counts}


def batch_geometry(batch, x, c, lig_batch, mode):
    """``ligand_geometry`` of a sampling state (``x`` [n_lig, 3], ``c`` type indices [n_lig] or scores [n_lig, C]: argmax, ``lig_batch``)
    against the batch's own pocket (``protein_pos``, ``protein_element``, ``protein_element_batch``), in the frame both share.  ``mode``:
    the atom-type vocabulary ('basic' / 'add_aromatic') that maps a type index to its atomic number."""
    if mode not in _ATOMIC_NUMBER:
        raise ValueError(mode)
    typ = c.argmax(-1) if c.dim() == 2 else c
    z = torch.tensor(_ATOMIC_NUMBER[mode], dtype=torch.long, device=x.device)[typ.to(torch.long)]
    n_graphs = int(batch["num_graphs"]) if "num_graphs" in batch else int(max(
        int(lig_batch.max()) if lig_batch.numel() else -1,
        int(batch["protein_element_batch"].max()) if batch["protein_element_batch"].numel() else -1)) + 1
    return ligand_geometry(x, z, lig_batch, batch["protein_pos"], batch["protein_element"], batch["protein_element_batch"], n_graphs)


# the job's integer totals: what ranks add up, and what the ratios are taken from
COUNT_KEYS = ("n_mol", "n_atoms", "n_stable", "n_mol_stable", "n_inter_clash_atoms", "n_intra_clash_atoms", "n_clash_mol",
              "n_protein_atoms_without_radius")
RATIOS = ("mol_stable", "atm_stable", "inter_clash_atom_ratio", "intra_clash_atom_ratio", "clash_mol_ratio")


def job_totals(graph_counts):
    """per-molecule counts ``graph_counts`` [n_mol, 6] (GRAPH_COLUMNS; any array-like) -> the integer totals, in COUNT_KEYS order"""
    if isinstance(graph_counts, torch.Tensor):
        graph_counts = graph_counts.cpu().numpy()
    gc = np.asarray(graph_counts, dtype=np.int64).reshape(-1, len(GRAPH_COLUMNS))
    n_atoms, n_stable, n_mol_stable, n_inter, n_intra, n_norad = (int(v) for v in gc.sum(0))
    return [int(gc.shape[0]), n_atoms, n_stable, n_mol_stable, n_inter, n_intra, int((gc[:, 3] > 0).sum()), n_norad]


def summarise_totals(totals):
    """the five ratios (RATIOS) of integer totals in COUNT_KEYS order, and the totals as ``counts``; a ratio over nothing is nan"""
    c = {k: int(v) for k, v in zip(COUNT_KEYS, totals)}
    ratio = lambda a, b: a / b if b else float("nan")
    return {"mol_stable": ratio(c["n_mol_stable"], c["n_mol"]), "atm_stable": ratio(c["n_stable"], c["n_atoms"]),
            "inter_clash_atom_ratio": ratio(c["n_inter_clash_atoms"], c["n_atoms"]),
            "intra_clash_atom_ratio": ratio(c["n_intra_clash_atoms"], c["n_atoms"]),
            "clash_mol_ratio": ratio(c["n_clash_mol"], c["n_mol"]), "counts": c}


def summarise(graph_counts):
    """The five numbers of evaluate_geom_single.py:126-130 from integer per-molecule counts (``graph_counts`` [n_mol, 6], GRAPH_COLUMNS;
    any array-like), plus the counts themselves (``counts``, COUNT_KEYS): mol_stable = sum(mol_stable) / n_mol, atm_stable =
    sum(n_stable) / sum(n_atoms), inter_clash_atom_ratio = sum(n_inter_clash_atoms) / sum(n_atoms), intra_clash_atom_ratio =
    sum(n_intra_clash_atoms) / sum(n_atoms) (intra-ligand pairs without a TABLE bond), clash_mol_ratio = share of molecules with at least
    one inter-clash atom."""
    return summarise_totals(job_totals(graph_counts))


# ---- the table-bond graph: bond list, fragments, connectivity ------------------------------------------------------------------------
def ligand_bonds(x_lig, z_lig, lig_batch, n_graphs):
    """The table bonds of ``n_graphs`` ligands and what follows from them, on the tensors' current stream: two launches
    (``cbgx_ligand_bonds_count``, ``cbgx_ligand_bonds_fill``) with a ``torch.cumsum`` between, whose last element is read on the host to
    size the list.

    Arguments as ``ligand_geometry``'s ligand side.  Returns device tensors: ``bond_index`` [2, n_bonds] int32 global ligand rows with
    i < j, in strict (i, j) order; ``bond_order`` [n_bonds] uint8 in 1..3; ``bond_length`` [n_bonds] float64, the distance the order was
    decided on, in Angstrom; ``bond_graph`` [n_bonds] int64, the graph of every bond; ``fragment`` [n_lig] int32, the smallest
    ligand-LOCAL index of the atom's connected component; ``graph_counts`` [n_graphs, 6] int32 (BOND_GRAPH_COLUMNS).  A ligand of more
    than MAX_LIGAND_ATOMS atoms raises ValueError.  There is no CPU path."""
    dev = x_lig.device
    if dev.type != "cuda":
        raise _native.NativeError("ligand_bonds runs on the GPU (cbgx_ligand_bonds_count / _fill): there is no CPU fallback")
    n_graphs = int(n_graphs)
    for name, t in (("z_lig", z_lig), ("lig_batch", lig_batch)):
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, x_lig on {dev}")
    n_lig = int(x_lig.shape[0])
    if tuple(x_lig.shape) != (n_lig, 3):
        raise ValueError("coordinates must be [n, 3]")
    if z_lig.shape != (n_lig,) or lig_batch.shape != (n_lig,):
        raise ValueError("one atomic number and one graph index per atom")
    lig_ptr = _csr(lig_batch, n_graphs, "lig_batch")
    x_lig = x_lig.to(torch.float32).contiguous()
    z_lig = torch.where((z_lig >= 0) & (z_lig <= 255), z_lig, torch.zeros_like(z_lig)).to(torch.uint8).contiguous()
    deg_up = torch.empty(n_lig, dtype=torch.int32, device=dev)
    fragment = torch.empty(n_lig, dtype=torch.int32, device=dev)
    graph_counts = torch.empty(n_graphs, len(BOND_GRAPH_COLUMNS), dtype=torch.int32, device=dev)
    p, lib, stream = _native.ptr, _native.lib(), _native.current_stream(dev)
    _native.check(lib.cbgx_ligand_bonds_count(p(x_lig), p(z_lig), p(lig_ptr), n_lig, n_graphs, p(deg_up), p(fragment), p(graph_counts),
                                              stream), "cbgx_ligand_bonds_count")
    ends = deg_up.cumsum(0, dtype=torch.int64)
    n_bonds = int(ends[-1]) if n_lig else 0
    if n_bonds > 2 ** 31 - 1:
        raise ValueError(f"{n_bonds} bonds in one batch: more than an int32 bond_ptr addresses")
    bond_ptr = torch.cat([ends.new_zeros(1), ends]).to(torch.int32).contiguous()
    bond_index = torch.empty(2, n_bonds, dtype=torch.int32, device=dev)
    bond_order = torch.empty(n_bonds, dtype=torch.uint8, device=dev)
    bond_length = torch.empty(n_bonds, dtype=torch.float64, device=dev)
    _native.check(lib.cbgx_ligand_bonds_fill(p(x_lig), p(z_lig), p(lig_ptr), n_lig, n_graphs, p(bond_ptr), n_bonds, p(bond_index),
                                             p(bond_order), p(bond_length), stream), "cbgx_ligand_bonds_fill")
    bond_graph = lig_batch.to(torch.long)[bond_index[0].to(torch.long)]
    return {"bond_index": bond_index, "bond_order": bond_order, "bond_length": bond_length, "bond_graph": bond_graph,
            "fragment": fragment, "graph_counts": graph_counts}


def batch_bonds(batch, x, c, lig_batch, mode):
    """``ligand_bonds`` of a sampling state (``x`` [n_lig, 3], ``c`` type indices [n_lig] or scores [n_lig, C]: argmax, ``lig_batch``);
    ``batch`` gives ``num_graphs`` when it has it.  ``mode``: the atom-type vocabulary that maps a type index to its atomic number."""
    if mode not in _ATOMIC_NUMBER:
        raise ValueError(mode)
    typ = c.argmax(-1) if c.dim() == 2 else c
    z = torch.tensor(_ATOMIC_NUMBER[mode], dtype=torch.long, device=x.device)[typ.to(torch.long)]
    n_graphs = int(batch["num_graphs"]) if "num_graphs" in batch else (int(lig_batch.max()) + 1 if lig_batch.numel() else 0)
    return ligand_bonds(x, z, lig_batch, n_graphs)


BOND_COUNT_KEYS = ("n_mol", "n_atoms", "n_bonds", "n_connected_mol", "n_largest_fragment_atoms", "n_fragments", "n_cycles")
BOND_RATIOS = ("connected_mol_ratio", "largest_fragment_atom_ratio", "fragments_per_mol", "cycles_per_mol", "bonds_per_atom")


def bond_totals(graph_counts):
    """per-molecule counts ``graph_counts`` [n_mol, 6] (BOND_GRAPH_COLUMNS; any array-like) -> the integer totals, in BOND_COUNT_KEYS
    order; a molecule is connected iff n_fragments == 1"""
    if isinstance(graph_counts, torch.Tensor):
        graph_counts = graph_counts.cpu().numpy()
    gc = np.asarray(graph_counts, dtype=np.int64).reshape(-1, len(BOND_GRAPH_COLUMNS))
    n_atoms, n_bonds, _, n_frag, n_largest, n_cycles = (int(v) for v in gc.sum(0))
    return [int(gc.shape[0]), n_atoms, n_bonds, int((gc[:, 3] == 1).sum()), n_largest, n_frag, n_cycles]


def summarise_bond_totals(totals):
    """the five ratios (BOND_RATIOS) of integer totals in BOND_COUNT_KEYS order, and the totals as ``counts``; a ratio over nothing is nan"""
    c = {k: int(v) for k, v in zip(BOND_COUNT_KEYS, totals)}
    ratio = lambda a, b: a / b if b else float("nan")
    return {"connected_mol_ratio": ratio(c["n_connected_mol"], c["n_mol"]),
            "largest_fragment_atom_ratio": ratio(c["n_largest_fragment_atoms"], c["n_atoms"]),
            "fragments_per_mol": ratio(c["n_fragments"], c["n_mol"]), "cycles_per_mol": ratio(c["n_cycles"], c["n_mol"]),
            "bonds_per_atom": ratio(c["n_bonds"], c["n_atoms"]), "counts": c}


def summarise_bonds(graph_counts):
    """connectivity of a set of molecules from integer per-molecule counts (``graph_counts`` [n_mol, 6], BOND_GRAPH_COLUMNS): the share of
    connected molecules (one fragment: the table-bond counterpart of the reference's ``'.' not in smiles``), the share of atoms in their
    molecule's largest fragment (what ``clean_frags`` would keep), fragments and cycles per molecule, bonds per atom; plus ``counts``"""
    return summarise_bond_totals(bond_totals(graph_counts))


# ---- ring sizes of the table-bond graph ----------------------------------------------------------------------------------------------
MAX_RING_SIZE, MAX_RING_ATOMS, MAX_RING_CYCLES = 9, 256, 128      # include/cbgx.h CBGX_RINGS_MAX_SIZE / _MAX_ATOMS / _MAX_CYCLES
RING_SIZES = range(3, MAX_RING_SIZE + 1)
# columns of ligand_rings' graph_counts (include/cbgx.h CBGX_RINGS_GRAPH_COLS)
RING_GRAPH_COLUMNS = (("n_atoms", "n_bonds", "n_cycles") + tuple(f"rings_{k}" for k in RING_SIZES)
                      + ("n_rings_larger", "n_ring_atoms", "status"))
# status bits (include/cbgx.h CBGX_RINGS_*): a graph with status != 0 was not evaluated
RINGS_TOO_MANY_ATOMS, RINGS_TOO_MANY_CYCLES, RINGS_BAD_BONDS = 1, 2, 4


def ligand_rings(bond_index, lig_batch, n_graphs):
    """Ring sizes of the bond graphs of ``n_graphs`` ligands, one launch (``cbgx_ligand_rings``, csrc/rings.hip; the definition is in
    include/cbgx.h) on the tensors' current stream.

    ``bond_index`` [2, n_bonds]: what ``ligand_bonds`` returns (global ligand rows, i < j, in (i, j) order); ``lig_batch`` [n_lig] the
    graph index of every atom, grouped by graph.  Returns device tensors: ``atom_ring_min`` [n_lig] uint8, the length of the shortest
    cycle through the atom (0: none of length <= 9), and ``graph_counts`` [n_graphs, 13] int32 (RING_GRAPH_COLUMNS): rings_k = the number
    of cycles of length k in a minimum cycle basis, n_rings_larger = n_cycles - sum_k rings_k, n_ring_atoms, status.  A graph of more than
    MAX_RING_ATOMS atoms, of more than MAX_RING_CYCLES independent cycles, or whose bonds are not such a list, is not an error: its status
    is non-zero (RINGS_*), its columns from n_cycles to n_ring_atoms are -1 and its atoms' ``atom_ring_min`` 255.  There is no CPU
    path."""
    dev = bond_index.device
    if dev.type != "cuda":
        raise _native.NativeError("ligand_rings runs on the GPU (cbgx_ligand_rings): there is no CPU fallback")
    n_graphs = int(n_graphs)
    if lig_batch.device != dev:
        raise ValueError(f"lig_batch is on {lig_batch.device}, bond_index on {dev}")
    if bond_index.dim() != 2 or bond_index.shape[0] != 2:
        raise ValueError("bond_index must be [2, n_bonds]")
    n_lig, n_bonds = int(lig_batch.shape[0]), int(bond_index.shape[1])
    if lig_batch.shape != (n_lig,):
        raise ValueError("one graph index per atom")
    lig_ptr = _csr(lig_batch, n_graphs, "lig_batch")
    bond_index = bond_index.to(torch.int32).contiguous()
    # bond_ptr as the bond entries define it: the bonds are sorted by their first atom, a is the first atom of bond_ptr[a] ... bond_ptr[a + 1]
    first = bond_index[0].to(torch.long).clamp(0, max(n_lig - 1, 0))
    counts = torch.bincount(first, minlength=n_lig) if n_lig else first.new_zeros(0)
    bond_ptr = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32).contiguous()
    atom_ring_min = torch.empty(n_lig, dtype=torch.uint8, device=dev)
    graph_counts = torch.empty(n_graphs, len(RING_GRAPH_COLUMNS), dtype=torch.int32, device=dev)
    p = _native.ptr
    _native.check(_native.lib().cbgx_ligand_rings(p(lig_ptr), n_lig, n_graphs, p(bond_ptr), p(bond_index) if n_bonds else None, n_bonds,
                                                  p(atom_ring_min), p(graph_counts), _native.current_stream(dev)), "cbgx_ligand_rings")
    return {"atom_ring_min": atom_ring_min, "graph_counts": graph_counts}


def batch_rings(batch, x, c, lig_batch, mode, bonds=None):
    """``ligand_rings`` of a sampling state; ``bonds``: what ``batch_bonds`` returned for the same state (it is called here when None)"""
    if bonds is None:
        bonds = batch_bonds(batch, x, c, lig_batch, mode)
    return ligand_rings(bonds["bond_index"], lig_batch.to(bonds["bond_index"].device), bonds["graph_counts"].shape[0])


RING_COUNT_KEYS = (("n_mol", "n_mol_evaluated", "n_mol_over_limit", "n_atoms", "n_ring_atoms", "n_rings")
                   + tuple(f"n_rings_{k}" for k in RING_SIZES) + ("n_rings_larger",)
                   + tuple(f"n_mol_with_ring_{k}" for k in RING_SIZES) + ("n_mol_with_larger_ring",))
RING_RATIOS = (tuple(f"ring_mol_ratio_{k}" for k in RING_SIZES) + tuple(f"rings_per_mol_{k}" for k in range(3, 9))
               + tuple(f"ring_size_distribution_{k}" for k in range(3, 9)) + ("macrocycle_mol_ratio", "ring_atom_ratio"))


def ring_totals(graph_counts):
    """per-molecule counts ``graph_counts`` [n_mol, 13] (RING_GRAPH_COLUMNS; any array-like) -> the integer totals, in RING_COUNT_KEYS
    order.  Everything but n_mol and n_mol_over_limit is summed over the evaluated molecules (status == 0) only; n_rings = n_cycles"""
    if isinstance(graph_counts, torch.Tensor):
        graph_counts = graph_counts.cpu().numpy()
    gc = np.asarray(graph_counts, dtype=np.int64).reshape(-1, len(RING_GRAPH_COLUMNS))
    ok = gc[gc[:, -1] == 0]
    sizes = ok[:, 3:3 + len(RING_SIZES) + 1]                    # rings_3 ... rings_9, n_rings_larger
    return ([int(gc.shape[0]), int(ok.shape[0]), int(gc.shape[0] - ok.shape[0]), int(ok[:, 0].sum()), int(ok[:, -2].sum()),
             int(ok[:, 2].sum())] + [int(v) for v in sizes.sum(0)] + [int(v) for v in (sizes > 0).sum(0)])


def summarise_ring_totals(totals):
    """the ratios (RING_RATIOS) of integer totals in RING_COUNT_KEYS order, and the totals as ``counts``.  Every ratio is over the EVALUATED
    molecules (n_mol_evaluated: status == 0) -- a molecule over a limit is counted in n_mol and n_mol_over_limit and nowhere else; a
    ratio over nothing is nan.  ring_mol_ratio_k, k = 3 ... 9: the share of molecules with at least one ring of size k
    (evaluate_geom_single.py:27-33, print_ring_ratio); rings_per_mol_k, k = 3 ... 8: rings of size k per molecule (eval_ring_type.py,
    eval_ring_type_ratio); ring_size_distribution_k, k = 3 ... 8: the share of size k among the rings of those six sizes
    (eval_ring_type_distribution); macrocycle_mol_ratio: the share of molecules with a ring above 9; ring_atom_ratio: ring atoms / atoms"""
    c = {k: int(v) for k, v in zip(RING_COUNT_KEYS, totals)}
    ratio = lambda a, b: a / b if b else float("nan")
    n_mol = c["n_mol_evaluated"]
    in_six = sum(c[f"n_rings_{k}"] for k in range(3, 9))
    out = {f"ring_mol_ratio_{k}": ratio(c[f"n_mol_with_ring_{k}"], n_mol) for k in RING_SIZES}
    out.update({f"rings_per_mol_{k}": ratio(c[f"n_rings_{k}"], n_mol) for k in range(3, 9)})
    out.update({f"ring_size_distribution_{k}": ratio(c[f"n_rings_{k}"], in_six) for k in range(3, 9)})
    out["macrocycle_mol_ratio"] = ratio(c["n_mol_with_larger_ring"], n_mol)
    out["ring_atom_ratio"] = ratio(c["n_ring_atoms"], c["n_atoms"])
    out["counts"] = c
    return out


def summarise_rings(graph_counts):
    """ring statistics of a set of molecules from integer per-molecule counts (``graph_counts`` [n_mol, 13], RING_GRAPH_COLUMNS): see
    ``summarise_ring_totals``; ratios are over the evaluated molecules only"""
    return summarise_ring_totals(ring_totals(graph_counts))


def ring_jsd(distribution, reference):
    """Jensen-Shannon distance (the square root of the divergence, natural logarithm: ``scipy.spatial.distance.jensenshannon``) of two
    ring-size distributions over the sizes 3 ... 8, e.g. ``ring_size_distribution_k`` of a job against a dataset's.  Both are normalised
    to sum 1 first; the reference's numbers are the caller's own: none ship with this package"""
    p, q = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (distribution, reference))
    if p.shape != (6,) or q.shape != (6,):
        raise ValueError("ring_jsd takes two vectors over the six ring sizes 3 ... 8")
    p, q = p / p.sum(), q / q.sum()
    mid = 0.5 * (p + q)
    kl = lambda a, b: float(np.sum(np.where(a > 0, a * np.log(np.where(a > 0, a, 1.0) / np.where(a > 0, b, 1.0)), 0.0)))
    return float(np.sqrt(max(0.5 * (kl(p, mid) + kl(q, mid)), 0.0)))

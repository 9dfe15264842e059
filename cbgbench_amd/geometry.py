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
that can differ from a minimum cycle basis on cage-like graphs.

``ligand_aromatic`` / ``batch_aromatic`` / ``summarise_aromatic`` add the aromatic bond type the table bonds lack: the closure of the
model's per-atom aromatic flags ('add_aromatic' atom types) under the two rules of the reference's ``reconstruct_mol``
(repo/tools/rdkit_utils.py:380-389, 552-572) over the chordless 5- and 6-cycles of the graph, in one launch on the bond list and the ring
report (``cbgx_ligand_aromatic``, csrc/aromatic.hip); a bond is aromatic (``bond_type`` 4) as an edge of a cycle inside the closure.
Deviations: the rules run to their fixed point (the reference applies each once); the link of biphenyl is not aromatic.  Handed to
``batch_distributions(..., aromatic=)`` it re-keys the bond-length and bond-angle histograms by four bond types (``n_orders=4``).
``sdf_record`` writes a sample as a V2000 record on the host.

``ligand_valence`` / ``batch_valence`` / ``summarise_valence`` ask whether the sample is a molecule at all: Kekule orders for the aromatic
bonds (per aromatic system the largest, lexicographically least set of double bonds that covers every carbon able to take one), implicit
hydrogens and a valence check per atom against this library's own table, in one launch on the bond list and the aromatic report
(``cbgx_ligand_valence``, csrc/valence.hip) -- the RDKit-free counterpart of kekulisation, ``evaluate_validity`` and the hydrogen counts
behind ``evaluate_chem_*`` (repo/tools/rdkit_utils.py:522-640) and ``repo/tools/eval_atom_type.py``.  Deviations: table bonds and a
property-defined Kekule choice; no charges.  ``formula`` / ``mol_weight`` are host helpers on the element counts.

``pocket_types`` / ``ligand_interactions`` / ``batch_interactions`` / ``summarise_interactions`` ask how the sample sits in its pocket:
donor / acceptor / hydrophobic types of both sides (the pocket's from a residue table, the ligand's from the bond list and the valence
report), rotatable bonds, and the five pair terms of the published Vina scoring function (Trott & Olson 2010) summed in a fixed order, in
two launches (``cbgx_pocket_types`` / ``cbgx_ligand_interactions``, csrc/interactions.hip) -- where the reference runs
``vina_task.run(mode='score_only')`` (evaluate_scripts/evaluate_chem_single.py:44-49) and PLIP (repo/tools/interaction.py).  A score in
Vina's functional form on this library's own atom typing: NOT the Vina program, not validated against it.  Deviations: table bonds, no
hydrogens or protonation states in the pocket, an acceptor rule of our own for N, no intramolecular term, no metals, no Br / I,
non-strict rotatable bonds.

``ligand_groups`` / ``batch_groups`` / ``summarise_groups`` / ``groups_against`` are the functional-group numbers of the reference's
substructure block (evaluate_scripts/evaluate_substruct_single.py; ``EFGs.mol2frag`` behind repo/tools/eval_fg_type.py): members by
marking rules, groups as connected components under the group bonds, and each group's class by an exact isomorphism test against the 25
template graphs of GROUP_NAMES, in one launch on the bond list and the aromatic report (``cbgx_ligand_groups``, csrc/groups.hip).
Deviations: table bonds and this library's aromatic bonds; marking rules of our own, not the EFGs program; no charges; a single-atom
group is 'other'.  ``groups_against`` takes the caller's own reference ratios and distribution: no dataset constants ship.

``ligand_fingerprints`` / ``group_diversity`` / ``batch_diversity`` / ``summarise_diversity`` are the first numbers ACROSS the samples of
a pocket: the share of distinct molecules and one minus the mean pairwise Tanimoto similarity, where the reference has
``tanimoto_sim`` on ``Chem.RDKFingerprint`` (repo/tools/similarity.py) and SMILES strings behind RDKit reconstruction.  A 1024-bit
fingerprint and a 64-bit hash per graph by colour refinement over the typed bonds from (element, degree, aromatic, smallest ring), then
one workgroup per pocket for the pairs (``cbgx_ligand_fingerprints`` / ``cbgx_group_diversity``, csrc/diversity.hip).  Integer work only.
Deviations: table bonds and this library's aromatic bonds; a fingerprint of our own in the manner of ECFP4, neither RDKit's Morgan
fingerprint nor ``RDKFingerprint``; equal hashes mean equivalence under the refinement, not isomorphism.  ``tanimoto_micro`` is the host
helper for fingerprints of different pockets or a ligand of the caller's own.

``ligand_pair_hist`` / ``ligand_angles`` / ``batch_distributions`` / ``summarise_distributions`` are the rest of that report, the
distributions it compares with a dataset's by Jensen-Shannon distance (``repo/tools/geometry/eval_bond_length.py``,
``eval_bond_angle.py``): pair-distance histograms (``All_12A``, ``CC_2A``; reproduced exactly: they need coordinates and elements only),
and bond-length and bond-angle histograms per type on the table-bond graph (``cbgx_ligand_pair_hist`` / ``cbgx_ligand_angles``,
csrc/distributions.hip).  Angles are binned in cosine space against a table of cosines: no inverse trigonometric function runs on the
device.  Deviations: table bonds, so no aromatic type; every angle is counted once under its canonical type where the reference lists it
under both orientations -- the same normalised profile.  ``distribution_jsd`` / ``jsd_against`` take the caller's own reference vectors:
no dataset constants ship."""
import collections
import ctypes

import numpy as np
import torch

from . import _native
from .config import _AROMATIC, _ATOMIC_NUMBER

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


def _gpu_only(dev, entry, kernels):
    if dev.type != "cuda":
        raise _native.NativeError(f"{entry} runs on the GPU ({kernels}): there is no CPU fallback")


def _z_bytes(z):
    """atomic numbers as bytes; anything outside a byte is no element the tables know: 0"""
    return torch.where((z >= 0) & (z <= 255), z, torch.zeros_like(z)).to(torch.uint8).contiguous()


def _ligand_arrays(x, z, batch, n_graphs, side="lig", dev=None):
    """one side (``lig``; ``rec`` for the pocket of ``ligand_geometry``, which lives on ``dev``, the ligand's device) of every entry:
    checks, CSR of the graph index, float32 coordinates, atomic numbers as bytes"""
    dev = x.device if dev is None else dev
    for name, t in ((f"x_{side}", x), (f"z_{side}", z), (f"{side}_batch", batch)):
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, x_lig on {dev}")
    n = int(x.shape[0])
    if tuple(x.shape) != (n, 3):
        raise ValueError("coordinates must be [n, 3]")
    if z.shape != (n,) or batch.shape != (n,):
        raise ValueError("one atomic number and one graph index per atom")
    return n, _csr(batch, n_graphs, f"{side}_batch"), x.to(torch.float32).contiguous(), _z_bytes(z)


def _bond_ptr(bond_index, n_lig):
    """[n_lig + 1] int32 as the bond entries define it: the bonds are sorted by their first atom, a is the first atom of
    bond_ptr[a] ... bond_ptr[a + 1]"""
    first = bond_index[0].to(torch.long).clamp(0, max(n_lig - 1, 0))
    counts = torch.bincount(first, minlength=n_lig) if n_lig else first.new_zeros(0)
    return torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32).contiguous()


def _state_atoms(c, mode, lig_batch, batch, dev):
    """a sampling state's type indices (``c``: indices [n_lig] or scores [n_lig, C]: argmax) and atomic numbers, both int64 on ``dev``,
    and the number of graphs: the batch's ``num_graphs`` when it has it, else what ``lig_batch`` shows"""
    if mode not in _ATOMIC_NUMBER:
        raise ValueError(mode)
    typ = (c.argmax(-1) if c.dim() == 2 else c).to(dev).to(torch.long)
    z = torch.tensor(_ATOMIC_NUMBER[mode], dtype=torch.long, device=dev)[typ]
    n_graphs = int(batch["num_graphs"]) if "num_graphs" in batch else (int(lig_batch.max()) + 1 if lig_batch.numel() else 0)
    return typ, z, n_graphs


def ligand_geometry(x_lig, z_lig, lig_batch, x_rec, z_rec, rec_batch, n_graphs):
    """Stability and clash report of ``n_graphs`` ligands in their pockets, one launch on the tensors' current stream.

    ``x_lig`` [n_lig, 3] / ``x_rec`` [n_rec, 3] coordinates (evaluated as float32), ``z_lig`` / ``z_rec`` atomic numbers, ``lig_batch`` /
    ``rec_batch`` the graph index of every atom, grouped by graph.  Returns device tensors: ``nr_bonds`` [n_lig] int32, ``flags`` [n_lig]
    uint8 (STABLE, INTER_CLASH, INTRA_CLASH -- against ligand atoms without a TABLE bond, not RDKit's bonds --, UNKNOWN_ELEMENT) and
    ``graph_counts`` [n_graphs, 6] int32 (GRAPH_COLUMNS).  A ligand of more than MAX_LIGAND_ATOMS atoms raises ValueError.  There is no CPU
    path."""
    dev = x_lig.device
    _gpu_only(dev, "ligand_geometry", "cbgx_ligand_geometry")
    n_graphs = int(n_graphs)
    n_lig, lig_ptr, x_lig, z_lig = _ligand_arrays(x_lig, z_lig, lig_batch, n_graphs)
    n_rec, rec_ptr, x_rec, z_rec = _ligand_arrays(x_rec, z_rec, rec_batch, n_graphs, "rec", dev)
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
    _, z, n_graphs = _state_atoms(c, mode, lig_batch, batch, x.device)
    if "num_graphs" not in batch and batch["protein_element_batch"].numel():     # (a pocket whose ligand is empty counts too)
        n_graphs = max(n_graphs, int(batch["protein_element_batch"].max()) + 1)
    return ligand_geometry(x, z, lig_batch, batch["protein_pos"], batch["protein_element"], batch["protein_element_batch"], n_graphs)


# the job's integer totals: what ranks add up, and what the ratios are taken from
COUNT_KEYS = ("n_mol", "n_atoms", "n_stable", "n_mol_stable", "n_inter_clash_atoms", "n_intra_clash_atoms", "n_clash_mol",
              "n_protein_atoms_without_radius")
RATIOS = ("mol_stable", "atm_stable", "inter_clash_atom_ratio", "intra_clash_atom_ratio", "clash_mol_ratio")


def _counts(graph_counts, columns):
    """per-molecule counts (a tensor or any array-like) as int64 [n_mol, len(columns)]"""
    if isinstance(graph_counts, torch.Tensor):
        graph_counts = graph_counts.cpu().numpy()
    return np.asarray(graph_counts, dtype=np.int64).reshape(-1, len(columns))


def _ratio(a, b):
    return a / b if b else float("nan")


def job_totals(graph_counts):
    """per-molecule counts ``graph_counts`` [n_mol, 6] (GRAPH_COLUMNS; any array-like) -> the integer totals, in COUNT_KEYS order"""
    gc = _counts(graph_counts, GRAPH_COLUMNS)
    n_atoms, n_stable, n_mol_stable, n_inter, n_intra, n_norad = (int(v) for v in gc.sum(0))
    return [int(gc.shape[0]), n_atoms, n_stable, n_mol_stable, n_inter, n_intra, int((gc[:, 3] > 0).sum()), n_norad]


def summarise_totals(totals):
    """the five ratios (RATIOS) of integer totals in COUNT_KEYS order, and the totals as ``counts``; a ratio over nothing is nan"""
    c = {k: int(v) for k, v in zip(COUNT_KEYS, totals)}
    return {"mol_stable": _ratio(c["n_mol_stable"], c["n_mol"]), "atm_stable": _ratio(c["n_stable"], c["n_atoms"]),
            "inter_clash_atom_ratio": _ratio(c["n_inter_clash_atoms"], c["n_atoms"]),
            "intra_clash_atom_ratio": _ratio(c["n_intra_clash_atoms"], c["n_atoms"]),
            "clash_mol_ratio": _ratio(c["n_clash_mol"], c["n_mol"]), "counts": c}


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
    _gpu_only(dev, "ligand_bonds", "cbgx_ligand_bonds_count / _fill")
    n_graphs = int(n_graphs)
    n_lig, lig_ptr, x_lig, z_lig = _ligand_arrays(x_lig, z_lig, lig_batch, n_graphs)
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
    _, z, n_graphs = _state_atoms(c, mode, lig_batch, batch, x.device)
    return ligand_bonds(x, z, lig_batch, n_graphs)


BOND_COUNT_KEYS = ("n_mol", "n_atoms", "n_bonds", "n_connected_mol", "n_largest_fragment_atoms", "n_fragments", "n_cycles")
BOND_RATIOS = ("connected_mol_ratio", "largest_fragment_atom_ratio", "fragments_per_mol", "cycles_per_mol", "bonds_per_atom")


def bond_totals(graph_counts):
    """per-molecule counts ``graph_counts`` [n_mol, 6] (BOND_GRAPH_COLUMNS; any array-like) -> the integer totals, in BOND_COUNT_KEYS
    order; a molecule is connected iff n_fragments == 1"""
    gc = _counts(graph_counts, BOND_GRAPH_COLUMNS)
    n_atoms, n_bonds, _, n_frag, n_largest, n_cycles = (int(v) for v in gc.sum(0))
    return [int(gc.shape[0]), n_atoms, n_bonds, int((gc[:, 3] == 1).sum()), n_largest, n_frag, n_cycles]


def summarise_bond_totals(totals):
    """the five ratios (BOND_RATIOS) of integer totals in BOND_COUNT_KEYS order, and the totals as ``counts``; a ratio over nothing is nan"""
    c = {k: int(v) for k, v in zip(BOND_COUNT_KEYS, totals)}
    return {"connected_mol_ratio": _ratio(c["n_connected_mol"], c["n_mol"]),
            "largest_fragment_atom_ratio": _ratio(c["n_largest_fragment_atoms"], c["n_atoms"]),
            "fragments_per_mol": _ratio(c["n_fragments"], c["n_mol"]), "cycles_per_mol": _ratio(c["n_cycles"], c["n_mol"]),
            "bonds_per_atom": _ratio(c["n_bonds"], c["n_atoms"]), "counts": c}


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
    _gpu_only(dev, "ligand_rings", "cbgx_ligand_rings")
    n_graphs = int(n_graphs)
    if lig_batch.device != dev:
        raise ValueError(f"lig_batch is on {lig_batch.device}, bond_index on {dev}")
    if bond_index.dim() != 2 or bond_index.shape[0] != 2:
        raise ValueError("bond_index must be [2, n_bonds]")
    n_lig, n_bonds = int(lig_batch.shape[0]), int(bond_index.shape[1])
    if lig_batch.shape != (n_lig,):
        raise ValueError("one graph index per atom")
    lig_ptr = _csr(lig_batch, n_graphs, "lig_batch")
    bond_index, bond_ptr = bond_index.to(torch.int32).contiguous(), _bond_ptr(bond_index, n_lig)
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
    gc = _counts(graph_counts, RING_GRAPH_COLUMNS)
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
    n_mol = c["n_mol_evaluated"]
    in_six = sum(c[f"n_rings_{k}"] for k in range(3, 9))
    out = {f"ring_mol_ratio_{k}": _ratio(c[f"n_mol_with_ring_{k}"], n_mol) for k in RING_SIZES}
    out.update({f"rings_per_mol_{k}": _ratio(c[f"n_rings_{k}"], n_mol) for k in range(3, 9)})
    out.update({f"ring_size_distribution_{k}": _ratio(c[f"n_rings_{k}"], in_six) for k in range(3, 9)})
    out["macrocycle_mol_ratio"] = _ratio(c["n_mol_with_larger_ring"], n_mol)
    out["ring_atom_ratio"] = _ratio(c["n_ring_atoms"], c["n_atoms"])
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


# ---- aromatic atoms and bonds of the table-bond graph --------------------------------------------------------------------------------
MAX_AROMATIC_ATOMS, MAX_AROMATIC_CYCLES = 256, 128      # include/cbgx.h CBGX_AROMATIC_MAX_ATOMS / _MAX_CYCLES
# columns of ligand_aromatic's graph_counts (include/cbgx.h CBGX_AROMATIC_GRAPH_COLS)
AROMATIC_GRAPH_COLUMNS = ("n_atoms", "n_bonds", "n_cycles56", "n_aromatic_cycles", "n_flagged", "n_closure", "n_aromatic_atoms",
                          "n_aromatic_bonds", "n_unsupported", "status")
# status bits (include/cbgx.h CBGX_AROMATIC_*): a graph with status != 0 was not evaluated
AROMATIC_TOO_MANY_ATOMS, AROMATIC_TOO_MANY_CYCLES, AROMATIC_BAD_BONDS, AROMATIC_NO_RINGS = 1, 2, 4, 8
AROMATIC_BOND_TYPE = 4                     # bond_type of an aromatic bond; 1 ... 3 are the bond orders
BOND_TYPE_NOT_EVALUATED = 255


def ligand_aromatic(z_lig, flag_lig, lig_batch, n_graphs, bonds, rings):
    """Aromatic atoms and bonds of the bond graphs of ``n_graphs`` ligands, one launch (``cbgx_ligand_aromatic``, csrc/aromatic.hip; the
    definition is in include/cbgx.h) on the tensors' current stream: the closure F of the model's per-atom flags ``flag_lig`` under the
    reference's two rules (``reconstruct_mol``, repo/tools/rdkit_utils.py:380-389, 552-572) over the chordless 5- and 6-cycles of the
    graph, as a least fixed point; an aromatic cycle is such a cycle inside F.

    ``z_lig`` [n_lig] atomic numbers, ``flag_lig`` [n_lig] bool or 0 / 1, ``lig_batch`` [n_lig] grouped by graph; ``bonds``: what
    ``ligand_bonds`` returned for the same atoms, ``rings``: what ``ligand_rings`` returned for that bond list.  Returns device tensors:
    ``aromatic_atom`` [n_lig] bool (on an aromatic cycle), ``in_closure`` [n_lig] bool (in F), ``aromatic_bond`` [n_bonds] bool (an edge
    of an aromatic cycle), ``bond_type`` [n_bonds] uint8 (4 for an aromatic bond, else ``bond_order``; 255 where not evaluated) and
    ``graph_counts`` [n_graphs, 10] int32 (AROMATIC_GRAPH_COLUMNS).  A graph over a limit, with a malformed list, or that the ring report
    did not evaluate is not an error: its status is non-zero (AROMATIC_*), its columns from n_cycles56 to n_unsupported are -1, its atoms
    and bonds are False here and its ``bond_type`` 255.  Deviations from the reference: the rules run to their fixed point (the
    reference applies each once, in OpenBabel's order: its result is contained in this one); a bond is aromatic only as an edge of an
    aromatic cycle (the reference marks every bond with two aromatic ends, e.g. the link of biphenyl).  There is no CPU path."""
    dev = z_lig.device
    _gpu_only(dev, "ligand_aromatic", "cbgx_ligand_aromatic")
    n_graphs = int(n_graphs)
    bond_index, bond_order, ring_min = bonds["bond_index"], bonds["bond_order"], rings["atom_ring_min"]
    for name, t in (("flag_lig", flag_lig), ("lig_batch", lig_batch), ("bond_index", bond_index), ("bond_order", bond_order),
                    ("atom_ring_min", ring_min)):
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, z_lig on {dev}")
    if bond_index.dim() != 2 or bond_index.shape[0] != 2:
        raise ValueError("bond_index must be [2, n_bonds]")
    n_lig, n_bonds = int(z_lig.shape[0]), int(bond_index.shape[1])
    if z_lig.shape != (n_lig,) or flag_lig.shape != (n_lig,) or lig_batch.shape != (n_lig,) or ring_min.shape != (n_lig,):
        raise ValueError("one atomic number, one flag, one graph index and one atom_ring_min per atom")
    if bond_order.shape != (n_bonds,):
        raise ValueError("one bond_order per bond")
    lig_ptr = _csr(lig_batch, n_graphs, "lig_batch")
    z_lig = _z_bytes(z_lig)
    flag_lig = (flag_lig != 0).to(torch.uint8).contiguous()
    ring_min = ring_min.to(torch.uint8).contiguous()
    bond_index, bond_ptr = bond_index.to(torch.int32).contiguous(), _bond_ptr(bond_index, n_lig)
    atom_out = torch.empty(n_lig, dtype=torch.uint8, device=dev)
    bond_out = torch.empty(n_bonds, dtype=torch.uint8, device=dev)
    graph_counts = torch.empty(n_graphs, len(AROMATIC_GRAPH_COLUMNS), dtype=torch.int32, device=dev)
    p = _native.ptr
    _native.check(_native.lib().cbgx_ligand_aromatic(p(z_lig), p(flag_lig), p(ring_min), p(lig_ptr), n_lig, n_graphs, p(bond_ptr),
                                                     p(bond_index) if n_bonds else None, n_bonds, p(atom_out),
                                                     p(bond_out) if n_bonds else None, p(graph_counts), _native.current_stream(dev)),
                  "cbgx_ligand_aromatic")
    evaluated, bond_evaluated = atom_out != 255, bond_out != 255
    bond_type = torch.where(bond_out == 1, torch.full_like(bond_out, AROMATIC_BOND_TYPE), bond_order.to(torch.uint8))
    bond_type = torch.where(bond_evaluated, bond_type, torch.full_like(bond_out, BOND_TYPE_NOT_EVALUATED))
    return {"aromatic_atom": evaluated & ((atom_out & 2) != 0), "in_closure": evaluated & ((atom_out & 1) != 0),
            "aromatic_bond": bond_out == 1, "bond_type": bond_type, "graph_counts": graph_counts}


def batch_aromatic(batch, x, c, lig_batch, mode, bonds=None, rings=None):
    """``ligand_aromatic`` of a sampling state: the flags are the aromatic atom types of the vocabulary (``config._AROMATIC[mode]``), so
    ``mode='basic'`` -- no flags to start from -- raises ValueError; ``bonds`` / ``rings``: what ``batch_bonds`` / ``batch_rings`` returned
    for the same state (called here when None)"""
    if mode not in _AROMATIC:
        raise ValueError(f"mode {mode!r} has no aromatic atom types: the aromatic report starts from the model's flags ('add_aromatic')")
    if bonds is None:
        bonds = batch_bonds(batch, x, c, lig_batch, mode)
    dev = bonds["bond_index"].device
    lig_batch = lig_batch.to(dev)
    typ, z, n_graphs = _state_atoms(c, mode, lig_batch, {"num_graphs": bonds["graph_counts"].shape[0]}, dev)
    if rings is None:
        rings = ligand_rings(bonds["bond_index"], lig_batch, n_graphs)
    flag = torch.tensor(_AROMATIC[mode], dtype=torch.bool, device=dev)[typ]
    return ligand_aromatic(z, flag, lig_batch, n_graphs, bonds, rings)


AROMATIC_COUNT_KEYS = ("n_mol", "n_mol_evaluated", "n_mol_over_limit", "n_atoms", "n_bonds", "n_cycles56", "n_aromatic_cycles",
                       "n_flagged", "n_closure", "n_aromatic_atoms", "n_aromatic_bonds", "n_unsupported", "n_aromatic_mol")
AROMATIC_RATIOS = ("aromatic_mol_ratio", "aromatic_rings_per_mol", "aromatic_cycle_share", "aromatic_atom_ratio", "aromatic_bond_ratio",
                   "unsupported_flag_ratio")


def aromatic_totals(graph_counts):
    """per-molecule counts ``graph_counts`` [n_mol, 10] (AROMATIC_GRAPH_COLUMNS; any array-like) -> the integer totals, in
    AROMATIC_COUNT_KEYS order.  Everything but n_mol and n_mol_over_limit is summed over the evaluated molecules (status == 0) only"""
    gc = _counts(graph_counts, AROMATIC_GRAPH_COLUMNS)
    ok = gc[gc[:, -1] == 0]
    return ([int(gc.shape[0]), int(ok.shape[0]), int(gc.shape[0] - ok.shape[0])] + [int(v) for v in ok[:, :9].sum(0)]
            + [int((ok[:, 3] > 0).sum())])


def summarise_aromatic_totals(totals):
    """the ratios (AROMATIC_RATIOS) of integer totals in AROMATIC_COUNT_KEYS order, and the totals as ``counts``; every ratio is over the
    EVALUATED molecules, a ratio over nothing is nan.  aromatic_mol_ratio: the share of molecules with at least one aromatic cycle;
    aromatic_rings_per_mol; aromatic_cycle_share: aromatic cycles / chordless 5- and 6-cycles; aromatic_atom_ratio / aromatic_bond_ratio:
    aromatic atoms / atoms, aromatic bonds / bonds; unsupported_flag_ratio: n_unsupported / n_flagged, how often the model emitted an
    aromatic type where the geometry built no ring to carry it"""
    c = {k: int(v) for k, v in zip(AROMATIC_COUNT_KEYS, totals)}
    return {"aromatic_mol_ratio": _ratio(c["n_aromatic_mol"], c["n_mol_evaluated"]),
            "aromatic_rings_per_mol": _ratio(c["n_aromatic_cycles"], c["n_mol_evaluated"]),
            "aromatic_cycle_share": _ratio(c["n_aromatic_cycles"], c["n_cycles56"]),
            "aromatic_atom_ratio": _ratio(c["n_aromatic_atoms"], c["n_atoms"]),
            "aromatic_bond_ratio": _ratio(c["n_aromatic_bonds"], c["n_bonds"]),
            "unsupported_flag_ratio": _ratio(c["n_unsupported"], c["n_flagged"]), "counts": c}


def summarise_aromatic(graph_counts):
    """aromatic statistics of a set of molecules from integer per-molecule counts (``graph_counts`` [n_mol, 10], AROMATIC_GRAPH_COLUMNS):
    see ``summarise_aromatic_totals``"""
    return summarise_aromatic_totals(aromatic_totals(graph_counts))


# ---- Kekule orders, implicit hydrogens and valence checks of the table-bond graph ---------------------------------------------------------
# include/cbgx.h CBGX_VALENCE_MAX_ATOMS / _MAX_ELIGIBLE / _MAX_STEPS
MAX_VALENCE_ATOMS, MAX_VALENCE_ELIGIBLE, MAX_VALENCE_STEPS = 256, 64, 65536
# columns of ligand_valence's graph_counts (include/cbgx.h CBGX_VALENCE_GRAPH_COLS); el_c: atoms of element code c (H C N O F P S Cl)
VALENCE_GRAPH_COLUMNS = (("n_atoms", "n_bonds", "n_fragments", "n_systems", "n_systems_failed", "n_kekule_double", "n_implicit_h",
                          "n_exceeded", "n_unknown", "n_nhoh", "n_no") + tuple(f"el_{c}" for c in range(8))
                         + ("valence_ok", "steps_max", "status"))
# atom_flags bits and status bits (include/cbgx.h CBGX_VALENCE_*): a graph with status != 0 was not evaluated
VALENCE_EXCEEDED, VALENCE_ON_FAILED_SYSTEM, VALENCE_UNKNOWN_ELEMENT, VALENCE_ON_AROMATIC_SYSTEM = 1, 2, 4, 8
VALENCE_TOO_MANY_ATOMS, VALENCE_BAD_BONDS, VALENCE_NO_AROMATIC, VALENCE_SEARCH_LIMIT = 1, 4, 8, 16
KEKULE_FAILED = 4                          # bond_kekule of the aromatic bonds of a system without a Kekule structure
VALENCE_NOT_EVALUATED = 255
ELEMENT_SYMBOLS = ("H", "C", "N", "O", "F", "P", "S", "Cl")                        # element codes 0 ... 7
ATOMIC_WEIGHTS = (1.008, 12.011, 14.007, 15.999, 18.998, 30.974, 32.06, 35.45)     # standard atomic weights, in element-code order


def ligand_valence(z_lig, lig_batch, n_graphs, bonds, aromatic=None, max_steps=MAX_VALENCE_STEPS):
    """Kekule bond orders, implicit hydrogens and valence flags of the bond graphs of ``n_graphs`` ligands, one launch
    (``cbgx_ligand_valence``, csrc/valence.hip; the definition is in include/cbgx.h) on the tensors' current stream: per aromatic system
    (a connected component of the aromatic bonds) the largest, lexicographically least set of double bonds that covers every carbon able
    to take one, found by a bounded search; then every atom's valence against this library's table (H 1, C 4, N 3, O 2, F 1, P 3 / 5,
    S 2 / 4 / 6, Cl 1; no charges).

    ``z_lig`` [n_lig] atomic numbers, ``lig_batch`` [n_lig] grouped by graph; ``bonds``: what ``ligand_bonds`` returned for the same atoms;
    ``aromatic``: what ``ligand_aromatic`` returned for that list, or None: no bond is aromatic ('basic' atom types); ``max_steps``: the
    search budget per system, 1 ... MAX_VALENCE_STEPS.  Returns device tensors: ``implicit_h`` [n_lig] uint8, ``atom_flags`` [n_lig] uint8
    (VALENCE_EXCEEDED, _ON_FAILED_SYSTEM, _UNKNOWN_ELEMENT, _ON_AROMATIC_SYSTEM), ``bond_kekule`` [n_bonds] uint8 (1 ... 3; KEKULE_FAILED
    = 4 on a system without a Kekule structure) and ``graph_counts`` [n_graphs, 22] int32 (VALENCE_GRAPH_COLUMNS).  A graph over a limit
    (atoms; 64 eligible bonds or atoms of one system; the step budget), with a malformed list, or that the aromatic report did not
    evaluate is not an error: its status is non-zero (VALENCE_*), its columns from n_fragments to steps_max are -1 and its bytes of the
    three arrays 255.  Deviations from the reference: table bonds and a property-defined Kekule choice (the reference's orders come from
    OpenBabel's perception, its Kekule form from RDKit's traversal); no charges: N(=O)=O, N-oxides and quaternary N are "exceeded".
    There is no CPU path."""
    dev = z_lig.device
    _gpu_only(dev, "ligand_valence", "cbgx_ligand_valence")
    n_graphs, max_steps = int(n_graphs), int(max_steps)
    bond_index, bond_order = bonds["bond_index"], bonds["bond_order"]
    given = [("lig_batch", lig_batch), ("bond_index", bond_index), ("bond_order", bond_order)]
    if aromatic is not None:
        given += [("aromatic_bond", aromatic["aromatic_bond"]), ("bond_type", aromatic["bond_type"])]
    for name, t in given:
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, z_lig on {dev}")
    if bond_index.dim() != 2 or bond_index.shape[0] != 2:
        raise ValueError("bond_index must be [2, n_bonds]")
    n_lig, n_bonds = int(z_lig.shape[0]), int(bond_index.shape[1])
    if z_lig.shape != (n_lig,) or lig_batch.shape != (n_lig,):
        raise ValueError("one atomic number and one graph index per atom")
    if any(t.shape != (n_bonds,) for _, t in given[2:]):
        raise ValueError("one bond_order (and one aromatic_bond and bond_type) per bond")
    if not 1 <= max_steps <= MAX_VALENCE_STEPS:
        raise ValueError(f"max_steps is 1 ... {MAX_VALENCE_STEPS}, not {max_steps}")
    lig_ptr = _csr(lig_batch, n_graphs, "lig_batch")
    z_lig = _z_bytes(z_lig)
    bond_index, bond_ptr = bond_index.to(torch.int32).contiguous(), _bond_ptr(bond_index, n_lig)
    bond_order = bond_order.to(torch.uint8).contiguous()
    flag = None
    if aromatic is not None:      # the bytes cbgx_ligand_aromatic wrote: 0, 1, or 255 where it did not evaluate the graph
        flag = torch.where(aromatic["bond_type"] == BOND_TYPE_NOT_EVALUATED, torch.full_like(bond_order, VALENCE_NOT_EVALUATED),
                           (aromatic["aromatic_bond"] != 0).to(torch.uint8)).contiguous()
    implicit_h = torch.empty(n_lig, dtype=torch.uint8, device=dev)
    atom_flags = torch.empty(n_lig, dtype=torch.uint8, device=dev)
    bond_kekule = torch.empty(n_bonds, dtype=torch.uint8, device=dev)
    graph_counts = torch.empty(n_graphs, len(VALENCE_GRAPH_COLUMNS), dtype=torch.int32, device=dev)
    p = _native.ptr
    _native.check(_native.lib().cbgx_ligand_valence(p(z_lig), p(lig_ptr), n_lig, n_graphs, p(bond_ptr), p(bond_index) if n_bonds else None,
                                                    p(bond_order) if n_bonds else None, p(flag) if flag is not None and n_bonds else None,
                                                    n_bonds, max_steps, p(implicit_h), p(atom_flags), p(bond_kekule) if n_bonds else None,
                                                    p(graph_counts), _native.current_stream(dev)), "cbgx_ligand_valence")
    return {"implicit_h": implicit_h, "atom_flags": atom_flags, "bond_kekule": bond_kekule, "graph_counts": graph_counts}


def batch_valence(batch, x, c, lig_batch, mode, bonds=None, aromatic=None):
    """``ligand_valence`` of a sampling state; ``bonds`` / ``aromatic``: what ``batch_bonds`` / ``batch_aromatic`` returned for the same
    state.  ``bonds`` is computed here when None; so is ``aromatic`` when None and ``mode`` has aromatic atom types ('add_aromatic').  In
    any other mode there are no flags to start from and no bond is aromatic"""
    if bonds is None:
        bonds = batch_bonds(batch, x, c, lig_batch, mode)
    if aromatic is None and mode in _AROMATIC:
        aromatic = batch_aromatic(batch, x, c, lig_batch, mode, bonds=bonds)
    dev = bonds["bond_index"].device
    lig_batch = lig_batch.to(dev)
    _, z, n_graphs = _state_atoms(c, mode, lig_batch, {"num_graphs": bonds["graph_counts"].shape[0]}, dev)
    return ligand_valence(z, lig_batch, n_graphs, bonds, aromatic)


def formula(el_counts, n_h=0):
    """Hill-order formula of the atoms per element code (``el_counts`` [8]: H C N O F P S Cl) with ``n_h`` implicit hydrogens added to
    the explicit ones: C, H, then the other symbols alphabetically when there is carbon, else all alphabetically; '' for no atoms"""
    count = {s: int(v) for s, v in zip(ELEMENT_SYMBOLS, el_counts)}
    count["H"] += int(n_h)
    symbols = sorted(s for s in count if count[s])
    if count["C"]:
        symbols = ["C"] + (["H"] if count["H"] else []) + [s for s in symbols if s not in ("C", "H")]
    return "".join(s + (str(count[s]) if count[s] > 1 else "") for s in symbols)


def mol_weight(el_counts, n_h=0):
    """molecular weight: the fp64 dot product of ATOMIC_WEIGHTS with the atoms per element code, the ``n_h`` implicit hydrogens added to
    el_0, summed in element-code order"""
    counts = np.asarray([int(v) for v in el_counts], np.float64)
    counts[0] += int(n_h)
    total = 0.0
    for w, k in zip(ATOMIC_WEIGHTS, counts):
        total += w * float(k)
    return total


VALENCE_COUNT_KEYS = (("n_mol", "n_mol_evaluated", "n_mol_over_limit", "n_atoms", "n_bonds", "n_fragments", "n_systems", "n_systems_failed",
                       "n_kekule_double", "n_implicit_h", "n_exceeded", "n_unknown", "n_nhoh", "n_no")
                      + tuple(f"n_el_{c}" for c in range(8)) + ("n_valence_ok_mol", "n_valid_mol"))
VALENCE_RATIOS = ("valence_ok_mol_ratio", "valid_mol_ratio", "kekulised_system_ratio", "exceeded_atom_ratio", "h_per_heavy_atom",
                  "nhoh_per_mol", "no_per_mol", "mean_mol_weight")


def valence_totals(graph_counts):
    """per-molecule counts ``graph_counts`` [n_mol, 22] (VALENCE_GRAPH_COLUMNS; any array-like) -> the integer totals, in
    VALENCE_COUNT_KEYS order.  Everything but n_mol and n_mol_over_limit is summed over the evaluated molecules (status == 0) only; a
    molecule is valid iff valence_ok and n_fragments == 1"""
    gc = _counts(graph_counts, VALENCE_GRAPH_COLUMNS)
    ok = gc[gc[:, -1] == 0]
    return ([int(gc.shape[0]), int(ok.shape[0]), int(gc.shape[0] - ok.shape[0])] + [int(v) for v in ok[:, :19].sum(0)]
            + [int((ok[:, 19] == 1).sum()), int(((ok[:, 19] == 1) & (ok[:, 2] == 1)).sum())])


def summarise_valence_totals(totals):
    """the ratios (VALENCE_RATIOS), ``element_distribution`` and the totals as ``counts``, of integer totals in VALENCE_COUNT_KEYS order;
    every ratio is over the EVALUATED molecules, a ratio over nothing is nan.  valence_ok_mol_ratio: no atom exceeded, no unknown
    element, every aromatic system kekulised; valid_mol_ratio: that and one fragment -- the table-bond counterpart of a molecule RDKit
    sanitises whose SMILES has no '.' (evaluate_validity, repo/tools/rdkit_utils.py:615-640); kekulised_system_ratio: solved systems /
    systems; exceeded_atom_ratio: exceeded atoms / atoms; h_per_heavy_atom: implicit H / atoms that are not H; nhoh_per_mol / no_per_mol:
    N and O with a hydrogen / N and O, per molecule (Lipinski's donors and acceptors); mean_mol_weight: ATOMIC_WEIGHTS over the element
    counts with the implicit H, per molecule; element_distribution: the 8 shares of the element codes among the atoms that have one (what
    repo/tools/eval_atom_type.py compares; no dataset constants ship)"""
    c = {k: int(v) for k, v in zip(VALENCE_COUNT_KEYS, totals)}
    el = [c[f"n_el_{k}"] for k in range(8)]
    n_mol = c["n_mol_evaluated"]
    return {"valence_ok_mol_ratio": _ratio(c["n_valence_ok_mol"], n_mol), "valid_mol_ratio": _ratio(c["n_valid_mol"], n_mol),
            "kekulised_system_ratio": _ratio(c["n_systems"] - c["n_systems_failed"], c["n_systems"]),
            "exceeded_atom_ratio": _ratio(c["n_exceeded"], c["n_atoms"]),
            "h_per_heavy_atom": _ratio(c["n_implicit_h"], c["n_atoms"] - el[0]),
            "nhoh_per_mol": _ratio(c["n_nhoh"], n_mol), "no_per_mol": _ratio(c["n_no"], n_mol),
            "mean_mol_weight": _ratio(mol_weight(el, c["n_implicit_h"]), n_mol),
            "element_distribution": [_ratio(v, sum(el)) for v in el], "counts": c}


def summarise_valence(graph_counts):
    """valence statistics of a set of molecules from integer per-molecule counts (``graph_counts`` [n_mol, 22], VALENCE_GRAPH_COLUMNS):
    see ``summarise_valence_totals``"""
    return summarise_valence_totals(valence_totals(graph_counts))


# ---- typed pocket contacts and a score in Vina's functional form --------------------------------------------------------------------------
MAX_INTERACTION_ATOMS = 256                # include/cbgx.h CBGX_INTERACTIONS_MAX_ATOMS
INTERACTION_TERMS = ("gauss1", "gauss2", "repulsion", "hydrophobic", "hbond")
# columns of ligand_interactions' graph_counts (include/cbgx.h CBGX_INTERACTIONS_GRAPH_COLS)
INTERACTION_GRAPH_COLUMNS = ("n_atoms", "n_bonds", "n_rotatable", "n_donors", "n_acceptors", "n_hydrophobic_atoms", "n_pairs",
                             "n_hbond_pairs", "n_hydrophobic_pairs", "n_close_pairs", "n_contact_atoms", "n_protein_untyped", "status")
# a type byte (include/cbgx.h CBGX_INTERACTIONS_*): element code 1 ... 7 (C N O F P S Cl) under the mask, three property bits; 0: takes
# no part; UNTYPED: a pocket atom of an element outside H C N O S
INTERACTION_ELEMENT_MASK, INTERACTION_HYDROPHOBIC, INTERACTION_DONOR, INTERACTION_ACCEPTOR, INTERACTION_UNTYPED = 7, 8, 16, 32, 64
# status bits: a graph with status != 0 was not evaluated
INTERACTIONS_TOO_MANY_ATOMS, INTERACTIONS_BAD_BONDS, INTERACTIONS_NO_VALENCE = 1, 4, 8
INTERACTION_NOT_EVALUATED = 255
# the published defaults of AutoDock Vina (O. Trott, A. J. Olson, J. Comput. Chem. 31 (2010) 455-461), in INTERACTION_TERMS order, and
# its weight per rotatable bond
INTERACTION_WEIGHTS = (-0.035579, -0.005156, 0.840245, -0.035069, -0.587439)
INTERACTION_ROT_WEIGHT = 0.05846
AA_NAMES = ("ALA", "CYS", "ASP", "GLU", "PHE", "GLY", "HIS", "ILE", "LYS", "LEU", "MET", "ASN", "PRO", "GLN", "ARG", "SER", "THR", "VAL",
            "TRP", "TYR")                 # the reference's aa_name_number order: what ``rec_aa`` indexes
BACKBONE_FEATURE = 6                       # the is_backbone column of ``protein_atom_feature`` (protein_featurizer.py:21-26)


def _small_bytes(t, other):
    """an index tensor as bytes; anything outside 0 ... 254 becomes ``other``"""
    t = t.to(torch.long)
    return torch.where((t >= 0) & (t < 255), t, torch.full_like(t, other)).to(torch.uint8).contiguous()


def pocket_types(x_rec, z_rec, rec_batch, n_graphs, rec_aa, rec_backbone):
    """Donor / acceptor / hydrophobic types of the pocket atoms of ``n_graphs`` graphs, one launch (``cbgx_pocket_types``,
    csrc/interactions.hip; the table is in include/cbgx.h) on the tensors' current stream.

    ``x_rec`` [n_rec, 3], ``z_rec`` [n_rec] atomic numbers, ``rec_batch`` [n_rec] grouped by graph, ``rec_aa`` [n_rec] residue indices in
    AA_NAMES order (anything else: "other"), ``rec_backbone`` [n_rec] bool or 0 / 1.  Returns ``rec_type`` [n_rec] uint8 on the device: the
    element code 1 ... 7 under INTERACTION_ELEMENT_MASK with INTERACTION_HYDROPHOBIC / _DONOR / _ACCEPTOR; 0 for H; INTERACTION_UNTYPED for
    an element outside H C N O S.  No hydrogens are read and no protonation state is modelled: HIS side-chain N is donor and acceptor.
    A carbon is hydrophobic unless it has a TABLE bond to an N, O or S atom of its pocket.  There is no CPU path."""
    dev = x_rec.device
    _gpu_only(dev, "pocket_types", "cbgx_pocket_types")
    n_graphs = int(n_graphs)
    n_rec, rec_ptr, x_rec, z_rec = _ligand_arrays(x_rec, z_rec, rec_batch, n_graphs, "rec")
    for name, t in (("rec_aa", rec_aa), ("rec_backbone", rec_backbone)):
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, x_rec on {dev}")
        if t.shape != (n_rec,):
            raise ValueError("one residue index and one backbone flag per pocket atom")
    aa = _small_bytes(rec_aa, len(AA_NAMES))
    backbone = (rec_backbone != 0).to(torch.uint8).contiguous()
    rec_type = torch.empty(n_rec, dtype=torch.uint8, device=dev)
    p = _native.ptr
    _native.check(_native.lib().cbgx_pocket_types(p(x_rec), p(z_rec), p(rec_ptr), n_rec, n_graphs, p(aa), p(backbone), p(rec_type),
                                                  _native.current_stream(dev)), "cbgx_pocket_types")
    return rec_type


def ligand_interactions(x_lig, z_lig, lig_batch, x_rec, rec_type, rec_batch, n_graphs, bonds, valence, aromatic=None):
    """Ligand atom types, rotatable bonds and the five pair terms of Vina's functional form of ``n_graphs`` ligands against their typed
    pockets, one launch (``cbgx_ligand_interactions``, csrc/interactions.hip; the definition, the constants and the order of every sum
    are in include/cbgx.h) on the tensors' current stream.  A score in Vina's functional form on this library's own atom typing: NOT a
    reproduction of the Vina program, and not validated against it.

    Ligand and pocket sides as ``ligand_geometry``; ``rec_type``: what ``pocket_types`` returned; ``bonds``: what ``ligand_bonds`` returned
    for the same atoms; ``valence``: what ``ligand_valence`` returned for that list; ``aromatic``: what ``ligand_aromatic`` returned, or
    None (an aromatic bond of that report is an edge of a cycle and never rotatable either way).  Returns device tensors: ``atom_terms``
    [n_lig, 5] float64 (INTERACTION_TERMS: a ligand atom's sums over the pocket), ``lig_type`` [n_lig] uint8, ``bond_rotatable`` [n_bonds]
    uint8, ``graph_terms`` [n_graphs, 5] float64 and ``graph_counts`` [n_graphs, 13] int32 (INTERACTION_GRAPH_COLUMNS).  A graph of more
    than MAX_INTERACTION_ATOMS atoms, with a malformed list, or that the valence report did not evaluate is not an error: its status is
    non-zero (INTERACTIONS_*), its columns from n_rotatable to n_protein_untyped are -1, its floats nan and its bytes 255.  Deviations
    from the reference's Vina / PLIP path: table bonds; residue-table pocket typing without hydrogens or protonation states; this
    library's acceptor rule for N; no intramolecular term, no metals, no Br / I; RDKit's non-strict rotatable-bond pattern.  There is no
    CPU path."""
    dev = x_lig.device
    _gpu_only(dev, "ligand_interactions", "cbgx_ligand_interactions")
    n_graphs = int(n_graphs)
    n_lig, lig_ptr, x_lig, z_lig = _ligand_arrays(x_lig, z_lig, lig_batch, n_graphs)
    n_rec, rec_ptr, x_rec, _ = _ligand_arrays(x_rec, rec_type, rec_batch, n_graphs, "rec", dev)
    bond_index = bonds["bond_index"]
    given = [("bond_index", bond_index), ("bond_kekule", valence["bond_kekule"]), ("implicit_h", valence["implicit_h"]),
             ("atom_flags", valence["atom_flags"]), ("valence graph_counts", valence["graph_counts"])]
    if aromatic is not None:
        given.append(("aromatic_bond", aromatic["aromatic_bond"]))
    for name, t in given:
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, x_lig on {dev}")
    if bond_index.dim() != 2 or bond_index.shape[0] != 2:
        raise ValueError("bond_index must be [2, n_bonds]")
    n_bonds = int(bond_index.shape[1])
    if valence["bond_kekule"].shape != (n_bonds,) or (aromatic is not None and aromatic["aromatic_bond"].shape != (n_bonds,)):
        raise ValueError("one bond_kekule (and one aromatic_bond) per bond")
    if valence["implicit_h"].shape != (n_lig,) or valence["atom_flags"].shape != (n_lig,):
        raise ValueError("one implicit_h and one atom_flags per atom")
    if tuple(valence["graph_counts"].shape) != (n_graphs, len(VALENCE_GRAPH_COLUMNS)):
        raise ValueError("the valence report's graph_counts must be [n_graphs, 22]")
    rec_type = rec_type.to(torch.uint8).contiguous()
    bond_index, bond_ptr = bond_index.to(torch.int32).contiguous(), _bond_ptr(bond_index, n_lig)
    kekule = valence["bond_kekule"].to(torch.uint8).contiguous()
    implicit_h, atom_flags = valence["implicit_h"].to(torch.uint8).contiguous(), valence["atom_flags"].to(torch.uint8).contiguous()
    val_status = valence["graph_counts"][:, -1].to(torch.int32).contiguous()
    flag = None if aromatic is None else (aromatic["aromatic_bond"] != 0).to(torch.uint8).contiguous()
    atom_terms = torch.empty(n_lig, len(INTERACTION_TERMS), dtype=torch.float64, device=dev)
    lig_type = torch.empty(n_lig, dtype=torch.uint8, device=dev)
    bond_rotatable = torch.empty(n_bonds, dtype=torch.uint8, device=dev)
    graph_terms = torch.empty(n_graphs, len(INTERACTION_TERMS), dtype=torch.float64, device=dev)
    graph_counts = torch.empty(n_graphs, len(INTERACTION_GRAPH_COLUMNS), dtype=torch.int32, device=dev)
    p = _native.ptr
    _native.check(_native.lib().cbgx_ligand_interactions(
        p(x_lig), p(z_lig), p(lig_ptr), n_lig, p(x_rec), p(rec_type), p(rec_ptr), n_rec, n_graphs, p(bond_ptr),
        p(bond_index) if n_bonds else None, p(kekule) if n_bonds else None, p(flag) if flag is not None and n_bonds else None, n_bonds,
        p(implicit_h), p(atom_flags), p(val_status), p(atom_terms), p(lig_type), p(bond_rotatable) if n_bonds else None, p(graph_terms),
        p(graph_counts), _native.current_stream(dev)), "cbgx_ligand_interactions")
    return {"atom_terms": atom_terms, "lig_type": lig_type, "bond_rotatable": bond_rotatable, "graph_terms": graph_terms,
            "graph_counts": graph_counts}


def batch_interactions(batch, x, c, lig_batch, mode, bonds=None, valence=None):
    """``pocket_types`` + ``ligand_interactions`` of a sampling state against the batch's own pocket (``protein_pos``,
    ``protein_element``, ``protein_element_batch``, ``protein_aa_type`` and the is_backbone column of ``protein_atom_feature``), in the
    frame both share; ``bonds`` / ``valence``: what ``batch_bonds`` / ``batch_valence`` returned for the same state (computed here when
    None).  Also returns ``rec_type``"""
    if bonds is None:
        bonds = batch_bonds(batch, x, c, lig_batch, mode)
    if valence is None:
        valence = batch_valence(batch, x, c, lig_batch, mode, bonds=bonds)
    dev = bonds["bond_index"].device
    lig_batch = lig_batch.to(dev)
    _, z, n_graphs = _state_atoms(c, mode, lig_batch, {"num_graphs": bonds["graph_counts"].shape[0]}, dev)
    x_rec, z_rec, rec_b = (batch[k].to(dev) for k in ("protein_pos", "protein_element", "protein_element_batch"))
    rec_type = pocket_types(x_rec, z_rec, rec_b, n_graphs, batch["protein_aa_type"].to(dev),
                            batch["protein_atom_feature"].to(dev)[:, BACKBONE_FEATURE])
    out = ligand_interactions(x.to(dev), z, lig_batch, x_rec, rec_type, rec_b, n_graphs, bonds, valence)
    out["rec_type"] = rec_type
    return out


INTERACTION_COUNT_KEYS = (("n_mol", "n_mol_evaluated", "n_mol_over_limit") + INTERACTION_GRAPH_COLUMNS[:-1]
                          + ("n_mol_with_hbond", "n_mol_negative_score", "score_micro", "score_inter_micro"))
INTERACTION_RATIOS = ("mean_score", "mean_score_inter", "negative_score_mol_ratio", "hbond_pairs_per_mol", "hydrophobic_pairs_per_mol",
                      "close_pairs_per_mol", "rotatable_per_mol", "mol_with_hbond_ratio")


def interaction_scores(graph_counts, graph_terms):
    """(score_inter [n_mol], score [n_mol]) float64 of per-molecule counts and terms: score_inter = sum_k INTERACTION_WEIGHTS[k]
    graph_terms[:, k], added in index order in float64; score = score_inter / (1 + INTERACTION_ROT_WEIGHT n_rotatable); nan where
    status != 0"""
    gc = _counts(graph_counts, INTERACTION_GRAPH_COLUMNS)
    terms = np.asarray(_np(graph_terms), np.float64).reshape(-1, len(INTERACTION_TERMS))
    if terms.shape[0] != gc.shape[0]:
        raise ValueError("one row of terms per row of counts")
    ok = gc[:, -1] == 0
    inter = np.zeros(gc.shape[0], np.float64)
    for k, w in enumerate(INTERACTION_WEIGHTS):
        inter = inter + w * np.where(ok, terms[:, k], 0.0)
    score = inter / (1.0 + INTERACTION_ROT_WEIGHT * np.where(ok, gc[:, 2], 0).astype(np.float64))
    return np.where(ok, inter, np.nan), np.where(ok, score, np.nan)


def score_micro(score):
    """a score as the integer ranks add up: int(rint(score 1e6))"""
    return int(np.rint(float(score) * 1e6))


def interaction_totals(graph_counts, graph_terms):
    """per-molecule counts ``graph_counts`` [n_mol, 13] (INTERACTION_GRAPH_COLUMNS) and terms ``graph_terms`` [n_mol, 5] (any array-likes)
    -> the integer totals, in INTERACTION_COUNT_KEYS order.  Everything but n_mol and n_mol_over_limit is summed over the evaluated
    molecules (status == 0) only; score_micro / score_inter_micro: the sums of the per-molecule ``score_micro`` integers, so that a job's
    mean does not depend on how its molecules were sharded"""
    gc = _counts(graph_counts, INTERACTION_GRAPH_COLUMNS)
    inter, score = interaction_scores(gc, graph_terms)
    ok = gc[:, -1] == 0
    good = gc[ok]
    return ([int(gc.shape[0]), int(good.shape[0]), int(gc.shape[0] - good.shape[0])] + [int(v) for v in good[:, :12].sum(0)]
            + [int((good[:, 7] > 0).sum()), int(sum(score_micro(s) < 0 for s in score[ok])), int(sum(score_micro(s) for s in score[ok])),
               int(sum(score_micro(s) for s in inter[ok]))])


def summarise_interaction_totals(totals):
    """the ratios (INTERACTION_RATIOS) of integer totals in INTERACTION_COUNT_KEYS order, and the totals as ``counts``; every ratio is
    over the EVALUATED molecules, a ratio over nothing is nan.  mean_score / mean_score_inter: score_micro / 1e6 per molecule, in the
    units of Vina's weights (kcal/mol there; here a score in its functional form, not validated against the program);
    negative_score_mol_ratio: the share of molecules whose score_micro < 0; hbond / hydrophobic / close pairs and rotatable bonds per
    molecule; mol_with_hbond_ratio: the share with at least one hbond pair"""
    c = {k: int(v) for k, v in zip(INTERACTION_COUNT_KEYS, totals)}
    n_mol = c["n_mol_evaluated"]
    return {"mean_score": _ratio(c["score_micro"] / 1e6, n_mol), "mean_score_inter": _ratio(c["score_inter_micro"] / 1e6, n_mol),
            "negative_score_mol_ratio": _ratio(c["n_mol_negative_score"], n_mol), "hbond_pairs_per_mol": _ratio(c["n_hbond_pairs"], n_mol),
            "hydrophobic_pairs_per_mol": _ratio(c["n_hydrophobic_pairs"], n_mol), "close_pairs_per_mol": _ratio(c["n_close_pairs"], n_mol),
            "rotatable_per_mol": _ratio(c["n_rotatable"], n_mol), "mol_with_hbond_ratio": _ratio(c["n_mol_with_hbond"], n_mol), "counts": c}


def summarise_interactions(graph_counts, graph_terms):
    """interaction statistics of a set of molecules from their per-molecule counts and terms: see ``summarise_interaction_totals``"""
    return summarise_interaction_totals(interaction_totals(graph_counts, graph_terms))


# ---- functional groups of the table-bond graph ---------------------------------------------------------------------------------------------
# include/cbgx.h CBGX_GROUPS_MAX_ATOMS / _CLASSES / _MAX_TEMPLATE_ATOMS / _MAX_TEMPLATE_BONDS
MAX_GROUP_ATOMS, GROUP_CLASSES, MAX_GROUP_TEMPLATE_ATOMS, MAX_GROUP_TEMPLATE_BONDS = 256, 25, 10, 11
# the named classes, in the order and under the names of the reference's vocabulary (repo/tools/eval_fg_type.py); class 25 is 'other'
GROUP_NAMES = ("c1ccccc1", "NC=O", "O=CO", "c1ccncc1", "c1ncc2nc[nH]c2n1", "NS(=O)=O", "O=P(O)(O)O", "OCO", "c1cncnc1", "c1cn[nH]c1",
               "O=P(O)O", "c1ccc2ccccc2c1", "c1ccsc1", "N=CN", "NC(N)=O", "O=c1cc[nH]c(=O)[nH]1", "c1ccc2ncccc2c1", "c1cscn1",
               "c1ccc2[nH]cnc2c1", "c1c[nH]cn1", "O=[N+][O-]", "O=CNO", "NC(=O)O", "O=S=O", "c1ccc2[nH]ccc2c1")
GROUP_OTHER, GROUP_NO_GROUP, GROUP_NOT_EVALUATED = 25, 254, 255       # atom_class beside 0 ... 24 (CBGX_GROUPS_NO_GROUP)
# columns of ligand_groups' graph_counts (include/cbgx.h CBGX_GROUPS_GRAPH_COLS); fg_k: groups of class k
GROUP_GRAPH_COLUMNS = (("n_atoms", "n_bonds", "n_groups", "n_group_atoms", "n_named", "largest_group")
                       + tuple(f"fg_{k}" for k in range(GROUP_CLASSES)) + ("n_other", "status"))
GROUPS_TOO_MANY_ATOMS, GROUPS_BAD_BONDS, GROUPS_NO_AROMATIC = 1, 4, 8     # status bits: a graph with status != 0 was not evaluated


def group_name(cls):
    """the name of a class 0 ... 25"""
    return GROUP_NAMES[cls] if cls < GROUP_CLASSES else "other"


def group_templates():
    """the template graphs the library's kernel was built with (``cbgx_ligand_groups_templates``; host only), one per GROUP_NAMES entry:
    {``name``, ``labels`` [(element code 0 ... 7 = H C N O F P S Cl, aromatic bit)], ``bonds`` [(atom, atom, type 1 ... 4)]}"""
    n_atoms, n_bonds = np.zeros(GROUP_CLASSES, np.uint8), np.zeros(GROUP_CLASSES, np.uint8)
    labels = np.zeros((GROUP_CLASSES, MAX_GROUP_TEMPLATE_ATOMS), np.uint8)
    bonds = np.zeros((GROUP_CLASSES, MAX_GROUP_TEMPLATE_BONDS, 3), np.uint8)
    _native.check(_native.lib().cbgx_ligand_groups_templates(*[ctypes.c_void_p(a.ctypes.data) for a in (n_atoms, n_bonds, labels, bonds)]),
                  "cbgx_ligand_groups_templates")
    return [{"name": GROUP_NAMES[k], "labels": [(int(v) >> 1, int(v) & 1) for v in labels[k, :n_atoms[k]]],
             "bonds": [tuple(int(v) for v in row) for row in bonds[k, :n_bonds[k]]]} for k in range(GROUP_CLASSES)]


def ligand_groups(z_lig, lig_batch, n_graphs, bonds, aromatic=None):
    """Functional groups of the bond graphs of ``n_graphs`` ligands, one launch (``cbgx_ligand_groups``, csrc/groups.hip; the definition
    is in include/cbgx.h) on the tensors' current stream: members by marking rules (aromatic atoms, hetero atoms, unsaturated, acetal and
    hetero-triangle carbons), groups as the connected components of the members under the group bonds, and every group's class by an
    exact isomorphism test against the 25 template graphs of GROUP_NAMES.

    ``z_lig`` [n_lig] atomic numbers, ``lig_batch`` [n_lig] grouped by graph; ``bonds``: what ``ligand_bonds`` returned for the same atoms;
    ``aromatic``: what ``ligand_aromatic`` returned for that list, or None: no bond is aromatic ('basic' atom types).  Returns device
    tensors: ``atom_group`` [n_lig] int32 (the graph-local index of the smallest atom of the atom's group; -1: in no group),
    ``atom_class`` [n_lig] uint8 (0 ... 24, GROUP_OTHER, GROUP_NO_GROUP) and ``graph_counts`` [n_graphs, 33] int32 (GROUP_GRAPH_COLUMNS).
    A graph of more than MAX_GROUP_ATOMS atoms, with a malformed list, or that the aromatic report did not evaluate is not an error: its
    status is non-zero (GROUPS_*), its columns from n_groups to n_other are -1, its ``atom_class`` 255 and its ``atom_group`` -2.
    Deviations from the reference: table bonds and this library's aromatic bonds; marking rules of this library's own, not the EFGs
    program (nothing claims agreement with it); no charges; a single-atom group is 'other'.  There is no CPU path."""
    dev = z_lig.device
    _gpu_only(dev, "ligand_groups", "cbgx_ligand_groups")
    n_graphs = int(n_graphs)
    bond_index, bond_order = bonds["bond_index"], bonds["bond_order"]
    given = [("lig_batch", lig_batch), ("bond_index", bond_index), ("bond_order", bond_order)]
    if aromatic is not None:
        given += [("aromatic_bond", aromatic["aromatic_bond"]), ("bond_type", aromatic["bond_type"])]
    for name, t in given:
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, z_lig on {dev}")
    if bond_index.dim() != 2 or bond_index.shape[0] != 2:
        raise ValueError("bond_index must be [2, n_bonds]")
    n_lig, n_bonds = int(z_lig.shape[0]), int(bond_index.shape[1])
    if z_lig.shape != (n_lig,) or lig_batch.shape != (n_lig,):
        raise ValueError("one atomic number and one graph index per atom")
    if any(t.shape != (n_bonds,) for _, t in given[2:]):
        raise ValueError("one bond_order (and one aromatic_bond and bond_type) per bond")
    lig_ptr = _csr(lig_batch, n_graphs, "lig_batch")
    z_lig = _z_bytes(z_lig)
    bond_index, bond_ptr = bond_index.to(torch.int32).contiguous(), _bond_ptr(bond_index, n_lig)
    bond_order = bond_order.to(torch.uint8).contiguous()
    flag = None
    if aromatic is not None:      # the bytes cbgx_ligand_aromatic wrote: 0, 1, or 255 where it did not evaluate the graph
        flag = torch.where(aromatic["bond_type"] == BOND_TYPE_NOT_EVALUATED, torch.full_like(bond_order, GROUP_NOT_EVALUATED),
                           (aromatic["aromatic_bond"] != 0).to(torch.uint8)).contiguous()
    atom_group = torch.empty(n_lig, dtype=torch.int32, device=dev)
    atom_class = torch.empty(n_lig, dtype=torch.uint8, device=dev)
    graph_counts = torch.empty(n_graphs, len(GROUP_GRAPH_COLUMNS), dtype=torch.int32, device=dev)
    p = _native.ptr
    _native.check(_native.lib().cbgx_ligand_groups(p(z_lig), p(lig_ptr), n_lig, n_graphs, p(bond_ptr), p(bond_index) if n_bonds else None,
                                                   p(bond_order) if n_bonds else None, p(flag) if flag is not None and n_bonds else None,
                                                   n_bonds, p(atom_group), p(atom_class), p(graph_counts), _native.current_stream(dev)),
                  "cbgx_ligand_groups")
    return {"atom_group": atom_group, "atom_class": atom_class, "graph_counts": graph_counts}


def batch_groups(batch, x, c, lig_batch, mode, bonds=None, aromatic=None):
    """``ligand_groups`` of a sampling state; ``bonds`` / ``aromatic``: what ``batch_bonds`` / ``batch_aromatic`` returned for the same
    state.  ``bonds`` is computed here when None; so is ``aromatic`` when None and ``mode`` has aromatic atom types ('add_aromatic').  In
    any other mode there are no flags to start from and no bond is aromatic"""
    if bonds is None:
        bonds = batch_bonds(batch, x, c, lig_batch, mode)
    if aromatic is None and mode in _AROMATIC:
        aromatic = batch_aromatic(batch, x, c, lig_batch, mode, bonds=bonds)
    dev = bonds["bond_index"].device
    lig_batch = lig_batch.to(dev)
    _, z, n_graphs = _state_atoms(c, mode, lig_batch, {"num_graphs": bonds["graph_counts"].shape[0]}, dev)
    return ligand_groups(z, lig_batch, n_graphs, bonds, aromatic)


def group_names(atom_group, atom_class):
    """the names of one molecule's groups in the order of their smallest atoms ('other' included), from its ``atom_group`` /
    ``atom_class`` rows: a group is named at the atom that is its own ``atom_group``"""
    grp, cls = (np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v).reshape(-1) for v in (atom_group, atom_class))
    return [group_name(int(cls[a])) for a in range(grp.shape[0]) if int(grp[a]) == a]


GROUP_COUNT_KEYS = (("n_mol", "n_mol_evaluated", "n_mol_over_limit", "n_atoms", "n_bonds", "n_groups", "n_group_atoms", "n_named")
                    + tuple(f"n_fg_{k}" for k in range(GROUP_CLASSES)) + ("n_other", "n_mol_with_named_group"))
GROUP_RATIOS = ("groups_per_mol", "named_group_ratio", "mol_with_named_group_ratio", "group_atom_ratio")


def group_totals(graph_counts):
    """per-molecule counts ``graph_counts`` [n_mol, 33] (GROUP_GRAPH_COLUMNS; any array-like) -> the integer totals, in GROUP_COUNT_KEYS
    order.  Everything but n_mol and n_mol_over_limit is summed over the evaluated molecules (status == 0) only"""
    gc = _counts(graph_counts, GROUP_GRAPH_COLUMNS)
    ok = gc[gc[:, -1] == 0]
    return ([int(gc.shape[0]), int(ok.shape[0]), int(gc.shape[0] - ok.shape[0])] + [int(v) for v in ok[:, :5].sum(0)]
            + [int(v) for v in ok[:, 6:6 + GROUP_CLASSES + 1].sum(0)] + [int((ok[:, 4] > 0).sum())])


def summarise_group_totals(totals):
    """the substructure numbers of integer totals in GROUP_COUNT_KEYS order, over the EVALUATED molecules; a ratio over nothing is nan.
    ``fg_ratio`` {name: groups of that class / molecules} is the reference's eval_fg_type_ratio, ``fg_distribution`` {name: groups of
    that class / named groups} its eval_fg_type_distribution (all zeros without a named group); groups_per_mol; named_group_ratio: named
    groups / groups; mol_with_named_group_ratio: molecules with at least one named group / molecules; group_atom_ratio: atoms in a group /
    atoms; and the totals as ``counts``"""
    c = {k: int(v) for k, v in zip(GROUP_COUNT_KEYS, totals)}
    fg = [c[f"n_fg_{k}"] for k in range(GROUP_CLASSES)]
    n_mol, n_named = c["n_mol_evaluated"], sum(fg)
    return {"fg_ratio": {name: _ratio(v, n_mol) for name, v in zip(GROUP_NAMES, fg)},
            "fg_distribution": {name: v / n_named if n_named else 0.0 for name, v in zip(GROUP_NAMES, fg)},
            "groups_per_mol": _ratio(c["n_groups"], n_mol), "named_group_ratio": _ratio(c["n_named"], c["n_groups"]),
            "mol_with_named_group_ratio": _ratio(c["n_mol_with_named_group"], n_mol),
            "group_atom_ratio": _ratio(c["n_group_atoms"], c["n_atoms"]), "counts": c}


def summarise_groups(graph_counts):
    """functional-group statistics of a set of molecules from integer per-molecule counts (``graph_counts`` [n_mol, 33],
    GROUP_GRAPH_COLUMNS): see ``summarise_group_totals``"""
    return summarise_group_totals(group_totals(graph_counts))


def _group_vector(values, what):
    """a reference's 25 values in GROUP_NAMES order, from {name: value} or a vector"""
    if isinstance(values, dict):
        missing = [name for name in GROUP_NAMES if name not in values]
        if missing:
            raise ValueError(f"the reference {what} lacks {missing}")
        values = [values[name] for name in GROUP_NAMES]
    vec = np.asarray(values, np.float64).reshape(-1)
    if vec.shape[0] != GROUP_CLASSES:
        raise ValueError(f"the reference {what} has {vec.shape[0]} values, not {GROUP_CLASSES}")
    return vec


def groups_against(summary, reference):
    """a job's functional groups (``summarise_group_totals``) against the caller's own reference -- none ships with this package --:
    ``reference`` {'ratio': ..., 'distribution': ...}, each {name: value} over GROUP_NAMES or a 25-vector in that order.  Returns
    ``MAE_fg``, the mean absolute difference of the 25 ratios (eval_fg_type_ratio), ``JSD_fg``, ``distribution_jsd`` of the two
    distributions (eval_fg_type_distribution), and ``not_evaluated`` {key: reason} for a number that is None: no evaluated molecule has
    no ratios, and a side that sums to zero has no distribution"""
    ratio, dist = _group_vector(reference["ratio"], "ratio"), _group_vector(reference["distribution"], "distribution")
    mine_ratio = np.asarray([summary["fg_ratio"][name] for name in GROUP_NAMES], np.float64)
    mine_dist = np.asarray([summary["fg_distribution"][name] for name in GROUP_NAMES], np.float64)
    out, why = {}, {}
    if summary["counts"]["n_mol_evaluated"]:
        out["MAE_fg"] = float(np.abs(ratio - mine_ratio).mean())
    else:
        out["MAE_fg"], why["MAE_fg"] = None, "no molecule was evaluated"
    if mine_dist.sum() > 0 and dist.sum() > 0:
        out["JSD_fg"] = distribution_jsd(mine_dist, dist)
    else:
        out["JSD_fg"] = None
        why["JSD_fg"] = "no named group among the samples" if not mine_dist.sum() > 0 else "the reference distribution sums to zero"
    out["not_evaluated"] = why
    return out


# ---- fingerprints of the table-bond graph; uniqueness and similarity across the samples of a pocket ----------------------------------------
# include/cbgx.h CBGX_FINGERPRINT_MAX_ATOMS / _BITS / _WORDS, CBGX_DIVERSITY_MAX_GROUP
MAX_FINGERPRINT_ATOMS, FINGERPRINT_BITS, FINGERPRINT_WORDS, MAX_DIVERSITY_GROUP = 256, 1024, 32, 1024
# columns of ligand_fingerprints' graph_counts (CBGX_FINGERPRINT_GRAPH_COLS) and of group_diversity's group_counts (CBGX_DIVERSITY_GROUP_COLS)
FINGERPRINT_GRAPH_COLUMNS = ("n_atoms", "n_bonds", "n_bits", "n_rounds", "status")
DIVERSITY_GROUP_COLUMNS = ("n_graphs", "n_evaluated", "n_unique", "n_pairs", "sim_micro_sum", "sim_micro_max", "status")
# status bits of a graph (a graph with status != 0 was not evaluated) and of a group
FINGERPRINT_TOO_MANY_ATOMS, FINGERPRINT_BAD_BONDS, FINGERPRINT_NO_TYPES, FINGERPRINT_EMPTY = 1, 4, 8, 16
DIVERSITY_TOO_MANY_GRAPHS, DIVERSITY_BAD_GROUPS = 1, 4
SIMILARITY_ONE = 1000000                   # similarities are whole millionths


def ligand_fingerprints(z_lig, lig_batch, n_graphs, bonds, rings, aromatic=None):
    """A 1024-bit fingerprint and a 64-bit hash of the bond graphs of ``n_graphs`` ligands, one launch (``cbgx_ligand_fingerprints``,
    csrc/diversity.hip; the definition is in include/cbgx.h) on the tensors' current stream: colour refinement from (element, degree,
    aromatic, smallest ring) over the typed bonds, max(n_atoms, 2) rounds; the labels of rounds 0, 1, 2 set the bits, those of the last
    round make the hash.  Integer work only; neither depends on the order of atoms or bonds.

    ``z_lig`` [n_lig] atomic numbers, ``lig_batch`` [n_lig] grouped by graph; ``bonds`` / ``rings``: what ``ligand_bonds`` /
    ``ligand_rings`` returned for the same atoms; ``aromatic``: what ``ligand_aromatic`` returned, or None: a bond's type is its order
    ('basic' atom types).  Returns device tensors: ``fingerprint`` [n_graphs, 32] int32 (the bit patterns of uint32 words: bit b is bit
    b & 31 of word b >> 5), ``mol_hash`` [n_graphs] int64 (the bit pattern of a uint64: ``mol_hash_int`` makes the Python int) and
    ``graph_counts`` [n_graphs, 5] int32 (FINGERPRINT_GRAPH_COLUMNS).  A graph of more than MAX_FINGERPRINT_ATOMS atoms, without atoms,
    with a malformed list, or that the ring or aromatic report did not evaluate is not an error: its status is non-zero
    (FINGERPRINT_*), its fingerprint and hash are 0, n_bits and n_rounds -1.  Equal hashes mean equivalence under this refinement up to
    64-bit collisions, not a proof of isomorphism (unsubstituted macrocycles above 9 atoms of equal atom counts are a known blind spot);
    a fingerprint of this library's own in the manner of ECFP4: neither RDKit's Morgan fingerprint nor ``RDKFingerprint``, and nothing
    claims agreement with them.  There is no CPU path."""
    dev = z_lig.device
    _gpu_only(dev, "ligand_fingerprints", "cbgx_ligand_fingerprints")
    n_graphs = int(n_graphs)
    bond_index, ring_min = bonds["bond_index"], rings["atom_ring_min"]
    bond_type = bonds["bond_order"] if aromatic is None else aromatic["bond_type"]
    for name, t in (("lig_batch", lig_batch), ("bond_index", bond_index), ("bond_type", bond_type), ("atom_ring_min", ring_min)):
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, z_lig on {dev}")
    if bond_index.dim() != 2 or bond_index.shape[0] != 2:
        raise ValueError("bond_index must be [2, n_bonds]")
    n_lig, n_bonds = int(z_lig.shape[0]), int(bond_index.shape[1])
    if z_lig.shape != (n_lig,) or lig_batch.shape != (n_lig,) or ring_min.shape != (n_lig,):
        raise ValueError("one atomic number, one graph index and one atom_ring_min per atom")
    if bond_type.shape != (n_bonds,):
        raise ValueError("one bond type per bond")
    lig_ptr = _csr(lig_batch, n_graphs, "lig_batch")
    z_lig = _z_bytes(z_lig)
    bond_index, bond_ptr = bond_index.to(torch.int32).contiguous(), _bond_ptr(bond_index, n_lig)
    bond_type, ring_min = bond_type.to(torch.uint8).contiguous(), ring_min.to(torch.uint8).contiguous()
    fp = torch.empty(n_graphs, FINGERPRINT_WORDS, dtype=torch.int32, device=dev)
    mol_hash = torch.empty(n_graphs, dtype=torch.int64, device=dev)
    graph_counts = torch.empty(n_graphs, len(FINGERPRINT_GRAPH_COLUMNS), dtype=torch.int32, device=dev)
    p = _native.ptr
    _native.check(_native.lib().cbgx_ligand_fingerprints(p(z_lig), p(lig_ptr), n_lig, n_graphs, p(bond_ptr),
                                                         p(bond_index) if n_bonds else None, p(bond_type) if n_bonds else None,
                                                         p(ring_min), n_bonds, p(fp), p(mol_hash), p(graph_counts),
                                                         _native.current_stream(dev)), "cbgx_ligand_fingerprints")
    return {"fingerprint": fp, "mol_hash": mol_hash, "graph_counts": graph_counts}


def group_pair_ptr(group_ptr, n_graphs):
    """[P + 1] list of ints: n (n - 1) / 2 pairs per group, n the size of the group's range as the kernel clamps it"""
    ptr = [0]
    for a, b in zip(group_ptr[:-1], group_ptr[1:]):
        g0 = min(max(int(a), 0), n_graphs)
        n = min(max(int(b), g0), n_graphs) - g0
        ptr.append(ptr[-1] + n * (n - 1) // 2)
    return ptr


def group_diversity(fingerprints, group_ptr):
    """What the graphs of every group share, one launch (``cbgx_group_diversity``, csrc/diversity.hip; one workgroup per group):
    ``fingerprints``: what ``ligand_fingerprints`` returned; ``group_ptr`` [P + 1] ints, a CSR over graphs: group p is the consecutive
    graphs group_ptr[p] ... group_ptr[p + 1] (the samples of a pocket).  Returns device tensors: ``pair_sim`` [sum n_p (n_p - 1) / 2]
    int32, the Tanimoto similarity in millionths of every pair i < j of a group in (i, j) order (-1 where either graph was not
    evaluated), with ``pair_ptr`` [P + 1] int64 and ``group_ptr`` [P + 1] int32 as handed to the kernel; per graph ``first_same`` (the
    group-local index of the first evaluated graph of the group with the same hash), ``nearest`` (that of the most similar other
    evaluated graph, the smallest on ties; -1: none) and ``nearest_micro`` [n_graphs] int32, all three -1 for a graph that was not
    evaluated or is in no group; ``group_counts`` [P, 7] int64 (DIVERSITY_GROUP_COLUMNS).  A group of more than MAX_DIVERSITY_GROUP
    graphs is not an error: status DIVERSITY_TOO_MANY_GRAPHS, -1 in its columns from n_evaluated to sim_micro_max, in its graphs and in
    its pairs; entries of ``group_ptr`` outside [0, n_graphs] or decreasing are clamped and reported (DIVERSITY_BAD_GROUPS).  There is
    no CPU path."""
    fp, mol_hash, gc = fingerprints["fingerprint"], fingerprints["mol_hash"], fingerprints["graph_counts"]
    dev = fp.device
    _gpu_only(dev, "group_diversity", "cbgx_group_diversity")
    n_graphs = int(fp.shape[0])
    if fp.shape != (n_graphs, FINGERPRINT_WORDS) or mol_hash.shape != (n_graphs,) or gc.shape != (n_graphs, len(FINGERPRINT_GRAPH_COLUMNS)):
        raise ValueError("one fingerprint row, one hash and one row of counts per graph")
    ptr = [int(v) for v in (group_ptr.tolist() if isinstance(group_ptr, (torch.Tensor, np.ndarray)) else group_ptr)]
    if not ptr or any(not -2 ** 31 <= v < 2 ** 31 for v in ptr):
        raise ValueError("group_ptr must be [P + 1] 32-bit integers")
    n_groups, pairs = len(ptr) - 1, group_pair_ptr(ptr, n_graphs)
    group_ptr = torch.tensor(ptr, dtype=torch.int32, device=dev)
    pair_ptr = torch.tensor(pairs, dtype=torch.int64, device=dev)
    fp, mol_hash = fp.to(torch.int32).contiguous(), mol_hash.to(torch.int64).contiguous()
    status = gc[:, -1].to(torch.int32).contiguous()
    pair_sim = torch.full((pairs[-1],), -1, dtype=torch.int32, device=dev)
    first_same, nearest, nearest_micro = (torch.full((n_graphs,), -1, dtype=torch.int32, device=dev) for _ in range(3))
    group_counts = torch.empty(n_groups, len(DIVERSITY_GROUP_COLUMNS), dtype=torch.int64, device=dev)
    p = _native.ptr
    some = lambda t: p(t) if t.numel() else None
    _native.check(_native.lib().cbgx_group_diversity(some(fp), some(mol_hash), some(status), p(group_ptr), p(pair_ptr), n_graphs, n_groups,
                                                     pairs[-1], some(pair_sim), some(first_same), some(nearest), some(nearest_micro),
                                                     some(group_counts), _native.current_stream(dev)), "cbgx_group_diversity")
    return {"pair_sim": pair_sim, "pair_ptr": pair_ptr, "group_ptr": group_ptr, "first_same": first_same, "nearest": nearest,
            "nearest_micro": nearest_micro, "group_counts": group_counts}


def batch_diversity(batch, x, c, lig_batch, mode, group_ptr, bonds=None, rings=None, aromatic=None):
    """``ligand_fingerprints`` and ``group_diversity`` of a sampling state whose graphs group_ptr[p] ... group_ptr[p + 1] are the samples
    of pocket p, as one dict; ``bonds`` / ``rings`` / ``aromatic``: what ``batch_bonds`` / ``batch_rings`` / ``batch_aromatic`` returned
    for the same state.  ``bonds`` and ``rings`` are computed here when None; so is ``aromatic`` when None and ``mode`` has aromatic atom
    types ('add_aromatic'), the only mode in which it is used: in any other a bond's type is its order"""
    if bonds is None:
        bonds = batch_bonds(batch, x, c, lig_batch, mode)
    if rings is None:
        rings = batch_rings(batch, x, c, lig_batch, mode, bonds=bonds)
    if mode not in _AROMATIC:
        aromatic = None
    elif aromatic is None:
        aromatic = batch_aromatic(batch, x, c, lig_batch, mode, bonds=bonds, rings=rings)
    dev = bonds["bond_index"].device
    lig_batch = lig_batch.to(dev)
    _, z, n_graphs = _state_atoms(c, mode, lig_batch, {"num_graphs": bonds["graph_counts"].shape[0]}, dev)
    fingerprints = ligand_fingerprints(z, lig_batch, n_graphs, bonds, rings, aromatic)
    return {**fingerprints, **group_diversity(fingerprints, group_ptr)}


def mol_hash_int(value):
    """a ``mol_hash`` element (an int64 bit pattern) as the Python int 0 ... 2**64 - 1 it stands for"""
    return int(value) & (2 ** 64 - 1)


def tanimoto_micro(fp_a, fp_b):
    """host helper: the Tanimoto similarity in millionths of two fingerprints ([32] words, as ``fingerprint`` rows or any integers
    holding their bit patterns), (popcount(a & b) 1000000 + popcount(a | b) // 2) // popcount(a | b) as the kernel computes it; 0 if
    neither has a bit.  For samples of different pockets, or a reference ligand of the caller's own"""
    a, b = ([int(v) & 0xFFFFFFFF for v in (w.tolist() if hasattr(w, "tolist") else w)] for w in (fp_a, fp_b))
    if len(a) != FINGERPRINT_WORDS or len(b) != FINGERPRINT_WORDS:
        raise ValueError(f"a fingerprint has {FINGERPRINT_WORDS} words")
    inter, uni = sum(bin(x & y).count("1") for x, y in zip(a, b)), sum(bin(x | y).count("1") for x, y in zip(a, b))
    return (inter * SIMILARITY_ONE + uni // 2) // uni if uni else 0


def similarity_matrix(pair_sim, evaluated):
    """a group's pairs (its range of ``pair_sim``, (i, j) order) and which of its n graphs were evaluated -> [n, n] int32: symmetric,
    SIMILARITY_ONE on the diagonal of an evaluated graph, -1 in the rows and columns of the others"""
    n = len(evaluated)
    out = torch.full((n, n), -1, dtype=torch.int32)
    upper = torch.triu_indices(n, n, offset=1)
    out[upper[0], upper[1]] = torch.as_tensor(pair_sim, dtype=torch.int32)
    out[upper[1], upper[0]] = out[upper[0], upper[1]]
    for i, ok in enumerate(evaluated):
        if ok:
            out[i, i] = SIMILARITY_ONE
    return out


DIVERSITY_POCKET_KEYS = ("n_mol", "n_mol_evaluated", "n_unique", "n_pairs", "sim_micro_sum", "diversity_micro")
DIVERSITY_COUNT_KEYS = ("n_pockets", "n_mol", "n_mol_evaluated", "n_mol_over_limit", "n_unique", "n_pairs", "sim_micro_sum",
                        "n_pockets_with_pair", "diversity_micro_sum", "n_pockets_with_two", "n_collapsed_pockets")
DIVERSITY_RATIOS = ("unique_mol_ratio", "duplicate_mol_ratio", "mean_pair_similarity", "mean_pocket_diversity", "collapsed_pocket_ratio")


def diversity_counts(group_row):
    """one row of ``group_counts`` -> the pocket's dict of integers (DIVERSITY_POCKET_KEYS): diversity_micro = 1000000 - (sim_micro_sum
    + n_pairs // 2) // n_pairs, one minus the mean pair similarity in millionths, -1 without a pair; a group over the limit has no
    evaluated molecule"""
    row = dict(zip(DIVERSITY_GROUP_COLUMNS, (int(v) for v in group_row)))
    if row["status"] & DIVERSITY_TOO_MANY_GRAPHS:
        row.update(n_evaluated=0, n_unique=0, n_pairs=0, sim_micro_sum=0)
    n_pairs, total = row["n_pairs"], row["sim_micro_sum"]
    return {"n_mol": row["n_graphs"], "n_mol_evaluated": row["n_evaluated"], "n_unique": row["n_unique"], "n_pairs": n_pairs,
            "sim_micro_sum": total, "diversity_micro": SIMILARITY_ONE - (total + n_pairs // 2) // n_pairs if n_pairs else -1}


def diversity_totals(group_counts):
    """per-pocket rows ``group_counts`` [P, 7] (DIVERSITY_GROUP_COLUMNS; any array-like) -> the integer totals, in DIVERSITY_COUNT_KEYS
    order: what ranks add up.  n_pockets_with_pair and diversity_micro_sum run over the pockets with a pair of evaluated molecules,
    n_pockets_with_two counts those with at least two evaluated molecules and n_collapsed_pockets those of them with one distinct hash"""
    totals = [0] * len(DIVERSITY_COUNT_KEYS)
    for row in _counts(group_counts, DIVERSITY_GROUP_COLUMNS):
        c = diversity_counts(row)
        two, pair = c["n_mol_evaluated"] >= 2, c["n_pairs"] > 0
        add = [1, c["n_mol"], c["n_mol_evaluated"], c["n_mol"] - c["n_mol_evaluated"], c["n_unique"], c["n_pairs"], c["sim_micro_sum"],
               int(pair), c["diversity_micro"] if pair else 0, int(two), int(two and c["n_unique"] == 1)]
        totals = [a + b for a, b in zip(totals, add)]
    return totals


def summarise_diversity_totals(totals):
    """the job's numbers from integer totals in DIVERSITY_COUNT_KEYS order; a ratio over nothing is nan.  unique_mol_ratio: distinct
    hashes per pocket, summed, / evaluated molecules; duplicate_mol_ratio: the rest; mean_pair_similarity: over all pairs of the job;
    mean_pocket_diversity: the mean over the pockets with a pair of 1 - the pocket's mean pair similarity, the per-pocket average papers
    print; collapsed_pocket_ratio: pockets with one distinct hash among those with at least two evaluated molecules; and the totals as
    ``counts``.  Uniqueness is per pocket: the same molecule in two pockets counts twice.  Hashes are equivalence under colour
    refinement, not isomorphism; the fingerprint is this library's own, not RDKit's"""
    c = {k: int(v) for k, v in zip(DIVERSITY_COUNT_KEYS, totals)}
    return {"unique_mol_ratio": _ratio(c["n_unique"], c["n_mol_evaluated"]),
            "duplicate_mol_ratio": _ratio(c["n_mol_evaluated"] - c["n_unique"], c["n_mol_evaluated"]),
            "mean_pair_similarity": _ratio(c["sim_micro_sum"], SIMILARITY_ONE * c["n_pairs"]),
            "mean_pocket_diversity": _ratio(c["diversity_micro_sum"], SIMILARITY_ONE * c["n_pockets_with_pair"]),
            "collapsed_pocket_ratio": _ratio(c["n_collapsed_pockets"], c["n_pockets_with_two"]),
            "n_mol_over_limit": c["n_mol_over_limit"], "counts": c}


def summarise_diversity(group_counts):
    """uniqueness and diversity of a set of pockets from their integer rows (``group_counts`` [P, 7], DIVERSITY_GROUP_COLUMNS): see
    ``summarise_diversity_totals``"""
    return summarise_diversity_totals(diversity_totals(group_counts))


# ---- samples against the ligand a pocket was crystallised with -------------------------------------------------------------------------------
CONTACTS_CUTOFF2 = 16.0                    # include/cbgx.h CBGX_CONTACTS_CUTOFF2: (4 A)^2
# columns of pocket_contacts' graph_counts (CBGX_CONTACTS_GRAPH_COLS), of native_compare's sample_counts and group_counts
CONTACTS_GRAPH_COLUMNS = ("n_atoms", "n_heavy", "n_rec", "n_rec_contact", "n_lig_contact", "status")
NATIVE_SAMPLE_COLUMNS = ("sim_micro", "same_hash", "contact_common", "contact_union", "contact_micro", "status")
NATIVE_GROUP_COLUMNS = ("n_graphs", "n_fp_compared", "n_same_hash", "sim_micro_sum", "sim_micro_max", "n_contact_compared",
                        "contact_micro_sum", "contact_micro_max", "status")
CONTACTS_EMPTY = 16
NATIVE_SAMPLE_NOT_EVALUATED, NATIVE_NATIVE_NOT_EVALUATED, NATIVE_POCKET_MISMATCH, NATIVE_BAD_GROUPS = 1, 2, 4, 8


def pocket_contacts(x_lig, z_lig, lig_batch, x_rec, z_rec, rec_batch, n_graphs, cutoff2=CONTACTS_CUTOFF2):
    """Which heavy pocket atoms the heavy atoms of ``n_graphs`` ligands touch, one launch (``cbgx_pocket_contacts``, csrc/native.hip; the
    definition is in include/cbgx.h) on the tensors' current stream.  Both sides as ``ligand_geometry`` takes them.  A heavy ligand atom
    and a heavy pocket atom (atomic number not 1) are in contact iff d2 <= ``cutoff2`` with the float64 squared distance of
    ``ligand_geometry``.  Returns device tensors: ``rec_contact`` [n_rec] / ``lig_contact`` [n_lig] uint8, ``centroid`` [n_graphs, 3]
    float64 (the heavy atoms' coordinates summed in atom order, divided by their number; nan without one), ``graph_counts`` [n_graphs, 6]
    int32 (CONTACTS_GRAPH_COLUMNS; status CONTACTS_EMPTY without a heavy atom, never an error) and ``rec_ptr`` [n_graphs + 1] int32.  A
    ligand of more than MAX_LIGAND_ATOMS atoms raises ValueError.  A descriptor of this library's own.  There is no CPU path."""
    dev = x_lig.device
    _gpu_only(dev, "pocket_contacts", "cbgx_pocket_contacts")
    n_graphs = int(n_graphs)
    n_lig, lig_ptr, x_lig, z_lig = _ligand_arrays(x_lig, z_lig, lig_batch, n_graphs)
    n_rec, rec_ptr, x_rec, z_rec = _ligand_arrays(x_rec, z_rec, rec_batch, n_graphs, "rec", dev)
    rec_contact = torch.empty(n_rec, dtype=torch.uint8, device=dev)
    lig_contact = torch.empty(n_lig, dtype=torch.uint8, device=dev)
    centroid = torch.empty(n_graphs, 3, dtype=torch.float64, device=dev)
    graph_counts = torch.empty(n_graphs, len(CONTACTS_GRAPH_COLUMNS), dtype=torch.int32, device=dev)
    p = _native.ptr
    some = lambda t: p(t) if t.numel() else None
    _native.check(_native.lib().cbgx_pocket_contacts(some(x_lig), some(z_lig), p(lig_ptr), n_lig, some(x_rec), some(z_rec), p(rec_ptr),
                                                     n_rec, n_graphs, float(cutoff2), some(rec_contact), some(lig_contact),
                                                     some(centroid), some(graph_counts), _native.current_stream(dev)),
                  "cbgx_pocket_contacts")
    return {"rec_contact": rec_contact, "lig_contact": lig_contact, "centroid": centroid, "graph_counts": graph_counts, "rec_ptr": rec_ptr}


def native_compare(fingerprints, contacts, native_fingerprints, native_contacts, group_ptr):
    """Every sample of a pocket against the pocket's native ligand, one launch (``cbgx_native_compare``, csrc/native.hip; one workgroup
    per pocket).  ``fingerprints`` / ``contacts``: what ``ligand_fingerprints`` / ``pocket_contacts`` returned for the B sample graphs;
    ``native_fingerprints`` / ``native_contacts``: the same for the P native ligands, one graph per pocket; ``group_ptr`` [P + 1] ints:
    the samples of pocket p are the graphs group_ptr[p] ... group_ptr[p + 1].  Returns device tensors: ``sample_counts`` [B, 6] int64
    (NATIVE_SAMPLE_COLUMNS: the Tanimoto similarity in millionths as ``tanimoto_micro`` computes it, equal hash, the pocket atoms both
    touch, those either touches, their quotient in millionths by the same rounding, status), ``centroid_d2`` [B] float64 and
    ``group_counts`` [P, 9] int64 (NATIVE_GROUP_COLUMNS), with ``group_ptr`` as handed to the kernel.  Nothing is an error: a fingerprint
    that was not evaluated on either side gives -1 in sim_micro and same_hash, pocket ranges of different lengths -1 in the contact
    columns, each with its status bit (NATIVE_*); a graph in no group keeps -1 in every column and nan.  There is no CPU path."""
    fp, mol_hash, fgc = fingerprints["fingerprint"], fingerprints["mol_hash"], fingerprints["graph_counts"]
    dev = fp.device
    _gpu_only(dev, "native_compare", "cbgx_native_compare")
    n_graphs, n_rec = int(fp.shape[0]), int(contacts["rec_contact"].shape[0])
    ptr = [int(v) for v in (group_ptr.tolist() if isinstance(group_ptr, (torch.Tensor, np.ndarray)) else group_ptr)]
    if not ptr or any(not -2 ** 31 <= v < 2 ** 31 for v in ptr):
        raise ValueError("group_ptr must be [P + 1] 32-bit integers")
    n_groups, n_rec_nat = len(ptr) - 1, int(native_contacts["rec_contact"].shape[0])
    for what, n, f, k in (("sample", n_graphs, fingerprints, contacts), ("native", n_groups, native_fingerprints, native_contacts)):
        if (f["fingerprint"].shape != (n, FINGERPRINT_WORDS) or f["mol_hash"].shape != (n,)
                or f["graph_counts"].shape != (n, len(FINGERPRINT_GRAPH_COLUMNS)) or k["centroid"].shape != (n, 3)
                or k["graph_counts"].shape != (n, len(CONTACTS_GRAPH_COLUMNS)) or k["rec_ptr"].shape != (n + 1,)):
            raise ValueError(f"one fingerprint row, hash, centroid and row of counts per {what} graph ({n}), and a rec_ptr of one more")
        for name, t in list(f.items()) + list(k.items()):
            if isinstance(t, torch.Tensor) and t.device != dev:
                raise ValueError(f"{what} {name} is on {t.device}, the fingerprints on {dev}")

    def side(f, k):
        return (f["fingerprint"].to(torch.int32).contiguous(), f["mol_hash"].to(torch.int64).contiguous(),
                f["graph_counts"][:, -1].to(torch.int32).contiguous(), k["rec_contact"].to(torch.uint8).contiguous(),
                k["rec_ptr"].to(torch.int32).contiguous(), k["centroid"].to(torch.float64).contiguous(),
                k["graph_counts"][:, -1].to(torch.int32).contiguous())

    mine, theirs = side(fingerprints, contacts), side(native_fingerprints, native_contacts)
    group_ptr = torch.tensor(ptr, dtype=torch.int32, device=dev)
    sample_counts = torch.full((n_graphs, len(NATIVE_SAMPLE_COLUMNS)), -1, dtype=torch.int64, device=dev)
    centroid_d2 = torch.full((n_graphs,), float("nan"), dtype=torch.float64, device=dev)
    group_counts = torch.empty(n_groups, len(NATIVE_GROUP_COLUMNS), dtype=torch.int64, device=dev)
    p = _native.ptr
    some = lambda t: p(t) if t.numel() else None
    _native.check(_native.lib().cbgx_native_compare(
        *[some(t) if i != 4 else p(t) for i, t in enumerate(mine)], n_graphs, n_rec,
        *[some(t) if i != 4 else p(t) for i, t in enumerate(theirs)], n_groups, n_rec_nat, p(group_ptr), some(sample_counts),
        some(centroid_d2), some(group_counts), _native.current_stream(dev)), "cbgx_native_compare")
    return {"sample_counts": sample_counts, "centroid_d2": centroid_d2, "group_counts": group_counts, "group_ptr": group_ptr}


_NATIVE_DEPS = ("bonds", "rings", "aromatic", "valence", "interactions", "diversity")


def _native_deps(batch, x, c, lig_batch, mode, group_ptr, given):
    """the reports ``batch_native`` reads of one state, in ``given`` (computed where None): bonds, rings, aromatic (with aromatic atom
    types only), valence, interactions and the fingerprints of ``batch_diversity``"""
    made = {k: given.get(k) for k in _NATIVE_DEPS}
    if made["bonds"] is None:
        made["bonds"] = batch_bonds(batch, x, c, lig_batch, mode)
    if made["rings"] is None:
        made["rings"] = batch_rings(batch, x, c, lig_batch, mode, bonds=made["bonds"])
    if mode not in _AROMATIC:
        made["aromatic"] = None
    elif made["aromatic"] is None:
        made["aromatic"] = batch_aromatic(batch, x, c, lig_batch, mode, bonds=made["bonds"], rings=made["rings"])
    if made["valence"] is None:
        made["valence"] = batch_valence(batch, x, c, lig_batch, mode, bonds=made["bonds"], aromatic=made["aromatic"])
    if made["interactions"] is None:
        made["interactions"] = batch_interactions(batch, x, c, lig_batch, mode, bonds=made["bonds"], valence=made["valence"])
    if made["diversity"] is None:
        made["diversity"] = batch_diversity(batch, x, c, lig_batch, mode, group_ptr, bonds=made["bonds"], rings=made["rings"],
                                            aromatic=made["aromatic"])
    return made


def batch_native(batch, x, c, lig_batch, mode, group_ptr, native_state, bonds=None, rings=None, aromatic=None, valence=None,
                 interactions=None, diversity=None):
    """A sampling state whose graphs group_ptr[p] ... group_ptr[p + 1] are the samples of pocket p against the P native ligands of
    ``native_state``: a dict with ``x`` [n_nat, 3], ``c`` (type indices of ``mode``) and ``lig_batch`` of a state of P graphs, ``batch``
    (the P pocket copies those graphs sit in: the keys ``batch_interactions`` reads, in the frame of ``x``) and, optionally, under the
    names of the keyword arguments what the ``batch_*`` functions returned for that state.  ``bonds`` ... ``diversity``: the same for the
    sample state; whatever is None is computed here, for the native state by the same functions (its fingerprints with groups of one).
    Two ``pocket_contacts`` launches and one ``native_compare`` on top.  Returns one dict of device tensors: ``sample_counts``,
    ``centroid_d2``, ``group_counts``, ``group_ptr`` (``native_compare``); ``rec_contact``, ``lig_contact``, ``centroid``,
    ``contact_counts``, ``rec_ptr`` (``pocket_contacts`` of the samples); ``interaction_counts`` / ``interaction_terms`` (the samples'
    rows of ``ligand_interactions``, from which ``interaction_scores`` makes the scores); and the same seven of the native ligands under
    ``native_`` + name."""
    ptr = [int(v) for v in (group_ptr.tolist() if isinstance(group_ptr, (torch.Tensor, np.ndarray)) else group_ptr)]
    n_groups = len(ptr) - 1
    mine = _native_deps(batch, x, c, lig_batch, mode, ptr, {"bonds": bonds, "rings": rings, "aromatic": aromatic, "valence": valence,
                                                            "interactions": interactions, "diversity": diversity})
    dev = mine["bonds"]["bond_index"].device
    nat_batch = {**{k: v.to(dev) if isinstance(v, torch.Tensor) else v for k, v in native_state["batch"].items()}, "num_graphs": n_groups}
    nx, nc, nb = native_state["x"].to(dev), native_state["c"].to(dev), native_state["lig_batch"].to(dev)
    theirs = _native_deps(nat_batch, nx, nc, nb, mode, list(range(n_groups + 1)), native_state)
    out = {}
    for prefix, made, (bt, xs, cs, lb, n) in (("", mine, (batch, x.to(dev), c, lig_batch.to(dev), mine["bonds"]["graph_counts"].shape[0])),
                                              ("native_", theirs, (nat_batch, nx, nc, nb, n_groups))):
        _, z, _ = _state_atoms(cs, mode, lb, {"num_graphs": n}, dev)
        x_rec, z_rec, rec_b = (bt[k].to(dev) for k in ("protein_pos", "protein_element", "protein_element_batch"))
        made["contacts"] = pocket_contacts(xs, z, lb, x_rec, z_rec, rec_b, n)
        for k in ("rec_contact", "lig_contact", "centroid", "rec_ptr"):
            out[prefix + k] = made["contacts"][k]
        out[prefix + "contact_counts"] = made["contacts"]["graph_counts"]
        out[prefix + "interaction_counts"] = made["interactions"]["graph_counts"]
        out[prefix + "interaction_terms"] = made["interactions"]["graph_terms"]
    out.update(native_compare(mine["diversity"], mine["contacts"], theirs["diversity"], theirs["contacts"], ptr))
    return out


def _half_up_micro(value):
    """a float rounded half up to whole millionths, None where it is not finite"""
    return int(np.floor(value * 1e6 + 0.5)) if np.isfinite(value) else None


NATIVE_EVALUATED, NATIVE_POSITIVE_NATIVE, NATIVE_NO_NATIVE_SCORE, NATIVE_NO_SAMPLE = 0, 1, 2, 3


def native_pocket_metrics(score_micro_samples, n_heavy_samples, score_micro_native):
    """``calculate_vina_metrics`` (the reference's evaluate_scripts/cal_chem_results.py:51-67) of one pocket, restated on this library's
    score: ``score_micro_samples``: the samples' ``score_micro`` integers (None: not evaluated), ``n_heavy_samples``: their heavy-atom
    counts, ``score_micro_native``: that of the native ligand (None: not evaluated).  With vina = score_micro / 1e6 of the evaluated
    samples with a heavy atom and ref = the native's: binding_gap = mean((vina - ref) / ref) 100 (MPBG, in percent as the reference
    prints it), improved_ratio = the share of samples with vina < ref (strictly; IMP / 100), mean_score = mean(vina),
    ligand_efficiency = mean(vina / n_heavy) (LBE, the reference's sign), all in float64 numpy arithmetic as the reference writes
    them; a native score of 0 divides by zero as it does there.  ``skipped``: NATIVE_EVALUATED, or why the four are nan:
    NATIVE_POSITIVE_NATIVE (ref > 0, the reference's condition), NATIVE_NO_NATIVE_SCORE, NATIVE_NO_SAMPLE.  Each of the four also
    rounded half up to whole millionths (``*_micro``; None where nan or infinite): what ranks add up.  n_scored, n_improved and
    native_score_micro are carried along.  A score in Vina's functional form on this library's typing, not the Vina program."""
    pairs = [(int(s), int(n)) for s, n in zip(score_micro_samples, n_heavy_samples) if s is not None and int(n) > 0]
    out = {"skipped": NATIVE_EVALUATED, "n_scored": len(pairs), "n_improved": 0,
           "native_score_micro": None if score_micro_native is None else int(score_micro_native)}
    names = ("binding_gap", "improved_ratio", "mean_score", "ligand_efficiency")
    if score_micro_native is None:
        out["skipped"] = NATIVE_NO_NATIVE_SCORE
    elif int(score_micro_native) > 0:
        out["skipped"] = NATIVE_POSITIVE_NATIVE
    elif not pairs:
        out["skipped"] = NATIVE_NO_SAMPLE
    if out["skipped"] != NATIVE_EVALUATED:
        out.update({k: float("nan") for k in names}, **{k + "_micro": None for k in names})
        return out
    vina = np.array([s for s, _ in pairs], np.int64) / 1e6
    atom_num = np.array([n for _, n in pairs], np.int64)
    ref = int(score_micro_native) / 1e6
    with np.errstate(divide="ignore", invalid="ignore"):
        values = (float(np.mean((vina - ref) / ref) * 100), float((vina < ref).sum() / len(vina)), float(np.mean(vina)),
                  float(np.mean(vina / atom_num)))
    out["n_improved"] = int((vina < ref).sum())
    out.update(zip(names, values), **{k + "_micro": _half_up_micro(v) for k, v in zip(names, values)})
    return out


NATIVE_POCKET_KEYS = (("n_mol",) + NATIVE_GROUP_COLUMNS[1:] + ("skipped", "n_scored", "n_improved", "native_score_micro", "binding_gap_micro",
                      "improved_ratio_micro", "mean_score_micro", "ligand_efficiency_micro"))
NATIVE_COUNT_KEYS = ("n_pockets", "n_pockets_evaluated", "n_pockets_positive_native", "n_pockets_native_not_evaluated",
                     "n_pockets_no_sample", "n_pockets_with_gap", "binding_gap_micro_sum", "improved_ratio_micro_sum",
                     "mean_score_micro_sum", "native_score_micro_sum", "ligand_efficiency_micro_sum", "n_mol", "n_mol_scored",
                     "n_mol_improved", "n_fp_compared", "n_same_hash", "sim_micro_sum", "n_contact_compared", "contact_micro_sum",
                     "n_pockets_fp_compared", "n_pockets_with_rediscovery")
NATIVE_RATIOS = ("improved_mol_ratio", "mean_binding_gap", "mean_score", "mean_native_score", "mean_ligand_efficiency",
                 "mean_native_similarity", "rediscovered_mol_ratio", "mean_contact_jaccard", "pockets_with_rediscovery_ratio")


def native_pocket_counts(group_row, metrics):
    """one row of ``native_compare``'s group_counts and the pocket's ``native_pocket_metrics`` -> the pocket's ``native_comparison``
    dict (NATIVE_POCKET_KEYS): integers, None for a number the pocket does not have"""
    row = dict(zip(NATIVE_GROUP_COLUMNS, (int(v) for v in group_row)))
    out = {"n_mol": row.pop("n_graphs"), **row}
    out.update({k: metrics[k] for k in NATIVE_POCKET_KEYS[len(NATIVE_GROUP_COLUMNS):]})
    return out


def native_totals(pockets):
    """the pockets' ``native_comparison`` dicts -> the integer totals, in NATIVE_COUNT_KEYS order: what ranks add up.  The sums of the
    four metrics and of the native score run over the evaluated pockets (skipped == NATIVE_EVALUATED); the binding gap, which a native
    score of exactly 0 makes infinite, over those of them where it is finite (n_pockets_with_gap)"""
    t = dict.fromkeys(NATIVE_COUNT_KEYS, 0)
    for c in pockets:
        t["n_pockets"] += 1
        for code, key in ((NATIVE_EVALUATED, "n_pockets_evaluated"), (NATIVE_POSITIVE_NATIVE, "n_pockets_positive_native"),
                          (NATIVE_NO_NATIVE_SCORE, "n_pockets_native_not_evaluated"), (NATIVE_NO_SAMPLE, "n_pockets_no_sample")):
            t[key] += int(c["skipped"] == code)
        if c["skipped"] == NATIVE_EVALUATED:
            if c["binding_gap_micro"] is not None:
                t["n_pockets_with_gap"] += 1
                t["binding_gap_micro_sum"] += c["binding_gap_micro"]
            for k in ("improved_ratio", "mean_score", "ligand_efficiency"):
                t[k + "_micro_sum"] += c[k + "_micro"]
            t["native_score_micro_sum"] += c["native_score_micro"]
            t["n_mol_scored"] += c["n_scored"]
            t["n_mol_improved"] += c["n_improved"]
        for k in ("n_mol", "n_fp_compared", "n_same_hash", "sim_micro_sum", "n_contact_compared", "contact_micro_sum"):
            t[k] += c[k]
        t["n_pockets_fp_compared"] += int(c["n_fp_compared"] > 0)
        t["n_pockets_with_rediscovery"] += int(c["n_same_hash"] > 0)
    return [t[k] for k in NATIVE_COUNT_KEYS]


def summarise_native_totals(totals):
    """the job's numbers (NATIVE_RATIOS) from integer totals in NATIVE_COUNT_KEYS order; a ratio over nothing is nan.  The first five are
    per-pocket averages over the evaluated pockets, as the reference averages (cal_chem_results.py:110-117): improved_mol_ratio (IMP as
    a ratio, not in percent), mean_binding_gap (MPBG, in percent; over the pockets with a finite gap), mean_score, mean_native_score,
    mean_ligand_efficiency (LBE).  mean_native_similarity and rediscovered_mol_ratio (equal hash) run over the samples whose
    fingerprint was compared, mean_contact_jaccard over those whose contacts were, pockets_with_rediscovery_ratio over the pockets with
    a compared sample.  The reference's formulas on this library's score in Vina's functional form, not Vina's; a fingerprint of this
    library's own, not RDKit's; the contact Jaccard index is a descriptor of this library's own"""
    c = {k: int(v) for k, v in zip(NATIVE_COUNT_KEYS, totals)}
    n = c["n_pockets_evaluated"]
    return {"improved_mol_ratio": _ratio(c["improved_ratio_micro_sum"], SIMILARITY_ONE * n),
            "mean_binding_gap": _ratio(c["binding_gap_micro_sum"], SIMILARITY_ONE * c["n_pockets_with_gap"]),
            "mean_score": _ratio(c["mean_score_micro_sum"], SIMILARITY_ONE * n),
            "mean_native_score": _ratio(c["native_score_micro_sum"], SIMILARITY_ONE * n),
            "mean_ligand_efficiency": _ratio(c["ligand_efficiency_micro_sum"], SIMILARITY_ONE * n),
            "mean_native_similarity": _ratio(c["sim_micro_sum"], SIMILARITY_ONE * c["n_fp_compared"]),
            "rediscovered_mol_ratio": _ratio(c["n_same_hash"], c["n_fp_compared"]),
            "mean_contact_jaccard": _ratio(c["contact_micro_sum"], SIMILARITY_ONE * c["n_contact_compared"]),
            "pockets_with_rediscovery_ratio": _ratio(c["n_pockets_with_rediscovery"], c["n_pockets_fp_compared"]),
            "n_pockets_positive_native": c["n_pockets_positive_native"],
            "n_pockets_native_not_evaluated": c["n_pockets_native_not_evaluated"], "n_pockets_no_sample": c["n_pockets_no_sample"],
            "counts": c}


def summarise_native(pockets):
    """the comparison with the native ligands of a set of pockets from their ``native_comparison`` dicts: see
    ``summarise_native_totals``"""
    return summarise_native_totals(native_totals(pockets))


# the five reports that are integer counts per molecule, for a driver that treats them alike: per-molecule columns -> totals (what ranks
# add up; count_keys) -> ratios and ``counts``
CountReport = collections.namedtuple("CountReport", "name graph_columns count_keys ratios totals summarise_totals")
COUNT_REPORTS = (CountReport("geometry", GRAPH_COLUMNS, COUNT_KEYS, RATIOS, job_totals, summarise_totals),
                 CountReport("bonds", BOND_GRAPH_COLUMNS, BOND_COUNT_KEYS, BOND_RATIOS, bond_totals, summarise_bond_totals),
                 CountReport("rings", RING_GRAPH_COLUMNS, RING_COUNT_KEYS, RING_RATIOS, ring_totals, summarise_ring_totals),
                 CountReport("aromatic", AROMATIC_GRAPH_COLUMNS, AROMATIC_COUNT_KEYS, AROMATIC_RATIOS, aromatic_totals,
                             summarise_aromatic_totals),
                 CountReport("valence", VALENCE_GRAPH_COLUMNS, VALENCE_COUNT_KEYS, VALENCE_RATIOS, valence_totals,
                             summarise_valence_totals))


# ---- SDF (V2000) records of samples: host only -----------------------------------------------------------------------------------------
_SDF_SYMBOLS = {1: "H", 6: "C", 7: "N", 8: "O", 9: "F", 15: "P", 16: "S", 17: "Cl"}
SDF_MAX_COUNT = 999                        # the counts line holds three digits


def sdf_record(name, pos, atomic_numbers, bond_index, bond_type):
    """one V2000 record as text: ``name``, two blank header lines, the counts line, atom lines ``%10.4f%10.4f%10.4f %-3s 0  0 ...``, bond
    lines ``%3d%3d%3d  0`` (1-based atoms; type 1 ... 3 the order, 4 aromatic), ``M  END`` and ``$$$$``.  ``pos`` [n, 3],
    ``atomic_numbers`` [n], ``bond_index`` [2, nb] local rows, ``bond_type`` [nb] (any array-like).  Raises ValueError for more than
    SDF_MAX_COUNT atoms or bonds, an element outside H C N O F P S Cl, or a bond type outside 1 ... 4.  No RDKit: nothing is sanitised,
    kekulised or given hydrogens"""
    pos = np.asarray(_np(pos), np.float64).reshape(-1, 3)
    zs = [int(v) for v in np.asarray(_np(atomic_numbers)).reshape(-1)]
    idx = np.asarray(_np(bond_index), np.int64).reshape(2, -1)
    types = [int(v) for v in np.asarray(_np(bond_type)).reshape(-1)]
    if len(zs) != pos.shape[0] or len(types) != idx.shape[1]:
        raise ValueError("sdf_record: one atomic number per position and one type per bond")
    if len(zs) > SDF_MAX_COUNT or len(types) > SDF_MAX_COUNT:
        raise ValueError(f"sdf_record: {len(zs)} atoms and {len(types)} bonds, a V2000 counts line holds {SDF_MAX_COUNT} of each")
    if any(z not in _SDF_SYMBOLS for z in zs):
        raise ValueError("sdf_record: an element outside H C N O F P S Cl")
    if any(t not in (1, 2, 3, 4) for t in types):
        raise ValueError("sdf_record: a bond type outside 1 ... 4")
    if idx.size and (idx.min() < 0 or idx.max() >= len(zs)):
        raise ValueError("sdf_record: a bond row outside the atoms")
    lines = [str(name), "  cbgbench_amd", "", "%3d%3d  0  0  0  0  0  0  0  0999 V2000" % (len(zs), len(types))]
    lines += ["%10.4f%10.4f%10.4f %-3s 0  0  0  0  0  0  0  0  0  0  0  0" % (x, y, z, _SDF_SYMBOLS[e]) for (x, y, z), e in zip(pos, zs)]
    lines += ["%3d%3d%3d  0" % (i + 1, j + 1, t) for i, j, t in zip(idx[0], idx[1], types)]
    return "\n".join(lines + ["M  END", "$$$$"]) + "\n"


# ---- distributions: pair distances, bond lengths, bond angles ------------------------------------------------------------------------
# include/cbgx.h CBGX_PAIR_HIST_MAX_EDGES / CBGX_ANGLES_MAX_EDGES / CBGX_ANGLES_MAX_PER_GRAPH / CBGX_ANGLE_BIN_DEGENERATE / CBGX_ANGLE_TYPES
MAX_PAIR_EDGES, MAX_ANGLE_EDGES, MAX_ANGLES_PER_GRAPH, ANGLE_BIN_DEGENERATE, N_ANGLE_TYPES = 255, 254, 16384, 255, 4608
N_BOND_TYPES = 192                         # ((order - 1) 8 + code_lo) 8 + code_hi
# with the aromatic type beside the three orders (include/cbgx.h CBGX_AROMATIC_BOND_TYPES / _ANGLE_TYPES): n_orders = 4
N_BOND_TYPES_4, N_ANGLE_TYPES_4 = 256, 8192


def n_type_codes(n_orders=3):
    """(bond type codes, angle type codes) of the three-order (default) or four-order (with the aromatic type) vocabulary"""
    if n_orders not in (3, 4):
        raise ValueError(f"n_orders is 3 (bond orders) or 4 (orders and the aromatic type), not {n_orders!r}")
    return (N_BOND_TYPES, N_ANGLE_TYPES) if n_orders == 3 else (N_BOND_TYPES_4, N_ANGLE_TYPES_4)
DISTRIBUTIONS_TOO_MANY_ANGLES = 1          # status bit (include/cbgx.h CBGX_DISTRIBUTIONS_TOO_MANY_ANGLES)
DISTRIBUTION_GRAPH_COLUMNS = ("n_atoms", "n_bonds", "n_angles", "n_degenerate_angles", "status")
PAIR_FAMILIES = ("All_12A", "CC_2A")       # family 0, family 1 of cbgx_ligand_pair_hist, named like the reference's profiles
BOND_SYMBOLS = "-=#"                       # orders 1, 2, 3 (eval_bond_length.get_bond_str; '?' is what it prints for anything else)
BOND_SYMBOLS_4 = BOND_SYMBOLS + ":"        # and type 4, the aromatic bond
DISTRIBUTION_BINS = (101, 120, 91)         # bins of the pair, bond-length and angle histograms under the default edges


def default_pair_edges():
    """the reference's EMPIRICAL_BINS (eval_bond_length_config.py:10-13) in family order: np.linspace(0, 12, 100), np.linspace(0, 2, 100)"""
    return np.linspace(0, 12, 100), np.linspace(0, 2, 100)


def default_bond_edges():
    """the reference's DISTANCE_BINS (eval_bond_length_config.py:8): 119 edges, 120 bins"""
    return np.arange(1.1, 1.7, 0.005)[:-1]


def default_cos_edges():
    """cosines of the reference's angle edges np.arange(0, 180, 2) (eval_bond_angle.py:35), rounded to 15 decimals: that makes the
    cosines of 0, 60, 90 and 120 degrees exact (cos(90 deg) would otherwise be 6e-17 and move every exact right angle one bin up) and
    moves no other edge by more than 1e-12 degrees"""
    return np.round(np.cos(np.deg2rad(np.arange(0, 180, 2))), 15)


def _edges(edges, what, limit, decreasing=False):
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
    if e.shape[0] > limit:
        raise ValueError(f"{what}: {e.shape[0]} edges, at most {limit}")
    step = np.diff(e)
    if not np.isfinite(e).all() or not ((step < 0).all() if decreasing else (step > 0).all()):
        raise ValueError(f"{what} must be finite and strictly {'decreasing' if decreasing else 'increasing'}")
    return e


def ligand_pair_hist(x_lig, z_lig, lig_batch, n_graphs, edges_all=None, edges_cc=None):
    """Pair-distance histograms of ``n_graphs`` ligands, one launch (``cbgx_ligand_pair_hist``, csrc/distributions.hip; the definition is
    in include/cbgx.h) on the tensors' current stream: the counterpart of ``pair_distance_from_pos_v`` + ``get_pair_length_profile``
    (eval_bond_length.py:77-84, 119-129), reproduced exactly.

    Arguments as ``ligand_bonds``; ``edges_all`` / ``edges_cc``: strictly increasing float64 edges of family 0 (every pair i < j of a
    ligand, atoms of unknown element included) and family 1 (both atoms carbon), at most MAX_PAIR_EDGES each; default
    ``default_pair_edges()``.  Returns ``pair_hist`` [n_graphs, 2, E_max + 1] int32 on the device: a pair takes part iff d <
    edges[-1], its bin is ``np.searchsorted(edges, d)``.  There is no CPU path."""
    dev = x_lig.device
    _gpu_only(dev, "ligand_pair_hist", "cbgx_ligand_pair_hist")
    n_graphs = int(n_graphs)
    n_lig, lig_ptr, x_lig, z_lig = _ligand_arrays(x_lig, z_lig, lig_batch, n_graphs)
    ea, ec = default_pair_edges()
    ea = _edges(ea if edges_all is None else edges_all, "edges_all", MAX_PAIR_EDGES)
    ec = _edges(ec if edges_cc is None else edges_cc, "edges_cc", MAX_PAIR_EDGES)
    dea, dec = torch.from_numpy(ea).to(dev), torch.from_numpy(ec).to(dev)
    pair_hist = torch.empty(n_graphs, 2, max(len(ea), len(ec)) + 1, dtype=torch.int32, device=dev)
    p = _native.ptr
    _native.check(_native.lib().cbgx_ligand_pair_hist(p(x_lig), p(z_lig), p(lig_ptr), n_lig, n_graphs, p(dea) if len(ea) else None, len(ea),
                                                      p(dec) if len(ec) else None, len(ec), p(pair_hist), _native.current_stream(dev)),
                  "cbgx_ligand_pair_hist")
    return pair_hist


_ELEMENT_CODE = None


def _element_code(dev):
    """[256] int64 on ``dev``: the element code 0 ... 7 of an atomic number (``tables()['elements']``), -1 when it has none"""
    global _ELEMENT_CODE
    if _ELEMENT_CODE is None:
        code = np.full(256, -1, np.int64)
        for c, z in enumerate(tables()["elements"].tolist()):
            code[z] = c
        _ELEMENT_CODE = torch.from_numpy(code)
    return _ELEMENT_CODE.to(dev)


def ligand_angles(x_lig, z_lig, lig_batch, n_graphs, bonds, cos_edges=None):
    """The bond angles of the table-bond graphs of ``n_graphs`` ligands (``cbgx_ligand_angles``, csrc/distributions.hip; the definition
    is in include/cbgx.h), on the tensors' current stream: the counterpart of ``bond_angle_from_mol`` (eval_bond_angle.py:69-96) on
    TABLE bonds -- same stated deviation as ``ligand_bonds`` / ``ligand_rings``: no aromatic type, no valence repair.

    ``bonds``: what ``ligand_bonds`` returned for the same arrays.  The symmetric adjacency (the list and its flip, sorted by (centre,
    neighbour)) and the prefix sum of C(deg, 2) are made with torch on the device; its last element is read on the host to size the
    list.  ``cos_edges``: strictly decreasing float64 cosines of the angle edges, at most MAX_ANGLE_EDGES; default
    ``default_cos_edges()``.  Returns device tensors: ``angle_index`` [3, n_angles] int32 (rows a, c, b: global ligand rows, a < b bonded
    partners of the centre c, in (c, a, b) order), ``angle_cos`` [n_angles] float64 (nan: degenerate), ``angle_bin`` [n_angles] uint8 (the
    number of edges strictly greater than the cosine; ANGLE_BIN_DEGENERATE for a degenerate angle, which belongs to no histogram),
    ``angle_type`` [n_angles] int16 (canonical, see ``angle_type_code``), ``angle_graph`` [n_angles] int64 and ``graph_counts``
    [n_graphs, 5] int32 (DISTRIBUTION_GRAPH_COLUMNS).  A graph of more than MAX_ANGLES_PER_GRAPH angles is not an error: its status is
    DISTRIBUTIONS_TOO_MANY_ANGLES, it has no angles in the list and n_angles = n_degenerate_angles = 0.  There is no CPU path."""
    dev = x_lig.device
    _gpu_only(dev, "ligand_angles", "cbgx_ligand_angles")
    n_graphs = int(n_graphs)
    n_lig, lig_ptr, x_lig, z_lig = _ligand_arrays(x_lig, z_lig, lig_batch, n_graphs)
    ce = _edges(default_cos_edges() if cos_edges is None else cos_edges, "cos_edges", MAX_ANGLE_EDGES, decreasing=True)
    bi = bonds["bond_index"].to(torch.long)
    n_bonds = int(bi.shape[1])
    graph = lig_batch.to(torch.long)
    centre, nbr = torch.cat([bi[0], bi[1]]), torch.cat([bi[1], bi[0]])
    perm = torch.argsort(centre * max(n_lig, 1) + nbr)                  # (a pair is listed once: the keys are distinct)
    adj_nbr = nbr[perm].to(torch.int32).contiguous()
    adj_order = torch.cat([bonds["bond_order"], bonds["bond_order"]])[perm].to(torch.uint8).contiguous()
    deg = torch.bincount(centre, minlength=n_lig) if n_lig else centre.new_zeros(0)
    adj_ptr = torch.cat([deg.new_zeros(1), deg.cumsum(0)]).to(torch.int32).contiguous()
    per_centre = deg * (deg - 1) // 2
    per_graph = torch.zeros(n_graphs, dtype=torch.long, device=dev).index_add_(0, graph, per_centre)
    over = per_graph > MAX_ANGLES_PER_GRAPH
    per_centre = torch.where(over[graph], torch.zeros_like(per_centre), per_centre)
    ends = per_centre.cumsum(0)
    n_angles = int(ends[-1]) if n_lig else 0
    if n_angles > 2 ** 31 - 1:
        raise ValueError(f"{n_angles} angles in one batch: more than an int32 angle_ptr addresses")
    angle_ptr = torch.cat([ends.new_zeros(1), ends]).to(torch.int32).contiguous()
    dce = torch.from_numpy(ce).to(dev)
    angle_index = torch.empty(3, n_angles, dtype=torch.int32, device=dev)
    angle_cos = torch.empty(n_angles, dtype=torch.float64, device=dev)
    angle_bin = torch.empty(n_angles, dtype=torch.uint8, device=dev)
    angle_type = torch.empty(n_angles, dtype=torch.int16, device=dev)
    p = _native.ptr
    _native.check(_native.lib().cbgx_ligand_angles(
        p(x_lig), p(z_lig), p(lig_ptr), n_lig, n_graphs, p(adj_ptr), p(adj_nbr) if n_bonds else None, p(adj_order) if n_bonds else None,
        2 * n_bonds, p(angle_ptr), n_angles, p(dce) if len(ce) else None, len(ce), p(angle_index) if n_angles else None,
        p(angle_cos) if n_angles else None, p(angle_bin) if n_angles else None, p(angle_type) if n_angles else None,
        _native.current_stream(dev)), "cbgx_ligand_angles")
    angle_graph = graph[angle_index[1].to(torch.long)]
    n_degenerate = torch.bincount(angle_graph[angle_bin == ANGLE_BIN_DEGENERATE], minlength=n_graphs)
    graph_counts = torch.stack([torch.bincount(graph, minlength=n_graphs), torch.bincount(graph[bi[0]], minlength=n_graphs),
                                torch.where(over, torch.zeros_like(per_graph), per_graph), n_degenerate,
                                over.to(torch.long) * DISTRIBUTIONS_TOO_MANY_ANGLES], 1).to(torch.int32)
    return {"angle_index": angle_index, "angle_cos": angle_cos, "angle_bin": angle_bin, "angle_type": angle_type,
            "angle_graph": angle_graph, "graph_counts": graph_counts}


def _sparse_hist(graph, code, bins, n_codes, n_bins):
    """per-graph histogram over (code, bin) as a sorted sparse list: (index [3, m] int32 rows graph, code, bin; count [m] int32), by
    ``torch.unique`` on graph n_codes n_bins + code n_bins + bin -- the non-zero cells of the dense [B, n_codes, n_bins] table"""
    key = (graph.to(torch.long) * n_codes + code.to(torch.long)) * n_bins + bins.to(torch.long)
    key, count = torch.unique(key, return_counts=True)
    index = torch.stack([key // (n_codes * n_bins), key // n_bins % n_codes, key % n_bins]).to(torch.int32)
    return index, count.to(torch.int32)


def _aromatic_types(out, bonds, aromatic, z, n_lig):
    """``bond_type`` / ``angle_type`` of ``batch_distributions`` in the four-order codes: the bond's type is ``aromatic['bond_type']`` (its
    order where the aromatic report did not evaluate the graph), an angle's two bonds are looked up in the bond list by ``searchsorted`` on
    lo n_lig + hi -- the list is in (i, j) order, so the keys are sorted -- and the canonical orientation is chosen as the kernel does"""
    dev = z.device
    bi = bonds["bond_index"].to(torch.long)
    t = torch.where(aromatic["bond_type"] == BOND_TYPE_NOT_EVALUATED, bonds["bond_order"].to(torch.uint8), aromatic["bond_type"]).to(torch.long)
    code = _element_code(dev)[z]
    ci, cj = code[bi[0]], code[bi[1]]
    bond_type = (((t - 1) * 8 + torch.minimum(ci, cj)) * 8 + torch.maximum(ci, cj)).to(torch.int16)
    ai = out["angle_index"].to(torch.long)
    keys = bi[0] * max(n_lig, 1) + bi[1]

    def type_of(u, v):
        at = torch.searchsorted(keys, torch.minimum(u, v) * max(n_lig, 1) + torch.maximum(u, v))
        return t[at.clamp(max=max(keys.numel() - 1, 0))] - 1          # (an angle's bonds are in the list: the clamp never acts)

    ta, tb = type_of(ai[0], ai[1]), type_of(ai[2], ai[1])
    ca, cc, cb = code[ai[0]], code[ai[1]], code[ai[2]]
    swap = (ca > cb) | ((ca == cb) & (ta > tb))
    c1, t1, c2, t2 = torch.where(swap, cb, ca), torch.where(swap, tb, ta), torch.where(swap, ca, cb), torch.where(swap, ta, tb)
    return bond_type, ((((c1 * 4 + t1) * 8 + cc) * 4 + t2) * 8 + c2).to(torch.int16)


def batch_distributions(batch, x, c, lig_batch, mode, bonds=None, aromatic=None):
    """The three distributions of a sampling state under the reference's bins (``default_pair_edges``, ``default_bond_edges``,
    ``default_cos_edges``); ``bonds``: what ``batch_bonds`` returned for the same state (it is called here when None).  Returns device
    tensors: the per-angle lists and ``graph_counts`` of ``ligand_angles``; ``bond_bin`` [n_bonds] uint8 (the number of edges strictly
    less than ``bond_length``: ``torch.bucketize``) and ``bond_type`` [n_bonds] int16 (``bond_type_code``) of the bond list;
    ``pair_hist`` [B, 2, 101] int32 of ``ligand_pair_hist``; and the per-graph histograms by type as sorted sparse lists,
    ``bond_hist_index`` [3, m] int32 (rows graph, type, bin) with ``bond_hist_count`` [m] int32, and ``angle_hist_index`` /
    ``angle_hist_count`` likewise (degenerate angles left out).

    ``aromatic``: what ``batch_aromatic`` returned for the same state and bonds; ``bond_type``, ``angle_type`` and both sparse
    histograms then use the four-order type codes (``bond_type_code`` / ``angle_type_code`` with ``n_orders=4``: an aromatic bond is type
    4 and no longer counted under its order).  With None (default) every output is what it is without the argument."""
    if bonds is None:
        bonds = batch_bonds(batch, x, c, lig_batch, mode)
    dev = bonds["bond_index"].device
    x, lig_batch = x.to(dev), lig_batch.to(dev)
    _, z, n_graphs = _state_atoms(c, mode, lig_batch, {"num_graphs": bonds["graph_counts"].shape[0]}, dev)
    out = ligand_angles(x, z, lig_batch, n_graphs, bonds)
    out["pair_hist"] = ligand_pair_hist(x, z, lig_batch, n_graphs)
    edges = torch.from_numpy(_edges(default_bond_edges(), "bond edges", 255)).to(dev)
    out["bond_bin"] = torch.bucketize(bonds["bond_length"], edges, right=False).to(torch.uint8)
    code = _element_code(dev)[z]
    ci, cj = code[bonds["bond_index"][0].to(torch.long)], code[bonds["bond_index"][1].to(torch.long)]
    out["bond_type"] = (((bonds["bond_order"].to(torch.long) - 1) * 8 + torch.minimum(ci, cj)) * 8 + torch.maximum(ci, cj)).to(torch.int16)
    n_bond_types, n_angle_types = n_type_codes(3 if aromatic is None else 4)
    if aromatic is not None:
        out["bond_type"], out["angle_type"] = _aromatic_types(out, bonds, aromatic, z, int(z.shape[0]))
    n_pair, n_bond_bins, n_angle_bins = DISTRIBUTION_BINS
    out["bond_hist_index"], out["bond_hist_count"] = _sparse_hist(bonds["bond_graph"], out["bond_type"], out["bond_bin"], n_bond_types,
                                                                  n_bond_bins)
    ok = out["angle_bin"] != ANGLE_BIN_DEGENERATE
    out["angle_hist_index"], out["angle_hist_count"] = _sparse_hist(out["angle_graph"][ok], out["angle_type"][ok], out["angle_bin"][ok],
                                                                    n_angle_types, n_angle_bins)
    return out


# ---- type codes and their strings ----------------------------------------------------------------------------------------------------
_ELEMENTS = (1, 6, 7, 8, 9, 15, 16, 17)      # atomic numbers of the element codes 0 ... 7 (``tables()['elements']``; asserted in the tests)


def bond_type_code(code_a, order, code_b, n_orders=3):
    """((order - 1) 8 + code_lo) 8 + code_hi, code_lo <= code_hi: element codes 0 ... 7, order 1 ... 3 -- with ``n_orders=4`` 1 ... 4, 4
    the aromatic type (the packing is the same: the three-order codes are the first 192 of the 256)"""
    lo, hi = min(code_a, code_b), max(code_a, code_b)
    return ((order - 1) * 8 + lo) * 8 + hi


def angle_type_code(code_a, order_ac, code_c, order_bc, code_b, n_orders=3):
    """the canonical code of an angle a - c - b: of the two orientations the one whose end (code, order) is lexicographically smaller
    comes first, packed as (((code_1 K + (o_1 - 1)) 8 + code_c) K + (o_2 - 1)) 8 + code_2 with K = ``n_orders``: in [0, N_ANGLE_TYPES)
    for K = 3, in [0, N_ANGLE_TYPES_4) for K = 4 (orders 1 ... 3 and the aromatic type 4)"""
    (c1, o1), (c2, o2) = sorted([(code_a, order_ac), (code_b, order_bc)])
    return (((c1 * n_orders + (o1 - 1)) * 8 + code_c) * n_orders + (o2 - 1)) * 8 + c2


def bond_type_string(code):
    """'6-6', '6=8', '6#7', '6:6': atomic numbers in ascending order around the bond symbol, as eval_bond_length._bond_type_str prints
    them; ':' is the aromatic type of the four-order codes"""
    code = int(code)
    return f"{_ELEMENTS[code // 8 % 8]}{BOND_SYMBOLS_4[code // 64]}{_ELEMENTS[code % 8]}"


def angle_type_string(code, n_orders=3):
    """'6-6=8', with ``n_orders=4`` also '6:6:6': as eval_bond_angle._angle_type_str prints the canonical orientation"""
    code, k = int(code), int(n_orders)
    c2, o2, cc, o1, c1 = code % 8, code // 8 % k, code // (8 * k) % 8, code // (64 * k) % k, code // (64 * k * k)
    return f"{_ELEMENTS[c1]}{BOND_SYMBOLS_4[o1]}{_ELEMENTS[cc]}{BOND_SYMBOLS_4[o2]}{_ELEMENTS[c2]}"


def _parse_type(key, n_orders=3):
    """a reference key -- 'CC_2A' / 'All_12A', a bond '6-6' or (6, 6, 1), an angle '8=6-6' or (8, 2, 6, 1, 6), in either orientation ->
    (kind, canonical string) or (None, reason).  Orders are 1, 2, 3 or the symbols - = #; 4, ':' and '?' (what the reference prints for
    it) name an aromatic bond, which is a type with ``n_orders=4`` and a reason not to evaluate the key with the default"""
    if isinstance(key, str) and key in PAIR_FAMILIES:
        return "pair_length", key
    if isinstance(key, str):
        import re
        m = re.fullmatch(r"(\d+)([-=#:?])(\d+)(?:([-=#:?])(\d+))?", key.strip())
        if not m:
            return None, "not a pair family, a bond type or an angle type"
        f = [t for t in m.groups() if t is not None]
        atoms, orders = [int(t) for t in f[0::2]], [BOND_SYMBOLS.index(t) + 1 if t in BOND_SYMBOLS else 4 for t in f[1::2]]
    else:
        f = [int(t) for t in key]
        if len(f) == 3:
            atoms, orders = f[:2], f[2:]
        elif len(f) == 5:
            atoms, orders = f[0::2], f[1::2]
        else:
            return None, "not a pair family, a bond type or an angle type"
    n_type_codes(n_orders)
    if n_orders == 3 and any(o == 4 for o in orders):
        return None, "aromatic bond type: table bonds have orders 1, 2, 3 only"
    if any(o not in (1, 2, 3, 4) for o in orders):
        return None, "unknown bond order"
    if any(z not in _ELEMENTS for z in atoms):
        return None, "an element outside H C N O F P S Cl"
    codes = [_ELEMENTS.index(z) for z in atoms]
    if len(codes) == 2:
        return "bond_length", bond_type_string(bond_type_code(codes[0], orders[0], codes[1], n_orders))
    return "bond_angle", angle_type_string(angle_type_code(codes[0], orders[0], codes[1], orders[1], codes[2], n_orders), n_orders)


def _key_string(key):
    """a reference key as the reference prints it: a string as it is; (6, 6, 4) -> '6?6', (8, 2, 6, 1, 6) -> '8=6-6'"""
    if isinstance(key, str):
        return key
    f = [int(t) for t in key]
    f = [f[0], f[2], f[1]] if len(f) == 3 else f            # a bond tuple carries its order last
    return "".join((BOND_SYMBOLS[t - 1] if 1 <= t <= 3 else "?") if k % 2 else str(t) for k, t in enumerate(f))


# ---- job totals, summaries, Jensen-Shannon distances ---------------------------------------------------------------------------------
DISTRIBUTION_COUNT_KEYS = ("n_mol", "n_mol_over_limit", "n_atoms", "n_bonds", "n_angles", "n_degenerate_angles")


def distribution_totals_length(bins=DISTRIBUTION_BINS, n_orders=3):
    """the length of the flat totals of ``distribution_totals``; ``n_orders=4``: with the aromatic type (``batch_distributions(...,
    aromatic=...)``)"""
    n_bond_types, n_angle_types = n_type_codes(n_orders)
    return len(DISTRIBUTION_COUNT_KEYS) + 2 * bins[0] + n_bond_types * bins[1] + n_angle_types * bins[2]


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def distribution_totals(dist, graphs=None, bins=DISTRIBUTION_BINS, n_orders=3):
    """what ``batch_distributions`` returned (tensors or arrays) -> the integer totals of its graphs, or of the graphs ``graphs`` = (g0, g1)
    only, as one flat int64 array that ranks can add: DISTRIBUTION_COUNT_KEYS, then the dense histograms flattened -- pairs [2, bins[0]],
    bond lengths [N_BOND_TYPES, bins[1]], angles [N_ANGLE_TYPES, bins[2]].  A molecule over the angle limit counts in n_mol and
    n_mol_over_limit, with its atoms, bonds, pair and bond-length histograms; it has no angles.  ``n_orders=4`` for what
    ``batch_distributions(..., aromatic=...)`` returned: N_BOND_TYPES_4 and N_ANGLE_TYPES_4 rows"""
    n_bond_types, n_angle_types = n_type_codes(n_orders)
    gc = _np(dist["graph_counts"]).astype(np.int64).reshape(-1, len(DISTRIBUTION_GRAPH_COLUMNS))
    g0, g1 = (0, gc.shape[0]) if graphs is None else (int(graphs[0]), int(graphs[1]))
    n_pair, n_bond_bins, n_angle_bins = bins
    pair = _np(dist["pair_hist"]).astype(np.int64)
    if pair.shape[1:] != (2, n_pair):
        raise ValueError(f"pair_hist is {pair.shape}, expected [B, 2, {n_pair}]")
    part = gc[g0:g1]
    head = [part.shape[0], int((part[:, 4] != 0).sum())] + [int(v) for v in part[:, :4].sum(0)]

    def dense(index, count, n_codes, n_bins):
        index, count = _np(index).astype(np.int64).reshape(3, -1), _np(count).astype(np.int64).reshape(-1)
        m = (index[0] >= g0) & (index[0] < g1)
        if index.shape[1] and int(index[1].max()) >= n_codes:
            raise ValueError(f"type code {int(index[1].max())} in a histogram of {n_codes} types: n_orders={n_orders} is not what made it")
        out = np.zeros(n_codes * n_bins, np.int64)
        np.add.at(out, index[1][m] * n_bins + index[2][m], count[m])
        return out

    return np.concatenate([np.asarray(head, np.int64), pair[g0:g1].sum(0).reshape(-1),
                           dense(dist["bond_hist_index"], dist["bond_hist_count"], n_bond_types, n_bond_bins),
                           dense(dist["angle_hist_index"], dist["angle_hist_count"], n_angle_types, n_angle_bins)])


def distribution_counts(totals, bins=DISTRIBUTION_BINS, n_orders=3):
    """the flat totals of ``distribution_totals`` as integers by name: ``counts`` (DISTRIBUTION_COUNT_KEYS), ``pair_hist`` [2][bins[0]],
    ``bond_hist`` / ``angle_hist`` {type string: [counts per bin]} for the types with a non-zero count"""
    t = np.asarray(totals, dtype=np.int64).reshape(-1)
    n_pair, n_bond_bins, n_angle_bins = bins
    n_head = len(DISTRIBUTION_COUNT_KEYS)
    n_bond_types, n_angle_types = n_type_codes(n_orders)
    sizes = [n_head, 2 * n_pair, n_bond_types * n_bond_bins, n_angle_types * n_angle_bins]
    if t.shape[0] != sum(sizes):
        raise ValueError(f"{t.shape[0]} totals, expected {sum(sizes)} for bins {tuple(bins)}")
    head, pair, bond, angle = np.split(t, np.cumsum(sizes)[:-1])
    bond, angle = bond.reshape(n_bond_types, n_bond_bins), angle.reshape(n_angle_types, n_angle_bins)
    return {"counts": {k: int(v) for k, v in zip(DISTRIBUTION_COUNT_KEYS, head)}, "pair_hist": pair.reshape(2, n_pair).tolist(),
            "bond_hist": {bond_type_string(k): bond[k].tolist() for k in np.flatnonzero(bond.sum(1))},
            "angle_hist": {angle_type_string(k, n_orders): angle[k].tolist() for k in np.flatnonzero(angle.sum(1))}}


def summarise_distribution_totals(totals, bins=DISTRIBUTION_BINS, n_orders=3):
    """the normalised distributions of integer totals (``distribution_totals``, summed over ranks): ``pair_length`` {'All_12A', 'CC_2A'},
    ``bond_length`` {'6-6', '6=8', ...} and ``bond_angle`` {'6-6=8', ...} -- keyed like the reference's profiles, atomic numbers around
    - = # -- each {'count': n, 'distribution': counts / n}; bond and angle types are listed when their count is non-zero, a pair family
    always, and a ratio over nothing is nan.  Plus ``counts`` (DISTRIBUTION_COUNT_KEYS).  What the reference compares with a dataset's
    profile by Jensen-Shannon distance (``jsd_against``).  ``n_orders=4``: totals with the aromatic type, keys such as '6:6' and '6:6:6'"""
    c = distribution_counts(totals, bins, n_orders)

    def profile(h):
        h = np.asarray(h, np.float64)
        n = h.sum()
        return {"count": int(n), "distribution": (h / n if n else np.full(h.shape, np.nan)).tolist()}

    return {"counts": c["counts"], "pair_length": {k: profile(h) for k, h in zip(PAIR_FAMILIES, c["pair_hist"])},
            "bond_length": {k: profile(h) for k, h in c["bond_hist"].items()},
            "bond_angle": {k: profile(h) for k, h in c["angle_hist"].items()}}


def summarise_distributions(dist, n_orders=3):
    """``summarise_distribution_totals`` of what ``batch_distributions`` returned (``n_orders=4`` when it was given ``aromatic=``)"""
    return summarise_distribution_totals(distribution_totals(dist, n_orders=n_orders), n_orders=n_orders)


def distribution_jsd(p, q):
    """Jensen-Shannon distance (the square root of the divergence, natural logarithm: ``scipy.spatial.distance.jensenshannon``) of two
    non-negative vectors of equal length; both are normalised to sum 1 first.  nan when either sums to nothing.  ``ring_jsd`` is this over
    the six ring sizes"""
    p, q = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (p, q))
    if p.shape != q.shape or p.shape[0] == 0:
        raise ValueError(f"distribution_jsd takes two vectors of one length, got {p.shape[0]} and {q.shape[0]}")
    if not (p.sum() > 0 and q.sum() > 0):
        return float("nan")
    p, q = p / p.sum(), q / q.sum()
    mid = (p + q) / 2.0
    kl = lambda a, b: np.sum(np.where(a > 0, a * np.log(np.where(a > 0, a, 1.0) / np.where(a > 0, b, 1.0)), 0.0))
    return float(np.sqrt(max((kl(p, mid) + kl(q, mid)) / 2.0, 0.0)))


def jsd_against(summary, reference, n_orders=3):
    """Jensen-Shannon distances of a job's distributions (``summarise_distribution_totals``) against the caller's own reference vectors --
    none ship with this package.  ``reference``: {key: vector}; a key is 'All_12A' / 'CC_2A', a bond type ('6-6' or (6, 6, 1)) or an angle
    type ('8=6-6' or (8, 2, 6, 1, 6)) in either orientation (canonicalised here).  Returns {'JSD_<key>': distance or None, ...} under
    the key's own spelling and ``not_evaluated`` {'JSD_<key>': reason}: a key that names an aromatic bond (type 4) cannot be met by table
    bonds -- unless the summary is one with the aromatic type and ``n_orders=4`` says so: (6, 6, 4), '6:6' and '6:6:6' are then types
    like any other --; a type without a sample has no distribution (the reference reports None there too).  A vector of another length
    than the job's raises ValueError"""
    out, why = {}, {}
    for key, vec in reference.items():
        name = "JSD_" + _key_string(key)
        kind, canon = _parse_type(key, n_orders)
        if kind is None:
            out[name], why[name] = None, canon
            continue
        mine = summary[kind].get(canon)
        if mine is None or not mine["count"]:
            out[name], why[name] = None, "no such type among the samples"
            continue
        vec = np.asarray(vec, np.float64).reshape(-1)
        if vec.shape[0] != len(mine["distribution"]):
            raise ValueError(f"reference {key!r} has {vec.shape[0]} bins, the job's distribution {len(mine['distribution'])}")
        out[name] = distribution_jsd(mine["distribution"], vec)
    out["not_evaluated"] = why
    return out

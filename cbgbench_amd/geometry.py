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
library."""
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

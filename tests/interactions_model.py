"""Plain numpy / Python float64 restatement of the interaction report's definition (include/cbgx.h, cbgx_pocket_types /
cbgx_ligand_interactions; csrc/interactions.hip), written from that text: the residue table, the ligand typing, rotatable bonds as bridges
found by depth-first search, the five pair terms, the per-graph columns, the limits and the status bits.  Distances are the written-out
roundings of tests/geometry_model.py; the table-bond thresholds come from the library (cbgx_ligand_geometry_tables).  Every float sum is
``math.fsum`` of its addends -- the correctly rounded sum, whatever order the kernel adds in -- and comes with the sum of the absolute values
of the same addends, which is what the GPU tests scale their bound by."""
import math

import numpy as np

from tests import geometry_model as GM

MAX_ATOMS, TERMS, COLS = 256, 5, 13
COLUMNS = ("n_atoms", "n_bonds", "n_rotatable", "n_donors", "n_acceptors", "n_hydrophobic_atoms", "n_pairs", "n_hbond_pairs",
           "n_hydrophobic_pairs", "n_close_pairs", "n_contact_atoms", "n_protein_untyped", "status")
MASK, HYD, DON, ACC, UNTYPED = 7, 8, 16, 32, 64
TOO_MANY_ATOMS, BAD_BONDS, NO_VALENCE = 1, 4, 8
VALENCE_EXCEEDED = 1
CODE = {6: 1, 7: 2, 8: 3, 9: 4, 15: 5, 16: 6, 17: 7}                     # atomic number -> element code of a type byte
RADIUS = {1: 1.9, 2: 1.8, 3: 1.7, 4: 1.5, 5: 2.1, 6: 2.0, 7: 1.8}        # by element code, in Angstrom
CUTOFF = 8.0
AA = ("ALA", "CYS", "ASP", "GLU", "PHE", "GLY", "HIS", "ILE", "LYS", "LEU", "MET", "ASN", "PRO", "GLN", "ARG", "SER", "THR", "VAL", "TRP",
      "TYR")
WEIGHTS, ROT_WEIGHT = (-0.035579, -0.005156, 0.840245, -0.035069, -0.587439), 0.05846


def residue(aa):
    aa = int(aa)
    return AA[aa] if 0 <= aa < len(AA) else "other"


def pocket_atom_type(z, aa, backbone, carbon_has_hetero_bond=False):
    """the type byte of one pocket atom; for a carbon, whether it has a table bond to N, O or S is the caller's"""
    z, res, backbone = int(z), residue(aa), bool(backbone)
    if z == 1:
        return 0
    if z == 6:
        return CODE[6] | (0 if carbon_has_hetero_bond else HYD)
    if z == 7:
        if backbone:
            return CODE[7] | (0 if res == "PRO" else DON)
        if res in ("LYS", "ARG", "ASN", "GLN", "TRP"):
            return CODE[7] | DON
        return CODE[7] | (DON | ACC if res == "HIS" else 0)
    if z == 8:
        return CODE[8] | ACC | (DON if not backbone and res in ("SER", "THR", "TYR") else 0)
    if z == 16:
        return CODE[16]
    return UNTYPED


def _clamp(lo, hi, size):
    lo = min(max(int(lo), 0), size)
    return lo, min(max(int(hi), lo), size)


def pocket_types(x_rec, z_rec, rec_ptr, rec_aa, rec_backbone):
    """[n_rec] uint8, every element the kernel writes; 255 where it writes nothing (atoms of no graph)"""
    x_rec = np.asarray(x_rec, np.float32).reshape(-1, 3)
    z_rec, rec_aa, rec_backbone = (np.asarray(v).reshape(-1) for v in (z_rec, rec_aa, rec_backbone))
    n_rec = len(z_rec)
    T = GM.tables()
    el = [int(v) for v in T["elements"]]
    single = {z: float(T["bond_pm"][0][el.index(6)][el.index(z)] + T["margins"][0]) for z in (7, 8, 16)}
    out = np.full(n_rec, 255, np.uint8)
    for g in range(len(rec_ptr) - 1):
        r0, r1 = _clamp(rec_ptr[g], rec_ptr[g + 1], n_rec)
        z = z_rec[r0:r1].astype(np.int64)
        carbons, hetero = np.flatnonzero(z == 6), np.flatnonzero((z == 7) | (z == 8) | (z == 16))
        bonded = np.zeros(r1 - r0, bool)
        if len(carbons) and len(hetero):
            p = 100.0 * GM.distances(x_rec[r0:r1][carbons], x_rec[r0:r1][hetero])
            limit = np.array([single[int(v)] for v in z[hetero]])
            bonded[carbons] = (p < limit[None, :]).any(1)
        for a in range(r0, r1):
            out[a] = pocket_atom_type(z_rec[a], rec_aa[a], rec_backbone[a], bonded[a - r0])
    return out


def takes_part(t):
    t = np.asarray(t).astype(np.int64)
    return (t > 0) & (t < UNTYPED) & ((t & MASK) != 0)


def bridges(n, pairs):
    """the set of positions of ``pairs`` (a strict list: no bond twice) that lie on no cycle: depth-first search with low links, no
    recursion"""
    adj = [[] for _ in range(n)]
    for e, (i, j) in enumerate(pairs):
        adj[i].append((j, e))
        adj[j].append((i, e))
    disc, low, out, clock = [-1] * n, [0] * n, set(), 0
    for root in range(n):
        if disc[root] >= 0:
            continue
        disc[root] = low[root] = clock
        clock += 1
        stack = [(root, -1, 0)]
        while stack:
            a, via, pos = stack.pop()
            if pos < len(adj[a]):
                stack.append((a, via, pos + 1))
                b, e = adj[a][pos]
                if e == via:
                    continue
                if disc[b] < 0:
                    disc[b] = low[b] = clock
                    clock += 1
                    stack.append((b, e, 0))
                else:
                    low[a] = min(low[a], disc[b])
            elif via >= 0:
                i, j = pairs[via]
                parent = i if j == a else j
                low[parent] = min(low[parent], low[a])
                if low[a] > disc[parent]:
                    out.add(via)
    return out


def ligand_graph(n, pairs, z, kekule, aromatic, implicit_h, atom_flags):
    """one graph that passed the checks -> (lig_type [n], bond_rotatable [m])"""
    heavy, hyd, hetero, triple = [0] * n, [0] * n, [False] * n, [False] * n
    for (i, j), o in zip(pairs, kekule):
        for a, b in ((i, j), (j, i)):
            if z[b] == 1:
                hyd[a] += 1
            else:
                heavy[a] += 1
            hetero[a] = hetero[a] or z[b] not in (1, 6)
            triple[a] = triple[a] or int(o) == 3
    types = []
    for a in range(n):
        h = int(implicit_h[a]) + hyd[a]
        code = CODE.get(int(z[a]), 0)
        if z[a] == 6:
            t = code | (0 if hetero[a] else HYD)
        elif z[a] in (9, 17):
            t = code | HYD
        elif z[a] == 8:
            t = code | ACC | (DON if h > 0 else 0)
        elif z[a] == 7:
            t = code | (DON if h > 0 else 0) | (ACC if h == 0 and heavy[a] <= 2 and not int(atom_flags[a]) & VALENCE_EXCEEDED else 0)
        else:
            t = code            # P, S; 0 for H and for anything else
        types.append(t)
    on_no_cycle = bridges(n, pairs)
    rot = [int(e in on_no_cycle and int(kekule[e]) == 1 and int(aromatic[e]) != 1 and heavy[i] >= 2 and heavy[j] >= 2 and not triple[i]
               and not triple[j]) for e, (i, j) in enumerate(pairs)]
    return types, rot


def pair_terms(x_lig, lig_type, x_rec, rec_type):
    """the five terms of every (ligand atom, pocket atom) pair of one graph -> (terms [5, n, nr] float64 with 0.0 where a pair adds
    nothing, within [n, nr] bool: both take part and r < 8, d [n, nr], donor_acceptor [n, nr] bool)"""
    ti, tj = np.asarray(lig_type).astype(np.int64), np.asarray(rec_type).astype(np.int64)
    r = GM.distances(x_lig, x_rec)
    within = takes_part(ti)[:, None] & takes_part(tj)[None, :] & (r < CUTOFF)
    ri = np.array([RADIUS.get(int(t) & MASK, 0.0) for t in ti])
    rj = np.array([RADIUS.get(int(t) & MASK, 0.0) for t in tj])
    d = (r - ri[:, None]) - rj[None, :]
    with np.errstate(all="ignore"):
        q1, q2 = d / 0.5, (d - 3.0) / 2.0
        gauss1, gauss2 = np.exp(-(q1 * q1)), np.exp(-(q2 * q2))
        repulsion = np.where(d < 0.0, d * d, 0.0)
        both_hyd = ((ti & HYD) != 0)[:, None] & ((tj & HYD) != 0)[None, :]
        hydrophobic = np.where(both_hyd, np.where(d < 0.5, 1.0, np.where(d < 1.5, 1.5 - d, 0.0)), 0.0)
        don_acc = (((ti & DON) != 0)[:, None] & ((tj & ACC) != 0)[None, :]) | (((ti & ACC) != 0)[:, None] & ((tj & DON) != 0)[None, :])
        hbond = np.where(don_acc, np.where(d < -0.7, 1.0, np.where(d < 0.0, (-d) / 0.7, 0.0)), 0.0)
    terms = np.stack([gauss1, gauss2, repulsion, hydrophobic, hbond])
    return np.where(within[None], terms, 0.0), within, d, don_acc


def batch_interactions(x_lig, z_lig, lig_ptr, x_rec, rec_type, rec_ptr, bond_ptr, bond_index, bond_kekule, bond_aromatic, implicit_h,
                       atom_flags, valence_status):
    """a batch as the entry takes it -> dict: atom_terms [n_lig, 5] float64, lig_type [n_lig] uint8, bond_rotatable [n_bonds] uint8,
    graph_terms [B, 5] float64, graph_out [B, 13] int32 -- every element the kernel writes; elements it does not write are nan / 255 --
    and atom_abs [n_lig, 5], graph_abs [B, 5]: per sum, the sum of the absolute values of its addends"""
    x_lig, x_rec = np.asarray(x_lig, np.float32).reshape(-1, 3), np.asarray(x_rec, np.float32).reshape(-1, 3)
    z_lig, rec_type = np.asarray(z_lig).reshape(-1), np.asarray(rec_type).reshape(-1)
    lig_ptr, rec_ptr, bond_ptr = (np.asarray(v, np.int64) for v in (lig_ptr, rec_ptr, bond_ptr))
    bond_index = np.asarray(bond_index, np.int64).reshape(2, -1)
    bond_kekule = np.asarray(bond_kekule).reshape(-1)
    n_lig, n_rec, n_bonds, B = len(z_lig), len(rec_type), bond_index.shape[1], len(lig_ptr) - 1
    bond_aromatic = np.zeros(n_bonds, np.uint8) if bond_aromatic is None else np.asarray(bond_aromatic).reshape(-1)
    atom_terms, atom_abs = np.full((n_lig, TERMS), np.nan), np.full((n_lig, TERMS), np.nan)
    graph_terms, graph_abs = np.full((B, TERMS), np.nan), np.full((B, TERMS), np.nan)
    lig_type, rotatable = np.full(n_lig, 255, np.uint8), np.full(n_bonds, 255, np.uint8)
    out = np.zeros((B, COLS), np.int32)
    for g in range(B):
        l0, l1 = _clamp(lig_ptr[g], lig_ptr[g + 1], n_lig)
        r0, r1 = _clamp(rec_ptr[g], rec_ptr[g + 1], n_rec)
        p0, p1 = int(bond_ptr[l0]), int(bond_ptr[l1])
        b0, b1 = _clamp(p0, p1, n_bonds)
        n, m = l1 - l0, b1 - b0
        no_valence = int(valence_status[g]) != 0
        bonds = [(int(bond_index[0, b]), int(bond_index[1, b])) for b in range(b0, b1)]
        bad = p0 != b0 or p1 != b1 or any(bond_ptr[a] > bond_ptr[a + 1] for a in range(l0, l1))
        bad = bad or any(not (l0 <= i < j < l1) for i, j in bonds) or any(not a < b for a, b in zip(bonds, bonds[1:]))
        bad = bad or (not no_valence and any(not 1 <= int(o) <= 4 for o in bond_kekule[b0:b1]))
        status = (TOO_MANY_ATOMS if n > MAX_ATOMS else 0) | (BAD_BONDS if bad else 0) | (NO_VALENCE if no_valence else 0)
        if status:
            out[g] = [n, m] + [-1] * (COLS - 3) + [status]
            atom_terms[l0:l1], lig_type[l0:l1], rotatable[b0:b1] = np.nan, 255, 255
            continue
        types, rot = ligand_graph(n, [(i - l0, j - l0) for i, j in bonds], [int(v) for v in z_lig[l0:l1]], bond_kekule[b0:b1],
                                  bond_aromatic[b0:b1], implicit_h[l0:l1], atom_flags[l0:l1])
        lig_type[l0:l1], rotatable[b0:b1] = types, rot
        terms, within, d, don_acc = pair_terms(x_lig[l0:l1], types, x_rec[r0:r1], rec_type[r0:r1])
        for t in range(TERMS):
            for a in range(n):
                row = terms[t, a][within[a]]
                atom_terms[l0 + a, t], atom_abs[l0 + a, t] = math.fsum(row), math.fsum(np.abs(row))
            flat = terms[t][within]
            graph_terms[g, t], graph_abs[g, t] = math.fsum(flat), math.fsum(np.abs(flat))
        tt = np.asarray(types, np.int64)
        out[g] = [n, m, sum(rot), int(((tt & DON) != 0).sum()), int(((tt & ACC) != 0).sum()), int(((tt & HYD) != 0).sum()),
                  int(within.sum()), int((terms[4] > 0).sum()), int((terms[3] > 0).sum()), int((within & (d < 0.0) & ~don_acc).sum()),
                  int((within & (d < 0.5)).any(1).sum()), int((rec_type[r0:r1] == UNTYPED).sum()), 0]
    return {"atom_terms": atom_terms, "lig_type": lig_type, "bond_rotatable": rotatable, "graph_terms": graph_terms, "graph_out": out,
            "atom_abs": atom_abs, "graph_abs": graph_abs}


def scores(graph_out, graph_terms):
    """(score_inter, score) per graph in float64, summed in index order; nan where status != 0"""
    inter, score = [], []
    for row, terms in zip(np.asarray(graph_out), np.asarray(graph_terms, np.float64)):
        if row[-1] != 0:
            inter.append(float("nan"))
            score.append(float("nan"))
            continue
        s = 0.0
        for w, v in zip(WEIGHTS, terms):
            s = s + w * float(v)
        inter.append(s)
        score.append(s / (1.0 + ROT_WEIGHT * float(row[2])))
    return np.array(inter), np.array(score)

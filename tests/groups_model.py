"""Plain Python restatement of the functional-group report's definition (include/cbgx.h, cbgx_ligand_groups; csrc/groups.hip), written
from that text alone: bond types, atom kinds, the three membership rules, group bonds, groups as connected components, and the class of a
group as isomorphism of labelled graphs.  The 25 template graphs are not copied from the library's table: they are PARSED here from their
names, which are SMILES strings (lower case: aromatic, bonds between aromatic neighbours type 4; the nitro name stands for N(=O)=O, as
the definition says).  Isomorphism is decided by a plain recursion over label-preserving partial maps of its own, which a brute force over
all permutations checks on small graphs.  What the GPU tests compare the kernel with, with ``==``."""
import itertools

import numpy as np

MAX_ATOMS, CLASSES, MAX_TEMPLATE_ATOMS, COLS = 256, 25, 10, 33
OTHER, NO_GROUP = 25, 254
TOO_MANY_ATOMS, BAD_BONDS, NO_AROMATIC = 1, 4, 8
NAMES = ("c1ccccc1", "NC=O", "O=CO", "c1ccncc1", "c1ncc2nc[nH]c2n1", "NS(=O)=O", "O=P(O)(O)O", "OCO", "c1cncnc1", "c1cn[nH]c1", "O=P(O)O",
         "c1ccc2ccccc2c1", "c1ccsc1", "N=CN", "NC(N)=O", "O=c1cc[nH]c(=O)[nH]1", "c1ccc2ncccc2c1", "c1cscn1", "c1ccc2[nH]cnc2c1",
         "c1c[nH]cn1", "O=[N+][O-]", "O=CNO", "NC(=O)O", "O=S=O", "c1ccc2[nH]ccc2c1")
COLUMNS = (("n_atoms", "n_bonds", "n_groups", "n_group_atoms", "n_named", "largest_group") + tuple(f"fg_{k}" for k in range(CLASSES))
           + ("n_other", "status"))
Z = {"H": 1, "C": 6, "N": 7, "O": 8, "F": 9, "P": 15, "S": 16, "Cl": 17}
HETERO, NOS = {7, 8, 9, 15, 16, 17}, {7, 8, 16}


def parse(name):
    """a SMILES string of the vocabulary -> (labels [(atomic number, aromatic)], {(i, j): type}): atoms, branches, ring-closure digits,
    '.', '-', '=' and '#', bracket atoms whose hydrogens and charges are dropped"""
    labels, bonds, stack, open_rings = [], {}, [], {}
    prev, pending, k = None, None, 0

    def join(a, b, order):
        t = order if order else (4 if labels[a][1] and labels[b][1] else 1)
        bonds[(min(a, b), max(a, b))] = t

    while k < len(name):
        ch = name[k]
        if ch == "(":
            stack.append(prev)
        elif ch == ")":
            prev = stack.pop()
        elif ch == ".":                       # the next atom starts a new piece
            prev, pending = None, None
        elif ch in "-=#":
            pending = "-=#".index(ch) + 1
        elif ch.isdigit():
            if ch in open_rings:
                other, order = open_rings.pop(ch)
                join(other, prev, order or pending)
            else:
                open_rings[ch] = (prev, pending)
            pending = None
        else:
            if ch == "[":
                end = name.index("]", k)
                symbol = name[k + 1:end].rstrip("+-")
                symbol = symbol[:-1] if len(symbol) > 1 and symbol.endswith("H") else symbol
                k = end
            elif name[k:k + 2] == "Cl":
                symbol, k = "Cl", k + 1
            else:
                symbol = ch
            labels.append((Z[symbol.capitalize()], symbol.islower()))
            if prev is not None:
                join(prev, len(labels) - 1, pending)
            prev, pending = len(labels) - 1, None
        k += 1
    assert not open_rings and not stack
    return labels, bonds


def _templates():
    out = []
    for name in NAMES:
        labels, bonds = parse(name)
        if name == "O=[N+][O-]":              # no charges: the graph N(=O)=O
            bonds = {e: 2 for e in bonds}
        out.append((labels, bonds))
    return out


TEMPLATES = _templates()


def isomorphic(labels_a, bonds_a, labels_b, bonds_b):
    """two labelled graphs (labels per atom; {(i, j) with i < j: type}): is there a bijection that keeps labels, bonds and bond types?
    Plain recursion over the atoms of a in their given order: every unused atom of b with the same label is tried as the image, and a
    partial map is dropped as soon as a pair of mapped atoms is bonded differently (type 0: not bonded) on the two sides"""
    if len(labels_a) != len(labels_b) or len(bonds_a) != len(bonds_b) or sorted(labels_a) != sorted(labels_b):
        return False
    type_a = lambda i, j: bonds_a.get((min(i, j), max(i, j)), 0)
    type_b = lambda i, j: bonds_b.get((min(i, j), max(i, j)), 0)
    n = len(labels_a)

    def extend(to):
        a = len(to)
        if a == n:
            return True
        for b in range(n):
            if b in to or labels_b[b] != labels_a[a]:
                continue
            if all(type_a(a, prev) == type_b(b, to[prev]) for prev in range(a)) and extend(to + [b]):
                return True
        return False

    return extend([])


def isomorphic_by_permutations(labels_a, bonds_a, labels_b, bonds_b):
    """the same question by brute force over all permutations: for small graphs, as a check of ``isomorphic``"""
    if len(labels_a) != len(labels_b) or len(bonds_a) != len(bonds_b):
        return False
    for to in itertools.permutations(range(len(labels_a))):
        if all(labels_b[to[a]] == labels_a[a] for a in range(len(to))) and \
                all(bonds_b.get((min(to[i], to[j]), max(to[i], to[j]))) == t for (i, j), t in bonds_a.items()):
            return True
    return False


def classify(labels, bonds):
    """the class of a group's labelled graph: the template it is isomorphic to, else OTHER; more atoms than any template: OTHER untested"""
    if len(labels) > MAX_TEMPLATE_ATOMS:
        return OTHER
    for k, (t_labels, t_bonds) in enumerate(TEMPLATES):
        if isomorphic(t_labels, t_bonds, labels, bonds):
            return k
    return OTHER


def graph_groups(n, pairs, z, order, aromatic):
    """one graph that passed the checks of the list -> (row [COLS - 1] without status, atom_group [n], atom_class [n], the groups in the
    order of their smallest atoms as (atoms, labels, {(u, v): type} on positions in ``atoms``, class))"""
    pairs = [(int(i), int(j)) for i, j in pairs]
    types = [4 if int(a) == 1 else int(o) for o, a in zip(order, aromatic)]
    nbrs = [[] for _ in range(n)]                              # (neighbour, type)
    for (i, j), t in zip(pairs, types):
        nbrs[i].append((j, t))
        nbrs[j].append((i, t))
    is_aromatic = [any(t == 4 for _, t in nbrs[a]) for a in range(n)]
    in_play = [z[a] in Z.values() and z[a] != 1 for a in range(n)]

    def single_only_nos(a):
        return z[a] in NOS and not is_aromatic[a] and all(t == 1 for _, t in nbrs[a])

    def on_hetero_triangle(a):
        plain = {b for b, t in nbrs[a] if t != 4}
        for b in plain:
            for c, t in nbrs[b]:
                if t != 4 and c in plain and (z[a] in NOS or z[b] in NOS or z[c] in NOS):
                    return True
        return False

    member = []
    for a in range(n):
        if not in_play[a]:
            member.append(False)
        elif is_aromatic[a] or z[a] in HETERO:
            member.append(True)
        else:                                                  # a non-aromatic carbon
            unsaturated = any(t in (2, 3) for _, t in nbrs[a])
            acetal = all(t == 1 for _, t in nbrs[a]) and sum(single_only_nos(b) for b, _ in nbrs[a]) >= 2
            member.append(unsaturated or acetal or on_hetero_triangle(a))

    def group_bond(i, j, t):
        if not (member[i] and member[j]):
            return False
        return t == 4 or (not is_aromatic[i] and not is_aromatic[j]) or (is_aromatic[i] != is_aromatic[j] and t == 2)

    seen, groups = set(), []                                   # flood fill from every unvisited member, smallest first
    for a in range(n):
        if not member[a] or a in seen:
            continue
        todo, atoms = [a], []
        seen.add(a)
        while todo:
            u = todo.pop()
            atoms.append(u)
            for v, t in nbrs[u]:
                if v not in seen and group_bond(u, v, t):
                    seen.add(v)
                    todo.append(v)
        atoms.sort()
        pos = {u: k for k, u in enumerate(atoms)}
        g_bonds = {(pos[i], pos[j]): t for (i, j), t in zip(pairs, types) if i in pos and j in pos and group_bond(i, j, t)}
        labels = [(z[u], is_aromatic[u]) for u in atoms]
        groups.append((atoms, labels, g_bonds, classify(labels, g_bonds)))
    atom_group, atom_class = [-1] * n, [NO_GROUP] * n
    fg = [0] * (CLASSES + 1)
    for atoms, _, _, cls in groups:
        fg[cls] += 1
        for u in atoms:
            atom_group[u], atom_class[u] = atoms[0], cls
    sizes = [len(g[0]) for g in groups]
    row = [n, len(pairs), len(groups), sum(sizes), len(groups) - fg[OTHER], max(sizes, default=0)] + fg
    return row, atom_group, atom_class, groups


def batch_groups(z, lig_ptr, n_lig, bond_ptr, bond_index, bond_order, bond_aromatic=None):
    """a batch as the entry takes it -> (atom_group [n_lig] int32, atom_class [n_lig] uint8, graph_out [B, 33] int32), every element the
    kernel writes; elements it does not write (atoms of no graph) are what 0xFF bytes read as: -1 and 255.  Ranges are clamped and lists
    checked as the header says."""
    lig_ptr, bond_ptr = np.asarray(lig_ptr, np.int64), np.asarray(bond_ptr, np.int64)
    bond_index = np.asarray(bond_index, np.int64).reshape(2, -1)
    z, bond_order = np.asarray(z).reshape(-1), np.asarray(bond_order).reshape(-1)
    n_bonds, B = bond_index.shape[1], len(lig_ptr) - 1
    bond_aromatic = np.zeros(n_bonds, np.uint8) if bond_aromatic is None else np.asarray(bond_aromatic).reshape(-1)
    grp, cls = np.full(n_lig, -1, np.int32), np.full(n_lig, 255, np.uint8)
    out = np.zeros((B, COLS), np.int32)
    for g in range(B):
        l0 = min(max(int(lig_ptr[g]), 0), n_lig)
        l1 = min(max(int(lig_ptr[g + 1]), l0), n_lig)
        p0, p1 = int(bond_ptr[l0]), int(bond_ptr[l1])
        b0 = min(max(p0, 0), n_bonds)
        b1 = min(max(p1, b0), n_bonds)
        n, m = l1 - l0, b1 - b0
        bonds = [(int(bond_index[0, b]), int(bond_index[1, b])) for b in range(b0, b1)]
        bad = p0 != b0 or p1 != b1 or any(bond_ptr[a] > bond_ptr[a + 1] for a in range(l0, l1))
        bad = bad or any(not (l0 <= i < j < l1) for i, j in bonds) or any(not a < b for a, b in zip(bonds, bonds[1:]))
        bad = bad or any(not 1 <= int(o) <= 3 for o in bond_order[b0:b1])
        status = ((TOO_MANY_ATOMS if n > MAX_ATOMS else 0) | (BAD_BONDS if bad else 0)
                  | (NO_AROMATIC if any(int(a) == 255 for a in bond_aromatic[b0:b1]) else 0))
        if status:
            out[g] = [n, m] + [-1] * (COLS - 3) + [status]
            grp[l0:l1], cls[l0:l1] = -2, 255
            continue
        row, atom_group, atom_class, _ = graph_groups(n, [(i - l0, j - l0) for i, j in bonds], [int(v) for v in z[l0:l1]],
                                                      bond_order[b0:b1], bond_aromatic[b0:b1])
        out[g] = row + [0]
        grp[l0:l1], cls[l0:l1] = atom_group, atom_class
    return grp, cls, out

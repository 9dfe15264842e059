"""Plain Python restatement of the aromatic report's definition (include/cbgx.h, cbgx_ligand_aromatic; csrc/aromatic.hip), written from
that text alone: chordless 5- and 6-cycles by a recursive walk over induced paths, the least fixed point of R2 and R3 by a loop that runs
until nothing changes, aromatic cycles, atoms and bonds, the limits and the status bits.  What the GPU tests compare the kernel with, with
``==``.  ``order`` (a ``random.Random`` or 'reversed') changes the order in which atoms and cycles are visited: the result may not."""
import numpy as np

MAX_ATOMS, MAX_CYCLES, COLS = 256, 128, 10
TOO_MANY_ATOMS, TOO_MANY_CYCLES, BAD_BONDS, NO_RINGS = 1, 2, 4, 8
COLUMNS = ("n_atoms", "n_bonds", "n_cycles56", "n_aromatic_cycles", "n_flagged", "n_closure", "n_aromatic_atoms", "n_aromatic_bonds",
           "n_unsupported", "status")


def chordless_cycles56(n, pairs):
    """every chordless simple cycle of length 5 or 6, as a tuple of atoms that starts at its smallest atom and runs towards the smaller of
    that atom's two cycle neighbours; sorted"""
    nbr = [set() for _ in range(n)]
    for i, j in pairs:
        nbr[i].add(j)
        nbr[j].add(i)
    found = []

    def walk(path):
        start, last = path[0], path[-1]
        for v in sorted(nbr[last]):
            if v <= start or v in path:
                continue
            # induced: v may be bonded to its predecessor, and to the start when that closes a cycle
            if any(v in nbr[u] for u in path[1:-1]):
                continue
            if v in nbr[start]:
                if len(path) + 1 >= 5 and path[1] < v:
                    found.append(tuple(path) + (v,))
                continue                            # shorter: a chord of anything longer
            if len(path) + 1 < 6:
                walk(path + [v])

    for a in range(n):
        for b in sorted(nbr[a]):
            if b > a:
                walk([a, b])
    return sorted(found)


def _shuffled(items, order):
    items = list(items)
    if order == "reversed":
        items.reverse()
    elif order is not None:
        order.shuffle(items)
    return items


def graph_aromatic(n, pairs, z, flags, ring_min, order=None):
    """one simple graph within the limits -> (row [COLS - 1] without status, in_closure [n], aromatic_atom [n], aromatic_bond [m])"""
    pairs = [(int(i), int(j)) for i, j in pairs]
    nbr = [set() for _ in range(n)]
    for i, j in pairs:
        nbr[i].add(j)
        nbr[j].add(i)
    cycles = _shuffled(chordless_cycles56(n, pairs), order)
    atoms = _shuffled(range(n), order)
    in_f = [bool(f) for f in flags]
    changed = True
    while changed:
        changed = False
        for a in atoms:                                  # R2
            if not in_f[a] and z[a] in (7, 8) and 3 <= ring_min[a] <= 9 and sum(in_f[w] for w in nbr[a]) >= 2:
                in_f[a] = changed = True
        for c in cycles:                                 # R3
            carbons = [a for a in c if z[a] == 6]
            if 2 * sum(in_f[a] for a in carbons) >= len(carbons) and not all(in_f[a] for a in c):
                for a in c:
                    in_f[a] = True
                changed = True
    aromatic = [c for c in cycles if all(in_f[a] for a in c)]
    on_atom = [False] * n
    edges = set()
    for c in aromatic:
        for k, a in enumerate(c):
            on_atom[a] = True
            b = c[(k + 1) % len(c)]
            edges.add((min(a, b), max(a, b)))
    on_bond = [e in edges for e in pairs]
    flagged = [bool(f) for f in flags]
    row = [n, len(pairs), len(cycles), len(aromatic), sum(flagged), sum(in_f), sum(on_atom), sum(on_bond),
           sum(f and not a for f, a in zip(flagged, on_atom))]
    return row, in_f, on_atom, on_bond


def batch_aromatic(z, flags, ring_min, lig_ptr, n_lig, bond_ptr, bond_index, order=None):
    """a batch as the entry takes it -> (atom_out [n_lig] uint8, bond_aromatic [n_bonds] uint8, graph_out [B, 10] int32), every element the
    kernel writes; elements it does not write (atoms and bonds of no graph) are 255 here.  Ranges are clamped and lists checked as the
    kernel does."""
    lig_ptr, bond_ptr = np.asarray(lig_ptr, np.int64), np.asarray(bond_ptr, np.int64)
    bond_index = np.asarray(bond_index, np.int64).reshape(2, -1)
    z, flags, ring_min = (np.asarray(v).reshape(-1) for v in (z, flags, ring_min))
    n_bonds, B = bond_index.shape[1], len(lig_ptr) - 1
    atom_out, bond_out, out = np.full(n_lig, 255, np.uint8), np.full(n_bonds, 255, np.uint8), np.zeros((B, COLS), np.int32)
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
        status = (TOO_MANY_ATOMS if n > MAX_ATOMS else 0) | (BAD_BONDS if bad else 0)
        if status == 0 and m >= n + MAX_CYCLES:
            status = TOO_MANY_CYCLES
        if any(int(v) == 255 for v in ring_min[l0:l1]):
            status |= NO_RINGS
        if status:
            out[g] = [n, m] + [-1] * (COLS - 3) + [status]
            atom_out[l0:l1] = 255
            bond_out[b0:b1] = 255
            continue
        row, in_f, on_atom, on_bond = graph_aromatic(n, [(i - l0, j - l0) for i, j in bonds], [int(v) for v in z[l0:l1]],
                                                     [int(v) != 0 for v in flags[l0:l1]], [int(v) for v in ring_min[l0:l1]], order)
        out[g] = row + [0]
        atom_out[l0:l1] = [int(f) | (int(a) << 1) for f, a in zip(in_f, on_atom)]
        bond_out[b0:b1] = [int(v) for v in on_bond]
    return atom_out, bond_out, out

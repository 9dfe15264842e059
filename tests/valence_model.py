"""Plain Python restatement of the valence report's definition (include/cbgx.h, cbgx_ligand_valence; csrc/valence.hip), written from that
text alone: the valence table, aromatic systems as connected components, candidates and must atoms, the eligible bonds in list order, the
recursive search ``node(p, M, dead)`` with its step count, Kekule orders, implicit hydrogens, flags, the per-graph columns, the limits and
the status bits.  What the GPU tests compare the kernel with, with ``==``."""
import numpy as np

MAX_ATOMS, MAX_ELIGIBLE, MAX_STEPS, COLS = 256, 64, 65536, 22
TOO_MANY_ATOMS, BAD_BONDS, NO_AROMATIC, SEARCH_LIMIT = 1, 4, 8, 16
EXCEEDED, ON_FAILED_SYSTEM, UNKNOWN_ELEMENT, ON_AROMATIC_SYSTEM = 1, 2, 4, 8
COLUMNS = (("n_atoms", "n_bonds", "n_fragments", "n_systems", "n_systems_failed", "n_kekule_double", "n_implicit_h", "n_exceeded",
            "n_unknown", "n_nhoh", "n_no") + tuple(f"el_{c}" for c in range(8)) + ("valence_ok", "steps_max", "status"))
ELEMENTS = (1, 6, 7, 8, 9, 15, 16, 17)                    # element codes 0 ... 7
VALENCES = {1: (1,), 6: (4,), 7: (3,), 8: (2,), 9: (1,), 15: (3, 5), 16: (2, 4, 6), 17: (1,)}


class SearchLimit(Exception):
    pass


def search(eligible, must, max_steps=MAX_STEPS):
    """the header's search on the eligible bonds ``[(i, j), ...]`` (list order) and the set of must atoms -> (the positions of M, sorted, or
    None: failed; steps).  Raises SearchLimit for more than MAX_ELIGIBLE bonds or atoms in them, or a search of more than max_steps steps"""
    m = len(eligible)
    last = {}
    for p, (i, j) in enumerate(eligible):
        last[i] = last[j] = p
    n_c = len(last)
    if m > MAX_ELIGIBLE or n_c > MAX_ELIGIBLE:
        raise SearchLimit
    if any(a not in last for a in must):
        return None, 1
    state = {"steps": 0, "best": None}
    matched = set()

    def node(p, chosen, dead):
        state["steps"] += 1
        if state["steps"] > max_steps:
            raise SearchLimit
        if p == m:
            if state["best"] is None or len(chosen) > len(state["best"]):
                state["best"] = list(chosen)
            return
        if state["best"] is not None and len(chosen) + (n_c - 2 * len(chosen) - dead) // 2 <= len(state["best"]):
            return
        i, j = eligible[p]
        if i not in matched and j not in matched:
            matched.update((i, j))
            node(p + 1, chosen + [p], dead)
            matched.difference_update((i, j))
        dying = [a for a in (i, j) if a not in matched and last[a] == p]
        if not any(a in must for a in dying):
            node(p + 1, chosen, dead + len(dying))

    node(0, [], 0)
    return state["best"], state["steps"]


def _components(n, pairs):
    """label [n]: the smallest atom of every atom's connected component"""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, j in pairs:
        ri, rj = find(i), find(j)
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    return [find(a) for a in range(n)]


def graph_valence(n, pairs, z, order, aromatic, max_steps=MAX_STEPS):
    """one graph that passed the checks of the list -> (row [COLS - 1] without status, implicit_h [n], flags [n], bond_kekule [m], the
    step counts of its systems in the order of their smallest atoms).  Raises SearchLimit"""
    pairs = [(int(i), int(j)) for i, j in pairs]
    is_aro = [int(a) == 1 for a in aromatic]
    k, s = [0] * n, [0] * n
    for (i, j), o, ar in zip(pairs, order, is_aro):
        for a in (i, j):
            if ar:
                k[a] += 1
            else:
                s[a] += int(o)
    system = _components(n, [e for e, ar in zip(pairs, is_aro) if ar])
    roots = sorted({system[a] for a in range(n) if k[a] > 0})
    candidate = [k[a] > 0 and z[a] in (6, 7) and VALENCES[z[a]][0] - s[a] - k[a] >= 1 for a in range(n)]
    kekule = [int(o) for o in order]
    failed_roots, steps, n_double = set(), [], 0
    for r in roots:
        rows = [b for b, ((i, j), ar) in enumerate(zip(pairs, is_aro)) if ar and system[i] == r]
        eligible_rows = [b for b in rows if candidate[pairs[b][0]] and candidate[pairs[b][1]]]
        must = {a for a in range(n) if system[a] == r and k[a] > 0 and candidate[a] and z[a] == 6}
        chosen, st = search([pairs[b] for b in eligible_rows], must, max_steps)
        steps.append(st)
        if chosen is None:
            failed_roots.add(r)
            for b in rows:
                kekule[b] = 4
            continue
        n_double += len(chosen)
        in_m = {eligible_rows[p] for p in chosen}
        for b in rows:
            kekule[b] = 2 if b in in_m else 1
    v = [0] * n
    for (i, j), t in zip(pairs, kekule):
        v[i] += 1 if t == 4 else t
        v[j] += 1 if t == 4 else t
    h, flags = [], []
    for a in range(n):
        table = VALENCES.get(z[a])
        fits = [t for t in table if t >= v[a]] if table else []
        h.append(fits[0] - v[a] if fits else 0)
        flags.append((EXCEEDED if table and not fits else 0) | (ON_FAILED_SYSTEM if k[a] > 0 and system[a] in failed_roots else 0)
                     | (0 if table else UNKNOWN_ELEMENT) | (ON_AROMATIC_SYSTEM if k[a] > 0 else 0))
    fragment = _components(n, pairs)
    n_exceeded, n_unknown = sum(bool(f & EXCEEDED) for f in flags), sum(bool(f & UNKNOWN_ELEMENT) for f in flags)
    row = [n, len(pairs), sum(fragment[a] == a for a in range(n)), len(roots), len(failed_roots), n_double, sum(h), n_exceeded, n_unknown,
           sum(z[a] in (7, 8) and h[a] >= 1 for a in range(n)), sum(zz in (7, 8) for zz in z)]
    row += [sum(zz == e for zz in z) for e in ELEMENTS]
    row += [int(n > 0 and n_exceeded == 0 and n_unknown == 0 and not failed_roots), max(steps, default=0)]
    return row, h, flags, kekule, steps


def batch_valence(z, lig_ptr, n_lig, bond_ptr, bond_index, bond_order, bond_aromatic=None, max_steps=MAX_STEPS):
    """a batch as the entry takes it -> (implicit_h [n_lig] uint8, atom_flags [n_lig] uint8, bond_kekule [n_bonds] uint8, graph_out
    [B, 22] int32), every element the kernel writes; elements it does not write (atoms and bonds of no graph) are 255 here.  Ranges are
    clamped and lists checked as the header says."""
    lig_ptr, bond_ptr = np.asarray(lig_ptr, np.int64), np.asarray(bond_ptr, np.int64)
    bond_index = np.asarray(bond_index, np.int64).reshape(2, -1)
    z, bond_order = np.asarray(z).reshape(-1), np.asarray(bond_order).reshape(-1)
    n_bonds, B = bond_index.shape[1], len(lig_ptr) - 1
    bond_aromatic = np.zeros(n_bonds, np.uint8) if bond_aromatic is None else np.asarray(bond_aromatic).reshape(-1)
    h_out, f_out, k_out = np.full(n_lig, 255, np.uint8), np.full(n_lig, 255, np.uint8), np.full(n_bonds, 255, np.uint8)
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
        if status == 0:
            try:
                row, h, flags, kekule, _ = graph_valence(n, [(i - l0, j - l0) for i, j in bonds], [int(v) for v in z[l0:l1]],
                                                         bond_order[b0:b1], bond_aromatic[b0:b1], max_steps)
            except SearchLimit:
                status = SEARCH_LIMIT
        if status:
            out[g] = [n, m] + [-1] * (COLS - 3) + [status]
            h_out[l0:l1] = f_out[l0:l1] = 255
            k_out[b0:b1] = 255
            continue
        out[g] = row + [0]
        h_out[l0:l1], f_out[l0:l1], k_out[b0:b1] = h, flags, kekule
    return h_out, f_out, k_out, out

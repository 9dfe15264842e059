"""Plain Python / numpy restatement of the ring sizes' definition (include/cbgx.h, cbgx_ligand_rings; csrc/rings.hip): Horton candidates from
breadth-first trees cut at depth 4, GF(2) elimination by size class, the smallest ring of an atom from the branch labels of its own tree,
the limits and the status bits.  What the GPU tests compare the kernel with, with ``==``.  The trees here are the deterministic ones of a
queue over sorted adjacency lists; the kernel's are whatever its lanes claim first: the definition does not depend on the trees."""
import collections

import numpy as np

MAX_SIZE, MAX_ATOMS, MAX_CYCLES, COLS = 9, 256, 128, 13
TOO_MANY_ATOMS, TOO_MANY_CYCLES, BAD_BONDS = 1, 2, 4
DEPTH = MAX_SIZE // 2


def _bfs(adj, root):
    """depth, parent and branch (the child of the root an atom hangs under) of every atom within DEPTH of ``root``"""
    depth, parent, branch = {root: 0}, {root: None}, {root: None}
    queue = collections.deque([root])
    while queue:
        u = queue.popleft()
        if depth[u] == DEPTH:
            continue
        for w in adj[u]:
            if w not in depth:
                depth[w], parent[w], branch[w] = depth[u] + 1, u, (w if u == root else branch[u])
                queue.append(w)
    return depth, parent, branch


def components(n, pairs):
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, j in pairs:
        parent[find(i)] = find(j)
    return len({find(a) for a in range(n)})


def graph_rings(n, pairs):
    """one simple graph within the limits (``pairs``: distinct (i, j), i < j < n) -> (rings [7] for the sizes 3 ... 9, n_cycles,
    atom_ring_min [n]).  A cycle-space vector is a Python integer with one bit per bond."""
    pairs = [(int(i), int(j)) for i, j in pairs]
    bond = {e: b for b, e in enumerate(pairs)}
    adj = [[] for _ in range(n)]
    for i, j in pairs:
        adj[i].append(j)
        adj[j].append(i)
    for a in adj:
        a.sort()
    candidates, ring_min = [], [0] * n
    for root in range(n):
        depth, parent, branch = _bfs(adj, root)

        def path(x):
            v = 0
            while parent[x] is not None:
                v ^= 1 << bond[(min(x, parent[x]), max(x, parent[x]))]
                x = parent[x]
            return v

        for x, y in pairs:
            if x in depth and y in depth and parent[x] != y and parent[y] != x:
                length = depth[x] + depth[y] + 1
                if length <= MAX_SIZE:
                    candidates.append((length, path(x) ^ path(y) ^ (1 << bond[(x, y)])))
                    # a bond at the root is a tree edge, so both ends have a branch
                    if branch[x] != branch[y] and (ring_min[root] == 0 or length < ring_min[root]):
                        ring_min[root] = length
    rings, basis = [0] * (MAX_SIZE - 2), {}
    for k in range(3, MAX_SIZE + 1):
        for length, v in candidates:
            if length != k:
                continue
            while v:
                p = v.bit_length() - 1
                if p not in basis:
                    basis[p] = v
                    rings[k - 3] += 1
                    break
                v ^= basis[p]
    return rings, len(pairs) - n + components(n, pairs), ring_min


def batch_rings(lig_ptr, n_lig, bond_ptr, bond_index):
    """a batch as the entry takes it -> (atom_ring_min [n_lig] uint8, graph_out [B, 13] int32), every element the kernel writes; elements it
    does not write (atoms of no graph) are 255 here.  Ranges are clamped and lists checked as the kernel does."""
    lig_ptr, bond_ptr = np.asarray(lig_ptr, np.int64), np.asarray(bond_ptr, np.int64)
    bond_index = np.asarray(bond_index, np.int64).reshape(2, -1)
    n_bonds, B = bond_index.shape[1], len(lig_ptr) - 1
    ring_min, out = np.full(n_lig, 255, np.uint8), np.zeros((B, COLS), np.int32)
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
        if status == 0:
            local = [(i - l0, j - l0) for i, j in bonds]
            if m - n + components(n, local) > MAX_CYCLES:
                status = TOO_MANY_CYCLES
        if status:
            out[g] = [n, m] + [-1] * (COLS - 3) + [status]
            ring_min[l0:l1] = 255
            continue
        rings, n_cycles, rmin = graph_rings(n, local)
        ring_min[l0:l1] = rmin
        out[g] = [n, m, n_cycles] + rings + [n_cycles - sum(rings), sum(1 for v in rmin if v > 0), 0]
    return ring_min, out

"""numpy restatement of the bond list's definition (include/cbgx.h, cbgx_ligand_bonds_count / cbgx_ligand_bonds_fill; csrc/geometry.hip),
built on tests/geometry_model.py: the pairs i < j with a table bond order > 0 in (i, j) order, their orders and the float64 distances the
orders were decided on, connected components by plain union-find (label = smallest index of the component) and the six per-graph counts.
What the GPU tests compare the kernels with, with ``==``."""
import numpy as np

from tests import geometry_model as GM


def components(n, pairs):
    """label [n] int32 = the smallest index of the connected component, by union-find over ``pairs`` (iterable of (i, j))"""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, j in pairs:
        ri, rj = find(int(i)), find(int(j))
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)        # the smaller root stays: a root is the smallest index of its set
    return np.array([find(a) for a in range(n)], np.int32).reshape(n)


def graph_bonds(x_lig, z_lig):
    """one graph -> dict(bond_index [2, nb] int32 local rows with i < j in (i, j) order, bond_order [nb] uint8, bond_length [nb] float64,
    deg_up [n] int32, fragment [n] int32, counts [6] int32: n_atoms, n_bonds, bond_order_sum, n_fragments, largest_fragment, n_cycles)"""
    x_lig = np.asarray(x_lig, np.float32).reshape(-1, 3)
    order, _, dist = GM.bond_orders(x_lig, z_lig)
    n = x_lig.shape[0]
    upper = np.triu(order, 1)
    i, j = np.nonzero(upper)                         # row-major: (i, j) lexicographic
    fragment = components(n, zip(i.tolist(), j.tolist()))
    sizes = np.bincount(fragment, minlength=n) if n else np.zeros(0, np.int64)
    n_frag = int((fragment == np.arange(n)).sum())
    nb = len(i)
    counts = np.array([n, nb, int(upper.sum()), n_frag, int(sizes.max()) if n else 0, nb - n + n_frag], np.int32)
    return {"bond_index": np.stack([i, j]).astype(np.int32).reshape(2, nb), "bond_order": upper[i, j].astype(np.uint8),
            "bond_length": dist[i, j].astype(np.float64), "deg_up": (upper > 0).sum(1).astype(np.int32).reshape(n),
            "fragment": fragment, "counts": counts}


def batch_bonds(x_lig, z_lig, lig_ptr):
    """a batch in CSR form -> dict(bond_index [2, nb] int32 GLOBAL rows, bond_order, bond_length, bond_graph [nb] int64, deg_up [n_lig],
    fragment [n_lig] (ligand-local labels), graph_counts [B, 6] int32)"""
    x_lig, z_lig = np.asarray(x_lig, np.float32).reshape(-1, 3), np.asarray(z_lig).reshape(-1)
    B = len(lig_ptr) - 1
    out = {"bond_index": [np.zeros((2, 0), np.int32)], "bond_order": [np.zeros(0, np.uint8)], "bond_length": [np.zeros(0, np.float64)],
           "bond_graph": [np.zeros(0, np.int64)], "deg_up": [np.zeros(0, np.int32)], "fragment": [np.zeros(0, np.int32)]}
    gc = np.zeros((B, 6), np.int32)
    for g in range(B):
        l0, l1 = int(lig_ptr[g]), int(lig_ptr[g + 1])
        r = graph_bonds(x_lig[l0:l1], z_lig[l0:l1])
        gc[g] = r["counts"]
        out["bond_index"].append(r["bond_index"] + np.int32(l0))
        out["bond_graph"].append(np.full(r["bond_index"].shape[1], g, np.int64))
        for k in ("bond_order", "bond_length", "deg_up", "fragment"):
            out[k].append(r[k])
    res = {k: np.concatenate(v, axis=1 if k == "bond_index" else 0) for k, v in out.items()}
    res["graph_counts"] = gc
    return res

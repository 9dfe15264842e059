"""numpy restatement of the distributions' definition (include/cbgx.h, cbgx_ligand_pair_hist / cbgx_ligand_angles; csrc/distributions.hip),
built on tests/geometry_model.py and tests/bonds_model.py: pair-distance histograms of two families, bond-length bins and types of the
table-bond list, and the bond angles of that graph in (c, a, b) order with cosine, bin against a cosine table and canonical type.
What the GPU tests compare the kernels with, with ``==`` (nan where the definition says nan).

numpy rounds every elementwise product, sum and quotient on its own and its sqrt is correctly rounded, so the expressions below ARE the
definition: u = x_a - x_c, v = x_b - x_c on float32 coordinates widened to float64, dot = (ux vx + uy vy) + uz vz, su = (ux ux + uy uy) +
uz uz, cos = dot / sqrt(su sv), clamped to [-1, 1]; bin = the number of table entries strictly greater than cos."""
import numpy as np

from cbgbench_amd import geometry as G
from tests import bonds_model as BM
from tests import geometry_model as GM

DEGENERATE = G.ANGLE_BIN_DEGENERATE
LIMIT = G.MAX_ANGLES_PER_GRAPH
TOO_MANY = G.DISTRIBUTIONS_TOO_MANY_ANGLES


def pair_hist(x_lig, z_lig, edges_all, edges_cc):
    """one graph -> [2, E_max + 1] int32: family 0 every pair i < j, family 1 pairs of two carbons; a pair takes part iff
    d < edges[-1] and its bin is np.searchsorted(edges, d) (side left: the number of edges strictly less than d)"""
    x_lig, z = np.asarray(x_lig, np.float32).reshape(-1, 3), np.asarray(z_lig).reshape(-1)
    i, j = np.triu_indices(x_lig.shape[0], 1)
    d = GM.distances(x_lig, x_lig)[i, j]
    cc = (z[i] == 6) & (z[j] == 6)
    cols = max(len(edges_all), len(edges_cc)) + 1
    out = np.zeros((2, cols), np.int32)
    for f, (edges, member) in enumerate(((edges_all, np.ones(len(d), bool)), (edges_cc, cc))):
        edges = np.asarray(edges, np.float64)
        if len(edges):
            take = member & (d < edges[-1])
            out[f] = np.bincount(np.searchsorted(edges, d[take], side="left"), minlength=cols)
    return out


def bond_bins(bond_length, edges):
    """[nb] uint8: the number of edges strictly less than the length"""
    return np.searchsorted(np.asarray(edges, np.float64), np.asarray(bond_length, np.float64), side="left").astype(np.uint8)


def bond_types(bond_index, bond_order, code):
    """[nb] int16: ((order - 1) 8 + code_lo) 8 + code_hi over the element codes of the two (local) rows"""
    ci, cj = code[bond_index[0]], code[bond_index[1]]
    return (((bond_order.astype(np.int64) - 1) * 8 + np.minimum(ci, cj)) * 8 + np.maximum(ci, cj)).astype(np.int16)


def angle_types(ca, oa, cc, ob, cb):
    """canonical type codes of angles (arrays): the smaller (code, order) end first"""
    ca, oa, cc, ob, cb = (np.asarray(v, np.int64) for v in (ca, oa, cc, ob, cb))
    swap = (ca > cb) | ((ca == cb) & (oa > ob))
    c1, o1, c2, o2 = np.where(swap, cb, ca), np.where(swap, ob, oa), np.where(swap, ca, cb), np.where(swap, oa, ob)
    return ((((c1 * 3 + (o1 - 1)) * 8 + cc) * 3 + (o2 - 1)) * 8 + c2).astype(np.int16)


def angle_cosines(x_lig, a, c, b):
    """float64 cosines of the angles (a, c, b) in the definition's order of operations, clamped; nan for a degenerate angle"""
    x = np.asarray(x_lig, np.float32).astype(np.float64).reshape(-1, 3)
    u, v = x[a] - x[c], x[b] - x[c]
    uv, uu, vv = u * v, u * u, v * v
    dot = (uv[:, 0] + uv[:, 1]) + uv[:, 2]
    su, sv = (uu[:, 0] + uu[:, 1]) + uu[:, 2], (vv[:, 0] + vv[:, 1]) + vv[:, 2]
    prod = su * sv
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = dot / np.sqrt(prod)
    degenerate = (prod == 0.0) | np.isnan(cos)
    return np.where(degenerate, np.nan, np.clip(cos, -1.0, 1.0))


def angle_bins(cos, cos_edges):
    """[n] uint8: the number of entries of the decreasing table strictly greater than cos; DEGENERATE where cos is nan"""
    cos_edges = np.asarray(cos_edges, np.float64)
    with np.errstate(invalid="ignore"):
        bins = (cos_edges[None, :] > cos[:, None]).sum(1)
    return np.where(np.isnan(cos), DEGENERATE, bins).astype(np.uint8)


def graph_angles(x_lig, z_lig, cos_edges, bonds=None):
    """one graph -> dict(angle_index [3, n] int32 local rows (a, c, b), a < b partners of c, in (c, a, b) order; angle_cos [n] float64;
    angle_bin [n] uint8; angle_type [n] int16; counts [5] int32: n_atoms, n_bonds, n_angles, n_degenerate_angles, status).  A graph whose
    sum of C(deg, 2) exceeds LIMIT has status TOO_MANY and no angles"""
    x_lig, z_lig = np.asarray(x_lig, np.float32).reshape(-1, 3), np.asarray(z_lig).reshape(-1)
    n = x_lig.shape[0]
    bonds = BM.graph_bonds(x_lig, z_lig) if bonds is None else bonds
    bi, bo = bonds["bond_index"].astype(np.int64), bonds["bond_order"].astype(np.int64)
    code = GM._codes(z_lig, GM.tables()["elements"])
    deg = np.bincount(np.concatenate([bi[0], bi[1]]), minlength=n)
    total = int((deg * (deg - 1) // 2).sum())
    rows = []
    if total <= LIMIT:
        partners = [[] for _ in range(n)]
        for (i, j), o in zip(bi.T.tolist(), bo.tolist()):      # bonds in (i, j) order: every list comes out ascending
            partners[i].append((j, o))
            partners[j].append((i, o))
        for c in range(n):
            ps = sorted(partners[c])
            rows += [(a, c, b, oa, ob) for k, (a, oa) in enumerate(ps) for b, ob in ps[k + 1:]]
    r = np.array(rows, np.int64).reshape(-1, 5)
    a, c, b, oa, ob = r.T
    cos = angle_cosines(x_lig, a, c, b)
    bins = angle_bins(cos, cos_edges)
    counts = np.array([n, bi.shape[1], len(r), int((bins == DEGENERATE).sum()), 0 if total <= LIMIT else TOO_MANY], np.int32)
    return {"angle_index": np.stack([a, c, b]).astype(np.int32).reshape(3, -1), "angle_cos": cos, "angle_bin": bins,
            "angle_type": angle_types(code[a], oa, code[c], ob, code[b]), "counts": counts}


def batch_distributions(x_lig, z_lig, lig_ptr, edges_all=None, edges_cc=None, bond_edges=None, cos_edges=None):
    """a batch in CSR form -> dict(pair_hist [B, 2, E_max + 1] int32; bond_bin [nb] uint8, bond_type [nb] int16 and the bond list itself
    (tests/bonds_model.py, GLOBAL rows); angle_index [3, n] int32 GLOBAL rows, angle_cos, angle_bin, angle_type, angle_graph [n] int64;
    graph_counts [B, 5] int32).  Default edges: the package's"""
    x_lig, z_lig = np.asarray(x_lig, np.float32).reshape(-1, 3), np.asarray(z_lig).reshape(-1)
    da, dc = G.default_pair_edges()
    edges_all, edges_cc = da if edges_all is None else edges_all, dc if edges_cc is None else edges_cc
    bond_edges = G.default_bond_edges() if bond_edges is None else bond_edges
    cos_edges = G.default_cos_edges() if cos_edges is None else cos_edges
    B = len(lig_ptr) - 1
    cols = max(len(edges_all), len(edges_cc)) + 1
    out = {"angle_index": [np.zeros((3, 0), np.int32)], "angle_cos": [np.zeros(0, np.float64)], "angle_bin": [np.zeros(0, np.uint8)],
           "angle_type": [np.zeros(0, np.int16)], "angle_graph": [np.zeros(0, np.int64)], "bond_bin": [np.zeros(0, np.uint8)],
           "bond_type": [np.zeros(0, np.int16)], "bond_index": [np.zeros((2, 0), np.int32)], "bond_order": [np.zeros(0, np.uint8)],
           "bond_length": [np.zeros(0, np.float64)], "bond_graph": [np.zeros(0, np.int64)]}
    pairs, gc = np.zeros((B, 2, cols), np.int32), np.zeros((B, 5), np.int32)
    for g in range(B):
        l0, l1 = int(lig_ptr[g]), int(lig_ptr[g + 1])
        x, z = x_lig[l0:l1], z_lig[l0:l1]
        bonds = BM.graph_bonds(x, z)
        r = graph_angles(x, z, cos_edges, bonds)
        pairs[g], gc[g] = pair_hist(x, z, edges_all, edges_cc), r["counts"]
        code = GM._codes(z, GM.tables()["elements"])
        out["angle_index"].append(r["angle_index"] + np.int32(l0))
        out["angle_graph"].append(np.full(r["angle_index"].shape[1], g, np.int64))
        for k in ("angle_cos", "angle_bin", "angle_type"):
            out[k].append(r[k])
        out["bond_bin"].append(bond_bins(bonds["bond_length"], bond_edges))
        out["bond_type"].append(bond_types(bonds["bond_index"], bonds["bond_order"], code))
        out["bond_index"].append(bonds["bond_index"] + np.int32(l0))
        out["bond_graph"].append(np.full(bonds["bond_index"].shape[1], g, np.int64))
        out["bond_order"].append(bonds["bond_order"])
        out["bond_length"].append(bonds["bond_length"])
    res = {k: np.concatenate(v, axis=1 if k.endswith("_index") else 0) for k, v in out.items()}
    res["pair_hist"], res["graph_counts"] = pairs, gc
    return res


def adjacency(bond_index, bond_order, n_lig):
    """the symmetric adjacency of a bond list (GLOBAL rows): adj_ptr [n_lig + 1] int32, adj_nbr [2 nb] int32 ascending per centre,
    adj_order [2 nb] uint8, and the per-centre numbers of angles C(deg, 2) [n_lig] int64"""
    bi = np.asarray(bond_index, np.int64).reshape(2, -1)
    centre, nbr = np.concatenate([bi[0], bi[1]]), np.concatenate([bi[1], bi[0]])
    perm = np.lexsort((nbr, centre))
    deg = np.bincount(centre, minlength=n_lig)
    return (np.concatenate([[0], np.cumsum(deg)]).astype(np.int32), nbr[perm].astype(np.int32),
            np.concatenate([bond_order, bond_order])[perm].astype(np.uint8), deg * (deg - 1) // 2)


def as_package_dict(res, bins=G.DISTRIBUTION_BINS):
    """a result of ``batch_distributions`` above with the per-graph sparse histograms the package's ``batch_distributions`` returns
    beside its lists (sorted non-zero cells of the dense [B, types, bins] tables; degenerate angles left out): what
    ``geometry.distribution_totals`` takes"""
    def sparse(graph, code, bins_, n_codes, n_bins):
        key = (graph.astype(np.int64) * n_codes + code.astype(np.int64)) * n_bins + bins_.astype(np.int64)
        key, count = np.unique(key, return_counts=True)
        return np.stack([key // (n_codes * n_bins), key // n_bins % n_codes, key % n_bins]).astype(np.int32), count.astype(np.int32)

    out = dict(res)
    out["bond_hist_index"], out["bond_hist_count"] = sparse(res["bond_graph"], res["bond_type"], res["bond_bin"], G.N_BOND_TYPES, bins[1])
    ok = res["angle_bin"] != DEGENERATE
    out["angle_hist_index"], out["angle_hist_count"] = sparse(res["angle_graph"][ok], res["angle_type"][ok], res["angle_bin"][ok],
                                                              G.N_ANGLE_TYPES, bins[2])
    return out

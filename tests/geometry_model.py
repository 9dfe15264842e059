"""numpy float64 restatement of the geometry report's definition (include/cbgx.h, cbgx_ligand_geometry; csrc/geometry.hip): what the GPU
tests compare the kernel with, bit for bit, and what tests/test_geometry.py compares with the reference's check_stability / detect_clash.
The constants come from the library (cbgx_ligand_geometry_tables): nothing is restated here.

numpy rounds every elementwise product and sum on its own and its sqrt is correctly rounded, so the expressions below ARE the definition:
coordinates as float32 widened to float64, dx = xi - xj, s = (dx dx + dy dy) + dz dz, d = sqrt(s), p = 100.0 d."""
import numpy as np

from cbgbench_amd import geometry as G

STABLE, INTER, INTRA, UNKNOWN = G.STABLE, G.INTER_CLASH, G.INTRA_CLASH, G.UNKNOWN_ELEMENT
_TABLES = None


def tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = G.tables()
    return _TABLES


def _codes(z, atomic_numbers):
    """index of every z in atomic_numbers, -1 when absent"""
    z = np.asarray(z).astype(np.int64).reshape(-1)
    code = np.full(z.shape, -1, np.int64)
    for c, zc in enumerate(atomic_numbers):
        code[z == int(zc)] = c
    return code


def distances(a, b):
    """[len(a), len(b)] float64 distances of float32 coordinates, in the definition's order of operations"""
    a = np.asarray(a, np.float32).astype(np.float64).reshape(-1, 3)
    b = np.asarray(b, np.float32).astype(np.float64).reshape(-1, 3)
    d = a[:, None, :] - b[None, :, :]
    sq = d * d
    return np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])


def bond_orders(x_lig, z_lig):
    """([n, n] table bond orders with a zero diagonal and zero rows / columns for unknown elements, element codes, distances)"""
    T = tables()
    code = _codes(z_lig, T["elements"])
    known = code >= 0
    ci = np.where(known, code, 0)
    dist = distances(x_lig, x_lig)
    p = 100.0 * dist
    b = T["bond_pm"][:, ci[:, None], ci[None, :]].astype(np.float64)
    t1, t2, t3 = (b[o] + float(T["margins"][o]) for o in range(3))
    order = np.where(p < t1, np.where(p < t2, np.where(p < t3, 3, 2), 1), 0)
    pair = known[:, None] & known[None, :] & ~np.eye(len(ci), dtype=bool)
    return order * pair, code, dist


def graph_geometry(x_lig, z_lig, x_rec, z_rec):
    """one graph -> (nr_bonds [n] int32, flags [n] uint8, counts [6] int32)"""
    T = tables()
    order, code, dist = bond_orders(x_lig, z_lig)
    n = len(code)
    known = code >= 0
    ci = np.where(known, code, 0)
    pair = known[:, None] & known[None, :] & ~np.eye(n, dtype=bool)
    nr = order.sum(1).astype(np.int32)
    stable = known & (nr > 0) & (nr <= T["allowed"][ci])
    r_lig = T["vdw_r"][ci]           # (element codes 0..7 are the first eight radius codes: elements == vdw_z[:8], asserted in the tests)
    intra = ((dist < (r_lig[:, None] + r_lig[None, :]) - T["tolerance"]) & pair & (order == 0)).any(1)
    rcode = _codes(z_rec, T["vdw_z"])
    has_r = rcode >= 0
    r_rec = T["vdw_r"][np.where(has_r, rcode, 0)]
    d_lr = distances(x_lig, x_rec)
    inter = ((d_lr < (r_lig[:, None] + r_rec[None, :]) - T["tolerance"]) & known[:, None] & has_r[None, :]).any(1)
    flags = (stable * STABLE + inter * INTER + intra * INTRA + (~known) * UNKNOWN).astype(np.uint8)
    n_stable = int(stable.sum())
    counts = np.array([n, n_stable, int(n_stable == n and n > 0), int(inter.sum()), int(intra.sum()), int((~has_r).sum())], np.int32)
    return nr, flags, counts


def batch_geometry(x_lig, z_lig, lig_ptr, x_rec, z_rec, rec_ptr):
    """a batch in CSR form -> dict(nr_bonds [n_lig] int32, flags [n_lig] uint8, graph_counts [B, 6] int32)"""
    x_lig, x_rec = np.asarray(x_lig, np.float32).reshape(-1, 3), np.asarray(x_rec, np.float32).reshape(-1, 3)
    z_lig, z_rec = np.asarray(z_lig).reshape(-1), np.asarray(z_rec).reshape(-1)
    B = len(lig_ptr) - 1
    nr, fl, gc = [np.zeros(0, np.int32)], [np.zeros(0, np.uint8)], np.zeros((B, 6), np.int32)
    for g in range(B):
        l0, l1, r0, r1 = int(lig_ptr[g]), int(lig_ptr[g + 1]), int(rec_ptr[g]), int(rec_ptr[g + 1])
        a, b, gc[g] = graph_geometry(x_lig[l0:l1], z_lig[l0:l1], x_rec[r0:r1], z_rec[r0:r1])
        nr.append(a)
        fl.append(b)
    return {"nr_bonds": np.concatenate(nr), "flags": np.concatenate(fl), "graph_counts": gc}

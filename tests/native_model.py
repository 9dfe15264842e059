"""A numpy / Python-int model of cbgx_pocket_contacts and cbgx_native_compare, written from the text of include/cbgx.h: float64 numpy
scalars (every product and sum rounded once, nothing fused), Python ints for the counts and the rounding.  No GPU, no library."""
import numpy as np

CUTOFF2 = 16.0
CONTACT_COLS, SAMPLE_COLS, GROUP_COLS, WORDS = 6, 6, 9, 32
EMPTY = 16
SAMPLE_NOT_EVALUATED, NATIVE_NOT_EVALUATED, POCKET_MISMATCH, BAD_GROUPS = 1, 2, 4, 8
MAX_LIGAND = 1024


def clamp_range(ptr, g, n):
    a = min(max(int(ptr[g]), 0), n)
    return a, min(max(int(ptr[g + 1]), a), n)


def dist2(a, b):
    """d2 = (dx dx + dy dy) + dz dz of two points given as float32 or float64 triples, in float64"""
    dx, dy, dz = (np.float64(a[k]) - np.float64(b[k]) for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def micro(common, union):
    return (common * 1000000 + union // 2) // union if union else 0


def pocket_contacts(x_lig, z_lig, lig_ptr, x_rec, z_rec, rec_ptr, n_graphs, cutoff2=CUTOFF2, fill=0xFF):
    """-> rec_contact [n_rec] uint8, lig_contact [n_lig] uint8, centroid [B, 3] float64, graph_out [B, 6] int32; rows of no graph
    keep ``fill``"""
    x_lig, x_rec = np.asarray(x_lig, np.float32).reshape(-1, 3), np.asarray(x_rec, np.float32).reshape(-1, 3)
    n_lig, n_rec = x_lig.shape[0], x_rec.shape[0]
    rec_contact, lig_contact = np.full(n_rec, fill, np.uint8), np.full(n_lig, fill, np.uint8)
    centroid, graph_out = np.zeros((n_graphs, 3), np.float64), np.zeros((n_graphs, CONTACT_COLS), np.int32)
    cutoff2 = np.float64(cutoff2)
    for g in range(n_graphs):
        l0, l1 = clamp_range(lig_ptr, g, n_lig)
        r0, r1 = clamp_range(rec_ptr, g, n_rec)
        assert l1 - l0 <= MAX_LIGAND
        heavy = [a for a in range(l0, l1) if z_lig[a] != 1]
        rec_contact[r0:r1], lig_contact[l0:l1] = 0, 0
        if heavy and r1 > r0:
            hx = x_lig[heavy].astype(np.float64)
            for r in range(r0, r1):
                if z_rec[r] == 1:
                    continue
                d = hx - x_rec[r].astype(np.float64)[None, :]          # exact: float32 differences fit float64
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                hit = d2 <= cutoff2
                if hit.any():
                    rec_contact[r] = 1
                    lig_contact[np.asarray(heavy)[hit]] = 1
        s = [np.float64(0.0)] * 3
        for a in heavy:                                                # one float64 addition after the other, in atom order
            s = [s[k] + np.float64(x_lig[a, k]) for k in range(3)]
        with np.errstate(invalid="ignore", divide="ignore"):
            centroid[g] = [s[k] / np.float64(len(heavy)) for k in range(3)] if heavy else [np.nan] * 3
        graph_out[g] = [l1 - l0, len(heavy), r1 - r0, int(rec_contact[r0:r1].sum()), int(lig_contact[l0:l1].sum()), 0 if heavy else EMPTY]
    return rec_contact, lig_contact, centroid, graph_out


def native_compare(fp, mol_hash, fp_status, rec_contact, rec_ptr, centroid, contacts_status, fp_nat, mol_hash_nat, fp_status_nat,
                   rec_contact_nat, rec_ptr_nat, centroid_nat, contacts_status_nat, group_ptr, fill=-1):
    """-> sample_out [B, 6] int64, centroid_d2 [B] float64, group_out [P, 9] int64; rows of a graph in no group keep ``fill`` (the
    float: its bit pattern repeated)"""
    n_graphs, n_groups = len(mol_hash), len(mol_hash_nat)
    n_rec, n_rec_nat = len(rec_contact), len(rec_contact_nat)
    words = lambda row: [int(v) & 0xFFFFFFFF for v in row]
    sample_out = np.full((n_graphs, SAMPLE_COLS), fill, np.int64)
    centroid_d2 = np.full(n_graphs, fill, np.int64).view(np.float64).copy()
    group_out = np.zeros((n_groups, GROUP_COLS), np.int64)
    for p in range(n_groups):
        g0, g1 = clamp_range(group_ptr, p, n_graphs)
        q0, q1 = clamp_range(rec_ptr_nat, p, n_rec_nat)
        nat_ok = int(fp_status_nat[p]) == 0
        n_fp = n_same = sim_sum = n_contact = contact_sum = 0
        sim_max = contact_max = -1
        for g in range(g0, g1):
            r0, r1 = clamp_range(rec_ptr, g, n_rec)
            fp_ok, same_pocket = nat_ok and int(fp_status[g]) == 0, r1 - r0 == q1 - q0
            sim = same = common = union = jac = -1
            if fp_ok:
                a, b = words(fp[g]), words(fp_nat[p])
                sim = micro(sum(bin(x & y).count("1") for x, y in zip(a, b)), sum(bin(x | y).count("1") for x, y in zip(a, b)))
                same = int(int(mol_hash[g]) & (2 ** 64 - 1) == int(mol_hash_nat[p]) & (2 ** 64 - 1))
                n_fp, n_same, sim_sum, sim_max = n_fp + 1, n_same + same, sim_sum + sim, max(sim_max, sim)
            if same_pocket:
                mine, theirs = np.asarray(rec_contact[r0:r1]) != 0, np.asarray(rec_contact_nat[q0:q1]) != 0
                common, union = int((mine & theirs).sum()), int((mine | theirs).sum())
                jac = micro(common, union)
                n_contact, contact_sum, contact_max = n_contact + 1, contact_sum + jac, max(contact_max, jac)
            status = ((SAMPLE_NOT_EVALUATED if int(fp_status[g]) != 0 else 0) | (0 if nat_ok else NATIVE_NOT_EVALUATED)
                      | (0 if same_pocket else POCKET_MISMATCH))
            sample_out[g] = [sim, same, common, union, jac, status]
            centroid_d2[g] = (dist2(centroid[g], centroid_nat[p]) if int(contacts_status[g]) == 0 and int(contacts_status_nat[p]) == 0
                              else np.nan)
        bad = (int(group_ptr[p]), int(group_ptr[p + 1])) != (g0, g1)
        group_out[p] = [g1 - g0, n_fp, n_same, sim_sum, sim_max, n_contact, contact_sum, contact_max,
                        (0 if nat_ok else NATIVE_NOT_EVALUATED) | (BAD_GROUPS if bad else 0)]
    return sample_out, centroid_d2, group_out


def same_floats(a, b):
    """== with NaN positions equal"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))

"""Plain-Python model of cbgx_ligand_fingerprints and cbgx_group_diversity, written from the definition in include/cbgx.h (not from
csrc/diversity.hip): Python ints masked to 64 bits, dicts and loops, no numpy in the arithmetic.  The arrays and their checks are those
of tests/groups_model.py: a graph's atoms are lig_ptr[g] ... lig_ptr[g + 1] (clamped), its bonds bond_ptr[first atom] ... bond_ptr[last
atom + 1] (clamped) of a list in strict (i, j) order with i < j."""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
BITS, WORDS, MAX_ATOMS, MAX_GROUP, COLS, GROUP_COLS = 1024, 32, 256, 1024, 5, 7
TOO_MANY_ATOMS, BAD_BONDS, NO_TYPES, EMPTY = 1, 4, 8, 16
TOO_MANY_GRAPHS, BAD_GROUPS = 1, 4


def mix(x):
    """the splitmix64 finaliser"""
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def fingerprint(z, bonds, ring):
    """one evaluated graph: ``z`` [n] atomic numbers, ``bonds`` [(a, b, type 1 ... 4)] over its own atoms, ``ring`` [n] atom_ring_min ->
    (fp [32] words, mol_hash, n_bits, n_rounds)"""
    n = len(z)
    assert n >= 1
    nbr = [[] for _ in range(n)]
    for a, b, t in bonds:
        nbr[a].append((b, t))
        nbr[b].append((a, t))
    ids = [mix(G + z[a] + 256 * len(nbr[a]) + 65536 * int(any(t == 4 for _, t in nbr[a])) + 131072 * ring[a]) for a in range(n)]
    rounds = max(n, 2)
    fp = [0] * WORDS
    for r in range(rounds + 1):          # ids is id_r here
        if r <= 2:
            for v in ids:
                bit = v & (BITS - 1)
                fp[bit >> 5] |= 1 << (bit & 31)
        if r < rounds:
            ids = [mix(ids[a] + sum(mix(ids[b] ^ ((t * G) & M64)) for b, t in nbr[a])) for a in range(n)]
    h = mix(sum(mix(v ^ G) for v in ids) + n + (len(bonds) << 32))
    return fp, h, sum(bin(w).count("1") for w in fp), rounds


def batch_fingerprints(z, lig_ptr, n_lig, bond_ptr, bond_index, bond_type, atom_ring_min):
    """the entry's arrays -> (fp [B, 32] uint32, mol_hash [B] uint64, graph_out [B, 5] int32)"""
    B, n_bonds = len(lig_ptr) - 1, len(bond_type)
    fp, hashes, out = np.zeros((B, WORDS), np.uint32), np.zeros(B, np.uint64), np.zeros((B, COLS), np.int32)
    clamp = lambda v, lo, hi: min(max(int(v), lo), hi)
    for g in range(B):
        l0 = clamp(lig_ptr[g], 0, n_lig)
        l1 = clamp(lig_ptr[g + 1], l0, n_lig)
        p0, p1 = int(bond_ptr[l0]), int(bond_ptr[l1])
        b0 = clamp(p0, 0, n_bonds)
        b1 = clamp(p1, b0, n_bonds)
        n, m = l1 - l0, b1 - b0
        bad = p0 != b0 or p1 != b1 or any(int(bond_ptr[a]) > int(bond_ptr[a + 1]) for a in range(l0, l1))
        no_types = any(int(atom_ring_min[a]) == 255 for a in range(l0, l1))
        rows = []
        for b in range(b0, b1):
            i, j, t = int(bond_index[0][b]), int(bond_index[1][b]), int(bond_type[b])
            bad = bad or not (l0 <= i < j < l1) or (t != 255 and not 1 <= t <= 4)
            if b > b0:
                bad = bad or not (int(bond_index[0][b - 1]), int(bond_index[1][b - 1])) < (i, j)
            no_types = no_types or t == 255
            rows.append((i - l0, j - l0, t))
        status = (TOO_MANY_ATOMS if n > MAX_ATOMS else 0) | (BAD_BONDS if bad else 0) | (NO_TYPES if no_types else 0) | (EMPTY if n == 0 else 0)
        out[g] = [n, m, -1, -1, status]
        if status == 0:
            words, h, n_bits, rounds = fingerprint([int(v) for v in z[l0:l1]], rows, [int(v) for v in atom_ring_min[l0:l1]])
            fp[g], hashes[g], out[g, 2], out[g, 3] = words, h, n_bits, rounds
    return fp, hashes, out


def as_int(row):
    """a row of fp as one 1024-bit Python int"""
    return sum((int(w) & 0xFFFFFFFF) << (32 * k) for k, w in enumerate(row))


def tanimoto_micro(a, b):
    """two rows of fp (or their ``as_int``) -> the similarity in millionths, rounded half up; 0 if neither has a bit (no row the
    fingerprint kernel writes for an evaluated graph is empty)"""
    a, b = (v if isinstance(v, int) else as_int(v) for v in (a, b))
    inter, uni = bin(a & b).count("1"), bin(a | b).count("1")
    return (inter * 1000000 + uni // 2) // uni if uni else 0


def group_ranges(group_ptr, B):
    """[(g0, g1, clamped?)] of a group_ptr as the kernel reads it"""
    out = []
    for p in range(len(group_ptr) - 1):
        g0 = min(max(int(group_ptr[p]), 0), B)
        g1 = min(max(int(group_ptr[p + 1]), g0), B)
        out.append((g0, g1, g0 != int(group_ptr[p]) or g1 != int(group_ptr[p + 1])))
    return out


def pair_ptr_of(group_ptr, B):
    """what the host computes from group_ptr: n (n - 1) / 2 entries per group, n the clamped size"""
    sizes = [g1 - g0 for g0, g1, _ in group_ranges(group_ptr, B)]
    return np.concatenate([[0], np.cumsum([n * (n - 1) // 2 for n in sizes])]).astype(np.int64)


def group_diversity(fp, mol_hash, status, group_ptr, pair_ptr=None, n_pairs=None):
    """-> (pair_sim [n_pairs] int32, first_same [B], nearest [B], nearest_micro [B] int32, group_out [P, 7] int64).  What no group
    writes stays at the fill value -1: graphs outside every group, and the pairs of a group whose pair range does not fit"""
    B, P = len(status), len(group_ptr) - 1
    pair_ptr = pair_ptr_of(group_ptr, B) if pair_ptr is None else pair_ptr
    n_pairs = int(pair_ptr[P]) if n_pairs is None else n_pairs
    pair_sim = np.full(n_pairs, -1, np.int32)
    first, nearest, micro = (np.full(B, -1, np.int32) for _ in range(3))
    out = np.zeros((P, GROUP_COLS), np.int64)
    for p, (g0, g1, clamped) in enumerate(group_ranges(group_ptr, B)):
        n = g1 - g0
        q0, q1 = int(pair_ptr[p]), int(pair_ptr[p + 1])
        fits = 0 <= q0 and q1 <= n_pairs and q1 - q0 == n * (n - 1) // 2
        st = (BAD_GROUPS if clamped or not fits else 0) | (TOO_MANY_GRAPHS if n > MAX_GROUP else 0)
        if n > MAX_GROUP:
            out[p] = [n, -1, -1, -1, -1, -1, st]
            first[g0:g1] = nearest[g0:g1] = micro[g0:g1] = -1
            if fits:
                pair_sim[q0:q1] = -1
            continue
        ok = [int(status[g]) == 0 for g in range(g0, g1)]
        rows = [as_int(fp[g]) for g in range(g0, g1)]
        n_pair, total, top, k = 0, 0, -1, q0
        best = [(-1, -1)] * n
        for i in range(n):
            for j in range(i + 1, n):
                s = tanimoto_micro(rows[i], rows[j]) if ok[i] and ok[j] else -1
                if fits:
                    pair_sim[k] = s
                k += 1
                if s >= 0:
                    n_pair, total, top = n_pair + 1, total + s, max(top, s)
                    if s > best[i][0]:
                        best[i] = (s, j)
                    if s > best[j][0]:
                        best[j] = (s, i)
        unique = 0
        for i in range(n):
            if not ok[i]:
                continue
            same = min(j for j in range(i + 1) if ok[j] and int(mol_hash[g0 + j]) == int(mol_hash[g0 + i]))
            first[g0 + i], nearest[g0 + i], micro[g0 + i] = same, best[i][1], best[i][0]
            unique += same == i
        out[p] = [n, sum(ok), unique, n_pair, total, top, st]
    return pair_sim, first, nearest, micro, out


def diversity_micro(total, n_pair):
    return 1000000 - (total + n_pair // 2) // n_pair if n_pair else -1

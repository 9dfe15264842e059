// libcbgx -- functional groups of the table-bond graph of a batch of sampled ligands (cbgx_ligand_groups; the definition is in
// include/cbgx.h): what the reference counts with EFGs.mol2frag after RDKit reconstruction (repo/tools/eval_fg_type.py), here a partition
// of the bond list of geometry.hip with the aromatic bonds of aromatic.hip into groups, and an exact isomorphism test of every group
// against the 25 template graphs of geo_tables.h, for a whole batch in ONE launch.
//   shape     one 64-thread workgroup = ONE WAVE per graph, as rings.hip, aromatic.hip and valence.hip.  No protocol with anybody, nothing
//             spins, no atomics on memory.  (The barriers are workgroup barriers of a one-wave workgroup: they order the wave's own LDS
//             traffic for the compiler and cannot wait for anyone.)
//   limits    the checks of ligand_valence_kernel on the two ranges and the list: more than GR_N atoms, a range that is not what the fill
//             kernel writes, an order outside 1..3 or an aromatic byte of 255 is reported in `status` and nothing is built.  Every index
//             into LDS below is a row of a checked bond minus the graph's first row: < GR_N.  There is NO limit on the bonds: everything
//             per bond stays in global memory.
//   marks     lanes over bonds OR the kinds of their bonds into both ends (aromatic, multiple), note where an atom's bonds start in the
//             (sorted) list and set the atom's row of the non-aromatic adjacency bit matrix; lanes over atoms make `acetal partner`; lanes
//             over bonds count those partners per atom and look for triangles: a non-aromatic bond whose ends share a non-aromatic
//             neighbour (the AND of two rows), one of the three an N, O or S (a mask of those atoms).  Lanes over atoms decide membership.
//   groups    the components of the members under the group bonds by min-label propagation with pointer jumping, as valence.hip: all
//             labels of a component end equal to its smallest atom, whatever order the lanes ran in.  Sizes and bond counts per root.
//   tables    the templates are copied from constant memory into LDS first: the matcher reads them at addresses that differ from lane to
//             lane, one read depending on the last.
//   classes   one group per lane (lane l takes the groups l, l + 64, ... in the order of their smallest atoms).  A group of at most 10
//             atoms gets its atoms numbered 0..9 (a byte per atom in LDS; an atom belongs to one group, so no two lanes touch the same
//             byte), its labels packed four bits apiece into one register and its bond types into a [10 x 10][lane] byte matrix in LDS.  A
//             template is tried when atom count, bond count and the histogram of labels agree; the test maps template atom k (each has a
//             bond to an earlier one) to the unused group atoms of its label whose bonds to the images of 0 .. k - 1 have exactly the
//             template's types, backtracking iteratively with the map packed four bits apiece: no recursion, no scratch.
//   output    one pass over the atoms writes atom_group and atom_class, lane 0 the graph's row; every element of the graph's ranges is
//             written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cbgx.h"
#include "geo_tables.h"
#include "kernels.h"

namespace cbgx {

constexpr int GR_THREADS = 64;
constexpr int GR_N = CBGX_GROUPS_MAX_ATOMS;
constexpr int GR_WORDS = GR_N / 32;
constexpr int GR_OTHER = GRP_CLASSES;
static_assert(sizeof(GroupTables) % sizeof(uint32_t) == 0, "the tables are staged word by word");
static_assert(GR_N == 4 * GR_THREADS && GRP_T_ATOMS <= 16 && (GEO_EL << 1) <= 16, "four atoms per lane; a map and the labels in 4-bit fields");

enum : int { GR_AROMATIC = 1, GR_MULTIPLE = 2, GR_TRIANGLE = 4, GR_PARTNER = 8, GR_MEMBER = 16 };

static const GroupTables h_groups = make_group_tables();      // what cbgx_ligand_groups_templates hands out
__constant__ GroupTables d_groups = make_group_tables();      // what the kernel reads: the same initialiser

struct GroupsGraph {                                   // a graph in LDS: 27 KiB
    GroupTables tables;                                // d_groups, staged: the matcher's reads are a chain of dependent loads
    int flags[GR_N], partners[GR_N];                   // GR_* bits; acetal partners among the neighbours
    int comp[GR_N], size[GR_N], bonds[GR_N];           // component label; at a group's smallest atom: its atoms and its group bonds
    int first[GR_N];                                   // where the bonds whose smaller end is the atom start in the graph's list
    unsigned adj[GR_N][GR_WORDS];                      // bit b of row a: a non-aromatic bond a - b
    unsigned nos[GR_WORDS];                            // bit a: atom a is N, O or S
    int fg[GRP_CLASSES + 1];
    uint8_t code[GR_N], root[GR_N], local[GR_N], cls[GR_N];            // element code (GEO_NONE: none); the roots in order; number in its group; class at the root
    uint8_t atom[GRP_T_ATOMS * GR_THREADS];                            // [k][lane] the lane's group: its atoms
    uint8_t type[GRP_T_ATOMS * GRP_T_ATOMS * GR_THREADS];              // [u * 10 + v][lane] ... and the type of its group bond u - v, 0: none
};

__device__ __forceinline__ int gr_sum(int v) {
#pragma unroll
    for (int off = GR_THREADS / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ int gr_max(int v) {
#pragma unroll
    for (int off = GR_THREADS / 2; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}

// element code 0..7 (H C N O F P S Cl) of an atomic number, GEO_NONE: none
__device__ __forceinline__ int gr_code(int z) {
    return z == 1 ? EL_H : z == 6 ? EL_C : z == 7 ? EL_N : z == 8 ? EL_O : z == 9 ? EL_F : z == 15 ? EL_P : z == 16 ? EL_S : z == 17 ? EL_CL : GEO_NONE;
}

__device__ __forceinline__ bool gr_nos(int code) { return code == EL_N || code == EL_O || code == EL_S; }

// is the bond i - j of type t between two members a group bond?
__device__ __forceinline__ bool gr_group_bond(int fi, int fj, int t) {
    if (!(fi & fj & GR_MEMBER)) return false;
    const bool ai = fi & GR_AROMATIC, aj = fj & GR_AROMATIC;
    return t == 4 || (!ai && !aj) || (ai != aj && t == 2);
}

// is the lane's group (n atoms, labels and bond types as staged) isomorphic to template k?  Counts and label histogram already agree
__device__ bool gr_matches(const GroupsGraph& G, int lane, int k, int n, uint64_t labels) {
    const GroupTemplate& T = G.tables.t[k];
    uint64_t map = 0;                 // 4 bits per template atom: its image
    unsigned used = 0;
    int level = 0, c = 0;             // the next candidate image of template atom `level`
    for (;;) {
        const int want = T.label[level];
        for (; c < n; ++c) {
            if (((used >> c) & 1) || (int)((labels >> (4 * c)) & 15) != want) continue;
            bool fits = true;
            for (int j = level - 1; j >= 0 && fits; --j) {      // latest first: the earlier atom it is bonded to is mostly the last one
                const int image = (int)((map >> (4 * j)) & 15);
                fits = G.type[(c * GRP_T_ATOMS + image) * GR_THREADS + lane] == G.tables.adj[k][level][j];
            }
            if (fits) break;
        }
        if (c < n) {
            if (level == n - 1) return true;
            map = (map & ~(15ull << (4 * level))) | ((uint64_t)c << (4 * level));
            used |= 1u << c;
            ++level; c = 0;
        } else {
            if (level == 0) return false;
            --level;
            c = (int)((map >> (4 * level)) & 15);
            used &= ~(1u << c);
            ++c;
        }
    }
}

__global__ __launch_bounds__(GR_THREADS) void ligand_groups_kernel(
    const uint8_t* __restrict__ z_lig, const int32_t* __restrict__ lig_ptr, int n_lig, const int32_t* __restrict__ bond_ptr,
    const int32_t* __restrict__ bond_index, const uint8_t* __restrict__ bond_order, const uint8_t* __restrict__ bond_aromatic, int n_bonds,
    int32_t* __restrict__ atom_group, uint8_t* __restrict__ atom_class, int32_t* __restrict__ graph_out) {
    __shared__ GroupsGraph G;
    const int g = blockIdx.x, lane = threadIdx.x;
    // both ranges clamped to their arrays, as ligand_valence_kernel does
    const int l0 = min(max(lig_ptr[g], 0), n_lig), l1 = min(max(lig_ptr[g + 1], l0), n_lig);
    const int p0 = bond_ptr[l0], p1 = bond_ptr[l1];
    const int b0 = min(max(p0, 0), n_bonds), b1 = min(max(p1, b0), n_bonds);
    const int n = l1 - l0, m = b1 - b0;
    const size_t row_j = (size_t)n_bonds;

    // ---- is this range of the list what the fill kernel writes?  orders 1..3?  did the aromatic report evaluate the graph? ---------------
    bool bad = p0 != b0 || p1 != b1, no_aromatic = false;
    for (int a = l0 + lane; a < l1; a += GR_THREADS) bad = bad || bond_ptr[a] > bond_ptr[a + 1];
    for (int b = b0 + lane; b < b1; b += GR_THREADS) {
        const int i = bond_index[b], j = bond_index[row_j + b], o = bond_order[b];
        bad = bad || !(l0 <= i && i < j && j < l1) || o < 1 || o > 3;
        if (b > b0) {
            const int pi = bond_index[b - 1], pj = bond_index[row_j + b - 1];
            bad = bad || !(pi < i || (pi == i && pj < j));
        }
        no_aromatic = no_aromatic || (bond_aromatic && bond_aromatic[b] == 255);
    }
    const int status = (n > GR_N ? CBGX_GROUPS_TOO_MANY_ATOMS : 0) | (__any(bad) ? CBGX_GROUPS_BAD_BONDS : 0) |
                       (__any(no_aromatic) ? CBGX_GROUPS_NO_AROMATIC : 0);

    int n_groups = 0, n_group_atoms = 0, largest = 0;
    if (status == 0) {
        // the type of bond e of the graph (0 <= e < m)
        auto type_of = [&](int e) { return bond_aromatic && bond_aromatic[b0 + e] == 1 ? 4 : (int)bond_order[b0 + e]; };
        // ---- atoms and the kinds of their bonds ------------------------------------------------------------------------------------------
        for (int a = lane; a < n; a += GR_THREADS) {
            const int code = gr_code(z_lig[l0 + a]);
            G.flags[a] = 0; G.partners[a] = 0; G.comp[a] = a; G.size[a] = 0; G.bonds[a] = 0; G.first[a] = m; G.code[a] = (uint8_t)code;
            G.local[a] = 0; G.cls[a] = GR_OTHER;
#pragma unroll
            for (int w = 0; w < GR_WORDS; ++w) G.adj[a][w] = 0;
        }
        {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(&d_groups);
            uint32_t* dst = reinterpret_cast<uint32_t*>(&G.tables);
            for (int w = lane; w < (int)(sizeof(GroupTables) / sizeof(uint32_t)); w += GR_THREADS) dst[w] = src[w];
        }
        if (lane < GR_WORDS) G.nos[lane] = 0;
        if (lane <= GRP_CLASSES) G.fg[lane] = 0;
        __syncthreads();
        for (int a = lane; a < n; a += GR_THREADS)
            if (gr_nos(G.code[a])) atomicOr(&G.nos[a >> 5], 1u << (a & 31));
        for (int e = lane; e < m; e += GR_THREADS) {
            const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0, t = type_of(e);      // 0 <= i < j < n: checked above
            const int kind = t == 4 ? GR_AROMATIC : t >= 2 ? GR_MULTIPLE : 0;
            if (kind) { atomicOr(&G.flags[i], kind); atomicOr(&G.flags[j], kind); }
            if (t != 4) { atomicOr(&G.adj[i][j >> 5], 1u << (j & 31)); atomicOr(&G.adj[j][i >> 5], 1u << (i & 31)); }
            if (e == 0 || bond_index[b0 + e - 1] - l0 != i) G.first[i] = e;      // the list is sorted by its first row: one lane per atom
        }
        __syncthreads();
        for (int a = lane; a < n; a += GR_THREADS)
            if (gr_nos(G.code[a]) && !(G.flags[a] & (GR_AROMATIC | GR_MULTIPLE))) G.flags[a] |= GR_PARTNER;
        __syncthreads();
        for (int e = lane; e < m; e += GR_THREADS) {
            const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;
            if (G.flags[j] & GR_PARTNER) atomicAdd(&G.partners[i], 1);
            if (G.flags[i] & GR_PARTNER) atomicAdd(&G.partners[j], 1);
            if (type_of(e) == 4) continue;
            bool third = false, third_nos = false;
#pragma unroll
            for (int w = 0; w < GR_WORDS; ++w) {
                const unsigned both = G.adj[i][w] & G.adj[j][w];
                third = third || both != 0; third_nos = third_nos || (both & G.nos[w]) != 0;
            }
            if (third && (third_nos || gr_nos(G.code[i]) || gr_nos(G.code[j]))) { atomicOr(&G.flags[i], GR_TRIANGLE); atomicOr(&G.flags[j], GR_TRIANGLE); }
        }
        __syncthreads();
        for (int a = lane; a < n; a += GR_THREADS) {
            const int code = G.code[a], f = G.flags[a];
            bool member = false;
            if (code != EL_H && code != GEO_NONE) {
                member = (f & GR_AROMATIC) || code != EL_C;
                // a non-aromatic carbon: unsaturated, an acetal carbon (only single bonds here), or on a hetero triangle
                member = member || (f & GR_MULTIPLE) || G.partners[a] >= 2 || (f & GR_TRIANGLE);
            }
            if (member) G.flags[a] = f | GR_MEMBER;
        }
        __syncthreads();
        // ---- groups: components of the members under the group bonds (a sweep carries the smallest atom one bond further) -----------------
        for (int sweep = 0; sweep <= n; ++sweep) {
            bool changed = false;
            for (int e = lane; e < m; e += GR_THREADS) {
                const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;
                if (!gr_group_bond(G.flags[i], G.flags[j], type_of(e))) continue;
                const int ci = G.comp[i], cj = G.comp[j];
                if (ci != cj) { atomicMin(&G.comp[i], cj); atomicMin(&G.comp[j], ci); changed = true; }
            }
            __syncthreads();
            for (int a = lane; a < n; a += GR_THREADS) {
                const int ca = G.comp[a], cc = G.comp[ca];
                if (cc < ca) { atomicMin(&G.comp[a], cc); changed = true; }
            }
            __syncthreads();
            if (!__any(changed)) break;
        }
        for (int a = lane; a < n; a += GR_THREADS)
            if (G.flags[a] & GR_MEMBER) atomicAdd(&G.size[G.comp[a]], 1);
        for (int e = lane; e < m; e += GR_THREADS) {
            const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;
            if (gr_group_bond(G.flags[i], G.flags[j], type_of(e))) atomicAdd(&G.bonds[G.comp[i]], 1);
        }
        // the groups in the order of their smallest atoms
        for (int c = 0; c < GR_N; c += GR_THREADS) {
            const int a = c + lane;
            const bool root = a < n && (G.flags[a] & GR_MEMBER) && G.comp[a] == a;
            const uint64_t roots = __ballot(root);
            if (root) G.root[n_groups + __popcll(roots & ((1ull << lane) - 1))] = (uint8_t)a;
            n_groups += __popcll(roots);
        }
        __syncthreads();

        // ---- one group per lane --------------------------------------------------------------------------------------------------------------
        for (int gidx = lane; gidx < n_groups; gidx += GR_THREADS) {
            const int root = G.root[gidx], size = G.size[root], nb = G.bonds[root];
            n_group_atoms += size; largest = max(largest, size);
            int cls = GR_OTHER;
            if (size <= GRP_T_ATOMS) {
                uint64_t labels = 0, hist = 0;
                for (int a = root, k = 0; k < size; ++a) {             // the group has `size` atoms at or after its smallest: a < n
                    if (!(G.flags[a] & GR_MEMBER) || G.comp[a] != root) continue;
                    const uint64_t label = (uint64_t)((G.code[a] << 1) | (G.flags[a] & GR_AROMATIC));
                    labels |= label << (4 * k); hist += 1ull << (4 * label);
                    G.atom[k * GR_THREADS + lane] = (uint8_t)a; G.local[a] = (uint8_t)k;
                    ++k;
                }
                bool candidate = false;
                for (int k = 0; k < GRP_CLASSES; ++k)
                    candidate = candidate || (G.tables.t[k].n_atoms == size && G.tables.t[k].n_bonds == nb && G.tables.hist[k] == hist);
                if (candidate) {
                    for (int u = 0; u < size * GRP_T_ATOMS; ++u) G.type[u * GR_THREADS + lane] = 0;
                    for (int u = 0; u < size; ++u) {
                        const int a = G.atom[u * GR_THREADS + lane];
                        for (int e = G.first[a]; e < m && bond_index[b0 + e] - l0 == a; ++e) {
                            const int j = bond_index[row_j + b0 + e] - l0, t = type_of(e);
                            if (!gr_group_bond(G.flags[a], G.flags[j], t)) continue;      // (a group bond of a joins a's own group)
                            const int v = G.local[j];
                            G.type[(u * GRP_T_ATOMS + v) * GR_THREADS + lane] = (uint8_t)t;
                            G.type[(v * GRP_T_ATOMS + u) * GR_THREADS + lane] = (uint8_t)t;
                        }
                    }
                    for (int k = 0; k < GRP_CLASSES && cls == GR_OTHER; ++k)
                        if (G.tables.t[k].n_atoms == size && G.tables.t[k].n_bonds == nb && G.tables.hist[k] == hist &&
                            gr_matches(G, lane, k, size, labels))
                            cls = k;
                }
            }
            G.cls[root] = (uint8_t)cls;
            atomicAdd(&G.fg[cls], 1);
        }
        __syncthreads();
        n_group_atoms = gr_sum(n_group_atoms); largest = gr_max(largest);
    }

    // ---- outputs: every element of the graph's rows -------------------------------------------------------------------------------------------
    for (int a = lane; a < n; a += GR_THREADS) {
        int grp = -2, cls = 255;
        if (status == 0) {
            const bool member = G.flags[a] & GR_MEMBER;
            grp = member ? G.comp[a] : -1;
            cls = member ? G.cls[G.comp[a]] : CBGX_GROUPS_NO_GROUP;
        }
        atom_group[(size_t)l0 + a] = grp;
        atom_class[(size_t)l0 + a] = (uint8_t)cls;
    }
    int32_t* o = graph_out + (size_t)CBGX_GROUPS_GRAPH_COLS * g;
    const bool ok = status == 0;
    if (lane <= GRP_CLASSES) o[6 + lane] = ok ? G.fg[lane] : -1;
    if (lane == 0) {
        o[0] = n; o[1] = m;
        o[2] = ok ? n_groups : -1; o[3] = ok ? n_group_atoms : -1; o[4] = ok ? n_groups - G.fg[GR_OTHER] : -1; o[5] = ok ? largest : -1;
        o[CBGX_GROUPS_GRAPH_COLS - 1] = status;
    }
}

hipError_t launch_ligand_groups(const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* bond_ptr,
                                const int32_t* bond_index, const uint8_t* bond_order, const uint8_t* bond_aromatic, int n_bonds,
                                int32_t* atom_group, uint8_t* atom_class, int32_t* graph_out, hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    hipLaunchKernelGGL(ligand_groups_kernel, dim3(n_graphs), dim3(GR_THREADS), 0, s, z_lig, lig_ptr, n_lig, bond_ptr, bond_index,
                       bond_order, bond_aromatic, n_bonds, atom_group, atom_class, graph_out);
    return hipGetLastError();
}

void ligand_groups_templates(uint8_t* n_atoms, uint8_t* n_bonds, uint8_t* labels, uint8_t* bonds) {
    for (int k = 0; k < GRP_CLASSES; ++k) {
        const GroupTemplate& T = h_groups.t[k];
        n_atoms[k] = T.n_atoms; n_bonds[k] = T.n_bonds;
        for (int a = 0; a < GRP_T_ATOMS; ++a) labels[k * GRP_T_ATOMS + a] = T.label[a];
        for (int b = 0; b < GRP_T_BONDS; ++b) {
            uint8_t* row = bonds + (k * GRP_T_BONDS + b) * 3;
            row[0] = T.bond[b].i; row[1] = T.bond[b].j; row[2] = T.bond[b].t;
        }
    }
}

}  // namespace cbgx

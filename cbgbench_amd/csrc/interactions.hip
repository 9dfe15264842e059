// libcbgx -- typed pocket contacts and a score in Vina's functional form for a batch of sampled ligands in their pockets
// (cbgx_pocket_types, cbgx_ligand_interactions; the definition, the constants and the deviations are in include/cbgx.h): what the
// reference gets from `vina_task.run(mode='score_only')` (evaluate_scripts/evaluate_chem_single.py:44-49) and the PLIP contact counts of
// repo/tools/interaction.py, here on this library's own atom typing, from coordinates, elements, the bond list of geometry.hip, the
// hydrogens and Kekule orders of valence.hip and the pocket's residue table.  NOT a reproduction of the Vina program.
//   shape     one 256-thread workgroup per graph in both kernels; nobody waits for anybody but at workgroup barriers, no atomics on memory,
//             integer atomics on LDS only.
//   pocket    cbgx_pocket_types streams the graph's protein atoms in tiles of IA_TILE through LDS: thread k types atom base + k; a carbon
//             walks every tile for a table bond (geometry.hip's distance and `p < b1 + margin`) to an N, O or S.  No size limit.
//   ligand    cbgx_ligand_interactions checks the two ranges and the list as valence.hip does; then, with the graph in LDS,
//             neighbours  lanes over bonds count heavy and hydrogen neighbours and mark hetero neighbours and triple bonds per atom;
//             bridges     fragment labels by min-label propagation (as valence.hip), BFS depths from every fragment's smallest atom by
//                         relaxation (depths only decrease, the fixed point is the BFS depth whatever order lanes ran in), parent = the
//                         smallest neighbour one level up; every bond that is no tree edge walks both ends up to their meeting point and
//                         marks the tree edges it passes: a bond is a bridge iff it is a tree edge nobody marked.
//             pairs       the pocket streamed in the same tiles.  Thread k of a pass serves ligand atom 64 pass + k / 4 in slot k % 4.
//   sum order (part of the interface: a function of the graph's own sizes only)
//             atom_terms[i][t]: slot s adds the pairs with pocket atoms j = s, s + 4, s + 8, ... of the graph (graph-local j, ascending)
//             to a partial p_s that starts at 0.0; the sum is (p_0 + p_1) + (p_2 + p_3).  Pocket atoms that take no part and pairs with
//             r >= 8 add nothing (they are skipped, not added as 0.0).  graph_terms[g][t] = ((0.0 + a_0) + a_1) + ... over the graph's
//             ligand atoms in ascending order, atoms that take no part included as 0.0.
//   distance  geometry.hip's: fp32 coordinates widened to fp64, every product and sum rounded on its own, sqrt correctly rounded;
//             contraction is OFF for this translation unit.  d = (r - R_i) - R_j; q1 = d / 0.5, gauss1 = exp(-(q1 q1)); q2 = (d - 3.0) / 2.0,
//             gauss2 = exp(-(q2 q2)); the arguments of exp are exact functions of r.  A pair with s >= 64 is skipped before the square root
//             (sqrt is monotonic and sqrt(64) = 8); one with s < 64 whose r rounds to 8 is excluded by r < 8.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/cbgx.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "geo_tables.h"      // element codes, make_interaction_tables, geo_dist2

namespace cbgx {

constexpr int IA_THREADS = 256;
constexpr int IA_N = CBGX_INTERACTIONS_MAX_ATOMS;
constexpr int IA_TILE = 256;                   // pocket atoms staged at a time
constexpr int IA_SLOTS = 4;                    // threads per ligand atom
constexpr int IA_PER_PASS = IA_THREADS / IA_SLOTS;
constexpr int IA_TERMS = CBGX_INTERACTIONS_TERMS;
constexpr int IA_FAR = 1 << 20;                // a depth / parent no atom has
constexpr double IA_CUT = 8.0, IA_CUT2 = 64.0;
constexpr int IA_HYD = CBGX_INTERACTIONS_HYDROPHOBIC, IA_DON = CBGX_INTERACTIONS_DONOR, IA_ACC = CBGX_INTERACTIONS_ACCEPTOR;
static_assert(IA_N == IA_THREADS && IA_TILE % IA_SLOTS == 0 && IA_TERMS == 5, "one atom per thread in the atom passes; slots see j mod 4");

__constant__ InteractionTables d_ia = make_interaction_tables();

// element code 0..7 (H C N O F P S Cl) of an atomic number, -1: none
__device__ __forceinline__ int ia_code(int z) {
    return z == 1 ? 0 : z == 6 ? 1 : z == 7 ? 2 : z == 8 ? 3 : z == 9 ? 4 : z == 15 ? 5 : z == 16 ? 6 : z == 17 ? 7 : -1;
}

// does a type byte take part in the pair terms?  (0: H or no element; CBGX_INTERACTIONS_UNTYPED and 255 do not)
__device__ __forceinline__ bool ia_takes_part(int t) { return t > 0 && t < CBGX_INTERACTIONS_UNTYPED && (t & CBGX_INTERACTIONS_ELEMENT_MASK); }

__device__ __forceinline__ int ia_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ---- pocket atom types ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IA_THREADS) void pocket_types_kernel(
    const float* __restrict__ x_rec, const uint8_t* __restrict__ z_rec, const int32_t* __restrict__ rec_ptr, int n_rec,
    const uint8_t* __restrict__ rec_aa, const uint8_t* __restrict__ rec_backbone, uint8_t* __restrict__ rec_type) {
    __shared__ float tx[IA_TILE], ty[IA_TILE], tz[IA_TILE];
    __shared__ uint8_t tk[IA_TILE];              // 1 N, 2 O, 3 S; 0: no partner of a carbon
    const int g = blockIdx.x, k = threadIdx.x;
    const int r0 = min(max(rec_ptr[g], 0), n_rec), r1 = min(max(rec_ptr[g + 1], r0), n_rec);
    const int nr = r1 - r0;
    for (int base = 0; base < nr; base += IA_THREADS) {
        const int q = base + k;
        const bool mine = q < nr;
        int zq = 0;
        double px = 0.0, py = 0.0, pz = 0.0;
        if (mine) {
            const size_t a = (size_t)(r0 + q);
            zq = z_rec[a];
            px = (double)x_rec[3 * a + 0]; py = (double)x_rec[3 * a + 1]; pz = (double)x_rec[3 * a + 2];
        }
        bool hetero = false;
        for (int tb = 0; tb < nr; tb += IA_TILE) {
            __syncthreads();
            int kind = 0;
            if (tb + k < nr) {
                const size_t a = (size_t)(r0 + tb + k);
                tx[k] = x_rec[3 * a + 0]; ty[k] = x_rec[3 * a + 1]; tz[k] = x_rec[3 * a + 2];
                const int zz = z_rec[a];
                kind = zz == 7 ? 1 : zz == 8 ? 2 : zz == 16 ? 3 : 0;
            }
            tk[k] = (uint8_t)kind;
            __syncthreads();
            if (mine && zq == 6 && !hetero) {
                const int cnt = min(IA_TILE, nr - tb);
                for (int j = 0; j < cnt; ++j) {
                    const int kj = tk[j];
                    if (!kj) continue;
                    const double s = geo_dist2(px, py, pz, tx[j], ty[j], tz[j]);
                    if (s >= GEO_FAR2) continue;
                    const double p = 100.0 * __dsqrt_rn(s);
                    if (p < d_ia.c_bond[kj]) hetero = true;
                }
            }
        }
        if (mine) {
            const int aa = rec_aa[r0 + q] < IA_RES ? rec_aa[r0 + q] : IA_RES, bb = rec_backbone[r0 + q] ? 1 : 0;
            int t;
            switch (zq) {
                case 1: t = 0; break;
                case 6: t = EL_C | (hetero ? 0 : IA_HYD); break;
                case 7: t = EL_N | d_ia.n_type[bb][aa]; break;
                case 8: t = EL_O | d_ia.o_type[bb][aa]; break;
                case 16: t = EL_S; break;
                default: t = CBGX_INTERACTIONS_UNTYPED;
            }
            rec_type[(size_t)(r0 + q)] = (uint8_t)t;
        }
    }
}

// ---- ligand types, rotatable bonds, pair terms ---------------------------------------------------------------------------------------------
struct InteractionGraph {                 // a graph in LDS: 24 KiB
    double terms[IA_N][IA_TERMS];
    float x[IA_N], y[IA_N], z[IA_N];
    int frag[IA_N], depth[IA_N], parent[IA_N];
    int heavy[IA_N], hyd[IA_N];           // neighbours that are not H; neighbours that are
    int mark[IA_N];                       // 1: a neighbour neither C nor H, 2: on a triple bond, 4: the tree edge to the parent lies on a cycle
    float tx[IA_TILE], ty[IA_TILE], tz[IA_TILE];
    uint8_t tt[IA_TILE];
    uint8_t zz[IA_N], type[IA_N];
    int count[10];                        // rotatable, donors, acceptors, hydrophobic atoms, pairs, hbond, hydrophobic, close pairs, contact atoms, untyped
};

// is bond (i, j) the tree edge of its deeper end?  child: that end
__device__ __forceinline__ bool ia_tree_edge(const InteractionGraph& G, int i, int j, int& child) {
    if (G.depth[j] == G.depth[i] + 1 && G.parent[j] == i) { child = j; return true; }
    if (G.depth[i] == G.depth[j] + 1 && G.parent[i] == j) { child = i; return true; }
    return false;
}

__global__ __launch_bounds__(IA_THREADS) void ligand_interactions_kernel(
    const float* __restrict__ x_lig, const uint8_t* __restrict__ z_lig, const int32_t* __restrict__ lig_ptr, int n_lig,
    const float* __restrict__ x_rec, const uint8_t* __restrict__ rec_type, const int32_t* __restrict__ rec_ptr, int n_rec,
    const int32_t* __restrict__ bond_ptr, const int32_t* __restrict__ bond_index, const uint8_t* __restrict__ bond_kekule,
    const uint8_t* __restrict__ bond_aromatic, int n_bonds, const uint8_t* __restrict__ implicit_h, const uint8_t* __restrict__ atom_flags,
    const int32_t* __restrict__ valence_status, double* __restrict__ atom_terms, uint8_t* __restrict__ lig_type,
    uint8_t* __restrict__ bond_rotatable, double* __restrict__ graph_terms, int32_t* __restrict__ graph_out) {
    __shared__ InteractionGraph G;
    const int g = blockIdx.x, k = threadIdx.x;
    // every range clamped to its array, as the sibling kernels do
    const int l0 = min(max(lig_ptr[g], 0), n_lig), l1 = min(max(lig_ptr[g + 1], l0), n_lig);
    const int r0 = min(max(rec_ptr[g], 0), n_rec), r1 = min(max(rec_ptr[g + 1], r0), n_rec);
    const int p0 = bond_ptr[l0], p1 = bond_ptr[l1];
    const int b0 = min(max(p0, 0), n_bonds), b1 = min(max(p1, b0), n_bonds);
    const int n = l1 - l0, m = b1 - b0, nr = r1 - r0;
    const size_t row_j = (size_t)n_bonds;
    const bool no_valence = valence_status[g] != 0;

    // ---- is this range of the list what the fill kernel writes?  Kekule orders 1..4 where the valence report evaluated the graph? -----------
    bool bad = p0 != b0 || p1 != b1;
    for (int a = l0 + k; a < l1; a += IA_THREADS) bad = bad || bond_ptr[a] > bond_ptr[a + 1];
    for (int b = b0 + k; b < b1; b += IA_THREADS) {
        const int i = bond_index[b], j = bond_index[row_j + b], o = bond_kekule[b];
        bad = bad || !(l0 <= i && i < j && j < l1) || (!no_valence && (o < 1 || o > 4));
        if (b > b0) {
            const int pi = bond_index[b - 1], pj = bond_index[row_j + b - 1];
            bad = bad || !(pi < i || (pi == i && pj < j));
        }
    }
    const int status = (n > IA_N ? CBGX_INTERACTIONS_TOO_MANY_ATOMS : 0) | (__syncthreads_or(bad) ? CBGX_INTERACTIONS_BAD_BONDS : 0) |
                       (no_valence ? CBGX_INTERACTIONS_NO_VALENCE : 0);

    if (status != 0) {      // counts -1, floats NaN, bytes 255: every element of the graph's ranges
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int a = k; a < n; a += IA_THREADS) {
            lig_type[(size_t)l0 + a] = 255;
            for (int t = 0; t < IA_TERMS; ++t) atom_terms[((size_t)l0 + a) * IA_TERMS + t] = nan;
        }
        for (int e = k; e < m; e += IA_THREADS) bond_rotatable[(size_t)b0 + e] = 255;
        if (k < IA_TERMS) graph_terms[(size_t)g * IA_TERMS + k] = nan;
        if (k == 0) {
            int32_t* o = graph_out + (size_t)CBGX_INTERACTIONS_GRAPH_COLS * g;
            o[0] = n; o[1] = m;
            for (int c = 2; c < CBGX_INTERACTIONS_GRAPH_COLS - 1; ++c) o[c] = -1;
            o[CBGX_INTERACTIONS_GRAPH_COLS - 1] = status;
        }
        return;
    }

    // (from here on n <= IA_N, every bond has l0 <= i < j < l1, and the list is strict: m <= n (n - 1) / 2)
    // ---- atoms and their neighbours ------------------------------------------------------------------------------------------------------------
    if (k < n) {
        const size_t a = (size_t)(l0 + k);
        G.x[k] = x_lig[3 * a + 0]; G.y[k] = x_lig[3 * a + 1]; G.z[k] = x_lig[3 * a + 2];
        G.zz[k] = z_lig[a];
        G.frag[k] = k; G.parent[k] = IA_FAR; G.heavy[k] = 0; G.hyd[k] = 0; G.mark[k] = 0;
    }
    if (k < 10) G.count[k] = 0;
    __syncthreads();
    for (int e = k; e < m; e += IA_THREADS) {
        const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;
        const int zi = G.zz[i], zj = G.zz[j];
        const int triple = bond_kekule[b0 + e] == 3 ? 2 : 0;
        if (zj == 1) atomicAdd(&G.hyd[i], 1); else atomicAdd(&G.heavy[i], 1);
        if (zi == 1) atomicAdd(&G.hyd[j], 1); else atomicAdd(&G.heavy[j], 1);
        const int mi = ((zj != 6 && zj != 1) ? 1 : 0) | triple, mj = ((zi != 6 && zi != 1) ? 1 : 0) | triple;
        if (mi) atomicOr(&G.mark[i], mi);
        if (mj) atomicOr(&G.mark[j], mj);
    }
    // ---- fragments: a sweep carries the smallest atom one bond further, pointer jumping shortens the way: at most n + 1 sweeps ----------------
    for (int sweep = 0; sweep <= n; ++sweep) {
        bool changed = false;
        __syncthreads();
        for (int e = k; e < m; e += IA_THREADS) {
            const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;
            const int fi = ia_load(&G.frag[i]), fj = ia_load(&G.frag[j]);
            if (fi != fj) { atomicMin(&G.frag[i], fj); atomicMin(&G.frag[j], fi); changed = true; }
        }
        __syncthreads();
        if (k < n) {
            const int fa = ia_load(&G.frag[k]), ff = ia_load(&G.frag[fa]);
            if (ff < fa) { atomicMin(&G.frag[k], ff); changed = true; }
        }
        if (!__syncthreads_or(changed)) break;
    }
    // ---- BFS depth from every fragment's smallest atom: relaxation to the fixed point; a sweep settles one more level: at most n sweeps --------
    if (k < n) G.depth[k] = G.frag[k] == k ? 0 : IA_FAR;
    for (int sweep = 0; sweep <= n; ++sweep) {
        bool changed = false;
        __syncthreads();
        for (int e = k; e < m; e += IA_THREADS) {
            const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;
            const int di = ia_load(&G.depth[i]), dj = ia_load(&G.depth[j]);
            if (di + 1 < dj) { atomicMin(&G.depth[j], di + 1); changed = true; }
            if (dj + 1 < di) { atomicMin(&G.depth[i], dj + 1); changed = true; }
        }
        if (!__syncthreads_or(changed)) break;
    }
    for (int e = k; e < m; e += IA_THREADS) {
        const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;
        if (G.depth[j] == G.depth[i] + 1) atomicMin(&G.parent[j], i);
        if (G.depth[i] == G.depth[j] + 1) atomicMin(&G.parent[i], j);
    }
    __syncthreads();
    // ---- every bond outside the tree closes a cycle with the two ways up to where they meet (depths fall by one per step: < 2 n steps) ---------
    for (int e = k; e < m; e += IA_THREADS) {
        int u = bond_index[b0 + e] - l0, v = bond_index[row_j + b0 + e] - l0, child;
        if (ia_tree_edge(G, u, v, child)) continue;
        for (int step = 0; u != v && step < 2 * IA_N; ++step) {
            if (G.depth[u] >= G.depth[v]) { atomicOr(&G.mark[u], 4); u = G.parent[u]; }
            else { atomicOr(&G.mark[v], 4); v = G.parent[v]; }
            if (u < 0 || u >= n || v < 0 || v >= n) break;      // (cannot happen: both ends hang under one root)
        }
    }
    __syncthreads();
    int n_rot = 0;
    for (int e = k; e < m; e += IA_THREADS) {
        const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;
        int child = 0;
        const bool bridge = ia_tree_edge(G, i, j, child) && !(G.mark[child] & 4);
        const bool aromatic = bond_aromatic && bond_aromatic[b0 + e] == 1;
        const bool rot = bridge && bond_kekule[b0 + e] == 1 && !aromatic && G.heavy[i] >= 2 && G.heavy[j] >= 2 && !(G.mark[i] & 2) &&
                         !(G.mark[j] & 2);
        bond_rotatable[(size_t)b0 + e] = (uint8_t)rot;
        n_rot += rot;
    }
    if (n_rot) atomicAdd(&G.count[0], n_rot);
    // ---- ligand atom types ---------------------------------------------------------------------------------------------------------------------
    if (k < n) {
        const size_t a = (size_t)(l0 + k);
        const int code = ia_code(G.zz[k]);
        const int h = (int)implicit_h[a] + G.hyd[k];
        int t = 0;
        switch (code) {
            case EL_C: t = EL_C | ((G.mark[k] & 1) ? 0 : IA_HYD); break;
            case EL_F: case EL_CL: t = code | IA_HYD; break;
            case EL_P: case EL_S: t = code; break;
            case EL_O: t = EL_O | IA_ACC | (h > 0 ? IA_DON : 0); break;
            case EL_N: t = EL_N | (h > 0 ? IA_DON : 0) |
                           ((h == 0 && G.heavy[k] <= 2 && !(atom_flags[a] & CBGX_VALENCE_EXCEEDED)) ? IA_ACC : 0); break;
            default: t = 0;
        }
        G.type[k] = (uint8_t)t;
        lig_type[a] = (uint8_t)t;
        if (t & IA_DON) atomicAdd(&G.count[1], 1);
        if (t & IA_ACC) atomicAdd(&G.count[2], 1);
        if (t & IA_HYD) atomicAdd(&G.count[3], 1);
    }
    __syncthreads();

    // ---- pair terms: IA_PER_PASS ligand atoms per pass, IA_SLOTS threads each; the pocket in tiles ------------------------------------------
    const int slot = k % IA_SLOTS;
    int untyped = 0;
    for (int pass = 0; pass * IA_PER_PASS < n; ++pass) {
        const int i = pass * IA_PER_PASS + k / IA_SLOTS;
        const int ti = i < n ? G.type[i] : 0;
        const bool active = ia_takes_part(ti);
        double xi = 0.0, yi = 0.0, zi = 0.0, ri = 0.0;
        if (active) { xi = (double)G.x[i]; yi = (double)G.y[i]; zi = (double)G.z[i]; ri = d_ia.radius[ti & CBGX_INTERACTIONS_ELEMENT_MASK]; }
        double acc[IA_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
        int n_pairs = 0, n_hb = 0, n_hp = 0, n_close = 0, contact = 0;
        for (int tb = 0; tb < nr; tb += IA_TILE) {
            __syncthreads();
            if (tb + k < nr) {
                const size_t a = (size_t)(r0 + tb + k);
                G.tx[k] = x_rec[3 * a + 0]; G.ty[k] = x_rec[3 * a + 1]; G.tz[k] = x_rec[3 * a + 2];
                const int tj = rec_type[a];
                G.tt[k] = (uint8_t)tj;
                if (pass == 0) untyped += tj == CBGX_INTERACTIONS_UNTYPED;
            }
            __syncthreads();
            if (!active) continue;
            const int cnt = min(IA_TILE, nr - tb);
            for (int j = slot; j < cnt; j += IA_SLOTS) {
                const int tj = G.tt[j];
                if (!ia_takes_part(tj)) continue;
                const double s = geo_dist2(xi, yi, zi, G.tx[j], G.ty[j], G.tz[j]);
                if (s >= IA_CUT2) continue;
                const double r = __dsqrt_rn(s);
                if (!(r < IA_CUT)) continue;
                const double d = (r - ri) - d_ia.radius[tj & CBGX_INTERACTIONS_ELEMENT_MASK];
                const double q1 = d / 0.5, q2 = (d - 3.0) / 2.0;
                acc[0] += exp(-(q1 * q1));
                acc[1] += exp(-(q2 * q2));
                if (d < 0.0) acc[2] += d * d;
                const bool pair_hb = ((ti & IA_DON) && (tj & IA_ACC)) || ((ti & IA_ACC) && (tj & IA_DON));
                ++n_pairs;
                if ((ti & IA_HYD) && (tj & IA_HYD) && d < 1.5) { acc[3] += d < 0.5 ? 1.0 : 1.5 - d; ++n_hp; }
                if (pair_hb && d < 0.0) { acc[4] += d < -0.7 ? 1.0 : (-d) / 0.7; ++n_hb; }
                n_close += d < 0.0 && !pair_hb;
                contact |= d < 0.5;
            }
        }
        // (p_0 + p_1) + (p_2 + p_3): addition commutes, so the four slots hold the same bits
#pragma unroll
        for (int t = 0; t < IA_TERMS; ++t) {
            acc[t] += __shfl_xor(acc[t], 1);
            acc[t] += __shfl_xor(acc[t], 2);
        }
        contact |= __shfl_xor(contact, 1);
        contact |= __shfl_xor(contact, 2);
        if (i < n && slot == 0) {
#pragma unroll
            for (int t = 0; t < IA_TERMS; ++t) {
                G.terms[i][t] = acc[t];
                atom_terms[((size_t)l0 + i) * IA_TERMS + t] = acc[t];
            }
            if (contact) atomicAdd(&G.count[8], 1);
        }
        if (n_pairs) {
            atomicAdd(&G.count[4], n_pairs);
            if (n_hb) atomicAdd(&G.count[5], n_hb);
            if (n_hp) atomicAdd(&G.count[6], n_hp);
            if (n_close) atomicAdd(&G.count[7], n_close);
        }
    }
    if (n == 0)      // no pass ran: the pocket's untyped atoms are still counted
        for (int j = k; j < nr; j += IA_THREADS) untyped += rec_type[(size_t)(r0 + j)] == CBGX_INTERACTIONS_UNTYPED;
    if (untyped) atomicAdd(&G.count[9], untyped);
    __syncthreads();
    if (k < IA_TERMS) {
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += G.terms[i][k];
        graph_terms[(size_t)g * IA_TERMS + k] = sum;
    }
    if (k == 0) {
        int32_t* o = graph_out + (size_t)CBGX_INTERACTIONS_GRAPH_COLS * g;
        o[0] = n; o[1] = m;
        for (int c = 0; c < 10; ++c) o[2 + c] = G.count[c];
        o[12] = 0;
    }
}

hipError_t launch_pocket_types(const float* x_rec, const uint8_t* z_rec, const int32_t* rec_ptr, int n_rec, int n_graphs,
                               const uint8_t* rec_aa, const uint8_t* rec_backbone, uint8_t* rec_type, hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    hipLaunchKernelGGL(pocket_types_kernel, dim3(n_graphs), dim3(IA_THREADS), 0, s, x_rec, z_rec, rec_ptr, n_rec, rec_aa, rec_backbone,
                       rec_type);
    return hipGetLastError();
}

hipError_t launch_ligand_interactions(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, const float* x_rec,
                                      const uint8_t* rec_type, const int32_t* rec_ptr, int n_rec, int n_graphs, const int32_t* bond_ptr,
                                      const int32_t* bond_index, const uint8_t* bond_kekule, const uint8_t* bond_aromatic, int n_bonds,
                                      const uint8_t* implicit_h, const uint8_t* atom_flags, const int32_t* valence_status,
                                      double* atom_terms, uint8_t* lig_type, uint8_t* bond_rotatable, double* graph_terms,
                                      int32_t* graph_out, hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    hipLaunchKernelGGL(ligand_interactions_kernel, dim3(n_graphs), dim3(IA_THREADS), 0, s, x_lig, z_lig, lig_ptr, n_lig, x_rec, rec_type,
                       rec_ptr, n_rec, bond_ptr, bond_index, bond_kekule, bond_aromatic, n_bonds, implicit_h, atom_flags, valence_status,
                       atom_terms, lig_type, bond_rotatable, graph_terms, graph_out);
    return hipGetLastError();
}

}  // namespace cbgx

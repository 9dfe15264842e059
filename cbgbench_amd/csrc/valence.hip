// libcbgx -- Kekule bond orders, implicit hydrogens and valence checks of the table-bond graph of a batch of sampled ligands
// (cbgx_ligand_valence; the definition is in include/cbgx.h): what RDKit's kekulisation and valence check make of the molecule the
// reference's reconstruct_mol (repo/tools/rdkit_utils.py:522-590) builds, here on the bond list of geometry.hip and the aromatic bonds of
// aromatic.hip, for a whole batch in ONE launch.
//   shape     one 64-thread workgroup = ONE WAVE per graph, as rings.hip and aromatic.hip.  No protocol with anybody, nothing spins, no
//             atomics on memory.  (The barriers are workgroup barriers of a one-wave workgroup: they order the wave's own LDS traffic for
//             the compiler and cannot wait for anyone.)
//   limits    the checks of ligand_aromatic_kernel on the two ranges and the list, plus bond_order in 1..3 and bond_aromatic != 255:
//             more than VL_N atoms or a range that is not what the fill kernel writes is reported in `status` and nothing is built.
//             Every index into LDS below is a row of a checked bond minus the graph's first row: < VL_N.  There is NO limit on the bonds:
//             a strict list over 256 atoms holds at most 32 640, and everything per bond stays in global memory but one bit (in_m).
//   atoms     lanes over bonds add k (aromatic bonds) and s (orders of the others) per atom with integer LDS atomics; lanes over atoms
//             make f, candidate and must.
//   labels    the components of all bonds (fragments) and of the aromatic bonds (systems) by min-label propagation with pointer jumping:
//             label[a] <= a is always an atom of a's component, a sweep lowers both ends of a bond to the smaller label, and the sweeps end
//             when one changes nothing: then all labels of a component are equal, and equal to its smallest atom, whatever order the
//             lanes ran in.
//   search    one system per lane (lane l takes the systems l, l + 64 in the order of their smallest atoms; at most 128).  The lane reads
//             the bonds between its first and its last aromatic bond, keeps the eligible ones as pairs of compact atom numbers
//             0..63 ([p][lane] bytes in LDS; bit 6: the atom's last eligible bond) with their position in the list, and runs the search of
//             the header iteratively: the matched atoms and the included bonds are 64-bit masks, a cleared bit of `inc` below p means
//             "excluded at that level", so that the walk back up needs no stack.  No recursion, no scratch.  The compact numbers are kept
//             per atom in LDS; an atom belongs to one system, so no two lanes touch the same byte.
//   output    bonds of the chosen sets are marked in a bit map (LDS, atomicOr); one pass over the bonds writes bond_kekule and adds v per
//             atom, one pass over the atoms writes implicit_h and the flags; every element of the graph's ranges is written.
//   cost      a launch lasts as long as its slowest lane's search.  A search step is two LDS bytes and some 150 instructions of a one-lane
//             wave, most of them branches on the lane's own state: 0.65 - 0.9 us per step measured, so a system
//             that uses the whole budget of 65 536 steps holds its launch for tens of milliseconds; a drug-sized system takes tens of
//             steps.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cbgx.h"
#include "kernels.h"

namespace cbgx {

constexpr int VL_THREADS = 64;
constexpr int VL_N = CBGX_VALENCE_MAX_ATOMS;
constexpr int VL_E = CBGX_VALENCE_MAX_ELIGIBLE;          // eligible bonds of a system, and atoms in them
constexpr int VL_MAX_BONDS = VL_N * (VL_N - 1) / 2;      // of a strict list over VL_N atoms
constexpr int VL_SYS = VL_N / 2;                         // a system has at least two atoms
static_assert(VL_N == 4 * VL_THREADS && VL_E == 64 && VL_MAX_BONDS < 65536, "four atoms per lane; 64-bit masks; 16-bit bond positions");

struct ValenceGraph {                 // a graph in LDS: 30 KiB
    int k[VL_N], s[VL_N], v[VL_N];    // aromatic bonds, order sum of the others, valence
    int frag[VL_N], sys[VL_N];        // component labels: all bonds, aromatic bonds
    int sys_last[VL_N], sys_lo[VL_N], sys_hi[VL_N];       // at a system's smallest atom: its largest atom, its first and last bond
    unsigned in_m[(VL_MAX_BONDS + 31) / 32];              // bit e: bond e of the graph is in a chosen set M
    uint16_t el_bond[VL_E * VL_THREADS];                  // [p][lane] the eligible bond's position in the graph's list
    uint8_t el_i[VL_E * VL_THREADS], el_j[VL_E * VL_THREADS];   // [p][lane] compact ends; bit 6: last(end) == p
    uint8_t z[VL_N], role[VL_N], cid[VL_N], failed[VL_N];       // role: 1 candidate, 2 must; failed: at the smallest atom
    uint8_t sys_root[VL_SYS];
};

__device__ __forceinline__ int vl_sum(int v) {
#pragma unroll
    for (int off = VL_THREADS / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ int vl_max(int v) {
#pragma unroll
    for (int off = VL_THREADS / 2; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}

// element code 0..7 (H C N O F P S Cl) of an atomic number, -1: none
__device__ __forceinline__ int vl_code(int z) {
    return z == 1 ? 0 : z == 6 ? 1 : z == 7 ? 2 : z == 8 ? 3 : z == 9 ? 4 : z == 15 ? 5 : z == 16 ? 6 : z == 17 ? 7 : -1;
}

// the smallest entry of the element's valence table that is >= v; -1: none (v0 is vl_valence(code, 0))
__device__ __forceinline__ int vl_valence(int code, int v) {
    switch (code) {
        case 0: case 4: case 7: return v <= 1 ? 1 : -1;
        case 1: return v <= 4 ? 4 : -1;
        case 2: return v <= 3 ? 3 : -1;
        case 3: return v <= 2 ? 2 : -1;
        case 5: return v <= 3 ? 3 : v <= 5 ? 5 : -1;
        case 6: return v <= 2 ? 2 : v <= 4 ? 4 : v <= 6 ? 6 : -1;
    }
    return -1;
}

// the ends of eligible bond p that an exclusion leaves without a partner: unmatched and last == p.  nd: how many; returns whether one is a
// must atom (the exclusion is then not taken)
__device__ __forceinline__ bool vl_dead(int bi, int bj, uint64_t matched, uint64_t must, int& nd) {
    const int i = bi & 63, j = bj & 63;
    const bool di = (bi & 64) && !((matched >> i) & 1), dj = (bj & 64) && !((matched >> j) & 1);
    nd = (int)di + (int)dj;
    return (di && ((must >> i) & 1)) || (dj && ((must >> j) & 1));
}

__global__ __launch_bounds__(VL_THREADS) void ligand_valence_kernel(
    const uint8_t* __restrict__ z_lig, const int32_t* __restrict__ lig_ptr, int n_lig, const int32_t* __restrict__ bond_ptr,
    const int32_t* __restrict__ bond_index, const uint8_t* __restrict__ bond_order, const uint8_t* __restrict__ bond_aromatic, int n_bonds,
    int max_steps, uint8_t* __restrict__ implicit_h, uint8_t* __restrict__ atom_flags, uint8_t* __restrict__ bond_kekule,
    int32_t* __restrict__ graph_out) {
    __shared__ ValenceGraph G;
    const int g = blockIdx.x, lane = threadIdx.x;
    // both ranges clamped to their arrays, as ligand_aromatic_kernel does
    const int l0 = min(max(lig_ptr[g], 0), n_lig), l1 = min(max(lig_ptr[g + 1], l0), n_lig);
    const int p0 = bond_ptr[l0], p1 = bond_ptr[l1];
    const int b0 = min(max(p0, 0), n_bonds), b1 = min(max(p1, b0), n_bonds);
    const int n = l1 - l0, m = b1 - b0;
    const size_t row_j = (size_t)n_bonds;

    // ---- is this range of the list what the fill kernel writes?  orders 1..3?  did the aromatic report evaluate the graph? ---------------
    bool bad = p0 != b0 || p1 != b1, no_aromatic = false;
    for (int a = l0 + lane; a < l1; a += VL_THREADS) bad = bad || bond_ptr[a] > bond_ptr[a + 1];
    for (int b = b0 + lane; b < b1; b += VL_THREADS) {
        const int i = bond_index[b], j = bond_index[row_j + b], o = bond_order[b];
        bad = bad || !(l0 <= i && i < j && j < l1) || o < 1 || o > 3;
        if (b > b0) {
            const int pi = bond_index[b - 1], pj = bond_index[row_j + b - 1];
            bad = bad || !(pi < i || (pi == i && pj < j));
        }
        no_aromatic = no_aromatic || (bond_aromatic && bond_aromatic[b] == 255);
    }
    int status = (n > VL_N ? CBGX_VALENCE_TOO_MANY_ATOMS : 0) | (__any(bad) ? CBGX_VALENCE_BAD_BONDS : 0) |
                 (__any(no_aromatic) ? CBGX_VALENCE_NO_AROMATIC : 0);

    int n_systems = 0, n_failed = 0, n_double = 0, steps_max = 0;
    if (status == 0) {
        // (a strict list inside the graph's rows: m <= n (n - 1) / 2 <= VL_MAX_BONDS)
        // ---- atoms: k, s ---------------------------------------------------------------------------------------------------------------------
        for (int a = lane; a < n; a += VL_THREADS) {
            G.k[a] = 0; G.s[a] = 0; G.v[a] = 0; G.frag[a] = a; G.sys[a] = a; G.sys_last[a] = 0; G.sys_lo[a] = VL_MAX_BONDS; G.sys_hi[a] = -1; G.z[a] = z_lig[l0 + a]; G.cid[a] = 255;
            G.failed[a] = 0;
        }
        for (int w = lane; w < (m + 31) / 32; w += VL_THREADS) G.in_m[w] = 0;
        __syncthreads();
        for (int e = lane; e < m; e += VL_THREADS) {
            const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;      // 0 <= i < j < n: checked above
            if (bond_aromatic && bond_aromatic[b0 + e] == 1) { atomicAdd(&G.k[i], 1); atomicAdd(&G.k[j], 1); }
            else { const int o = bond_order[b0 + e]; atomicAdd(&G.s[i], o); atomicAdd(&G.s[j], o); }
        }
        __syncthreads();
        for (int a = lane; a < n; a += VL_THREADS) {
            const int zz = G.z[a];
            const int f = vl_valence(vl_code(zz), 0) - G.s[a] - G.k[a];
            const bool cand = G.k[a] > 0 && (zz == 6 || zz == 7) && f >= 1;
            G.role[a] = cand ? (zz == 6 ? 3 : 1) : 0;
        }
        // ---- labels: fragments and aromatic systems (a sweep carries the smallest atom one bond further: at most n + 1 sweeps) -----------------------------
        for (int sweep = 0; sweep <= n; ++sweep) {
            bool changed = false;
            for (int e = lane; e < m; e += VL_THREADS) {
                const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;
                const int fi = G.frag[i], fj = G.frag[j];
                if (fi != fj) { atomicMin(&G.frag[i], fj); atomicMin(&G.frag[j], fi); changed = true; }
                if (bond_aromatic && bond_aromatic[b0 + e] == 1) {
                    const int si = G.sys[i], sj = G.sys[j];
                    if (si != sj) { atomicMin(&G.sys[i], sj); atomicMin(&G.sys[j], si); changed = true; }
                }
            }
            __syncthreads();
            for (int a = lane; a < n; a += VL_THREADS) {
                const int fa = G.frag[a], ff = G.frag[fa], sa = G.sys[a], ss = G.sys[sa];
                if (ff < fa) { atomicMin(&G.frag[a], ff); changed = true; }
                if (ss < sa) { atomicMin(&G.sys[a], ss); changed = true; }
            }
            __syncthreads();
            if (!__any(changed)) break;
        }
        // ---- the systems in the order of their smallest atoms; the largest atom of each --------------------------------------------------------
        for (int a = lane; a < n; a += VL_THREADS)
            if (G.k[a] > 0) atomicMax(&G.sys_last[G.sys[a]], a);
        for (int e = lane; e < m; e += VL_THREADS) {
            if (!bond_aromatic || bond_aromatic[b0 + e] != 1) continue;
            const int root = G.sys[bond_index[b0 + e] - l0];
            atomicMin(&G.sys_lo[root], e); atomicMax(&G.sys_hi[root], e);
        }
        for (int c = 0; c < VL_N; c += VL_THREADS) {
            const int a = c + lane;
            const bool root = a < n && G.k[a] > 0 && G.sys[a] == a;
            const uint64_t roots = __ballot(root);
            if (root) G.sys_root[n_systems + __popcll(roots & ((1ull << lane) - 1))] = (uint8_t)a;
            n_systems += __popcll(roots);
        }
        __syncthreads();

        // ---- one system per lane -----------------------------------------------------------------------------------------------------------
        bool limit = false;
        for (int sidx = lane; sidx < n_systems; sidx += VL_THREADS) {
            const int root = G.sys_root[sidx], top = G.sys_last[root];
            const int e0 = G.sys_lo[root], e1 = G.sys_hi[root] + 1;                           // positions of its aromatic bonds: in [0, m]
            int m_el = 0, nc = 0;
            bool over = false;
            for (int e = e0; e < e1 && !over; ++e) {
                if (bond_aromatic[b0 + e] != 1) continue;
                const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;
                if (G.sys[i] != root || !(G.role[i] & 1) || !(G.role[j] & 1)) continue;
                if (m_el == VL_E) { over = true; break; }
                if (G.cid[i] == 255) { if (nc == VL_E) { over = true; break; } G.cid[i] = (uint8_t)nc++; }
                if (G.cid[j] == 255) { if (nc == VL_E) { over = true; break; } G.cid[j] = (uint8_t)nc++; }
                G.el_i[m_el * VL_THREADS + lane] = G.cid[i]; G.el_j[m_el * VL_THREADS + lane] = G.cid[j];
                G.el_bond[m_el * VL_THREADS + lane] = (uint16_t)e;
                ++m_el;
            }
            if (over) { limit = true; continue; }
            uint64_t must = 0;
            bool uncovered = false;
            for (int a = root; a <= top; ++a) {
                if (G.sys[a] != root || !(G.role[a] & 2)) continue;
                if (G.cid[a] == 255) uncovered = true; else must |= 1ull << G.cid[a];
            }
            if (uncovered) { G.failed[root] = 1; ++n_failed; steps_max = max(steps_max, 1); continue; }
            uint64_t seen = 0;
            for (int p = m_el - 1; p >= 0; --p) {
                const int i = G.el_i[p * VL_THREADS + lane], j = G.el_j[p * VL_THREADS + lane];
                if (!((seen >> i) & 1)) { seen |= 1ull << i; G.el_i[p * VL_THREADS + lane] = (uint8_t)(i | 64); }
                if (!((seen >> j) & 1)) { seen |= 1ull << j; G.el_j[p * VL_THREADS + lane] = (uint8_t)(j | 64); }
            }
            // node(p, M, dead) of the header, iteratively: `down` enters node p, !down returns from it to level p - 1
            int p = 0, size = 0, dead = 0, best = -1, steps = 0, nd;
            uint64_t inc = 0, matched = 0, best_inc = 0;
            bool down = true, out_of_steps = false;
            for (;;) {
                if (down) {
                    if (steps == max_steps) { out_of_steps = true; break; }
                    ++steps;
                    if (p == m_el) { if (size > best) { best = size; best_inc = inc; } down = false; continue; }
                    if (best >= 0 && size + ((nc - 2 * size - dead) >> 1) <= best) { down = false; continue; }
                    const int bi = G.el_i[p * VL_THREADS + lane], bj = G.el_j[p * VL_THREADS + lane];
                    const uint64_t ends = (1ull << (bi & 63)) | (1ull << (bj & 63));
                    if (!(matched & ends)) { inc |= 1ull << p; matched |= ends; ++size; ++p; continue; }
                    if (!vl_dead(bi, bj, matched, must, nd)) { dead += nd; ++p; continue; }
                    down = false;
                } else {
                    if (p == 0) break;
                    --p;
                    const int bi = G.el_i[p * VL_THREADS + lane], bj = G.el_j[p * VL_THREADS + lane];
                    if ((inc >> p) & 1) {
                        inc &= ~(1ull << p); matched &= ~((1ull << (bi & 63)) | (1ull << (bj & 63))); --size;
                        if (!vl_dead(bi, bj, matched, must, nd)) { dead += nd; ++p; down = true; }
                    } else {
                        vl_dead(bi, bj, matched, must, nd);
                        dead -= nd;
                    }
                }
            }
            if (out_of_steps) { limit = true; continue; }
            steps_max = max(steps_max, steps);
            if (best < 0) { G.failed[root] = 1; ++n_failed; continue; }
            n_double += best;
            for (int q = 0; q < m_el; ++q)
                if ((best_inc >> q) & 1) { const int e = G.el_bond[q * VL_THREADS + lane]; atomicOr(&G.in_m[e >> 5], 1u << (e & 31)); }
        }
        __syncthreads();
        if (__any(limit)) status = CBGX_VALENCE_SEARCH_LIMIT;
        n_failed = vl_sum(n_failed); n_double = vl_sum(n_double); steps_max = vl_max(steps_max);
    }

    // ---- outputs: every element of the graph's rows -------------------------------------------------------------------------------------------
    for (int e = lane; e < m; e += VL_THREADS) {
        int kek = 255;
        if (status == 0) {
            const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;
            int val;
            if (bond_aromatic && bond_aromatic[b0 + e] == 1) {
                const bool failed = G.failed[G.sys[i]] != 0;
                kek = failed ? 4 : ((G.in_m[e >> 5] >> (e & 31)) & 1) ? 2 : 1;
                val = failed ? 1 : kek;
            } else {
                kek = val = bond_order[b0 + e];
            }
            atomicAdd(&G.v[i], val); atomicAdd(&G.v[j], val);
        }
        bond_kekule[(size_t)b0 + e] = (uint8_t)kek;
    }
    __syncthreads();
    int n_fragments = 0, n_h = 0, n_exceeded = 0, n_unknown = 0, n_nhoh = 0, n_no = 0, el[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int a = lane; a < n; a += VL_THREADS) {
        int h = 255, fl = 255;
        if (status == 0) {
            const int zz = G.z[a], code = vl_code(zz), on_system = G.k[a] > 0;
            const int target = code < 0 ? -1 : vl_valence(code, G.v[a]);
            const bool exceeded = code >= 0 && target < 0;
            h = target < 0 ? 0 : target - G.v[a];
            fl = (exceeded ? CBGX_VALENCE_EXCEEDED : 0) | (on_system && G.failed[G.sys[a]] ? CBGX_VALENCE_ON_FAILED_SYSTEM : 0) |
                 (code < 0 ? CBGX_VALENCE_UNKNOWN_ELEMENT : 0) | (on_system ? CBGX_VALENCE_ON_AROMATIC_SYSTEM : 0);
            n_fragments += G.frag[a] == a; n_h += h; n_exceeded += exceeded; n_unknown += code < 0;
            n_nhoh += (zz == 7 || zz == 8) && h >= 1; n_no += zz == 7 || zz == 8;
#pragma unroll
            for (int c = 0; c < 8; ++c) el[c] += code == c;
        }
        implicit_h[(size_t)l0 + a] = (uint8_t)h;
        atom_flags[(size_t)l0 + a] = (uint8_t)fl;
    }
    n_fragments = vl_sum(n_fragments); n_h = vl_sum(n_h); n_exceeded = vl_sum(n_exceeded); n_unknown = vl_sum(n_unknown);
    n_nhoh = vl_sum(n_nhoh); n_no = vl_sum(n_no);
#pragma unroll
    for (int c = 0; c < 8; ++c) el[c] = vl_sum(el[c]);
    if (lane == 0) {
        int32_t* o = graph_out + (size_t)CBGX_VALENCE_GRAPH_COLS * g;
        const bool ok = status == 0;
        o[0] = n; o[1] = m;
        o[2] = ok ? n_fragments : -1; o[3] = ok ? n_systems : -1; o[4] = ok ? n_failed : -1; o[5] = ok ? n_double : -1;
        o[6] = ok ? n_h : -1; o[7] = ok ? n_exceeded : -1; o[8] = ok ? n_unknown : -1; o[9] = ok ? n_nhoh : -1; o[10] = ok ? n_no : -1;
#pragma unroll
        for (int c = 0; c < 8; ++c) o[11 + c] = ok ? el[c] : -1;
        o[19] = ok ? (int)(n > 0 && n_exceeded == 0 && n_unknown == 0 && n_failed == 0) : -1;
        o[20] = ok ? steps_max : -1;
        o[21] = status;
    }
}

hipError_t launch_ligand_valence(const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* bond_ptr,
                                 const int32_t* bond_index, const uint8_t* bond_order, const uint8_t* bond_aromatic, int n_bonds,
                                 int max_steps, uint8_t* implicit_h, uint8_t* atom_flags, uint8_t* bond_kekule, int32_t* graph_out,
                                 hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    hipLaunchKernelGGL(ligand_valence_kernel, dim3(n_graphs), dim3(VL_THREADS), 0, s, z_lig, lig_ptr, n_lig, bond_ptr, bond_index,
                       bond_order, bond_aromatic, n_bonds, max_steps, implicit_h, atom_flags, bond_kekule, graph_out);
    return hipGetLastError();
}

}  // namespace cbgx

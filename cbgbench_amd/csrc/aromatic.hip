// libcbgx -- aromatic atoms and bonds of the table-bond graph of a batch of sampled ligands (cbgx_ligand_aromatic; the definition is in
// include/cbgx.h): what the reference's reconstruct_mol (repo/tools/rdkit_utils.py:522-590; fixup :380-389, the ring loop :552-572) makes
// of the model's per-atom aromatic flags, here as a least fixed point over the chordless 5- and 6-cycles of the bond list of geometry.hip,
// for a whole batch in ONE launch.
//   shape     one 64-thread workgroup = ONE WAVE per graph, as rings.hip: a thousand graphs of 10 - 45 atoms, more graphs than SIMDs.  No
//             protocol with anybody, nothing spins, no atomics on memory.  (The barriers are workgroup barriers of a one-wave workgroup:
//             they order the wave's own LDS traffic for the compiler and cannot wait for anyone.)
//   limits    the checks of ligand_rings_kernel, word for word: more than AR_N atoms, AR_C or more bonds beyond the atoms, or a range of
//             the list that is not what the fill kernel writes, is reported in `status` and nothing is built.  Every index into LDS below
//             is a row of a checked bond minus the graph's first row: < AR_N.  A graph whose atom_ring_min holds 255 was not evaluated by
//             the ring report and is not evaluated here (NO_RINGS).
//   staging   local bond ends, a CSR adjacency whose slots carry neighbour, owner and bond id (integer LDS atomics count and fill it; the
//             order of an atom's slots is free), an n x n adjacency bit matrix (8 KiB at 256 atoms) for the chord tests, and z, the
//             closure flags, the input flags and ring_min as bytes.
//   cycles    C56 is enumerated, never stored: a work item is an adjacency slot (start a, first neighbour b > a), lane s takes slots s,
//             s + 64, ...: one atom of high degree is then not one lane's loop.  From (a, b) the walk goes over atoms above a, four nested
//             loops deep, and drops a new atom v as soon as v is bonded to an earlier atom of the path other than its predecessor -- the
//             path stays INDUCED --; a bond v - a at the fifth or sixth atom closes a chordless cycle (every chord of it has been tested on
//             the way), which is taken iff b < v: once, from its smallest atom, in one direction.  The walk's atoms live in registers (the
//             loops are written out): no scratch.
//   closure   sweeps until one changes nothing: R2 over atoms (lane-strided), then R3 over the enumerated cycles; both set flag bytes to
//             1 and never clear one.  Lanes may set the same byte and may read a byte another lane sets in the same sweep: the rules are
//             monotone, so every sweep ends between the state it started from and the least fixed point, and a sweep without a write has
//             read the state it started from everywhere: that state is closed.  At most n_atoms + 1 sweeps; a drug-like graph takes 2.
//   output    one more enumeration counts C56 and marks atoms and bonds of the cycles that lie in F (the closing bond is looked up in the
//             start atom's slots); then every element of the graph's rows is written.
//   cost      a step of the walk is one slot and at most four bit tests.  From one work item the walk visits at most
//             min(D^4, (2 m)^2) slots (D the largest degree, m < n + AR_C bonds).  The pruning is what keeps collapsed graphs cheap: in K17
//             every third atom is bonded to the start (nothing below depth 2); in K(2,120) every fourth is.  The worst case within the
//             limits is layered: b - 7 - 7 - 7 - 7 with complete bipartite layers (154 bonds over 29 atoms) has no chords between layers
//             two apart, 7^4 = 2401 slots per item, 308 items: about 12 000 steps per lane and enumeration, microseconds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cbgx.h"
#include "kernels.h"

namespace cbgx {

constexpr int AR_THREADS = 64;
constexpr int AR_N = CBGX_AROMATIC_MAX_ATOMS;
constexpr int AR_C = CBGX_AROMATIC_MAX_CYCLES;
constexpr int AR_M = AR_N + AR_C - 1;        // bonds of a graph that passes the check m < n + AR_C
constexpr int AR_W = AR_N / 32;              // words of a row of the adjacency bit matrix
static_assert(AR_N <= 256 && AR_N % 32 == 0 && AR_N <= 4 * AR_THREADS, "local atom indices are bytes; the degree scan gives a lane 4 atoms");
static_assert(AR_M < 65536, "bond ids are 16-bit");

struct AromaticGraph {                // a graph in LDS: 16.5 KiB
    int cursor[AR_N];                 // staging: degrees, then fill cursors
    int adj_ptr[AR_N + 1];
    unsigned adj_bits[AR_N * AR_W];   // bit v of row u: u and v are bonded
    uint16_t adj_bond[2 * AR_M];      // the bond of an adjacency slot
    uint8_t adj_atom[2 * AR_M], adj_owner[2 * AR_M];
    uint8_t end_i[AR_M], end_j[AR_M]; // local ends of a bond, i < j
    uint8_t z[AR_N], in_f[AR_N], flagged[AR_N], ring_min[AR_N], aromatic_atom[AR_N];
    uint8_t aromatic_bond[AR_M];
};

__device__ __forceinline__ bool ar_bonded(const AromaticGraph& G, int u, int v) { return (G.adj_bits[u * AR_W + (v >> 5)] >> (v & 31)) & 1u; }

__device__ __forceinline__ int ar_sum(int v) {
#pragma unroll
    for (int off = AR_THREADS / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// a chordless cycle a - b - c - d - e (- f; f < 0: five atoms) with the bonds of its path; the closing bond is looked up when needed.
// !FINAL: rule R3, returns whether a flag was set.  FINAL: counts the cycle and marks it when it lies in F.
template <bool FINAL>
__device__ __forceinline__ bool ar_cycle(AromaticGraph& G, int a, int b, int c, int d, int e, int f, int s1, int s2, int s3, int s4, int s5,
                                         int& n_cycles, int& n_aromatic) {
    const int atoms[6] = {a, b, c, d, e, f};        // (indexed by unrolled loops only: registers)
    const int len = f < 0 ? 5 : 6;
    int carbons = 0, carbons_in_f = 0, in_f = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        if (t < len) {
            const int v = atoms[t];
            const bool is_c = G.z[v] == 6, is_f = G.in_f[v] != 0;
            carbons += is_c; carbons_in_f += is_c && is_f; in_f += is_f;
        }
    }
    if (!FINAL) {
        if (in_f == len || 2 * carbons_in_f < carbons) return false;
#pragma unroll
        for (int t = 0; t < 6; ++t)
            if (t < len) G.in_f[atoms[t]] = 1;
        return true;
    }
    ++n_cycles;
    if (in_f != len) return false;
    ++n_aromatic;
#pragma unroll
    for (int t = 0; t < 6; ++t)
        if (t < len) G.aromatic_atom[atoms[t]] = 1;
    const int last = f < 0 ? e : f;
    G.aromatic_bond[G.adj_bond[s1]] = 1; G.aromatic_bond[G.adj_bond[s2]] = 1; G.aromatic_bond[G.adj_bond[s3]] = 1;
    G.aromatic_bond[G.adj_bond[s4]] = 1;
    if (f >= 0) G.aromatic_bond[G.adj_bond[s5]] = 1;
    for (int s = G.adj_ptr[a]; s < G.adj_ptr[a + 1]; ++s)
        if (G.adj_atom[s] == last) G.aromatic_bond[G.adj_bond[s]] = 1;
    return false;
}

// every cycle of C56 once (see `cycles` above); returns whether this lane set a flag (!FINAL)
template <bool FINAL>
__device__ bool ar_enumerate(AromaticGraph& G, int m, int lane, int& n_cycles, int& n_aromatic) {
    bool changed = false;
    for (int s1 = lane; s1 < 2 * m; s1 += AR_THREADS) {
        const int a = G.adj_owner[s1], b = G.adj_atom[s1];
        if (b <= a) continue;
        for (int s2 = G.adj_ptr[b]; s2 < G.adj_ptr[b + 1]; ++s2) {
            const int c = G.adj_atom[s2];
            if (c <= a || ar_bonded(G, c, a)) continue;
            for (int s3 = G.adj_ptr[c]; s3 < G.adj_ptr[c + 1]; ++s3) {
                const int d = G.adj_atom[s3];
                if (d <= a || d == b || ar_bonded(G, d, a) || ar_bonded(G, d, b)) continue;
                for (int s4 = G.adj_ptr[d]; s4 < G.adj_ptr[d + 1]; ++s4) {
                    const int e = G.adj_atom[s4];
                    if (e <= a || e == c || ar_bonded(G, e, b) || ar_bonded(G, e, c)) continue;
                    if (ar_bonded(G, e, a)) {
                        if (b < e) changed |= ar_cycle<FINAL>(G, a, b, c, d, e, -1, s1, s2, s3, s4, 0, n_cycles, n_aromatic);
                        continue;
                    }
                    for (int s5 = G.adj_ptr[e]; s5 < G.adj_ptr[e + 1]; ++s5) {
                        const int f = G.adj_atom[s5];
                        if (f <= a || f == d || f <= b || !ar_bonded(G, f, a)) continue;
                        if (ar_bonded(G, f, b) || ar_bonded(G, f, c) || ar_bonded(G, f, d)) continue;
                        changed |= ar_cycle<FINAL>(G, a, b, c, d, e, f, s1, s2, s3, s4, s5, n_cycles, n_aromatic);
                    }
                }
            }
        }
    }
    return changed;
}

__global__ __launch_bounds__(AR_THREADS) void ligand_aromatic_kernel(
    const uint8_t* __restrict__ z_lig, const uint8_t* __restrict__ flag_lig, const uint8_t* __restrict__ atom_ring_min,
    const int32_t* __restrict__ lig_ptr, int n_lig, const int32_t* __restrict__ bond_ptr, const int32_t* __restrict__ bond_index,
    int n_bonds, uint8_t* __restrict__ atom_out, uint8_t* __restrict__ bond_aromatic, int32_t* __restrict__ graph_out) {
    __shared__ AromaticGraph G;
    const int g = blockIdx.x, lane = threadIdx.x;
    // both ranges clamped to their arrays, as ligand_rings_kernel does: l0 <= l1 <= n_lig index bond_ptr [n_lig + 1] and the per-atom
    // arrays, b0 <= b1 <= n_bonds the list
    const int l0 = min(max(lig_ptr[g], 0), n_lig), l1 = min(max(lig_ptr[g + 1], l0), n_lig);
    const int p0 = bond_ptr[l0], p1 = bond_ptr[l1];
    const int b0 = min(max(p0, 0), n_bonds), b1 = min(max(p1, b0), n_bonds);
    const int n = l1 - l0, m = b1 - b0;
    const size_t row_j = (size_t)n_bonds;

    // ---- is this range of the list what the fill kernel writes?  did the ring report evaluate the graph? ----------------------------------
    bool bad = p0 != b0 || p1 != b1, no_rings = false;
    for (int a = l0 + lane; a < l1; a += AR_THREADS) {
        bad = bad || bond_ptr[a] > bond_ptr[a + 1];
        no_rings = no_rings || atom_ring_min[a] == 255;
    }
    for (int b = b0 + lane; b < b1; b += AR_THREADS) {
        const int i = bond_index[b], j = bond_index[row_j + b];
        bad = bad || !(l0 <= i && i < j && j < l1);
        if (b > b0) {
            const int pi = bond_index[b - 1], pj = bond_index[row_j + b - 1];
            bad = bad || !(pi < i || (pi == i && pj < j));
        }
    }
    int status = (n > AR_N ? CBGX_AROMATIC_TOO_MANY_ATOMS : 0) | (__any(bad) ? CBGX_AROMATIC_BAD_BONDS : 0);
    if (status == 0 && m >= n + AR_C) status = CBGX_AROMATIC_TOO_MANY_CYCLES;
    if (__any(no_rings)) status |= CBGX_AROMATIC_NO_RINGS;

    int n_cycles = 0, n_aromatic = 0, n_flagged = 0, n_closure = 0, n_aromatic_atoms = 0, n_aromatic_bonds = 0, n_unsupported = 0;
    if (status == 0) {
        // ---- staging: atoms, bond ends, adjacency -------------------------------------------------------------------------------------------
        for (int i = lane; i < n; i += AR_THREADS) {
            const uint8_t fl = flag_lig[l0 + i] != 0;
            G.cursor[i] = 0; G.z[i] = z_lig[l0 + i]; G.in_f[i] = fl; G.flagged[i] = fl; G.ring_min[i] = atom_ring_min[l0 + i];
            G.aromatic_atom[i] = 0;
        }
        for (int w = lane; w < n * AR_W; w += AR_THREADS) G.adj_bits[w] = 0;
        __syncthreads();
        for (int e = lane; e < m; e += AR_THREADS) {
            const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;      // 0 <= i < j < n: checked above
            G.end_i[e] = (uint8_t)i; G.end_j[e] = (uint8_t)j; G.aromatic_bond[e] = 0;
            atomicAdd(&G.cursor[i], 1); atomicAdd(&G.cursor[j], 1);
            atomicOr(&G.adj_bits[i * AR_W + (j >> 5)], 1u << (j & 31)); atomicOr(&G.adj_bits[j * AR_W + (i >> 5)], 1u << (i & 31));
        }
        __syncthreads();
        // exclusive prefix sum of the degrees: lane l takes atoms 4 l ... 4 l + 3
        int deg[4], sum = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) { const int a = 4 * lane + t; deg[t] = a < n ? G.cursor[a] : 0; sum += deg[t]; }
        int incl = sum;
#pragma unroll
        for (int off = 1; off < AR_THREADS; off <<= 1) { const int v = __shfl_up(incl, off); if (lane >= off) incl += v; }
        __syncthreads();
        int at = incl - sum;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int a = 4 * lane + t;
            if (a < n) { G.adj_ptr[a] = at; G.cursor[a] = at; at += deg[t]; }
        }
        if (lane == 0) G.adj_ptr[n] = 2 * m;
        __syncthreads();
        for (int e = lane; e < m; e += AR_THREADS) {
            const int i = G.end_i[e], j = G.end_j[e];
            int s = atomicAdd(&G.cursor[i], 1);
            G.adj_atom[s] = (uint8_t)j; G.adj_owner[s] = (uint8_t)i; G.adj_bond[s] = (uint16_t)e;
            s = atomicAdd(&G.cursor[j], 1);
            G.adj_atom[s] = (uint8_t)i; G.adj_owner[s] = (uint8_t)j; G.adj_bond[s] = (uint16_t)e;
        }
        __syncthreads();

        // ---- closure: sweeps of R2 and R3 until one sets nothing (every sweep but the last adds an atom: at most n + 1 of them) -------------
        for (int sweep = 0; sweep <= n; ++sweep) {
            bool changed = false;
            for (int a = lane; a < n; a += AR_THREADS) {
                const int zz = G.z[a], rm = G.ring_min[a];
                if (G.in_f[a] || (zz != 7 && zz != 8) || rm < 3 || rm > CBGX_RINGS_MAX_SIZE) continue;
                int in_f = 0;
                for (int s = G.adj_ptr[a]; s < G.adj_ptr[a + 1]; ++s) in_f += G.in_f[G.adj_atom[s]] != 0;
                if (in_f >= 2) { G.in_f[a] = 1; changed = true; }
            }
            __syncthreads();
            int unused0 = 0, unused1 = 0;
            changed |= ar_enumerate<false>(G, m, lane, unused0, unused1);
            __syncthreads();
            if (!__any(changed)) break;
        }

        // ---- aromatic cycles, atoms and bonds ----------------------------------------------------------------------------------------------
        ar_enumerate<true>(G, m, lane, n_cycles, n_aromatic);
        __syncthreads();
        n_cycles = ar_sum(n_cycles); n_aromatic = ar_sum(n_aromatic);
    }

    // ---- outputs: every element of the graph's rows -------------------------------------------------------------------------------------------
    for (int i = lane; i < n; i += AR_THREADS) {
        int v = 255;
        if (status == 0) {
            const int in_f = G.in_f[i] != 0, ar = G.aromatic_atom[i] != 0, fl = G.flagged[i] != 0;
            v = in_f | (ar << 1);
            n_flagged += fl; n_closure += in_f; n_aromatic_atoms += ar; n_unsupported += fl && !ar;
        }
        atom_out[(size_t)l0 + i] = (uint8_t)v;
    }
    for (int e = lane; e < m; e += AR_THREADS) {
        const int v = status ? 255 : G.aromatic_bond[e];
        if (status == 0) n_aromatic_bonds += v;
        bond_aromatic[(size_t)b0 + e] = (uint8_t)v;
    }
    n_flagged = ar_sum(n_flagged); n_closure = ar_sum(n_closure); n_aromatic_atoms = ar_sum(n_aromatic_atoms);
    n_unsupported = ar_sum(n_unsupported); n_aromatic_bonds = ar_sum(n_aromatic_bonds);
    if (lane == 0) {
        int32_t* o = graph_out + (size_t)CBGX_AROMATIC_GRAPH_COLS * g;
        o[0] = n; o[1] = m;
        o[2] = status ? -1 : n_cycles; o[3] = status ? -1 : n_aromatic; o[4] = status ? -1 : n_flagged; o[5] = status ? -1 : n_closure;
        o[6] = status ? -1 : n_aromatic_atoms; o[7] = status ? -1 : n_aromatic_bonds; o[8] = status ? -1 : n_unsupported;
        o[9] = status;
    }
}

hipError_t launch_ligand_aromatic(const uint8_t* z_lig, const uint8_t* flag_lig, const uint8_t* atom_ring_min, const int32_t* lig_ptr,
                                  int n_lig, int n_graphs, const int32_t* bond_ptr, const int32_t* bond_index, int n_bonds,
                                  uint8_t* atom_out, uint8_t* bond_aromatic, int32_t* graph_out, hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    hipLaunchKernelGGL(ligand_aromatic_kernel, dim3(n_graphs), dim3(AR_THREADS), 0, s, z_lig, flag_lig, atom_ring_min, lig_ptr, n_lig,
                       bond_ptr, bond_index, n_bonds, atom_out, bond_aromatic, graph_out);
    return hipGetLastError();
}

}  // namespace cbgx

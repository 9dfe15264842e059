// libcbgx -- ring sizes of the table-bond graph of a batch of sampled ligands (cbgx_ligand_rings; the definition is in include/cbgx.h): the
// substructure diagnostic of the reference's quality path (evaluate_scripts/evaluate_geom_single.py:27-33, print_ring_ratio;
// repo/tools/eval_ring_type.py, eval_ring_type_ratio / eval_ring_type_distribution), which the reference takes from RDKit's
// mol.GetRingInfo().AtomRings() after reconstruction -- here from the bond list of geometry.hip, for a whole batch in ONE launch.
//   shape     one 64-thread workgroup = ONE WAVE per graph.  The job shape is a thousand graphs of 10 - 45 atoms: there are more graphs
//             than SIMDs, so a graph needs no more than a wave, and a wave needs no protocol with anybody: the basis below is shared
//             by nobody else, nothing is locked, nothing spins.  (The barriers in this file are workgroup barriers of a one-wave
//             workgroup: they order the wave's own LDS traffic for the compiler and cannot wait for anyone.)
//   limits    a graph of more than RG_N atoms, with RG_C or more bonds beyond its atoms, or whose range of the list is not what the fill
//             kernel writes (rows not i < j inside the graph, bonds out of (i, j) order, bond_ptr decreasing) is reported in `status`
//             and nothing is built for it.  Every index into LDS below is a row of a checked bond minus the graph's first row: < RG_N.
//   staging   the bonds' local ends (a byte each), and a CSR adjacency whose slots carry the bond id; integer LDS atomics count and
//             fill it (the order of an atom's slots is free: nothing below depends on it).
//   forest    breadth-first trees from every atom no earlier tree reached: the number of components c, n_cycles = m - n + c, and
//             the bonds no tree claimed -- the co-tree -- numbered 0 ... n_cycles - 1 < RG_C.  A vector of the cycle space is determined
//             by its co-tree bonds, so every candidate is a 128-bit vector and a whole basis is RG_C x 16 B whatever the bond count.
//   classes   for k = 3 ... 9 in order, for every root atom of degree >= 2 (a candidate that is a cycle passes through its root on two
//             bonds): the breadth-first tree of the root cut at depth k / 2 -- a prefix of a tree cut at depth 4, and deep enough for
//             depth(x) + depth(y) + 1 = k --, then lane e, e + 64, ... takes bond e: if both ends were reached, it is no tree edge and
//             depth(x) + depth(y) + 1 == k, the lane XORs the co-tree bits of the bond and of both tree paths and reduces the vector
//             against the basis (kept by leading bit; read-only here, so the lanes work side by side).  Lanes left with a non-zero vector
//             are then taken one at a time: the vector is broadcast, reduced again by the whole wave against the basis as it now stands,
//             and stored under its leading bit if anything is left: rank + 1, rings_k + 1.  All of class k is in before class k + 1
//             starts; the loop ends after the class at which the rank reaches n_cycles.
//   ring_min  the class-k walk of root r also sees whether a candidate's ends hang under different children of r: the first k at which
//             one does is the length of the shortest cycle through r.  (Every atom on a cycle is on a basis cycle, so no atom is missed
//             by ending the loop at full rank.)
//   order     a breadth-first tree here depends on which lane claims an atom first; rank(S_k) does not depend on the trees nor on the
//             order of insertion (include/cbgx.h), and the shortest cycle through r is found from any tree of r.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cbgx.h"
#include "kernels.h"

namespace cbgx {

constexpr int RG_THREADS = 64;
constexpr int RG_N = CBGX_RINGS_MAX_ATOMS;
constexpr int RG_C = CBGX_RINGS_MAX_CYCLES;
constexpr int RG_M = RG_N + RG_C - 1;        // bonds of a graph within both limits: m = n_cycles + n - c <= RG_C + RG_N - 1
constexpr int RG_K0 = 3, RG_K1 = CBGX_RINGS_MAX_SIZE;
constexpr int RG_UNSEEN = -1;
static_assert(RG_N <= 256 && RG_N % 4 == 0 && RG_N <= 4 * RG_THREADS, "local atom indices are bytes; the degree scan gives a lane 4 atoms");
static_assert(RG_C == 128, "a cycle-space vector is two 64-bit words");
static_assert(RG_M < 32768, "bond ids and co-tree indices are 16-bit");

typedef unsigned long long u64;

struct RingGraph {                    // a graph in LDS: 9.6 KiB
    int depth[RG_N];                  // breadth-first depth from the current root, RG_UNSEEN: not reached (staging: degrees, cursors)
    int adj_ptr[RG_N + 1];
    u64 basis[RG_C][2];               // [leading bit] -> the basis vector with that leading bit, 0: none
    uint16_t adj_bond[2 * RG_M];      // the bond of an adjacency slot
    uint16_t up_bond[RG_N];           // the tree bond to the parent
    int16_t cotree[RG_M];             // co-tree index of a bond, -1: a bond of the spanning forest
    uint8_t end_i[RG_M], end_j[RG_M]; // local ends of a bond, i < j
    uint8_t adj_atom[2 * RG_M];
    uint8_t parent[RG_N], branch[RG_N], queue[RG_N], ring_min[RG_N];
    int tail;
    int rings[RG_K1 - RG_K0 + 1];
};

__device__ __forceinline__ u64 rg_shfl(u64 v, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ void rg_flip(u64& v0, u64& v1, int cotree) {
    if (cotree >= 0) {
        if (cotree < 64) v0 ^= 1ull << cotree; else v1 ^= 1ull << (cotree - 64);
    }
}

// reduces (v0, v1) against the basis; returns the leading bit under which what is left would be stored, -1 if nothing is left
__device__ __forceinline__ int rg_reduce(const RingGraph& G, u64& v0, u64& v1) {
    while (v0 | v1) {
        const int p = v1 ? 127 - __clzll((long long)v1) : 63 - __clzll((long long)v0);
        const u64 b0 = G.basis[p][0], b1 = G.basis[p][1];
        if (!(b0 | b1)) return p;
        v0 ^= b0; v1 ^= b1;         // (the leading bit goes: the loop ends after at most RG_C rounds)
    }
    return -1;
}

// breadth-first tree of `root` over the atoms whose depth is RG_UNSEEN, level by level, cut at max_depth: depth, parent, up_bond, branch
// (the child of the root an atom hangs under) of every atom reached; returns their number, queue[0 ... number) holds them (root first).
// An atom is claimed by an integer LDS compare-and-swap on its depth: once, by whichever lane comes first.
__device__ int rg_bfs(RingGraph& G, int root, int max_depth, int lane) {
    if (lane == 0) { G.depth[root] = 0; G.parent[root] = (uint8_t)root; G.branch[root] = (uint8_t)root; G.queue[0] = (uint8_t)root; G.tail = 1; }
    __syncthreads();
    int head = 0, tail = 1;
    for (int d = 0; d < max_depth && head < tail; ++d) {
        for (int q = head + lane; q < tail; q += RG_THREADS) {
            const int u = G.queue[q];
            for (int s = G.adj_ptr[u]; s < G.adj_ptr[u + 1]; ++s) {
                const int w = G.adj_atom[s];
                if (atomicCAS(&G.depth[w], RG_UNSEEN, d + 1) != RG_UNSEEN) continue;
                G.parent[w] = (uint8_t)u;
                G.up_bond[w] = G.adj_bond[s];
                G.branch[w] = d == 0 ? (uint8_t)w : G.branch[u];
                G.queue[atomicAdd(&G.tail, 1)] = (uint8_t)w;      // (an atom is claimed once: at most n <= RG_N entries)
            }
        }
        __syncthreads();
        head = tail;
        tail = G.tail;
        __syncthreads();
    }
    return tail;
}

__global__ __launch_bounds__(RG_THREADS) void ligand_rings_kernel(
    const int32_t* __restrict__ lig_ptr, int n_lig, const int32_t* __restrict__ bond_ptr, const int32_t* __restrict__ bond_index,
    int n_bonds, uint8_t* __restrict__ atom_ring_min, int32_t* __restrict__ graph_out) {
    __shared__ RingGraph G;
    const int g = blockIdx.x, lane = threadIdx.x;
    // both ranges clamped to their arrays, as the bond kernels do: l0 <= l1 <= n_lig index bond_ptr [n_lig + 1], b0 <= b1 <= n_bonds the list
    const int l0 = min(max(lig_ptr[g], 0), n_lig), l1 = min(max(lig_ptr[g + 1], l0), n_lig);
    const int p0 = bond_ptr[l0], p1 = bond_ptr[l1];
    const int b0 = min(max(p0, 0), n_bonds), b1 = min(max(p1, b0), n_bonds);
    const int n = l1 - l0, m = b1 - b0;
    const size_t row_j = (size_t)n_bonds;

    // ---- is this range of the list what the fill kernel writes? ---------------------------------------------------------------------------
    bool bad = p0 != b0 || p1 != b1;
    for (int a = l0 + lane; a < l1; a += RG_THREADS) bad = bad || bond_ptr[a] > bond_ptr[a + 1];
    for (int b = b0 + lane; b < b1; b += RG_THREADS) {
        const int i = bond_index[b], j = bond_index[row_j + b];
        bad = bad || !(l0 <= i && i < j && j < l1);
        if (b > b0) {
            const int pi = bond_index[b - 1], pj = bond_index[row_j + b - 1];
            bad = bad || !(pi < i || (pi == i && pj < j));
        }
    }
    int status = (n > RG_N ? CBGX_RINGS_TOO_MANY_ATOMS : 0) | (__any(bad) ? CBGX_RINGS_BAD_BONDS : 0);
    if (status == 0 && m >= n + RG_C) status = CBGX_RINGS_TOO_MANY_CYCLES;
    int n_cycles = 0;

    if (status == 0) {
        // ---- staging: bond ends, adjacency ------------------------------------------------------------------------------------------------
        for (int i = lane; i < n; i += RG_THREADS) { G.depth[i] = 0; G.ring_min[i] = 0; }
        if (lane < RG_K1 - RG_K0 + 1) G.rings[lane] = 0;
        for (int p = lane; p < RG_C; p += RG_THREADS) G.basis[p][0] = G.basis[p][1] = 0;
        __syncthreads();
        for (int e = lane; e < m; e += RG_THREADS) {
            const int i = bond_index[b0 + e] - l0, j = bond_index[row_j + b0 + e] - l0;      // 0 <= i < j < n: checked above
            G.end_i[e] = (uint8_t)i; G.end_j[e] = (uint8_t)j;
            atomicAdd(&G.depth[i], 1); atomicAdd(&G.depth[j], 1);
        }
        __syncthreads();
        // exclusive prefix sum of the degrees: lane l takes atoms 4 l ... 4 l + 3
        int deg[4], sum = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) { const int a = 4 * lane + t; deg[t] = a < n ? G.depth[a] : 0; sum += deg[t]; }
        int incl = sum;
#pragma unroll
        for (int off = 1; off < RG_THREADS; off <<= 1) { const int v = __shfl_up(incl, off); if (lane >= off) incl += v; }
        __syncthreads();
        int at = incl - sum;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int a = 4 * lane + t;
            if (a < n) { G.adj_ptr[a] = at; G.depth[a] = at; at += deg[t]; }      // (depth: the atom's fill cursor)
        }
        if (lane == 0) G.adj_ptr[n] = 2 * m;
        __syncthreads();
        for (int e = lane; e < m; e += RG_THREADS) {
            const int i = G.end_i[e], j = G.end_j[e];
            int s = atomicAdd(&G.depth[i], 1);
            G.adj_atom[s] = (uint8_t)j; G.adj_bond[s] = (uint16_t)e;
            s = atomicAdd(&G.depth[j], 1);
            G.adj_atom[s] = (uint8_t)i; G.adj_bond[s] = (uint16_t)e;
        }
        __syncthreads();

        // ---- spanning forest: components, cycle rank, co-tree numbering -------------------------------------------------------------------
        for (int i = lane; i < n; i += RG_THREADS) G.depth[i] = RG_UNSEEN;
        for (int e = lane; e < m; e += RG_THREADS) G.cotree[e] = 0;               // 0: no tree has claimed the bond
        __syncthreads();
        int n_comp = 0;
        for (int root = 0; root < n; ++root) {
            if (G.depth[root] != RG_UNSEEN) continue;                             // (the same value in every lane)
            ++n_comp;
            const int reached = rg_bfs(G, root, n, lane);
            for (int q = 1 + lane; q < reached; q += RG_THREADS) G.cotree[G.up_bond[G.queue[q]]] = -1;
            __syncthreads();
        }
        n_cycles = m - n + n_comp;
        int numbered = 0;
        for (int e0 = 0; e0 < m; e0 += RG_THREADS) {
            const int e = e0 + lane;
            const bool co = e < m && G.cotree[e] == 0;
            const u64 mask = __ballot(co);
            if (co) G.cotree[e] = (int16_t)(numbered + __popcll(mask & ((1ull << lane) - 1)));
            numbered += __popcll(mask);
        }
        if (n_cycles > RG_C) status = CBGX_RINGS_TOO_MANY_CYCLES;
        for (int i = lane; i < n; i += RG_THREADS) G.depth[i] = RG_UNSEEN;
        __syncthreads();
    }

    if (status == 0) {
        // ---- size classes ------------------------------------------------------------------------------------------------------------------
        int rank = 0;
        for (int k = RG_K0; k <= RG_K1 && rank < n_cycles; ++k) {
            int found = 0;
            for (int root = 0; root < n; ++root) {
                if (G.adj_ptr[root + 1] - G.adj_ptr[root] < 2) continue;
                const int reached = rg_bfs(G, root, k >> 1, lane);
                bool through = false;
                for (int e0 = 0; e0 < m; e0 += RG_THREADS) {
                    const int e = e0 + lane;
                    u64 v0 = 0, v1 = 0;
                    if (e < m) {
                        const int x = G.end_i[e], y = G.end_j[e];
                        const int dx = G.depth[x], dy = G.depth[y];
                        // (the graph is simple, so a tree edge is a bond between an atom and its parent; the root is its own parent)
                        if (dx != RG_UNSEEN && dy != RG_UNSEEN && dx + dy + 1 == k && G.parent[x] != y && G.parent[y] != x) {
                            through = through || G.branch[x] != G.branch[y];
                            rg_flip(v0, v1, G.cotree[e]);
                            for (int a = x; a != root; a = G.parent[a]) rg_flip(v0, v1, G.cotree[G.up_bond[a]]);
                            for (int a = y; a != root; a = G.parent[a]) rg_flip(v0, v1, G.cotree[G.up_bond[a]]);
                            rg_reduce(G, v0, v1);
                        }
                    }
                    // what is left is inserted one lane at a time, by the whole wave
                    for (u64 pending = __ballot((v0 | v1) != 0); pending; pending &= pending - 1) {
                        const int src = __ffsll((long long)pending) - 1;
                        u64 w0 = rg_shfl(v0, src), w1 = rg_shfl(v1, src);
                        const int p = rg_reduce(G, w0, w1);
                        if (p >= 0) {
                            if (lane == 0) { G.basis[p][0] = w0; G.basis[p][1] = w1; }
                            ++rank; ++found;
                        }
                        __syncthreads();
                    }
                }
                if (__any(through) && lane == 0 && G.ring_min[root] == 0) G.ring_min[root] = (uint8_t)k;
                for (int q = lane; q < reached; q += RG_THREADS) G.depth[G.queue[q]] = RG_UNSEEN;
                __syncthreads();
            }
            if (lane == 0) G.rings[k - RG_K0] = found;
        }
        __syncthreads();
    }

    // ---- outputs: every element of the graph's rows -----------------------------------------------------------------------------------------
    int n_ring_atoms = 0;
    for (int i0 = 0; i0 < n; i0 += RG_THREADS) {
        const int i = i0 + lane;
        int v = 0;
        if (i < n) {
            v = status ? 255 : G.ring_min[i];
            atom_ring_min[(size_t)l0 + i] = (uint8_t)v;
        }
        n_ring_atoms += __popcll(__ballot(v > 0));
    }
    if (lane == 0) {
        int32_t* o = graph_out + (size_t)CBGX_RINGS_GRAPH_COLS * g;
        o[0] = n; o[1] = m;
        int in_classes = 0;
        for (int c = 0; c <= RG_K1 - RG_K0; ++c) { const int r = status ? -1 : G.rings[c]; o[3 + c] = r; in_classes += r; }
        o[2] = status ? -1 : n_cycles;
        o[3 + RG_K1 - RG_K0 + 1] = status ? -1 : n_cycles - in_classes;
        o[4 + RG_K1 - RG_K0 + 1] = status ? -1 : n_ring_atoms;
        o[5 + RG_K1 - RG_K0 + 1] = status;
    }
}

hipError_t launch_ligand_rings(const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* bond_ptr, const int32_t* bond_index,
                               int n_bonds, uint8_t* atom_ring_min, int32_t* graph_out, hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    hipLaunchKernelGGL(ligand_rings_kernel, dim3(n_graphs), dim3(RG_THREADS), 0, s, lig_ptr, n_lig, bond_ptr, bond_index, n_bonds,
                       atom_ring_min, graph_out);
    return hipGetLastError();
}

}  // namespace cbgx

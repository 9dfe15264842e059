// libcbgx -- fingerprints of the table-bond graphs of a batch of sampled ligands and what they say ACROSS the samples of a pocket
// (cbgx_ligand_fingerprints, cbgx_group_diversity; the definitions are in include/cbgx.h): the raw material of the uniqueness and
// diversity numbers the reference takes from RDKit fingerprints and SMILES strings after reconstruction (repo/tools/similarity.py,
// evaluate_scripts/evaluate_chem_single.py).  Integer work only; nothing here depends on the order of atoms, bonds or lanes.
//
// ligand_fingerprints_kernel
//   shape     one 64-thread workgroup = ONE WAVE per graph, as rings.hip, aromatic.hip, valence.hip and groups.hip.  No protocol with
//             anybody, nothing spins, no atomics on memory.  (The barriers are workgroup barriers of a one-wave workgroup.)
//   limits    the checks of ligand_groups_kernel on the two ranges and the list; a type outside 1..4, a 255 byte in the graph's types or
//             ring bytes, no atom or more than FP_N atoms are reported in `status` and nothing is built.  Every index into LDS below is a
//             row of a checked bond minus the graph's first row: < FP_N.  There is NO limit on the bonds (the interface has no status for
//             one): up to FP_M bonds are staged in LDS as (i, j, type) words, which covers every graph the ring report evaluates (fewer
//             than n + 128 bonds), and a longer list is read from global memory every round instead.
//   rounds    lanes over BONDS add mix(id[other end] ^ type G) into a 64-bit accumulator of either end with LDS integer adds, lanes over
//             ATOMS then fold their accumulator into their id and clear it.  Sums of integers: the order of the adds is immaterial, so
//             there is no adjacency to sort and no degree to bound, and the lanes stay evenly loaded on star-like graphs.  The 64-bit
//             products of mix() compile to v_mul_lo_u32 / v_mul_hi_u32 / v_mad_u64_u32 sequences (three 32 x 32 products per
//             multiplication; checked in the ISA).
//   output    the fingerprint words are ORed together in LDS after rounds 0, 1 and 2; the hash is a wave sum over the atoms.
//
// group_diversity_kernel
//   shape     one DV_THREADS workgroup per group (pocket).  The cells (i, j) of the group's n x n square are dealt to the threads in
//             row-major order and the cells with i < j do the work: the lanes of a wave then share i and walk j, so the row of i is a
//             broadcast load and no square root is needed to find a pair.  Fingerprints stay in global memory (1024 rows are 128 KiB).
//   results   per graph a 64-bit key (similarity << 32 | ~index) under LDS integer max gives the nearest neighbour with the smallest
//             index on ties, an LDS integer min over the graphs of equal hash the first of them; sums, maxima and counts are reduced over
//             the workgroup.  Integers under commutative operations: nothing depends on scheduling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cbgx.h"
#include "kernels.h"

namespace cbgx {

constexpr int FP_THREADS = 64;
constexpr int FP_N = CBGX_FINGERPRINT_MAX_ATOMS;
constexpr int FP_M = 512;                                   // bonds staged in LDS; an evaluated ring report means fewer than FP_N + 128
constexpr int FP_WORDS = CBGX_FINGERPRINT_WORDS;
constexpr uint64_t FP_G = 0x9E3779B97F4A7C15ull;
static_assert(FP_N <= 256 && FP_WORDS * 32 == CBGX_FINGERPRINT_BITS && FP_WORDS <= FP_THREADS, "graph-local atoms fit a byte; a lane per word");
static_assert(FP_M >= FP_N + 128, "every graph the ring report evaluates is staged");

__device__ __forceinline__ uint64_t fp_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

struct FingerprintGraph {                                   // a graph in LDS: 7.1 KiB
    unsigned long long id[FP_N], acc[FP_N];                 // id_r of every atom; the sum over its bonds of round r
    unsigned bond[FP_M];                                    // i | j << 8 | type << 16, graph-local
    unsigned deg[FP_N];                                     // bonds of the atom; bit 31: one of them has type 4
    unsigned fp[FP_WORDS];
};

__global__ __launch_bounds__(FP_THREADS) void ligand_fingerprints_kernel(
    const uint8_t* __restrict__ z_lig, const int32_t* __restrict__ lig_ptr, int n_lig, const int32_t* __restrict__ bond_ptr,
    const int32_t* __restrict__ bond_index, const uint8_t* __restrict__ bond_type, const uint8_t* __restrict__ atom_ring_min, int n_bonds,
    uint32_t* __restrict__ fp, uint64_t* __restrict__ mol_hash, int32_t* __restrict__ graph_out) {
    __shared__ FingerprintGraph L;
    const int g = blockIdx.x, lane = threadIdx.x;
    // both ranges clamped to their arrays, as ligand_groups_kernel does
    const int l0 = min(max(lig_ptr[g], 0), n_lig), l1 = min(max(lig_ptr[g + 1], l0), n_lig);
    const int p0 = bond_ptr[l0], p1 = bond_ptr[l1];
    const int b0 = min(max(p0, 0), n_bonds), b1 = min(max(p1, b0), n_bonds);
    const int n = l1 - l0, m = b1 - b0;
    const size_t row_j = (size_t)n_bonds;

    // ---- is this range of the list what the fill kernel writes?  types 1..4?  did the ring and aromatic reports evaluate the graph? ------
    bool bad = p0 != b0 || p1 != b1, no_types = false;
    for (int a = l0 + lane; a < l1; a += FP_THREADS) {
        bad = bad || bond_ptr[a] > bond_ptr[a + 1];
        no_types = no_types || atom_ring_min[a] == 255;
    }
    for (int b = b0 + lane; b < b1; b += FP_THREADS) {
        const int i = bond_index[b], j = bond_index[row_j + b], t = bond_type[b];
        bad = bad || !(l0 <= i && i < j && j < l1) || (t != 255 && (t < 1 || t > 4));
        if (b > b0) {
            const int pi = bond_index[b - 1], pj = bond_index[row_j + b - 1];
            bad = bad || !(pi < i || (pi == i && pj < j));
        }
        no_types = no_types || t == 255;
    }
    const int status = (n > FP_N ? CBGX_FINGERPRINT_TOO_MANY_ATOMS : 0) | (__any(bad) ? CBGX_FINGERPRINT_BAD_BONDS : 0) |
                       (__any(no_types) ? CBGX_FINGERPRINT_NO_TYPES : 0) | (n == 0 ? CBGX_FINGERPRINT_EMPTY : 0);

    uint64_t hash = 0;
    int n_bits = -1, n_rounds = -1;
    if (lane < FP_WORDS) L.fp[lane] = 0;
    if (status == 0) {
        const bool staged = m <= FP_M;
        // bond e of the graph (0 <= e < m) as i | j << 8 | type << 16: 0 <= i < j < n <= 256 and 1 <= type <= 4 were checked above
        auto from_list = [&](int e) {
            return (unsigned)(bond_index[b0 + e] - l0) | (unsigned)(bond_index[row_j + b0 + e] - l0) << 8 | (unsigned)bond_type[b0 + e] << 16;
        };
        auto bond_of = [&](int e) { return staged ? L.bond[e] : from_list(e); };
        for (int a = lane; a < n; a += FP_THREADS) { L.deg[a] = 0; L.acc[a] = 0; }
        if (staged)
            for (int e = lane; e < m; e += FP_THREADS)
                L.bond[e] = from_list(e);
        __syncthreads();
        for (int e = lane; e < m; e += FP_THREADS) {
            const unsigned w = bond_of(e);
            const int i = w & 255, j = (w >> 8) & 255;
            // (the count cannot carry into bit 31: an atom has fewer than 256 bonds; the flag is ORed in on its own)
            atomicAdd(&L.deg[i], 1u); atomicAdd(&L.deg[j], 1u);
            if ((w >> 16) == 4) { atomicOr(&L.deg[i], 0x80000000u); atomicOr(&L.deg[j], 0x80000000u); }
        }
        __syncthreads();
        for (int a = lane; a < n; a += FP_THREADS) {
            const unsigned d = L.deg[a];
            const uint64_t id = fp_mix(FP_G + z_lig[l0 + a] + 256ull * (d & 0x7FFFFFFFu) + 65536ull * (d >> 31) + 131072ull * atom_ring_min[l0 + a]);
            L.id[a] = id;
            atomicOr(&L.fp[(id & (CBGX_FINGERPRINT_BITS - 1)) >> 5], 1u << (id & 31));
        }
        __syncthreads();
        n_rounds = max(n, 2);
        for (int r = 0; r < n_rounds; ++r) {               // id_r -> id_(r + 1)
            for (int e = lane; e < m; e += FP_THREADS) {
                const unsigned w = bond_of(e);
                const int i = w & 255, j = (w >> 8) & 255;
                const uint64_t tg = (uint64_t)(w >> 16) * FP_G;
                atomicAdd(&L.acc[i], (unsigned long long)fp_mix(L.id[j] ^ tg));
                atomicAdd(&L.acc[j], (unsigned long long)fp_mix(L.id[i] ^ tg));
            }
            __syncthreads();
            for (int a = lane; a < n; a += FP_THREADS) {
                const uint64_t id = fp_mix(L.id[a] + L.acc[a]);
                L.id[a] = id; L.acc[a] = 0;
                if (r < 2) atomicOr(&L.fp[(id & (CBGX_FINGERPRINT_BITS - 1)) >> 5], 1u << (id & 31));
            }
            __syncthreads();
        }
        for (int a = lane; a < n; a += FP_THREADS) hash += fp_mix(L.id[a] ^ FP_G);
        int bits = lane < FP_WORDS ? __popc(L.fp[lane]) : 0;
#pragma unroll
        for (int off = FP_THREADS / 2; off > 0; off >>= 1) {
            hash += __shfl_xor((unsigned long long)hash, off);
            bits += __shfl_xor(bits, off);
        }
        hash = fp_mix(hash + (uint64_t)n + ((uint64_t)m << 32));
        n_bits = bits;
    }

    // ---- outputs: every element of the graph's rows ---------------------------------------------------------------------------------------
    if (lane < FP_WORDS) fp[(size_t)FP_WORDS * g + lane] = L.fp[lane];      // (all zero with a status: written by this lane above)
    if (lane == 0) {
        mol_hash[g] = hash;
        int32_t* o = graph_out + (size_t)CBGX_FINGERPRINT_GRAPH_COLS * g;
        o[0] = n; o[1] = m; o[2] = n_bits; o[3] = n_rounds; o[4] = status;
    }
}

hipError_t launch_ligand_fingerprints(const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* bond_ptr,
                                      const int32_t* bond_index, const uint8_t* bond_type, const uint8_t* atom_ring_min, int n_bonds,
                                      uint32_t* fp, uint64_t* mol_hash, int32_t* graph_out, hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    hipLaunchKernelGGL(ligand_fingerprints_kernel, dim3(n_graphs), dim3(FP_THREADS), 0, s, z_lig, lig_ptr, n_lig, bond_ptr, bond_index,
                       bond_type, atom_ring_min, n_bonds, fp, mol_hash, graph_out);
    return hipGetLastError();
}

// ---- across the graphs of a group ------------------------------------------------------------------------------------------------------------
constexpr int DV_THREADS = 256;
constexpr int DV_WAVES = DV_THREADS / 64;
constexpr int DV_N = CBGX_DIVERSITY_MAX_GROUP;

struct DiversityGroup {                                     // a group in LDS: 21 KiB
    unsigned long long key[DV_N];                           // (best similarity << 32) | (0xFFFFFFFF - its index); 0: no neighbour
    unsigned long long hash[DV_N];
    int first[DV_N];                                        // the smallest evaluated index of equal hash
    uint8_t ok[DV_N];
    long long sum[DV_WAVES], pairs[DV_WAVES];
    int top[DV_WAVES], evaluated[DV_WAVES], unique[DV_WAVES];
};

__global__ __launch_bounds__(DV_THREADS) void group_diversity_kernel(
    const uint32_t* __restrict__ fp, const uint64_t* __restrict__ mol_hash, const int32_t* __restrict__ status,
    const int32_t* __restrict__ group_ptr, const int64_t* __restrict__ pair_ptr, int n_graphs, long long n_pairs,
    int32_t* __restrict__ pair_sim, int32_t* __restrict__ first_same, int32_t* __restrict__ nearest, int32_t* __restrict__ nearest_micro,
    int64_t* __restrict__ group_out) {
    __shared__ DiversityGroup L;
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const int r0 = group_ptr[p], r1 = group_ptr[p + 1];
    const int g0 = min(max(r0, 0), n_graphs), g1 = min(max(r1, g0), n_graphs);
    const int n = g1 - g0;
    const long long q0 = pair_ptr[p], q1 = pair_ptr[p + 1], want = (long long)n * (n - 1) / 2;
    // pair_sim is written only where the group's range of it is what the host computes and lies inside the array
    const bool fits = q0 >= 0 && q1 <= n_pairs && q1 - q0 == want;
    const int st = ((r0 != g0 || r1 != g1 || !fits) ? CBGX_DIVERSITY_BAD_GROUPS : 0) | (n > DV_N ? CBGX_DIVERSITY_TOO_MANY_GRAPHS : 0);
    int64_t* o = group_out + (size_t)CBGX_DIVERSITY_GROUP_COLS * p;

    if (n > DV_N) {
        for (int i = tid; i < n; i += DV_THREADS) { first_same[g0 + i] = -1; nearest[g0 + i] = -1; nearest_micro[g0 + i] = -1; }
        if (fits)
            for (long long k = tid; k < want; k += DV_THREADS) pair_sim[q0 + k] = -1;
        if (tid == 0) { o[0] = n; o[1] = o[2] = o[3] = o[4] = o[5] = -1; o[6] = st; }
        return;
    }

    int evaluated = 0;
    for (int i = tid; i < n; i += DV_THREADS) {
        const bool ok = status[g0 + i] == 0;
        L.ok[i] = ok; L.hash[i] = mol_hash[g0 + i]; L.key[i] = 0; L.first[i] = i;
        evaluated += ok;
    }
    __syncthreads();

    long long sum = 0, pairs = 0;
    int top = -1;
    const int cells = n * n;                                 // n <= 1024
    for (int c = tid; c < cells; c += DV_THREADS) {
        const int i = c / n, j = c - i * n;
        if (i >= j) continue;
        int sim = -1;
        if (L.ok[i] && L.ok[j]) {
            const uint4* a = reinterpret_cast<const uint4*>(fp + (size_t)CBGX_FINGERPRINT_WORDS * (g0 + i));
            const uint4* b = reinterpret_cast<const uint4*>(fp + (size_t)CBGX_FINGERPRINT_WORDS * (g0 + j));
            int inter = 0, uni = 0;
#pragma unroll
            for (int w = 0; w < CBGX_FINGERPRINT_WORDS / 4; ++w) {
                const uint4 x = a[w], y = b[w];
                inter += __popc(x.x & y.x) + __popc(x.y & y.y) + __popc(x.z & y.z) + __popc(x.w & y.w);
                uni += __popc(x.x | y.x) + __popc(x.y | y.y) + __popc(x.z | y.z) + __popc(x.w | y.w);
            }
            // an evaluated graph has an atom and so a bit; a caller's all-zero rows give 0, not a division by zero
            sim = uni ? (int)(((long long)inter * 1000000 + uni / 2) / uni) : 0;
            sum += sim; ++pairs; top = max(top, sim);
            atomicMax(&L.key[i], (unsigned long long)sim << 32 | (0xFFFFFFFFu - (unsigned)j));
            atomicMax(&L.key[j], (unsigned long long)sim << 32 | (0xFFFFFFFFu - (unsigned)i));
            if (L.hash[i] == L.hash[j]) atomicMin(&L.first[j], i);
        }
        if (fits) pair_sim[q0 + (long long)i * n - (long long)i * (i + 1) / 2 + (j - i - 1)] = sim;
    }
    __syncthreads();

    int unique = 0;
    for (int i = tid; i < n; i += DV_THREADS) {
        const bool ok = L.ok[i];
        const unsigned long long key = L.key[i];
        first_same[g0 + i] = ok ? L.first[i] : -1;
        nearest[g0 + i] = ok && key ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
        nearest_micro[g0 + i] = ok && key ? (int)(key >> 32) : -1;
        unique += ok && L.first[i] == i;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off); pairs += __shfl_xor(pairs, off);
        top = max(top, __shfl_xor(top, off)); evaluated += __shfl_xor(evaluated, off); unique += __shfl_xor(unique, off);
    }
    if ((tid & 63) == 0) { L.sum[wave] = sum; L.pairs[wave] = pairs; L.top[wave] = top; L.evaluated[wave] = evaluated; L.unique[wave] = unique; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < DV_WAVES; ++w) {
            sum += L.sum[w]; pairs += L.pairs[w]; top = max(top, L.top[w]); evaluated += L.evaluated[w]; unique += L.unique[w];
        }
        o[0] = n; o[1] = evaluated; o[2] = unique; o[3] = pairs; o[4] = sum; o[5] = top; o[6] = st;
    }
}

hipError_t launch_group_diversity(const uint32_t* fp, const uint64_t* mol_hash, const int32_t* status, const int32_t* group_ptr,
                                  const int64_t* pair_ptr, int n_graphs, int n_groups, long long n_pairs, int32_t* pair_sim,
                                  int32_t* first_same, int32_t* nearest, int32_t* nearest_micro, int64_t* group_out, hipStream_t s) {
    if (n_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(group_diversity_kernel, dim3(n_groups), dim3(DV_THREADS), 0, s, fp, mol_hash, status, group_ptr, pair_ptr, n_graphs,
                       n_pairs, pair_sim, first_same, nearest, nearest_micro, group_out);
    return hipGetLastError();
}

}  // namespace cbgx

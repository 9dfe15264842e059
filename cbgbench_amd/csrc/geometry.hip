// libcbgx -- geometry report of a batch of sampled ligands: atom / molecule stability and protein-ligand steric clash, the two metrics of
// the reference's quality path that need coordinates and elements only (repo/tools/geometry/eval_stability.py, check_stability with
// hs=False; repo/tools/geometry/eval_steric_clash.py, detect_clash), for a whole batch in ONE launch, one 256-thread workgroup per graph.
//   staging   the graph's ligand coordinates (fp32) and element codes go to LDS; a ligand has at most GEO_MAX atoms (the host entry
//             refuses larger ones before the launch).  The number of protein atoms is not limited: they are streamed.
//   distance  coordinates widened to fp64; dx = xi - xj (dy, dz likewise); s = (dx dx + dy dy) + dz dz, every product and sum rounded on
//             its own; d = sqrt(s), correctly rounded.  Contraction is OFF for this translation unit (the pragma below): the products and
//             sums are written as plain operators because the header's __dmul_rn / __dadd_rn are plain operators too and would be fused
//             after inlining under the default -ffp-contract=fast-honor-pragmas.
//   bonds     order(i, j) of a ligand pair i != j from the pair's single / double / triple bond lengths b1 / b2 / b3 (pm, -1: none) and
//             p = 100.0 d:   p < b1 + 10 ? (p < b2 + 5 ? (p < b3 + 3 ? 3 : 2) : 1) : 0, comparisons strict.  nr_bonds[i] = sum_j order(i, j):
//             thread i, i + 256, ... walks its whole row -- the symmetric work is done twice, so there are no atomics and no order.
//             Atom i is stable iff allowed[z_i] >= nr_bonds[i] > 0.
//   clash     d < (r_lig + r_other) - 0.4 in fp64, in that order.  Inter-clash: thread k, k + 256, ... takes protein atoms and tests them
//             against the ligand in LDS; a hit marks the ligand atom with an LDS integer atomicOr (order-independent).  Intra-clash:
//             ligand pairs i != j whose TABLE bond order is 0, found in the row walk.  The reference masks intra-ligand pairs with RDKit's
//             bond adjacency; the table bond is this library's RDKit-free stand-in (flag CBGX_GEOM_INTRA_CLASH, field
//             intra_clash_table_bonds of the Python side).
//   elements  a protein atom whose element has no radius (Se: the reference raises KeyError there) takes no part and is counted per graph;
//             a ligand atom outside {H, C, N, O, F, P, S, Cl} has nr_bonds = 0, is unstable, takes no part in bonds or clashes and carries
//             CBGX_GEOM_UNKNOWN_ELEMENT.
//   shortcut  a pair with s >= 25 (d >= 5 A exactly, sqrt being monotonic and sqrt(25) = 5) is skipped before the square root: the largest
//             bond threshold is 2.31 A (P-P, 221 + 10 pm) and the largest clash threshold 4.14 A (Cl...Cl), so no result can change.
//   outputs   nr_bonds, flags and the six per-graph counts (integer reductions of the flags) -- every element of every graph is written.
//
// Constants (physical; written in geo_tables.h as dense arrays over an element code, built at compile time from pair lists):
//   bond lengths  the table EDM's stability metric uses (Hoogeboom et al., "Equivariant Diffusion for Molecule Generation in 3D", 2022,
//                 qm9/bond_analyze.py), itself from http://www.wiredchemist.com/chemistry/data/bond_energies_lengths.html and
//                 http://chemistry-reference.com/tables/Bond%20Lengths%20and%20Enthalpies.pdf; margins 10 / 5 / 3 pm as tuned there on QM9.
//   valences      the usual maximum valences of the eight elements (same source).
//   radii, 0.4 A  van der Waals radii (Bondi-type) and the overlap of Proteopedia's definition: "a clash is considered to occur when the
//                 van der Waals radii overlap by >= 0.4 A between non-bound atoms" (https://proteopedia.org/wiki/index.php/Clashes).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cbgx.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "geo_tables.h"      // limits, element codes, GeoTables / make_geo_tables, geo_dist2

namespace cbgx {

static const GeoTables h_geo = make_geo_tables();      // what cbgx_ligand_geometry_tables hands out
__constant__ GeoTables d_geo = make_geo_tables();      // what the kernel reads: the same initialiser

// element code of an atomic number among the first `n_codes` codes, GEO_NONE when it has none
__device__ __forceinline__ int geo_code(uint8_t z, int n_codes) {
    int code = GEO_NONE;
#pragma unroll
    for (int c = 0; c < GEO_VDW; ++c)
        if (c < n_codes && d_geo.z[c] == z) code = c;
    return code;
}

__global__ __launch_bounds__(GEO_THREADS) void ligand_geometry_kernel(
    const float* __restrict__ x_lig, const uint8_t* __restrict__ z_lig, const int32_t* __restrict__ lig_ptr, int n_lig,
    const float* __restrict__ x_rec, const uint8_t* __restrict__ z_rec, const int32_t* __restrict__ rec_ptr, int n_rec,
    int32_t* __restrict__ nr_bonds, uint8_t* __restrict__ flags, int32_t* __restrict__ graph_out) {
    __shared__ float sx[GEO_MAX], sy[GEO_MAX], sz[GEO_MAX];
    __shared__ uint8_t scode[GEO_MAX];
    __shared__ int sflag[GEO_MAX];               // CBGX_GEOM_* bits of a ligand atom
    __shared__ int snb[GEO_MAX];
    __shared__ double sbond[GEO_EL * GEO_EL][3]; // bond length + margin of a pair, as the fp64 value p is compared with
    __shared__ double sclash[GEO_EL][GEO_VDW];   // (r_lig + r_other) - tolerance
    __shared__ int scount[4];                    // stable, inter-clash, intra-clash atoms; protein atoms without a radius
    const int g = blockIdx.x, k = threadIdx.x;
    // a malformed CSR must not reach outside the arrays: both ranges are clamped to them (and the ligand to the LDS it is staged in)
    const int r0 = min(max(rec_ptr[g], 0), n_rec), r1 = min(max(rec_ptr[g + 1], r0), n_rec);
    const int l0 = min(max(lig_ptr[g], 0), n_lig), l1 = min(max(lig_ptr[g + 1], l0), n_lig);
    const int nr = r1 - r0, nl = min(l1 - l0, GEO_MAX);

    for (int i = k; i < nl; i += GEO_THREADS) {
        const size_t a = (size_t)(l0 + i);
        sx[i] = x_lig[3 * a + 0]; sy[i] = x_lig[3 * a + 1]; sz[i] = x_lig[3 * a + 2];
        const int code = geo_code(z_lig[a], GEO_EL);
        scode[i] = (uint8_t)code;
        sflag[i] = code == GEO_NONE ? (int)CBGX_GEOM_UNKNOWN_ELEMENT : 0;
    }
    for (int p = k; p < GEO_EL * GEO_EL; p += GEO_THREADS)
        for (int o = 0; o < 3; ++o) sbond[p][o] = (double)(d_geo.bond_pm[o][p / GEO_EL][p % GEO_EL] + d_geo.margin[o]);
    for (int p = k; p < GEO_EL * GEO_VDW; p += GEO_THREADS)
        sclash[p / GEO_VDW][p % GEO_VDW] = (d_geo.radius[p / GEO_VDW] + d_geo.radius[p % GEO_VDW]) - d_geo.tolerance;
    if (k < 4) scount[k] = 0;
    __syncthreads();

    // ---- ligand rows: bond orders and intra-ligand clashes ----------------------------------------------------------------------------
    for (int i = k; i < nl; i += GEO_THREADS) {
        const int ci = scode[i];
        int nb = 0;
        bool intra = false;
        if (ci != GEO_NONE) {
            const double xi = (double)sx[i], yi = (double)sy[i], zi = (double)sz[i];
            for (int j = 0; j < nl; ++j) {
                const int cj = scode[j];
                if (j == i || cj == GEO_NONE) continue;
                const double s = geo_dist2(xi, yi, zi, sx[j], sy[j], sz[j]);
                if (s >= GEO_FAR2) continue;
                const double d = __dsqrt_rn(s);
                const double p = 100.0 * d;
                const double* t = sbond[ci * GEO_EL + cj];
                int order = 0;
                if (p < t[0]) order = p < t[1] ? (p < t[2] ? 3 : 2) : 1;
                nb += order;
                intra = intra || (order == 0 && d < sclash[ci][cj]);
            }
        }
        snb[i] = nb;
        if (intra) atomicOr(&sflag[i], (int)CBGX_GEOM_INTRA_CLASH);
    }
    // ---- protein atoms against the ligand ---------------------------------------------------------------------------------------------
    int no_radius = 0;
    for (int q = k; q < nr; q += GEO_THREADS) {
        const size_t a = (size_t)(r0 + q);
        const int cr = geo_code(z_rec[a], GEO_VDW);
        if (cr == GEO_NONE) { ++no_radius; continue; }
        const double px = (double)x_rec[3 * a + 0], py = (double)x_rec[3 * a + 1], pz = (double)x_rec[3 * a + 2];
        for (int j = 0; j < nl; ++j) {
            const int cj = scode[j];
            if (cj == GEO_NONE) continue;
            // (d = |x_lig - x_rec|: the squares make the order of the subtraction irrelevant)
            const double s = geo_dist2(px, py, pz, sx[j], sy[j], sz[j]);
            if (s >= GEO_FAR2) continue;
            if (__dsqrt_rn(s) < sclash[cj][cr]) atomicOr(&sflag[j], (int)CBGX_GEOM_INTER_CLASH);
        }
    }
    if (no_radius) atomicAdd(&scount[3], no_radius);
    __syncthreads();

    // ---- flags, counts ----------------------------------------------------------------------------------------------------------------
    int n_stable = 0, n_inter = 0, n_intra = 0;
    for (int i = k; i < nl; i += GEO_THREADS) {
        const int ci = scode[i], nb = snb[i];
        int f = sflag[i];
        if (ci != GEO_NONE && nb > 0 && nb <= d_geo.allowed[ci]) f |= (int)CBGX_GEOM_STABLE;
        const size_t a = (size_t)(l0 + i);
        nr_bonds[a] = nb;
        flags[a] = (uint8_t)f;
        n_stable += f & 1; n_inter += (f >> 1) & 1; n_intra += (f >> 2) & 1;
    }
    if (n_stable) atomicAdd(&scount[0], n_stable);
    if (n_inter) atomicAdd(&scount[1], n_inter);
    if (n_intra) atomicAdd(&scount[2], n_intra);
    __syncthreads();
    if (k == 0) {
        int32_t* o = graph_out + (size_t)CBGX_GEOMETRY_GRAPH_COLS * g;
        o[0] = nl; o[1] = scount[0]; o[2] = (scount[0] == nl && nl > 0) ? 1 : 0; o[3] = scount[1]; o[4] = scount[2]; o[5] = scount[3];
    }
}

hipError_t launch_ligand_geometry(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, const float* x_rec,
                                  const uint8_t* z_rec, const int32_t* rec_ptr, int n_rec, int n_graphs, int32_t* nr_bonds,
                                  uint8_t* flags, int32_t* graph_out, hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    hipLaunchKernelGGL(ligand_geometry_kernel, dim3(n_graphs), dim3(GEO_THREADS), 0, s, x_lig, z_lig, lig_ptr, n_lig, x_rec, z_rec,
                       rec_ptr, n_rec, nr_bonds, flags, graph_out);
    return hipGetLastError();
}

// ---- bond list, fragments and connectivity (cbgx_ligand_bonds_count / cbgx_ligand_bonds_fill) -------------------------------------------
// The molecular graph the row walk above sums over and throws away, kept: the pairs i < j of a ligand whose table bond order is > 0, in
// (i, j) order, and the connected components of that graph.  Same staging, same distance, same order, same tables as the kernel above;
// proteins play no part.  The number of bonds of a graph is not bounded by its number of atoms (all atoms at one point: n (n - 1) / 2), so
// the list is made in two launches: `count` writes every atom's number of partners j > i, the caller turns them into an exclusive prefix
// sum, `fill` walks the same pairs again and writes atom a's partners in ascending j from bond_ptr[a] on -- no atomics, one order.
//   components  label[i] = the smallest ligand-local index of i's component, by min-label propagation with root hooking and pointer
//               jumping over rounds that recompute the distances (no adjacency is stored: 128 KiB of LDS for a bit matrix would leave one
//               workgroup per CU).  Labels live in LDS, start at label[i] = i and only ever decrease, to labels of atoms of the same
//               component; so label[i] <= i and label[i] >= min(component) throughout.
//                 hook   atom i reads m = min(label[i], label[j] over its bonded j); if m < label[i]: integer atomicMin of label[i] and of
//                        label[old label[i]] with m, and the round is marked as changed.
//                 jump   label[i] = the root reached by following labels (l = label[l] while label[l] < l: strictly decreasing, ends).
//               A round without a change read a snapshot nobody wrote to, in which no atom has a bonded partner with a smaller label:
//               labels are constant over a component, and since the component's smallest atom m has label[m] <= m inside the component,
//               that constant is m.  That fixed point is unique, so the result does not depend on the order in which threads saw each
//               other's updates.  Plain propagation alone gives an atom at graph distance r from m the label m after r rounds, so n - 1
//               rounds always suffice and the loop is bounded by n; hooking and jumping make it a handful in practice.
//   counts      n_bonds, the sum of orders (integer LDS atomics), the number of roots, the largest component (integer LDS histogram over
//               the roots), n_cycles = n_bonds - n_atoms + n_fragments (the cycle rank of the graph).

struct GeoLigand {       // a graph's ligand in LDS
    float x[GEO_MAX], y[GEO_MAX], z[GEO_MAX];
    uint8_t code[GEO_MAX];
    double bond[GEO_EL * GEO_EL][3];      // bond length + margin of a pair of codes, as the fp64 value p is compared with
};

// stages graph g's ligand; returns its number of atoms and its first row (the range clamped to the array and to the LDS, as above)
__device__ __forceinline__ int geo_stage_ligand(GeoLigand& L, const float* __restrict__ x_lig, const uint8_t* __restrict__ z_lig,
                                                const int32_t* __restrict__ lig_ptr, int n_lig, int g, int k, int& l0) {
    l0 = min(max(lig_ptr[g], 0), n_lig);
    const int l1 = min(max(lig_ptr[g + 1], l0), n_lig);
    const int nl = min(l1 - l0, GEO_MAX);
    for (int i = k; i < nl; i += GEO_THREADS) {
        const size_t a = (size_t)(l0 + i);
        L.x[i] = x_lig[3 * a + 0]; L.y[i] = x_lig[3 * a + 1]; L.z[i] = x_lig[3 * a + 2];
        L.code[i] = (uint8_t)geo_code(z_lig[a], GEO_EL);
    }
    for (int p = k; p < GEO_EL * GEO_EL; p += GEO_THREADS)
        for (int o = 0; o < 3; ++o) L.bond[p][o] = (double)(d_geo.bond_pm[o][p / GEO_EL][p % GEO_EL] + d_geo.margin[o]);
    return nl;
}

// table bond order of the staged atoms i != j, both with a code (0: none); d: the distance the order was decided on (set when s < 25)
__device__ __forceinline__ int geo_pair_order(const GeoLigand& L, double xi, double yi, double zi, int ci, int j, int cj, double& d) {
    const double s = geo_dist2(xi, yi, zi, L.x[j], L.y[j], L.z[j]);
    if (s >= GEO_FAR2) return 0;
    d = __dsqrt_rn(s);
    const double p = 100.0 * d;
    const double* t = L.bond[ci * GEO_EL + cj];
    return p < t[0] ? (p < t[1] ? (p < t[2] ? 3 : 2) : 1) : 0;
}

__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__global__ __launch_bounds__(GEO_THREADS) void ligand_bonds_count_kernel(
    const float* __restrict__ x_lig, const uint8_t* __restrict__ z_lig, const int32_t* __restrict__ lig_ptr, int n_lig,
    int32_t* __restrict__ deg_up, int32_t* __restrict__ fragment, int32_t* __restrict__ graph_out) {
    __shared__ GeoLigand L;
    __shared__ int slabel[GEO_MAX];
    __shared__ int ssize[GEO_MAX];      // atoms of the component whose root this is
    __shared__ int scount[4];           // bonds, sum of orders, roots, largest component
    __shared__ int schanged;
    const int g = blockIdx.x, k = threadIdx.x;
    int l0;
    const int nl = geo_stage_ligand(L, x_lig, z_lig, lig_ptr, n_lig, g, k, l0);
    for (int i = k; i < nl; i += GEO_THREADS) { slabel[i] = i; ssize[i] = 0; }
    if (k < 4) scount[k] = 0;
    __syncthreads();

    // ---- partners j > i of every atom ----------------------------------------------------------------------------------------------
    int n_bonds = 0, order_sum = 0;
    for (int i = k; i < nl; i += GEO_THREADS) {
        const int ci = L.code[i];
        int deg = 0;
        if (ci != GEO_NONE) {
            const double xi = (double)L.x[i], yi = (double)L.y[i], zi = (double)L.z[i];
            for (int j = i + 1; j < nl; ++j) {
                const int cj = L.code[j];
                if (cj == GEO_NONE) continue;
                double d;
                const int order = geo_pair_order(L, xi, yi, zi, ci, j, cj, d);
                deg += order > 0;
                order_sum += order;
            }
        }
        deg_up[(size_t)(l0 + i)] = deg;
        n_bonds += deg;
    }
    if (n_bonds) { atomicAdd(&scount[0], n_bonds); atomicAdd(&scount[1], order_sum); }
    __syncthreads();

    // ---- components: rounds of hook + jump until a round changes nothing; at most nl rounds (see above) --------------------------------
    const bool any_bond = scount[0] > 0;                 // (uniform: read after the barrier, written before it)
    for (int round = 0; any_bond && round < nl; ++round) {
        if (k == 0) schanged = 0;
        __syncthreads();
        for (int i = k; i < nl; i += GEO_THREADS) {
            const int ci = L.code[i];
            if (ci == GEO_NONE) continue;
            const double xi = (double)L.x[i], yi = (double)L.y[i], zi = (double)L.z[i];
            const int li = lds_load(&slabel[i]);
            int m = li;
            for (int j = 0; j < nl; ++j) {
                const int cj = L.code[j];
                if (j == i || cj == GEO_NONE) continue;
                double d;
                if (geo_pair_order(L, xi, yi, zi, ci, j, cj, d) > 0) m = min(m, lds_load(&slabel[j]));
            }
            if (m < li) {
                atomicMin(&slabel[i], m);
                atomicMin(&slabel[li], m);
                schanged = 1;
            }
        }
        __syncthreads();
        if (!schanged) break;                            // (uniform; thread 0 resets it only after the barrier below)
        for (int i = k; i < nl; i += GEO_THREADS) {
            int l = lds_load(&slabel[i]);
            for (int next = lds_load(&slabel[l]); next < l; next = lds_load(&slabel[l])) l = next;
            slabel[i] = l;                               // (only this thread writes label[i] in this phase; roots stay roots)
        }
        __syncthreads();
    }

    // ---- labels, counts ----------------------------------------------------------------------------------------------------------------
    int n_roots = 0;
    for (int i = k; i < nl; i += GEO_THREADS) {
        const int l = slabel[i];
        fragment[(size_t)(l0 + i)] = l;
        n_roots += l == i;
        atomicAdd(&ssize[l], 1);
    }
    if (n_roots) atomicAdd(&scount[2], n_roots);
    __syncthreads();
    int largest = 0;
    for (int i = k; i < nl; i += GEO_THREADS) largest = max(largest, ssize[i]);
    if (largest) atomicMax(&scount[3], largest);
    __syncthreads();
    if (k == 0) {
        int32_t* o = graph_out + (size_t)CBGX_BONDS_GRAPH_COLS * g;
        o[0] = nl; o[1] = scount[0]; o[2] = scount[1]; o[3] = scount[2]; o[4] = scount[3]; o[5] = scount[0] - nl + scount[2];
    }
}

__global__ __launch_bounds__(GEO_THREADS) void ligand_bonds_fill_kernel(
    const float* __restrict__ x_lig, const uint8_t* __restrict__ z_lig, const int32_t* __restrict__ lig_ptr, int n_lig,
    const int32_t* __restrict__ bond_ptr, int n_bonds, int32_t* __restrict__ bond_index, uint8_t* __restrict__ bond_order,
    double* __restrict__ bond_length) {
    __shared__ GeoLigand L;
    const int g = blockIdx.x, k = threadIdx.x;
    int l0;
    const int nl = geo_stage_ligand(L, x_lig, z_lig, lig_ptr, n_lig, g, k, l0);
    __syncthreads();
    for (int i = k; i < nl; i += GEO_THREADS) {
        const int ci = L.code[i];
        if (ci == GEO_NONE) continue;
        // the atom's slots, clamped to the lists: a wrong bond_ptr loses bonds, it does not reach outside the buffers
        const int b0 = min(max(bond_ptr[l0 + i], 0), n_bonds), b1 = min(max(bond_ptr[l0 + i + 1], b0), n_bonds);
        int b = b0;
        const double xi = (double)L.x[i], yi = (double)L.y[i], zi = (double)L.z[i];
        for (int j = i + 1; j < nl && b < b1; ++j) {
            const int cj = L.code[j];
            if (cj == GEO_NONE) continue;
            double d;
            const int order = geo_pair_order(L, xi, yi, zi, ci, j, cj, d);
            if (order == 0) continue;
            bond_index[b] = l0 + i;
            bond_index[(size_t)n_bonds + b] = l0 + j;
            bond_order[b] = (uint8_t)order;
            bond_length[b] = d;
            ++b;
        }
    }
}

hipError_t launch_ligand_bonds_count(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs,
                                     int32_t* deg_up, int32_t* fragment, int32_t* graph_out, hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    hipLaunchKernelGGL(ligand_bonds_count_kernel, dim3(n_graphs), dim3(GEO_THREADS), 0, s, x_lig, z_lig, lig_ptr, n_lig, deg_up, fragment,
                       graph_out);
    return hipGetLastError();
}

hipError_t launch_ligand_bonds_fill(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs,
                                    const int32_t* bond_ptr, int n_bonds, int32_t* bond_index, uint8_t* bond_order, double* bond_length,
                                    hipStream_t s) {
    if (n_graphs == 0 || n_bonds == 0) return hipSuccess;
    hipLaunchKernelGGL(ligand_bonds_fill_kernel, dim3(n_graphs), dim3(GEO_THREADS), 0, s, x_lig, z_lig, lig_ptr, n_lig, bond_ptr, n_bonds,
                       bond_index, bond_order, bond_length);
    return hipGetLastError();
}

void ligand_geometry_tables(int32_t* bond_pm, int32_t* margins, int32_t* allowed, uint8_t* elements, uint8_t* vdw_z, double* vdw_r,
                            double* tolerance) {
    for (int o = 0; o < 3; ++o) {
        if (margins) margins[o] = h_geo.margin[o];
        for (int p = 0; bond_pm && p < GEO_EL * GEO_EL; ++p) bond_pm[o * GEO_EL * GEO_EL + p] = h_geo.bond_pm[o][p / GEO_EL][p % GEO_EL];
    }
    for (int c = 0; c < GEO_EL; ++c) {
        if (allowed) allowed[c] = h_geo.allowed[c];
        if (elements) elements[c] = h_geo.z[c];
    }
    for (int c = 0; c < GEO_VDW; ++c) {
        if (vdw_z) vdw_z[c] = h_geo.z[c];
        if (vdw_r) vdw_r[c] = h_geo.radius[c];
    }
    if (tolerance) *tolerance = h_geo.tolerance;
}

}  // namespace cbgx

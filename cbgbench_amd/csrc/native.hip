// libcbgx -- the samples of a pocket AGAINST the ligand the pocket was crystallised with (cbgx_pocket_contacts, cbgx_native_compare; the
// definitions are in include/cbgx.h): which pocket atoms a ligand touches and where it sits, and per sample the fingerprint similarity
// to the native ligand, the overlap of the two contact sets and the distance of the two centroids.  The reference compares scores only
// (evaluate_scripts/cal_chem_results.py, calculate_vina_metrics: host arithmetic on the scores of cbgx_ligand_interactions); the contact
// set and the centroid are descriptors of this library's own.
//
// pocket_contacts_kernel
//   shape     one 256-thread workgroup per graph, as ligand_geometry_kernel: the ligand (at most NC_MAX atoms: the host entry refuses
//             more, and the kernel clamps) is staged in LDS, the pocket atoms are streamed, one per thread and round.  A thread walks the
//             WHOLE ligand for its pocket atom, because every ligand atom it touches is marked too (an LDS integer OR: order-free).
//   distance  geo_dist2 of geo_tables.h with contraction off for this translation unit, as geometry.hip: three differences, three
//             products, two sums, each rounded once.
//   centroid  lanes 0, 1, 2 of the workgroup sum one component each over the staged heavy atoms in atom order: the sequential sum of the
//             header, not a tree.  At most 1024 dependent additions beside the other threads' pocket work.
//   counts    integer reductions over the workgroup.
// native_compare_kernel
//   shape     one 256-thread workgroup per pocket, ONE WAVE per sample and round: lanes 0 ... 31 take a word of the two fingerprints,
//             all 64 lanes walk the two contact rows, a butterfly of __shfl_xor adds the four counts.  Lane 0 of a wave writes the sample's
//             row and keeps the wave's share of the group's sums, which meet in LDS at the end.  No limit on the group: a wave loops.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cbgx.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "geo_tables.h"      // GEO_MAX, geo_dist2

namespace cbgx {

constexpr int NC_THREADS = 256;
constexpr int NC_WAVES = NC_THREADS / 64;
constexpr int NC_MAX = GEO_MAX;

struct ContactsGraph {                                       // a graph in LDS: 17 KiB
    float x[NC_MAX], y[NC_MAX], z[NC_MAX];
    int hit[NC_MAX];                                         // 1: a heavy pocket atom is in contact
    uint8_t heavy[NC_MAX];
    int n_rec_contact[NC_WAVES], n_lig_contact[NC_WAVES], n_heavy[NC_WAVES];
};

__device__ __forceinline__ int nc_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(NC_THREADS) void pocket_contacts_kernel(
    const float* __restrict__ x_lig, const uint8_t* __restrict__ z_lig, const int32_t* __restrict__ lig_ptr, int n_lig,
    const float* __restrict__ x_rec, const uint8_t* __restrict__ z_rec, const int32_t* __restrict__ rec_ptr, int n_rec, double cutoff2,
    uint8_t* __restrict__ rec_contact, uint8_t* __restrict__ lig_contact, double* __restrict__ centroid, int32_t* __restrict__ graph_out) {
    __shared__ ContactsGraph L;
    const int g = blockIdx.x, k = threadIdx.x, wave = k >> 6;
    // both ranges clamped to their arrays, and the ligand to the LDS it is staged in, as ligand_geometry_kernel does
    const int r0 = min(max(rec_ptr[g], 0), n_rec), r1 = min(max(rec_ptr[g + 1], r0), n_rec);
    const int l0 = min(max(lig_ptr[g], 0), n_lig), l1 = min(max(lig_ptr[g + 1], l0), n_lig);
    const int nr = r1 - r0, nl = min(l1 - l0, NC_MAX);

    int heavy = 0;
    for (int i = k; i < nl; i += NC_THREADS) {
        const size_t a = (size_t)(l0 + i);
        L.x[i] = x_lig[3 * a + 0]; L.y[i] = x_lig[3 * a + 1]; L.z[i] = x_lig[3 * a + 2];
        const bool h = z_lig[a] != 1;
        L.heavy[i] = h; L.hit[i] = 0;
        heavy += h;
    }
    __syncthreads();

    // ---- the centroid: lane c of the first wave sums component c in atom order ---------------------------------------------------------
    double s = 0.0;
    if (k < 3) {
        const float* v = k == 0 ? L.x : (k == 1 ? L.y : L.z);
        for (int i = 0; i < nl; ++i)
            if (L.heavy[i]) s = s + (double)v[i];
    }

    // ---- pocket atoms against the ligand ----------------------------------------------------------------------------------------------------
    int rec_hits = 0;
    for (int q = k; q < nr; q += NC_THREADS) {
        const size_t a = (size_t)(r0 + q);
        bool hit = false;
        if (z_rec[a] != 1) {
            const double px = (double)x_rec[3 * a + 0], py = (double)x_rec[3 * a + 1], pz = (double)x_rec[3 * a + 2];
            for (int j = 0; j < nl; ++j) {
                if (!L.heavy[j]) continue;
                if (geo_dist2(px, py, pz, L.x[j], L.y[j], L.z[j]) <= cutoff2) {
                    hit = true;
                    atomicOr(&L.hit[j], 1);
                }
            }
        }
        rec_contact[a] = hit;
        rec_hits += hit;
    }
    __syncthreads();

    int lig_hits = 0;
    for (int i = k; i < l1 - l0; i += NC_THREADS) {          // (rows past NC_MAX: the host entry refuses them; written all the same)
        const bool hit = i < nl && L.hit[i] != 0;
        lig_contact[(size_t)(l0 + i)] = hit;
        lig_hits += hit;
    }
    rec_hits = nc_wave_sum(rec_hits); lig_hits = nc_wave_sum(lig_hits); heavy = nc_wave_sum(heavy);
    if ((k & 63) == 0) { L.n_rec_contact[wave] = rec_hits; L.n_lig_contact[wave] = lig_hits; L.n_heavy[wave] = heavy; }
    __syncthreads();
    int n_heavy = 0;
    for (int w = 0; w < NC_WAVES; ++w) n_heavy += L.n_heavy[w];
    if (k < 3) centroid[3 * (size_t)g + k] = n_heavy ? s / (double)n_heavy : __longlong_as_double(0x7FF8000000000000ll);
    if (k == 0) {
        int n_rec_contact = 0, n_lig_contact = 0;
        for (int w = 0; w < NC_WAVES; ++w) { n_rec_contact += L.n_rec_contact[w]; n_lig_contact += L.n_lig_contact[w]; }
        int32_t* o = graph_out + (size_t)CBGX_CONTACTS_GRAPH_COLS * g;
        o[0] = l1 - l0; o[1] = n_heavy; o[2] = nr; o[3] = n_rec_contact; o[4] = n_lig_contact; o[5] = n_heavy ? 0 : CBGX_CONTACTS_EMPTY;
    }
}

hipError_t launch_pocket_contacts(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, const float* x_rec,
                                  const uint8_t* z_rec, const int32_t* rec_ptr, int n_rec, int n_graphs, double cutoff2,
                                  uint8_t* rec_contact, uint8_t* lig_contact, double* centroid, int32_t* graph_out, hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    hipLaunchKernelGGL(pocket_contacts_kernel, dim3(n_graphs), dim3(NC_THREADS), 0, s, x_lig, z_lig, lig_ptr, n_lig, x_rec, z_rec, rec_ptr,
                       n_rec, cutoff2, rec_contact, lig_contact, centroid, graph_out);
    return hipGetLastError();
}

// ---- every sample of a pocket against the pocket's native ligand ------------------------------------------------------------------------------
struct NativeGroup {
    long long sim_sum[NC_WAVES], contact_sum[NC_WAVES];
    int sim_max[NC_WAVES], contact_max[NC_WAVES], n_fp[NC_WAVES], n_same[NC_WAVES], n_contact[NC_WAVES];
};

// (common 1000000 + uni / 2) / uni, 0 when uni is 0: common <= uni < 2^31
__device__ __forceinline__ long long nc_micro(int common, int uni) {
    return uni ? ((long long)common * 1000000 + uni / 2) / uni : 0;
}

__global__ __launch_bounds__(NC_THREADS) void native_compare_kernel(
    const uint32_t* __restrict__ fp, const uint64_t* __restrict__ mol_hash, const int32_t* __restrict__ fp_status,
    const uint8_t* __restrict__ rec_contact, const int32_t* __restrict__ rec_ptr, const double* __restrict__ centroid,
    const int32_t* __restrict__ contacts_status, int n_graphs, int n_rec, const uint32_t* __restrict__ fp_nat,
    const uint64_t* __restrict__ mol_hash_nat, const int32_t* __restrict__ fp_status_nat, const uint8_t* __restrict__ rec_contact_nat,
    const int32_t* __restrict__ rec_ptr_nat, const double* __restrict__ centroid_nat, const int32_t* __restrict__ contacts_status_nat,
    int n_rec_nat, const int32_t* __restrict__ group_ptr, int64_t* __restrict__ sample_out, double* __restrict__ centroid_d2,
    int64_t* __restrict__ group_out) {
    __shared__ NativeGroup L;
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int a0 = group_ptr[p], a1 = group_ptr[p + 1];
    const int g0 = min(max(a0, 0), n_graphs), g1 = min(max(a1, g0), n_graphs);
    const int q0 = min(max(rec_ptr_nat[p], 0), n_rec_nat), q1 = min(max(rec_ptr_nat[p + 1], q0), n_rec_nat);
    const bool nat_ok = fp_status_nat[p] == 0;
    const uint64_t hash_nat = mol_hash_nat[p];
    const uint32_t word_nat = lane < CBGX_FINGERPRINT_WORDS ? fp_nat[(size_t)CBGX_FINGERPRINT_WORDS * p + lane] : 0u;
    const bool nat_here = contacts_status_nat[p] == 0;
    const double cx = centroid_nat[3 * (size_t)p + 0], cy = centroid_nat[3 * (size_t)p + 1], cz = centroid_nat[3 * (size_t)p + 2];

    long long sim_sum = 0, contact_sum = 0;
    int sim_max = -1, contact_max = -1, n_fp = 0, n_same = 0, n_contact = 0;
    for (int g = g0 + wave; g < g1; g += NC_WAVES) {        // (g is the same in all lanes of a wave)
        const int r0 = min(max(rec_ptr[g], 0), n_rec), r1 = min(max(rec_ptr[g + 1], r0), n_rec);
        const bool fp_ok = nat_ok && fp_status[g] == 0, same_pocket = r1 - r0 == q1 - q0;
        int inter = 0, uni = 0, common = 0, either = 0;
        if (fp_ok && lane < CBGX_FINGERPRINT_WORDS) {
            const uint32_t w = fp[(size_t)CBGX_FINGERPRINT_WORDS * g + lane];
            inter = __popc(w & word_nat); uni = __popc(w | word_nat);
        }
        if (same_pocket)
            for (int k = lane; k < r1 - r0; k += 64) {
                const bool a = rec_contact[(size_t)r0 + k] != 0, b = rec_contact_nat[(size_t)q0 + k] != 0;
                common += a && b; either += a || b;
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            inter += __shfl_xor(inter, off); uni += __shfl_xor(uni, off);
            common += __shfl_xor(common, off); either += __shfl_xor(either, off);
        }
        if (lane == 0) {
            const long long sim = fp_ok ? nc_micro(inter, uni) : -1, jac = same_pocket ? nc_micro(common, either) : -1;
            const int same = fp_ok ? (int)(mol_hash[g] == hash_nat) : -1;
            int64_t* o = sample_out + (size_t)CBGX_NATIVE_SAMPLE_COLS * g;
            o[0] = sim; o[1] = same; o[2] = same_pocket ? common : -1; o[3] = same_pocket ? either : -1; o[4] = jac;
            o[5] = (fp_status[g] != 0 ? CBGX_NATIVE_SAMPLE_NOT_EVALUATED : 0) | (nat_ok ? 0 : CBGX_NATIVE_NATIVE_NOT_EVALUATED) |
                   (same_pocket ? 0 : CBGX_NATIVE_POCKET_MISMATCH);
            double d2 = __longlong_as_double(0x7FF8000000000000ll);
            if (nat_here && contacts_status[g] == 0) {
                const double dx = centroid[3 * (size_t)g + 0] - cx, dy = centroid[3 * (size_t)g + 1] - cy, dz = centroid[3 * (size_t)g + 2] - cz;
                const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
                d2 = (xx + yy) + zz;
            }
            centroid_d2[g] = d2;
            if (fp_ok) { sim_sum += sim; sim_max = max(sim_max, (int)sim); ++n_fp; n_same += same; }
            if (same_pocket) { contact_sum += jac; contact_max = max(contact_max, (int)jac); ++n_contact; }
        }
    }
    if (lane == 0) {
        L.sim_sum[wave] = sim_sum; L.contact_sum[wave] = contact_sum; L.sim_max[wave] = sim_max; L.contact_max[wave] = contact_max;
        L.n_fp[wave] = n_fp; L.n_same[wave] = n_same; L.n_contact[wave] = n_contact;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NC_WAVES; ++w) {
            sim_sum += L.sim_sum[w]; contact_sum += L.contact_sum[w]; sim_max = max(sim_max, L.sim_max[w]);
            contact_max = max(contact_max, L.contact_max[w]); n_fp += L.n_fp[w]; n_same += L.n_same[w]; n_contact += L.n_contact[w];
        }
        int64_t* o = group_out + (size_t)CBGX_NATIVE_GROUP_COLS * p;
        o[0] = g1 - g0; o[1] = n_fp; o[2] = n_same; o[3] = sim_sum; o[4] = sim_max; o[5] = n_contact; o[6] = contact_sum; o[7] = contact_max;
        o[8] = (nat_ok ? 0 : CBGX_NATIVE_NATIVE_NOT_EVALUATED) | ((a0 != g0 || a1 != g1) ? CBGX_NATIVE_BAD_GROUPS : 0);
    }
}

hipError_t launch_native_compare(const uint32_t* fp, const uint64_t* mol_hash, const int32_t* fp_status, const uint8_t* rec_contact,
                                 const int32_t* rec_ptr, const double* centroid, const int32_t* contacts_status, int n_graphs, int n_rec,
                                 const uint32_t* fp_nat, const uint64_t* mol_hash_nat, const int32_t* fp_status_nat,
                                 const uint8_t* rec_contact_nat, const int32_t* rec_ptr_nat, const double* centroid_nat,
                                 const int32_t* contacts_status_nat, int n_groups, int n_rec_nat, const int32_t* group_ptr,
                                 int64_t* sample_out, double* centroid_d2, int64_t* group_out, hipStream_t s) {
    if (n_groups == 0) return hipSuccess;
    hipLaunchKernelGGL(native_compare_kernel, dim3(n_groups), dim3(NC_THREADS), 0, s, fp, mol_hash, fp_status, rec_contact, rec_ptr, centroid,
                       contacts_status, n_graphs, n_rec, fp_nat, mol_hash_nat, fp_status_nat, rec_contact_nat, rec_ptr_nat, centroid_nat,
                       contacts_status_nat, n_rec_nat, group_ptr, sample_out, centroid_d2, group_out);
    return hipGetLastError();
}

}  // namespace cbgx

// libcbgx -- distributions of a batch of sampled ligands (include/cbgx.h: cbgx_ligand_pair_hist, cbgx_ligand_angles): the pair-distance
// histograms and the bond angles of the reference's geometry report (repo/tools/geometry/eval_bond_length.py:77-84, 119-129;
// eval_bond_angle.py:69-96), one 256-thread workgroup per graph, the ligand staged in LDS as in geometry.hip.
//   distance  as geometry.hip: fp32 widened to fp64, s = (dx dx + dy dy) + dz dz, d = sqrt(s) correctly rounded, contraction OFF.
//   pairs     the n (n - 1) / 2 pairs i < j in row-major order are cut into 256 equal runs: a thread unranks the first pair of its run
//             once (a float guess corrected by integer comparisons) and walks on from there, so the work is even whatever n is -- the
//             triangular row walk would give thread 0 n - 1 pairs and the last thread none.  Bins go to an LDS integer histogram
//             (atomicAdd on LDS ints: order-independent) and are written out densely.  The bin is found by a binary search over the
//             staged edges for the number of edges strictly less than d: exact at a distance equal to an edge too.
//   angles    a centre's partners are a range of the symmetric adjacency; its angles are the pairs (p, q), p < q, of positions in
//             that range, in row-major order, from the centre's slot on.  The numbers of angles per centre are prefix-summed in LDS and
//             the graph's angles are dealt to the threads round-robin over that flat index (a binary search over the prefix finds the
//             centre, the unranking above the pair), so one high-degree centre does not serialise a wave.  The cosine is compared with
//             a cosine table: no inverse trigonometric function runs here.
//   clamping  every range read from lig_ptr, adj_ptr and angle_ptr is clamped to its array and made non-decreasing; every neighbour row
//             is checked against the graph's atom range before it is used; the flat index only covers slots inside a centre's clamped
//             slot range.  No content of the inputs makes a kernel read or write outside the buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cbgx.h"
#include "kernels.h"

#pragma clang fp contract(off)

#include "geo_tables.h"

namespace cbgx {

constexpr int DIST_BINS = 256;                          // rows of an LDS histogram: CBGX_PAIR_HIST_MAX_EDGES + 1
constexpr int DIST_PER_THREAD = GEO_MAX / GEO_THREADS;  // centres a thread owns in the prefix sum
static_assert(CBGX_PAIR_HIST_MAX_EDGES + 1 <= DIST_BINS && CBGX_ANGLES_MAX_EDGES < CBGX_ANGLE_BIN_DEGENERATE, "bins fit their types");
static_assert(GEO_MAX % GEO_THREADS == 0, "the prefix sum gives every thread the same number of centres");

// element code of an atomic number (0 ... 7 = H C N O F P S Cl), GEO_NONE when it has none: the table of geometry.hip, folded into compares
__device__ __forceinline__ int dist_code(uint8_t z) {
    constexpr GeoTables T = make_geo_tables();
    int code = GEO_NONE;
#pragma unroll
    for (int c = 0; c < GEO_EL; ++c)
        if (T.z[c] == z) code = c;
    return code;
}

// the number of pairs (i, j), i < j < n, in front of row i in row-major order
__device__ __forceinline__ int tri_offset(int i, int n) { return (i * (2 * n - i - 1)) >> 1; }

// row i of pair number p (0 <= p < n (n - 1) / 2, 2 <= n <= GEO_MAX): a float guess, made exact by integer comparisons
__device__ __forceinline__ int tri_row(int p, int n) {
    const float b = (float)(2 * n - 1);
    int i = (int)(0.5f * (b - sqrtf(fmaxf(b * b - 8.0f * (float)p, 0.0f))));
    i = min(max(i, 0), n - 2);
    while (i > 0 && tri_offset(i, n) > p) --i;
    while (i < n - 2 && tri_offset(i + 1, n) <= p) ++i;
    return i;
}

// the number of the `n` ascending edges that are strictly less than d (0 for a d that is not a number)
__device__ __forceinline__ int bin_ascending(const double* edges, int n, double d) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid] < d) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(GEO_THREADS) void ligand_pair_hist_kernel(
    const float* __restrict__ x_lig, const uint8_t* __restrict__ z_lig, const int32_t* __restrict__ lig_ptr, int n_lig,
    const double* __restrict__ edges_all, int n_all, const double* __restrict__ edges_cc, int n_cc, int32_t* __restrict__ pair_hist) {
    __shared__ float sx[GEO_MAX], sy[GEO_MAX], sz[GEO_MAX];
    __shared__ uint8_t scarbon[GEO_MAX];
    __shared__ double sedge[2][DIST_BINS];
    __shared__ int shist[2][DIST_BINS];
    const int g = blockIdx.x, k = threadIdx.x;
    const int l0 = min(max(lig_ptr[g], 0), n_lig), l1 = min(max(lig_ptr[g + 1], l0), n_lig);
    const int nl = min(l1 - l0, GEO_MAX);
    n_all = min(max(n_all, 0), CBGX_PAIR_HIST_MAX_EDGES);
    n_cc = min(max(n_cc, 0), CBGX_PAIR_HIST_MAX_EDGES);
    for (int i = k; i < nl; i += GEO_THREADS) {
        const size_t a = (size_t)(l0 + i);
        sx[i] = x_lig[3 * a + 0]; sy[i] = x_lig[3 * a + 1]; sz[i] = x_lig[3 * a + 2];
        scarbon[i] = dist_code(z_lig[a]) == EL_C;
    }
    for (int e = k; e < DIST_BINS; e += GEO_THREADS) {
        sedge[0][e] = e < n_all ? edges_all[e] : 0.0;
        sedge[1][e] = e < n_cc ? edges_cc[e] : 0.0;
        shist[0][e] = 0; shist[1][e] = 0;
    }
    __syncthreads();

    const int n_pairs = (nl * (nl - 1)) >> 1;                    // (<= 523 776)
    const int run = (n_pairs + GEO_THREADS - 1) / GEO_THREADS;
    const int p0 = min(k * run, n_pairs), p1 = min(p0 + run, n_pairs);
    if (p0 < p1) {
        const double last_all = n_all ? sedge[0][n_all - 1] : 0.0, last_cc = n_cc ? sedge[1][n_cc - 1] : 0.0;
        int i = tri_row(p0, nl);
        int j = i + 1 + (p0 - tri_offset(i, nl));
        double xi = (double)sx[i], yi = (double)sy[i], zi = (double)sz[i];
        for (int p = p0; p < p1; ++p) {
            const double d = __dsqrt_rn(geo_dist2(xi, yi, zi, sx[j], sy[j], sz[j]));
            if (n_all && d < last_all) atomicAdd(&shist[0][bin_ascending(sedge[0], n_all, d)], 1);
            if (n_cc && scarbon[i] && scarbon[j] && d < last_cc) atomicAdd(&shist[1][bin_ascending(sedge[1], n_cc, d)], 1);
            if (++j == nl) {
                ++i; j = i + 1;                                  // (the last pair is (nl - 2, nl - 1): i stays below nl - 1 while p < p1)
                if (p + 1 < p1) { xi = (double)sx[i]; yi = (double)sy[i]; zi = (double)sz[i]; }
            }
        }
    }
    __syncthreads();
    const int cols = max(n_all, n_cc) + 1;                       // (<= DIST_BINS)
    int32_t* o = pair_hist + (size_t)g * 2 * cols;
    for (int e = k; e < 2 * cols; e += GEO_THREADS) o[e] = shist[e / cols][e % cols];
}

hipError_t launch_ligand_pair_hist(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs,
                                   const double* edges_all, int n_edges_all, const double* edges_cc, int n_edges_cc, int32_t* pair_hist,
                                   hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    hipLaunchKernelGGL(ligand_pair_hist_kernel, dim3(n_graphs), dim3(GEO_THREADS), 0, s, x_lig, z_lig, lig_ptr, n_lig, edges_all,
                       n_edges_all, edges_cc, n_edges_cc, pair_hist);
    return hipGetLastError();
}

// ---- bond angles ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GEO_THREADS) void ligand_angles_kernel(
    const float* __restrict__ x_lig, const uint8_t* __restrict__ z_lig, const int32_t* __restrict__ lig_ptr, int n_lig,
    const int32_t* __restrict__ adj_ptr, const int32_t* __restrict__ adj_nbr, const uint8_t* __restrict__ adj_order, int n_adj,
    const int32_t* __restrict__ angle_ptr, int n_angles, const double* __restrict__ cos_edges, int n_edges,
    int32_t* __restrict__ angle_index, double* __restrict__ angle_cos, uint8_t* __restrict__ angle_bin, int16_t* __restrict__ angle_type) {
    __shared__ float sx[GEO_MAX], sy[GEO_MAX], sz[GEO_MAX];
    __shared__ uint8_t scode[GEO_MAX];
    __shared__ double sedge[DIST_BINS];
    __shared__ int sadj[GEO_MAX];            // first adjacency entry of a centre
    __shared__ int sdeg[GEO_MAX];            // its number of partners (0 when it has no angle to write)
    __shared__ int sslot[GEO_MAX];           // its first slot
    __shared__ int sfirst[GEO_MAX + 1];      // exclusive prefix sum of the angles the centres write
    __shared__ int spart[2][GEO_THREADS];
    __shared__ int sall[2];                  // the graph's number of angles by its adjacency; a centre above the limit on its own
    const int g = blockIdx.x, k = threadIdx.x;
    const int l0 = min(max(lig_ptr[g], 0), n_lig), l1 = min(max(lig_ptr[g + 1], l0), n_lig);
    const int nl = min(l1 - l0, GEO_MAX);
    n_edges = min(max(n_edges, 0), CBGX_ANGLES_MAX_EDGES);
    for (int i = k; i < nl; i += GEO_THREADS) {
        const size_t a = (size_t)(l0 + i);
        sx[i] = x_lig[3 * a + 0]; sy[i] = x_lig[3 * a + 1]; sz[i] = x_lig[3 * a + 2];
        scode[i] = (uint8_t)dist_code(z_lig[a]);
    }
    for (int e = k; e < n_edges; e += GEO_THREADS) sedge[e] = cos_edges[e];
    if (k < 2) sall[k] = 0;
    __syncthreads();

    // ---- the centres' ranges and counts; thread k owns centres DIST_PER_THREAD k ... ------------------------------------------------
    int mine[DIST_PER_THREAD], sum = 0;
#pragma unroll
    for (int m = 0; m < DIST_PER_THREAD; ++m) {
        const int i = DIST_PER_THREAD * k + m;
        mine[m] = 0;
        if (i >= nl) continue;
        const int e0 = min(max(adj_ptr[l0 + i], 0), n_adj), e1 = min(max(adj_ptr[l0 + i + 1], e0), n_adj);
        const int s0 = min(max(angle_ptr[l0 + i], 0), n_angles), s1 = min(max(angle_ptr[l0 + i + 1], s0), n_angles);
        const int64_t deg = e1 - e0, full = (deg * (deg - 1)) >> 1;
        int count = 0;
        if (full > CBGX_ANGLES_MAX_PER_GRAPH) atomicOr(&sall[1], 1);
        else if (full > 0) { atomicAdd(&sall[0], (int)full); count = min((int)full, s1 - s0); }     // (sum <= 1024 * 16384)
        sadj[i] = e0; sdeg[i] = count ? (int)deg : 0; sslot[i] = s0;
        mine[m] = count;
        sum += count;
    }
    spart[0][k] = sum;
    __syncthreads();
    int cur = 0;
    for (int step = 1; step < GEO_THREADS; step <<= 1, cur ^= 1) {      // inclusive scan of the threads' sums, double-buffered
        spart[cur ^ 1][k] = spart[cur][k] + (k >= step ? spart[cur][k - step] : 0);
        __syncthreads();
    }
    int first = spart[cur][k] - sum;
#pragma unroll
    for (int m = 0; m < DIST_PER_THREAD; ++m) {
        const int i = DIST_PER_THREAD * k + m;
        if (i < nl) sfirst[i] = first;
        first += mine[m];
    }
    if (k == GEO_THREADS - 1) sfirst[nl] = spart[cur][k];               // (centres >= nl count 0: the last thread's sum is the total)
    __syncthreads();
    const int total = sfirst[nl];
    if (sall[1] || sall[0] > CBGX_ANGLES_MAX_PER_GRAPH) return;         // (uniform) over the limit: nothing is written

    // ---- the angles, round-robin over the flat index ---------------------------------------------------------------------------------
    for (int t = k; t < total; t += GEO_THREADS) {
        int lo = 0, hi = nl;                                             // the last centre c with sfirst[c] <= t: it has an angle t
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (sfirst[mid] <= t) lo = mid; else hi = mid;
        }
        const int c = lo, r = t - sfirst[c], deg = sdeg[c];              // (r < count <= C(deg, 2), 2 <= deg <= 181)
        if (deg < 2) continue;
        const int p = tri_row(r, deg), q = p + 1 + (r - tri_offset(p, deg));
        if (q >= deg) continue;
        const int ea = sadj[c] + p, eb = sadj[c] + q;                    // (< sadj[c] + deg <= n_adj)
        const int ra = adj_nbr[ea], rb = adj_nbr[eb];
        if (ra < l0 || ra >= l0 + nl || rb < l0 || rb >= l0 + nl) continue;
        const int a = ra - l0, b = rb - l0;
        const int ca = scode[a], cc = scode[c], cb = scode[b];
        if (ca == GEO_NONE || cc == GEO_NONE || cb == GEO_NONE) continue;
        const int oa = min(max((int)adj_order[ea], 1), 3) - 1, ob = min(max((int)adj_order[eb], 1), 3) - 1;

        const double xc = (double)sx[c], yc = (double)sy[c], zc = (double)sz[c];
        const double ux = (double)sx[a] - xc, uy = (double)sy[a] - yc, uz = (double)sz[a] - zc;
        const double vx = (double)sx[b] - xc, vy = (double)sy[b] - yc, vz = (double)sz[b] - zc;
        const double dxx = ux * vx, dyy = uy * vy, dzz = uz * vz;
        const double dot = (dxx + dyy) + dzz;
        const double uxx = ux * ux, uyy = uy * uy, uzz = uz * uz;
        const double su = (uxx + uyy) + uzz;
        const double vxx = vx * vx, vyy = vy * vy, vzz = vz * vz;
        const double sv = (vxx + vyy) + vzz;
        const double prod = su * sv;
        double cs = dot / __dsqrt_rn(prod);
        int bin = CBGX_ANGLE_BIN_DEGENERATE;
        if (prod == 0.0 || cs != cs) {
            cs = __longlong_as_double(0x7ff8000000000000ll);
        } else {
            cs = cs < -1.0 ? -1.0 : (cs > 1.0 ? 1.0 : cs);
            int blo = 0, bhi = n_edges;                                  // the number of entries strictly greater than cs
            while (blo < bhi) {
                const int mid = (blo + bhi) >> 1;
                if (sedge[mid] > cs) blo = mid + 1; else bhi = mid;
            }
            bin = blo;
        }
        const bool swap = ca > cb || (ca == cb && oa > ob);              // the smaller (code, order) end first
        const int c1 = swap ? cb : ca, o1 = swap ? ob : oa, c2 = swap ? ca : cb, o2 = swap ? oa : ob;
        const int type = (((c1 * 3 + o1) * 8 + cc) * 3 + o2) * 8 + c2;

        const size_t slot = (size_t)(sslot[c] + r);                      // (< s0 + (s1 - s0) <= n_angles)
        angle_index[slot] = ra;
        angle_index[(size_t)n_angles + slot] = l0 + c;
        angle_index[2 * (size_t)n_angles + slot] = rb;
        angle_cos[slot] = cs;
        angle_bin[slot] = (uint8_t)bin;
        angle_type[slot] = (int16_t)type;
    }
}

hipError_t launch_ligand_angles(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs,
                                const int32_t* adj_ptr, const int32_t* adj_nbr, const uint8_t* adj_order, int n_adj,
                                const int32_t* angle_ptr, int n_angles, const double* cos_edges, int n_cos_edges, int32_t* angle_index,
                                double* angle_cos, uint8_t* angle_bin, int16_t* angle_type, hipStream_t s) {
    if (n_graphs == 0 || n_angles == 0) return hipSuccess;
    hipLaunchKernelGGL(ligand_angles_kernel, dim3(n_graphs), dim3(GEO_THREADS), 0, s, x_lig, z_lig, lig_ptr, n_lig, adj_ptr, adj_nbr,
                       adj_order, n_adj, angle_ptr, n_angles, cos_edges, n_cos_edges, angle_index, angle_cos, angle_bin, angle_type);
    return hipGetLastError();
}

}  // namespace cbgx

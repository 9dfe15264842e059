// libcbgx -- fused x2h / h2x edge kernels on the gfx950 matrix cores (v_mfma_f32_16x16x4_f32, exact fp32).
//
// One wavefront owns one destination node i and its <= 32 incoming edges; a persistent 8-wave workgroup
// keeps the layer's rbf weight fragments (and, for x2h, the second v Linear) in LDS and loops over nodes.
//
//   pre[e][m] = PD[i][m] + PS[j_e][m] + dWt[e][m] + sum_g Wr[type_e][g][m] rbf_g(|x_i - x_j|)     (k and v)
//               the rbf sum was 160 of the node's 288 fp32 MFMAs; it runs on the f16 matrix pipe in split-f16 arithmetic
//               (weights and rbf values as hi + lo f16 pairs, three products per term, fp32 accumulate: 2^-22 relative, see
//               rbf_tuples) -- 128 v_mfma_f32_16x16x16_f16 of half the issue time each, with the same LDS footprint
//   hid       = ReLU(LayerNorm(pre))
//   score[e][a] = Qt[i][a] . hid_k[e]          (the key's 2nd Linear and 1/sqrt(8) are folded into Qt)
//   alpha     = softmax over the node's incoming edges, per head
//   x2h:  S[a] = sum_e alpha e_w hid_v[e]  ->  h_out = h + Wbv_a S[a] + bbv * sum_e alpha e_w
//   h2x:  wv[e][a] = Wbv[a] . hid_v[e] + bbv[a]  ->  dx = 1/16 sum_a sum_e alpha wv e_w (x_i - x_j)
//
// Pack-time algebra that removes VALU work here (cbgx_pack_weights, node_mfma.hip):
//   * the first Linear is centred over its 128 output channels (W - colmean(W), b - mean(b)), so pre[e][:]
//     has zero mean by construction and LayerNorm only needs sum(pre^2);
//   * PD already contains the bias and the type column of a protein source, Wt[type(src prot, dst i)];
//     only ligand-source edges add dWt = Wt[type(src lig, dst i)] - Wt[type(src prot, dst i)].
//
// All contractions are MFMAs and every accumulator is consumed in the layout it was produced in (no LDS
// transposes, no atomics -> deterministic).  tests/lanesim.py is the lane-by-lane model of this file and is
// checked against the reference on the CPU (tests/test_lanesim.py).  Lane l: c = l & 15, q = l >> 4.
//   edge-major tile t    (k; h2x v): lane column = edge e16, C row rho = 4q+r <-> channel m = 16t + rho
//   channel-major tile t (x2h v):    lane column c <-> channel m = 64(t>>2) + 4c + (t&3); C row 4q+r <-> edge 4q+r+16hf
// Both labelings make every gather instruction touch whole 64..256-byte runs of a row (16 cache lines per
// wave instruction instead of 64): the texture addresser, not the ALUs, was the first bottleneck.
//
// The kernels' body (edge_body, edge_major_half, the work partition) lives in edge_body.h, shared with edge_x2h_f16.hip, which runs the
// scores and the aggregation in split-f16; this file instantiates it with that flag off and holds the pack kernels of the LDS images
// and the launchers.  What the pack kernels below and the body must agree on: the protein-only role reads its fold table
// (pack_pp_image_kernel: [t 8][d 8][lane 64][4]) as `wf + 2048 * t + 256 * d` with wf = `lds + PP_WFOLD + 4 * lane`; the h2x value
// contraction reads its 16 head rows (pack_wbv_swz_kernel) as `ld4(lds_brow + 256 * t)` with lds_brow = `lds + IMG_WBV + 4 * lane`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdlib.h>

#include <atomic>

#include "edge_common.h"
#include "kernels.h"
#include "layout.h"

namespace cbgx {


__constant__ float c_mu[G] = {0.f, 1.f, 1.25f, 1.5f, 1.75f, 2.f, 2.25f, 2.5f, 2.75f, 3.f,
                              3.5f, 4.f, 4.5f, 5.f, 5.5f, 6.f, 7.f, 8.f, 9.f, 10.f};

}  // namespace cbgx

#include "edge_body.h"

namespace cbgx {

template <bool X2H, int WAVES, bool LISTED>
__global__ __launch_bounds__(WAVES * 64) void edge_mfma_kernel(
    const float* __restrict__ att, const float* __restrict__ x, const float* __restrict__ h,
    const float* __restrict__ P, const float* __restrict__ Qt, const int32_t* __restrict__ nbr,
    const int32_t* __restrict__ deg, const uint8_t* __restrict__ lig, const uint8_t* __restrict__ gen,
    const float* __restrict__ e_w, int n_nodes, float* __restrict__ out, float* __restrict__ dx_out,
    const int* __restrict__ act, const int* __restrict__ act_count) {
    __shared__ __attribute__((aligned(16))) float lds[X2H ? (int)IMG_SIZE_X2H : (int)IMG_SIZE_H2X];
    __shared__ float lds_mu[G];
    edge_body<X2H, WAVES, LISTED, false>(lds, lds_mu, blockIdx.x, gridDim.x, att, x, h, P, Qt, nbr, deg, lig, gen, e_w, n_nodes, out,
                                         dx_out, act, act_count);
}

// x2h over TWO work lists in one launch: the protein-only destinations (`list_pp`: the node and all its neighbours are protein
// atoms; query folded in registers from q[N,128]) and the rest (`list_gen`: general kernel, folded rows from Qt[N,16,128], which
// node_qfold_kernel has produced for THESE nodes only).  The first `n_pp_wg` workgroups play the protein-only role, the others
// the general one; the split follows the list lengths (device-side counts; a general node is priced at 1.15 protein-only ones:
// mixed neighbourhoods run both source-class passes and read 8 KB of Qt) in multiples of 8 workgroups, so that a role's
// workgroup index modulo 8 is still its XCD.  One launch per layer, one LDS fill per workgroup, both lists' tails overlap.
// FULL_LAYER changes no code: the launches whose two lists together are all N nodes of a batch (the dominant kernel of the roofline)
// get their own kernel name, so that rocprofv3 --stats reports them apart from the cached / pruned layers' launches.
template <int WAVES, bool FULL_LAYER>
__global__ __launch_bounds__(WAVES * 64) void edge_x2h_dual_kernel(
    const float* __restrict__ att, const float* __restrict__ x, const float* __restrict__ h,
    const float* __restrict__ P, const float* __restrict__ Qt, const float* __restrict__ qbuf,
    const int32_t* __restrict__ nbr, const int32_t* __restrict__ deg, const uint8_t* __restrict__ lig,
    const uint8_t* __restrict__ gen, const float* __restrict__ e_w, int n_nodes, float* __restrict__ out,
    const int* __restrict__ list_pp, const int* __restrict__ count_pp, const int* __restrict__ list_gen,
    const int* __restrict__ count_gen) {
    __shared__ __attribute__((aligned(16))) float lds[IMG_SIZE_X2H];
    __shared__ float lds_mu[G];
    const int c_pp = *count_pp, c_gen = *count_gen;
    const int n_wg = gridDim.x;
    int n_pp_wg;
    // small input: both roles at `wv` nodes per workgroup, the spacing a single list of c_pp + c_gen items would get (the launcher adds
    // a workgroup for the second role's remainder): a proportional split left one role two nodes per wave, 36 instead of 27 us at one graph
    const int wv = edge_active_waves(c_pp + c_gen, n_wg > 1 ? n_wg - 1 : 1, WAVES);
    const int need_pp = (c_pp + wv - 1) / wv, need_gen = (c_gen + wv - 1) / wv;
    if (c_gen == 0) n_pp_wg = n_wg;
    else if (c_pp == 0) n_pp_wg = 0;
    else if (need_pp + need_gen <= n_wg) n_pp_wg = need_pp;
    else {
        const float share = (float)c_pp / ((float)c_pp + DUAL_GEN_COST * (float)c_gen);
        const int unit = n_wg >= 64 ? 8 : 1;
        n_pp_wg = (int)(share * (float)(n_wg / unit) + 0.5f) * unit;
        n_pp_wg = max(unit, min(n_wg - unit, n_pp_wg));
        if (n_wg < 2) n_pp_wg = 0;            // a single workgroup cannot play both roles: see the launcher (grid >= 2)
    }
    if ((int)blockIdx.x < n_pp_wg)
        edge_body<true, WAVES, true, true>(lds, lds_mu, blockIdx.x, n_pp_wg, att, x, h, P, qbuf, nbr, deg, lig, gen, e_w, n_nodes,
                                           out, nullptr, list_pp, count_pp);
    else
        edge_body<true, WAVES, true, false>(lds, lds_mu, (int)blockIdx.x - n_pp_wg, n_wg - n_pp_wg, att, x, h, P, Qt, nbr, deg, lig,
                                            gen, e_w, n_nodes, out, nullptr, list_gen, count_gen);
}

// ------------------------------------------------------------------------------------------------
// packing helpers for the LDS image
// ------------------------------------------------------------------------------------------------
// split-f16 pieces of the rbf columns of a (centred) first Linear W_a [128][340], block order [type][t] (layout.h): a weight
// w is carried as h = f16(w) (round to nearest) and l = f16(w - h)
// ---- pack kernels, one launch for all attention blocks (blockIdx.y = block; kernels.h PackBlocks) -------------------------------
// rbf table scales of a block (layout.h A_RBF_SC): per path the exponent kw that puts the largest |Wr| of all four edge types
// into [2^14, 2^15), clamped to RBF_KW_MAX; one 1024-thread workgroup per (path, block), from the CENTRED first Linears
__global__ __launch_bounds__(1024) void pack_rbf_scale_kernel(PackBlocks pb) {
    __shared__ float red[16];
    const int kv = blockIdx.x;
    float* att = pb.att[blockIdx.y];
    const float* w = att + (kv ? A_WAVC : A_WAKC);
    float mx = 0.f;
    // row m of the first Linear holds its 80 rbf columns contiguously at [m][NT .. NT + 80)
    for (int u = threadIdx.x; u < H * NT * G; u += 1024) mx = fmaxf(mx, fabsf(w[(size_t)(u / (NT * G)) * KV_IN + NT + u % (NT * G)]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 16; ++k) mx = fmaxf(mx, red[k]);
        const int E = (int)((__float_as_uint(mx) >> 23) & 0xffu);      // max in [2^(E-127), 2^(E-126))
        const int kw = max(RBF_KW_MIN, min(RBF_KW_MAX, 141 - E));
        const float S = ldexpf(1.f, kw + RBF_EXP);
        float* sc = att + A_RBF_SC + 4 * kv;
        sc[0] = S;
        sc[1] = 1.f / ((float)H * S * S);
        sc[2] = 1.f / S;
        sc[3] = (float)kw;
    }
}

// split-f16 pieces of the rbf columns of a (centred) first Linear W_a [128][340], block order [type][t] (layout.h): a weight
// w 2^kw is carried as h = f16(.) (round to nearest) and l = f16(. - h).  blockIdx.z: 0 = k table (edge-major), 1 = v table
// (x2h: channel-major B operand; h2x: edge-major), 2 = the edge-major v table of x2h blocks (training backward, A_FRAGV_EM)
__global__ void pack_frag_kernel(PackBlocks pb) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // (type*8 + t)*64 + lane
    if (idx >= NT * 8 * 64) return;
    float* att = pb.att[blockIdx.y];
    const bool x2h = pb.x2h[blockIdx.y] != 0;
    const int which = blockIdx.z;
    if (which == 2 && !x2h) return;
    const float* w_a = att + (which == 0 ? A_WAKC : A_WAVC);
    const int mode = which == 1 && x2h ? 1 : 0;
    float* dst = which == 0 ? att + A_IMG + IMG_FRAG_K : (which == 1 ? att + A_IMG + IMG_FRAG_V : att + A_FRAGV_EM);
    const int lane = idx & 63, t = (idx >> 6) & 7, type = idx >> 9;
    const int c = lane & 15, q = lane >> 4;
    const int m = mode == 0 ? 16 * t + c : 64 * (t >> 2) + 4 * c + (t & 3);
    const int kw = (int)att[A_RBF_SC + (which == 0 ? 0 : 4) + 3];
    _Float16 h[5], l[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const float w = ldexpf(w_a[(size_t)m * KV_IN + NT + G * type + 4 * s + q], kw);
        h[s] = (_Float16)w;
        l[s] = (_Float16)(w - (float)h[s]);
    }
    float* tb = dst + (size_t)type * 8 * FRAG_BLK;     // the type's 8 tiles: layout of load_wtuples (edge_common.h)
    _Float16* a0 = reinterpret_cast<_Float16*>(tb + frag_d0_index(t, lane));   // (d0, d1) = [h0 h1 h2 h3], (d2, d3) = [h4 l0 l1 l2]
    _Float16* a2 = reinterpret_cast<_Float16*>(tb + frag_d4_index(t, lane));   //  d4      = [l3 l4]
    a0[0] = h[0]; a0[1] = h[1]; a0[2] = h[2]; a0[3] = h[3];
    a0[4] = h[4]; a0[5] = l[0]; a0[6] = l[1]; a0[7] = l[2];
    a2[0] = l[3]; a2[1] = l[4];
}

// dWt[dst class lig_i][k|v][m] = Wt[type(src lig, lig_i)][m] - Wt[type(src prot, lig_i)][m]   (centred first Linears)
__global__ void pack_dwt_kernel(PackBlocks pb) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // [lig_i][kv][m]
    if (idx >= 2 * 2 * H) return;
    float* att = pb.att[blockIdx.y];
    const int m = idx & 127, kv = (idx >> 7) & 1, li = idx >> 8;
    const float* w = att + (kv ? A_WAVC : A_WAKC);
    const int tl = li ? 0 : 1, tp = li ? 2 : 3;
    att[A_IMG + IMG_WT + idx] = w[(size_t)m * KV_IN + tl] - w[(size_t)m * KV_IN + tp];
}

// x2h blocks: second v Linear [128 n][128 m] as the edge kernel's epilogue reads it: column m = 64 hh + 16 q + 4 r + j goes to
// 16-byte chunk K = 16 hh + 4 q + j, position r; the chunk index is XOR-swizzled by wbv_swizzle(head n >> 3)
__global__ void pack_wbv_swz_kernel(PackBlocks pb) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // n * 128 + m
    if (idx >= H * H) return;
    if (!pb.x2h[blockIdx.y]) {
        // h2x blocks: the 16 head rows [head][m] in the B-operand order of the value contraction (layout.h, image "wbv"):
        // lane (c = head, q) reads Wbv[c][16 t + 4 q + r] at (64 t + lane) * 4 + r
        if (idx >= HEADS * H) return;
        const int head = idx >> 7, m = idx & 127, t = m >> 4, q = (m >> 2) & 3, r = m & 3;
        pb.att[blockIdx.y][A_IMG + IMG_WBV + ((64 * t + 16 * q + head) << 2) + r] = pb.wv1[blockIdx.y][idx];
        return;
    }
    const int n = idx >> 7, m = idx & 127;
    const int chunk = 16 * (m >> 6) + 4 * ((m >> 4) & 3) + (m & 3), r = (m >> 2) & 3;
    pb.att[blockIdx.y][A_IMG + IMG_WBV + n * H + (((chunk ^ wbv_swizzle((n >> 3) & 15)) << 2) | r)] = pb.wv1[blockIdx.y][idx];
}

// x2h blocks: the LDS image of the protein-only kernel (layout.h A_IMG_PP), assembled from the general image this stream has just
// written (type-3 table slices, LayerNorm affine, swizzled second v Linear) plus the fold table of the second k Linear
__global__ void pack_pp_image_kernel(PackBlocks pb) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int)PP_IMG_SIZE || !pb.x2h[blockIdx.y]) return;
    float* att = pb.att[blockIdx.y];
    const float* img = att + A_IMG;
    float v;
    if (idx < (int)PP_FRAG_V) v = img[IMG_FRAG_K + 3 * 8 * FRAG_BLK + idx];
    else if (idx < (int)PP_LN) v = img[IMG_FRAG_V + 3 * 8 * FRAG_BLK + (idx - PP_FRAG_V)];
    else if (idx < (int)PP_WBV) v = img[IMG_LN + (idx - PP_LN)];
    else if (idx < (int)PP_WFOLD) v = img[IMG_WBV + (idx - PP_WBV)];
    else {
        const int u = idx - (int)PP_WFOLD;                      // ((t * 8 + d) * 64 + lane) * 4 + r
        const int r = u & 3, lane = (u >> 2) & 63, d = (u >> 8) & 7, t = u >> 11;
        const int c = lane & 15, q = lane >> 4;
        v = pb.wk1[blockIdx.y][(size_t)(8 * c + d) * H + 16 * t + 4 * q + r] * 0.35355339059327376220f;   // same factor as A_WBK_FRAG
    }
    att[A_IMG_PP + idx] = v;
}

// centre the first Linears of k and v over their 128 output channels: wc = w - colmean(w), bc = b - mean(b)   (w [128][340]);
// blockIdx.x = column (KV_IN -> the bias), blockIdx.y = 2 block + (k | v)
__global__ void center_linear_kernel(PackBlocks pb) {
    const int col = blockIdx.x, blk = blockIdx.y >> 1, kv = blockIdx.y & 1;
    const float* w = kv ? pb.wv0[blk] : pb.wk0[blk];
    const float* b = kv ? pb.bv0[blk] : pb.bk0[blk];
    float* wc = pb.att[blk] + (kv ? A_WAVC : A_WAKC);
    float* bc = pb.att[blk] + (kv ? A_BAVC : A_BAKC);
    __shared__ float red[128];
    const int r = threadIdx.x;
    const float v = col < KV_IN ? w[(size_t)r * KV_IN + col] : b[r];
    red[r] = v;
    __syncthreads();
    for (int o = 64; o >= 1; o >>= 1) {
        if (r < o) red[r] += red[r + o];
        __syncthreads();
    }
    const float mean = red[0] * (1.f / 128.f);
    if (col < KV_IN) wc[(size_t)r * KV_IN + col] = v - mean; else bc[r] = v - mean;
}

hipError_t launch_pack_stage1(const PackBlocks& pb, hipStream_t s) {
    if (pb.n == 0) return hipSuccess;
    hipLaunchKernelGGL(center_linear_kernel, dim3(KV_IN + 1, 2 * pb.n), dim3(128), 0, s, pb);
    return hipGetLastError();
}

hipError_t launch_pack_stage2(const PackBlocks& pb, hipStream_t s) {
    if (pb.n == 0) return hipSuccess;
    hipError_t e = launch_pack_node_tables(pb, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pack_rbf_scale_kernel, dim3(2, pb.n), dim3(1024), 0, s, pb);
    hipLaunchKernelGGL(pack_frag_kernel, dim3(NT * 8 * 64 / 256, pb.n, 3), dim3(256), 0, s, pb);
    hipLaunchKernelGGL(pack_dwt_kernel, dim3(2, pb.n), dim3(256), 0, s, pb);
    hipLaunchKernelGGL(pack_wbv_swz_kernel, dim3(H * H / 256, pb.n), dim3(256), 0, s, pb);
    hipLaunchKernelGGL(pack_pp_image_kernel, dim3((PP_IMG_SIZE + 255) / 256, pb.n), dim3(256), 0, s, pb);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_pack_h2l_image(pb, s);      // h2x blocks: the ligand-row kernel's image (edge_h2x_lig.hip), from the general one
}

// cbgx_set_edge_workgroups (include/cbgx.h): upper bound of the persistent x2h grid, 0 = one workgroup per CU
// process-wide (the one piece of library state shared between host threads): relaxed atomic, read once per launch
static std::atomic<int> g_edge_wg_limit{0};
int set_edge_workgroup_limit(int n) { return g_edge_wg_limit.exchange(n < 0 ? 0 : n, std::memory_order_relaxed); }

hipError_t launch_edge_mfma(bool x2h, const float* att, const Graph& g, const float* x, const float* h, const NodeBufs& b, float* out,
                            float* dx_out, RowList dst, hipStream_t s) {
    if (g.n_nodes == 0) return hipSuccess;
    if (!edge_offsets_fit(g.n_nodes)) return hipErrorInvalidValue;
    constexpr int W = 8;                        // waves per persistent workgroup: 2 per SIMD at <= 256 VGPRs per lane
    const int grid = edge_persistent_grid(g.n_nodes, x2h ? g_edge_wg_limit.load(std::memory_order_relaxed) : 0);
    profile_mark_begin(x2h ? (dst.rows ? K_EDGE_X2H_LISTED : K_EDGE_X2H) : K_EDGE_H2X, s);
#define CBGX_LAUNCH_EDGE(X2H_, L_)                                                                                          \
    hipLaunchKernelGGL((edge_mfma_kernel<X2H_, W, L_>), dim3(grid), dim3(W * 64), 0, s, att, x, h, b.P, b.Qt, g.nbr, g.deg, \
                       g.lig, g.gen, g.e_w, g.n_nodes, out, dx_out, dst.rows, dst.count)
    if (x2h) {
        if (dst.rows) CBGX_LAUNCH_EDGE(true, true); else CBGX_LAUNCH_EDGE(true, false);
    } else {
        if (dst.rows) CBGX_LAUNCH_EDGE(false, true); else CBGX_LAUNCH_EDGE(false, false);
    }
#undef CBGX_LAUNCH_EDGE
    profile_mark_end(s);
    return hipGetLastError();
}

// x2h edge stage over the (protein-only, general) list pair of a layer: one launch of edge_x2h_dual_kernel.  `full_layer`: the two
// lists together are all N nodes (profile class of the dominant kernel) -- otherwise a cached / pruned layer.
hipError_t launch_edge_x2h_dual(const float* att, const Graph& g, const float* x, const float* h, const NodeBufs& b, float* out,
                                RowList pp, RowList gen, bool full_layer, hipStream_t s) {
    if (g.n_nodes == 0) return hipSuccess;
    if (!edge_offsets_fit(g.n_nodes)) return hipErrorInvalidValue;
    constexpr int W = 8;
    int grid = (g.n_nodes + EDGE_MIN_WAVES - 1) / EDGE_MIN_WAVES + 1;     // + 1: each role rounds its list up to whole workgroups
    if (grid > 256) grid = 256;                 // persistent: one workgroup per CU (a multiple of 8 -> XCD-aware partition per role)
    const int wg_limit = g_edge_wg_limit.load(std::memory_order_relaxed);
    if (wg_limit >= 8 && grid > wg_limit) grid = wg_limit & ~7;
    if (grid < 2) grid = 2;                     // one workgroup per role at least
    profile_mark_begin(full_layer ? K_EDGE_X2H : K_EDGE_X2H_LISTED, s);
    // scores and aggregation on the f16 matrix pipe (edge_x2h_f16.hip) unless CBGX_X2H_F16=0 in the environment (read once per process)
    static const bool use_f16 = [] { const char* v = getenv("CBGX_X2H_F16"); return !(v && v[0] == '0' && v[1] == 0); }();
    if (use_f16)
        launch_edge_x2h_f16_grid(grid, att, g, x, h, b, out, pp, gen, full_layer, s);
    else if (full_layer)
        hipLaunchKernelGGL((edge_x2h_dual_kernel<W, true>), dim3(grid), dim3(W * 64), 0, s, att, x, h, b.P, b.Qt, b.q, g.nbr, g.deg,
                           g.lig, g.gen, g.e_w, g.n_nodes, out, pp.rows, pp.count, gen.rows, gen.count);
    else
        hipLaunchKernelGGL((edge_x2h_dual_kernel<W, false>), dim3(grid), dim3(W * 64), 0, s, att, x, h, b.P, b.Qt, b.q, g.nbr, g.deg,
                           g.lig, g.gen, g.e_w, g.n_nodes, out, pp.rows, pp.count, gen.rows, gen.count);
    profile_mark_end(s);
    return hipGetLastError();
}

}  // namespace cbgx

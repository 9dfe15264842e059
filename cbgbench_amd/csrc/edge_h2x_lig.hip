// libcbgx -- the h2x edge kernel of the inference forward for destination lists that hold ligand atoms only.
//
// Same partition, memory pipeline and arithmetic per edge as edge_mfma_kernel<false, 8, true> (edge_mfma.hip): both instantiate
// edge_body (edge_body.h).  What differs is where the score MFMAs' B operand comes from.  The general h2x kernel reads the folded query
// Qt[i][16][128] -- 8 KB per movable atom that node_qfold_kernel has written a moment before, read once.  Every destination the samplers
// hand to an h2x block is a ligand atom, so of the four edge types only 0 (lig -> lig) and 2 (prot -> lig) occur and the second v Linear
// is 16 rows: the LDS image (layout.h A_IMG_H2L, 115 KB) has room for the second k Linear as the fold table of the protein-only x2h
// role, and the lane folds its head's eight query channels q[i][8c .. 8c + 7] in registers between the rbf MFMA block and the
// LayerNorm tail of k half 0 (edge_major_half FOLD).  Qt never exists for an h2x block and its node stage ends with the query MLP
// (launch_node_mfma / add_node_stage_jobs `no_fold`).
//
// The caller promises gen_flag[i] => lig_flag[i] (include/cbgx.h CBGX_FWD_GEN_IS_LIGAND); without the promise, or with CBGX_H2X_FOLD=0
// in the environment, the general kernel runs.  This file also holds the pack kernel of the image.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdlib.h>

#include "edge_common.h"
#include "kernels.h"
#include "layout.h"

namespace cbgx {

// (a copy per translation unit: device constants have no external linkage in a non-relocatable build)
static __constant__ float c_mu[G] = {0.f, 1.f, 1.25f, 1.5f, 1.75f, 2.f, 2.25f, 2.5f, 2.75f, 3.f,
                                     3.5f, 4.f, 4.5f, 5.f, 5.5f, 6.f, 7.f, 8.f, 9.f, 10.f};

}  // namespace cbgx

#include "edge_body.h"

namespace cbgx {

template <int WAVES, bool LISTED>
__global__ __launch_bounds__(WAVES * 64) void edge_h2x_lig_kernel(
    const float* __restrict__ att, const float* __restrict__ x, const float* __restrict__ h,
    const float* __restrict__ P, const float* __restrict__ qbuf, const int32_t* __restrict__ nbr,
    const int32_t* __restrict__ deg, const uint8_t* __restrict__ lig, const uint8_t* __restrict__ gen,
    const float* __restrict__ e_w, int n_nodes, float* __restrict__ out, float* __restrict__ dx_out,
    const int* __restrict__ act, const int* __restrict__ act_count) {
    __shared__ __attribute__((aligned(16))) float lds[H2L_IMG_SIZE];
    __shared__ float lds_mu[G];
    edge_body<false, WAVES, LISTED, false, false, true>(lds, lds_mu, blockIdx.x, gridDim.x, att, x, h, P, qbuf, nbr, deg, lig, gen, e_w,
                                                        n_nodes, out, dx_out, act, act_count);
}

// h2x blocks: the image of the kernel above (layout.h A_IMG_H2L), assembled from the general image this stream has just written (type-0
// and type-2 table slices, the lig_i = 1 rows of dWt, LayerNorm affine, the 16 head rows of the second v Linear) plus the fold table of
// the block's second k Linear, in the order and with the factor of pack_pp_image_kernel (edge_mfma.hip)
__global__ void pack_h2l_image_kernel(PackBlocks pb) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int)H2L_IMG_SIZE || pb.x2h[blockIdx.y]) return;
    float* att = pb.att[blockIdx.y];
    const float* img = att + A_IMG;
    constexpr int SLOT = 8 * (int)FRAG_BLK;
    float v;
    if (idx < (int)H2L_WT) {
        const int slot = idx / SLOT, u = idx % SLOT;            // [k 0 | v 0 | k 2 | v 2]
        v = img[((slot & 1) ? IMG_FRAG_V : IMG_FRAG_K) + (size_t)(slot & 2) * SLOT + u];
    } else if (idx < (int)H2L_LN) v = img[IMG_WT + 2 * H + (idx - H2L_WT)];
    else if (idx < (int)H2L_WBV) v = img[IMG_LN + (idx - H2L_LN)];
    else if (idx < (int)H2L_WFOLD) v = img[IMG_WBV + (idx - H2L_WBV)];
    else {
        const int u = idx - (int)H2L_WFOLD;                     // ((t * 8 + d) * 64 + lane) * 4 + r
        const int r = u & 3, lane = (u >> 2) & 63, d = (u >> 8) & 7, t = u >> 11;
        const int c = lane & 15, q = lane >> 4;
        v = pb.wk1[blockIdx.y][(size_t)(8 * c + d) * H + 16 * t + 4 * q + r] * 0.35355339059327376220f;   // same factor as A_WBK_FRAG
    }
    att[A_IMG_H2L + idx] = v;
}

// after the pack kernels of the general image on the same stream (launch_pack_stage2)
hipError_t launch_pack_h2l_image(const PackBlocks& pb, hipStream_t s) {
    bool any = false;
    for (int k = 0; k < pb.n; ++k) any = any || !pb.x2h[k];
    if (!any) return hipSuccess;
    hipLaunchKernelGGL(pack_h2l_image_kernel, dim3((H2L_IMG_SIZE + 255) / 256, pb.n), dim3(256), 0, s, pb);
    return hipGetLastError();
}

// CBGX_H2X_FOLD=0 in the environment (read once per process): the h2x blocks of callers that promise ligand destinations keep the
// general kernel and the folded rows of node_qfold_kernel (A/B runs, equality tests)
bool h2x_fold_enabled() {
    static const bool on = [] { const char* v = getenv("CBGX_H2X_FOLD"); return !(v && v[0] == '0' && v[1] == 0); }();
    return on;
}

// the launch of launch_edge_mfma(false, ...) on a work list, with b.q = q[N,128] in place of Qt
hipError_t launch_edge_h2x_lig(const float* att, const Graph& g, const float* x, const float* h, const NodeBufs& b, float* out,
                               float* dx_out, RowList dst, hipStream_t s) {
    if (g.n_nodes == 0) return hipSuccess;
    if (!dst.rows || !dst.count) return hipErrorInvalidValue;       // a work-list kernel
    if (!edge_offsets_fit(g.n_nodes)) return hipErrorInvalidValue;
    constexpr int W = 8;
    const int grid = edge_persistent_grid(g.n_nodes);
    profile_mark_begin(K_EDGE_H2X, s);
    hipLaunchKernelGGL((edge_h2x_lig_kernel<W, true>), dim3(grid), dim3(W * 64), 0, s, att, x, h, b.P, b.q, g.nbr, g.deg, g.lig, g.gen,
                       g.e_w, g.n_nodes, out, dx_out, dst.rows, dst.count);
    profile_mark_end(s);
    return hipGetLastError();
}

}  // namespace cbgx

// libcbgx -- the two-role x2h edge kernel of the inference forward with ALL matrix work on the f16 matrix pipe.
//
// Same roles, partition, LDS images and memory pipeline as edge_x2h_dual_kernel (edge_mfma.hip): both instantiate edge_body
// (edge_body.h).  What differs is the arithmetic of the two contractions that edge_mfma.hip runs as exact-fp32 16x16x4 MFMAs
// (128 per node, 32 cycles each, on the vector ALU's issue port):
//   scores       hid_k . Qt      48 v_mfma_f32_16x16x16_f16 per node (one K = 16 step per tile and half, hi hi + lo hi + hi lo)
//   aggregation  hid_v^T . w     48 v_mfma_f32_16x16x16_f16 per node (one K = 16 step per tile and half, three products)
// in the split-f16 scheme of the rbf pre-activation: operands scaled by exact powers of two so that their largest value sits in
// [2^14, 2^15), fp32 accumulation, the scales undone in fp32 (edge_common.h split_f16x8; edge_body.h F16 / QS).  The rbf
// pre-activation itself is unchanged.  launch_edge_x2h_dual (edge_mfma.hip) picks this kernel unless CBGX_X2H_F16=0.
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// FULL_LAYER changes no code: a kernel name of its own for the launches over all N nodes (see edge_x2h_dual_kernel)
template <int WAVES, bool FULL_LAYER>
__global__ __launch_bounds__(WAVES * 64) void edge_x2h_f16_kernel(
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
    const int n_pp_wg = dual_pp_workgroups<WAVES>(c_pp, c_gen, n_wg);
    if ((int)blockIdx.x < n_pp_wg)
        edge_body<true, WAVES, true, true, true>(lds, lds_mu, blockIdx.x, n_pp_wg, att, x, h, P, qbuf, nbr, deg, lig, gen, e_w,
                                                 n_nodes, out, nullptr, list_pp, count_pp);
    else
        edge_body<true, WAVES, true, false, true>(lds, lds_mu, (int)blockIdx.x - n_pp_wg, n_wg - n_pp_wg, att, x, h, P, Qt, nbr, deg,
                                                  lig, gen, e_w, n_nodes, out, nullptr, list_gen, count_gen);
}

// the launch itself; grid, profile marks and argument checks are launch_edge_x2h_dual's (edge_mfma.hip)
void launch_edge_x2h_f16_grid(int grid, const float* att, const Graph& g, const float* x, const float* h, const NodeBufs& b,
                              float* out, RowList pp, RowList gen, bool full_layer, hipStream_t s) {
    constexpr int W = 8;
    if (full_layer)
        hipLaunchKernelGGL((edge_x2h_f16_kernel<W, true>), dim3(grid), dim3(W * 64), 0, s, att, x, h, b.P, b.Qt, b.q, g.nbr, g.deg,
                           g.lig, g.gen, g.e_w, g.n_nodes, out, pp.rows, pp.count, gen.rows, gen.count);
    else
        hipLaunchKernelGGL((edge_x2h_f16_kernel<W, false>), dim3(grid), dim3(W * 64), 0, s, att, x, h, b.P, b.Qt, b.q, g.nbr, g.deg,
                           g.lig, g.gen, g.e_w, g.n_nodes, out, pp.rows, pp.count, gen.rows, gen.count);
}

}  // namespace cbgx

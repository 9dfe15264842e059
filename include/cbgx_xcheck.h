/* libcbgx_xcheck.so -- TEST-ONLY build of libcbgx (same sources compiled with -DCBGX_XCHECK).
 *
 * It exports everything include/cbgx.h declares plus the two functions below, and additionally contains the first-generation
 * VALU kernels (tests/xcheck/csrc/kernels_v1.hip, train_bwd_v1.hip).  Those implement the same stages as the MFMA
 * kernels of libcbgx.so with different code, which makes them an independent on-device cross-check at sizes the CPU
 * oracle cannot reach (tests/test_gpu_parity.py, tests/test_gpu_training.py).  The product library libcbgx.so contains
 * neither the switch nor those kernels. */
#ifndef CBGX_XCHECK_H
#define CBGX_XCHECK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 0 = the kernels libcbgx.so always runs, 1 = first-generation VALU kernels, 2 = as 0 but the x2h backward of the
 * second generation (one workgroup per node, train_bwd_mfma.hip) instead of train_bwd_x2h.hip.
 * Returns the previous setting (>= 0) or CBGX_E_INVALID.  Process-wide. */
int cbgx_debug_set_edge_kernel(int impl);

/* The distance gate's backward as a stage of its own: the kernels and slab reductions every training step runs, on a caller-supplied
 * de_w = dL/de_w [n_nodes][32] (device).  Writes grads[6] (dist_emb.1: net.0.weight [160][20], net.0.bias, net.1.weight, net.1.bias,
 * net.3.weight [160], net.3.bias [1]).  rows / n_rows (device; both or neither): only the listed nodes' edges are walked (de_w is zero
 * on the others).  grad_x (optional, [n_nodes][3]): the gate's dL/dx is ADDED to it.  workspace: the training workspace (include/cbgx.h). */
int cbgx_debug_gate_backward(const float* packed, const float* x, const int32_t* nbr, const int32_t* deg, int n_nodes,
                             const float* de_w, const int* rows, const int* n_rows, float* const* grads, float* grad_x,
                             void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif

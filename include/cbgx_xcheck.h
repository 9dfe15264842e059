/* libcbgx_xcheck.so -- TEST-ONLY build of libcbgx (same sources compiled with -DCBGX_XCHECK).
 *
 * It exports everything include/cbgx.h declares plus the functions below, and additionally contains the first-generation
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

/* A view into a forward workspace: where cbgx_unitransformer_forward{,_cached} of n_nodes nodes keeps the graph stage and the node
 * lists it builds on the device.  Launches nothing and reads nothing: it carves `workspace` exactly as the forward does and writes
 * CBGX_FWD_VIEW_PTRS device addresses to out[] (host memory).  Valid from the return of a forward call on that workspace (in stream
 * order) until the next call that uses it; no stage of a forward call overwrites a list once it is built.
 *   out[0] nbr [n][32] int32   out[1] deg [n] int32   out[2] e_w [n][32] float
 *   out[3] d1flag [n] bytes (the node or one of its neighbours is a ligand atom, from the call's own neighbour lists)
 *   out[4] D1 [n] bytes (proximity flags of a graph-cached call; zero otherwise)
 *   out[5 + 2 k] list k (int32 node ids, any order), out[6 + 2 k] its count (one int32), k = 0 .. CBGX_FWD_VIEW_LISTS - 1:
 *     act, A1, A2, A3, D1, S1, D2, S2, then the (general, protein-only) pairs of {all nodes, D2, A1, A2}.
 * A list the call does not need is not built and has count 0: A2, A3 and the A1 / A2 pairs without pruning (h_out given and no
 * CBGX_FWD_H_ON_SOURCES, or fewer than 3 layers), D1 .. S2 and the D2 pair without the static features. */
#define CBGX_FWD_VIEW_LISTS 16
#define CBGX_FWD_VIEW_PTRS (5 + 2 * CBGX_FWD_VIEW_LISTS)
int cbgx_debug_forward_view(void* workspace, int n_nodes, void** out);

#ifdef __cplusplus
}
#endif
#endif

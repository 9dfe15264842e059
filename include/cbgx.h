/*
 * cbgx.h -- C ABI of libcbgx.so: the MI355X (gfx950) implementation of CBGBench's
 * per-diffusion-step E(3)-equivariant message passing.
 *
 * The reference is pure Python; the natives it calls on this path are the
 * un-vendored torch_cluster / torch_scatter wheels and ATen.  Each entry point
 * below names the reference interface it replaces (paths relative to the
 * reference tree).  All pointers are DEVICE pointers unless said otherwise, all
 * float tensors are contiguous fp32 row-major, `stream` is a hipStream_t passed
 * as void* (NULL = default stream).  Every call is asynchronous on `stream`,
 * re-entrant, keeps no pointer after it returns and never frees or allocates
 * device memory: the caller owns inputs, outputs and the workspace.
 *
 * The only state the library owns, besides the optional profiling hook at the end of this file:
 * one auxiliary non-blocking HIP stream and two events per HOST THREAD AND CALLER STREAM (at most eight per thread, created on the
 * first multi-layer forward on that stream; a ninth caller stream takes over the oldest entry's stream and events -- nothing is
 * destroyed or waited for, so this is legal under stream capture; results stay correct, only the overlap of that caller's node
 * stages with its other calls is lost), and the process-wide workgroup limit of cbgx_set_edge_workgroups (a relaxed atomic int:
 * the one value shared between host threads).  cbgx_unitransformer_forward{,_cached} fork the node stage of
 * layer l+1 onto it next to the h2x block of layer l and join it back before returning work to `stream`, so
 * from the caller's point of view everything is still ordered on `stream` (hipGraph capture of `stream`
 * records the fork/join).  One device per host thread (the one-process-per-GPU model): a thread that switches
 * devices falls back to the serial schedule.  CBGX_OVERLAP=0 in the environment disables the auxiliary stream.
 *
 * Return value: 0 on success, negative CBGX_E_* on failure (never abort());
 * cbgx_last_error() gives a thread-local message.
 *
 * Arithmetic contract: inputs, outputs and accumulators are fp32.  The node projection, the query MLP's second Linear and the
 * radial-basis part of the edge pre-activation run on the f16 matrix pipe as "split-f16" products (every fp32 operand v is carried
 * as hi = f16(v 2^k), lo = f16(v 2^k - hi) with 2^k an exact power of two chosen per weight column / per table at pack time and per
 * row of activations at run time; three f16 products hi hi + hi lo + lo hi, fp32 accumulation, 2^-k applied to the fp32 result),
 * everything else on fp32 MFMA / VALU.  The result is fp32-grade over the range the scale exponents cover: error <= ~2^-21 of
 * sum |a||b| per dot product, measured 5 - 8e-8 against 1.3 - 2.5e-7 for a plain fp32 FMA chain over weight scales 1e-4 .. 30 and
 * activations 1e-3 .. 1e5 (tests/test_splitf16_range.py, tests/test_gpu_range.py; |h| > 65 504 is fine).  That is the supported and
 * tested range.  The scale exponents are clamped so that every factor stays a normal fp32 number (rbf tables: 2^-40 .. 2^20, node
 * tables 2^-100 .. 2^60, activation rows 2^-100 .. 2^100); outside of what they can compensate (rbf columns above 2^54, rows whose
 * largest entry is denormal) accuracy degrades gradually towards plain f16 -- never an error code, and finite inputs never give a
 * non-finite result because of the scaling.
 * Non-finite inputs propagate as in the reference.
 *
 * Node order (as produced by compose_context, repo/modules/common.py:189-214):
 * nodes sorted by graph; graph g owns rows [graph_ptr[g], graph_ptr[g+1]).
 */
#ifndef CBGX_H
#define CBGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: the packed-weight layout carries the power-of-two scales of the split-f16 tables (range-safe arithmetic, below); a blob
 * packed by a version-1 library is not understood by version 2 and vice versa -- re-pack with the library that consumes it.
 * 4 (round 5): cbgx_unitransformer_backward with grad_h_out == NULL also prunes the classifier head's backward to the ligand rows
 * (round 4 changed that without a bump), the cbgx_targetdiff_train_noise / _loss / _loss_backward exports exist, and the workspace
 * layout of cbgx_unitransformer_forward changed: a caller built against version 3 must not load this library. */
#define CBGX_ABI_VERSION 6

#define CBGX_OK 0
#define CBGX_E_INVALID (-1)   /* bad argument (shape, NULL pointer, unsupported hyper-parameter) */
/* Unsupported hyper-parameters -- the encoder options of unitransformer.py:17-39 that no shipped config sets and this library does not
 * implement: num_x2h / num_h2x != 1, num_blocks != 1, ew_type in {'r', 'm'} (x2h_attention.py:70-76; the 'r' branch of
 * h2x_attention.py:54 is broken in the reference), cutoff_mode in {'radius', 'hybrid'} (unitransformer.py:77,83 reference undefined
 * names there), x2h_out_fc=True (x2h_attention.py:93-94), n_heads != 16, node_feat_dim != 128, k != 32, num_r_gaussian != 20,
 * act_fn != 'relu', norm=False, and a `time:` embedding (context_emb.py:190-195).  The host mirror raises ValueError naming the option
 * (cbgbench_amd/unitransformer.py; texts pinned by tests/test_host.py), the C entry points return CBGX_E_INVALID. */
#define CBGX_E_WORKSPACE (-2) /* workspace too small */
#define CBGX_E_HIP (-3)       /* a HIP runtime call / kernel launch failed */

/* Fixed hyper-parameters of every shipped diffusion config
 * (configs/{denovo,linker,frag,scaffold,sidechain}/train/{targetdiff,diffbp,diffsbdd}.yml:3-7 and the
 * defaults at repo/modules/e3nn/unitransformer.py:17-39). The kernels are specialised for them. */
#define CBGX_HIDDEN 128
#define CBGX_HEADS 16
#define CBGX_NUM_GAUSSIANS 20
#define CBGX_KNN 32
#define CBGX_EDGE_TYPES 4
#define CBGX_GATE_HIDDEN 160
/* Largest classifier width: the head's node products hold one [128 x num_classes] weight tile per workgroup, so num_classes is
 * 1 .. CBGX_MAX_CLASSES.  cbgx_pack_weights, every cbgx_unitransformer_forward* entry point, cbgx_classifier and
 * cbgx_unitransformer_backward(_ex) return CBGX_E_INVALID for a larger value, before anything is launched
 * (cbgx_packed_weights_floats returns 0). */
#define CBGX_MAX_CLASSES 128

int cbgx_abi_version(void);
const char *cbgx_last_error(void);

/* ---- scheduling hint (changes no result) -----------------------------------------------------------------------
 * The fused x2h edge kernel is persistent: one 8-wave workgroup per CU, all registers and 150 KB of LDS, so nothing else runs
 * beside it, while the node kernels of the same call are HBM-bound and leave the matrix cores idle.  A caller that keeps TWO
 * forward calls in flight on two of its streams (two resident batches; every call gets its own auxiliary stream) can let the
 * node kernels of one call run under the edge kernel of the other by leaving a few CUs free: n = upper bound of the edge
 * kernel's workgroups (a multiple of 8; e.g. 224 of 256), 0 = default (one per CU).  Process-wide; returns the previous value.
 * cbgbench_amd.TargetDiff.sample_many / bench.py --streams 2 use it. */
int cbgx_set_edge_workgroups(int n);

/* ---- weights -------------------------------------------------------------------------------
 * The library consumes one packed fp32 blob built from the reference state_dict tensors
 * (SURVEY.md A.2 key names).  `tensors` is a HOST array of DEVICE pointers in this order:
 *   [0..5]   denoiser.dist_emb.1.net.{0.weight,0.bias,1.weight,1.bias,3.weight,3.bias}
 *   then for each layer l, 36 pointers:
 *     x2h_layers.0.hk_func.net.{0.weight,0.bias,1.weight,1.bias,3.weight,3.bias}, hv_func (6), hq_func (6),
 *     h2x_layers.0.xk_func (6), xv_func (6), xq_func (6)
 *   then classifier.{0.weight,0.bias,2.weight,2.bias}
 * i.e. 6 + 36*num_layers + 4 pointers.  Re-pack whenever the parameters change. */
size_t cbgx_packed_weights_floats(int num_layers, int num_classes);
int cbgx_pack_weights(const float *const *tensors, int num_tensors, int num_layers, int num_classes,
                      float *packed, void *stream);

/* ---- whole denoiser call ---------------------------------------------------------------------
 * Replaces UniTransformer.forward (repo/modules/e3nn/unitransformer.py:102-123) with
 * cutoff_mode='knn', k=32, ew_type='global', num_blocks=1, num_x2h=num_h2x=1, relu+LayerNorm.
 * x[N,3], h[N,128], graph_ptr[B+1] int32, lig_flag[N]/gen_flag[N] uint8 (0/1).
 * Outputs x_out[N,3], h_out[N,128], logits[N,num_classes] (logits may be NULL).
 * h_out may be NULL when the caller only consumes x_out and the logits of ligand rows (what the samplers do,
 * targetdiff.py:164-165): the last two x2h blocks are then restricted to the nodes whose features can still reach
 * those outputs (receptive-field pruning) and logits are defined on lig_flag rows only. */
size_t cbgx_workspace_bytes(int n_nodes, int n_graphs);
int cbgx_unitransformer_forward(const float *packed, int num_layers, int num_classes,
                                const float *x, const float *h, const int32_t *graph_ptr,
                                const uint8_t *lig_flag, const uint8_t *gen_flag,
                                int n_nodes, int n_graphs,
                                float *x_out, float *h_out, float *logits,
                                void *workspace, size_t workspace_bytes, void *stream);

/* Same call with a *static-context cache* for samplers, where the protein half of (x, h) is identical in every one of
 * the T denoiser calls of a run (protein atoms never move, unitransformer.py:182; no time embedding in the shipped
 * configs).  static_h1 / static_h2 [N,128]: the features leaving layer 0 / layer 1 when the same call is made on the
 * ligand-free pockets (rows of ligand atoms are ignored) -- obtain them with two cbgx_unitransformer_forward calls of
 * num_layers = 1 and 2 on the protein rows alone and scatter to the composed row order.  A protein node whose 32
 * neighbours contain no ligand atom sees exactly the ligand-free pocket in layer 0 (and, one hop further, in layer 1),
 * so those rows are copied from the cache and the first two x2h blocks run only on the rows that differ.
 * Optional graph part (all four or none; NULL = recompute): static_nbr [N,32] / static_deg [N] / static_ew [N,32] = the
 * ligand-free pockets' cbgx_knn_graph lists (in composed row numbers) and cbgx_edge_gate values, static_r32sq [N] = squared
 * distance to the last (32nd) of those neighbours, +inf where deg < 32.  A protein node whose nearest ligand atom is not
 * closer than that keeps its cached list and gate; only the others get fresh ones.  static_nbr rows must be what cbgx_knn_graph
 * writes: ids of nodes of the SAME graph in the first static_deg[i] slots, -1 in the rest (an entry outside its graph is treated as
 * padding by the list kernels; it is never dereferenced).
 * Results are bit-identical to cbgx_unitransformer_forward.  Requires num_layers >= 4 (otherwise the cache is ignored).
 * flags: CBGX_FWD_H_ON_SOURCES -- the caller reads h_out only on the rows A1 = gen_flag | lig_flag | in-neighbours of gen_flag rows
 *   (what an H2X stack run on the same coordinates reads: DiffBP's CoMPredictor, diffbp.py:79-101; pass the same rows to
 *   cbgx_h2x_stack_forward).  The last two x2h blocks are then pruned to the receptive field of those rows exactly as when
 *   h_out is NULL; rows of h_out outside A1 are left unwritten.  Without the flag h_out is defined on every row (no pruning). */
#define CBGX_FWD_H_ON_SOURCES 1u
/* CBGX_FWD_GEN_IS_LIGAND -- the caller promises gen_flag[i] != 0 => lig_flag[i] != 0 (every movable node is a ligand atom: what all
 *   samplers of this project produce).  The h2x blocks then run the ligand-row edge kernel (csrc/edge_h2x_lig.hip), which folds the
 *   query into the key's second Linear in registers; the folded rows Qt are neither written nor read for those blocks.  Same
 *   arithmetic per edge; the fold itself is eight fp32 FMAs per value in place of two 16x16x4 fp32 MFMA steps.  Without the flag, or
 *   with CBGX_H2X_FOLD=0 in the environment (read once per process), nothing changes, launches included.  A call that sets the flag
 *   on inputs that break the promise gets undefined coordinates for the offending rows (no out-of-bounds access). */
#define CBGX_FWD_GEN_IS_LIGAND 2u
/* cbgx_unitransformer_forward with `flags` (CBGX_FWD_GEN_IS_LIGAND; CBGX_FWD_H_ON_SOURCES as in the cached call) */
int cbgx_unitransformer_forward_v2(const float *packed, int num_layers, int num_classes,
                                   const float *x, const float *h, const int32_t *graph_ptr,
                                   const uint8_t *lig_flag, const uint8_t *gen_flag,
                                   int n_nodes, int n_graphs,
                                   float *x_out, float *h_out, float *logits, unsigned flags,
                                   void *workspace, size_t workspace_bytes, void *stream);
int cbgx_unitransformer_forward_cached(const float *packed, int num_layers, int num_classes,
                                       const float *x, const float *h, const int32_t *graph_ptr,
                                       const uint8_t *lig_flag, const uint8_t *gen_flag, int n_nodes, int n_graphs,
                                       const float *static_h1, const float *static_h2,
                                       const int32_t *static_nbr, const int32_t *static_deg,
                                       const float *static_ew, const float *static_r32sq,
                                       float *x_out, float *h_out, float *logits, unsigned flags,
                                       void *workspace, size_t workspace_bytes, void *stream);

/* The cached call with a *step cache*: a block of device memory owned by one sampling state, which carries the node stage of layers
 * 0 / 1 (P and q of every row) and those layers' output arrays from one denoiser call of the state to the next.  After the first call
 * on a reset block, layer 0 projects the ligand rows only (the protein rows of h do not change during a run), layer 1 the rows whose
 * layer-0 output can differ from the previous call's (D1 of this call and of the previous one), and only the rows the previous call
 * overwrote are placed again from static_h1 / static_h2.  Every output is bit-identical to cbgx_unitransformer_forward_cached.
 * The caller's promises: the protein rows of (x, h), the flags, the static context and the weights are those of the first call after
 * the reset (a state whose static context is rebuilt gets a reset block); one call at a time per block, each ordered after the previous
 * one (same stream, or an event).  Calls of other states, each with a block of its own, may run in between and beside it.
 * The block serves graph-cached calls (all four static graph arrays given) of more than 8 192 nodes; in every other call, and with
 * CBGX_STEP_CACHE=0 in the environment (read once per process), it is not touched and the launches are the cached call's.
 * cbgx_step_cache_bytes: size of the block (0: no call of n_nodes would use one -- pass NULL).  cbgx_step_cache_reset: marks every row
 * as not computed, on `stream`; nothing of an earlier run is read afterwards.  cbgx_step_cache_layout: byte offsets of the block's
 * arrays, for tests: P0 [N,640], q0 [N,128], h1 [N,128], P1, q1, h2, then the per-node flags fresh0, prevD1, prevD2. */
#define CBGX_STEP_CACHE_ARRAYS 9
size_t cbgx_step_cache_bytes(int n_nodes);
int cbgx_step_cache_reset(void *step_cache, size_t step_cache_bytes, int n_nodes, void *stream);
int cbgx_step_cache_layout(int n_nodes, size_t *offsets);
int cbgx_unitransformer_forward_step_cached(const float *packed, int num_layers, int num_classes,
                                            const float *x, const float *h, const int32_t *graph_ptr,
                                            const uint8_t *lig_flag, const uint8_t *gen_flag, int n_nodes, int n_graphs,
                                            const float *static_h1, const float *static_h2,
                                            const int32_t *static_nbr, const int32_t *static_deg,
                                            const float *static_ew, const float *static_r32sq,
                                            float *x_out, float *h_out, float *logits, unsigned flags,
                                            void *step_cache, size_t step_cache_bytes,
                                            void *workspace, size_t workspace_bytes, void *stream);

/* ---- stages (also what the parity tests call one by one) ------------------------------------- */

/* torch_cluster.knn_graph(x, k, batch, loop=False, flow='source_to_target') as called at
 * unitransformer.py:80.  nbr[N,32] int32: neighbours of centre i in ascending (squared distance,
 * index) order, -1 padded; deg[N] = min(k, n_graph-1).  Edge (src=nbr[i][s], dst=i). k must be 32. */
int cbgx_knn_graph(const float *x, const int32_t *graph_ptr, int n_graphs, int n_nodes, int k,
                   int32_t *nbr, int32_t *deg, void *stream);

/* Global distance gate, unitransformer.py:109-112 + repo/modules/embs/dist_emb.py:6-9:
 * e_w[N,32] = sigmoid(MLP_{20->160->1}(rbf(|x_i - x_nbr|))), 0 in padded slots. */
int cbgx_edge_gate(const float *packed, const float *x, const int32_t *nbr, const int32_t *deg,
                   int n_nodes, float *e_w, void *stream);

/* X2HAttention.forward, repo/modules/attention/x2h_attention.py:43-97 (includes the residual):
 * h_out = h + sum_e softmax_e(q_i.k_e/sqrt(8)) * v_e * e_w.  `layer` selects denoiser.blocks[layer]. */
int cbgx_x2h_attention(const float *packed, int layer, const float *x, const float *h,
                       const int32_t *nbr, const int32_t *deg, const uint8_t *lig_flag, const float *e_w,
                       int n_nodes, float *h_out, void *workspace, size_t workspace_bytes, void *stream);

/* H2XAttention.forward, repo/modules/attention/h2x_attention.py:34-73, plus the masked update of
 * E3DualAttentionLayer.forward (unitransformer.py:178-184): x_out = x + delta_x * gen_flag.
 * Only gen_flag nodes are computed (the others cannot move); delta_x[N,3] (may be NULL) receives the attention
 * output for gen_flag nodes and 0 elsewhere. */
int cbgx_h2x_attention(const float *packed, int layer, const float *x, const float *h,
                       const int32_t *nbr, const int32_t *deg, const uint8_t *lig_flag,
                       const uint8_t *gen_flag, const float *e_w, int n_nodes,
                       float *x_out, float *delta_x, void *workspace, size_t workspace_bytes, void *stream);
/* the same with `flags`: CBGX_FWD_GEN_IS_LIGAND (above) or 0 */
int cbgx_h2x_attention_v2(const float *packed, int layer, const float *x, const float *h,
                          const int32_t *nbr, const int32_t *deg, const uint8_t *lig_flag,
                          const uint8_t *gen_flag, const float *e_w, int n_nodes,
                          float *x_out, float *delta_x, unsigned flags, void *workspace, size_t workspace_bytes, void *stream);

/* The node stage of one attention block on its own (stage-level tests): P[N,640] = h Wn + bn (PDk | PDv | PSk | PSv | q hidden),
 * q[N,128] = the query MLP and Qt[N,16,128] = the query folded into the key's second Linear, of denoiser.blocks[layer]'s x2h
 * (x2h != 0) or h2x block.  `rows` / `n_rows` (DEVICE pointers, or both NULL): the own columns, q and Qt are produced for the rows
 * rows[0 .. *n_rows) only, the PS columns for every row.  q_direct != 0: what the inference forward runs above 8192 rows -- q
 * straight from h in one launch, the q-hidden columns P[:, 512:640) are NOT written; q_direct == 0: projection -> query MLP chain. */
int cbgx_node_stage(const float *packed, int layer, int x2h, const float *h, const uint8_t *lig_flag, int n_nodes,
                    const int32_t *rows, const int32_t *n_rows, int q_direct, float *P, float *q, float *Qt, void *stream);

/* classifier head, unitransformer.py:46-51,119-120: Linear -> softplus - ln2 -> Linear. */
int cbgx_classifier(const float *packed, int num_layers, int num_classes, const float *h, int n_nodes,
                    float *logits, void *workspace, size_t workspace_bytes, void *stream);

/* ---- a stack of H2X blocks on its own graph: DiffBP's CoMPredictor -----------------------------------
 * CoMPredictor.forward (repo/models/diffusion/diffbp.py:79-101): kNN graph + gate from x, then num_layers
 * H2XAttention blocks with x_out = x_out + delta_x * gen_flag, h fixed.  `tensors` for the pack: HOST array of
 * DEVICE pointers com_head.dist_emb.1.net.{0.weight,0.bias,1.weight,1.bias,3.weight,3.bias} followed, per layer,
 * by com_head.h2xattentions.{l}.{xk_func,xv_func,xq_func}.net.{0.weight,...,3.bias} (6 + 18*num_layers). */
size_t cbgx_packed_h2x_stack_floats(int num_layers);
int cbgx_pack_h2x_stack(const float *const *tensors, int num_tensors, int num_layers, float *packed, void *stream);
int cbgx_h2x_stack_forward(const float *packed, int num_layers, const float *x, const float *h,
                           const int32_t *graph_ptr, const uint8_t *lig_flag, const uint8_t *gen_flag,
                           int n_nodes, int n_graphs, float *x_out, void *workspace, size_t workspace_bytes,
                           void *stream);
/* the same with `flags`: CBGX_FWD_GEN_IS_LIGAND (above) or 0 */
int cbgx_h2x_stack_forward_v2(const float *packed, int num_layers, const float *x, const float *h,
                              const int32_t *graph_ptr, const uint8_t *lig_flag, const uint8_t *gen_flag,
                              int n_nodes, int n_graphs, float *x_out, unsigned flags, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ---- TargetDiff step prologue / epilogue ----------------------------------------------------------
 * The per-step work around the denoiser in TargetDiff.sample (repo/models/diffusion/targetdiff.py:150-182).
 * prologue: x[lig_rows[a]] = x_lig[a];  h[lig_rows[a]] = ligand_atom_emb(c_lig[a]) + ligand_indicator(1)
 *           (PLContextEmbedder.forward, repo/modules/context_emb.py:179-230; no time embedding in shipped configs).
 *           lig_emb_w [128,C], lig_emb_b [128], ind_w [128,1], ind_b [128] are the reference parameters
 *           context_embedder.{ligand_atom_emb,ligand_indicator}.{weight,bias}; c_lig [n_lig,C] float (one-hot).
 * epilogue: x_next = posterior sample of positions (CTNVPScheduler.backward_remove_noise 'denoise',
 *           diffusion_scheduler.py:144-165), c_next / v_next = posterior sample of atom types by Gumbel-argmax
 *           (TypeVPScheduler.backward_remove_noise, :367-378, 407-441; categorical.py:26-32); atoms with
 *           gen_lig == 0 keep position and type.  x_den [N,3] / logits [N,C] are the denoiser outputs, read at
 *           lig_rows.  `tables` = HOST array of 7 DEVICE pointers into the reference's frozen schedule tables:
 *           pos_scheduler.{posterior_mean_c0_coef, posterior_mean_ct_coef, posterior_logvar},
 *           type_scheduler.{log_alphas_v, log_one_minus_alphas_v, log_alphas_cumprod_v,
 *           log_one_minus_alphas_cumprod_v}.  t is the (batch-uniform) step index; eps ~ N(0,1) [n_lig,3] and
 *           u ~ U(0,1) [n_lig,C] are the noise draws (the reference draws randn_like then rand_like). */
int cbgx_targetdiff_prologue(const float *x_lig, const float *c_lig, const int32_t *lig_rows, int n_lig,
                             int num_classes, const float *lig_emb_w, const float *lig_emb_b, const float *ind_w,
                             const float *ind_b, float *x, float *h, void *stream);
int cbgx_targetdiff_epilogue(const float *x_den, const float *logits, const int32_t *lig_rows, const float *x_lig,
                             const float *c_lig, const uint8_t *gen_lig, int n_lig, int num_classes, int t,
                             int num_timesteps, const float *const *tables, const float *eps, const float *u,
                             float *x_next, float *c_next, int32_t *v_next, void *stream);

/* Epilogue of step t and prologue of step t - 1 in one launch (round 5): cbgx_targetdiff_epilogue's outputs x_next / c_next, and
 * in the same launch the composed rows of the NEXT denoiser call -- x[lig_rows] = x_next, h[lig_rows] = ligand_atom_emb(c_next) +
 * ligand_indicator(1) -- exactly what cbgx_targetdiff_prologue would write from (x_next, c_next).  Same arithmetic, bit for bit,
 * as the two calls it replaces (targetdiff.py:164-182 followed by :155-158 of the next iteration); x_den must not alias x. */
int cbgx_targetdiff_step_boundary(const float *x_den, const float *logits, const int32_t *lig_rows, const float *x_lig,
                                  const float *c_lig, const uint8_t *gen_lig, int n_lig, int num_classes, int t,
                                  int num_timesteps, const float *const *tables, const float *eps, const float *u,
                                  float *x_next, float *c_next, const float *lig_emb_w, const float *lig_emb_b,
                                  const float *ind_w, const float *ind_b, float *x, float *h, void *stream);

/* Trajectory-resident variants: the ligand state lives in traj_x [T+1, n_lig, 3] / traj_c [T+1, n_lig, C] (slot s+1 = the
 * state entering step s, slot 0 = the final state) and the step index in a device int (*t_dev).  The prologue reads slot
 * *t_dev + 1; the epilogue reads slot *t_dev + 1, writes slot *t_dev and then decrements *t_dev.  No argument changes
 * from step to step, so one captured hipGraph of {prologue_traj, forward, noise draw, epilogue_traj} can be replayed for
 * all T steps -- the launch-bound regime of small batches (TargetDiff.sample(..., use_graph=True)). */
int cbgx_targetdiff_prologue_traj(const float *traj_x, const float *traj_c, const int32_t *t_dev,
                                  const int32_t *lig_rows, int n_lig, int num_classes, const float *lig_emb_w,
                                  const float *lig_emb_b, const float *ind_w, const float *ind_b, float *x, float *h,
                                  void *stream);
int cbgx_targetdiff_epilogue_traj(const float *x_den, const float *logits, const int32_t *lig_rows, float *traj_x,
                                  float *traj_c, const uint8_t *gen_lig, int n_lig, int num_classes, int32_t *t_dev,
                                  const float *const *tables, const float *eps, const float *u, void *stream);

/* ---- DiffBP / DiffSBDD: the per-step arithmetic around the network calls, one launch per step -------------------
 * cbgx_diffbp_epilogue: diffbp.py:262-297 after the denoiser and the CoMPredictor stack -- zero-COM noise estimate,
 *   mean shift of the H2X stack (CoMPredictor.forward, diffbp.py:79-101), score step on the positions
 *   (CTNVPScheduler.backward_remove_noise(type='score'), diffusion_scheduler.py:154-158) and the absorbing-state type
 *   step (MaskTypeSchedule.backward_remove_noise, :475-496).  x_den / x_com / x_in: [N,3] denoiser output, H2X-stack
 *   output and their common input; lig_ptr [B+1]: ligand atoms of graph g are [lig_ptr[g], lig_ptr[g+1]) (ligand arrays are
 *   sorted by graph); tables: alphas_cumprod [T], betas [T] of the position scheduler; eps [n_lig,3], u [n_lig].
 * cbgx_diffsbdd_step: one iteration of diffsbdd.py:296-304 after the denoiser (sample_p_zs_given_zt for positions with
 *   the ligand's centre of mass removed and the pocket translated with it, and for types; diffusion_scheduler.py:1012-1040).
 *   inv_alpha, coef, sigma: 1 / alpha_ts, sigma2_ts / alpha_ts / sigma_t and sigma_ts sigma_s / sigma_t of the step.  Updates
 *   the composed x IN PLACE (pocket rows of every graph, ligand rows) and writes h on ligand rows from the new types, so
 *   that the next denoiser call needs no prologue; shift [B,3] (may be NULL) receives the removed mean per graph.
 *   frame_shift [B,3] (in / out, may be NULL) selects the FRAMED mode: the pocket rows of x are left where they are (so the
 *   static-context cache of cbgx_unitransformer_forward_cached holds for the whole run) and the translation the reference applies
 *   to the pocket is accumulated in frame_shift instead: true position = position in x - frame_shift[graph].  x_den is then the
 *   denoiser's output in the frame of x (the network is translation-equivariant), x_lig / x_next stay in true coordinates, the
 *   ligand rows of x get x_next + frame_shift (without frame_shift they get x_next).  Start with frame_shift = 0.
 *   update_positions == 0: x_next = x_lig, the removed mean is 0 and the pocket stays; update_types == 0: c_next = c_lig.
 * Both calls: a graph without ligand atoms has a zero mean (the reference's clamp(count, min=1)): its shift row is 0, its
 *   frame_shift row and its pocket rows keep their values.  n_lig == 0 (with any n_graphs) or n_graphs == 0 returns CBGX_OK
 *   before any other argument is looked at and writes NOTHING: not x_next / c_next, not x / h, not shift, not frame_shift. */
int cbgx_diffbp_epilogue(const float *x_den, const float *x_com, const float *x_in, const float *logits,
                         const int32_t *lig_rows, const int32_t *lig_ptr, const float *x_lig, const float *c_lig,
                         const uint8_t *gen_lig, int n_lig, int n_graphs, int num_classes, int t, int num_timesteps,
                         const float *alphas_cumprod, const float *betas, int absorbing_state, const float *eps,
                         const float *u, float *x_next, float *c_next, void *stream);
int cbgx_diffsbdd_step(const float *x_den, const float *logits, const int32_t *graph_ptr, const int32_t *lig_rows,
                       const int32_t *lig_ptr, const uint8_t *lig_flag, const float *x_lig, const float *c_lig, int n_lig,
                       int n_graphs, int num_classes, float inv_alpha, float coef, float sigma, int update_positions,
                       int update_types, const float *eps_x, const float *eps_c, const float *lig_emb_w,
                       const float *lig_emb_b, const float *ind_w, const float *ind_b, float *x_next, float *c_next,
                       float *x, float *h, float *shift, float *frame_shift, void *stream);

/* ---- counter-based noise ("counter" noise mode of the samplers; csrc/rng.h) ------------------------------------------
 * Every random number of a sampling run is a pure function of an address, evaluated on the device where it is consumed:
 *   Philox4x32-10( counter = (atom's index inside its ligand, step, purpose base + purpose, block),
 *                  key     = the low and the high half of the graph's 64-bit stream key )
 * The four output words are the components 4 * block .. 4 * block + 3 of the draw.  A uniform is (w >> 8) * 2^-24 in [0, 1); normals
 * are Box-Muller pairs: words (0, 1) give components 4 block + 0 / + 1 (r cos, r sin), words (2, 3) components 4 block + 2 / + 3, with
 * r = sqrt(-2 log(((w_r >> 8) + 1) * 2^-24)) and the angle 2 pi (w_a >> 8) * 2^-24.  The stream key of graph (pocket, sample) comes
 * from one Philox call on the host: counter = (seed low, seed high, pocket index, sample index), key = (0x58474243, 0x53494F4E), stream
 * key = word 0 | word 1 << 32 (cbgbench_amd/noise.py::stream_keys).  The samples of a graph are then independent of its place in the
 * batch, of the batch, the rank and the stream it runs on; the one precondition is that the atoms of a ligand keep their order.
 * Purposes (no two draws of a run share an address): */
#define CBGX_NOISE_POS_NORMAL 0   /* position normal of a reverse step, components 0..2 (all three model classes) */
#define CBGX_NOISE_TYPE_UNIFORM 1 /* type uniform of a reverse step, components 0..C-1 (TargetDiff's Gumbel draw) */
#define CBGX_NOISE_MASK_UNIFORM 2 /* mask draw of a reverse step, component 0 (DiffBP) */
#define CBGX_NOISE_TYPE_NORMAL 3  /* type normal of a reverse step, components 0..C-1 (DiffSBDD) */
#define CBGX_NOISE_INIT_POS 4     /* initial position normal, step 0 (DiffSBDD) */
#define CBGX_NOISE_INIT_TYPE 5    /* initial type normal, step 0 (DiffSBDD) */
#define CBGX_NOISE_FINAL_POS 6    /* position normal of sample_p_xh_given_z0, step 0 (DiffSBDD; the type normal the reference
                                     draws there and discards has no address) */
#define CBGX_NOISE_TRAIN_TIME 7          /* time of a graph in a training call: counter (0, 0, base + 7, 0), word 0 */
#define CBGX_NOISE_TRAIN_POS_NORMAL 8    /* position normal of a training / validation call, components 0..2 (all three classes) */
#define CBGX_NOISE_TRAIN_TYPE_UNIFORM 9  /* type uniform, components 0..C-1 (TargetDiff's Gumbel draw) */
#define CBGX_NOISE_TRAIN_MASK_UNIFORM 10 /* mask draw, component 0 (DiffBP) */
#define CBGX_NOISE_TRAIN_TYPE_NORMAL 11  /* type normal, components 0..C-1 (DiffSBDD) */
#define CBGX_NOISE_TRAIN_PROTEIN_NORMAL 12 /* protein-coordinate augmentation of a training visit, components 0..2: counter (the atom's
                                            index inside its POCKET, 0, base + 12, 0); see cbgx_train_transform_rng */
#define CBGX_NOISE_TRAIN_CHOOSE_CTX 13 /* which decomposition of its ligand a visit trains on: counter (0, 0, base + 13, 0), word 0; see
                                        cbgx_train_transform_choose_rng */
#define CBGX_NOISE_PURPOSE_STRIDE 16 /* purpose bases are multiples of this (0: a plain run) */
/* cbgx_noise_fill: out[a][col] (caller-owned, [n_lig, cols] floats) = component col of the draw of `purpose` at `step` for ligand
 *   atom a -- normals (uniform == 0) or uniforms (uniform != 0).  stream_keys [B] uint64; lig_ptr [B+1] the ligand CSR (ligand arrays
 *   sorted by graph); the step is *step_dev when step_dev != NULL (a device int: trajectory / hipGraph mode), else `step`.  These
 *   are the very numbers the _rng entry points below generate in place, bit for bit.  DiffBP and DiffSBDD take the counter mode
 *   through this call followed by cbgx_diffbp_epilogue / cbgx_diffsbdd_step on the filled buffers.
 * cbgx_targetdiff_{epilogue,step_boundary,epilogue_traj}_rng: the entry points of the same name without _rng, with eps / u replaced
 *   by (stream_keys [B], lig_graph [n_lig] = graph of every ligand atom, lig_ptr [B+1], purpose_base): lanes evaluate their
 *   position normal (purpose_base + CBGX_NOISE_POS_NORMAL) and type uniform (purpose_base + CBGX_NOISE_TYPE_UNIFORM) at step t
 *   (*t_dev in trajectory mode) themselves.  n_graphs (B) is only validated (>= 1), it does not reach the kernels: as with lig_rows and
 *   lig_ptr elsewhere in this library the caller vouches for the arrays -- every lig_graph[a] in [0, B), and lig_graph consistent
 *   with lig_ptr (lig_ptr[lig_graph[a]] <= a < lig_ptr[lig_graph[a] + 1]); keys[] and lig_ptr[] are indexed with it unchecked. */
int cbgx_noise_fill(const uint64_t *stream_keys, const int32_t *lig_ptr, int n_graphs, int n_lig, int cols, int uniform,
                    int purpose, int step, const int32_t *step_dev, float *out, void *stream);
/* Training and validation in counter mode (purposes CBGX_NOISE_TRAIN_*).  The stream key of a graph is the key of (seed, example index,
 *   visit): the example's index in its dataset stands where the pocket index stands, the training iteration -- the same number on
 *   every rank -- where the sample index stands.  Validation uses visit 0 and purpose_base = CBGX_NOISE_PURPOSE_STRIDE, so it never
 *   shares an address with a training draw.  The noised inputs of an example at an iteration then depend neither on the world size nor
 *   on the batch size nor on the example's place in its batch.
 *   Time of a graph: t_g = (uint64(w0) * n_t) >> 32 in [0, n_t) (w0 = 0xFFFFFFFF gives n_t - 1), w0 = word 0 of the call at counter
 *   (0, 0, purpose_base + CBGX_NOISE_TRAIN_TIME, 0) under the graph's key; n_t = T for TargetDiff and DiffBP, T + 1 for DiffSBDD.  The
 *   marginal of every t_g is the 'symmetric' sampler's (uniform on [0, T)); its antithetic pairing t, T - 1 - t inside a batch is a
 *   function of batch position and is not kept.
 *   Per-atom draws: counter (atom's index inside its ligand, step = t_g, purpose_base + purpose, block), words / uniforms / Box-Muller
 *   as in cbgx_noise_fill.  The step word is the graph's integer time in training and in eval mode: the evaluation times of one
 *   validation call draw at different addresses (two that coincide after truncation to an integer -- tiny T -- get the same draw), and
 *   DiffSBDD's second eval-mode network call (time 0) draws at step 0, which none of its evaluation times uses.
 * cbgx_train_noise_draw: the draws of one get_loss call in ONE launch.  t_out [B] int64 = t_in (when t_in != NULL: the caller's times)
 *   or the drawn times; written for every graph, a graph without a ligand atom included.  a [n_lig,3] (may be NULL): normals of
 *   CBGX_NOISE_TRAIN_POS_NORMAL; b [n_lig,cols_b] (may be NULL; cols_b in 1..32): normals (uniform_b == 0) or uniforms of purpose_b
 *   (0..15); both at step t_out[graph].  lig_ptr [B+1] the ligand CSR (ligand arrays sorted by graph).
 * cbgx_targetdiff_train_noise_rng: cbgx_targetdiff_train_noise (below) with eps / u / t replaced by (stream_keys, lig_ptr, n_graphs,
 *   purpose_base, n_t, t_in or NULL, t_out): every lane evaluates its graph's time, its position normal and its type uniforms
 *   (CBGX_NOISE_TRAIN_TYPE_UNIFORM, one Philox call per block of four classes) itself -- the numbers cbgx_train_noise_draw followed
 *   by cbgx_targetdiff_train_noise give, bit for bit, without a noise buffer.  An atom whose batch[a] is outside [0, n_graphs) is
 *   left unwritten. */
int cbgx_train_noise_draw(const uint64_t *stream_keys, const int32_t *lig_ptr, int n_graphs, int n_lig, int purpose_base, int n_t,
                          const int64_t *t_in, int64_t *t_out, float *a, float *b, int cols_b, int purpose_b, int uniform_b,
                          void *stream);
int cbgx_targetdiff_train_noise_rng(const float *x0, const int64_t *v0, const int64_t *batch, const uint8_t *gen, int n_lig,
                                    int num_classes, const float *alphas_cumprod, const float *log_alphas_cumprod,
                                    const float *log_one_minus_alphas_cumprod, const uint64_t *stream_keys,
                                    const int32_t *lig_ptr, int n_graphs, int purpose_base, int n_t, const int64_t *t_in,
                                    int64_t *t_out, float *x_t, float *c_t, int64_t *v_t, void *stream);
/* Per-visit transforms of a training batch: the protein-coordinate augmentation (add_pos_noise) followed by the centring of the graph
 *   (center_pos / center_whole_pos), for the whole batch in ONE launch, one 256-thread workgroup per graph, out of place; the caller
 *   owns every buffer.  x_rec [n_rec,3], x_lig [n_lig,3]: the stored coordinates, both arrays sorted by graph; rec_ptr, lig_ptr [B+1]
 *   int32: their CSR; ctx [n_lig] uint8 (context atoms != 0) or NULL (no graph has a context atom).
 *   Noise: x_rec' = fmaf(sigma, eps, x_rec) when sigma > 0, x_rec itself when sigma == 0.  eps [n_rec,3], or NULL, which means no noise
 *   and requires sigma == 0.
 *   Centre of graph g = mean of its centre set: */
#define CBGX_CENTER_PROTEIN 0 /* the NOISED protein atoms (center_pos, center_flag protein, after add_pos_noise) */
#define CBGX_CENTER_CONTEXT 1 /* the ligand atoms with ctx != 0; a graph without one: its whole ligand (translation.py:13-16) */
#define CBGX_CENTER_LIGAND 2  /* the ligand atoms */
#define CBGX_CENTER_WHOLE 3   /* the noised protein atoms followed by the ligand atoms (center_whole_pos) */
/*   The sum has a fixed order that depends on the graph's own atoms only: the candidates of the set are numbered in atom order (WHOLE:
 *   protein atoms first, then ligand atoms; CONTEXT: every ligand atom is a candidate and an atom outside the context adds nothing),
 *   thread k adds candidates k, k + 256, ... in that order, a fixed tree (strides 128 ... 1) adds the 256 partial sums, one IEEE
 *   division by the member count follows; no atomics.  An empty set (after the CONTEXT -> LIGAND fallback) gives the zero vector.
 *   Outputs: x_rec_out [n_rec,3] = x_rec' - centre, x_lig_out [n_lig,3] = x_lig - centre, center_out [B,3] = centre.  Every element of
 *   every graph is written, center_out rows of empty graphs too.  CSR entries outside [0, n] are clamped.
 *   CBGX_E_INVALID, before anything touches the device: a NULL output or input that has elements, negative sizes, sigma < 0 (or NaN), an
 *   unknown center_mode, eps == NULL with sigma > 0, a purpose_base that is not a non-negative multiple of CBGX_NOISE_PURPOSE_STRIDE.
 * cbgx_train_transform_rng: the same with eps replaced by (stream_keys [B], purpose_base): every lane evaluates the normals of its
 *   protein atoms itself, at counter (the atom's index inside its pocket, step 0, purpose_base + CBGX_NOISE_TRAIN_PROTEIN_NORMAL,
 *   block 0), components 0..2, under the graph's training / validation stream key -- the bits of cbgx_noise_fill(stream_keys, rec_ptr,
 *   B, n_rec, cols = 3, normals, purpose_base + CBGX_NOISE_TRAIN_PROTEIN_NORMAL, step = 0) followed by cbgx_train_transform.
 *   Precondition: the protein atoms of an example keep their order. */
int cbgx_train_transform(const float *x_rec, const float *x_lig, const int32_t *rec_ptr, const int32_t *lig_ptr,
                         const uint8_t *ctx, int n_graphs, int n_rec, int n_lig, float sigma, int center_mode, const float *eps,
                         float *x_rec_out, float *x_lig_out, float *center_out, void *stream);
int cbgx_train_transform_rng(const float *x_rec, const float *x_lig, const int32_t *rec_ptr, const int32_t *lig_ptr,
                             const uint8_t *ctx, int n_graphs, int n_rec, int n_lig, float sigma, int center_mode,
                             const uint64_t *stream_keys, int purpose_base, float *x_rec_out, float *x_lig_out,
                             float *center_out, void *stream);
/* The same behind the reference's choose_ctx_gen (select.py:21-58), in the same launch: every graph picks one of its decompositions, the
 *   atoms that one names become the generated atoms, the others the context (ctx = !gen_flag) of the steps above.
 *   dec_ptr [B+1] int32: graph g owns the decompositions dec_ptr[g] .. dec_ptr[g+1], K_g of them; gen_ptr [n_dec+1] int32:
 *   decomposition d names the atoms gen_idx[gen_ptr[d] .. gen_ptr[d+1]]; gen_idx [n_idx] int32: indices INSIDE the graph's ligand.  All
 *   three CSRs are clamped to their arrays; an index outside [0, atoms of the graph's ligand) is skipped; duplicates are harmless; an
 *   empty decomposition (all context) and one that names every atom (no context: CBGX_CENTER_CONTEXT falls back to the whole ligand)
 *   are both legal.
 *   Choice k_g: choice_in[g] clamped into [0, K_g) (choice_in [B] int32, or NULL: decomposition 0 everywhere).  K_g == 0: k_g = -1 and
 *   every ligand atom of the graph is generated.
 *   Outputs beside those of cbgx_train_transform: gen_flag_out [n_lig] uint8 (1 generated, 0 context) and choice_out [B] int32 = k_g;
 *   every element of every graph is written.  The noise, the centre and the shift are cbgx_train_transform's, bit for bit, on
 *   ctx = !gen_flag_out.  All four centre modes are accepted; the flag is produced whatever the mode.
 *   CBGX_E_INVALID as for cbgx_train_transform, and for negative n_dec / n_idx or a NULL dec_ptr, choice_out, gen_flag_out, gen_ptr or
 *   gen_idx that has elements.
 * cbgx_train_transform_choose_rng: choice and eps both drawn in the kernel: k_g = (uint64(w0) * K_g) >> 32 with w0 = word 0 of the call
 *   at counter (0, 0, purpose_base + CBGX_NOISE_TRAIN_CHOOSE_CTX, 0) under stream_keys[g] (the formula of the training time at an
 *   address no other draw uses); the protein normals as in cbgx_train_transform_rng. */
int cbgx_train_transform_choose(const float *x_rec, const float *x_lig, const int32_t *rec_ptr, const int32_t *lig_ptr,
                                const int32_t *dec_ptr, const int32_t *gen_ptr, const int32_t *gen_idx, const int32_t *choice_in,
                                int n_graphs, int n_rec, int n_lig, int n_dec, int n_idx, float sigma, int center_mode,
                                const float *eps, float *x_rec_out, float *x_lig_out, float *center_out, uint8_t *gen_flag_out,
                                int32_t *choice_out, void *stream);
int cbgx_train_transform_choose_rng(const float *x_rec, const float *x_lig, const int32_t *rec_ptr, const int32_t *lig_ptr,
                                    const int32_t *dec_ptr, const int32_t *gen_ptr, const int32_t *gen_idx, int n_graphs, int n_rec,
                                    int n_lig, int n_dec, int n_idx, float sigma, int center_mode, const uint64_t *stream_keys,
                                    int purpose_base, float *x_rec_out, float *x_lig_out, float *center_out,
                                    uint8_t *gen_flag_out, int32_t *choice_out, void *stream);
int cbgx_targetdiff_epilogue_rng(const float *x_den, const float *logits, const int32_t *lig_rows, const float *x_lig,
                                 const float *c_lig, const uint8_t *gen_lig, int n_lig, int num_classes, int t,
                                 int num_timesteps, const float *const *tables, const uint64_t *stream_keys,
                                 const int32_t *lig_graph, const int32_t *lig_ptr, int n_graphs, int purpose_base,
                                 float *x_next, float *c_next, int32_t *v_next, void *stream);
int cbgx_targetdiff_step_boundary_rng(const float *x_den, const float *logits, const int32_t *lig_rows, const float *x_lig,
                                      const float *c_lig, const uint8_t *gen_lig, int n_lig, int num_classes, int t,
                                      int num_timesteps, const float *const *tables, const uint64_t *stream_keys,
                                      const int32_t *lig_graph, const int32_t *lig_ptr, int n_graphs, int purpose_base,
                                      float *x_next, float *c_next, const float *lig_emb_w, const float *lig_emb_b,
                                      const float *ind_w, const float *ind_b, float *x, float *h, void *stream);
int cbgx_targetdiff_epilogue_traj_rng(const float *x_den, const float *logits, const int32_t *lig_rows, float *traj_x,
                                      float *traj_c, const uint8_t *gen_lig, int n_lig, int num_classes, int32_t *t_dev,
                                      const float *const *tables, const uint64_t *stream_keys, const int32_t *lig_graph,
                                      const int32_t *lig_ptr, int n_graphs, int purpose_base, void *stream);

/* ---- training: taped forward and backward -----------------------------------------------------------
 * train.py:185-189 runs `loss_dict, _ = model(batch); loss.backward()`; autograd walks UniTransformer.forward
 * (unitransformer.py:102-123) backwards through every X2HAttention / H2XAttention (x2h_attention.py:43-97,
 * h2x_attention.py:34-73), the gate and the classifier.  libcbgx replaces that pair with
 *   cbgx_unitransformer_forward_train : same outputs as cbgx_unitransformer_forward and a *tape*
 *       (caller-owned, cbgx_train_tape_bytes) holding the kNN lists, the gate, the per-layer x / h inputs and the node
 *       stage of every block (projection [N,640] + folded query [N,16,128]: 177 KB per node and layer).  h_out != NULL: no
 *       pruning.  h_out == NULL (round 6): the caller promises that its loss reads x_out on gen_flag rows and logits on
 *       lig_flag rows only -- and will call the backward with grad_h_out == NULL; the last two x2h blocks, the neighbour
 *       projections of the h2x blocks and the classifier then run on the receptive field of those rows, as in the sampling
 *       forward (rows of `logits` outside gen | lig | nbr(gen) are not written);
 *   cbgx_unitransformer_backward      : given dL/dx_out [N,3], dL/dh_out [N,128], dL/dlogits [N,C] (each may be
 *       NULL = zero) it recomputes the per-edge intermediates block by block (nothing per-edge is ever stored) and
 *       writes dL/dh_in [N,128] (may be NULL) and the gradient of every parameter tensor: `grads` is a HOST array
 *       of DEVICE pointers, same order and shapes as the `tensors` of cbgx_pack_weights (6 + 36*L + 4), each
 *       OVERWRITTEN.  No gradient is produced for the input coordinates (the training losses treat them as data:
 *       targetdiff.py:87-101); cbgx_unitransformer_backward_ex below also returns it.
 *       PRECONDITION of grad_h_out == NULL: the caller's loss reads x_out on gen_flag rows and logits on lig_flag rows only
 *       (what TargetDiff.get_loss / DiffSBDD.get_loss do, targetdiff.py:103-121); the backward of the last x2h blocks is
 *       then pruned to the receptive field of those rows, the classifier head's backward walks the lig_flag rows only, and
 *       gradient entries on other rows are ignored.  A loss that touches other rows must pass a (possibly all-zero) grad_h_out
 *       (and must have run the forward with h_out != NULL): the backward is then exact for ANY loss -- since round 6 it still
 *       prunes, but around the support of the caller's gradients, which it finds itself (the rows of grad_h_out / grad_logits
 *       with a non-zero entry are marked on the device and join the seed of the receptive field; DiffBP's centre-of-mass head
 *       reads h_out on the movable atoms and their neighbours only: + 9.6 % on its training step).
 * Both take the larger training workspace (cbgx_train_workspace_bytes).  Neighbour-row gradients are accumulated with
 * fp32 atomics, so results are reproducible only up to summation order (as with the reference's torch_scatter on GPU).
 * CBGX_BX_EDGE_ROWS=1 in the environment (read at every backward call; ABI unchanged, the workspace always holds the buffers:
 * 32 KB per node) selects the edge-row mode of the x2h blocks instead: every edge's contribution goes to its own row and the rows of
 * every source node are summed in a fixed order (csrc/train_scatter.hip) -- dL/dh then has the same bits in every run, the
 * coordinate gradient still uses atomics, and a training step is 1 - 3 % slower.  Same mathematics, same tolerances in the tests. */
/* cbgx_unitransformer_forward_train_ex (ABI 5): the same with `flags`; CBGX_FWD_H_ON_SOURCES = h_out is wanted on
 * A1 = gen_flag | lig_flag | in-neighbours of gen_flag rows only (zero elsewhere) -- the taped forward prunes as with h_out == NULL,
 * and the caller's dL/dh_out must vanish outside A1 (DiffBP: the centre-of-mass head reads h_out on the movable atoms and their
 * neighbours in the same k-nearest-neighbour graph). */
size_t cbgx_train_tape_bytes(int n_nodes, int num_layers);
size_t cbgx_train_workspace_bytes(int n_nodes);
int cbgx_unitransformer_forward_train(const float *packed, int num_layers, int num_classes,
                                      const float *x, const float *h, const int32_t *graph_ptr,
                                      const uint8_t *lig_flag, const uint8_t *gen_flag, int n_nodes, int n_graphs,
                                      float *x_out, float *h_out, float *logits, void *tape, size_t tape_bytes,
                                      void *workspace, size_t workspace_bytes, void *stream);
int cbgx_unitransformer_backward(const float *packed, int num_layers, int num_classes, const void *tape,
                                 size_t tape_bytes, const uint8_t *lig_flag, const uint8_t *gen_flag, int n_nodes,
                                 const float *grad_x_out, const float *grad_h_out, const float *grad_logits,
                                 float *const *grads, int num_grads, float *grad_h_in, void *workspace,
                                 size_t workspace_bytes, void *stream);
/* cbgx_unitransformer_backward_ex (ABI 6, additive): the same, plus grad_x_in [N,3] (may be NULL) = the full dL/dx_in, OVERWRITTEN --
 * what autograd gives the reference's UniTransformer input `x` (unitransformer.py:102-123): the layer chain x_{l+1} = x_l + gen * H2X
 * (h2x_attention.py:34-73: rel_x and the distance features of every block, x2h_attention.py:43-97: the distance features) and the
 * distance gate e_w = sigmoid(MLP(rbf(|x_i - x_j|))) computed once from x (unitransformer.py:109-112).  The kNN selection itself is
 * piecewise constant (no gradient), as in the reference.  Exact under every pruning mode of the backward above (grad_h_out == NULL,
 * the marked support, CBGX_FWD_H_ON_SOURCES) and in the edge-row mode: skipped rows carry an exactly zero gradient.  grad_x_in is
 * accumulated with fp32 atomics: reproducible only up to summation order.  grad_x_in == NULL: exactly cbgx_unitransformer_backward
 * (same launches). */
int cbgx_unitransformer_backward_ex(const float *packed, int num_layers, int num_classes, const void *tape,
                                    size_t tape_bytes, const uint8_t *lig_flag, const uint8_t *gen_flag, int n_nodes,
                                    const float *grad_x_out, const float *grad_h_out, const float *grad_logits,
                                    float *const *grads, int num_grads, float *grad_h_in, float *grad_x_in, void *workspace,
                                    size_t workspace_bytes, void *stream);
/* Backward of one attention block (stage-level parity tests).  Inputs as the forward stage; `grads` = 18 DEVICE
 * pointers {hk,hv,hq}_func (x2h) / {xk,xv,xq}_func (h2x) x net.{0.weight,0.bias,1.weight,1.bias,3.weight,3.bias}.
 * x2h: grad_h includes the residual path.  h2x: grad_x includes the identity path of x_out = x + delta_x * gen_flag.
 * grad_e_w [N,32] is the gradient with respect to the gate values. */
int cbgx_unitransformer_forward_train_ex(const float *packed, int num_layers, int num_classes, const float *x, const float *h,
                                         const int32_t *graph_ptr, const uint8_t *lig_flag, const uint8_t *gen_flag,
                                         int n_nodes, int n_graphs, float *x_out, float *h_out, float *logits, unsigned flags,
                                         void *tape, size_t tape_bytes, void *workspace, size_t workspace_bytes, void *stream);
int cbgx_x2h_attention_backward(const float *packed, int layer, const float *x, const float *h,
                                const int32_t *nbr, const int32_t *deg, const uint8_t *lig_flag, const float *e_w,
                                int n_nodes, const float *grad_h_out, float *grad_h, float *grad_x, float *grad_e_w,
                                float *const *grads, void *workspace, size_t workspace_bytes, void *stream);
int cbgx_h2x_attention_backward(const float *packed, int layer, const float *x, const float *h,
                                const int32_t *nbr, const int32_t *deg, const uint8_t *lig_flag,
                                const uint8_t *gen_flag, const float *e_w, int n_nodes, const float *grad_x_out,
                                float *grad_h, float *grad_x, float *grad_e_w, float *const *grads, void *workspace,
                                size_t workspace_bytes, void *stream);

/* The same pair for a stack of H2X blocks on its own graph: DiffBP's CoMPredictor inside `DiffBP.get_loss`
 * (repo/models/diffusion/diffbp.py:79-101, 195-198).  The tape holds the stack's kNN lists, gate and per-layer
 * coordinates; h is the same tensor in every layer.  backward: grad_x_out [N,3] -> grad_h [N,128] (overwritten) and
 * `grads` = 6 + 18*L DEVICE pointers in the order of cbgx_pack_h2x_stack's `tensors`, each overwritten.  No gradient for the
 * input coordinates (in DiffBP's losses they are the noised data); cbgx_h2x_stack_backward_ex returns it.
 * cbgx_h2x_stack_backward_ex (ABI 6, additive): the same, plus grad_x_in [N,3] (may be NULL) = dL/dx_in, OVERWRITTEN -- autograd of
 * CoMPredictor's input x (diffbp.py:79-101): the stack's blocks (h2x_attention.py:34-73) and its own distance gate
 * (diffbp.py:87-90), exact on the movable-row lists the backward walks.  fp32 atomics: reproducible only up to summation order.
 * grad_x_in == NULL: exactly cbgx_h2x_stack_backward. */
size_t cbgx_h2x_stack_tape_bytes(int n_nodes, int num_layers);
int cbgx_h2x_stack_forward_train(const float *packed, int num_layers, const float *x, const float *h,
                                 const int32_t *graph_ptr, const uint8_t *lig_flag, const uint8_t *gen_flag,
                                 int n_nodes, int n_graphs, float *x_out, void *tape, size_t tape_bytes,
                                 void *workspace, size_t workspace_bytes, void *stream);
int cbgx_h2x_stack_backward(const float *packed, int num_layers, const void *tape, size_t tape_bytes, const float *h,
                            const uint8_t *lig_flag, const uint8_t *gen_flag, int n_nodes, const float *grad_x_out,
                            float *const *grads, int num_grads, float *grad_h, void *workspace,
                            size_t workspace_bytes, void *stream);
int cbgx_h2x_stack_backward_ex(const float *packed, int num_layers, const void *tape, size_t tape_bytes, const float *h,
                               const uint8_t *lig_flag, const uint8_t *gen_flag, int n_nodes, const float *grad_x_out,
                               float *const *grads, int num_grads, float *grad_h, float *grad_x_in, void *workspace,
                               size_t workspace_bytes, void *stream);

/* TargetDiff's training arithmetic around the denoiser call (targetdiff.py:82-124), one launch each instead of the ~260 small
 * launches the same formulas take as tensor operations (a training step is bound by its launch count as much as by its kernels).
 * Index tensors are int64 as PyTorch holds them (no conversion launches); gen / masks are bytes.  Preconditions the library cannot
 * check without reading device memory: 0 <= batch[a] < n_graphs (the per-graph sums are indexed by it), 0 <= t[g] < T, types < C.
 * cbgx_targetdiff_train_noise: q(x_t | x_0) on gen rows (CTNVPScheduler.forward_add_noise, diffusion_scheduler.py:117-134) and
 *   q(v_t | v_0) by Gumbel-argmax (TypeVPScheduler.forward_add_noise, :339-365).  t [B] per graph, batch [n_lig] graph of each
 *   ligand atom; eps [n_lig,3] ~ N(0,1), u [n_lig,C] ~ U(0,1) are inputs.  Outputs x_t [n_lig,3], c_t [n_lig,C] one-hot, v_t [n_lig].
 * cbgx_targetdiff_loss: position loss (type 'denoise': sum of squares against x0, :185-201) and atom-type loss (KL between
 *   q(v_{t-1} | v_t, v_0) and q(v_{t-1} | v_t, softmax(logits)); the decoder NLL for graphs at t = 0; :380-441), each the mean over
 *   the gen atoms of a graph, then over the graphs (targetdiff.py:103-121).  x_out [N,3] / logits [N,C] are the denoiser outputs,
 *   lig_rows [n_lig] the composed row of each ligand atom; tables = {log_alphas_v, log_one_minus_alphas_v, log_alphas_cumprod_v,
 *   log_one_minus_alphas_cumprod_v} [T].  losses [2] = {pos, atom}; x_pred [n_lig,3], c_pred [n_lig,C] = softmax(logits) (the
 *   `results` of the reference; may be NULL); grad_pos [n_lig,3], grad_logit [n_lig,C] receive d loss_pos / d x_out[row] and
 *   d loss_atom / d logits[row].  n_graphs <= 4096.
 * cbgx_targetdiff_loss_backward: grad_x_out [N,3] = *g_loss_pos * grad_pos and grad_logits [N,C] = *g_loss_atom * grad_logit on
 *   ligand rows, zero on protein rows; sort_idx [N] is the composition permutation (composed row r holds entry sort_idx[r] of
 *   cat(protein, ligand)); g_loss_* are DEVICE scalars (NULL = 0). */
int cbgx_targetdiff_train_noise(const float *x0, const int64_t *v0, const int64_t *t, const int64_t *batch,
                                const uint8_t *gen, int n_lig, int num_classes, const float *alphas_cumprod,
                                const float *log_alphas_cumprod, const float *log_one_minus_alphas_cumprod,
                                const float *eps, const float *u, float *x_t, float *c_t, int64_t *v_t, void *stream);
int cbgx_targetdiff_loss(const float *x_out, const float *logits, const int64_t *lig_rows, const float *x0,
                         const int64_t *v0, const int64_t *v_t, const int64_t *t, const int64_t *batch, const uint8_t *gen,
                         int n_lig, int n_graphs, int num_classes, const float *const *tables, float *losses, float *x_pred,
                         float *c_pred, float *grad_pos, float *grad_logit, void *stream);
int cbgx_targetdiff_loss_backward(const float *grad_pos, const float *grad_logit, const int64_t *sort_idx, int n_protein,
                                  int n_nodes, int num_classes, const float *g_loss_pos, const float *g_loss_atom,
                                  float *grad_x_out, float *grad_logits, void *stream);
/* cbgx_diffbp_loss (ABI 5): DiffBP's four training losses around its two network calls -- zero-COM noise prediction + centre-of-mass
 *   prediction (CoMPredictor.forward, diffbp.py:79-101), get_score_loss x 2 (diffusion_scheduler.py:203-218), MaskTypeSchedule.get_loss
 *   (:499-511: cross_entropy of the softmax OUTPUT, as the reference has it), xs_mean (:166-183) and interior_loss (diffbp.py:18-28)
 *   -- in two launches, with their gradients with respect to the network outputs.  All [N,.] arrays are in the COMPOSED row order
 *   (per graph: protein rows, then ligand rows; graph_ptr [B+1]; sort_idx [N] as above; lig_flag [N]); x_in = the composed input
 *   positions (protein positions and x_t), x_stack = the centre-of-mass head's output positions.  pos_noise / com_noise [n_lig,3],
 *   v0, type_flag (the mask of the type loss), gen [n_lig] in LIGAND order; t [B].  cbgx_diffbp_loss takes ligands of at most 48 atoms.
 *   Beyond that the reference restricts every protein atom to its 48 nearest ligand atoms (torch_cluster.knn(k=48), diffbp.py:18-28):
 *   cbgx_diffbp_loss_knn, the same entry with knn_scratch [2 N] floats (N = n_protein + n_lig), takes ligands of at most 128 atoms and,
 *   for a graph of more than 48, keeps the pair (protein p, ligand l) iff (d^2(p,l), l) is among the 48 lexicographically smallest pairs
 *   of p's row -- exactly 48 neighbours, ties broken by the ligand's index within its graph; the selection carries no gradient; graphs of
 *   at most 48 ligand atoms get the same bits from both entries.  A graph over the entry's limit sets *bad to 1 (the host must take its
 *   tensor path), adds nothing to the losses and gets zeros in its rows of the five gradient pieces.
 *   losses [4] = {pos, atom, com, inter}; scal [2] = {1 / D_gen, 1 / D_type}, the graph-count divisors of the masked means;
 *   gstats [8 n_graphs] scratch.  Gradient pieces, [N,3] / [N,C], zero on protein rows, to be combined by the caller with the
 *   upstream gradients g_* of the four losses:
 *     d L / d x_out   = g_pos scal[0] a_pos + g_inter a_int        d L / d x_stack = g_com scal[0] b_com + g_inter b_int
 *     d L / d logits  = g_atom scal[1] z_atom */
int cbgx_diffbp_loss(const float *x_out, const float *x_in, const float *x_stack, const float *logits, const int64_t *sort_idx,
                     const int32_t *graph_ptr, const uint8_t *lig_flag, const float *pos_noise, const float *com_noise,
                     const int64_t *v0, const uint8_t *type_flag, const uint8_t *gen, const int64_t *t, int n_protein, int n_lig,
                     int n_graphs, int num_classes, const float *alphas_cumprod, const float *betas, float rho, float gamma,
                     float *losses, float *scal, float *gstats, float *a_pos, float *a_int, float *b_com, float *b_int,
                     float *z_atom, int32_t *bad, void *stream);
int cbgx_diffbp_loss_knn(const float *x_out, const float *x_in, const float *x_stack, const float *logits, const int64_t *sort_idx,
                         const int32_t *graph_ptr, const uint8_t *lig_flag, const float *pos_noise, const float *com_noise,
                         const int64_t *v0, const uint8_t *type_flag, const uint8_t *gen, const int64_t *t, int n_protein, int n_lig,
                         int n_graphs, int num_classes, const float *alphas_cumprod, const float *betas, float rho, float gamma,
                         float *losses, float *scal, float *gstats, float *a_pos, float *a_int, float *b_com, float *b_int,
                         float *z_atom, int32_t *bad, float *knn_scratch, void *stream);
/* cbgx_diffbp_train_noise: the forward noising of a DiffBP training step in one launch -- CTNVPScheduler.forward_add_noise with
 *   zero_center=True (diffusion_scheduler.py:117-134) and MaskTypeSchedule.forward_add_noise (:452-473).  x0 [n_lig,3], v0 [n_lig], gen
 *   [n_lig], eps [n_lig,3] ~ N(0,1), u [n_lig] ~ U(0,1) in LIGAND order; t [B]; sort_idx [N] / graph_ptr [B+1] from cbgx_compose_plan
 *   (the ligand index array need not be sorted).  Outputs, in ligand order:
 *     x_t = gen ? sqrt(a_t) x0 + sqrt(1 - a_t) eps : x0        com_noise = the graph's mean of eps over ALL its ligand atoms
 *     pos_noise = eps - com_noise                               type_flag = (u < t / T) & gen   (bytes; t / T an fp32 division)
 *     v_t = type_flag ? absorbing_state : v0                    c_t [n_lig,C] = onehot(v_t)
 *   The mean is summed in a fixed order (no atomics): the same bits run to run. */
int cbgx_diffbp_train_noise(const float *x0, const int64_t *v0, const int64_t *t, const uint8_t *gen, const float *eps, const float *u,
                            const int64_t *sort_idx, const int32_t *graph_ptr, int n_protein, int n_lig, int n_graphs,
                            int num_classes, const float *alphas_cumprod, int num_timesteps, int absorbing_state, float *x_t,
                            float *pos_noise, float *com_noise, int64_t *v_t, float *c_t, uint8_t *type_flag, void *stream);

/* cbgx_compose_plan (ABI 6): the index work of compose_context (repo/modules/common.py:189-214) -- sort_idx [N] = the STABLE argsort of
 *   cat(batch_protein, batch_ligand) (graph ids in [0, n_graphs), int64), and what its callers derive from it: batch_idx [N] the sorted ids,
 *   lig_flag [N] (1 = ligand atom), lig_rows [n_ligand] the composed row of every ligand atom, graph_ptr [n_graphs + 1] the CSR offsets --
 *   as a counting sort in three launches.  Exact for any order of the ids (arrays that are not non-decreasing, which no collated batch is,
 *   take a slow rank pass); ids outside [0, n_graphs) are dropped.  scratch: 4 n_graphs + 1 ints. */
int cbgx_compose_plan(const int64_t *batch_protein, const int64_t *batch_ligand, int n_protein, int n_ligand, int n_graphs,
                      int32_t *scratch, int64_t *sort_idx, int64_t *batch_idx, uint8_t *lig_flag, int64_t *lig_rows,
                      int32_t *graph_ptr, void *stream);

/* cbgx_diffsbdd_train_noise / cbgx_diffsbdd_loss (ABI 6): the tensor operations of DiffSBDD.get_loss (training mode) around its denoiser
 *   call, diffsbdd.py:91-195.  All graph-wise sums are taken per graph of the COMPOSED order (graph_ptr [B+1], sort_idx [N] as above), in a
 *   fixed order.  x0 [n_lig,3], x_protein [n_protein,3], v0 [n_lig] class indices (the one-hot / 4 features are formed inside), eps_x
 *   [n_lig,3] / eps_c [n_lig,C] the Gaussian draws, gen [n_lig], t [B] integer time steps in [0, T]; alpha_table / sigma_table [T+1] =
 *   sqrt(sigmoid(-gamma)), sqrt(sigmoid(gamma)) of the predefined schedule (schedule_utils.py:60-96).
 *   _train_noise: ligand centred on its mean, z_t for coordinates and types with the pocket re-centred on the noisy ligand
 *   (diffusion_scheduler.py:740-790) -> x_t, x_protein_t, c_t; gdata [4 B] = per graph {ligand atoms, KL prior of the coordinates, KL prior
 *   of the types (:846-868), -log p(c | z_0) [t == 0] (:930-945)}: every term of the loss that does not depend on the network.
 *   _loss: x_out [N,3] / logits [N,C] = the denoiser's outputs (composed order); losses [2] = {pos, atom} = mean over graphs of
 *   0.5 sum(err^2) [t != 0] / (n dim) + the t == 0 terms + KL (:886-900); glosses [2 B] scratch; x_pred / c_pred = the outputs on the
 *   ligand rows, in ligand order; grad_pos [n_lig,3] / grad_logit [n_lig,C] = d losses / d those rows -- scatter them with
 *   cbgx_targetdiff_loss_backward. */
int cbgx_diffsbdd_train_noise(const float *x0, const float *x_protein, const int64_t *v0, const float *eps_x, const float *eps_c,
                              const uint8_t *gen, const int64_t *t, const int64_t *sort_idx, const int32_t *graph_ptr, int n_protein,
                              int n_lig, int n_graphs, int num_classes, const float *alpha_table, const float *sigma_table,
                              int num_timesteps, float *x_t, float *x_protein_t, float *c_t, float *gdata, void *stream);
int cbgx_diffsbdd_loss(const float *x_out, const float *logits, const float *eps_x, const float *eps_c, const int64_t *t,
                       const int64_t *sort_idx, const int32_t *graph_ptr, int n_protein, int n_lig, int n_graphs, int num_classes,
                       const float *gdata, float *glosses, float *losses, float *x_pred, float *c_pred, float *grad_pos,
                       float *grad_logit, void *stream);

/* cbgx_embed_compose / cbgx_embed_compose_backward (ABI 6): the input side of a training step -- PLContextEmbedder
 *   (repo/modules/context_emb.py:137-230, the shipped configuration: Linear atom / residue / ligand-indicator embeddings, no time / vec)
 *   and compose_context (repo/modules/common.py:189-214) -- as one launch, and the embedder's weight gradients as two.
 *     protein row:  h = W_pa feat + b_pa + W_res onehot(aa) + b_res + b_ind           ligand row:  h = W_la c + b_la + W_ind + b_ind
 *     x = cat(x_protein, x_ligand)[sort_idx],  h likewise,  gen_flag = cat(gen_protein, gen_ligand)[sort_idx]
 *   protein_feat [n_protein, feat_dim] fp32, protein_aa [n_protein] class indices (an index outside [0, num_aa) embeds as no residue),
 *   ligand_feat [n_ligand, lig_dim] fp32 (one-hot or noised types); sort_idx [N] as above; gen_protein may be NULL (all 0), gen_flag may be
 *   NULL (not written).  params: the eight tensors of the embedder in nn.Linear layout -- protein_atom_emb.weight [128, feat_dim], .bias,
 *   residue_emb.weight [128, num_aa], .bias, ligand_atom_emb.weight [128, lig_dim], .bias, ligand_indicator.weight [128, 1], .bias.
 *   feat_dim + num_aa + lig_dim + 2 <= 120.  Outputs x [N,3], h [N,128] and ext [N,128], the rows
 *     ext = [ feat | onehot(aa) | 1 if protein | c | 1 if ligand | 0 ... ]
 *   that the backward multiplies with: h = ext . Wext for the stacked weights, so  dWext[c][j] = sum_r grad_h[r][c] ext[r][j]  holds
 *   every parameter's gradient.  cbgx_embed_compose_backward: partial = scratch of `groups` slabs of 128 x 128 floats (1 <= groups <= 256:
 *   the rows are split into that many partial sums, added in slab order -- reproducible); grad_out [128 (feat_dim + num_aa + lig_dim + 2)]
 *   = dW_pa [128, feat_dim] | dW_res [128, num_aa] | u [128] | dW_la [128, lig_dim] | v [128]  back to back, with
 *   db_pa = db_res = u,  db_la = dW_ind[:, 0] = v,  db_ind = u + v.  Coordinates and features get no gradient (they are data). */
int cbgx_embed_compose(const float *x_protein, const float *x_ligand, const float *protein_feat, const int64_t *protein_aa,
                       const float *ligand_feat, const int64_t *sort_idx, const uint8_t *gen_protein, const uint8_t *gen_ligand,
                       int n_protein, int n_ligand, int feat_dim, int num_aa, int lig_dim, const float *const *params, float *x,
                       float *h, float *ext, uint8_t *gen_flag, void *stream);
int cbgx_embed_compose_backward(const float *grad_h, const float *ext, int n_nodes, int feat_dim, int num_aa, int lig_dim,
                                float *partial, int groups, float *grad_out, void *stream);

/* ---- geometry report of sampled ligands: stability and steric clash (geometry.hip) ---------------------------------------------------
 * For a whole batch in ONE launch, one 256-thread workgroup per graph: the two coordinate-and-element metrics of the reference's
 *   quality path -- atom / molecule stability (repo/tools/geometry/eval_stability.py, check_stability with hs=False) and steric clash
 *   (repo/tools/geometry/eval_steric_clash.py, detect_clash) -- without RDKit.
 *   x_lig [n_lig,3] fp32, z_lig [n_lig] uint8 atomic numbers, lig_ptr [B+1] int32; x_rec [n_rec,3], z_rec [n_rec], rec_ptr [B+1]
 *   likewise; both arrays sorted by graph.  CSR entries outside [0, n] are clamped.  A ligand has at most CBGX_GEOMETRY_MAX_LIGAND
 *   atoms (they are staged in LDS); the number of protein atoms is not limited.
 *   Distance of two atoms: the fp32 coordinates widened to fp64, dx = xi - xj (dy, dz likewise), s = (dx dx + dy dy) + dz dz with every
 *   product and sum rounded on its own (no contraction), d = sqrt(s) correctly rounded.
 *   Bond order of a ligand pair i != j over the elements {H, C, N, O, F, P, S, Cl}, p = 100.0 d (pm), b1 / b2 / b3 the single / double /
 *   triple bond lengths of the pair in pm (-1: none):  p < b1 + 10 ?  (p < b2 + 5 ? (p < b3 + 3 ? 3 : 2) : 1)  : 0, comparisons strict.
 *   nr_bonds[i] = sum over j of order(i, j); atom i is stable iff allowed[z_i] >= nr_bonds[i] > 0 (a one-atom ligand is unstable).
 *   Clash of a pair: d < (r_lig + r_other) - 0.4 in fp64, in that order, r the van der Waals radius of the element (H C N O F P S Cl Br).
 *   Inter-clash: ligand atom x protein atom of the same graph, all pairs.  Intra-clash: ligand pairs i != j whose TABLE bond order is 0
 *   -- the reference masks with RDKit's bond adjacency instead; the table bond is this library's RDKit-free stand-in.
 *   A protein atom whose element has no radius takes no part and is counted.  A ligand atom outside the 8 elements has nr_bonds = 0, is
 *   unstable, takes no part in bonds or clashes (of other atoms either) and carries CBGX_GEOM_UNKNOWN_ELEMENT.
 *   Outputs, every element of every graph written (graphs without ligand or protein atoms too): nr_bonds [n_lig] int32; flags [n_lig]
 *   uint8 (bits below); graph_out [B, CBGX_GEOMETRY_GRAPH_COLS] int32: n_atoms, n_stable, mol_stable (n_stable == n_atoms && n_atoms > 0),
 *   n_inter_clash_atoms, n_intra_clash_atoms, n_protein_atoms_without_radius.  Integer results, no atomics on memory, no dependence on
 *   the order of anything: a graph's rows are a function of its own atoms.
 *   The pointers are device pointers.  The entry itself reads lig_ptr to find the largest ligand -- through a copy on `stream` and a
 *   wait for it when lig_ptr is device memory -- before the launch.
 *   Returns 0, and 0 without a launch when B == 0.  CBGX_E_INVALID, before anything is launched: a NULL pointer with a non-zero count,
 *   negative counts, a ligand above CBGX_GEOMETRY_MAX_LIGAND atoms (lig_ptr in plain host memory is read in place for this check, so that
 *   it needs no device; such a call is then refused as well: the kernel could not read it). */
#define CBGX_GEOMETRY_MAX_LIGAND 1024
#define CBGX_GEOMETRY_GRAPH_COLS 6
#define CBGX_GEOM_STABLE 1u          /* flags bit 0 */
#define CBGX_GEOM_INTER_CLASH 2u     /* bit 1: closer than the clash threshold to a protein atom */
#define CBGX_GEOM_INTRA_CLASH 4u     /* bit 2: closer than the clash threshold to a ligand atom it has no table bond with */
#define CBGX_GEOM_UNKNOWN_ELEMENT 8u /* bit 3: not one of H C N O F P S Cl */
int cbgx_ligand_geometry(const float *x_lig, const uint8_t *z_lig, const int32_t *lig_ptr, int n_lig, const float *x_rec,
                         const uint8_t *z_rec, const int32_t *rec_ptr, int n_rec, int n_graphs, int32_t *nr_bonds, uint8_t *flags,
                         int32_t *graph_out, void *stream);
/* The constants the kernel was built with (host only, no device): bond_pm [3][8][8] (order - 1, element code, element code), margins [3]
 *   (pm), allowed [8] valences, elements [8] the atomic number of each element code, vdw_z [9] / vdw_r [9] the atomic numbers that have a
 *   radius and the radii (Angstrom), tolerance (Angstrom).  A NULL argument is skipped.  Returns 0. */
int cbgx_ligand_geometry_tables(int32_t *bond_pm, int32_t *margins, int32_t *allowed, uint8_t *elements, uint8_t *vdw_z, double *vdw_r,
                                double *tolerance);

/* ---- table-bond graph of sampled ligands: bond list, fragments, connectivity (geometry.hip) ------------------------------------------------
 * What the reference learns about a sample only after RDKit / OpenBabel reconstruction -- which atoms are bonded, and whether the sample
 *   is one molecule or several pieces (repo/tools/rdkit_utils.py:597-640: clean_frags keeps the largest fragment, evaluate_validity calls
 *   a sample incomplete when its SMILES contains a '.') -- from the TABLE bonds of cbgx_ligand_geometry above: same arrays, same limit
 *   CBGX_GEOMETRY_MAX_LIGAND, same distance (fp32 widened to fp64, s = (dx dx + dy dy) + dz dz without contraction, d = sqrt(s) correctly
 *   rounded), same order (p = 100.0 d compared strictly with b + margin; pairs with s >= 25 skipped; an atom outside the eight elements
 *   has no bonds), same tables (cbgx_ligand_geometry_tables).  No aromaticity, no valence repair: these are not RDKit's bonds.  Proteins
 *   play no part.  One 256-thread workgroup per graph; a graph's rows are a function of its own atoms.
 * The number of bonds of a graph is not bounded by its number of atoms, so the list is made in two launches with a prefix sum between:
 * cbgx_ligand_bonds_count: deg_up [n_lig] int32 = the number of bonded partners j > i of atom i inside its ligand; fragment [n_lig] int32
 *   = the connected-component label of the atom, defined as the smallest ligand-local index in its component (an atom without bonds or
 *   with an unknown element is its own fragment); graph_out [B, CBGX_BONDS_GRAPH_COLS] int32: n_atoms, n_bonds (pairs i < j with order
 *   > 0), bond_order_sum (sum of the orders of those pairs), n_fragments, largest_fragment (atoms; 0 for an empty graph), n_cycles =
 *   n_bonds - n_atoms + n_fragments.  Every element of every graph is written.  Integer results; the components are the unique fixed point
 *   of min-label propagation, found in at most n_atoms rounds, independent of the order in which threads run.
 *   Checks, the lig_ptr read-back and return values as cbgx_ligand_geometry: CBGX_E_INVALID before any dereference or launch for negative
 *   counts, a NULL pointer with a non-zero count, a ligand above CBGX_GEOMETRY_MAX_LIGAND atoms (graph and size in the message), lig_ptr
 *   the device cannot read; 0 without a launch when B == 0.
 * cbgx_ligand_bonds_fill: bond_ptr [n_lig + 1] int32 = the exclusive prefix sum of deg_up, n_bonds = bond_ptr[n_lig]; bond_index
 *   [2, n_bonds] int32 global ligand rows with i < j (row 0: i, row 1: j); bond_order [n_bonds] uint8 in 1..3; bond_length [n_bonds] fp64
 *   = the d the order was decided on, in Angstrom.  Atom a writes its partners in ascending j at bond_ptr[a] ...: the list is in strict
 *   lexicographic (i, j) order, without atomics.  bond_ptr entries are clamped to [0, n_bonds] and made non-decreasing per atom: an atom
 *   writes at most bond_ptr[a + 1] - bond_ptr[a] entries and nothing at or beyond n_bonds, so a wrong bond_ptr loses bonds and never
 *   reaches outside the buffers.  Same checks; 0 without a launch when B == 0 or n_bonds == 0. */
#define CBGX_BONDS_GRAPH_COLS 6
int cbgx_ligand_bonds_count(const float *x_lig, const uint8_t *z_lig, const int32_t *lig_ptr, int n_lig, int n_graphs, int32_t *deg_up,
                            int32_t *fragment, int32_t *graph_out, void *stream);
int cbgx_ligand_bonds_fill(const float *x_lig, const uint8_t *z_lig, const int32_t *lig_ptr, int n_lig, int n_graphs,
                           const int32_t *bond_ptr, int n_bonds, int32_t *bond_index, uint8_t *bond_order, double *bond_length,
                           void *stream);

/* ---- ring sizes of the table-bond graph of sampled ligands (rings.hip) ------------------------------------------------------------------
 * What rings a sample's bond graph holds: the substructure diagnostic of the reference's quality path -- the share of molecules with a
 *   ring of size 3 ... 9 (evaluate_scripts/evaluate_geom_single.py:27-33, print_ring_ratio), rings of size k per molecule and the
 *   distribution over sizes 3 ... 8 (repo/tools/eval_ring_type.py, eval_ring_type_ratio / eval_ring_type_distribution) -- which the
 *   reference takes from RDKit's mol.GetRingInfo().AtomRings() after reconstruction.  Here: from the bond list of cbgx_ligand_bonds_fill,
 *   in ONE launch, one wave per graph, integer work only.
 *   lig_ptr [B + 1] int32 (entries clamped to [0, n_lig]); bond_ptr [n_lig + 1] int32 and bond_index [2, n_bonds] int32 as
 *   cbgx_ligand_bonds_fill defines them: global ligand rows, i < j, in strict (i, j) order.  Graph g's atoms are the rows lig_ptr[g] ...
 *   lig_ptr[g + 1], its bonds the entries bond_ptr[lig_ptr[g]] ... bond_ptr[lig_ptr[g + 1]] of the list.
 * Ring sizes: rings_k, k = 3 ... CBGX_RINGS_MAX_SIZE, is the number of cycles of length k in a minimum cycle basis of the graph.  The
 *   multiset of lengths of a minimum cycle basis is unique (the cycle space over GF(2) is a matroid), so rings_k does not depend on which
 *   basis is taken.  n_rings_larger = n_cycles - sum_k rings_k, n_cycles = n_bonds - n_atoms + n_components.  Computed as
 *   rings_k = rank(S_k) - rank(S_(k-1)), S_k the GF(2) span of the edge vectors of all closed walks P_v(x) + P_v(y) + xy with
 *   depth_v(x) + depth_v(y) + 1 <= k, over every root atom v and every bond xy that is not an edge of a breadth-first tree of v (any such
 *   tree, cut at depth 4; P_v: the tree path from v).  Horton's candidate set contains a minimum cycle basis, a degenerate candidate is a
 *   sum of cycles no longer than itself, and matroid greedy does the rest: the ranks depend neither on the trees nor on the order in which
 *   candidates of one length are inserted.
 *   This is the RDKit-free counterpart of the sizes of AtomRings(), which RDKit takes from its SSSR.  Deviations: these are table bonds;
 *   RDKit's SSSR is a heuristic that can differ from a minimum cycle basis on cage-like graphs.
 * atom_ring_min [n_lig] uint8: the length of the shortest cycle through the atom, 0 if there is none of length <= CBGX_RINGS_MAX_SIZE:
 *   the minimum of depth(x) + depth(y) + 1 over the non-tree bonds xy of the breadth-first tree rooted at the atom whose ends hang under
 *   different children of the root.
 * graph_out [B, CBGX_RINGS_GRAPH_COLS] int32: n_atoms, n_bonds, n_cycles, rings_3 ... rings_9, n_rings_larger, n_ring_atoms (atoms with
 *   atom_ring_min > 0), status.  Every element of both outputs is written for every graph, empty graphs and graphs without bonds included.
 * Limits, per graph, reported in status and never an error: more than CBGX_RINGS_MAX_ATOMS atoms (CBGX_RINGS_TOO_MANY_ATOMS); n_cycles
 *   above CBGX_RINGS_MAX_CYCLES (CBGX_RINGS_TOO_MANY_CYCLES; a graph within both limits has fewer than n_atoms + CBGX_RINGS_MAX_CYCLES
 *   bonds, and one with that many or more is refused before anything is built); a list that is not what cbgx_ligand_bonds_fill writes
 *   (CBGX_RINGS_BAD_BONDS): bond_ptr decreasing over the graph's atoms or outside [0, n_bonds], a bond of the graph's range whose rows
 *   are not i < j inside the graph's atom range, or bonds out of strict (i, j) order.  With status != 0 the columns n_cycles ...
 *   n_ring_atoms are -1 and atom_ring_min is 255 for the graph's atoms; n_atoms and n_bonds are the (clamped) sizes of the two ranges.
 *   Every entry of lig_ptr, bond_ptr and bond_index is clamped or checked before it is used as an index: no content of the three arrays
 *   makes the kernel read or write outside the buffers.  No atomics on memory; a graph's rows are a function of its own bonds.
 * Returns 0, and 0 without a launch when B == 0.  CBGX_E_INVALID before any dereference or launch: negative counts, a NULL pointer with
 *   a non-zero count (bond_index may be NULL when n_bonds == 0), lig_ptr the device cannot read. */
#define CBGX_RINGS_MAX_SIZE 9
#define CBGX_RINGS_MAX_ATOMS 256
#define CBGX_RINGS_MAX_CYCLES 128
#define CBGX_RINGS_GRAPH_COLS 13   /* n_atoms, n_bonds, n_cycles, rings_3 ... rings_9, n_rings_larger, n_ring_atoms, status */
#define CBGX_RINGS_TOO_MANY_ATOMS 1
#define CBGX_RINGS_TOO_MANY_CYCLES 2
#define CBGX_RINGS_BAD_BONDS 4
int cbgx_ligand_rings(const int32_t *lig_ptr, int n_lig, int n_graphs, const int32_t *bond_ptr, const int32_t *bond_index, int n_bonds,
                      uint8_t *atom_ring_min, int32_t *graph_out, void *stream);

/* ---- aromatic atoms and bonds of the table-bond graph of sampled ligands (aromatic.hip) -------------------------------------------------
 * What the reference's reconstruct_mol (repo/tools/rdkit_utils.py:522-590) makes of the model's per-atom aromatic flags (`add_aromatic`
 *   atom types): aromatic bonds, from three rules of its own -- fixup :380-389, the ring loop :552-572, the bond loop :574-579 -- that
 *   need elements, flags, bonds and small rings only.  Here: per ligand graph, on the bond list of cbgx_ligand_bonds_fill, in ONE launch,
 *   one wave per graph, integer work only.  lig_ptr, bond_ptr, bond_index as cbgx_ligand_rings takes them.
 * Inputs per atom: z_lig [n_lig] uint8 atomic numbers, flag_lig [n_lig] uint8 the model's flags (non-zero: flagged), atom_ring_min
 *   [n_lig] uint8 as cbgx_ligand_rings wrote it for the same list.
 * Cycles: C56 is every CHORDLESS (induced) simple cycle of length 5 or 6 of the bond graph: a cycle none of whose non-consecutive atoms
 *   are bonded.  That is what a ring perception reports on fused systems -- naphthalene's two hexagons and not its perimeter, norbornane's
 *   5, 5 and 6, nothing for the chorded perimeter of bicyclo[2.2.0]hexane -- and it involves no choice (networkx.chordless_cycles is an
 *   independent truth).
 * Closure: F is the smallest set of atoms that contains the flagged atoms and is closed under
 *   R2 (fixup): an atom with z = 7 or 8, with 3 <= atom_ring_min <= 9, and with at least two bonded neighbours in F, is in F;
 *   R3 (ring loop): if a cycle c of C56 has 2 |{a in c: z = 6, a in F}| >= |{a in c: z = 6}|, all atoms of c are in F.  A cycle without
 *     carbons satisfies the condition (0 >= 0), as in the reference: a ring of five nitrogens is in F with no flag at all.
 *   Both rules are monotone, so the least fixed point exists, is unique and does not depend on the order in which atoms or cycles are
 *   visited.  Deviation 1: the reference applies each rule once, in OpenBabel's atom and ring order; its result is contained in F, and
 *   equals F whenever no rule fires because of an earlier firing.
 * Aromatic cycle: a cycle of C56 all of whose atoms are in F.  aromatic_atom: the atom lies on an aromatic cycle.  aromatic_bond: the
 *   bond is an edge of an aromatic cycle.  Deviation 2: the bond between the rings of biphenyl is therefore NOT aromatic; the reference
 *   marks every bond with two aromatic ends (:574-579), and RDKit's sanitisation then rejects that molecule.
 *   bond_type = 4 for an aromatic bond, else the bond's order (made by the caller; elementwise on the list).
 * Outputs, dense, every element of every graph's ranges written: atom_out [n_lig] uint8 (bit 0: in F, bit 1: aromatic_atom),
 *   bond_aromatic [n_bonds] uint8 (0 / 1), graph_out [B, CBGX_AROMATIC_GRAPH_COLS] int32: n_atoms, n_bonds, n_cycles56,
 *   n_aromatic_cycles, n_flagged, n_closure (|F|), n_aromatic_atoms, n_aromatic_bonds, n_unsupported (flagged and not aromatic_atom: an
 *   aromatic type where the geometry built no ring to carry it), status.
 * Status, per graph, never an error: CBGX_AROMATIC_TOO_MANY_ATOMS (more than CBGX_AROMATIC_MAX_ATOMS atoms), CBGX_AROMATIC_BAD_BONDS
 *   (the conditions of CBGX_RINGS_BAD_BONDS), CBGX_AROMATIC_TOO_MANY_CYCLES (neither of those two and n_bonds >= n_atoms +
 *   CBGX_AROMATIC_MAX_CYCLES: the test cbgx_ligand_rings applies before staging), CBGX_AROMATIC_NO_RINGS (some atom of the graph has
 *   atom_ring_min == 255: the ring report did not evaluate the graph; set beside any of the others).  With status != 0 the columns
 *   n_cycles56 ... n_unsupported are -1 and the graph's bytes of atom_out and bond_aromatic are 255; n_atoms and n_bonds are the
 *   (clamped) sizes of the two ranges.  Every entry of lig_ptr, bond_ptr and bond_index is clamped or checked before it is used as an
 *   index: no content of the arrays makes the kernel read or write outside the buffers.  A graph writes its own (clamped) ranges; where
 *   a malformed bond_ptr or lig_ptr makes two graphs' ranges overlap, which of the two writes lasts is not defined.  No atomics on memory;
 *   nothing in the outputs depends on how the closure was scheduled.
 * Returns 0, and 0 without a launch when B == 0.  CBGX_E_INVALID before any dereference or launch: negative counts, a NULL pointer with
 *   a non-zero count (bond_index and bond_aromatic may be NULL when n_bonds == 0), lig_ptr the device cannot read. */
#define CBGX_AROMATIC_MAX_ATOMS 256
#define CBGX_AROMATIC_MAX_CYCLES 128
#define CBGX_AROMATIC_GRAPH_COLS 10   /* n_atoms, n_bonds, n_cycles56, n_aromatic_cycles, n_flagged, n_closure, n_aromatic_atoms, n_aromatic_bonds, n_unsupported, status */
#define CBGX_AROMATIC_TOO_MANY_ATOMS 1
#define CBGX_AROMATIC_TOO_MANY_CYCLES 2
#define CBGX_AROMATIC_BAD_BONDS 4
#define CBGX_AROMATIC_NO_RINGS 8
#define CBGX_AROMATIC_BOND_TYPES 256   /* ((type - 1) 8 + code_lo) 8 + code_hi, type 1 ... 4 */
#define CBGX_AROMATIC_ANGLE_TYPES 8192 /* (((code_1 4 + (t_1 - 1)) 8 + code_c) 4 + (t_2 - 1)) 8 + code_2 */
int cbgx_ligand_aromatic(const uint8_t *z_lig, const uint8_t *flag_lig, const uint8_t *atom_ring_min, const int32_t *lig_ptr, int n_lig,
                         int n_graphs, const int32_t *bond_ptr, const int32_t *bond_index, int n_bonds, uint8_t *atom_out,
                         uint8_t *bond_aromatic, int32_t *graph_out, void *stream);

/* ---- Kekule bond orders, implicit hydrogens and valence checks of the table-bond graph of sampled ligands (valence.hip) ----------------
 * Is the sample a molecule at all?  The reference decides that after reconstruct_mol (repo/tools/rdkit_utils.py:522-590), when RDKit
 *   kekulises the aromatic bonds, assigns implicit hydrogens and checks valences, and evaluate_validity (:615-640) adds "one piece".
 *   Here the same questions are answered on the bond list of cbgx_ligand_bonds_fill and the aromatic bonds of cbgx_ligand_aromatic, one
 *   launch, one wave per graph, integer work only.  Deviations: these are TABLE bonds (the reference's orders come from OpenBabel's
 *   geometric perception); the Kekule structure is chosen by a property (below), not by RDKit's traversal; no charges are modelled: a
 *   nitro group drawn N(=O)=O, an N-oxide and a quaternary N count as "valence exceeded".
 * Inputs: z_lig [n_lig] atomic numbers; lig_ptr [B + 1], bond_ptr [n_lig + 1], bond_index [2, n_bonds] as cbgx_ligand_rings takes them;
 *   bond_order [n_bonds] in 1..3; bond_aromatic [n_bonds] as cbgx_ligand_aromatic writes it: 1 aromatic, 255 not evaluated, anything else
 *   not aromatic; NULL means all 0 (8-type 'basic' configs); max_steps in 1 ... CBGX_VALENCE_MAX_STEPS.
 * Valence table (of this library; NOT the stability table of cbgx_ligand_geometry): H {1}, C {4}, N {3}, O {2}, F {1}, P {3, 5},
 *   S {2, 4, 6}, Cl {1}.  v0(z) is its smallest entry.
 * Aromatic system: a connected component of the graph formed by the bonds with bond_aromatic == 1.  For an atom a of a system: k(a) = the
 *   number of its aromatic bonds, s(a) = the sum of the orders of its other bonds, f(a) = v0(z_a) - s(a) - k(a).  a is a CANDIDATE if
 *   z in {6, 7} and f(a) >= 1, and a MUST atom if it is a candidate with z = 6.  (O, S and P never take a ring double bond: furan,
 *   thiophene.  A carbon with an exocyclic double bond has f = 0 and takes none: pyridone.)
 * Eligible bonds of a system: e_0 < ... < e_(m-1), its aromatic bonds both of whose ends are candidates, in list order.  last(a) = the
 *   largest p with a in e_p; n_c = the number of atoms that occur in them.
 * Kekule structure of a system: a set M of eligible bonds such that no two share an atom, every must atom is covered, M has the largest
 *   size among such sets, and among those of the largest size its sorted list of positions is lexicographically least.  (Imidazole's
 *   tautomer is decided by the order of the list; the largest size makes a two-neighbour N pyridine-type where it can be and N-H where
 *   it cannot.)  If no such M exists the system has FAILED (cyclopentadienyl).
 * Search -- written out because its step count is part of the interface.  A system with more than CBGX_VALENCE_MAX_ELIGIBLE eligible
 *   bonds, or more than CBGX_VALENCE_MAX_ELIGIBLE atoms in them, is not searched (SEARCH_LIMIT).  Otherwise, if a must atom occurs in
 *   no eligible bond the system fails in 1 step.  Otherwise node(0, {}, 0) runs, where node(p, M, dead) is:
 *     steps += 1;
 *     if p == m: best = M if there is no best yet or |M| > |best|; return;
 *     if best exists and |M| + floor((n_c - 2 |M| - dead) / 2) <= |best|: return;
 *     e_p = (i, j);
 *     include: if i and j are both unmatched by M: node(p + 1, M + {e_p}, dead);
 *     exclude: D = the ends of e_p that are unmatched by M and have last == p; if no atom of D is a must atom: node(p + 1, M, dead + |D|).
 *   Include-first order visits sets of equal size in lexicographic order: the first best of the final size is the required M; no best
 *   at the end: failed.  A search that would take more than max_steps steps is abandoned (SEARCH_LIMIT).
 * After the search: bond_kekule = 2 for the bonds of M and 1 for the other aromatic bonds of a solved system, 4 for every aromatic bond
 *   of a failed system, bond_order for every other bond.  v(a) = the sum of bond_kekule over a's bonds, a 4 counted as 1.  implicit_h(a) =
 *   (the smallest table entry >= v(a)) - v(a); without such an entry the atom is EXCEEDED and implicit_h = 0.  An atom outside the eight
 *   elements has the flag UNKNOWN_ELEMENT only and implicit_h 0 (the bond list holds no bond of such an atom).
 * Outputs, dense, every element of every graph's ranges written: implicit_h [n_lig] uint8; atom_flags [n_lig] uint8 (CBGX_VALENCE_EXCEEDED,
 *   _ON_FAILED_SYSTEM, _UNKNOWN_ELEMENT, _ON_AROMATIC_SYSTEM); bond_kekule [n_bonds] uint8; graph_out [B, CBGX_VALENCE_GRAPH_COLS] int32:
 *   n_atoms, n_bonds, n_fragments (the components of the bond list, every atom counted: column 3 of cbgx_ligand_bonds_count), n_systems,
 *   n_systems_failed, n_kekule_double, n_implicit_h, n_exceeded, n_unknown, n_nhoh (z in {7, 8} and implicit_h >= 1), n_no (z in {7, 8}),
 *   el_0 ... el_7 (atoms per element code H C N O F P S Cl), valence_ok (n_atoms > 0 and n_exceeded == n_unknown == n_systems_failed ==
 *   0), steps_max (the largest step count among the graph's systems, 0 without systems), status.
 * Status, per graph, never an error: CBGX_VALENCE_TOO_MANY_ATOMS (more than CBGX_VALENCE_MAX_ATOMS atoms), CBGX_VALENCE_BAD_BONDS (the
 *   conditions of CBGX_RINGS_BAD_BONDS, or a bond_order outside 1..3), CBGX_VALENCE_NO_AROMATIC (a bond of the graph has bond_aromatic ==
 *   255) -- these three are set side by side --, CBGX_VALENCE_SEARCH_LIMIT (none of those three, and a system that is not searched or
 *   whose search is abandoned).  With status != 0 the columns from n_fragments on, except status, are -1 and the graph's bytes of the
 *   three arrays are 255; n_atoms and n_bonds are the (clamped) sizes of the two ranges.  Every entry of lig_ptr, bond_ptr and
 *   bond_index is clamped or checked before it is used as an index, as in cbgx_ligand_aromatic, and overlapping ranges of a malformed
 *   lig_ptr or bond_ptr are undefined in the same way.  No atomics on memory; nothing in the outputs depends on scheduling.
 * Returns 0, and 0 without a launch when B == 0.  CBGX_E_INVALID before any dereference or launch: negative counts, max_steps outside
 *   1 ... CBGX_VALENCE_MAX_STEPS, a NULL pointer with a non-zero count (bond_index, bond_order and bond_kekule may be NULL when n_bonds
 *   == 0; bond_aromatic always), lig_ptr the device cannot read. */
#define CBGX_VALENCE_MAX_ATOMS 256
#define CBGX_VALENCE_MAX_ELIGIBLE 64
#define CBGX_VALENCE_MAX_STEPS 65536
#define CBGX_VALENCE_GRAPH_COLS 22   /* n_atoms, n_bonds, n_fragments, n_systems, n_systems_failed, n_kekule_double, n_implicit_h, n_exceeded, n_unknown, n_nhoh, n_no, el_0 ... el_7, valence_ok, steps_max, status */
#define CBGX_VALENCE_EXCEEDED 1
#define CBGX_VALENCE_ON_FAILED_SYSTEM 2
#define CBGX_VALENCE_UNKNOWN_ELEMENT 4
#define CBGX_VALENCE_ON_AROMATIC_SYSTEM 8
#define CBGX_VALENCE_TOO_MANY_ATOMS 1
#define CBGX_VALENCE_BAD_BONDS 4
#define CBGX_VALENCE_NO_AROMATIC 8
#define CBGX_VALENCE_SEARCH_LIMIT 16
int cbgx_ligand_valence(const uint8_t *z_lig, const int32_t *lig_ptr, int n_lig, int n_graphs, const int32_t *bond_ptr,
                        const int32_t *bond_index, const uint8_t *bond_order, const uint8_t *bond_aromatic, int n_bonds, int max_steps,
                        uint8_t *implicit_h, uint8_t *atom_flags, uint8_t *bond_kekule, int32_t *graph_out, void *stream);

/* ---- typed pocket contacts and a score in Vina's functional form (interactions.hip) -----------------------------------------------------
 * How well does the sample sit in its pocket?  The reference answers with `vina_task.run(mode='score_only')`
 *   (evaluate_scripts/evaluate_chem_single.py:44-49) and the PLIP contact counts of repo/tools/interaction.py, behind RDKit, OpenBabel,
 *   meeko, Vina and PLIP.  Here: the five pair terms of the published Vina scoring function (O. Trott, A. J. Olson, "AutoDock Vina:
 *   improving the speed and accuracy of docking with a new scoring function, efficient optimization, and multithreading", J. Comput.
 *   Chem. 31 (2010) 455-461: gauss1, gauss2, repulsion, hydrophobic, hydrogen bonding over surface distances, cutoff 8 A, the radii
 *   below; its weights -0.035579, -0.005156, 0.840245, -0.035069, -0.587439 and 0.05846 per rotatable bond are applied by the caller) on
 *   THIS LIBRARY'S OWN atom typing, in two launches, one workgroup per graph.  It is a score in Vina's functional form and NOT a
 *   reproduction of the Vina program: it has not been validated against it and nothing may claim agreement with it.
 *   Deviations: TABLE bonds (cbgx_ligand_bonds_fill), Kekule orders and hydrogens of cbgx_ligand_valence; pocket types from a residue
 *   table, with no hydrogens in the file and no protonation states (HIS is always donor + acceptor); this library's own acceptor rule for
 *   N; no intramolecular term, no metals, no Br / I; rotatable bonds by RDKit's NON-strict pattern (the reference's obey_lipinski uses the
 *   strict one).
 * A type byte: element code 1 ... 7 (C N O F P S Cl) in the bits of CBGX_INTERACTIONS_ELEMENT_MASK, and CBGX_INTERACTIONS_HYDROPHOBIC,
 *   _DONOR, _ACCEPTOR.  0: the atom takes no part (H; a ligand atom of no known element).  CBGX_INTERACTIONS_UNTYPED: a pocket atom that
 *   takes no part and is counted.  An atom takes part in the pair terms iff its byte is in 1 ... 63 with a non-zero element code.
 * Distances and table bonds are cbgx_ligand_geometry's: fp32 coordinates widened to fp64, s = (dx dx + dy dy) + dz dz with every
 *   operation rounded on its own, r = sqrt(s) correctly rounded, contraction off; order >= 1 iff 100.0 r < b1 + 10 (pm), strictly.
 *
 * cbgx_pocket_types -- rec_type [n_rec] uint8 from x_rec [n_rec, 3], z_rec [n_rec] atomic numbers, rec_ptr [B + 1] (as
 *   cbgx_ligand_geometry takes them; the range of a graph is clamped to the arrays; any number of atoms), rec_aa [n_rec] uint8 (an index
 *   into the reference's aa_name_number order: ALA 0, CYS 1, ASP 2, GLU 3, PHE 4, GLY 5, HIS 6, ILE 7, LYS 8, LEU 9, MET 10, ASN 11,
 *   PRO 12, GLN 13, ARG 14, SER 15, THR 16, VAL 17, TRP 18, TYR 19; anything else is "other"), rec_backbone [n_rec] uint8 (non-zero: a
 *   backbone atom).  H: 0.  An element outside H C N O S (Se included): CBGX_INTERACTIONS_UNTYPED.  N: backbone: donor, except PRO (none);
 *   side chain of LYS, ARG, ASN, GLN, TRP: donor; of HIS: donor + acceptor; any other: neither.  O: acceptor; side chain of SER, THR, TYR:
 *   donor + acceptor (ASP / GLU / ASN / GLN and a terminal OXT: acceptor).  S: no bit.  C: hydrophobic unless it has a table bond
 *   (order >= 1) to an N, O or S protein atom of the same graph.
 *
 * cbgx_ligand_interactions -- inputs: x_lig, z_lig, lig_ptr, x_rec, rec_ptr as above; rec_type as written by cbgx_pocket_types; bond_ptr
 *   [n_lig + 1], bond_index [2, n_bonds] as cbgx_ligand_rings takes them; bond_kekule, implicit_h, atom_flags as cbgx_ligand_valence
 *   writes them; valence_status [B] int32, the status column of its graph_out; bond_aromatic [n_bonds] as cbgx_ligand_valence takes it
 *   (1: aromatic; NULL: no bond is).
 *   Ligand types, with h(a) = implicit_h(a) + the number of a's H neighbours in the bond list and heavy(a) = the number of its other
 *   neighbours: H: 0.  C: hydrophobic unless bonded to an atom that is neither C nor H.  F, Cl: hydrophobic.  P, S: no bit.  O: acceptor;
 *   donor iff h > 0.  N: donor iff h > 0; acceptor iff h == 0 and heavy <= 2 and no CBGX_VALENCE_EXCEEDED flag (pyridine, imine, nitrile;
 *   not a tertiary amine, not an amide).  Any other element: 0.
 *   Rotatable bonds: bond_rotatable = 1 iff bond_kekule == 1 and bond_aromatic != 1, the bond is a bridge of the bond graph (it lies on no
 *   cycle), both ends have heavy >= 2 and neither end has a bond with bond_kekule == 3; else 0.  (RDKit's non-strict
 *   [!$(*#*)&!D1]-&!@[!$(*#*)&!D1] on table bonds.)
 *   Pair terms: for every ligand atom i and pocket atom j of the same graph that both take part, with r < 8.0 strictly:
 *   d = (r - R_i) - R_j, radii in A by element C 1.9, N 1.8, O 1.7, P 2.1, S 2.0, F 1.5, Cl 1.8;
 *     0 gauss1       exp(-(q q)), q = d / 0.5                                        every pair
 *     1 gauss2       exp(-(q q)), q = (d - 3.0) / 2.0                                every pair
 *     2 repulsion    d d if d < 0, else 0                                            every pair
 *     3 hydrophobic  1 if d < 0.5; 1.5 - d if d < 1.5; else 0                        both atoms hydrophobic
 *     4 hbond        1 if d < -0.7; (-d) / 0.7 if d < 0; else 0                      one atom a donor and the other an acceptor
 *   Outputs, dense, every element of every graph's ranges written: atom_terms [n_lig, 5] fp64, a ligand atom's sums over the pocket
 *   (zeros for an atom that takes no part); lig_type [n_lig] uint8; bond_rotatable [n_bonds] uint8; graph_terms [B, 5] fp64;
 *   graph_out [B, CBGX_INTERACTIONS_GRAPH_COLS] int32: n_atoms, n_bonds, n_rotatable, n_donors, n_acceptors, n_hydrophobic_atoms (ligand
 *   atoms with the bit), n_pairs (within 8 A), n_hbond_pairs (hbond term > 0), n_hydrophobic_pairs (hydrophobic term > 0), n_close_pairs
 *   (d < 0 and not a donor-acceptor pair), n_contact_atoms (ligand atoms with any pair at d < 0.5), n_protein_untyped (rec_type ==
 *   CBGX_INTERACTIONS_UNTYPED in the graph's pocket), status.
 *   Order of every floating sum (a function of the graph's own sizes only; no float atomics; the bits of a graph's outputs do not depend
 *   on what else is in the batch or where the graph stands in it): atom_terms[i][t] = (p_0 + p_1) + (p_2 + p_3), where p_s starts at 0.0
 *   and adds the pairs of i with the pocket atoms j = s, s + 4, s + 8, ... (j counted from the graph's first pocket atom) in ascending j;
 *   pocket atoms that take no part and pairs with r >= 8 are skipped.  graph_terms[g][t] = ((0.0 + a_0) + a_1) + ... over the graph's
 *   ligand atoms in ascending order.  exp is the device library's fp64 exp.
 *   Status, per graph, never an error, set side by side: CBGX_INTERACTIONS_TOO_MANY_ATOMS (more than CBGX_INTERACTIONS_MAX_ATOMS ligand
 *   atoms), CBGX_INTERACTIONS_BAD_BONDS (the conditions of CBGX_RINGS_BAD_BONDS, or -- where valence_status == 0 -- a bond_kekule outside
 *   1..4), CBGX_INTERACTIONS_NO_VALENCE (valence_status != 0).  With status != 0 the columns from n_rotatable on, except status, are -1,
 *   the graph's floats NaN and its bytes of lig_type and bond_rotatable 255; n_atoms and n_bonds are the (clamped) sizes of the two
 *   ranges.  Every entry of lig_ptr, rec_ptr, bond_ptr and bond_index is clamped or checked before it is used as an index.
 *   Clamping keeps every access inside the arrays; it does NOT make the ranges of different graphs disjoint.  A lig_ptr, rec_ptr or
 *   bond_ptr that decreases from one graph to the next (lig_ptr = 0, 10, 5, 12) gives two graphs overlapping ranges: both kernels then
 *   have two workgroups write the same elements of atom_terms, lig_type, bond_rotatable or rec_type, in no order, and those elements are
 *   undefined (in bounds, and each graph's own row of graph_terms and graph_out is still what its range gives), as in
 *   cbgx_ligand_aromatic and cbgx_ligand_valence.  Non-decreasing pointers, which is what the Python side builds, never overlap.
 * Both return 0, and 0 without a launch when B == 0.  CBGX_E_INVALID before any dereference or launch: negative counts, a NULL pointer
 *   with a non-zero count (the per-bond arrays may be NULL when n_bonds == 0; bond_aromatic always), and any array with a non-zero count
 *   whose pointer is not memory the device can read (plain host memory: every pointer argument is asked for, in argument order, and
 *   the first such array is named in cbgx_last_error). */
#define CBGX_INTERACTIONS_MAX_ATOMS 256
#define CBGX_INTERACTIONS_TERMS 5
#define CBGX_INTERACTIONS_GRAPH_COLS 13   /* n_atoms, n_bonds, n_rotatable, n_donors, n_acceptors, n_hydrophobic_atoms, n_pairs, n_hbond_pairs, n_hydrophobic_pairs, n_close_pairs, n_contact_atoms, n_protein_untyped, status */
#define CBGX_INTERACTIONS_ELEMENT_MASK 7
#define CBGX_INTERACTIONS_HYDROPHOBIC 8
#define CBGX_INTERACTIONS_DONOR 16
#define CBGX_INTERACTIONS_ACCEPTOR 32
#define CBGX_INTERACTIONS_UNTYPED 64
#define CBGX_INTERACTIONS_TOO_MANY_ATOMS 1
#define CBGX_INTERACTIONS_BAD_BONDS 4
#define CBGX_INTERACTIONS_NO_VALENCE 8
int cbgx_pocket_types(const float *x_rec, const uint8_t *z_rec, const int32_t *rec_ptr, int n_rec, int n_graphs, const uint8_t *rec_aa,
                      const uint8_t *rec_backbone, uint8_t *rec_type, void *stream);
int cbgx_ligand_interactions(const float *x_lig, const uint8_t *z_lig, const int32_t *lig_ptr, int n_lig, const float *x_rec,
                             const uint8_t *rec_type, const int32_t *rec_ptr, int n_rec, int n_graphs, const int32_t *bond_ptr,
                             const int32_t *bond_index, const uint8_t *bond_kekule, const uint8_t *bond_aromatic, int n_bonds,
                             const uint8_t *implicit_h, const uint8_t *atom_flags, const int32_t *valence_status, double *atom_terms,
                             uint8_t *lig_type, uint8_t *bond_rotatable, double *graph_terms, int32_t *graph_out, void *stream);

/* ---- functional groups of the table-bond graph of sampled ligands (groups.hip) -----------------------------------------------------------
 * Which functional groups does the sample hold?  The reference counts them with `EFGs.mol2frag` after RDKit reconstruction
 *   (repo/tools/eval_fg_type.py; evaluate_scripts/evaluate_substruct_single.py) and compares 25 named ones with a dataset.  Here: a
 *   partition of the bond graph into groups by marking rules in the manner of P. Ertl ("An algorithm to identify functional groups in
 *   organic molecules", J. Cheminform. 9 (2017) 36), and an exact graph-isomorphism test of every group against 25 template graphs.  One
 *   launch, one wave per graph, integer work only.  Deviations: TABLE bonds (cbgx_ligand_bonds_fill) and this library's aromatic bonds
 *   (cbgx_ligand_aromatic); marking rules of this library's own, NOT the EFGs program: nothing may claim agreement with it; no charges
 *   (a nitro group is the graph N(=O)=O); a group of a single atom (an ether O, an amine N, a halogen) is `other`.
 * Inputs: z_lig, lig_ptr, bond_ptr, bond_index, bond_order (1..3), bond_aromatic (1 aromatic, 255 not evaluated, anything else not
 *   aromatic; NULL: no bond is aromatic) as cbgx_ligand_valence takes them.  The TYPE of a bond is t = 4 if bond_aromatic == 1, else its
 *   order.  No Kekule structure and no hydrogens are needed.
 * Atom kinds: an atom is AROMATIC if it has a bond of type 4, HETERO if it is N, O, F, P, S or Cl.  H atoms and atoms outside the eight
 *   elements belong to no group (their bonds still make their partners aromatic, or unsaturated under (a)).
 * Members: every aromatic atom, every hetero atom, and a non-aromatic carbon for which one of these holds:
 *   (a) it has a bond of type 2 or 3;
 *   (b) acetal: all its bonds are type 1, and at least two of its neighbours are non-aromatic N, O or S atoms all of whose own bonds are
 *       type 1;
 *   (c) it lies on a triangle of bonds, none of type 4, one of whose atoms is N, O or S (oxirane, aziridine, thiirane).
 * Group bonds: a bond between two members is a group bond iff it has type 4, or neither end is aromatic, or exactly one end is aromatic
 *   and the type is 2 (an exocyclic double bond: pyridone, uracil).  A single bond from a ring to a substituent is none (phenol: a ring
 *   and an O), nor is a non-aromatic bond between two aromatic atoms (biphenyl: two rings).
 * Groups: the connected components of the members under the group bonds.  The labelled graph of a group: its atoms as (element code,
 *   aromatic bit) and its group bonds with their types; a bond between two atoms of a group that is no group bond is not part of it.
 * Classes: 25 named ones, in the order and under the names of the reference's vocabulary, and other = CBGX_GROUPS_CLASSES:
 *    0 c1ccccc1   1 NC=O   2 O=CO   3 c1ccncc1   4 c1ncc2nc[nH]c2n1   5 NS(=O)=O   6 O=P(O)(O)O   7 OCO   8 c1cncnc1   9 c1cn[nH]c1
 *   10 O=P(O)O   11 c1ccc2ccccc2c1   12 c1ccsc1   13 N=CN   14 NC(N)=O   15 O=c1cc[nH]c(=O)[nH]1   16 c1ccc2ncccc2c1   17 c1cscn1
 *   18 c1ccc2[nH]cnc2c1   19 c1c[nH]cn1   20 O=[N+][O-]   21 O=CNO   22 NC(=O)O   23 O=S=O   24 c1ccc2[nH]ccc2c1
 *   Each name stands for one template graph in the same labelling (csrc/geo_tables.h; cbgx_ligand_groups_templates hands it out):
 *   lower-case atoms are aromatic and their ring bonds type 4; [nH] is an aromatic N like any other (hydrogens and tautomers play no
 *   part); O=[N+][O-] is N(=O)=O; OCO is O-C-O with single bonds.  A group has class k iff its labelled graph is isomorphic to template
 *   k, elements, aromatic bits and bond types preserved; a group of more than CBGX_GROUPS_MAX_TEMPLATE_ATOMS atoms is `other` without a
 *   test; everything else is `other`.  The class is a property: no step budget is part of the interface.
 * Outputs, dense, every element of every graph's ranges written: atom_group [n_lig] int32, the graph-local index of the smallest atom of
 *   the atom's group, -1 for an atom in no group; atom_class [n_lig] uint8, the class of its group 0 ... 25, CBGX_GROUPS_NO_GROUP for an
 *   atom in no group; graph_out [B, CBGX_GROUPS_GRAPH_COLS] int32: n_atoms, n_bonds, n_groups, n_group_atoms, n_named (groups of class <
 *   25), largest_group (atoms; 0 without groups), fg_0 ... fg_24, n_other, status.
 * Status, per graph, never an error, set side by side: CBGX_GROUPS_TOO_MANY_ATOMS (more than CBGX_GROUPS_MAX_ATOMS atoms),
 *   CBGX_GROUPS_BAD_BONDS (the conditions of CBGX_RINGS_BAD_BONDS, or a bond_order outside 1..3), CBGX_GROUPS_NO_AROMATIC (a bond of the
 *   graph has bond_aromatic == 255).  With status != 0 the columns from n_groups on, except status, are -1, the graph's bytes of
 *   atom_class are 255 and its entries of atom_group -2; n_atoms and n_bonds are the (clamped) sizes of the two ranges.  Every entry of
 *   lig_ptr, bond_ptr and bond_index is clamped or checked before it is used as an index, and overlapping ranges of a malformed lig_ptr
 *   or bond_ptr are undefined as in cbgx_ligand_valence.  No atomics on memory; nothing in the outputs depends on scheduling.
 * Returns 0, and 0 without a launch when B == 0.  CBGX_E_INVALID before any dereference or launch: negative counts, a NULL pointer with a
 *   non-zero count (bond_index and bond_order may be NULL when n_bonds == 0; bond_aromatic always), and any array with a non-zero count
 *   whose pointer is not memory the device can read (plain host memory; asked for in argument order, the first such array is named in
 *   cbgx_last_error).
 * cbgx_ligand_groups_templates (host only): n_atoms [25] uint8, n_bonds [25] uint8, labels [25, 10] uint8 ((element code << 1) |
 *   aromatic bit; codes H C N O F P S Cl = 0 ... 7), bonds [25, 11, 3] uint8 (atom, atom, type); unused entries 0. */
#define CBGX_GROUPS_MAX_ATOMS 256
#define CBGX_GROUPS_CLASSES 25
#define CBGX_GROUPS_MAX_TEMPLATE_ATOMS 10
#define CBGX_GROUPS_MAX_TEMPLATE_BONDS 11
#define CBGX_GROUPS_NO_GROUP 254
#define CBGX_GROUPS_GRAPH_COLS 33   /* n_atoms, n_bonds, n_groups, n_group_atoms, n_named, largest_group, fg_0 ... fg_24, n_other, status */
#define CBGX_GROUPS_TOO_MANY_ATOMS 1
#define CBGX_GROUPS_BAD_BONDS 4
#define CBGX_GROUPS_NO_AROMATIC 8
int cbgx_ligand_groups(const uint8_t *z_lig, const int32_t *lig_ptr, int n_lig, int n_graphs, const int32_t *bond_ptr,
                       const int32_t *bond_index, const uint8_t *bond_order, const uint8_t *bond_aromatic, int n_bonds,
                       int32_t *atom_group, uint8_t *atom_class, int32_t *graph_out, void *stream);
int cbgx_ligand_groups_templates(uint8_t *n_atoms, uint8_t *n_bonds, uint8_t *labels, uint8_t *bonds);

/* ---- fingerprints of sampled ligands, and uniqueness and Tanimoto similarity across the samples of a pocket (diversity.hip) ---------------
 * Does a pocket's set of samples hold different molecules?  The reference's raw material is RDKit after reconstruction: `tanimoto_sim` /
 *   `tanimoto_sim_N_to_1` on `Chem.RDKFingerprint` (repo/tools/similarity.py) and the SMILES strings of evaluate_chem_single.py.  Here:
 *   a fingerprint and a hash of this library's own, by colour refinement of the table-bond graph in the manner of ECFP4, and a second
 *   kernel that compares the graphs of a group.  Integer work only, on unsigned 64-bit integers with wrap-around; every number is a
 *   function of the graph's own atoms and bonds and of no order among them.  Deviations: TABLE bonds and this library's aromatic bonds;
 *   the fingerprint is NEITHER RDKit's Morgan fingerprint NOR `RDKFingerprint`: nothing may claim agreement with them.
 * cbgx_ligand_fingerprints -- one launch, one wave per graph.
 *   Inputs: z_lig, lig_ptr, bond_ptr, bond_index as cbgx_ligand_groups takes them; bond_type [n_bonds] uint8: 1..3 the order, 4 aromatic,
 *   255 = the aromatic report did not evaluate the graph (with atom types without aromatic flags: the order); atom_ring_min [n_lig] uint8
 *   as cbgx_ligand_rings writes it: 0 = no ring of length <= 9 through the atom, 255 = not evaluated.
 *   G = 0x9E3779B97F4A7C15.  mix(x), the splitmix64 finaliser: x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27;
 *   x *= 0x94D049BB133111EB; x ^= x >> 31.  For atom a with atomic number z: deg = the number of bonds of the graph it appears in,
 *   arom = 1 iff one of them has type 4, ring = its atom_ring_min;
 *     id_0(a) = mix(G + z + 256 deg + 65536 arom + 131072 ring)
 *     id_(r+1)(a) = mix(id_r(a) + sum over the bonds a - b of type t of mix(id_r(b) ^ (t G)))
 *   for r = 0 ... R - 1 with R = max(n_atoms, 2): a property of the graph (a refinement is stable after n_atoms rounds at the latest), not
 *   a budget.  The sum is commutative: no order of atoms or bonds enters.
 *   fp [B, CBGX_FINGERPRINT_WORDS] uint32, CBGX_FINGERPRINT_BITS bits: bit id_r(a) & 1023 is set for every atom and r = 0, 1, 2 (the
 *   atom, its neighbours, theirs: the radius of ECFP4); bit b is bit b & 31 of word b >> 5.
 *   mol_hash [B] uint64 = mix(sum over the atoms of mix(id_R(a) ^ G) + n_atoms + (n_bonds << 32)).
 *   What the hash means: equal hashes say that the two graphs are equivalent under this colour refinement (1-dimensional
 *   Weisfeiler-Leman on the labels above), up to collisions of 64-bit values.  That is NOT a proof of isomorphism.  The ring term is an
 *   input because without it cyclohexane and two cyclopropanes are equivalent, and so are decalin and bicyclopentyl; a known blind spot
 *   that remains: unsubstituted macrocycles of more than CBGX_RINGS_MAX_SIZE atoms with equal atom counts (one C20 ring against two C10
 *   rings) get equal hashes.
 *   graph_out [B, CBGX_FINGERPRINT_GRAPH_COLS] int32: n_atoms, n_bonds (the clamped sizes of the two ranges), n_bits (bits set in the
 *   graph's row of fp), n_rounds (R), status.  Every element of fp, mol_hash and graph_out is written for every graph.
 *   Status, per graph, never an error, set side by side: CBGX_FINGERPRINT_TOO_MANY_ATOMS (more than CBGX_FINGERPRINT_MAX_ATOMS atoms),
 *   CBGX_FINGERPRINT_BAD_BONDS (the conditions of CBGX_RINGS_BAD_BONDS, or a bond_type outside 1..4 that is not 255),
 *   CBGX_FINGERPRINT_NO_TYPES (a 255 among the graph's bytes of bond_type or atom_ring_min), CBGX_FINGERPRINT_EMPTY (no atom).  With
 *   status != 0 the graph's row of fp is all zero, its mol_hash 0, n_bits and n_rounds -1.  There is no limit on the bonds.  Every entry of
 *   lig_ptr, bond_ptr and bond_index is clamped or checked before it is used as an index.  No atomics on memory; nothing in the outputs
 *   depends on scheduling.
 *   Returns 0, and 0 without a launch when B == 0.  CBGX_E_INVALID before any dereference or launch: negative counts, a NULL pointer with
 *   a non-zero count (bond_index and bond_type may be NULL when n_bonds == 0), and any array with a non-zero count whose pointer is not
 *   memory the device can read (asked for in argument order, the first such array is named in cbgx_last_error).
 * cbgx_group_diversity -- one launch, one workgroup per group.
 *   Inputs: fp (16-byte aligned) and mol_hash as above; status [B] int32, the status column; group_ptr [P + 1] int32, a CSR over graphs:
 *   group p holds the consecutive graphs group_ptr[p] ... group_ptr[p + 1] (entries clamped to [0, B], an end below its start to the
 *   start: reported as CBGX_DIVERSITY_BAD_GROUPS, the clamped range is evaluated); pair_ptr [P + 1] int64 with pair_ptr[p + 1] -
 *   pair_ptr[p] = n_p (n_p - 1) / 2, n_p the (clamped) size of group p, computed by the caller; n_pairs, the length of pair_sim.  A group
 *   whose range of pair_ptr is not that long or does not lie inside [0, n_pairs] carries CBGX_DIVERSITY_BAD_GROUPS too, and nothing of
 *   pair_sim is written for it.  A graph is evaluated iff its status is 0.
 *   For two evaluated graphs i < j of a group (group-local indices): inter = popcount(fp_i & fp_j), uni = popcount(fp_i | fp_j),
 *   sim_micro = (inter 1000000 + uni / 2) / uni in integer division: the Tanimoto similarity in millionths, rounded half up.  uni >= 1
 *   for rows cbgx_ligand_fingerprints wrote (an evaluated graph has an atom); two all-zero rows of a caller's own have sim_micro 0.
 *   pair_sim [n_pairs] int32: the group's pairs in (i, j) order from pair_ptr[p] on, -1 where either graph is not evaluated.
 *   Per graph (int32 [B] each; -1 in all three for a graph that is not evaluated; a graph in no group is not written): first_same, the
 *   group-local index of the first evaluated graph of the group with the same mol_hash (its own index if none is earlier); nearest, the
 *   group-local index of the evaluated graph j != i of largest sim_micro, the smallest index on ties, -1 if there is none;
 *   nearest_micro, that similarity (-1 if there is none).
 *   group_out [P, CBGX_DIVERSITY_GROUP_COLS] int64: n_graphs, n_evaluated, n_unique (graphs that are their own first_same), n_pairs (pairs
 *   of evaluated graphs), sim_micro_sum, sim_micro_max (-1 without a pair), status.  A group of more than CBGX_DIVERSITY_MAX_GROUP graphs
 *   carries CBGX_DIVERSITY_TOO_MANY_GRAPHS: its columns n_evaluated ... sim_micro_max are -1, and so are its per-graph outputs and pairs.
 *   Every number is a sum, a minimum or a maximum of integers: nothing depends on scheduling.  No atomics on memory.  Overlapping groups
 *   have two workgroups write the same per-graph elements, in no order: those elements are undefined.
 *   Returns 0, and 0 without a launch when P == 0.  CBGX_E_INVALID before any dereference or launch: negative counts, a NULL pointer with
 *   a non-zero count (the per-graph arrays with B, group_ptr, pair_ptr and group_out with P, pair_sim with n_pairs), an fp that is not
 *   16-byte aligned, and any array with a non-zero count whose pointer is not memory the device can read, named as above. */
#define CBGX_FINGERPRINT_MAX_ATOMS 256
#define CBGX_FINGERPRINT_BITS 1024
#define CBGX_FINGERPRINT_WORDS 32
#define CBGX_FINGERPRINT_GRAPH_COLS 5   /* n_atoms, n_bonds, n_bits, n_rounds, status */
#define CBGX_FINGERPRINT_TOO_MANY_ATOMS 1
#define CBGX_FINGERPRINT_BAD_BONDS 4
#define CBGX_FINGERPRINT_NO_TYPES 8
#define CBGX_FINGERPRINT_EMPTY 16
#define CBGX_DIVERSITY_MAX_GROUP 1024
#define CBGX_DIVERSITY_GROUP_COLS 7   /* n_graphs, n_evaluated, n_unique, n_pairs, sim_micro_sum, sim_micro_max, status */
#define CBGX_DIVERSITY_TOO_MANY_GRAPHS 1
#define CBGX_DIVERSITY_BAD_GROUPS 4
int cbgx_ligand_fingerprints(const uint8_t *z_lig, const int32_t *lig_ptr, int n_lig, int n_graphs, const int32_t *bond_ptr,
                             const int32_t *bond_index, const uint8_t *bond_type, const uint8_t *atom_ring_min, int n_bonds, uint32_t *fp,
                             uint64_t *mol_hash, int32_t *graph_out, void *stream);
int cbgx_group_diversity(const uint32_t *fp, const uint64_t *mol_hash, const int32_t *status, const int32_t *group_ptr,
                         const int64_t *pair_ptr, int n_graphs, int n_groups, long long n_pairs, int32_t *pair_sim, int32_t *first_same,
                         int32_t *nearest, int32_t *nearest_micro, int64_t *group_out, void *stream);

/* ---- samples against the ligand a pocket was crystallised with (native.hip) ----------------------------------------------------------------
 * The reference reports its interaction numbers relative to the pocket's own ligand (evaluate_scripts/cal_chem_results.py,
 *   calculate_vina_metrics).  The native ligand goes through the entries above like a sample; these two say which pocket atoms a ligand
 *   touches and where it sits, and compare every sample of a pocket with the pocket's native ligand.  The contact set, its Jaccard
 *   index and the centroid distance are descriptors of this library's own: the reference has no counterpart.
 * cbgx_pocket_contacts -- one launch, one workgroup per graph; any pocket size, a ligand of at most CBGX_GEOMETRY_MAX_LIGAND atoms.
 *   Inputs: x_lig [n_lig, 3] / x_rec [n_rec, 3] float32, z_lig / z_rec atomic numbers as bytes, lig_ptr / rec_ptr [B + 1] int32 (entries
 *   clamped to their arrays, an end below its start to the start), cutoff2 (double; CBGX_CONTACTS_CUTOFF2 = 16.0 = (4 A)^2 is the default
 *   of the Python side).  An atom is HEAVY iff its atomic number is not 1; hydrogens on either side take no part.
 *   A heavy ligand atom l and a heavy pocket atom r of one graph are in CONTACT iff d2 <= cutoff2 with
 *     dx = (double)x_l - (double)x_r (exact; dy, dz likewise), d2 = (dx dx + dy dy) + dz dz,
 *   every product and sum rounded to float64 once, nothing fused: the distance of cbgx_ligand_geometry.  A NaN d2 or cutoff2 is no contact.
 *   rec_contact [n_rec] uint8: 1 iff some heavy ligand atom of the graph is in contact with that pocket atom, else 0.
 *   lig_contact [n_lig] uint8: the same from the ligand's side.  Atoms in no graph's range are not written.
 *   centroid [B, 3] float64: per component s = 0.0; s = s + (double)x_a for the graph's heavy atoms a in atom order, one float64 addition
 *   after the other; centroid = s / (double)n_heavy (one IEEE division).  NaN in all three without a heavy atom.
 *   graph_out [B, CBGX_CONTACTS_GRAPH_COLS] int32: n_atoms, n_heavy, n_rec (the clamped sizes of the ranges), n_rec_contact,
 *   n_lig_contact, status: CBGX_CONTACTS_EMPTY without a heavy ligand atom, never an error.  Every output is written for every graph:
 *   bytes 0 and counts 0 on an empty one.  No atomics on memory; nothing depends on scheduling.
 *   Returns 0, and 0 without a launch when B == 0.  CBGX_E_INVALID before any launch: negative counts, a NULL pointer with a non-zero
 *   count, a graph of more than CBGX_GEOMETRY_MAX_LIGAND ligand atoms (lig_ptr is read back, as cbgx_ligand_geometry does), and any
 *   array with a non-zero count whose pointer is not memory the device can read (the first such array is named in cbgx_last_error).
 * cbgx_native_compare -- one launch, one workgroup per pocket; integer work and one float64 distance per sample.
 *   Inputs for the B sample graphs: fp [B, 32] (16-byte aligned), mol_hash [B], fp_status [B] int32 (the status column of
 *   cbgx_ligand_fingerprints), rec_contact [n_rec] with rec_ptr [B + 1], centroid [B, 3], contacts_status [B] int32 (the status column
 *   above).  The same six for the P native ligands, one per pocket (fp_nat ... contacts_status_nat, rec_ptr_nat [P + 1], n_rec_nat).
 *   group_ptr [P + 1] int32: the samples of pocket p are the consecutive graphs group_ptr[p] ... group_ptr[p + 1], clamped as
 *   cbgx_group_diversity clamps them; there is no limit on the size of a group.  All four pocket ranges are clamped to their arrays.
 *   sample_out [B, CBGX_NATIVE_SAMPLE_COLS] int64, for sample g of pocket p:
 *     sim_micro       (common 1000000 + union / 2) / union in integer division with common = popcount(fp_g & fp_nat_p), union =
 *                     popcount(fp_g | fp_nat_p); 0 when union is 0: the Tanimoto similarity in millionths, rounded half up
 *     same_hash       1 iff mol_hash[g] == mol_hash_nat[p], else 0
 *     contact_common  pocket atoms k with rec_contact[r0 + k] != 0 and rec_contact_nat[q0 + k] != 0 (r0, q0 the starts of the two ranges)
 *     contact_union   ... with either != 0
 *     contact_micro   the same rounding formula on those two, 0 when contact_union is 0
 *     status          bits, side by side: CBGX_NATIVE_SAMPLE_NOT_EVALUATED (fp_status[g] != 0) and CBGX_NATIVE_NATIVE_NOT_EVALUATED
 *                     (fp_status_nat[p] != 0): sim_micro and same_hash are -1 with either; CBGX_NATIVE_POCKET_MISMATCH (the two
 *                     clamped pocket ranges differ in length): the three contact columns are -1
 *   centroid_d2 [B] float64: the squared distance of the two centroids by the formula above on float64 components; NaN where either
 *   contacts status is not 0 or either centroid has a NaN.
 *   group_out [P, CBGX_NATIVE_GROUP_COLS] int64: n_graphs, n_fp_compared (samples with sim_micro >= 0), n_same_hash, sim_micro_sum,
 *   sim_micro_max (-1 without one), n_contact_compared (samples without CBGX_NATIVE_POCKET_MISMATCH), contact_micro_sum,
 *   contact_micro_max (-1 without one), status: CBGX_NATIVE_NATIVE_NOT_EVALUATED, and CBGX_NATIVE_BAD_GROUPS where the range of
 *   group_ptr is decreasing or outside [0, B] (the clamped range is evaluated).
 *   A graph in no group is not written.  Sums, maxima and counts of integers: nothing depends on scheduling.  No atomics on memory.
 *   Overlapping groups have two workgroups write the same rows, in no order: those rows are undefined.
 *   Returns 0, and 0 without a launch when P == 0.  CBGX_E_INVALID before any dereference or launch: negative counts, a NULL pointer with
 *   a non-zero count (the per-sample arrays with B, rec_contact with n_rec, the per-native arrays, rec_ptr_nat, group_ptr and group_out
 *   with P, rec_contact_nat with n_rec_nat; rec_ptr whenever P > 0), an fp or fp_nat that is not 16-byte aligned, and any array with a
 *   non-zero count whose pointer is not memory the device can read, named as above. */
#define CBGX_CONTACTS_CUTOFF2 16.0
#define CBGX_CONTACTS_GRAPH_COLS 6   /* n_atoms, n_heavy, n_rec, n_rec_contact, n_lig_contact, status */
#define CBGX_CONTACTS_EMPTY 16
#define CBGX_NATIVE_SAMPLE_COLS 6    /* sim_micro, same_hash, contact_common, contact_union, contact_micro, status */
#define CBGX_NATIVE_GROUP_COLS 9     /* n_graphs, n_fp_compared, n_same_hash, sim_micro_sum, sim_micro_max, n_contact_compared,
                                        contact_micro_sum, contact_micro_max, status */
#define CBGX_NATIVE_SAMPLE_NOT_EVALUATED 1
#define CBGX_NATIVE_NATIVE_NOT_EVALUATED 2
#define CBGX_NATIVE_POCKET_MISMATCH 4
#define CBGX_NATIVE_BAD_GROUPS 8
int cbgx_pocket_contacts(const float *x_lig, const uint8_t *z_lig, const int32_t *lig_ptr, int n_lig, const float *x_rec,
                         const uint8_t *z_rec, const int32_t *rec_ptr, int n_rec, int n_graphs, double cutoff2, uint8_t *rec_contact,
                         uint8_t *lig_contact, double *centroid, int32_t *graph_out, void *stream);
int cbgx_native_compare(const uint32_t *fp, const uint64_t *mol_hash, const int32_t *fp_status, const uint8_t *rec_contact,
                        const int32_t *rec_ptr, const double *centroid, const int32_t *contacts_status, int n_graphs, int n_rec,
                        const uint32_t *fp_nat, const uint64_t *mol_hash_nat, const int32_t *fp_status_nat, const uint8_t *rec_contact_nat,
                        const int32_t *rec_ptr_nat, const double *centroid_nat, const int32_t *contacts_status_nat, int n_groups,
                        int n_rec_nat, const int32_t *group_ptr, int64_t *sample_out, double *centroid_d2, int64_t *group_out,
                        void *stream);

/* ---- distributions of sampled ligands: pair distances, bond lengths, bond angles (distributions.hip) -----------------------------------
 * The rest of the reference's geometry report (evaluate_scripts/evaluate_geom_single.py; repo/tools/geometry/eval_bond_length.py,
 *   eval_bond_angle.py): histograms that are compared with a dataset's by Jensen-Shannon distance.  Distances and element codes are those
 *   of cbgx_ligand_geometry: fp32 coordinates widened to fp64, s = (dx dx + dy dy) + dz dz with every operation rounded on its own,
 *   d = sqrt(s) correctly rounded, contraction off in the translation unit; codes 0 ... 7 = H C N O F P S Cl.  Same arrays, same limit
 *   CBGX_GEOMETRY_MAX_LIGAND, same lig_ptr read-back and size check.  No atomics on memory; a graph's rows are a function of its own atoms.
 * Pair-distance histograms (cbgx_ligand_pair_hist; pair_distance_from_pos_v + get_pair_length_profile, eval_bond_length.py:77-84,
 *   119-129): per graph two families over the pairs i < j of its ligand atoms -- family 0 (`All`): every pair, atoms of unknown element
 *   included; family 1 (`CC`): pairs with both atomic numbers 6.  Family f has its own strictly increasing fp64 edge array of
 *   E_f <= CBGX_PAIR_HIST_MAX_EDGES edges (device memory; that they increase is the caller's contract -- any content gives bins inside
 *   the row).  A pair takes part iff d < edges[E_f - 1], strictly (so never with E_f == 0, nor with a d that is not a number); its bin is
 *   the number of edges strictly less than d (np.searchsorted(edges, d), side left).  pair_hist [B, 2, E_max + 1] int32, E_max =
 *   max(E_0, E_1): every element of every graph is written (bins a family does not have are 0).  The edges are inputs so that the kernel
 *   never re-derives numpy's linspace arithmetic; the reference's are np.linspace(0, 12, 100) (All_12A) and np.linspace(0, 2, 100) (CC_2A).
 * Bond angles (cbgx_ligand_angles; bond_angle_from_mol, eval_bond_angle.py:69-96, on the TABLE-bond graph of cbgx_ligand_bonds_fill):
 *   an angle is an unordered pair {a, b}, a < b, of bonded partners of a centre atom c; the list is in lexicographic (c, a, b) order of
 *   global ligand rows.  The graph comes as a symmetric adjacency of the bond list: adj_ptr [n_lig + 1] int32, adj_nbr [n_adj] int32
 *   (n_adj = 2 n_bonds; global rows, ascending per centre), adj_order [n_adj] uint8 (1 ... 3); and angle_ptr [n_lig + 1] int32 = the
 *   exclusive prefix sum of C(deg, 2) per centre, n_angles = angle_ptr[n_lig].
 *   With u = x_a - x_c, v = x_b - x_c in fp64: dot = (ux vx + uy vy) + uz vz, su = (ux ux + uy uy) + uz uz, sv likewise,
 *   cos = dot / sqrt(su sv), every operation rounded on its own, then clamped to [-1, 1].  NO inverse trigonometric function runs on the
 *   device: angle_bin = the number of entries of the strictly decreasing fp64 table cos_edges [E_a], E_a <= CBGX_ANGLES_MAX_EDGES, that
 *   are strictly greater than cos -- what searchsorted(edges_deg, theta) gives wherever theta is not within rounding of an edge.  A
 *   degenerate angle (su sv == 0: a partner coincident with the centre, which IS bonded by the table; or a cos that is not a number, from
 *   coordinates that are not finite) has angle_cos = NaN and angle_bin = CBGX_ANGLE_BIN_DEGENERATE and belongs to no histogram.
 *   angle_type int16 = the canonical code of (code_a, order_ac, code_c, order_bc, code_b): of the two orientations the one whose
 *   (code, order) end pair is lexicographically smaller comes first, packed as (((code_1 3 + (o_1 - 1)) 8 + code_c) 3 + (o_2 - 1)) 8 +
 *   code_2, in [0, CBGX_ANGLE_TYPES).  The reference appends every angle under both orientations; for a NORMALISED profile that is the
 *   same distribution as counting each angle once under its canonical type, which is what is done here.
 *   Outputs: angle_index [3, n_angles] int32 (rows a, c, b: global ligand rows), angle_cos [n_angles] fp64, angle_bin [n_angles] uint8,
 *   angle_type [n_angles] int16; written without atomics, in that one order.
 *   Limit: a graph whose number of angles, the sum of C(deg_c, 2) over its centres, exceeds CBGX_ANGLES_MAX_PER_GRAPH (a collapsed
 *   sample; a sane 128-atom molecule has under 400) is never an error: the caller gives it no slots (its entries of the prefix sum are 0
 *   wide) and reports it (CBGX_DISTRIBUTIONS_TOO_MANY_ANGLES in the Python side's status column); the kernel writes nothing for such a
 *   graph whatever angle_ptr says.
 *   Clamping, as cbgx_ligand_bonds_fill clamps bond_ptr: a centre's adjacency range is clamped to [0, n_adj] and its slots to
 *   [0, n_angles], both made non-decreasing; the centre writes its first min(slots, C(deg, 2)) angles; an angle with a partner row
 *   outside the graph's atom range, or an atom without an element code, is skipped.  A wrong angle_ptr or adjacency loses angles (or,
 *   where slot ranges overlap, overwrites them) and never reaches outside a buffer.
 * Bond-length bins are elementwise on the bond list (bond_bin = the number of edges strictly less than bond_length, bond_type =
 *   ((order - 1) 8 + code_lo) 8 + code_hi with code_lo <= code_hi) and are made by the caller; they have no entry here.
 * Both return 0, and 0 without a launch when B == 0 (cbgx_ligand_angles also when n_angles == 0).  CBGX_E_INVALID before any dereference
 *   or launch: negative counts, a NULL pointer with a non-zero count, more edges than the limit, a ligand above
 *   CBGX_GEOMETRY_MAX_LIGAND atoms, lig_ptr the device cannot read. */
#define CBGX_PAIR_HIST_MAX_EDGES 255
#define CBGX_ANGLES_MAX_EDGES 254
#define CBGX_ANGLES_MAX_PER_GRAPH 16384
#define CBGX_ANGLE_BIN_DEGENERATE 255
#define CBGX_ANGLE_TYPES 4608
#define CBGX_DISTRIBUTIONS_TOO_MANY_ANGLES 1
int cbgx_ligand_pair_hist(const float *x_lig, const uint8_t *z_lig, const int32_t *lig_ptr, int n_lig, int n_graphs,
                          const double *edges_all, int n_edges_all, const double *edges_cc, int n_edges_cc, int32_t *pair_hist,
                          void *stream);
int cbgx_ligand_angles(const float *x_lig, const uint8_t *z_lig, const int32_t *lig_ptr, int n_lig, int n_graphs, const int32_t *adj_ptr,
                       const int32_t *adj_nbr, const uint8_t *adj_order, int n_adj, const int32_t *angle_ptr, int n_angles,
                       const double *cos_edges, int n_cos_edges, int32_t *angle_index, double *angle_cos, uint8_t *angle_bin,
                       int16_t *angle_type, void *stream);

/* ---- measurement hook (bench.py) ----------------------------------------------------------------
 * Between cbgx_profile_begin() and cbgx_profile_end() every kernel launch is bracketed by HIP events on
 * its own stream.  cbgx_profile_end() synchronises them and returns, per kernel class, the summed
 * device time in ms and the launch count.  Classes: 0 knn, 1 gate, 2 node GEMM, 3 node query fold,
 * 4 x2h edge kernel over all nodes, 5 h2x edge kernel (node list), 6 x2h edge kernel over a node list (pruned last
 * layers), 7 x2h edge backward over all nodes, 8 h2x edge backward, 9 training GEMMs, 10 x2h edge backward over a node list
 * 11 the ordered gather of the x2h backward's edge-row mode (CBGX_PROFILE_CLASSES = 12).  Not thread-safe with concurrent launches
 * from other threads; process-wide. */
#define CBGX_PROFILE_CLASSES 12
int cbgx_profile_begin(int max_launches);
int cbgx_profile_end(double *ms_by_class, int *launches_by_class, int num_classes);

#ifdef __cplusplus
}
#endif
#endif /* CBGX_H */

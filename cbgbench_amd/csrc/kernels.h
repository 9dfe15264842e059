// internal launcher declarations (host side)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cbgx {

// Auxiliary stream of a caller stream (api.hip: one per (host thread, caller stream), created on first use, reused for the life of
// the thread): the forward's two-stream schedule forks / joins it with `fork` / `join`; the training backward runs the weight-gradient
// part of a block on it and records `done[set]` when the block's buffer set is free again (api_train.hip).  NULL when unavailable.
struct AuxStream {
    hipStream_t owner = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr, done[2] = {nullptr, nullptr};
};
AuxStream* aux_for(hipStream_t caller);

// ---- what the launchers below take instead of loose pointers ----
// a node list built on the device: row ids (any order) and the address of their number
struct NodeList {
    int* rows;
    int* count;
};
// the read-only view of one that a launcher takes; {nullptr, nullptr} (the default): every row
struct RowList {
    const int* rows = nullptr;
    const int* count = nullptr;
    RowList() = default;
    RowList(const int* r, const int* c) : rows(r), count(c) {}
    RowList(NodeList l) : rows(l.rows), count(l.count) {}
};
// of one attention block's node stage: projection, query, folded query
struct NodeBufs { float *P, *q, *Qt; };
// the graph an attention block runs on, built once per call (`gen` may be NULL where no block of the call moves coordinates)
struct Graph {
    const int32_t *nbr, *deg;
    const float* e_w;
    const uint8_t *lig, *gen;
    int n_nodes;
};

// ---- optional per-kernel timing (cbgx_profile_begin / cbgx_profile_end) ----
enum KernelClass { K_KNN = 0, K_GATE, K_NODE_GEMM, K_NODE_QUERY, K_EDGE_X2H, K_EDGE_H2X, K_EDGE_X2H_LISTED, K_EDGE_X2H_BWD, K_EDGE_H2X_BWD,
                   K_TRAIN_GEMM, K_EDGE_X2H_BWD_LISTED, K_EDGE_ROWS_REDUCE, K_NUM_CLASSES };
void profile_mark_begin(int cls, hipStream_t s);
void profile_mark_end(hipStream_t s);
bool profile_is_on();

hipError_t launch_knn(const float* x, const int32_t* graph_ptr, int n_graphs, int n_nodes, int32_t* nbr,
                      int32_t* deg, hipStream_t s);
hipError_t launch_gate(const float* packed, const float* x, const int32_t* nbr, const int32_t* deg, int n_nodes,
                       float* e_w, hipStream_t s);
hipError_t launch_node_gemm(const float* A, int lda, const float* Wt, const float* bias, float* C, int ldc, int M,
                            int nout, int act, hipStream_t s, RowList rows = {});
// node projection + query fold + fused edge kernel of one attention block on the destination rows `dst`, whose sources are in `src`.
// x2h: out = h_out[N,128]; h2x: out = x_out[N,3], dx_out optional.
// h2x_lig (h2x on a work list of ligand atoms, h2x_lig_selected): no fold in the node stage, edge_h2x_lig_kernel folds in registers
hipError_t launch_attention(bool x2h, const float* att, const Graph& g, const float* x, const float* h, const NodeBufs& b, float* out,
                            float* dx_out, RowList dst, RowList src, hipStream_t s, bool h2x_lig = false);
// which generation of kernels the stage dispatchers (dispatch.hip) use: always the MFMA one in libcbgx.so; the test-only
// library libcbgx_xcheck.so (-DCBGX_XCHECK) can switch to the first-generation VALU kernels at run time
#ifdef CBGX_XCHECK
extern int g_edge_impl;
hipError_t launch_knn_v1(const float* x, const int32_t* graph_ptr, int n_graphs, int n_nodes, int32_t* nbr, int32_t* deg,
                         hipStream_t s);
hipError_t launch_gate_v1(const float* packed, const float* x, const int32_t* nbr, const int32_t* deg, int n_nodes,
                          float* e_w, hipStream_t s);
hipError_t launch_node_gemm_v1(const float* A, int lda, const float* Wt, const float* bias, float* C, int ldc, int M, int nout, int act,
                               hipStream_t s, RowList rows);
hipError_t launch_node_query_v1(const float* att, const float* P, float* Qt, int n_nodes, hipStream_t s);
hipError_t launch_attention_v1(bool x2h, const float* att, const Graph& g, const float* x, const float* h, const NodeBufs& b,
                               float* out, float* dx_out, hipStream_t s);
#else
constexpr int g_edge_impl = 0;
#endif
// ---- weight packing, batched over attention blocks (the weights are re-packed every training step: 18 blocks x 12 small kernels
// were 216 launches and 1.5 ms per step; one launch per kernel for all blocks is ~20) ----------------------------------------------
constexpr int PACK_BLOCKS_MAX = 20;
struct PackBlocks {                       // per attention block: the reference tensors the pack kernels read and the block's ATT region
    const float* wk0[PACK_BLOCKS_MAX];    // k first Linear [128][340], its bias
    const float* bk0[PACK_BLOCKS_MAX];
    const float* wv0[PACK_BLOCKS_MAX];
    const float* bv0[PACK_BLOCKS_MAX];
    const float* wq0[PACK_BLOCKS_MAX];    // q first Linear [128][128], its bias
    const float* bq0[PACK_BLOCKS_MAX];
    const float* wq1[PACK_BLOCKS_MAX];    // q second Linear [128][128]
    const float* wk1[PACK_BLOCKS_MAX];    // k second Linear [128][128]
    const float* wv1[PACK_BLOCKS_MAX];    // v second Linear ([128][128] x2h, [16][128] h2x)
    float* att[PACK_BLOCKS_MAX];
    // the five 128-column groups of the assembled node projection (PDk | PDv | PSk | PSv | q hidden): base pointer of each group's
    // source matrix -- the CENTRED first Linears inside `att` for the first four, wq0 for the fifth.  A table indexed by the group,
    // not an if-chain over pointers: hipcc 7.2 selected the wrong base for the fifth group in the wave-per-column scale kernel.
    const float* nsrc[PACK_BLOCKS_MAX][5];
    unsigned char x2h[PACK_BLOCKS_MAX];
    int n;
};
// stage 1: centred first Linears of k and v (A_WAKC / A_BAKC / A_WAVC / A_BAVC) of every block
hipError_t launch_pack_stage1(const PackBlocks& pb, hipStream_t s);
// stage 2 (after stage 1 on the same stream): column scales, split-f16 node tables, Wbk fragments, bn2, rbf scales, rbf fragment
// tables (k, v, and the edge-major v table of x2h blocks), dWt, the swizzled Wbv image of x2h blocks
hipError_t launch_pack_stage2(const PackBlocks& pb, hipStream_t s);
// second-generation graph kernels (graph_mfma.hip)
hipError_t launch_pack_gate_img(const float* w1, const float* b1, const float* g, const float* be, const float* w2,
                                float* img, hipStream_t s);
hipError_t launch_knn_reg(const float* x, const int32_t* graph_ptr, int n_graphs, int n_nodes, int32_t* nbr,
                          int32_t* deg, hipStream_t s, RowList rows = {});
// graph-cached calls: the listed centres' lists from (pocket list U the graph's ligand atoms) by rank counting (graph_mfma.hip)
// `s_ew` / `e_w` / `newmask` (optional): kept pocket entries carry their cached gate value to their new rank, newmask[i] = the ranks
// that hold new entries -- what launch_gate_mfma(..., newmask) then evaluates instead of all 32 slots
hipError_t launch_knn_merge(const float* x, const int32_t* graph_ptr, int n_graphs, int n_nodes, const uint8_t* lig,
                            const int32_t* s_nbr, const int32_t* s_deg, int32_t* nbr, int32_t* deg, hipStream_t s, RowList rows,
                            const float* s_ew = nullptr, float* e_w = nullptr, unsigned* newmask = nullptr);
// graph-cached calls: the listed centres' merged neighbour lists and their gate values in one launch -- kept pocket entries carry
// their cached gate value to their new rank, the gate MLP runs on the entries that are new (graph_mfma.hip, knn_merge_gate_kernel)
hipError_t launch_knn_merge_gate(const float* packed, const float* x, const int32_t* graph_ptr, int n_graphs, int n_nodes,
                                 const uint8_t* lig, const int32_t* s_nbr, const int32_t* s_deg, const float* s_ew, int32_t* nbr,
                                 int32_t* deg, float* e_w, hipStream_t s, RowList rows);
hipError_t launch_gate_mfma(const float* packed, const float* x, const int32_t* nbr, const int32_t* deg, int n_nodes,
                            float* e_w, hipStream_t s, RowList rows = {}, const unsigned* newmask = nullptr);
// head of a graph-cached forward call in one launch: proximity flags -> `dirty`, their compaction -> `list` / `count` (zero on
// entry), the pocket's graph -> nbr / deg / ew, the cached features of layers 0 / 1 -> out1 / out2 (graph_mfma.hip); with `keep1` /
// `keep2` (per-node flags) only into the flagged rows: the other rows of out1 / out2 already hold them (step cache, api.hip)
hipError_t launch_graph_cache_begin(const float* x, const int32_t* graph_ptr, int n_graphs, const uint8_t* lig, const float* r32sq,
                                    int n, uint8_t* dirty, int* list, int* count, const int32_t* s_nbr, const int32_t* s_deg,
                                    const float* s_ew, int32_t* nbr, int32_t* deg, float* ew, const float* h1, const float* h2,
                                    float* out1, float* out2, hipStream_t s, const uint8_t* keep1 = nullptr,
                                    const uint8_t* keep2 = nullptr);
// MFMA node kernels (node_mfma.hip): P = h Wn + bn, q = MLP tail, Qt = folded query
hipError_t launch_pack_node_tables(const PackBlocks& pb, hipStream_t s);     // node_mfma.hip part of stage 2
// counter_zeroed: the caller has already set *count to zero on this stream (cbgx_unitransformer_forward zeroes all its list counters
// with ONE memset instead of one per list: ~15 fills of 4.6 us per denoising step)
hipError_t launch_build_active(const uint8_t* flag, int n, NodeList out, hipStream_t s, bool counter_zeroed = false);
hipError_t launch_mark_seed(const uint8_t* a, const uint8_t* b, int n, uint8_t* m, hipStream_t s);
hipError_t launch_mark_from_nbr(const uint8_t* flag, const int32_t* nbr, const int32_t* deg, int n, uint8_t* out,
                                hipStream_t s);
hipError_t launch_mark_nbr(RowList rows, int n_upper, const int32_t* nbr, const int32_t* deg, uint8_t* m, hipStream_t s);
// the node stage of one attention block: own columns, q and Qt on `dst`, PS columns on `src`.  Its options, all off by default:
// large_lists: the destination list (when given) is expected to hold a sizeable part of the nodes (x2h blocks of the cached / pruned
// layers) rather than the few movable atoms of an h2x block: throughput launches instead of one workgroup per column chunk
// q_direct (inputs above NODE_STAGE_MAX_ROWS only): q comes straight from h (node_query_kernel) and the q-hidden columns of P are
// NOT produced -- for callers whose edge stage is all that reads P (the inference forward; the training tape keeps them)
// fold (a list): Qt is produced for these rows instead of for all of `dst`;  no_fold: the stage ends with the query MLP (h2x_lig)
// dst_all_columns (inputs above NODE_STAGE_MAX_ROWS only): ONE projection launch writes the own AND the PS columns of `dst`, nothing is
// projected on `src` -- for P arrays that outlive the call and hold every other row already (step cache, api.hip)
struct NodeStageOpts {
    bool large_lists = false;
    RowList fold;
    bool q_direct = false;
    bool no_fold = false;
    bool dst_all_columns = false;
};
hipError_t launch_node_mfma(const float* att, const float* h, const uint8_t* lig, int n_nodes, const NodeBufs& b, RowList dst,
                            RowList src, hipStream_t s, const NodeStageOpts& o = {});
// CBGX_NODE_QDIRECT=0 in the environment: the inference forward keeps the projection -> query MLP chain (A/B runs, bit-identity tests)
bool node_qdirect_enabled();
// the fused node stage (node_stage_kernel, inputs of <= NODE_STAGE_MAX_ROWS rows) as a list of jobs on the same input features:
// blockIdx.y = job.  `rows` NULL: all n_nodes rows.  `chunk_mask`: 64-column chunks of the projection to produce (CHUNKS_*);
// `proj_only`: phase 1 only (the PS columns of a block's source rows).
struct NodeStageJob {
    const float* att;
    float *P, *q, *Qt;
    const int *rows, *n_rows;
    unsigned chunk_mask;
    int proj_only;
    // optional: the folded query Qt is produced only for rows with fold_flag[row] != 0 -- the x2h edge stage reads it for
    // general-role destinations only (the node or a neighbour is a ligand atom: ~28 % of a pocket), protein-only ones fold in
    // registers (edge_mfma.hip) -- 8 KB of stores per row saved for the others
    const uint8_t* fold_flag;
    int no_fold;        // the stage ends with the query MLP: the edge kernel folds q itself (edge_h2x_lig.hip), Qt is not written
};
constexpr int NS_JOBS_MAX = 4;
struct NodeStageJobs { NodeStageJob j[NS_JOBS_MAX]; int n; };
constexpr int NODE_STAGE_MAX_ROWS = 8192;   // up to here the latency-built fused kernel replaces the three-kernel chain
// the jobs of one attention block's node stage appended to `jobs` (same selection as launch_node_mfma's fused path): with a
// destination list two jobs (own columns on `dst`, PS columns on `src` -- all rows when src is NULL), without one job on all rows
bool add_node_stage_jobs(NodeStageJobs& jobs, const float* att, const NodeBufs& b, RowList dst, RowList src,
                         const uint8_t* fold_flag = nullptr, bool no_fold = false);
hipError_t launch_node_stage_jobs(const NodeStageJobs& jobs, const float* h, const uint8_t* lig, int n_nodes, hipStream_t s);
// all node lists of a forward call in four launches (node_mfma.hip): three level kernels over flags + one multi-job compaction
struct GraphFlags {
    const uint8_t *gen, *lig;
    const uint8_t* D1;            // input of the cached levels (may alias d1)
    uint8_t *d1, *a1, *a2, *a3, *D2, *S1, *S2;
};
constexpr int LIST_JOBS_MAX = 20;      // (a cached + pruned + dual call uses 16)
struct ListJobs {
    const uint8_t* flag[LIST_JOBS_MAX];      // member if flag != 0 (NULL: every node) ...
    const uint8_t* flag2[LIST_JOBS_MAX];     // ... and (flag2 != 0) == want2 when flag2 is given
    int want2[LIST_JOBS_MAX];
    int* list[LIST_JOBS_MAX];
    int* count[LIST_JOBS_MAX];
    int n_jobs;
};
hipError_t launch_list_level(const GraphFlags& f, const int32_t* nbr, const int32_t* deg, int n, int level, bool cached, bool prune,
                             hipStream_t s);
// Small inputs (n <= GRAPH_LISTS_MAX_NODES): the three level kernels and the compaction above as ONE launch, one workgroup per graph
// with the graph's flags in LDS (flags only ever propagate along edges, and edges stay inside a graph).  The jobs name their flags by
// id instead of by pointer; of the flag arrays in global memory only the three inputs are read and only d1 is written.
enum GraphFlagId { GF_GEN = 0, GF_LIG, GF_D1IN, GF_d1, GF_a1, GF_a2, GF_a3, GF_D2, GF_S1, GF_S2, GF_COUNT, GF_ALL = -1 };
constexpr int GRAPH_LISTS_MAX_NODES = 8192;
struct GraphListJobs {
    signed char flag[LIST_JOBS_MAX];         // GraphFlagId (GF_ALL: every node) ...
    signed char flag2[LIST_JOBS_MAX];        // ... and (flag2 != 0) == want2 unless GF_ALL
    signed char want2[LIST_JOBS_MAX];
    int* list[LIST_JOBS_MAX];
    int* count[LIST_JOBS_MAX];
    int n_jobs;
};
// `d1_out` [n]: the d1 flags (the node or one of its neighbours is a ligand atom) are also written to global memory
hipError_t launch_graph_lists(const uint8_t* gen, const uint8_t* lig, const uint8_t* d1_in, const int32_t* nbr, const int32_t* deg,
                              const int32_t* graph_ptr, int n_graphs, const GraphListJobs& jobs, bool cached, bool prune,
                              uint8_t* d1_out, hipStream_t s);
hipError_t launch_build_lists(const ListJobs& jobs, int n, hipStream_t s);
hipError_t launch_split_list(RowList in, int n, const uint8_t* flag, NodeList out1, NodeList out0, hipStream_t s,
                             bool counters_zeroed = false);
// MFMA edge kernel (edge_mfma.hip)
int set_edge_workgroup_limit(int n);
hipError_t launch_edge_mfma(bool x2h, const float* att, const Graph& g, const float* x, const float* h, const NodeBufs& b, float* out,
                            float* dx_out, RowList dst, hipStream_t s);
hipError_t launch_edge_x2h_dual(const float* att, const Graph& g, const float* x, const float* h, const NodeBufs& b, float* out,
                                RowList pp, RowList gen, bool full_layer, hipStream_t s);
// edge_h2x_lig.hip: the h2x edge kernel for work lists of ligand atoms (query folded in registers from b.q = q[N,128]), the pack
// kernel of its LDS image (part of stage 2), and CBGX_H2X_FOLD (default on)
hipError_t launch_edge_h2x_lig(const float* att, const Graph& g, const float* x, const float* h, const NodeBufs& b, float* out,
                               float* dx_out, RowList dst, hipStream_t s);
hipError_t launch_pack_h2l_image(const PackBlocks& pb, hipStream_t s);
bool h2x_fold_enabled();
// edge_x2h_f16.hip: the same launch with scores and aggregation in split-f16 (called by launch_edge_x2h_dual, which owns the grid)
void launch_edge_x2h_f16_grid(int grid, const float* att, const Graph& g, const float* x, const float* h, const NodeBufs& b,
                              float* out, RowList pp, RowList gen, bool full_layer, hipStream_t s);
// TargetDiff step prologue / epilogue (step.hip)
hipError_t launch_step_prologue(const float* x_lig, const float* c_lig, const int32_t* lig_rows, int n_lig, int C,
                                const float* emb_w, const float* emb_b, const float* ind_w, const float* ind_b, float* x,
                                float* h, hipStream_t s, const int32_t* t_ptr = nullptr);
// where the eps / u of a TargetDiff step come from: the tape pair, or (keys != NULL) the counter-based generator of rng.h, evaluated by the
// kernel at (keys[lig_graph[a]], a - lig_ptr[lig_graph[a]], step, purpose_base + purpose) -- the numbers launch_noise_fill writes out
struct StepNoise {
    const float *eps = nullptr, *u = nullptr;
    const uint64_t* keys = nullptr;
    const int32_t *lig_graph = nullptr, *lig_ptr = nullptr;
    int n_graphs = 0, purpose_base = 0;
};
hipError_t launch_step_epilogue(const float* x_den, const float* logits, const int32_t* lig_rows, const float* x_lig,
                                const float* c_lig, const uint8_t* gen_lig, int n_lig, int C, int t,
                                const float* const* tabs, float log_c, const StepNoise& noise, float* x_next, float* c_next,
                                int32_t* v_next, hipStream_t s, int32_t* t_ptr = nullptr);
// epilogue of step t + prologue of step t - 1 (the composed rows x[lig_rows], h[lig_rows] of the next denoiser call) in one launch
hipError_t launch_step_boundary(const float* x_den, const float* logits, const int32_t* lig_rows, const float* x_lig,
                                const float* c_lig, const uint8_t* gen_lig, int n_lig, int C, int t, const float* const* tabs,
                                float log_c, const StepNoise& noise, float* x_next, float* c_next, const float* emb_w,
                                const float* emb_b, const float* ind_w, const float* ind_b, float* x, float* h, hipStream_t s);
hipError_t launch_noise_fill(const uint64_t* keys, const int32_t* lig_ptr, int n_graphs, int n_lig, int cols, int uniform,
                             uint32_t purpose, int step, const int32_t* step_ptr, float* out, hipStream_t s);
hipError_t launch_diffbp_epilogue(const float* x_den, const float* x_com, const float* x_in, const float* logits,
                                  const int32_t* lig_rows, const int32_t* lig_ptr, const float* x_lig, const float* c_lig,
                                  const uint8_t* gen_lig, int n_graphs, int C, int t, int T, const float* acp_tab,
                                  const float* beta_tab, int absorbing, const float* eps, const float* u, float* x_next,
                                  float* c_next, hipStream_t s);
hipError_t launch_diffsbdd_step(const float* x_den, const float* logits, const int32_t* graph_ptr, const int32_t* lig_rows,
                                const int32_t* lig_ptr, const uint8_t* lig_flag, const float* x_lig, const float* c_lig,
                                int n_graphs, int C, float inv_alpha, float coef, float sigma, int do_x, int do_c,
                                const float* eps_x, const float* eps_c, const float* emb_w, const float* emb_b,
                                const float* ind_w, const float* ind_b, float* x_next, float* c_next, float* x, float* h,
                                float* shift_out, float* frame, hipStream_t s);
// geometry.hip: stability and steric-clash report of a batch of ligands, one workgroup per graph (ligands of at most
// CBGX_GEOMETRY_MAX_LIGAND atoms: the caller checks), and the host copies of its constant tables
hipError_t launch_ligand_geometry(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, const float* x_rec,
                                  const uint8_t* z_rec, const int32_t* rec_ptr, int n_rec, int n_graphs, int32_t* nr_bonds,
                                  uint8_t* flags, int32_t* graph_out, hipStream_t s);
void ligand_geometry_tables(int32_t* bond_pm, int32_t* margins, int32_t* allowed, uint8_t* elements, uint8_t* vdw_z, double* vdw_r,
                            double* tolerance);
// geometry.hip: the table-bond graph of the same ligands in two launches -- partners j > i per atom, component labels and per-graph counts;
// then, given the exclusive prefix sum of the partner counts, the bond list in (i, j) order
hipError_t launch_ligand_bonds_count(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs,
                                     int32_t* deg_up, int32_t* fragment, int32_t* graph_out, hipStream_t s);
hipError_t launch_ligand_bonds_fill(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs,
                                    const int32_t* bond_ptr, int n_bonds, int32_t* bond_index, uint8_t* bond_order, double* bond_length,
                                    hipStream_t s);
// rings.hip: ring sizes (lengths of a minimum cycle basis) and the shortest ring through every atom, from that bond list; one wave per graph
hipError_t launch_ligand_rings(const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* bond_ptr, const int32_t* bond_index,
                               int n_bonds, uint8_t* atom_ring_min, int32_t* graph_out, hipStream_t s);
// aromatic.hip: the closure of the model's aromatic flags over the chordless 5- and 6-cycles of that bond list, aromatic atoms and bonds;
// one wave per graph
hipError_t launch_ligand_aromatic(const uint8_t* z_lig, const uint8_t* flag_lig, const uint8_t* atom_ring_min, const int32_t* lig_ptr,
                                  int n_lig, int n_graphs, const int32_t* bond_ptr, const int32_t* bond_index, int n_bonds,
                                  uint8_t* atom_out, uint8_t* bond_aromatic, int32_t* graph_out, hipStream_t s);
// valence.hip: Kekule orders of the aromatic systems of that bond list (a bounded search, one system per lane), implicit hydrogens and
// valence flags; one wave per graph
hipError_t launch_ligand_valence(const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* bond_ptr,
                                 const int32_t* bond_index, const uint8_t* bond_order, const uint8_t* bond_aromatic, int n_bonds,
                                 int max_steps, uint8_t* implicit_h, uint8_t* atom_flags, uint8_t* bond_kekule, int32_t* graph_out,
                                 hipStream_t s);
// interactions.hip: donor / acceptor / hydrophobic types of the pocket atoms from the residue table (a carbon's table bonds to N, O, S
// included), then ligand types, rotatable bonds and the five Vina-form pair terms against the typed pocket; one workgroup per graph each
hipError_t launch_pocket_types(const float* x_rec, const uint8_t* z_rec, const int32_t* rec_ptr, int n_rec, int n_graphs,
                               const uint8_t* rec_aa, const uint8_t* rec_backbone, uint8_t* rec_type, hipStream_t s);
hipError_t launch_ligand_interactions(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, const float* x_rec,
                                      const uint8_t* rec_type, const int32_t* rec_ptr, int n_rec, int n_graphs, const int32_t* bond_ptr,
                                      const int32_t* bond_index, const uint8_t* bond_kekule, const uint8_t* bond_aromatic, int n_bonds,
                                      const uint8_t* implicit_h, const uint8_t* atom_flags, const int32_t* valence_status,
                                      double* atom_terms, uint8_t* lig_type, uint8_t* bond_rotatable, double* graph_terms,
                                      int32_t* graph_out, hipStream_t s);
// groups.hip: functional groups of that bond list -- members by marking rules, groups as components under the group bonds, every group
// held against the 25 template graphs of geo_tables.h by an exact isomorphism test (one group per lane); one wave per graph
hipError_t launch_ligand_groups(const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* bond_ptr,
                                const int32_t* bond_index, const uint8_t* bond_order, const uint8_t* bond_aromatic, int n_bonds,
                                int32_t* atom_group, uint8_t* atom_class, int32_t* graph_out, hipStream_t s);
void ligand_groups_templates(uint8_t* n_atoms, uint8_t* n_bonds, uint8_t* labels, uint8_t* bonds);
// diversity.hip: a 1024-bit fingerprint and a 64-bit hash of every graph of that bond list by colour refinement over its typed bonds (one
// wave per graph), and, one workgroup per group of consecutive graphs, the Tanimoto similarity of every pair, each graph's nearest
// neighbour and the first graph of equal hash
hipError_t launch_ligand_fingerprints(const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs, const int32_t* bond_ptr,
                                      const int32_t* bond_index, const uint8_t* bond_type, const uint8_t* atom_ring_min, int n_bonds,
                                      uint32_t* fp, uint64_t* mol_hash, int32_t* graph_out, hipStream_t s);
hipError_t launch_group_diversity(const uint32_t* fp, const uint64_t* mol_hash, const int32_t* status, const int32_t* group_ptr,
                                  const int64_t* pair_ptr, int n_graphs, int n_groups, long long n_pairs, int32_t* pair_sim,
                                  int32_t* first_same, int32_t* nearest, int32_t* nearest_micro, int64_t* group_out, hipStream_t s);
// native.hip: the heavy pocket atoms within a cutoff of a ligand's heavy atoms, the ligand's side of the same, and the centroid of its heavy
// atoms (one workgroup per graph); and, one workgroup per pocket, every sample against the pocket's native ligand: fingerprint
// similarity, equal hash, the overlap of the two contact sets, the squared distance of the two centroids
hipError_t launch_pocket_contacts(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, const float* x_rec,
                                  const uint8_t* z_rec, const int32_t* rec_ptr, int n_rec, int n_graphs, double cutoff2,
                                  uint8_t* rec_contact, uint8_t* lig_contact, double* centroid, int32_t* graph_out, hipStream_t s);
hipError_t launch_native_compare(const uint32_t* fp, const uint64_t* mol_hash, const int32_t* fp_status, const uint8_t* rec_contact,
                                 const int32_t* rec_ptr, const double* centroid, const int32_t* contacts_status, int n_graphs, int n_rec,
                                 const uint32_t* fp_nat, const uint64_t* mol_hash_nat, const int32_t* fp_status_nat,
                                 const uint8_t* rec_contact_nat, const int32_t* rec_ptr_nat, const double* centroid_nat,
                                 const int32_t* contacts_status_nat, int n_groups, int n_rec_nat, const int32_t* group_ptr,
                                 int64_t* sample_out, double* centroid_d2, int64_t* group_out, hipStream_t s);
// distributions.hip: pair-distance histograms of the same ligands (two families, LDS integer histograms), and the bond angles of the
// table-bond graph from its symmetric adjacency -- cosine, bin against a cosine table, canonical type; one workgroup per graph each
hipError_t launch_ligand_pair_hist(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs,
                                   const double* edges_all, int n_edges_all, const double* edges_cc, int n_edges_cc, int32_t* pair_hist,
                                   hipStream_t s);
hipError_t launch_ligand_angles(const float* x_lig, const uint8_t* z_lig, const int32_t* lig_ptr, int n_lig, int n_graphs,
                                const int32_t* adj_ptr, const int32_t* adj_nbr, const uint8_t* adj_order, int n_adj,
                                const int32_t* angle_ptr, int n_angles, const double* cos_edges, int n_cos_edges, int32_t* angle_index,
                                double* angle_cos, uint8_t* angle_bin, int16_t* angle_type, hipStream_t s);
constexpr int PACK_MAX = 64;
struct PackPiece {
    const float* src; float* dst; int src_ld, src_off, transpose, dst_ld, rows, cols;
};
struct PackBatch {
    PackPiece p[PACK_MAX]; int n;
};
hipError_t launch_pack_copy_multi(const PackBatch& b, hipStream_t s);
hipError_t launch_pack_copy(const float* src, int src_ld, int src_off, int transpose, float* dst, int dst_ld,
                            int rows, int cols, hipStream_t s);

}  // namespace cbgx

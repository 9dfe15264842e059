// libcbgx C ABI, training half (include/cbgx.h "training" section): taped forward, backward of single
// attention blocks (what the parity tests call) and of the whole denoiser.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "../../include/cbgx.h"
#ifdef CBGX_XCHECK
#include "../../include/cbgx_xcheck.h"
#endif
#include "kernels.h"
#include "layout.h"
#include "train.h"
#include "workspace.h"

using namespace cbgx;

namespace cbgx { int set_error(int code, const char* fmt, ...); }

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) return set_error(CBGX_E_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
#define RC_TRY(expr)         \
    do {                     \
        int _rc = (expr);    \
        if (_rc) return _rc; \
    } while (0)

// Neighbour-row gradients of the x2h edge backward: 0 = fp32 atomics on dP (default: the faster training step), 1 = edge rows + a gather
// in a fixed order (train_scatter.hip): the kernel is 10 % faster (750 vs 832 us per 16.5 k-node launch) and dL/dh becomes reproducible
// bit for bit, but the gather reads N x 32 KB (105 us, HBM-bound) and the step is 2 - 3 % slower (profiles/ab_train_r06[jkmn].log).
// Same mathematics, different summation order; chosen per call by the environment (CBGX_BX_EDGE_ROWS=1), this macro is the default.
#ifndef CBGX_BX_EDGE_ROWS
#define CBGX_BX_EDGE_ROWS 0
#endif
static inline bool edge_rows_mode() {
    const char* e = getenv("CBGX_BX_EDGE_ROWS");
    return e ? atoi(e) != 0 : CBGX_BX_EDGE_ROWS != 0;
}
// schedule-only knobs of the training path, read at every call (a getenv next to a 15 ms step) so that one process can compare them
// (tests/test_gpu_training.py, scripts/ab_train_base.sh)
static inline bool env_on(const char* name) { const char* e = getenv(name); return !e || atoi(e) != 0; }
constexpr int EDGE_GRID = 256;    // persistent workgroups of the edge backward (one per CU: ~97 KB LDS each)
#ifndef CBGX_NODE_GRID
#define CBGX_NODE_GRID 256        // A/B knob (scripts/build_variant.py)
#endif
constexpr int NODE_GRID = CBGX_NODE_GRID;    // persistent workgroups of the node-level reductions (one NS_SIZE slab each)
constexpr int FOLD = 8;           // slab reductions are two-level: n_slabs -> FOLD (slab_fold_kernel) -> 1 (reduce_store)
constexpr int GATE_GRID = 1024;  // gate weight-gradient kernel: 160-thread workgroups, four per CU keep every SIMD busy
constexpr int MAX_SPLITS = 128;   // node groups of the weight-gradient products (one [128 x 640] partial slab each)
constexpr int QLN_SLOTS = 64;     // query-LayerNorm affine gradient accumulators (atomics): one zeroed slot per attention block of a backward

// ---- tape: what the taped forward keeps for the backward ------------------------------------------------
struct Tape {
    int32_t* nbr;
    int32_t* deg;
    float* e_w;
    float* xs;   // [(L+1)][N][3]   xs[l] = coordinates entering layer l
    float* hs;   // [(L+1)][N][128] hs[l] = features entering layer l (hs[l+1] = x2h output = h2x input)
    // node stage of every attention block as the forward computed it (block 2l = x2h of layer l, 2l+1 = h2x): the
    // projection P [N][640] and the folded query Qt [N][16][128].  177 KB per node and layer -- 3.2 GB for a 32-graph
    // batch, a cheap trade on a 288 GB part for not running three node kernels per block again in the backward.
    float* P;    // [2L][N][640]
    float* Qt;   // [2L][N][16][128]
    size_t total;
};

static Tape carve_tape(void* base, int n, int L) {
    Tape t;
    Carver c(base);
    const size_t N = (size_t)(n > 0 ? n : 1);
    t.nbr = c.take<int32_t>(N * KNN * 4);
    t.deg = c.take<int32_t>(N * 4);
    t.e_w = c.take<float>(N * KNN * 4);
    t.xs = c.take<float>((size_t)(L + 1) * N * 3 * 4);
    t.hs = c.take<float>((size_t)(L + 1) * N * H * 4);
    t.P = c.take<float>((size_t)2 * L * N * PROW * 4);
    t.Qt = c.take<float>((size_t)2 * L * N * HEADS * H * 4);
    t.total = c.off;
    return t;
}

// ---- backward workspace -----------------------------------------------------------------------------------
// the per-block buffers: two sets, consecutive blocks alternate between them (BlockOverlap)
struct BlockSet {
    float *T, *S, *sw, *qs, *dqb, *zb, *dP;
    // an attention block's three slab sets live side by side (edge slabs in `partial`), so that ONE fold launch and ONE
    // reduce-and-store launch per block serve all of them
    float *partial, *folded, *partial_node, *partial_wgrad, *folded_node, *folded_wgrad;
};

struct TrainWs {
    float *P, *Qt, *Gt, *gb, *gh, *gx[2], *de_w, *tmp, *qln, *nk;
    BlockSet set[2];
    NodeList act;         // gen_flag rows (h2x work list)
    uint8_t* mask;        // receptive field of the loss, walked backwards (see cbgx_unitransformer_backward)
    NodeList A1, A2, A3;  // receptive-field lists, one hop apart
    // The third list has two lives: A3 of the pruned taped forward, and in the backward the classifier head's row list -- the rows with
    // lig_flag (or the support of grad_logits), which the head's backward walks when the loss reads ligand rows only
    NodeList head_rows() const { return A3; }
    float *gate_partial, *gate_folded;     // the gate backward's own slabs: it runs before the auxiliary stream is joined (round 6)
    // round 6, x2h edge backward without neighbour-row atomics (train_scatter.hip, CBGX_BX_EDGE_ROWS=1): one row per edge, and the
    // incoming-edge lists of every source node (built once per backward call)
    float* dE;            // [N][32][256]
    int *rin_cnt, *rin_ptr, *rin_tmp, *rin_edge;
    size_t total;
};

static BlockSet carve_block_set(Carver& c, size_t N) {
    BlockSet b;
    for (float** p : {&b.T, &b.S}) *p = c.take<float>(N * HEADS * H * 4);
    b.sw = c.take<float>(N * HEADS * 4);
    for (float** p : {&b.qs, &b.dqb, &b.zb}) *p = c.take<float>(N * H * 4);
    b.dP = c.take<float>(N * PROW * 4 + 256);      // + the x2h edge backward's work counters: zeroed by the same fill
    // (the largest of the slab sets that borrow it: edge kernel, node-level reductions, split products, gate)
    b.partial = c.take<float>(4 * std::max({(size_t)EDGE_GRID * PB_SIZE, (size_t)NODE_GRID * NS_SIZE, (size_t)MAX_SPLITS * H * PROW,
                                            (size_t)GATE_GRID * GB_SIZE}));
    b.folded = c.take<float>((size_t)FOLD * H * PROW * 4);
    b.partial_node = c.take<float>((size_t)NODE_GRID * NS_SIZE * 4);
    b.partial_wgrad = c.take<float>((size_t)MAX_SPLITS * H * PROW * 4);
    b.folded_node = c.take<float>((size_t)FOLD * NS_SIZE * 4);
    b.folded_wgrad = c.take<float>((size_t)FOLD * H * PROW * 4);
    return b;
}

// The only place that knows where a list's count lives: 64 bytes apart (a counter word is hammered by returning atomics).
static TrainWs carve_train(void* base, int n) {
    TrainWs w;
    Carver c(base);
    const size_t N = (size_t)(n > 0 ? n : 1);
    w.P = c.take<float>(N * PROW * 4);
    for (float** p : {&w.Qt, &w.Gt}) *p = c.take<float>(N * HEADS * H * 4);
    w.gb = c.take<float>(N * HEADS * 4);
    w.set[0] = carve_block_set(c, N);
    w.gh = c.take<float>(N * H * 4);
    for (float*& g : w.gx) g = c.take<float>(N * 3 * 4);
    w.de_w = c.take<float>(N * KNN * 4);
    w.tmp = c.take<float>(N * H * 4);
    w.act.rows = c.take<int>(N * 4);
    w.act.count = c.take<int>(256);
    w.mask = c.take<uint8_t>(N);
    w.A1.rows = c.take<int>(N * 4);
    w.A2.rows = c.take<int>(N * 4);
    int* counts = c.take<int>(256);
    w.A1.count = counts; w.A2.count = counts + 16; w.A3.count = counts + 32;
    w.A3.rows = c.take<int>(N * 4);
    w.qln = c.take<float>((size_t)QLN_SLOTS * 2 * H * 4);
    w.nk = c.take<float>(BX_NK_FLOATS * 4);     // x2h edge backward: the key path of every wave in flight, parked between two phases
    w.gate_partial = c.take<float>((size_t)GATE_GRID * GB_SIZE * 4);
    w.gate_folded = c.take<float>((size_t)FOLD * GB_SIZE * 4);
    w.dE = c.take<float>(N * KNN * 2 * H * 4);
    w.rin_cnt = c.take<int>(N * 4);
    w.rin_ptr = c.take<int>((N + 1) * 4);
    for (int** p : {&w.rin_tmp, &w.rin_edge}) *p = c.take<int>(N * KNN * 4);
    w.set[1] = carve_block_set(c, N);
    w.total = c.off;
    return w;
}

static inline int edge_grid(int n) { return n < EDGE_GRID ? (n > 0 ? n : 1) : EDGE_GRID; }
static inline int node_grid(int n) { return n < NODE_GRID ? (n > 0 ? n : 1) : NODE_GRID; }
// node groups of wgrad_mfma_kernel: at least 128 nodes (8 passes) each
#ifndef CBGX_WGRAD_GROUPS_MAX
#define CBGX_WGRAD_GROUPS_MAX 51      // x 5 column blocks = 255 workgroups, one round on 256 CUs; 16.7 MB of partial slabs instead of 42
                                      // (A/B, scripts/build_variant.py: 128 -> 1944, 102 -> 1965, 64 -> 1957, 51 -> 1968 graph-steps/s)
#endif
static inline int wgrad_groups(int n) {
    int g = (n + 127) / 128;
    return g < 1 ? 1 : (g > CBGX_WGRAD_GROUPS_MAX ? CBGX_WGRAD_GROUPS_MAX : g);
}
static inline int splits_for(int n) {
    int s = (n + 511) / 512;
    return s < 1 ? 1 : (s > MAX_SPLITS ? MAX_SPLITS : s);
}

// two-level reduction of `n_slabs` partial slabs of `size` floats: what reduce_store then reads is the FOLD-slab buffer `folded`
// (stride = size), or the input itself when it is already small
struct Slabs { const float* p; int n; size_t stride; };
static int fold_slabs(const float* src, int n_slabs, size_t stride, int size, float* folded, Slabs& out, hipStream_t s) {
    if (n_slabs <= FOLD) { out = Slabs{src, n_slabs, stride}; return CBGX_OK; }
    HIP_TRY(launch_slab_fold(src, n_slabs, stride, size, FOLD, folded, s));
    out = Slabs{folded, FOLD, (size_t)size};
    return CBGX_OK;
}

// Backward of one attention block.
//   x2h: g_out = dL/dh_out [N,128];   h2x: g_out = dL/dx_out [N,3] (only gen rows matter; rows = gen list)
// Effects: gh [N,128] += dL/dh_in contributions (x2h: gh must already hold g_out -- the residual path -- and is
// updated in place; h2x: gh += ...), dx [N,3] += coordinate gradients (atomics), de_w += gate gradients,
// grads[18] (k6 v6 q6 tensors, reference layouts) overwritten.
// Round 5: `ov` (optional) -- the weight-gradient part of the block (the node-level outer products and column sums, the dense
// projection's weight gradient, the slab folds and the reduce-and-store of all 18 tensors: ~135 us of small kernels per block,
// 2 ms of a 16 ms training step, none of it needed by the next block) runs on an auxiliary stream behind a fork event recorded
// after the query backward, while the caller's stream goes on with dgrad and the next block.  Consecutive blocks alternate between
// two sets of the buffers those kernels read (T, S, sw, qs, dqb, zb, dP and the slab sets); before a block touches its set it waits
// for the auxiliary work of the block that used the set before it (two blocks earlier -- which also covers g_out: the x2h block two
// blocks later is the first to overwrite the gradient buffer an x2h block's outer products read).
struct BlockOverlap {
    AuxStream* aux;       // auxiliary stream + events of the caller's stream (api.hip); NULL: everything on the caller's stream
    int next_set;       // set of the next block
    bool used[2];       // done[set] has been recorded
    bool joined = false;
    // Every exit path joins the auxiliary stream: an RC_TRY / HIP_TRY return from inside the layer loop must not leave it writing
    // gradients and slab buffers that the caller -- or the next call on this workspace, which starts with used = {false, false} and
    // would wait on nothing -- reuses.  The success path joins with stream-side waits (cbgx_unitransformer_backward, below) and sets
    // `joined`; a failure path blocks the host here until the auxiliary stream has drained.
    ~BlockOverlap() {
        if (aux && !joined && (used[0] || used[1])) (void)hipStreamSynchronize(aux->s);
    }
};

struct BlockArgs {
    // the block: x2h or h2x, its packed weights, its inputs as the forward saw them, the gradient of its output, the graph
    bool x2h = false;
    const float *att = nullptr, *x = nullptr, *h_in = nullptr, *g_out = nullptr;
    Graph g{};                  // (gen is not read: a block's movable rows are its `rows`)
    RowList rows;               // destination rows of the block (default: every row)
    // (h2x blocks) a list that contains every row of dP this block can touch (the listed nodes and their neighbours); the dense
    // products and column sums over dP then walk the list instead of all N rows
    RowList dp_rows;
    // the outputs
    float *gh = nullptr, *dx = nullptr, *de_w = nullptr;
    float* const* grads = nullptr;
    // gh = gh_src + (this block's contribution) instead of gh += (the caller then needs no snapshot of g_out == gh_src)
    const float* gh_src = nullptr;
    // (h2x blocks of a layer loop) dx = dx_init (the identity path of x_{l+1} = x_l + ...) before the block adds to it
    const float* dx_init = nullptr;
    const float *P_saved = nullptr, *Qt_saved = nullptr;    // the forward's own node stage from the tape (without both: recomputed)
    float* qln = nullptr;       // [2][128] zeroed accumulator of the query LayerNorm's affine gradients (nullptr: w.qln, zeroed here)
    BlockOverlap* ov = nullptr;
    bool rin_ready = false;     // the caller has built the incoming-edge lists (w.rin_ptr / rin_edge): the edge-row mode may run
};

static int attention_block_backward(const BlockArgs& a, TrainWs& w, hipStream_t s) {
    const bool x2h = a.x2h;
    const int n = a.g.n_nodes;
    BlockOverlap* const ov = a.ov;
    const RowList rows = a.rows, dp_rows = a.dp_rows;
    const float* dx_init = a.dx_init;
    float* qln = a.qln;
    const int set = (ov && ov->aux) ? ov->next_set : 0;
    BlockSet& b = w.set[set];      // this block's per-block buffers
    if (ov && ov->aux) {
        if (ov->used[set]) HIP_TRY(hipStreamWaitEvent(s, ov->aux->done[set], 0));    // the set's previous user has finished with it
        ov->next_set = set ^ 1;
    }
    // x2h blocks run the one-wave-per-node backward (8 nodes in flight per workgroup); h2x blocks and, in libcbgx_xcheck.so,
    // cbgx_debug_set_edge_kernel(2) the second-generation workgroup-per-node kernel
    const bool gen3 = x2h && g_edge_impl == 0;
    // (gen3: 8 nodes in flight per workgroup; a grid that is a multiple of 8 switches on its XCD-aware node partition)
    int eg = gen3 ? edge_grid((n + 7) / 8) : edge_grid(n);
    // with the weight-gradient kernels on the auxiliary stream (BlockOverlap), the x2h edge backward may leave a few compute units to
    // them: it takes a CU whole, so on 256 workgroups nothing runs next to it (CBGX_BX_GRID: its largest grid; an experiment knob)
    static const int bx_grid = [] { const char* e = getenv("CBGX_BX_GRID"); const int v = e ? atoi(e) : 0; return v >= 8 && v <= EDGE_GRID ? v : EDGE_GRID; }();
    if (gen3 && ov && ov->aux && eg > bx_grid) eg = bx_grid;
    if (gen3 && eg >= 64) eg &= ~7;
    const int ng = node_grid(n);
    // recompute the node stage of the forward: the MFMA node kernels (centred projection; own columns and query fold only
    // for the listed rows) with the MFMA edge backward, the first-generation ones with the VALU cross-check kernel
    // (skipped when the taped forward left its own P / Qt: P_saved, Qt_saved)
    const bool mfma = g_edge_impl != 1;
    const bool saved = a.P_saved && a.Qt_saved;
    const float* Pn = saved ? a.P_saved : w.P;
    const float* Qn = saved ? a.Qt_saved : w.Qt;
    if (!saved) {
#ifdef CBGX_XCHECK
        if (!mfma) {
            HIP_TRY(launch_node_gemm_v1(a.h_in, H, a.att + A_WN, a.att + A_BN, w.P, PROW, n, PROW, 0, s, {}));
            HIP_TRY(launch_node_query_v1(a.att, w.P, w.Qt, n, s));
        } else
#endif
        {
            NodeStageOpts o;
            o.large_lists = x2h;
            HIP_TRY(launch_node_mfma(a.att, a.h_in, a.g.lig, n, NodeBufs{w.P, b.qs, w.Qt}, rows, {}, s, o));
        }
    }
    if (x2h) HIP_TRY(launch_fold_grad(a.att, a.g_out, n, w.Gt, w.gb, s, mfma ? rows : RowList()));      // (a listed block reads listed rows' folds only)
    // Edge rows (CBGX_BX_EDGE_ROWS=1, round 6): a full launch of the one-wave-per-node kernel writes d pre of every edge to the edge's own
    // row of w.dE and launch_edge_rows_reduce gathers the rows of every source node in a fixed order -- no atomics on dP.  Every column
    // of dP then has exactly one writer (PD: the edge kernel's plain stores, PS: the gather, q hidden: the query backward), so only the
    // work counters behind it are zeroed.
    const bool er = gen3 && !rows.rows && a.rin_ready;
    if (er) HIP_TRY(hipMemsetAsync(b.dP + (size_t)n * PROW, 0, 256, s));
    else if (!x2h && dp_rows.rows && mfma && ov && ov->aux && env_on("CBGX_TRAIN_ZERO_ROWS"))
        // h2x block in the layer loop: every reader of dP walks `dp_rows`, so only those rows are zeroed (a fill of all N rows was 42 MB
        // per block; +0.4 % on the training line, profiles/ab_train_r06r.log)
    {
        HIP_TRY(launch_zero_rows(b.dP, PROW, dp_rows, n, s, dx_init ? a.dx : nullptr, dx_init, n * 3));
        dx_init = nullptr;
    } else HIP_TRY(hipMemsetAsync(b.dP, 0, (size_t)n * PROW * sizeof(float) + 256, s));     // (and the work counters behind it)
    if (dx_init) HIP_TRY(hipMemcpyAsync(a.dx, dx_init, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (!qln) {
        qln = w.qln;
        HIP_TRY(hipMemsetAsync(qln, 0, 2 * H * sizeof(float), s));
    }
    // libcbgx_xcheck.so only: cbgx_debug_set_edge_kernel(1) selects the first-generation (VALU) backward kernels as an
    // on-device cross-check
#ifdef CBGX_XCHECK
    if (!mfma)
        HIP_TRY(launch_edge_backward(x2h, a.att, a.g, a.x, Pn, Qn, w.Gt, w.gb, a.g_out, rows, b.T, b.S, b.sw, b.dP, a.dx, a.de_w,
                                     b.partial, eg, s));
    else
#endif
    if (gen3) {
        HIP_TRY(launch_edge_backward_x2h(a.att, a.g, a.x, Pn, Qn, w.Gt, w.gb, rows, b.T, b.S, b.sw, b.dP, a.dx, a.de_w, b.partial, w.nk,
                                         reinterpret_cast<int*>(b.dP + (size_t)n * PROW), eg, s, er ? w.dE : nullptr));
        if (er) HIP_TRY(launch_edge_rows_reduce(w.dE, w.rin_ptr, w.rin_edge, n, b.dP, s));
    } else
        HIP_TRY(launch_edge_backward_mfma(x2h, a.att, a.g, a.x, Pn, Qn, w.Gt, w.gb, a.g_out, rows, b.T, b.S, b.sw, b.dP, a.dx, a.de_w,
                                          b.partial, eg, s, 1));
    float *k0w = a.grads[0], *k0b = a.grads[1], *kg = a.grads[2], *kb = a.grads[3], *k1w = a.grads[4], *k1b = a.grads[5];
    float *v0w = a.grads[6], *v0b = a.grads[7], *vg = a.grads[8], *vb = a.grads[9], *v1w = a.grads[10], *v1b = a.grads[11];
    float *q0w = a.grads[12], *q0b = a.grads[13], *qg = a.grads[14], *qb = a.grads[15], *q1w = a.grads[16], *q1b = a.grads[17];
    // The block's three slab sets (edge kernel, node-level reductions, dense projection) are reduced at its end: one first-level
    // fold launch for the sets with more than FOLD slabs, one reduce-and-store launch for every gradient tensor of the block
    // (six launches and three 512-byte fills per block before; the sums are the same, slab by slab).
    RsBatch rb;
    rb.n = 0;
    FoldBatch fb;
    fb.n = 0;
    bool batch_overflow = false;      // (a stack struct passed by value to a kernel must not be overrun by one more piece)
    auto piece = [&](const float* src, int nsl, size_t stride, int ld, int rws, int cls, float* dst, int dld, int tr) {
        if (rb.n >= RS_MAX) { batch_overflow = true; return; }
        rb.p[rb.n++] = RsPiece{src, dst, stride, nsl, ld, rws, cls, dld, tr};
    };
    const float* fz; int fn; size_t fs;
    auto folded = [&](const float* src, int nsl, size_t stride, int size, float* dst) {
        if (nsl <= FOLD) { fz = src; fn = nsl; fs = stride; return; }
        if (fb.n >= FOLD_JOBS_MAX) { batch_overflow = true; fz = src; fn = nsl; fs = stride; return; }
        fb.j[fb.n++] = FoldJob{src, dst, stride, nsl, size};
        fz = dst; fn = FOLD; fs = (size_t)size;
    };
    {   // edge-indexed weight gradients: type / rbf columns of the first Linears, LayerNorm affine
        folded(b.partial, eg, PB_SIZE, PB_SIZE, b.folded);
        piece(fz + PB_WT, fn, fs, 2 * H, NT, H, k0w, KV_IN, 1);
        piece(fz + PB_WT + H, fn, fs, 2 * H, NT, H, v0w, KV_IN, 1);
        piece(fz + PB_WR, fn, fs, 2 * H, NT * G, H, k0w + NT, KV_IN, 1);
        piece(fz + PB_WR + H, fn, fs, 2 * H, NT * G, H, v0w + NT, KV_IN, 1);
        piece(fz + PB_LNG, fn, fs, H, 1, H, kg, H, 0);
        piece(fz + PB_LNG + H, fn, fs, H, 1, H, vg, H, 0);
        piece(fz + PB_LNB, fn, fs, H, 1, H, kb, H, 0);
        piece(fz + PB_LNB + H, fn, fs, H, 1, H, vb, H, 0);
        if (!x2h) {
            piece(fz + PB_WBV16, fn, fs, H, HEADS, H, v1w, H, 0);
            piece(fz + PB_BBV16, fn, fs, HEADS, 1, HEADS, v1b, HEADS, 0);
        }
    }
    // query MLP backward (fills dP[:, 512:640]); its LayerNorm affine gradients are accumulated into qln by atomics
    {
        const int tiles = (n + 15) / 16, qgrid = tiles < 1024 ? tiles : 1024;   // 25 KB of LDS, four waves per SIMD: four workgroups per CU
#ifdef CBGX_XCHECK
        if (!mfma) HIP_TRY(launch_q_backward(a.att, Pn, b.T, rows, n, b.qs, b.dqb, b.zb, b.dP, qln, qgrid, s));
        else
#endif
            HIP_TRY(launch_q_backward_mfma(a.att, Pn, b.T, rows, n, b.qs, b.dqb, b.zb, b.dP, qln, qgrid, s));
    }
    // ---- from here to the reduce-and-store: weight gradients only.  With `ov` they go to the auxiliary stream (`s` is shadowed) and
    // dgrad -- what the next block waits for -- is issued on the caller's stream first.
    hipStream_t s_main = s;
    const bool deferred = ov && ov->aux;
    // dL/dh_in = (gh_src or gh itself) + dP Wn^T
    auto dgrad = [&](hipStream_t st) -> int {
        if (mfma)
            HIP_TRY(launch_dgrad_mfma(b.dP, PROW, a.att + A_WN, PROW, a.gh, H, n, PROW, 1, st, a.gh_src, a.gh_src ? RowList() : dp_rows));
        else {
            if (a.gh_src && a.gh_src != a.gh) HIP_TRY(hipMemcpyAsync(a.gh, a.gh_src, (size_t)n * H * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(launch_sgemm(false, true, b.dP, PROW, a.att + A_WN, PROW, a.gh, H, n, H, PROW, 1, 0, 1, st));
        }
        return CBGX_OK;
    };
    if (deferred) {
        HIP_TRY(hipEventRecord(ov->aux->fork, s_main));
        HIP_TRY(hipStreamWaitEvent(ov->aux->s, ov->aux->fork, 0));
        RC_TRY(dgrad(s_main));
        s = ov->aux->s;
    }
    // node-level reductions, all into one slab per workgroup (NS_* layout), folded and scattered once:
    //   second Linears: dWbk = sum_i (q_i / sqrt 8) (x) T_i ;  x2h: dWbv = sum_i G_i (x) S_i ;  dWq1 = sum_i dq_i (x) z_i
    //   biases: second v / q Linears, and the first Linears = column sums of dP (k | v | - | - | q hidden)
#ifdef CBGX_XCHECK
    const auto outer = mfma ? launch_outer_accum_mfma : launch_outer_accum;
#else
    const auto outer = launch_outer_accum_mfma;
#endif
    float* pn = b.partial_node;
    HIP_TRY(outer(true, b.qs, b.T, rows, n, pn + NS_WBK, NS_SIZE, ng, s));
    if (x2h) {
        HIP_TRY(outer(true, a.g_out, b.S, rows, n, pn + NS_WBV, NS_SIZE, ng, s));
        HIP_TRY(launch_colsum(a.g_out, H, H, b.sw, rows, n, pn + NS_V1B, NS_SIZE, ng, s));
    }
    HIP_TRY(outer(false, b.dqb, b.zb, rows, n, pn + NS_WQ1, NS_SIZE, ng, s));
    HIP_TRY(launch_colsum(b.dqb, H, H, nullptr, rows, n, pn + NS_Q1B, NS_SIZE, ng, s));
    HIP_TRY(launch_colsum(b.dP, PROW, PROW, nullptr, dp_rows, n, pn + NS_DP, NS_SIZE, ng, s));
    {
        folded(pn, ng, NS_SIZE, NS_SIZE, b.folded_node);
        piece(fz + NS_WBK, fn, fs, H, H, H, k1w, H, 0);
        piece(fz + NS_WQ1, fn, fs, H, H, H, q1w, H, 0);
        piece(fz + NS_Q1B, fn, fs, H, 1, H, q1b, H, 0);
        piece(fz + NS_DP, fn, fs, PROW, 1, H, k0b, H, 0);
        piece(fz + NS_DP + H, fn, fs, PROW, 1, H, v0b, H, 0);
        piece(fz + NS_DP + 4 * H, fn, fs, PROW, 1, H, q0b, H, 0);
        if (x2h) {
            piece(fz + NS_WBV, fn, fs, H, H, H, v1w, H, 0);
            piece(fz + NS_V1B, fn, fs, H, 1, H, v1b, H, 0);
        }
        piece(qln, 1, 0, H, 1, H, qg, H, 0);
        piece(qln + H, 1, 0, H, 1, H, qb, H, 0);
        piece(qln, 0, 0, H, 1, H, k1b, H, 0);      // a sum over zero slabs: the key bias cancels in the softmax, its gradient is 0
    }
    // dense projection: dWn[k][n] = sum_i h_in[i][k] dP[i][n]  -> h_dst / h_src / q columns of the first Linears
    const int sp = mfma ? wgrad_groups(n) : (splits_for(n) > 32 ? 32 : splits_for(n));
    if (mfma)
        HIP_TRY(launch_wgrad_mfma(a.h_in, H, b.dP, PROW, n, PROW / H, b.partial_wgrad, PROW, (size_t)H * PROW, sp, s, dp_rows));
    else
        HIP_TRY(launch_sgemm(true, false, a.h_in, H, b.dP, PROW, b.partial_wgrad, PROW, H, PROW, n, sp, (size_t)H * PROW, 0, s));
    {
        folded(b.partial_wgrad, sp, (size_t)H * PROW, H * PROW, b.folded_wgrad);
        piece(fz + 0 * H, fn, fs, PROW, H, H, k0w + NT + NT * G, KV_IN, 1);
        piece(fz + 1 * H, fn, fs, PROW, H, H, v0w + NT + NT * G, KV_IN, 1);
        piece(fz + 2 * H, fn, fs, PROW, H, H, k0w + NT + NT * G + H, KV_IN, 1);
        piece(fz + 3 * H, fn, fs, PROW, H, H, v0w + NT + NT * G + H, KV_IN, 1);
        piece(fz + 4 * H, fn, fs, PROW, H, H, q0w, H, 1);
    }
    if (batch_overflow) return cbgx::set_error(CBGX_E_INVALID, "backward: reduce batch overflow (RS_MAX / FOLD_JOBS_MAX too small)");
    HIP_TRY(launch_slab_fold_multi(fb, FOLD, s));
    HIP_TRY(launch_reduce_store_multi(rb, s));
    if (deferred) {
        HIP_TRY(hipEventRecord(ov->aux->done[set], s));
        ov->used[set] = true;
        return CBGX_OK;       // (dgrad was issued above, on the caller's stream)
    }
    return dgrad(s);
}

// backward of the distance gate: weight gradients from the accumulated dL/de_w, on the workspace's gate slabs (no buffer of a block set);
// grad_x != NULL: the gate's coordinate gradient is also ADDED to grad_x (the kernel's DX variant)
static int gate_backward(const float* packed, const float* xs, const int32_t* nbr, const int32_t* deg, int n, TrainWs& w,
                         float* const* grads, hipStream_t s, RowList rows, float* grad_x) {
    HIP_TRY(launch_gate_backward_mfma(packed, xs, nbr, deg, n, w.de_w, w.gate_partial, GATE_GRID, s, rows, grad_x));
    Slabs f;
    RC_TRY(fold_slabs(w.gate_partial, GATE_GRID, GB_SIZE, GB_SIZE, w.gate_folded, f, s));
    auto rs = [&](int off, int ld, int rws, int cls, float* dst) { return launch_reduce_store(f.p + off, f.n, f.stride, ld, rws, cls, dst, ld, 0, s); };
    HIP_TRY(rs(GB_W1, G, GH, G, grads[0]));
    HIP_TRY(rs(GB_B1, GH, 1, GH, grads[1]));
    HIP_TRY(rs(GB_LNG, GH, 1, GH, grads[2]));
    HIP_TRY(rs(GB_LNB, GH, 1, GH, grads[3]));
    HIP_TRY(rs(GB_W2, GH, 1, GH, grads[4]));
    HIP_TRY(rs(GB_B2, 1, 1, 1, grads[5]));
    return CBGX_OK;
}

// Backward of the classifier head (Linear, shifted softplus, Linear on h_L = `hl`; `c`: its packed weights): cg[0..3] = dW0, db0, dW1,
// db1 are overwritten and w.gh += dL/dh_L.  `rows`: rows outside it have a zero grad_logits -- the ligand rows by the caller's promise
// behind grad_h_out == NULL (include/cbgx.h: its loss reads the logits on lig_flag rows only), or the support marked on the device.
// The head then walks a twentieth of the nodes: listed node GEMMs for the recompute, listed weight- / input-gradient products, nothing
// read outside the list.  {NULL, NULL}: every row.  The scratch is borrowed from block set 0 (no block has run yet).
static int classifier_head_backward(const float* c, int C, const float* hl, const float* grad_logits, int n, TrainWs& w,
                                    float* const* cg, RowList rows, hipStream_t s) {
    BlockSet& b = w.set[0];
    float *pre = b.qs, *act = b.zb, *dact = b.dqb;      // [N,128] scratch (a listed head: listed rows only)
    const int ng = node_grid(n), sp = splits_for(n), wg = wgrad_groups(n);
    const bool mfma = g_edge_impl != 1;      // (a listed head always is)
    // sum of `nsl` slabs [rws][cls] in b.partial -> dst
    auto reduce = [&](int nsl, int rws, int cls, float* dst) -> int {
        Slabs f;
        RC_TRY(fold_slabs(b.partial, nsl, (size_t)rws * cls, rws * cls, b.folded, f, s));
        HIP_TRY(launch_reduce_store(f.p, f.n, f.stride, cls, rws, cls, dst, cls, 0, s));
        return CBGX_OK;
    };
    HIP_TRY(launch_node_gemm(hl, H, c + C_W0T, c + C_B0, pre, H, n, H, 0, s, rows));
    HIP_TRY(launch_node_gemm(hl, H, c + C_W0T, c + C_B0, act, H, n, H, 1, s, rows));
    // classifier.2: dW1[c][k] = sum_i dlogits[i][c] act[i][k];  db1 = colsum(dlogits)
    if (rows.rows) HIP_TRY(launch_cls_w1_grad_rows(grad_logits, C, act, rows, cg[2], s));
    else {
        HIP_TRY(launch_sgemm(true, false, grad_logits, C, act, H, b.partial, H, C, H, n, sp, (size_t)C * H, 0, s));
        RC_TRY(reduce(sp, C, H, cg[2]));
    }
    HIP_TRY(launch_colsum(grad_logits, C, C, nullptr, rows, n, b.partial, C, ng, s));
    RC_TRY(reduce(ng, 1, C, cg[3]));
    // d(act) = dlogits W1 (C_W1T is [128][C]; all rows: a [N x C] x [C x 128] product, zero outside the list);  d(pre) = d(act) sigmoid(pre)
    HIP_TRY(launch_sgemm(false, true, grad_logits, C, c + C_W1T, C, dact, H, n, H, C, 1, 0, 0, s));
    if (rows.rows) HIP_TRY(launch_ssp_backward_rows(pre, dact, rows, n, w.tmp, s));
    else HIP_TRY(launch_ssp_backward(pre, dact, (long)n * H, w.tmp, s));
    // classifier.0: dW0[n][k] = sum_i dpre[i][n] h[i][k];  db0 = colsum(dpre);  dh += dpre W0
    if (mfma) HIP_TRY(launch_wgrad_mfma(w.tmp, H, hl, H, n, 1, b.partial, H, (size_t)H * H, wg, s, rows));
    else HIP_TRY(launch_sgemm(true, false, w.tmp, H, hl, H, b.partial, H, H, H, n, sp, (size_t)H * H, 0, s));
    RC_TRY(reduce(mfma ? wg : sp, H, H, cg[0]));
    HIP_TRY(launch_colsum(w.tmp, H, H, nullptr, rows, n, b.partial, H, ng, s));
    RC_TRY(reduce(ng, 1, H, cg[1]));
    if (mfma) HIP_TRY(launch_dgrad_mfma(w.tmp, H, c + C_W0T, H, w.gh, H, n, H, 1, s, nullptr, rows));
    else HIP_TRY(launch_sgemm(false, true, w.tmp, H, c + C_W0T, H, w.gh, H, n, H, H, 1, 0, 1, s));
    return CBGX_OK;
}

static int check_grads(float* const* g, int count, const char* who) {
    if (!g) return set_error(CBGX_E_INVALID, "%s: grads is NULL", who);
    for (int i = 0; i < count; ++i)
        if (!g[i]) return set_error(CBGX_E_INVALID, "%s: grads[%d] is NULL", who, i);
    return CBGX_OK;
}

// carve + size check of the entry points that take a training workspace / a denoiser tape (as carve_checked, api.hip)
static int carve_train_checked(const char* who, void* workspace, size_t bytes, int n, TrainWs& w) {
    w = carve_train(workspace, n);
    return bytes < w.total ? set_error(CBGX_E_WORKSPACE, "%s: workspace %zu < %zu", who, bytes, w.total) : CBGX_OK;
}
static int carve_tape_checked(const char* who, const void* tape, size_t bytes, int n, int L, Tape& tp) {
    tp = carve_tape((void*)tape, n, L);
    return bytes < tp.total ? set_error(CBGX_E_WORKSPACE, "%s: tape %zu < %zu", who, bytes, tp.total) : CBGX_OK;
}

extern "C" {

size_t cbgx_train_tape_bytes(int n_nodes, int num_layers) {
    if (n_nodes < 0 || num_layers < 1) return 0;
    return carve_tape(nullptr, n_nodes, num_layers).total;
}

size_t cbgx_train_workspace_bytes(int n_nodes) {
    if (n_nodes < 0) return 0;
    return carve_train(nullptr, n_nodes).total;
}

int cbgx_unitransformer_forward_train(const float* packed, int num_layers, int num_classes, const float* x,
                                      const float* h, const int32_t* graph_ptr, const uint8_t* lig_flag,
                                      const uint8_t* gen_flag, int n_nodes, int n_graphs, float* x_out, float* h_out,
                                      float* logits, void* tape, size_t tape_bytes, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return cbgx_unitransformer_forward_train_ex(packed, num_layers, num_classes, x, h, graph_ptr, lig_flag, gen_flag, n_nodes, n_graphs,
                                                x_out, h_out, logits, 0u, tape, tape_bytes, workspace, workspace_bytes, stream);
}

int cbgx_unitransformer_forward_train_ex(const float* packed, int num_layers, int num_classes, const float* x,
                                         const float* h, const int32_t* graph_ptr, const uint8_t* lig_flag,
                                         const uint8_t* gen_flag, int n_nodes, int n_graphs, float* x_out, float* h_out,
                                         float* logits, unsigned flags, void* tape, size_t tape_bytes, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    if (flags & ~CBGX_FWD_H_ON_SOURCES) return set_error(CBGX_E_INVALID, "forward_train: unknown flags 0x%x", flags);
    if (n_nodes < 0 || n_graphs < 0 || num_layers < 1) return set_error(CBGX_E_INVALID, "forward_train: bad sizes");
    if (num_classes > CBGX_MAX_CLASSES)
        return set_error(CBGX_E_INVALID, "forward_train: num_classes=%d > %d", num_classes, CBGX_MAX_CLASSES);
    if (n_nodes == 0) return CBGX_OK;
    if (!packed || !x || !h || !graph_ptr || !lig_flag || !gen_flag || !x_out || !tape || !workspace)
        return set_error(CBGX_E_INVALID, "forward_train: NULL pointer");
    Tape tp;
    RC_TRY(carve_tape_checked("forward_train", tape, tape_bytes, n_nodes, num_layers, tp));
    TrainWs w;
    RC_TRY(carve_train_checked("forward_train", workspace, workspace_bytes, n_nodes, w));
    hipStream_t s = (hipStream_t)stream;
    const size_t nx = (size_t)n_nodes * 3, nh = (size_t)n_nodes * H;
    HIP_TRY(hipMemcpyAsync(tp.xs, x, nx * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(tp.hs, h, nh * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(launch_knn(x, graph_ptr, n_graphs, n_nodes, tp.nbr, tp.deg, s));
    HIP_TRY(launch_gate(packed, x, tp.nbr, tp.deg, n_nodes, tp.e_w, s));
    HIP_TRY(launch_build_active(gen_flag, n_nodes, w.act, s));
    const Graph g{tp.nbr, tp.deg, tp.e_w, lig_flag, gen_flag, n_nodes};
    // Round 6: the node stage of the x2h block of layer l + 1 (projection, query MLP, fold: ~57 us at 16.5 k nodes) reads h_{l+1} only,
    // like the h2x block of layer l (~60 us) -- it runs on the caller's auxiliary stream next to that block (what the sampling forward
    // has done since round 3); every block owns its P / Qt on the tape, the two node stages use different query scratch rows.
    // +0.7 % on the training line (profiles/ab_train_r06r.log).  CBGX_TRAIN_OVERLAP=0 / CBGX_TRAIN_FWD_OVERLAP=0, the per-kernel
    // profile and the VALU cross-check kernels keep one stream.
    AuxStream* aux = (env_on("CBGX_TRAIN_OVERLAP") && env_on("CBGX_TRAIN_FWD_OVERLAP") && g_edge_impl == 0 && !profile_is_on() &&
                    num_layers > 1) ? aux_for(s) : nullptr;
    struct Joiner {     // a failure between fork and join must not leave the auxiliary stream writing the tape
        AuxStream* a; bool out = false;
        ~Joiner() { if (a && out) (void)hipStreamSynchronize(a->s); }
    } jn{aux};
    // Round 6, h_out == NULL (the caller does not read h': TargetDiff / DiffSBDD training, whose backward then comes with
    // grad_h_out == NULL and prunes the same way): the receptive-field pruning of the sampling forward.  The outputs that remain are
    // x_out and the logits of ligand rows, so the last x2h block only has to produce h' on A1 = gen | lig | nbr(gen), the one before it
    // on A2 = A1 | nbr(A1) (its sources: A3 = A2 | nbr(A2)); h2x blocks need the neighbour projection on nbr(gen) only (subset of A1).
    // Rows outside those sets are zero on the tape (the pruned backward's dense products over h walk all rows with zero weights).
    // (CBGX_FWD_H_ON_SOURCES: h_out is wanted, but on A1 only -- DiffBP's centre-of-mass head reads it on the movable atoms and their
    // neighbours; the backward then prunes around the support of its dL/dh_out, which lies inside A1, unless CBGX_TRAIN_PRUNE_GH=0)
    const bool fprune = (!h_out || ((flags & CBGX_FWD_H_ON_SOURCES) && env_on("CBGX_TRAIN_PRUNE_GH"))) && num_layers >= 3 &&
                        g_edge_impl != 1 && env_on("CBGX_TRAIN_FWD_PRUNE");
    const NodeList every{nullptr, nullptr};
    const NodeList A[3] = {w.A1, w.A2, w.A3};
    if (fprune) {
        HIP_TRY(launch_mark_seed(gen_flag, lig_flag, n_nodes, w.mask, s));
        HIP_TRY(walk_receptive_field(w.mask, w.act, tp.nbr, tp.deg, n_nodes, {w.A1, w.A2, w.A3}, s));
    }
    // (destination list, source list) of the x2h block of layer l
    auto x2h_lists = [&](int l, NodeList& d, NodeList& sr) {
        d = sr = every;
        const int k = num_layers - 1 - l;      // 0 for the last layer
        if (fprune && k < 2) { d = A[k]; sr = A[k + 1]; }
    };
    const NodeList a1 = fprune ? w.A1 : every;     // sources of the h2x blocks; rows of the logits
    float *qs = w.set[0].qs, *qs_aux = w.set[1].qs;     // query scratch borrowed from the block sets: caller's / auxiliary stream
    // the node stage of block k (2l: x2h, 2l + 1: h2x) lives on the tape; `q`: the query scratch of the stream it runs on
    auto bufs = [&](int k, float* q) { return NodeBufs{tp.P + (size_t)k * n_nodes * PROW, q, tp.Qt + (size_t)k * n_nodes * HEADS * H}; };
    NodeStageOpts large;
    large.large_lists = true;
    for (int l = 0; l < num_layers; ++l) {
        const float* xc = tp.xs + (size_t)l * nx;
        const float* hc = tp.hs + (size_t)l * nh;
        float* xn = tp.xs + (size_t)(l + 1) * nx;
        float* hn = tp.hs + (size_t)(l + 1) * nh;
        NodeList d, sr;
        x2h_lists(l, d, sr);
        if (d.rows) HIP_TRY(hipMemsetAsync(hn, 0, nh * 4, s));      // rows the listed launch does not write
        if (!aux) {
            HIP_TRY(launch_attention(true, packed + x2h_off(l), g, xc, hc, bufs(2 * l, qs), hn, nullptr, d, sr, s));
        } else {
            if (l == 0)
                HIP_TRY(launch_node_mfma(packed + x2h_off(0), hc, lig_flag, n_nodes, bufs(0, qs_aux), d, sr, s, large));
            else { HIP_TRY(hipStreamWaitEvent(s, aux->join, 0)); jn.out = false; }      // this layer's node stage (auxiliary stream)
            HIP_TRY(launch_edge_mfma(true, packed + x2h_off(l), g, xc, hc, bufs(2 * l, qs_aux), hn, nullptr, d, s));
            if (l + 1 < num_layers) {
                NodeList d2, s2;
                x2h_lists(l + 1, d2, s2);
                HIP_TRY(hipEventRecord(aux->fork, s));
                HIP_TRY(hipStreamWaitEvent(aux->s, aux->fork, 0));
                jn.out = true;
                HIP_TRY(launch_node_mfma(packed + x2h_off(l + 1), hn, lig_flag, n_nodes, bufs(2 * l + 2, qs_aux), d2, s2, aux->s, large));
                HIP_TRY(hipEventRecord(aux->join, aux->s));
            }
        }
        HIP_TRY(launch_attention(false, packed + h2x_off(l), g, xc, hn, bufs(2 * l + 1, qs), xn, nullptr, w.act, a1, s));
    }
    const float* hl = tp.hs + (size_t)num_layers * nh;
    HIP_TRY(hipMemcpyAsync(x_out, tp.xs + (size_t)num_layers * nx, nx * 4, hipMemcpyDeviceToDevice, s));
    if (h_out) HIP_TRY(hipMemcpyAsync(h_out, hl, nh * 4, hipMemcpyDeviceToDevice, s));
    if (logits) {
        if (num_classes < 1) return set_error(CBGX_E_INVALID, "forward_train: num_classes=%d", num_classes);
        const float* c = packed + cls_off(num_layers);
        // (pruned: the logits of the A1 rows -- the ligand rows are among them; other rows of `logits` are not written)
        HIP_TRY(launch_node_gemm(hl, H, c + C_W0T, c + C_B0, w.P, H, n_nodes, H, 1, s, a1));
        HIP_TRY(launch_node_gemm(w.P, H, c + C_W1T, c + cls_b1(num_classes), logits, num_classes, n_nodes, num_classes,
                                 0, s, a1));
    }
    return CBGX_OK;
}

int cbgx_x2h_attention_backward(const float* packed, int layer, const float* x, const float* h, const int32_t* nbr,
                                const int32_t* deg, const uint8_t* lig_flag, const float* e_w, int n_nodes,
                                const float* grad_h_out, float* grad_h, float* grad_x, float* grad_e_w,
                                float* const* grads, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_nodes <= 0 || layer < 0) return set_error(CBGX_E_INVALID, "x2h_backward: bad sizes");
    if (!packed || !x || !h || !nbr || !deg || !lig_flag || !e_w || !grad_h_out || !grad_h || !grad_x || !grad_e_w ||
        !workspace)
        return set_error(CBGX_E_INVALID, "x2h_backward: NULL pointer");
    RC_TRY(check_grads(grads, 18, "x2h_backward"));
    TrainWs w;
    RC_TRY(carve_train_checked("x2h_backward", workspace, workspace_bytes, n_nodes, w));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(grad_h, grad_h_out, (size_t)n_nodes * H * 4, hipMemcpyDeviceToDevice, s));   // residual
    HIP_TRY(hipMemsetAsync(grad_x, 0, (size_t)n_nodes * 3 * 4, s));
    HIP_TRY(hipMemsetAsync(grad_e_w, 0, (size_t)n_nodes * KNN * 4, s));
    const bool rin = edge_rows_mode() && g_edge_impl == 0;
    if (rin) HIP_TRY(launch_rin_build(nbr, deg, n_nodes, w.rin_cnt, w.rin_ptr, w.rin_tmp, w.rin_edge, s));
    BlockArgs a;
    a.x2h = true; a.att = packed + x2h_off(layer); a.x = x; a.h_in = h; a.g_out = grad_h_out;
    a.g = Graph{nbr, deg, e_w, lig_flag, nullptr, n_nodes};
    a.gh = grad_h; a.dx = grad_x; a.de_w = grad_e_w; a.grads = grads; a.rin_ready = rin;
    return attention_block_backward(a, w, s);
}

int cbgx_h2x_attention_backward(const float* packed, int layer, const float* x, const float* h, const int32_t* nbr,
                                const int32_t* deg, const uint8_t* lig_flag, const uint8_t* gen_flag, const float* e_w,
                                int n_nodes, const float* grad_x_out, float* grad_h, float* grad_x, float* grad_e_w,
                                float* const* grads, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_nodes <= 0 || layer < 0) return set_error(CBGX_E_INVALID, "h2x_backward: bad sizes");
    if (!packed || !x || !h || !nbr || !deg || !lig_flag || !gen_flag || !e_w || !grad_x_out || !grad_h || !grad_x ||
        !grad_e_w || !workspace)
        return set_error(CBGX_E_INVALID, "h2x_backward: NULL pointer");
    RC_TRY(check_grads(grads, 18, "h2x_backward"));
    TrainWs w;
    RC_TRY(carve_train_checked("h2x_backward", workspace, workspace_bytes, n_nodes, w));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_build_active(gen_flag, n_nodes, w.act, s));
    HIP_TRY(hipMemsetAsync(grad_h, 0, (size_t)n_nodes * H * 4, s));
    HIP_TRY(hipMemcpyAsync(grad_x, grad_x_out, (size_t)n_nodes * 3 * 4, hipMemcpyDeviceToDevice, s));   // x_out = x + ...
    HIP_TRY(hipMemsetAsync(grad_e_w, 0, (size_t)n_nodes * KNN * 4, s));
    BlockArgs a;
    a.att = packed + h2x_off(layer); a.x = x; a.h_in = h; a.g_out = grad_x_out;
    a.g = Graph{nbr, deg, e_w, lig_flag, gen_flag, n_nodes}; a.rows = w.act;
    a.gh = grad_h; a.dx = grad_x; a.de_w = grad_e_w; a.grads = grads;
    return attention_block_backward(a, w, s);
}

int cbgx_unitransformer_backward(const float* packed, int num_layers, int num_classes, const void* tape,
                                 size_t tape_bytes, const uint8_t* lig_flag, const uint8_t* gen_flag, int n_nodes,
                                 const float* grad_x_out, const float* grad_h_out, const float* grad_logits,
                                 float* const* grads, int num_grads, float* grad_h_in, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    return cbgx_unitransformer_backward_ex(packed, num_layers, num_classes, tape, tape_bytes, lig_flag, gen_flag, n_nodes, grad_x_out,
                                           grad_h_out, grad_logits, grads, num_grads, grad_h_in, nullptr, workspace, workspace_bytes,
                                           stream);
}

int cbgx_unitransformer_backward_ex(const float* packed, int num_layers, int num_classes, const void* tape,
                                    size_t tape_bytes, const uint8_t* lig_flag, const uint8_t* gen_flag, int n_nodes,
                                    const float* grad_x_out, const float* grad_h_out, const float* grad_logits,
                                    float* const* grads, int num_grads, float* grad_h_in, float* grad_x_in, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (n_nodes <= 0 || num_layers < 1 || num_classes < 1) return set_error(CBGX_E_INVALID, "backward: bad sizes");
    if (num_classes > CBGX_MAX_CLASSES) return set_error(CBGX_E_INVALID, "backward: num_classes=%d > %d", num_classes, CBGX_MAX_CLASSES);
    if (!packed || !tape || !lig_flag || !gen_flag || !workspace) return set_error(CBGX_E_INVALID, "backward: NULL pointer");
    if (num_grads != 6 + 36 * num_layers + 4)
        return set_error(CBGX_E_INVALID, "backward: expected %d gradient tensors, got %d", 6 + 36 * num_layers + 4, num_grads);
    RC_TRY(check_grads(grads, num_grads, "backward"));
    Tape tp;
    RC_TRY(carve_tape_checked("backward", tape, tape_bytes, n_nodes, num_layers, tp));
    TrainWs w;
    RC_TRY(carve_train_checked("backward", workspace, workspace_bytes, n_nodes, w));
    hipStream_t s = (hipStream_t)stream;
    const int n = n_nodes, L = num_layers, C = num_classes;
    const size_t nx = (size_t)n * 3, nh = (size_t)n * H;
    const NodeList every{nullptr, nullptr};
    const Graph graph{tp.nbr, tp.deg, tp.e_w, lig_flag, gen_flag, n};

    // dL/dh_L: the caller's gradient plus the classifier head
    if (grad_h_out) HIP_TRY(hipMemcpyAsync(w.gh, grad_h_out, nh * 4, hipMemcpyDeviceToDevice, s));
    else HIP_TRY(hipMemsetAsync(w.gh, 0, nh * 4, s));
    // (round 6: with a caller gradient on h_out the same listed head runs on the SUPPORT of grad_logits -- the rows with a non-zero
    // entry, marked on the device; DiffBP's losses read the logits of ligand rows only as well.  CBGX_TRAIN_PRUNE_GH=0: the dense head)
    const bool head_listed = grad_logits && g_edge_impl != 1 && (grad_h_out == nullptr || env_on("CBGX_TRAIN_PRUNE_GH"));
    if (grad_logits) {
        NodeList rows = every;
        if (head_listed) {
            rows = w.head_rows();
            if (grad_h_out) {       // no promise about grad_logits: its support
                HIP_TRY(launch_mark_nonzero_rows(grad_logits, n, w.mask, s, C, 1));
                HIP_TRY(launch_build_active(w.mask, n, rows, s));
            } else
                HIP_TRY(launch_build_active(lig_flag, n, rows, s));
        }
        RC_TRY(classifier_head_backward(packed + cls_off(L), C, tp.hs + (size_t)L * nh, grad_logits, n, w, grads + 6 + 36 * L, rows, s));
    } else {
        float* const* cg = grads + 6 + 36 * L;
        HIP_TRY(hipMemsetAsync(cg[0], 0, (size_t)H * H * 4, s));
        HIP_TRY(hipMemsetAsync(cg[1], 0, H * 4, s));
        HIP_TRY(hipMemsetAsync(cg[2], 0, (size_t)C * H * 4, s));
        HIP_TRY(hipMemsetAsync(cg[3], 0, C * 4, s));
    }
    int cur = 0;
    if (grad_x_out) HIP_TRY(hipMemcpyAsync(w.gx[cur], grad_x_out, nx * 4, hipMemcpyDeviceToDevice, s));
    else HIP_TRY(hipMemsetAsync(w.gx[cur], 0, nx * 4, s));
    HIP_TRY(hipMemsetAsync(w.de_w, 0, (size_t)n * KNN * 4, s));
    HIP_TRY(launch_build_active(gen_flag, n, w.act, s));
    // Receptive-field pruning, the mirror image of the forward's: without a caller gradient on h_out, dL/dh_L is non-zero
    // on ligand rows only (classifier), the last h2x block adds rows of A1 = gen | lig | nbr(gen), and the x2h block of a
    // layer spreads its input gradient one hop further (A2 = A1 | nbr(A1)).  Rows outside carry an exactly zero gradient
    // and contribute exactly zero to everything, so the last two x2h blocks are walked on A1 / A2 only.
    // Round 6: with a caller gradient on h_out the same pruning holds around ITS support (the rows with a non-zero entry, marked on
    // the device): DiffBP's centre-of-mass head reads h_out on the movable atoms and their neighbours only, and until now its
    // training ran all nine x2h blocks -- and the dense products of all nine h2x blocks -- on every row (CBGX_TRAIN_PRUNE_GH=0: as before).
    const bool prune = (grad_h_out == nullptr || env_on("CBGX_TRAIN_PRUNE_GH")) && L >= 3;
    if (prune) {
        HIP_TRY(launch_mark_seed(gen_flag, lig_flag, n, w.mask, s));
        if (grad_h_out) {       // the seed: every row where dL/dh_L can be non-zero (no promise about the caller's two gradients)
            HIP_TRY(launch_mark_nonzero_rows(grad_h_out, n, w.mask, s));
            if (grad_logits) HIP_TRY(launch_mark_nonzero_rows(grad_logits, n, w.mask, s, C, 0));
        }
        HIP_TRY(walk_receptive_field(w.mask, w.act, tp.nbr, tp.deg, n, {w.A1, w.A2}, s));
    }

    // one zeroed accumulator per attention block for the query LayerNorm's affine gradients (atomics): a single fill here
    // instead of one per block
    const bool qln_slots = 2 * L <= QLN_SLOTS;
    if (qln_slots) HIP_TRY(hipMemsetAsync(w.qln, 0, (size_t)2 * L * 2 * H * sizeof(float), s));
    float* gh_cur = w.gh;       // dL/dh of the layer boundary being crossed; the x2h blocks write the other buffer (no snapshot copy)
    float* gh_oth = w.tmp;
    // weight-gradient work of every block on the caller's auxiliary stream (attention_block_backward, BlockOverlap): off while the
    // per-kernel profile runs (its sections are timed on one stream), with the VALU cross-check kernels, or by CBGX_TRAIN_OVERLAP=0
    const bool overlap_env = env_on("CBGX_TRAIN_OVERLAP");
    // (and only with one query-LayerNorm accumulator slot per block: the shared fallback slot would be refilled by the next block
    // while the auxiliary stream still reads it)
    BlockOverlap ov{(overlap_env && g_edge_impl != 1 && !profile_is_on() && qln_slots) ? aux_for(s) : nullptr, 0, {false, false}};
    // edge-row mode: incoming-edge lists of every source node, once for all layers
    const bool rin = edge_rows_mode() && g_edge_impl == 0 && (!prune || L > 2);
    if (rin) HIP_TRY(launch_rin_build(tp.nbr, tp.deg, n, w.rin_cnt, w.rin_ptr, w.rin_tmp, w.rin_edge, s));
    for (int l = L - 1; l >= 0; --l) {
        const float* xl = tp.xs + (size_t)l * nx;
        const float* h_in = tp.hs + (size_t)l * nh;
        const float* h_mid = tp.hs + (size_t)(l + 1) * nh;
        float* const* g = grads + 6 + 36 * l;
        // x_{l+1} = x_l + gen * H2X(x_l, h_mid): identity path first, then the block's own contributions
        const int nxt = cur ^ 1;
        const float* Px = tp.P + (size_t)(2 * l) * n * PROW;
        const float* Qx = tp.Qt + (size_t)(2 * l) * n * HEADS * H;
        BlockArgs both;     // what the layer's two blocks share
        both.x = xl; both.g = graph;
        both.dx = w.gx[nxt]; both.de_w = w.de_w; both.ov = &ov;
        BlockArgs a = both;
        a.att = packed + h2x_off(l); a.h_in = h_mid; a.g_out = w.gx[cur]; a.rows = w.act;
        // dP of an h2x block is non-zero on gen | nbr(gen) only, a subset of the receptive-field list A1
        a.dp_rows = prune ? w.A1 : every;
        a.gh = gh_cur; a.dx_init = w.gx[cur]; a.grads = g + 18; a.P_saved = Px + (size_t)n * PROW; a.Qt_saved = Qx + (size_t)n * HEADS * H;
        a.qln = qln_slots ? w.qln + (size_t)(2 * l + 1) * 2 * H : nullptr;
        RC_TRY(attention_block_backward(a, w, s));
        // h_mid = h_in + X2H(x_l, h_in): gh_cur holds dL/dh_mid, which is also the residual part of dL/dh_in.  The block reads it
        // (fold, outer products, bias sums) and writes dL/dh_in = gh_cur + dP Wn^T into the OTHER buffer.
        const int k = L - 1 - l;      // 0 for the last layer
        BlockArgs c = both;
        c.x2h = true; c.att = packed + x2h_off(l); c.h_in = h_in; c.g_out = gh_cur;
        c.rows = (prune && k < 2) ? (k ? w.A2 : w.A1) : every;
        c.gh = gh_oth; c.gh_src = gh_cur; c.grads = g; c.P_saved = Px; c.Qt_saved = Qx; c.rin_ready = rin;
        c.qln = qln_slots ? w.qln + (size_t)(2 * l) * 2 * H : nullptr;
        RC_TRY(attention_block_backward(c, w, s));
        { float* t = gh_cur; gh_cur = gh_oth; gh_oth = t; }
        cur = nxt;
    }
    if (grad_h_in) HIP_TRY(hipMemcpyAsync(grad_h_in, gh_cur, nh * 4, hipMemcpyDeviceToDevice, s));
    // grad_x_in: w.gx[cur] now holds dL/dx_0 through the layer chain (the identity paths, every h2x block's rel_x and distance terms,
    // the distance terms of every x2h block); the gate adds its own distance path below.  Under every pruning mode this is exact:
    // a block skips only rows whose dL/dh (x2h) or dL/dx (h2x) is exactly zero, and every coordinate term of an edge (i, j) is a
    // product with that edge's upstream gradient, which is zero when row i is skipped -- so the skipped rows contribute exactly
    // zero to both x_i and x_j.  The same holds for the gate: dL/de_w is zero on every edge no block wrote.  (The edge-row mode
    // changes only how dL/dh is summed; its coordinate terms use the same atomics.)
    if (grad_x_in) HIP_TRY(hipMemcpyAsync(grad_x_in, w.gx[cur], nx * 4, hipMemcpyDeviceToDevice, s));
    // distance gate (computed once from the input coordinates, used by all 2L blocks): on its own slab buffers, BEFORE the auxiliary
    // stream is joined -- the last blocks' weight-gradient kernels (~150 us) run beside it instead of ahead of it
    RC_TRY(gate_backward(packed, tp.xs, tp.nbr, tp.deg, n, w, grads, s, every, grad_x_in));
    // the auxiliary stream's last weight gradients must be in place when this call's work on `s` is: join both sets
    if (ov.aux)
        for (int k = 0; k < 2; ++k)
            if (ov.used[k]) HIP_TRY(hipStreamWaitEvent(s, ov.aux->done[k], 0));
    ov.joined = true;
    return CBGX_OK;
}

// ---- a stack of H2X blocks on its own graph (DiffBP's CoMPredictor, diffbp.py:30-101): taped forward + backward -------
struct StackTape { int32_t* nbr; int32_t* deg; float* e_w; float* xs; size_t total; };
static StackTape carve_stack_tape(void* base, int n, int L) {
    StackTape t;
    Carver c(base);
    const size_t N = (size_t)(n > 0 ? n : 1);
    t.nbr = c.take<int32_t>(N * KNN * 4);
    t.deg = c.take<int32_t>(N * 4);
    t.e_w = c.take<float>(N * KNN * 4);
    t.xs = c.take<float>((size_t)(L + 1) * N * 3 * 4);
    t.total = c.off;
    return t;
}
static int carve_stack_tape_checked(const char* who, const void* tape, size_t bytes, int n, int L, StackTape& tp) {
    tp = carve_stack_tape((void*)tape, n, L);
    return bytes < tp.total ? set_error(CBGX_E_WORKSPACE, "%s: tape too small", who) : CBGX_OK;
}

size_t cbgx_h2x_stack_tape_bytes(int n_nodes, int num_layers) {
    if (n_nodes < 0 || num_layers < 1) return 0;
    return carve_stack_tape(nullptr, n_nodes, num_layers).total;
}

int cbgx_h2x_stack_forward_train(const float* packed, int num_layers, const float* x, const float* h,
                                 const int32_t* graph_ptr, const uint8_t* lig_flag, const uint8_t* gen_flag, int n_nodes,
                                 int n_graphs, float* x_out, void* tape, size_t tape_bytes, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (n_nodes <= 0 || n_graphs < 1 || num_layers < 1) return set_error(CBGX_E_INVALID, "h2x_stack_forward_train: bad sizes");
    if (!packed || !x || !h || !graph_ptr || !lig_flag || !gen_flag || !x_out || !tape || !workspace)
        return set_error(CBGX_E_INVALID, "h2x_stack_forward_train: NULL pointer");
    StackTape tp;
    RC_TRY(carve_stack_tape_checked("h2x_stack_forward_train", tape, tape_bytes, n_nodes, num_layers, tp));
    TrainWs w;
    RC_TRY(carve_train_checked("h2x_stack_forward_train", workspace, workspace_bytes, n_nodes, w));
    hipStream_t s = (hipStream_t)stream;
    const size_t nx = (size_t)n_nodes * 3;
    HIP_TRY(hipMemcpyAsync(tp.xs, x, nx * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(launch_build_active(gen_flag, n_nodes, w.act, s));
    // As cbgx_h2x_stack_forward (api.hip): an h2x block only reads the neighbour lists and gate values of the rows it moves and the
    // projections of their in-neighbours, so the kNN search, the gate MLP and the neighbour projection run on those lists (round 6;
    // the backward walks the same lists -- CBGX_TRAIN_STACK_LISTS=0 switches both back to all rows)
    const bool lists = g_edge_impl == 0 && env_on("CBGX_TRAIN_STACK_LISTS");
    RowList src;
    if (lists) {
        HIP_TRY(launch_knn_reg(x, graph_ptr, n_graphs, n_nodes, tp.nbr, tp.deg, s, w.act));
        HIP_TRY(launch_gate_mfma(packed, x, tp.nbr, tp.deg, n_nodes, tp.e_w, s, w.act));
        HIP_TRY(launch_mark_seed(gen_flag, gen_flag, n_nodes, w.mask, s));
        HIP_TRY(walk_receptive_field(w.mask, w.act, tp.nbr, tp.deg, n_nodes, {w.A1}, s));
        src = w.A1;
    } else {
        HIP_TRY(launch_knn(x, graph_ptr, n_graphs, n_nodes, tp.nbr, tp.deg, s));
        HIP_TRY(launch_gate(packed, x, tp.nbr, tp.deg, n_nodes, tp.e_w, s));
    }
    const Graph g{tp.nbr, tp.deg, tp.e_w, lig_flag, gen_flag, n_nodes};
    const NodeBufs b{w.P, w.set[0].qs, w.Qt};
    for (int l = 0; l < num_layers; ++l)
        HIP_TRY(launch_attention(false, packed + GATE_SIZE + (size_t)l * ATT_SIZE, g, tp.xs + (size_t)l * nx, h, b,
                                 tp.xs + (size_t)(l + 1) * nx, nullptr, w.act, src, s));
    HIP_TRY(hipMemcpyAsync(x_out, tp.xs + (size_t)num_layers * nx, nx * 4, hipMemcpyDeviceToDevice, s));
    return CBGX_OK;
}

int cbgx_h2x_stack_backward(const float* packed, int num_layers, const void* tape, size_t tape_bytes, const float* h,
                            const uint8_t* lig_flag, const uint8_t* gen_flag, int n_nodes, const float* grad_x_out,
                            float* const* grads, int num_grads, float* grad_h, void* workspace, size_t workspace_bytes,
                            void* stream) {
    return cbgx_h2x_stack_backward_ex(packed, num_layers, tape, tape_bytes, h, lig_flag, gen_flag, n_nodes, grad_x_out, grads,
                                      num_grads, grad_h, nullptr, workspace, workspace_bytes, stream);
}

int cbgx_h2x_stack_backward_ex(const float* packed, int num_layers, const void* tape, size_t tape_bytes, const float* h,
                               const uint8_t* lig_flag, const uint8_t* gen_flag, int n_nodes, const float* grad_x_out,
                               float* const* grads, int num_grads, float* grad_h, float* grad_x_in, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (n_nodes <= 0 || num_layers < 1) return set_error(CBGX_E_INVALID, "h2x_stack_backward: bad sizes");
    if (!packed || !tape || !h || !lig_flag || !gen_flag || !grad_x_out || !grad_h || !workspace)
        return set_error(CBGX_E_INVALID, "h2x_stack_backward: NULL pointer");
    if (num_grads != 6 + 18 * num_layers)
        return set_error(CBGX_E_INVALID, "h2x_stack_backward: expected %d gradient tensors, got %d", 6 + 18 * num_layers, num_grads);
    RC_TRY(check_grads(grads, num_grads, "h2x_stack_backward"));
    StackTape tp;
    RC_TRY(carve_stack_tape_checked("h2x_stack_backward", tape, tape_bytes, n_nodes, num_layers, tp));
    TrainWs w;
    RC_TRY(carve_train_checked("h2x_stack_backward", workspace, workspace_bytes, n_nodes, w));
    hipStream_t s = (hipStream_t)stream;
    const int n = n_nodes;
    const size_t nx = (size_t)n * 3, nh = (size_t)n * H;
    HIP_TRY(hipMemsetAsync(w.gh, 0, nh * 4, s));
    int cur = 0;
    HIP_TRY(hipMemcpyAsync(w.gx[cur], grad_x_out, nx * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(w.de_w, 0, (size_t)n * KNN * 4, s));
    HIP_TRY(launch_build_active(gen_flag, n, w.act, s));
    // Round 6, as the denoiser's layer loop: the projection gradient of an h2x block is non-zero on gen | nbr(gen) only (this stack's
    // own graph), so its fill and every dense product over it walk that list; the weight-gradient kernels of a block run on the caller's
    // auxiliary stream on alternating buffer sets, one query-LayerNorm accumulator slot per block (CBGX_TRAIN_OVERLAP=0: one stream)
    const bool lists = g_edge_impl != 1 && env_on("CBGX_TRAIN_STACK_LISTS");
    if (lists) {
        HIP_TRY(launch_mark_seed(gen_flag, gen_flag, n, w.mask, s));
        HIP_TRY(walk_receptive_field(w.mask, w.act, tp.nbr, tp.deg, n, {w.A1}, s));
    }
    const Graph g{tp.nbr, tp.deg, tp.e_w, lig_flag, gen_flag, n};
    const bool qln_slots = num_layers <= QLN_SLOTS;
    if (qln_slots) HIP_TRY(hipMemsetAsync(w.qln, 0, (size_t)num_layers * 2 * H * sizeof(float), s));
    BlockOverlap ov{(lists && env_on("CBGX_TRAIN_OVERLAP") && !profile_is_on() && qln_slots) ? aux_for(s) : nullptr, 0, {false, false}};
    for (int l = num_layers - 1; l >= 0; --l) {
        const int nxt = cur ^ 1;
        // x_out = x + gen * delta: the identity part of the coordinate gradient is the block's `dx_init`
        BlockArgs a;
        a.att = packed + GATE_SIZE + (size_t)l * ATT_SIZE; a.x = tp.xs + (size_t)l * nx; a.h_in = h; a.g_out = w.gx[cur];
        a.g = g;
        a.rows = w.act; a.dp_rows = lists ? RowList(w.A1) : RowList();
        a.gh = w.gh; a.dx = w.gx[nxt]; a.dx_init = w.gx[cur]; a.de_w = w.de_w; a.grads = grads + 6 + 18 * l;
        a.qln = qln_slots ? w.qln + (size_t)l * 2 * H : nullptr; a.ov = &ov;
        RC_TRY(attention_block_backward(a, w, s));
        cur = nxt;
    }
    HIP_TRY(hipMemcpyAsync(grad_h, w.gh, nh * 4, hipMemcpyDeviceToDevice, s));
    // grad_x_in: the chain's dL/dx_0 (identity paths + the blocks' coordinate terms; the listed products skip only rows whose terms are
    // exactly zero, as in the denoiser's backward), then the gate's distance path, which lives on the movable rows' edges only
    if (grad_x_in) HIP_TRY(hipMemcpyAsync(grad_x_in, w.gx[cur], nx * 4, hipMemcpyDeviceToDevice, s));
    // (the stack's blocks add to de_w on the movable rows only: the gate backward walks that list -- 16.5 k rows -> ~900)
    RC_TRY(gate_backward(packed, tp.xs, tp.nbr, tp.deg, n, w, grads, s, lists ? RowList(w.act) : RowList(), grad_x_in));
    if (ov.aux)
        for (int k = 0; k < 2; ++k)
            if (ov.used[k]) HIP_TRY(hipStreamWaitEvent(s, ov.aux->done[k], 0));
    ov.joined = true;
    return CBGX_OK;
}

// ---- TargetDiff's training arithmetic around the denoiser (train_loss.hip) ---------------------------------------------------------
constexpr int LOSS_MAX_GRAPHS = 4096;     // per-graph sums of the loss kernel live in LDS (3 floats per graph)

int cbgx_targetdiff_train_noise(const float* x0, const int64_t* v0, const int64_t* t, const int64_t* batch, const uint8_t* gen,
                                int n_lig, int num_classes, const float* alphas_cumprod, const float* log_alphas_cumprod,
                                const float* log_one_minus_alphas_cumprod, const float* eps, const float* u, float* x_t,
                                float* c_t, int64_t* v_t, void* stream) {
    if (n_lig == 0) return CBGX_OK;
    if (n_lig < 0 || num_classes < 1 || num_classes > 32)
        return set_error(CBGX_E_INVALID, "train_noise: bad sizes (n_lig=%d C=%d)", n_lig, num_classes);
    if (!x0 || !v0 || !t || !batch || !gen || !alphas_cumprod || !log_alphas_cumprod || !log_one_minus_alphas_cumprod || !eps ||
        !u || !x_t || !c_t || !v_t)
        return set_error(CBGX_E_INVALID, "train_noise: NULL pointer");
    HIP_TRY(launch_train_noise(x0, v0, t, batch, gen, n_lig, num_classes, alphas_cumprod, log_alphas_cumprod,
                               log_one_minus_alphas_cumprod, (float)log((double)num_classes), eps, u, x_t, c_t, v_t,
                               (hipStream_t)stream));
    return CBGX_OK;
}

// ---- counter-mode draws of a training / validation call (train_noise.hip, rng.h) -----------------------------------------------------
static bool bad_purpose_base(int purpose_base) { return purpose_base < 0 || purpose_base % CBGX_NOISE_PURPOSE_STRIDE != 0; }

int cbgx_train_noise_draw(const uint64_t* stream_keys, const int32_t* lig_ptr, int n_graphs, int n_lig, int purpose_base, int n_t,
                          const int64_t* t_in, int64_t* t_out, float* a, float* b, int cols_b, int purpose_b, int uniform_b,
                          void* stream) {
    if (n_graphs < 0 || n_lig < 0 || n_t < 1 || bad_purpose_base(purpose_base) ||
        (b && (cols_b < 1 || cols_b > 32 || purpose_b < 0 || purpose_b >= CBGX_NOISE_PURPOSE_STRIDE)))
        return set_error(CBGX_E_INVALID, "train_noise_draw: bad sizes (n_lig=%d B=%d n_t=%d purpose_base=%d cols_b=%d purpose_b=%d)",
                         n_lig, n_graphs, n_t, purpose_base, cols_b, purpose_b);
    if (n_graphs == 0) return CBGX_OK;
    if (!stream_keys || !lig_ptr || !t_out) return set_error(CBGX_E_INVALID, "train_noise_draw: NULL pointer");
    HIP_TRY(launch_train_noise_draw(stream_keys, lig_ptr, n_graphs, n_lig, (uint32_t)purpose_base, (uint32_t)n_t, t_in, t_out, a, b,
                                    cols_b, (uint32_t)purpose_b, uniform_b, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_targetdiff_train_noise_rng(const float* x0, const int64_t* v0, const int64_t* batch, const uint8_t* gen, int n_lig,
                                    int num_classes, const float* alphas_cumprod, const float* log_alphas_cumprod,
                                    const float* log_one_minus_alphas_cumprod, const uint64_t* stream_keys, const int32_t* lig_ptr,
                                    int n_graphs, int purpose_base, int n_t, const int64_t* t_in, int64_t* t_out, float* x_t,
                                    float* c_t, int64_t* v_t, void* stream) {
    if (n_lig < 0 || n_graphs < 0 || num_classes < 1 || num_classes > 32 || n_t < 1 || bad_purpose_base(purpose_base))
        return set_error(CBGX_E_INVALID, "train_noise_rng: bad sizes (n_lig=%d B=%d C=%d n_t=%d purpose_base=%d)", n_lig, n_graphs,
                         num_classes, n_t, purpose_base);
    if (n_graphs == 0) return CBGX_OK;     // (no graph: no atom either)
    if (!stream_keys || !lig_ptr || !t_out ||
        (n_lig > 0 && (!x0 || !v0 || !batch || !gen || !alphas_cumprod || !log_alphas_cumprod || !log_one_minus_alphas_cumprod ||
                       !x_t || !c_t || !v_t)))
        return set_error(CBGX_E_INVALID, "train_noise_rng: NULL pointer");
    HIP_TRY(launch_train_noise_rng(x0, v0, batch, gen, n_lig, n_graphs, num_classes, alphas_cumprod, log_alphas_cumprod,
                                   log_one_minus_alphas_cumprod, (float)log((double)num_classes), stream_keys, lig_ptr,
                                   (uint32_t)purpose_base, (uint32_t)n_t, t_in, t_out, x_t, c_t, v_t, (hipStream_t)stream));
    return CBGX_OK;
}

// ---- per-visit transforms of a training batch: protein noise + centring (train_transform.hip) ------------------------------------------
static int tt_check(const char* what, const float* x_rec, const float* x_lig, const int32_t* rec_ptr, const int32_t* lig_ptr,
                    int n_graphs, int n_rec, int n_lig, float sigma, int center_mode, const float* x_rec_out, const float* x_lig_out,
                    const float* center_out) {
    if (n_graphs < 0 || n_rec < 0 || n_lig < 0 || !(sigma >= 0.f) ||
        center_mode < CBGX_CENTER_PROTEIN || center_mode > CBGX_CENTER_WHOLE)
        return set_error(CBGX_E_INVALID, "%s: bad arguments (B=%d n_rec=%d n_lig=%d sigma=%g center_mode=%d)", what, n_graphs, n_rec,
                         n_lig, (double)sigma, center_mode);
    if ((n_graphs > 0 && (!rec_ptr || !lig_ptr || !center_out)) || (n_rec > 0 && (!x_rec || !x_rec_out)) ||
        (n_lig > 0 && (!x_lig || !x_lig_out)))
        return set_error(CBGX_E_INVALID, "%s: NULL pointer", what);
    return CBGX_OK;
}

int cbgx_train_transform(const float* x_rec, const float* x_lig, const int32_t* rec_ptr, const int32_t* lig_ptr, const uint8_t* ctx,
                         int n_graphs, int n_rec, int n_lig, float sigma, int center_mode, const float* eps, float* x_rec_out,
                         float* x_lig_out, float* center_out, void* stream) {
    const int rc = tt_check("train_transform", x_rec, x_lig, rec_ptr, lig_ptr, n_graphs, n_rec, n_lig, sigma, center_mode, x_rec_out,
                            x_lig_out, center_out);
    if (rc != CBGX_OK) return rc;
    if (!eps && sigma > 0.f) return set_error(CBGX_E_INVALID, "train_transform: eps == NULL needs sigma == 0 (got %g)", (double)sigma);
    HIP_TRY(launch_train_transform(x_rec, x_lig, rec_ptr, lig_ptr, ctx, n_graphs, n_rec, n_lig, sigma, center_mode, eps, nullptr, 0u,
                                   x_rec_out, x_lig_out, center_out, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_train_transform_rng(const float* x_rec, const float* x_lig, const int32_t* rec_ptr, const int32_t* lig_ptr,
                             const uint8_t* ctx, int n_graphs, int n_rec, int n_lig, float sigma, int center_mode,
                             const uint64_t* stream_keys, int purpose_base, float* x_rec_out, float* x_lig_out, float* center_out,
                             void* stream) {
    const int rc = tt_check("train_transform_rng", x_rec, x_lig, rec_ptr, lig_ptr, n_graphs, n_rec, n_lig, sigma, center_mode,
                            x_rec_out, x_lig_out, center_out);
    if (rc != CBGX_OK) return rc;
    if (purpose_base < 0 || purpose_base % CBGX_NOISE_PURPOSE_STRIDE != 0)
        return set_error(CBGX_E_INVALID, "train_transform_rng: purpose_base=%d is not a non-negative multiple of %d", purpose_base,
                         CBGX_NOISE_PURPOSE_STRIDE);
    if (n_graphs > 0 && !stream_keys) return set_error(CBGX_E_INVALID, "train_transform_rng: NULL pointer");
    HIP_TRY(launch_train_transform(x_rec, x_lig, rec_ptr, lig_ptr, ctx, n_graphs, n_rec, n_lig, sigma, center_mode, nullptr,
                                   stream_keys, (uint32_t)purpose_base + (uint32_t)CBGX_NOISE_TRAIN_PROTEIN_NORMAL, x_rec_out, x_lig_out,
                                   center_out, (hipStream_t)stream));
    return CBGX_OK;
}

// the same behind the decomposition choice of every graph (choose_ctx_gen): what the three CSRs and the two further outputs must satisfy
static int tt_choose_check(const char* what, const int32_t* dec_ptr, const int32_t* gen_ptr, const int32_t* gen_idx, int n_graphs,
                           int n_lig, int n_dec, int n_idx, const uint8_t* gen_flag_out, const int32_t* choice_out) {
    if (n_dec < 0 || n_idx < 0) return set_error(CBGX_E_INVALID, "%s: bad arguments (n_dec=%d n_idx=%d)", what, n_dec, n_idx);
    if ((n_graphs > 0 && (!dec_ptr || !choice_out)) || (n_dec > 0 && !gen_ptr) || (n_idx > 0 && !gen_idx) || (n_lig > 0 && !gen_flag_out))
        return set_error(CBGX_E_INVALID, "%s: NULL pointer", what);
    return CBGX_OK;
}

int cbgx_train_transform_choose(const float* x_rec, const float* x_lig, const int32_t* rec_ptr, const int32_t* lig_ptr,
                                const int32_t* dec_ptr, const int32_t* gen_ptr, const int32_t* gen_idx, const int32_t* choice_in,
                                int n_graphs, int n_rec, int n_lig, int n_dec, int n_idx, float sigma, int center_mode, const float* eps,
                                float* x_rec_out, float* x_lig_out, float* center_out, uint8_t* gen_flag_out, int32_t* choice_out,
                                void* stream) {
    int rc = tt_check("train_transform_choose", x_rec, x_lig, rec_ptr, lig_ptr, n_graphs, n_rec, n_lig, sigma, center_mode, x_rec_out,
                      x_lig_out, center_out);
    if (rc != CBGX_OK) return rc;
    rc = tt_choose_check("train_transform_choose", dec_ptr, gen_ptr, gen_idx, n_graphs, n_lig, n_dec, n_idx, gen_flag_out, choice_out);
    if (rc != CBGX_OK) return rc;
    if (!eps && sigma > 0.f)
        return set_error(CBGX_E_INVALID, "train_transform_choose: eps == NULL needs sigma == 0 (got %g)", (double)sigma);
    HIP_TRY(launch_train_transform_choose(x_rec, x_lig, rec_ptr, lig_ptr, dec_ptr, gen_ptr, gen_idx, choice_in, n_graphs, n_rec, n_lig,
                                          n_dec, n_idx, sigma, center_mode, eps, nullptr, 0u, x_rec_out, x_lig_out, center_out,
                                          gen_flag_out, choice_out, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_train_transform_choose_rng(const float* x_rec, const float* x_lig, const int32_t* rec_ptr, const int32_t* lig_ptr,
                                    const int32_t* dec_ptr, const int32_t* gen_ptr, const int32_t* gen_idx, int n_graphs, int n_rec,
                                    int n_lig, int n_dec, int n_idx, float sigma, int center_mode, const uint64_t* stream_keys,
                                    int purpose_base, float* x_rec_out, float* x_lig_out, float* center_out, uint8_t* gen_flag_out,
                                    int32_t* choice_out, void* stream) {
    int rc = tt_check("train_transform_choose_rng", x_rec, x_lig, rec_ptr, lig_ptr, n_graphs, n_rec, n_lig, sigma, center_mode,
                      x_rec_out, x_lig_out, center_out);
    if (rc != CBGX_OK) return rc;
    rc = tt_choose_check("train_transform_choose_rng", dec_ptr, gen_ptr, gen_idx, n_graphs, n_lig, n_dec, n_idx, gen_flag_out,
                         choice_out);
    if (rc != CBGX_OK) return rc;
    if (purpose_base < 0 || purpose_base % CBGX_NOISE_PURPOSE_STRIDE != 0)
        return set_error(CBGX_E_INVALID, "train_transform_choose_rng: purpose_base=%d is not a non-negative multiple of %d", purpose_base,
                         CBGX_NOISE_PURPOSE_STRIDE);
    if (n_graphs > 0 && !stream_keys) return set_error(CBGX_E_INVALID, "train_transform_choose_rng: NULL pointer");
    HIP_TRY(launch_train_transform_choose(x_rec, x_lig, rec_ptr, lig_ptr, dec_ptr, gen_ptr, gen_idx, nullptr, n_graphs, n_rec, n_lig,
                                          n_dec, n_idx, sigma, center_mode, nullptr, stream_keys, (uint32_t)purpose_base, x_rec_out,
                                          x_lig_out, center_out, gen_flag_out, choice_out, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_targetdiff_loss(const float* x_out, const float* logits, const int64_t* lig_rows, const float* x0, const int64_t* v0,
                         const int64_t* v_t, const int64_t* t, const int64_t* batch, const uint8_t* gen, int n_lig, int n_graphs,
                         int num_classes, const float* const* tables, float* losses, float* x_pred, float* c_pred,
                         float* grad_pos, float* grad_logit, void* stream) {
    if (n_lig <= 0 || n_graphs <= 0 || n_graphs > LOSS_MAX_GRAPHS || num_classes < 1 || num_classes > 32)
        return set_error(CBGX_E_INVALID, "targetdiff_loss: bad sizes (n_lig=%d B=%d (max %d) C=%d)", n_lig, n_graphs,
                         LOSS_MAX_GRAPHS, num_classes);
    if (!x_out || !logits || !lig_rows || !x0 || !v0 || !v_t || !t || !batch || !gen || !tables || !losses || !grad_pos ||
        !grad_logit)
        return set_error(CBGX_E_INVALID, "targetdiff_loss: NULL pointer");
    for (int i = 0; i < 4; ++i)
        if (!tables[i]) return set_error(CBGX_E_INVALID, "targetdiff_loss: table %d is NULL", i);
    HIP_TRY(launch_train_loss(x_out, logits, lig_rows, x0, v0, v_t, t, batch, gen, n_lig, n_graphs, num_classes, tables,
                              (float)log((double)num_classes), losses, x_pred, c_pred, grad_pos, grad_logit,
                              (hipStream_t)stream));
    return CBGX_OK;
}

static int diffbp_loss_entry(const float* x_out, const float* x_in, const float* x_stack, const float* logits, const int64_t* sort_idx,
                             const int32_t* graph_ptr, const uint8_t* lig_flag, const float* pos_noise, const float* com_noise,
                             const int64_t* v0, const uint8_t* type_flag, const uint8_t* gen, const int64_t* t, int n_protein, int n_lig,
                             int n_graphs, int num_classes, const float* alphas_cumprod, const float* betas, float rho, float gamma,
                             float* losses, float* scal, float* gstats, float* a_pos, float* a_int, float* b_com, float* b_int,
                             float* z_atom, int32_t* bad, float* knn_scratch, void* stream) {
    if (n_lig <= 0 || n_graphs <= 0 || n_protein < 0 || num_classes < 1 || num_classes > 32)
        return set_error(CBGX_E_INVALID, "diffbp_loss: bad sizes (n_lig=%d B=%d C=%d)", n_lig, n_graphs, num_classes);
    if (!x_out || !x_in || !x_stack || !logits || !sort_idx || !graph_ptr || !lig_flag || !pos_noise || !com_noise || !v0 || !type_flag ||
        !gen || !t || !alphas_cumprod || !betas || !losses || !scal || !gstats || !a_pos || !a_int || !b_com || !b_int || !z_atom || !bad)
        return set_error(CBGX_E_INVALID, "diffbp_loss: NULL pointer");
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int32_t), (hipStream_t)stream));
    HIP_TRY(launch_diffbp_loss(x_out, x_in, x_stack, logits, sort_idx, graph_ptr, lig_flag, pos_noise, com_noise, v0, type_flag, gen, t,
                               n_protein, n_lig, n_graphs, num_classes, alphas_cumprod, betas, rho, gamma, gstats, losses, scal, a_pos,
                               a_int, b_com, b_int, z_atom, bad, knn_scratch, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_diffbp_loss(const float* x_out, const float* x_in, const float* x_stack, const float* logits, const int64_t* sort_idx,
                     const int32_t* graph_ptr, const uint8_t* lig_flag, const float* pos_noise, const float* com_noise,
                     const int64_t* v0, const uint8_t* type_flag, const uint8_t* gen, const int64_t* t, int n_protein, int n_lig,
                     int n_graphs, int num_classes, const float* alphas_cumprod, const float* betas, float rho, float gamma,
                     float* losses, float* scal, float* gstats, float* a_pos, float* a_int, float* b_com, float* b_int, float* z_atom,
                     int32_t* bad, void* stream) {
    return diffbp_loss_entry(x_out, x_in, x_stack, logits, sort_idx, graph_ptr, lig_flag, pos_noise, com_noise, v0, type_flag, gen, t,
                             n_protein, n_lig, n_graphs, num_classes, alphas_cumprod, betas, rho, gamma, losses, scal, gstats, a_pos,
                             a_int, b_com, b_int, z_atom, bad, nullptr, stream);
}

int cbgx_diffbp_loss_knn(const float* x_out, const float* x_in, const float* x_stack, const float* logits, const int64_t* sort_idx,
                         const int32_t* graph_ptr, const uint8_t* lig_flag, const float* pos_noise, const float* com_noise,
                         const int64_t* v0, const uint8_t* type_flag, const uint8_t* gen, const int64_t* t, int n_protein, int n_lig,
                         int n_graphs, int num_classes, const float* alphas_cumprod, const float* betas, float rho, float gamma,
                         float* losses, float* scal, float* gstats, float* a_pos, float* a_int, float* b_com, float* b_int,
                         float* z_atom, int32_t* bad, float* knn_scratch, void* stream) {
    if (!knn_scratch) return set_error(CBGX_E_INVALID, "diffbp_loss_knn: NULL scratch");
    return diffbp_loss_entry(x_out, x_in, x_stack, logits, sort_idx, graph_ptr, lig_flag, pos_noise, com_noise, v0, type_flag, gen, t,
                             n_protein, n_lig, n_graphs, num_classes, alphas_cumprod, betas, rho, gamma, losses, scal, gstats, a_pos,
                             a_int, b_com, b_int, z_atom, bad, knn_scratch, stream);
}

int cbgx_diffbp_train_noise(const float* x0, const int64_t* v0, const int64_t* t, const uint8_t* gen, const float* eps, const float* u,
                            const int64_t* sort_idx, const int32_t* graph_ptr, int n_protein, int n_lig, int n_graphs, int num_classes,
                            const float* alphas_cumprod, int num_timesteps, int absorbing_state, float* x_t, float* pos_noise,
                            float* com_noise, int64_t* v_t, float* c_t, uint8_t* type_flag, void* stream) {
    if (n_lig == 0) return CBGX_OK;
    if (n_lig < 0 || n_graphs <= 0 || n_protein < 0 || num_classes < 1 || num_timesteps < 1 || absorbing_state < 0 ||
        absorbing_state >= num_classes)
        return set_error(CBGX_E_INVALID, "diffbp_train_noise: bad sizes (n_lig=%d B=%d C=%d T=%d absorbing=%d)", n_lig, n_graphs,
                         num_classes, num_timesteps, absorbing_state);
    if (!x0 || !v0 || !t || !gen || !eps || !u || !sort_idx || !graph_ptr || !alphas_cumprod || !x_t || !pos_noise || !com_noise ||
        !v_t || !c_t || !type_flag)
        return set_error(CBGX_E_INVALID, "diffbp_train_noise: NULL pointer");
    HIP_TRY(launch_diffbp_noise(x0, v0, t, gen, eps, u, sort_idx, graph_ptr, n_protein, n_graphs, num_classes, alphas_cumprod,
                                num_timesteps, absorbing_state, x_t, pos_noise, com_noise, v_t, c_t, type_flag, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_diffsbdd_train_noise(const float* x0, const float* x_protein, const int64_t* v0, const float* eps_x, const float* eps_c,
                              const uint8_t* gen, const int64_t* t, const int64_t* sort_idx, const int32_t* graph_ptr, int n_protein,
                              int n_lig, int n_graphs, int num_classes, const float* alpha_table, const float* sigma_table,
                              int num_timesteps, float* x_t, float* x_protein_t, float* c_t, float* gdata, void* stream) {
    if (n_lig <= 0 || n_graphs <= 0 || n_protein < 0 || num_classes < 1 || num_classes > 32 || num_timesteps < 1)
        return set_error(CBGX_E_INVALID, "diffsbdd_train_noise: bad sizes (n_lig=%d B=%d C=%d T=%d)", n_lig, n_graphs, num_classes,
                         num_timesteps);
    if (!x0 || (n_protein && (!x_protein || !x_protein_t)) || !v0 || !eps_x || !eps_c || !gen || !t || !sort_idx || !graph_ptr ||
        !alpha_table || !sigma_table || !x_t || !c_t || !gdata)
        return set_error(CBGX_E_INVALID, "diffsbdd_train_noise: NULL pointer");
    HIP_TRY(launch_diffsbdd_noise(x0, x_protein, v0, eps_x, eps_c, gen, t, sort_idx, graph_ptr, n_protein, n_graphs, num_classes,
                                  alpha_table, sigma_table, num_timesteps, x_t, x_protein_t, c_t, gdata, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_diffsbdd_loss(const float* x_out, const float* logits, const float* eps_x, const float* eps_c, const int64_t* t,
                       const int64_t* sort_idx, const int32_t* graph_ptr, int n_protein, int n_lig, int n_graphs, int num_classes,
                       const float* gdata, float* glosses, float* losses, float* x_pred, float* c_pred, float* grad_pos,
                       float* grad_logit, void* stream) {
    if (n_lig <= 0 || n_graphs <= 0 || n_protein < 0 || num_classes < 1 || num_classes > 32)
        return set_error(CBGX_E_INVALID, "diffsbdd_loss: bad sizes (n_lig=%d B=%d C=%d)", n_lig, n_graphs, num_classes);
    if (!x_out || !logits || !eps_x || !eps_c || !t || !sort_idx || !graph_ptr || !gdata || !glosses || !losses || !x_pred || !c_pred ||
        !grad_pos || !grad_logit)
        return set_error(CBGX_E_INVALID, "diffsbdd_loss: NULL pointer");
    HIP_TRY(launch_diffsbdd_loss(x_out, logits, eps_x, eps_c, t, sort_idx, graph_ptr, n_protein, n_graphs, num_classes, gdata, glosses,
                                 losses, x_pred, c_pred, grad_pos, grad_logit, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_compose_plan(const int64_t* batch_protein, const int64_t* batch_ligand, int n_protein, int n_ligand, int n_graphs,
                      int32_t* scratch, int64_t* sort_idx, int64_t* batch_idx, uint8_t* lig_flag, int64_t* lig_rows, int32_t* graph_ptr,
                      void* stream) {
    if (n_protein < 0 || n_ligand < 0 || n_graphs < 1 || n_graphs > (1 << 20))
        return set_error(CBGX_E_INVALID, "compose_plan: bad sizes (N_protein=%d N_ligand=%d B=%d)", n_protein, n_ligand, n_graphs);
    if (!scratch || !graph_ptr || (n_protein && !batch_protein) || (n_ligand && (!batch_ligand || !lig_rows)) ||
        ((n_protein + n_ligand) && (!sort_idx || !batch_idx || !lig_flag)))
        return set_error(CBGX_E_INVALID, "compose_plan: NULL pointer");
    HIP_TRY(launch_compose_plan(batch_protein, batch_ligand, n_protein, n_ligand, n_graphs, scratch, sort_idx, batch_idx, lig_flag,
                                lig_rows, graph_ptr, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_embed_compose(const float* x_protein, const float* x_ligand, const float* protein_feat, const int64_t* protein_aa,
                       const float* ligand_feat, const int64_t* sort_idx, const uint8_t* gen_protein, const uint8_t* gen_ligand,
                       int n_protein, int n_ligand, int feat_dim, int num_aa, int lig_dim, const float* const* params, float* x, float* h,
                       float* ext, uint8_t* gen_flag, void* stream) {
    if (n_protein < 0 || n_ligand < 0 || feat_dim < 1 || num_aa < 1 || lig_dim < 1 || feat_dim + num_aa + lig_dim + 2 > EMB_MAX_J)
        return set_error(CBGX_E_INVALID, "embed_compose: bad sizes (N_protein=%d N_ligand=%d F=%d A=%d C=%d; F + A + C + 2 <= %d)",
                         n_protein, n_ligand, feat_dim, num_aa, lig_dim, EMB_MAX_J);
    if (n_protein + n_ligand == 0) return CBGX_OK;
    if (!params || !sort_idx || !x || !h || !ext || (n_protein && (!x_protein || !protein_feat || !protein_aa)) ||
        (n_ligand && (!x_ligand || !ligand_feat)) || (gen_flag && n_ligand && !gen_ligand))
        return set_error(CBGX_E_INVALID, "embed_compose: NULL pointer");
    for (int i = 0; i < 8; ++i)
        if (!params[i]) return set_error(CBGX_E_INVALID, "embed_compose: parameter %d is NULL", i);
    const EmbedParams p{params[0], params[1], params[2], params[3], params[4], params[5], params[6], params[7]};
    HIP_TRY(launch_embed_compose(x_protein, x_ligand, protein_feat, protein_aa, ligand_feat, sort_idx, gen_protein, gen_ligand, n_protein,
                                 n_ligand, feat_dim, num_aa, lig_dim, p, x, h, ext, gen_flag, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_embed_compose_backward(const float* grad_h, const float* ext, int n_nodes, int feat_dim, int num_aa, int lig_dim, float* partial,
                                int groups, float* grad_out, void* stream) {
    if (n_nodes < 0 || feat_dim < 1 || num_aa < 1 || lig_dim < 1 || feat_dim + num_aa + lig_dim + 2 > EMB_MAX_J || groups < 1 ||
        groups > 256)
        return set_error(CBGX_E_INVALID, "embed_compose_backward: bad sizes (N=%d F=%d A=%d C=%d groups=%d)", n_nodes, feat_dim, num_aa,
                         lig_dim, groups);
    if (!grad_out || (n_nodes && (!grad_h || !ext || !partial))) return set_error(CBGX_E_INVALID, "embed_compose_backward: NULL pointer");
    if (n_nodes == 0) {
        HIP_TRY(hipMemsetAsync(grad_out, 0, sizeof(float) * H * (feat_dim + num_aa + lig_dim + 2), (hipStream_t)stream));
        return CBGX_OK;
    }
    HIP_TRY(launch_embed_compose_backward(grad_h, ext, n_nodes, feat_dim, num_aa, lig_dim, partial, groups, grad_out,
                                          (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_targetdiff_loss_backward(const float* grad_pos, const float* grad_logit, const int64_t* sort_idx, int n_protein,
                                  int n_nodes, int num_classes, const float* g_loss_pos, const float* g_loss_atom,
                                  float* grad_x_out, float* grad_logits, void* stream) {
    if (n_nodes == 0) return CBGX_OK;
    if (n_nodes < 0 || n_protein < 0 || n_protein > n_nodes || num_classes < 1 || num_classes > 32)
        return set_error(CBGX_E_INVALID, "targetdiff_loss_backward: bad sizes (N=%d N_protein=%d C=%d)", n_nodes, n_protein,
                         num_classes);
    if (!grad_pos || !grad_logit || !sort_idx || !grad_x_out || !grad_logits)
        return set_error(CBGX_E_INVALID, "targetdiff_loss_backward: NULL pointer");
    HIP_TRY(launch_train_loss_bwd(grad_pos, grad_logit, sort_idx, n_protein, n_nodes, num_classes, g_loss_pos, g_loss_atom,
                                  grad_x_out, grad_logits, (hipStream_t)stream));
    return CBGX_OK;
}

#ifdef CBGX_XCHECK
// test-only library (include/cbgx_xcheck.h): the gate backward as a stage of its own -- the static gate_backward above, the kernels
// and reductions the training steps run, on a caller-supplied dL/de_w
int cbgx_debug_gate_backward(const float* packed, const float* x, const int32_t* nbr, const int32_t* deg, int n_nodes,
                             const float* de_w, const int* rows, const int* n_rows, float* const* grads, float* grad_x,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (n_nodes <= 0) return set_error(CBGX_E_INVALID, "debug_gate_backward: bad sizes");
    if (!packed || !x || !nbr || !deg || !de_w || !workspace || (rows != nullptr) != (n_rows != nullptr))
        return set_error(CBGX_E_INVALID, "debug_gate_backward: NULL pointer");
    RC_TRY(check_grads(grads, 6, "debug_gate_backward"));
    TrainWs w;
    RC_TRY(carve_train_checked("debug_gate_backward", workspace, workspace_bytes, n_nodes, w));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(w.de_w, de_w, (size_t)n_nodes * KNN * 4, hipMemcpyDeviceToDevice, s));
    return gate_backward(packed, x, nbr, deg, n_nodes, w, grads, s, RowList{rows, n_rows}, grad_x);
}
#endif

}  // extern "C"

// libcbgx C ABI (include/cbgx.h): argument checking, workspace carving, kernel sequencing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>

#include "../../include/cbgx.h"
#ifdef CBGX_XCHECK
#include "../../include/cbgx_xcheck.h"
#endif
#include "kernels.h"
#include "layout.h"
#include "workspace.h"

using namespace cbgx;

static thread_local char g_err[512] = "";

namespace cbgx {
// the thread-local message of cbgx_last_error, also for the entry points that live in other translation units (api_train.hip)
int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace cbgx
static constexpr auto& fail = cbgx::set_error;

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return fail(CBGX_E_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

struct Workspace {
    int32_t *nbr, *deg;
    float* e_w;
    // three node-stage buffer sets: the x2h blocks alternate between 0 and 1 (the node stage of layer l + 1 runs before layer l is
    // over: next to its h2x block on an auxiliary stream, or in one launch with that block's node stage), the h2x blocks use 2
    NodeBufs set[3];
    // The sixteen node lists of a forward call, in the order of stages.FORWARD_LISTS / include/cbgx_xcheck.h:
    NodeList act;                 // gen_flag nodes (h2x work list)
    NodeList A1, A2, A3;          // receptive-field pruning
    NodeList D1, S1, D2, S2;      // static-context cache: D_k differs from the ligand-free pocket in layer k - 1, S_k = D_k | nbr(D_k)
    // x2h layers run as ONE launch over two work lists (edge_mfma.hip, edge_x2h_dual_kernel): destinations with a ligand atom among
    // themselves and their neighbours (d1flag; general role, folded query from Qt) and protein-only ones (query folded in registers).
    // The (general, protein-only) split of: all nodes | the cached layer 1 (D2) | the pruned layers (A1, A2)
    NodeList all_gen, all_pp, D2_gen, D2_pp, A1_gen, A1_pp, A2_gen, A2_pp;
    NodeList empty;               // always empty: a count nothing writes after the call's fill
    int* step_count[2];           // counts of the step cache's two lists (their rows live in the cache block: StepCache)
    // per-node flags behind the lists (node_mfma.hip, list_level_kernel), zeroed with the counts by ONE fill per forward call:
    // receptive-field sets a1 a2 a3; "differs from the ligand-free pocket" D1 (proximity flags of the graph cache) D2 S1 S2; d1flag
    uint8_t *fa1, *fa2, *fa3, *fD1, *fD2, *fS1, *fS2;
    uint8_t* d1flag;     // the node or one of its neighbours is a ligand atom: general role of the x2h edge stage
    float *hbuf[2], *xbuf[2];
    unsigned* newmask;   // graph-cached calls: per listed centre, the ranks of its merged neighbour list that hold new entries
    void* counters;      // the flags and every list count are carved from ONE block: one fill per call
    size_t counters_bytes, total;
};

// The only place that knows where a list's count lives (nothing else adds a literal to a count pointer).
static Workspace carve(void* base, int n) {
    Workspace w;
    Carver c(base);
    size_t N = (size_t)(n > 0 ? n : 1);
    w.nbr = c.take<int32_t>(N * KNN * 4);
    w.deg = c.take<int32_t>(N * 4);
    w.e_w = c.take<float>(N * KNN * 4);
    for (NodeBufs& b : w.set) {
        b.P = c.take<float>(N * PROW * 4);
        b.Qt = c.take<float>(N * HEADS * H * 4);
        b.q = c.take<float>(N * H * 4);
    }
    for (NodeList* l : {&w.act, &w.A1, &w.A2, &w.A3, &w.D1, &w.S1, &w.D2, &w.S2}) l->rows = c.take<int>(N * 4);
    for (float*& h : w.hbuf) h = c.take<float>(N * H * 4);
    for (float*& x : w.xbuf) x = c.take<float>(N * 3 * 4);
    for (NodeList* l : {&w.all_gen, &w.all_pp, &w.D2_gen, &w.D2_pp, &w.A1_gen, &w.A1_pp, &w.A2_gen, &w.A2_pp})
        l->rows = c.take<int>(N * 4);
    w.empty.rows = w.all_pp.rows;      // (never read: its count is zero)
    w.newmask = c.take<unsigned>(N * 4);
    // eight flag arrays, then every list count of a forward call, 64 bytes apart (a counter word is hammered by returning
    // atomics): 256 bytes for act, 256 for A1 - A3, 256 for D1 - S2, 128 per (general, protein-only) pair, 256 for the empty list
    const size_t fl = align_up(N);
    w.counters_bytes = 8 * fl + 256 + 256 + 256 + 4 * 128 + 256;
    uint8_t* f = c.take<uint8_t>(w.counters_bytes);
    w.counters = f;
    w.d1flag = f; w.fa1 = w.d1flag + fl; w.fa2 = w.fa1 + fl; w.fa3 = w.fa2 + fl;
    w.fD1 = w.fa3 + fl; w.fD2 = w.fD1 + fl; w.fS1 = w.fD2 + fl; w.fS2 = w.fS1 + fl;
    auto counts = [&](size_t region, std::initializer_list<NodeList*> lists) {
        int k = 0;
        for (NodeList* l : lists) l->count = (int*)(f + 8 * fl + region + 64 * k++);
    };
    counts(0, {&w.act});
    counts(256, {&w.A1, &w.A2, &w.A3});
    counts(512, {&w.D1, &w.S1, &w.D2, &w.S2});
    counts(768, {&w.all_gen, &w.all_pp, &w.D2_gen, &w.D2_pp, &w.A1_gen, &w.A1_pp, &w.A2_gen, &w.A2_pp});
    NodeList step_l0, step_u1;    // (the empty list's 256 bytes hold four counts)
    counts(768 + 4 * 128, {&w.empty, &step_l0, &step_u1});
    w.step_count[0] = step_l0.count; w.step_count[1] = step_u1.count;
    w.total = c.off;
    return w;
}

// carve + size check of the entry points that take a forward workspace
static int carve_checked(const char* who, void* workspace, size_t workspace_bytes, int n_nodes, Workspace& w) {
    w = carve(workspace, n_nodes);
    if (workspace_bytes < w.total) return fail(CBGX_E_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, w.total);
    return CBGX_OK;
}

// The step cache of a sampling state (cbgx_unitransformer_forward_step_cached): what the first two layers of a static-context call
// compute again in every one of the T calls although its inputs did not change.  The block outlives the call; the arrays hold EVERY row.
//   P[0] / q[0]   node stage of layer 0 (input: the caller's h).  Protein rows of h never change, so after the first call only the
//                 ligand rows are computed.
//   hbuf[0]       output of layer 0: the static_h1 row outside D1(t).  Per call the rows of D1(t-1) are placed again, then the layer
//                 writes D1(t).
//   P[1] / q[1]   node stage of layer 1 (input: hbuf[0]): computed on D1(t) | D1(t-1) -- a row that left D1 is computed from its restored
//                 static row, which gives the static projection again.
//   hbuf[1]       output of layer 1, the same with D2 and static_h2.
// Three flag arrays carry the state from call to call, all ones after cbgx_step_cache_reset, so that the first call computes and places
// every row through the same launches: fresh0 (layer-0 node stage not yet computed), prevD1 / prevD2 (adjacent: saved by one copy).
struct StepCache {
    float *P[2], *q[2], *hbuf[2];
    NodeList L0, U1;            // rows of the layer-0 / layer-1 node stage of this call (counts: in the workspace's counter block)
    uint8_t *fresh0, *prevD1, *prevD2;
    size_t flag_stride, total;
};
static StepCache carve_step_cache(void* base, int n) {
    StepCache c;
    Carver k(base);
    const size_t N = (size_t)(n > 0 ? n : 1);
    for (int l = 0; l < 2; ++l) {
        c.P[l] = k.take<float>(N * PROW * 4);
        c.q[l] = k.take<float>(N * H * 4);
        c.hbuf[l] = k.take<float>(N * H * 4);
    }
    c.L0.rows = k.take<int>(N * 4);
    c.U1.rows = k.take<int>(N * 4);
    c.L0.count = c.U1.count = nullptr;
    c.flag_stride = align_up(N);
    c.fresh0 = k.take<uint8_t>(3 * c.flag_stride);
    c.prevD1 = c.fresh0 + c.flag_stride;
    c.prevD2 = c.prevD1 + c.flag_stride;
    c.total = k.off;
    return c;
}
// CBGX_STEP_CACHE=0 (schedule knob, read once per process): step-cached calls run the launches of cbgx_unitransformer_forward_cached
static bool step_cache_enabled() {
    static const bool on = [] { const char* e = getenv("CBGX_STEP_CACHE"); return !e || atoi(e) != 0; }();
    return on;
}

// Auxiliary streams: one per (host thread, caller stream), created on first use, with the two events that fork it from and join it
// back into that caller stream.  A caller that keeps two forward calls in flight on two of its streams (two resident batches: the
// HBM-bound node kernels of one run under the matrix-bound edge kernel of the other) must not have them share an auxiliary stream --
// the node stages of the second call would queue behind all nine of the first.  A small table keyed by the caller's stream handle;
// when it is full the entries change owner round-robin (aux_for).  Nothing here is shared between host threads.
constexpr int MAX_AUX = 8;    // batches a caller can keep in flight without aux streams changing owner (bench --streams 8, sample_many)
struct AuxTable {
    int dev = -1;
    int n = 0;
    int next_victim = 0;
    AuxStream e[MAX_AUX];
};
static thread_local AuxTable g_aux_table;
namespace cbgx {
AuxStream* aux_for(hipStream_t caller) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    AuxTable& t = g_aux_table;
    if (t.n && t.dev != dev) return nullptr;   // one device per host thread (one process per GPU); otherwise stay serial
    for (int k = 0; k < t.n; ++k)
        if (t.e[k].owner == caller) return &t.e[k];
    if (t.n == MAX_AUX) {
        // table full: the entries change owner round-robin.  Stream and events are reused, not destroyed -- work the previous
        // owner's calls queued on the stream simply stays ahead of the new owner's (stream order), waits already enqueued on the
        // events keep referring to the records they were enqueued after, and nothing here blocks the host, so this is also
        // legal while the caller's stream is being captured into a graph.
        AuxStream& e = t.e[t.next_victim];
        t.next_victim = (t.next_victim + 1) % MAX_AUX;
        e.owner = caller;
        return &e;
    }
    AuxStream a;
    a.owner = caller;
    // CBGX_AUX_PRIORITY=low (opt-in, schedule only): the auxiliary stream at the device's least priority, so that the caller's node-level
    // kernels get the CUs first where both queues have workgroups ready (measured: profiles/ab_train_r06r2.log)
    static const bool low = [] { const char* e = getenv("CBGX_AUX_PRIORITY"); return e && e[0] == 'l'; }();
    int least = 0, greatest = 0;
    if (low && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest) {
        if (hipStreamCreateWithPriority(&a.s, hipStreamNonBlocking, least) != hipSuccess) return nullptr;
    } else if (hipStreamCreateWithFlags(&a.s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&a.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&a.join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&a.done[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&a.done[1], hipEventDisableTiming) != hipSuccess) {
        (void)hipStreamDestroy(a.s);
        return nullptr;
    }
    t.dev = dev;
    t.e[t.n] = a;
    return &t.e[t.n++];
}
}  // namespace cbgx

extern "C" {

int cbgx_abi_version(void) { return CBGX_ABI_VERSION; }
const char* cbgx_last_error(void) { return g_err; }

#ifdef CBGX_XCHECK
// test-only library (include/cbgx_xcheck.h): route the stages through the first-generation VALU kernels
int cbgx_debug_set_edge_kernel(int impl) {
    if (impl < 0 || impl > 2) return fail(CBGX_E_INVALID, "debug_set_edge_kernel: impl must be 0 (current), 1 (valu) or 2 (mfma, second-generation x2h backward)");
    int old = g_edge_impl;
    g_edge_impl = impl;
    return old;
}

// test-only library: where a forward call of n_nodes nodes keeps its graph stage and node lists (the same carve, no launch)
int cbgx_debug_forward_view(void* workspace, int n_nodes, void** out) {
    if (!workspace || !out || n_nodes < 1) return fail(CBGX_E_INVALID, "debug_forward_view: bad argument");
    const Workspace w = carve(workspace, n_nodes);
    int k = 0;
    out[k++] = w.nbr; out[k++] = w.deg; out[k++] = w.e_w; out[k++] = w.d1flag; out[k++] = w.fD1;
    const NodeList lists[] = {w.act,     w.A1,     w.A2,     w.A3,    w.D1,     w.S1,    w.D2,     w.S2,
                              w.all_gen, w.all_pp, w.D2_gen, w.D2_pp, w.A1_gen, w.A1_pp, w.A2_gen, w.A2_pp};
    for (const NodeList& l : lists) { out[k++] = l.rows; out[k++] = l.count; }
    static_assert(sizeof(lists) / sizeof(lists[0]) == CBGX_FWD_VIEW_LISTS, "cbgx_debug_forward_view: list count");
    static_assert(CBGX_FWD_VIEW_PTRS == 5 + 2 * 16, "cbgx_debug_forward_view: list count");
    return k == CBGX_FWD_VIEW_PTRS ? CBGX_OK : fail(CBGX_E_INVALID, "debug_forward_view: %d pointers", k);
}
#endif

int cbgx_set_edge_workgroups(int n) { return set_edge_workgroup_limit(n); }

size_t cbgx_packed_weights_floats(int num_layers, int num_classes) {
    if (num_layers < 0 || num_classes < 1 || num_classes > CBGX_MAX_CLASSES) return 0;
    return packed_floats(num_layers, num_classes);
}

// strided / transposed copies are collected and issued as one launch per batch (they only read the caller's tensors and
// are only consumed by later forward calls, so deferring them to the next flush on the same stream is safe)
static thread_local PackBatch g_pack;
static int flush_pack(hipStream_t s) {
    if (g_pack.n) {
        HIP_TRY(launch_pack_copy_multi(g_pack, s));
        g_pack.n = 0;
    }
    return CBGX_OK;
}
static int queue_pack(const float* src, int ld, int off, int tr, float* dst, int dld, int rows, int cols, hipStream_t s) {
    if (g_pack.n == PACK_MAX) { int rc = flush_pack(s); if (rc) return rc; }
    g_pack.p[g_pack.n++] = PackPiece{src, dst, ld, off, tr, dld, rows, cols};
    return CBGX_OK;
}
#define CP(src, ld, off, tr, dst, dld, rows, cols)                                 \
    do {                                                                           \
        int _rc = queue_pack(src, ld, off, tr, dst, dld, rows, cols, s);           \
        if (_rc) return _rc;                                                       \
    } while (0)

// gate section (GATE_* offsets) from dist_emb.1.net.{0.weight,0.bias,1.weight,1.bias,3.weight,3.bias}
static int pack_gate_section(const float* const* t, float* packed, hipStream_t s) {
    // gate MLP: net.0 [160,20], net.1 LN(160), net.3 [1,160]
    CP(t[0], G, 0, 0, packed + GATE_W1, G, GH, G);
    CP(t[1], GH, 0, 0, packed + GATE_B1, GH, 1, GH);
    CP(t[2], GH, 0, 0, packed + GATE_LNG, GH, 1, GH);
    CP(t[3], GH, 0, 0, packed + GATE_LNB, GH, 1, GH);
    CP(t[4], GH, 0, 0, packed + GATE_W2, GH, 1, GH);
    CP(t[5], 1, 0, 0, packed + GATE_B2, 1, 1, 1);
    HIP_TRY(launch_pack_gate_img(t[0], t[1], t[2], t[3], t[4], packed + GATE_IMG, s));
    return flush_pack(s);
}

// ---- attention blocks (ATT layout) from k(6) v(6) q(6) MLP tensors each; blk 0 = x2h, 1 = h2x.  Packed for ALL blocks of a
// model phase by phase (the weights are re-packed every training step): copies of the reference tensors, stage 1 (centring),
// copies of the centred matrices, stage 2 (every fragment table) -- ~20 launches instead of 12 per block.
struct BlockRef { const float* const* p; int blk; float* a; };

// copies that read the caller's tensors only
static int queue_block_copies(const BlockRef& r, hipStream_t s) {
    const float* const* p = r.p;
    float* a = r.a;
    const int blk = r.blk;
    const float *wk0 = p[0], *bk0 = p[1], *gk = p[2], *bek = p[3], *wk1 = p[4];
    const float *wv0 = p[6], *bv0 = p[7], *gv = p[8], *bev = p[9], *wv1 = p[10], *bv1 = p[11];
    const float *wq0 = p[12], *bq0 = p[13], *gq = p[14], *beq = p[15], *wq1 = p[16], *bq1 = p[17];
    // node projection [k][c]: PDk | PDv | PSk | PSv | q hidden
    CP(wk0, KV_IN, NT + NT * G, 1, a + A_WN + 0 * H, PROW, H, H);
    CP(wv0, KV_IN, NT + NT * G, 1, a + A_WN + 1 * H, PROW, H, H);
    CP(wk0, KV_IN, NT + NT * G + H, 1, a + A_WN + 2 * H, PROW, H, H);
    CP(wv0, KV_IN, NT + NT * G + H, 1, a + A_WN + 3 * H, PROW, H, H);
    CP(wq0, H, 0, 1, a + A_WN + 4 * H, PROW, H, H);
    CP(bk0, H, 0, 0, a + A_BN + 0 * H, H, 1, H);
    CP(bv0, H, 0, 0, a + A_BN + 1 * H, H, 1, H);
    CP(bq0, H, 0, 0, a + A_BN + 4 * H, H, 1, H);
    // edge-type one-hot columns and rbf columns of the first Linear
    CP(wk0, KV_IN, 0, 1, a + A_WT, 2 * H, NT, H);
    CP(wv0, KV_IN, 0, 1, a + A_WT + H, 2 * H, NT, H);
    CP(wk0, KV_IN, NT, 1, a + A_WR, 2 * H, NT * G, H);
    CP(wv0, KV_IN, NT, 1, a + A_WR + H, 2 * H, NT * G, H);
    CP(gk, H, 0, 0, a + A_LNK_G, H, 1, H);
    CP(bek, H, 0, 0, a + A_LNK_B, H, 1, H);
    CP(gv, H, 0, 0, a + A_LNV_G, H, 1, H);
    CP(bev, H, 0, 0, a + A_LNV_B, H, 1, H);
    CP(gq, H, 0, 0, a + A_LNQ_G, H, 1, H);
    CP(beq, H, 0, 0, a + A_LNQ_B, H, 1, H);
    CP(wq1, H, 0, 1, a + A_WQ1T, H, H, H);
    CP(bq1, H, 0, 0, a + A_BQ1, H, 1, H);
    CP(wk1, H, 0, 0, a + A_WBK, H, H, H);
    CP(wk1, H, 0, 1, a + A_WBKT, H, H, H);
    CP(wq1, H, 0, 0, a + A_WQ1O, H, H, H);
    for (int ty = 0; ty < NT; ++ty) {   // WRT[ty][c][g] = W_a[c][4 + 20 ty + g]  (g 20..31 stay zero)
        CP(wk0, KV_IN, NT + G * ty, 0, a + A_WRT + (size_t)ty * 2 * H * 32, 32, H, G);
        CP(wv0, KV_IN, NT + G * ty, 0, a + A_WRT + ((size_t)ty * 2 * H + H) * 32, 32, H, G);
    }
    // LDS image of the MFMA edge kernel: LayerNorm affines; second v Linear
    float* img = a + A_IMG;
    CP(gk, H, 0, 0, img + IMG_LN + 0 * H, H, 1, H);
    CP(bek, H, 0, 0, img + IMG_LN + 1 * H, H, 1, H);
    CP(gv, H, 0, 0, img + IMG_LN + 2 * H, H, 1, H);
    CP(bev, H, 0, 0, img + IMG_LN + 3 * H, H, 1, H);
    if (blk == 0) {
        CP(wv1, H, 0, 1, a + A_WBV, H, H, H);   // [m][n]
        CP(bv1, H, 0, 0, a + A_BBV, H, 1, H);
    } else {
        CP(wv1, H, 0, 0, a + A_WBV, H, HEADS, H);  // [head][m]
        CP(bv1, HEADS, 0, 0, a + A_BBV, HEADS, 1, HEADS);
    }
    return CBGX_OK;
}

// copies that read the centred first Linears stage 1 has just produced on this stream
static int queue_centred_copies(const BlockRef& r, hipStream_t s) {
    float* a = r.a;
    CP(a + A_WAKC, KV_IN, NT, 1, a + A_WRC, 2 * H, NT * G, H);
    CP(a + A_WAVC, KV_IN, NT, 1, a + A_WRC + H, 2 * H, NT * G, H);
    return CBGX_OK;
}

static int pack_attention_blocks(const BlockRef* refs, int n_blocks, hipStream_t s) {
    for (int k0 = 0; k0 < n_blocks; k0 += PACK_BLOCKS_MAX) {
        const int nb = n_blocks - k0 < PACK_BLOCKS_MAX ? n_blocks - k0 : PACK_BLOCKS_MAX;
        PackBlocks pb;
        memset(&pb, 0, sizeof(pb));
        pb.n = nb;
        for (int k = 0; k < nb; ++k) {
            const BlockRef& r = refs[k0 + k];
            pb.wk0[k] = r.p[0]; pb.bk0[k] = r.p[1]; pb.wk1[k] = r.p[4];
            pb.wv0[k] = r.p[6]; pb.bv0[k] = r.p[7]; pb.wv1[k] = r.p[10];
            pb.wq0[k] = r.p[12]; pb.bq0[k] = r.p[13]; pb.wq1[k] = r.p[16];
            pb.att[k] = r.a;
            pb.nsrc[k][0] = r.a + A_WAKC; pb.nsrc[k][1] = r.a + A_WAVC; pb.nsrc[k][2] = r.a + A_WAKC; pb.nsrc[k][3] = r.a + A_WAVC;
            pb.nsrc[k][4] = r.p[12];
            pb.x2h[k] = r.blk == 0;
            int rc = queue_block_copies(r, s);
            if (rc) return rc;
        }
        { int rc = flush_pack(s); if (rc) return rc; }
        HIP_TRY(launch_pack_stage1(pb, s));
        for (int k = 0; k < nb; ++k) { int rc = queue_centred_copies(refs[k0 + k], s); if (rc) return rc; }
        { int rc = flush_pack(s); if (rc) return rc; }
        HIP_TRY(launch_pack_stage2(pb, s));
    }
    return CBGX_OK;
}

int cbgx_pack_weights(const float* const* t, int num_tensors, int L, int C, float* packed, void* stream) {
    if (C > CBGX_MAX_CLASSES) return fail(CBGX_E_INVALID, "pack_weights: num_classes=%d > %d", C, CBGX_MAX_CLASSES);
    if (!t || !packed) return fail(CBGX_E_INVALID, "pack_weights: NULL pointer");
    if (L < 1 || C < 1) return fail(CBGX_E_INVALID, "pack_weights: num_layers=%d num_classes=%d", L, C);
    if (num_tensors != 6 + 36 * L + 4)
        return fail(CBGX_E_INVALID, "pack_weights: expected %d tensors, got %d", 6 + 36 * L + 4, num_tensors);
    for (int i = 0; i < num_tensors; ++i)
        if (!t[i]) return fail(CBGX_E_INVALID, "pack_weights: tensor %d is NULL", i);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(packed, 0, packed_floats(L, C) * sizeof(float), s));
    { int rc = pack_gate_section(t, packed, s); if (rc) return rc; }
    {
        std::vector<BlockRef> refs;
        for (int l = 0; l < L; ++l)
            for (int blk = 0; blk < 2; ++blk)
                refs.push_back(BlockRef{t + 6 + 36 * l + 18 * blk /* k(6) v(6) q(6) */, blk, packed + (blk == 0 ? x2h_off(l) : h2x_off(l))});
        int rc = pack_attention_blocks(refs.data(), (int)refs.size(), s);
        if (rc) return rc;
    }
    const float* const* c = t + 6 + 36 * L;
    float* cp = packed + cls_off(L);
    CP(c[0], H, 0, 1, cp + C_W0T, H, H, H);
    CP(c[1], H, 0, 0, cp + C_B0, H, 1, H);
    CP(c[2], H, 0, 1, cp + C_W1T, C, H, C);
    CP(c[3], C, 0, 0, cp + cls_b1(C), C, 1, C);
    return flush_pack(s);
}

// ---- a stack of H2X blocks on its own kNN graph + gate (DiffBP's CoMPredictor) ---------------------
size_t cbgx_packed_h2x_stack_floats(int num_layers) {
    if (num_layers < 1) return 0;
    return GATE_SIZE + (size_t)num_layers * ATT_SIZE;
}

int cbgx_pack_h2x_stack(const float* const* t, int num_tensors, int L, float* packed, void* stream) {
    if (!t || !packed) return fail(CBGX_E_INVALID, "pack_h2x_stack: NULL pointer");
    if (L < 1 || num_tensors != 6 + 18 * L)
        return fail(CBGX_E_INVALID, "pack_h2x_stack: expected %d tensors for %d layers, got %d", 6 + 18 * L, L, num_tensors);
    for (int i = 0; i < num_tensors; ++i)
        if (!t[i]) return fail(CBGX_E_INVALID, "pack_h2x_stack: tensor %d is NULL", i);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(packed, 0, cbgx_packed_h2x_stack_floats(L) * sizeof(float), s));
    { int rc = pack_gate_section(t, packed, s); if (rc) return rc; }
    std::vector<BlockRef> refs;
    for (int l = 0; l < L; ++l) refs.push_back(BlockRef{t + 6 + 18 * l, 1, packed + GATE_SIZE + (size_t)l * ATT_SIZE});
    { int rc = pack_attention_blocks(refs.data(), (int)refs.size(), s); if (rc) return rc; }
    return flush_pack(s);
}

// the h2x blocks of a call run the ligand-row edge kernel (edge_h2x_lig.hip; no folded rows Qt): the caller's promise, the product
// kernels, and CBGX_H2X_FOLD
static bool h2x_lig_selected(unsigned flags) { return (flags & CBGX_FWD_GEN_IS_LIGAND) && g_edge_impl != 1 && h2x_fold_enabled(); }

int cbgx_h2x_stack_forward_v2(const float* packed, int num_layers, const float* x, const float* h,
                              const int32_t* graph_ptr, const uint8_t* lig_flag, const uint8_t* gen_flag, int n_nodes,
                              int n_graphs, float* x_out, unsigned flags, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_nodes < 0 || n_graphs < 0 || num_layers < 1) return fail(CBGX_E_INVALID, "h2x_stack: bad sizes");
    if (flags & ~CBGX_FWD_GEN_IS_LIGAND) return fail(CBGX_E_INVALID, "h2x_stack: unknown flags 0x%x", flags);
    if (n_nodes == 0) return CBGX_OK;
    if (!packed || !x || !h || !graph_ptr || !lig_flag || !gen_flag || !x_out || !workspace)
        return fail(CBGX_E_INVALID, "h2x_stack: NULL pointer");
    Workspace w;
    if (int rc = carve_checked("h2x_stack", workspace, workspace_bytes, n_nodes, w)) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_build_active(gen_flag, n_nodes, w.act, s));
    if (g_edge_impl == 1) {
        HIP_TRY(launch_knn(x, graph_ptr, n_graphs, n_nodes, w.nbr, w.deg, s));
        HIP_TRY(launch_gate(packed, x, w.nbr, w.deg, n_nodes, w.e_w, s));
    } else {
        // An H2X block only ever reads the neighbour list and the gate values of the nodes it moves (edge kernel and source marking
        // both run over the gen_flag list), and the stack's graph is built once from the input coordinates (diffbp.py:84-93): the
        // kNN search and the gate MLP run on the listed rows only -- the ligand atoms, ~5 % of a pocket -- instead of on every node
        // (DiffBP paid 415 + 276 us per step for them at 200 graphs, against 163 + 112 us for the denoiser's cached graph).
        HIP_TRY(launch_knn_reg(x, graph_ptr, n_graphs, n_nodes, w.nbr, w.deg, s, w.act));
        HIP_TRY(launch_gate_mfma(packed, x, w.nbr, w.deg, n_nodes, w.e_w, s, w.act));
    }
    // The source rows of the stack: the in-neighbours of the movable rows (and those rows themselves).  Only their PS columns are
    // ever gathered, so only they are projected -- and only their rows of h are read, which is what lets the denoiser in front
    // (cbgx_unitransformer_forward_cached, CBGX_FWD_H_ON_SOURCES) skip every other row of its last layers.
    RowList src;
    if (g_edge_impl != 1) {
        HIP_TRY(launch_mark_seed(gen_flag, gen_flag, n_nodes, w.fa1, s));
        HIP_TRY(walk_receptive_field(w.fa1, w.act, w.nbr, w.deg, n_nodes, {w.A1}, s));
        src = w.A1;
    }
    const Graph g{w.nbr, w.deg, w.e_w, lig_flag, gen_flag, n_nodes};
    const float* xc = x;
    for (int l = 0; l < num_layers; ++l) {
        float* xn = (l == num_layers - 1) ? x_out : w.xbuf[l & 1];
        HIP_TRY(launch_attention(false, packed + GATE_SIZE + (size_t)l * ATT_SIZE, g, xc, h, w.set[0], xn, nullptr, w.act, src, s,
                                 h2x_lig_selected(flags)));
        xc = xn;
    }
    return CBGX_OK;
}

int cbgx_h2x_stack_forward(const float* packed, int num_layers, const float* x, const float* h,
                           const int32_t* graph_ptr, const uint8_t* lig_flag, const uint8_t* gen_flag, int n_nodes,
                           int n_graphs, float* x_out, void* workspace, size_t workspace_bytes, void* stream) {
    return cbgx_h2x_stack_forward_v2(packed, num_layers, x, h, graph_ptr, lig_flag, gen_flag, n_nodes, n_graphs, x_out, 0u, workspace,
                                     workspace_bytes, stream);
}

size_t cbgx_workspace_bytes(int n_nodes, int n_graphs) {
    (void)n_graphs;
    return carve(nullptr, n_nodes).total;
}

int cbgx_knn_graph(const float* x, const int32_t* graph_ptr, int n_graphs, int n_nodes, int k, int32_t* nbr,
                   int32_t* deg, void* stream) {
    if (k != KNN) return fail(CBGX_E_INVALID, "knn_graph: only k=%d is supported (got %d)", KNN, k);
    if (n_nodes < 0 || n_graphs < 0) return fail(CBGX_E_INVALID, "knn_graph: negative size");
    if (n_nodes == 0) return CBGX_OK;
    if (!x || !graph_ptr || !nbr || !deg || n_graphs < 1) return fail(CBGX_E_INVALID, "knn_graph: NULL pointer");
    HIP_TRY(launch_knn(x, graph_ptr, n_graphs, n_nodes, nbr, deg, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_edge_gate(const float* packed, const float* x, const int32_t* nbr, const int32_t* deg, int n_nodes,
                   float* e_w, void* stream) {
    if (n_nodes == 0) return CBGX_OK;
    if (!packed || !x || !nbr || !deg || !e_w || n_nodes < 0) return fail(CBGX_E_INVALID, "edge_gate: bad argument");
    HIP_TRY(launch_gate(packed, x, nbr, deg, n_nodes, e_w, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_x2h_attention(const float* packed, int layer, const float* x, const float* h, const int32_t* nbr,
                       const int32_t* deg, const uint8_t* lig_flag, const float* e_w, int n_nodes, float* h_out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (n_nodes == 0) return CBGX_OK;
    if (!packed || !x || !h || !nbr || !deg || !lig_flag || !e_w || !h_out || !workspace || layer < 0 || n_nodes < 0)
        return fail(CBGX_E_INVALID, "x2h_attention: bad argument");
    Workspace w;
    if (int rc = carve_checked("x2h_attention", workspace, workspace_bytes, n_nodes, w)) return rc;
    const NodeBufs& b = w.set[0];
    const Graph g{nbr, deg, e_w, lig_flag, nullptr, n_nodes};
    const float* att = packed + x2h_off(layer);
    hipStream_t s = (hipStream_t)stream;
    if (g_edge_impl == 1) {
        HIP_TRY(launch_attention(true, att, g, x, h, b, h_out, nullptr, {}, {}, s));
        return CBGX_OK;
    }
    // what a layer of cbgx_unitransformer_forward runs: protein-only destinations fold their query in registers, Qt is
    // produced for the others only, one two-role edge launch
    HIP_TRY(launch_mark_from_nbr(lig_flag, nbr, deg, n_nodes, w.d1flag, s));
    HIP_TRY(launch_split_list({}, n_nodes, w.d1flag, w.all_gen, w.all_pp, s));
    NodeStageOpts o;
    o.large_lists = true;
    o.fold = w.all_gen;
    HIP_TRY(launch_node_mfma(att, h, lig_flag, n_nodes, b, {}, {}, s, o));
    HIP_TRY(launch_edge_x2h_dual(att, g, x, h, b, h_out, w.all_pp, w.all_gen, true, s));
    return CBGX_OK;
}

int cbgx_h2x_attention_v2(const float* packed, int layer, const float* x, const float* h, const int32_t* nbr,
                          const int32_t* deg, const uint8_t* lig_flag, const uint8_t* gen_flag, const float* e_w,
                          int n_nodes, float* x_out, float* delta_x, unsigned flags, void* workspace, size_t workspace_bytes,
                          void* stream) {
    if (flags & ~CBGX_FWD_GEN_IS_LIGAND) return fail(CBGX_E_INVALID, "h2x_attention: unknown flags 0x%x", flags);
    if (n_nodes == 0) return CBGX_OK;
    if (!packed || !x || !h || !nbr || !deg || !lig_flag || !gen_flag || !e_w || !x_out || !workspace || layer < 0 ||
        n_nodes < 0)
        return fail(CBGX_E_INVALID, "h2x_attention: bad argument");
    Workspace w;
    if (int rc = carve_checked("h2x_attention", workspace, workspace_bytes, n_nodes, w)) return rc;
    const Graph g{nbr, deg, e_w, lig_flag, gen_flag, n_nodes};
    HIP_TRY(launch_build_active(gen_flag, n_nodes, w.act, (hipStream_t)stream));
    HIP_TRY(launch_attention(false, packed + h2x_off(layer), g, x, h, w.set[0], x_out, delta_x, w.act, {}, (hipStream_t)stream,
                             h2x_lig_selected(flags)));
    return CBGX_OK;
}

int cbgx_h2x_attention(const float* packed, int layer, const float* x, const float* h, const int32_t* nbr,
                       const int32_t* deg, const uint8_t* lig_flag, const uint8_t* gen_flag, const float* e_w,
                       int n_nodes, float* x_out, float* delta_x, void* workspace, size_t workspace_bytes,
                       void* stream) {
    return cbgx_h2x_attention_v2(packed, layer, x, h, nbr, deg, lig_flag, gen_flag, e_w, n_nodes, x_out, delta_x, 0u, workspace,
                                 workspace_bytes, stream);
}

int cbgx_node_stage(const float* packed, int layer, int x2h, const float* h, const uint8_t* lig_flag, int n_nodes,
                    const int32_t* rows, const int32_t* n_rows, int q_direct, float* P, float* q, float* Qt, void* stream) {
    if (n_nodes == 0) return CBGX_OK;
    if (!packed || !h || !lig_flag || !P || !q || !Qt || layer < 0 || n_nodes < 0 || (rows == nullptr) != (n_rows == nullptr))
        return fail(CBGX_E_INVALID, "node_stage: bad argument");
    NodeStageOpts o;
    o.large_lists = true;
    o.q_direct = q_direct != 0;
    HIP_TRY(launch_node_mfma(packed + (x2h ? x2h_off(layer) : h2x_off(layer)), h, lig_flag, n_nodes, NodeBufs{P, q, Qt},
                             RowList{rows, n_rows}, {}, (hipStream_t)stream, o));
    return CBGX_OK;
}

// the classifier head on every row, or on the listed ones (`hidden`: [n_nodes][128] scratch)
static int classifier_head(const float* packed, int num_layers, int num_classes, const float* h, int n_nodes, float* hidden,
                           float* logits, RowList rows, hipStream_t s) {
    const float* c = packed + cls_off(num_layers);
    HIP_TRY(launch_node_gemm(h, H, c + C_W0T, c + C_B0, hidden, H, n_nodes, H, 1, s, rows));
    HIP_TRY(launch_node_gemm(hidden, H, c + C_W1T, c + cls_b1(num_classes), logits, num_classes, n_nodes, num_classes, 0, s, rows));
    return CBGX_OK;
}

int cbgx_classifier(const float* packed, int num_layers, int num_classes, const float* h, int n_nodes, float* logits,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (num_classes > CBGX_MAX_CLASSES) return fail(CBGX_E_INVALID, "classifier: num_classes=%d > %d", num_classes, CBGX_MAX_CLASSES);
    if (n_nodes == 0) return CBGX_OK;
    if (!packed || !h || !logits || !workspace || num_layers < 0 || num_classes < 1 || n_nodes < 0)
        return fail(CBGX_E_INVALID, "classifier: bad argument");
    Workspace w;
    if (int rc = carve_checked("classifier", workspace, workspace_bytes, n_nodes, w)) return rc;
    return classifier_head(packed, num_layers, num_classes, h, n_nodes, w.set[0].P, logits, {}, (hipStream_t)stream);
}

// ---- the denoiser's forward (cbgx_unitransformer_forward, cbgx_unitransformer_forward_cached) ---------------------------------------
// What layer l works on, computed once per call (plan_layers) and read by all three schedules
struct LayerPlan {
    NodeList dst, src;          // x2h node stage: own columns, q and Qt on dst, PS columns on src ({NULL, NULL}: every row)
    NodeList gen, pp;           // x2h edge launch: general-role and protein-only destinations
    bool full_layer;            // ... which together are every node
    const uint8_t* fold_flag;   // fused node stage: Qt only for the flagged rows of dst (NULL: for all of them)
    NodeList node;              // step cache: P (own and PS columns) and q on these rows alone, in place of dst / src
};

// a forward call: its arguments, then what forward_impl derives from them for its parts
struct Forward {
    const float* packed; int num_layers, num_classes; const float *x, *h; const int32_t* graph_ptr; const uint8_t *lig_flag, *gen_flag;
    int n_nodes, n_graphs; float *x_out, *h_out, *logits;
    const float *static_h1, *static_h2; const int32_t *static_nbr, *static_deg; const float *static_ew, *static_r32sq;
    unsigned flags; void* workspace; size_t workspace_bytes; hipStream_t s;
    void* step_block = nullptr; size_t step_block_bytes = 0;     // (cbgx_unitransformer_forward_step_cached)
    Workspace w;
    Graph graph;                // w.nbr / deg / e_w with the caller's flags: what every attention block of the call runs on
    bool cached, graph_cached, prune, dual;
    bool h2x_lig;               // h2x blocks: ligand-row edge kernel, node stage without the fold (CBGX_FWD_GEN_IS_LIGAND)
    bool step;                  // layers 0 / 1 on the step cache `sc`
    StepCache sc;
    std::vector<LayerPlan> plan;
};

// nbr / deg / e_w of the call
static int forward_graph_stage(const Forward& f) {
    const Workspace& w = f.w;
    const int n_nodes = f.n_nodes, n_graphs = f.n_graphs;
    hipStream_t s = f.s;
    if (!f.graph_cached) {
        HIP_TRY(launch_knn(f.x, f.graph_ptr, n_graphs, n_nodes, w.nbr, w.deg, s));
        HIP_TRY(launch_gate(f.packed, f.x, w.nbr, w.deg, n_nodes, w.e_w, s));
        return CBGX_OK;
    }
    // D1 flags + list, the pocket's own graph and the cached features of layers 0 / 1 (into hbuf[0] / hbuf[1]: num_layers >= 4,
    // so neither is the caller's h_out, and nothing else touches them before their layer): one launch
    HIP_TRY(launch_graph_cache_begin(f.x, f.graph_ptr, n_graphs, f.lig_flag, f.static_r32sq, n_nodes, w.fD1, w.D1.rows, w.D1.count,
                                     f.static_nbr, f.static_deg, f.static_ew, w.nbr, w.deg, w.e_w, f.static_h1, f.static_h2,
                                     f.step ? f.sc.hbuf[0] : w.hbuf[0], f.step ? f.sc.hbuf[1] : w.hbuf[1], s,
                                     f.step ? f.sc.prevD1 : nullptr, f.step ? f.sc.prevD2 : nullptr));
    // the D1 centres' merged neighbour lists and gate values: kept pocket entries carry their cached value to their new rank, the gate
    // MLP runs on the ligand atoms that entered the list.  Small inputs: ONE launch (knn_merge_gate_kernel: a persistent kernel at one
    // wave per SIMD -- at 173 k nodes it measured 612 us against 153 + 175 for the two kernels, profiles/ab_fwd_r05f.log); large inputs:
    // the merge marks the new ranks and the gate kernel evaluates only those.  CBGX_MERGE_GATE=0: the round-4 pair (all slots).
    static const int merge_gate = [] { const char* e = getenv("CBGX_MERGE_GATE"); return e ? atoi(e) : 1; }();
    if (merge_gate && n_nodes <= GRAPH_LISTS_MAX_NODES) {
        HIP_TRY(launch_knn_merge_gate(f.packed, f.x, f.graph_ptr, n_graphs, n_nodes, f.lig_flag, f.static_nbr, f.static_deg, f.static_ew,
                                      w.nbr, w.deg, w.e_w, s, w.D1));
    } else {
        const bool carry = merge_gate != 0;
        HIP_TRY(launch_knn_merge(f.x, f.graph_ptr, n_graphs, n_nodes, f.lig_flag, f.static_nbr, f.static_deg, w.nbr, w.deg, s, w.D1,
                                 carry ? f.static_ew : nullptr, carry ? w.e_w : nullptr, carry ? w.newmask : nullptr));
        HIP_TRY(launch_gate_mfma(f.packed, f.x, w.nbr, w.deg, n_nodes, w.e_w, s, w.D1, carry ? w.newmask : nullptr));
    }
    return CBGX_OK;
}

// Every list of the call.  Large inputs: three level kernels over the flags (a level reads what the previous one completed) and one
// compaction; inputs of <= GRAPH_LISTS_MAX_NODES nodes: one launch, a workgroup per graph with the graph's flags in LDS (round 5:
// the four launches were 20 us of a 600 us one-graph step)
static int forward_list_stage(const Forward& f) {
    const Workspace& w = f.w;
    hipStream_t s = f.s;
    const bool per_graph = f.n_nodes <= GRAPH_LISTS_MAX_NODES && g_edge_impl != 1;
    const GraphFlags gf{f.gen_flag, f.lig_flag, f.graph_cached ? w.fD1 : w.d1flag, w.d1flag, w.fa1, w.fa2, w.fa3, w.fD2, w.fS1, w.fS2};
    const uint8_t* flag_ptr[GF_COUNT] = {f.gen_flag, f.lig_flag, gf.D1, w.d1flag, w.fa1, w.fa2, w.fa3, w.fD2, w.fS1, w.fS2};
    ListJobs jobs;
    GraphListJobs gjobs;
    memset(&jobs, 0, sizeof(jobs));
    memset(&gjobs, 0, sizeof(gjobs));
    bool jobs_overflow = false;
    auto add = [&](int flag, int flag2, int want2, NodeList l) {
        if (jobs.n_jobs >= LIST_JOBS_MAX) { jobs_overflow = true; return; }
        const int k = jobs.n_jobs++;
        jobs.flag[k] = flag == GF_ALL ? nullptr : flag_ptr[flag]; jobs.flag2[k] = flag2 == GF_ALL ? nullptr : flag_ptr[flag2];
        jobs.want2[k] = want2; jobs.list[k] = l.rows; jobs.count[k] = l.count;
        gjobs.flag[k] = (signed char)flag; gjobs.flag2[k] = (signed char)flag2; gjobs.want2[k] = (signed char)want2;
        gjobs.list[k] = l.rows; gjobs.count[k] = l.count;
        gjobs.n_jobs = jobs.n_jobs;
    };
    auto pair = [&](int flag, NodeList gen, NodeList pp) { add(flag, GF_d1, 1, gen); add(flag, GF_d1, 0, pp); };
    add(GF_GEN, GF_ALL, 0, w.act);
    add(GF_a1, GF_ALL, 0, w.A1);
    if (f.prune) {
        add(GF_a2, GF_ALL, 0, w.A2);
        add(GF_a3, GF_ALL, 0, w.A3);
    }
    if (f.cached) {
        if (!f.graph_cached) add(GF_d1, GF_ALL, 0, w.D1);      // (graph-cached calls: graph_cache_begin has built it)
        add(GF_D2, GF_ALL, 0, w.D2);
        add(GF_S1, GF_ALL, 0, w.S1);
        add(GF_S2, GF_ALL, 0, w.S2);
    }
    if (f.step) {
        // L0 = ligand rows | rows never computed;  U1 = D1(t) | D1(t-1): two disjoint jobs appending to one list each
        auto add_ptr = [&](const uint8_t* flag, const uint8_t* flag2, NodeList l) {
            if (jobs.n_jobs >= LIST_JOBS_MAX) { jobs_overflow = true; return; }
            const int k = jobs.n_jobs++;
            jobs.flag[k] = flag; jobs.flag2[k] = flag2; jobs.want2[k] = 0; jobs.list[k] = l.rows; jobs.count[k] = l.count;
        };
        add_ptr(f.lig_flag, nullptr, f.sc.L0);
        add_ptr(f.sc.fresh0, f.lig_flag, f.sc.L0);
        add_ptr(w.fD1, nullptr, f.sc.U1);
        add_ptr(f.sc.prevD1, w.fD1, f.sc.U1);
    }
    if (f.dual) {
        pair(GF_ALL, w.all_gen, w.all_pp);
        if (f.cached) pair(GF_D2, w.D2_gen, w.D2_pp);
        if (f.prune) { pair(GF_a1, w.A1_gen, w.A1_pp); pair(GF_a2, w.A2_gen, w.A2_pp); }
    }
    if (jobs_overflow) return fail(CBGX_E_INVALID, "forward: more than %d node lists (LIST_JOBS_MAX)", LIST_JOBS_MAX);
    if (per_graph) {
        HIP_TRY(launch_graph_lists(f.gen_flag, f.lig_flag, f.graph_cached ? w.fD1 : nullptr, w.nbr, w.deg, f.graph_ptr, f.n_graphs, gjobs,
                                   f.cached, f.prune, w.d1flag, s));
    } else {
        HIP_TRY(launch_list_level(gf, w.nbr, w.deg, f.n_nodes, 0, f.cached, f.prune, s));
        if (f.cached || f.prune) {
            HIP_TRY(launch_list_level(gf, w.nbr, w.deg, f.n_nodes, 1, f.cached, f.prune, s));
            HIP_TRY(launch_list_level(gf, w.nbr, w.deg, f.n_nodes, 2, f.cached, f.prune, s));
        }
        HIP_TRY(launch_build_lists(jobs, f.n_nodes, s));
    }
    if (f.step) {
        // what the next call of this state starts from: every row of the layer-0 node stage exists, D1 / D2 of this call
        HIP_TRY(hipMemsetAsync(f.sc.fresh0, 0, f.sc.flag_stride, s));
        HIP_TRY(hipMemcpyAsync(f.sc.prevD1, w.fD1, 2 * f.sc.flag_stride, hipMemcpyDeviceToDevice, s));      // (fD1 | fD2, adjacent)
    }
    return CBGX_OK;
}

static void plan_layers(Forward& f) {
    const Workspace& w = f.w;
    const int L = f.num_layers;
    const NodeList every{nullptr, nullptr};
    f.plan.assign(L, LayerPlan{every, every, w.all_gen, w.all_pp, true, w.d1flag, every});
    if (f.cached) {     // (num_layers >= 4)
        // layer 0 on D1, all of it in the general role -- every row of D1 has a ligand atom among itself and its neighbours -- so
        // folded rows for the whole list; layer 1 on D2, of which d1flag picks the general part as in every other layer
        f.plan[0] = LayerPlan{w.D1, w.S1, w.D1, w.empty, false, nullptr, f.step ? f.sc.L0 : every};
        f.plan[1] = LayerPlan{w.D2, w.S2, w.D2_gen, w.D2_pp, false, w.d1flag, f.step ? f.sc.U1 : every};
    }
    if (f.prune) {      // (num_layers >= 3)
        f.plan[L - 2] = LayerPlan{w.A2, w.A3, w.A2_gen, w.A2_pp, false, w.d1flag, every};
        f.plan[L - 1] = LayerPlan{w.A1, w.A2, w.A1_gen, w.A1_pp, false, w.d1flag, every};
    }
}

// Where layer l writes -- the caller's buffers for the last layer, the workspace's otherwise -- and, in a static-features call without
// the graph part, the cached rows placed under the layer's output (graph-cached calls: graph_cache_begin has placed both)
static hipError_t begin_layer(const Forward& f, int l, float*& hn, float*& xn) {
    const bool last = l == f.num_layers - 1;
    hn = (last && f.h_out) ? f.h_out : ((f.step && l < 2) ? f.sc.hbuf[l] : f.w.hbuf[l & 1]);     // (step: num_layers >= 4, never last)
    xn = last ? f.x_out : f.w.xbuf[l & 1];
    if (!f.cached || l >= 2 || f.graph_cached) return hipSuccess;
    return hipMemcpyAsync(hn, l == 0 ? f.static_h1 : f.static_h2, (size_t)f.n_nodes * H * sizeof(float), hipMemcpyDeviceToDevice, f.s);
}

static hipError_t edge_x2h(const Forward& f, int l, const NodeBufs& b, const float* xc, const float* hc, float* hn) {
    const LayerPlan& p = f.plan[l];
    return launch_edge_x2h_dual(f.packed + x2h_off(l), f.graph, xc, hc, b, hn, p.pp, p.gen, p.full_layer, f.s);
}
// (q straight from h, no q-hidden columns in P: launch_node_mfma, large inputs only)
static hipError_t node_x2h(const Forward& f, int l, const NodeBufs& b, const float* h_in, hipStream_t on) {
    const LayerPlan& p = f.plan[l];
    NodeStageOpts o;
    o.large_lists = true;
    o.fold = p.gen;
    o.q_direct = node_qdirect_enabled();
    if (p.node.rows) {
        o.dst_all_columns = true;
        return launch_node_mfma(f.packed + x2h_off(l), h_in, f.lig_flag, f.n_nodes, b, p.node, {}, on, o);
    }
    return launch_node_mfma(f.packed + x2h_off(l), h_in, f.lig_flag, f.n_nodes, b, p.dst, p.src, on, o);
}
// the node-stage buffers of x2h layer l: P and q of a step-cached layer live in the cache block, its Qt stays in the workspace set
static NodeBufs bufs_x2h(const Forward& f, int l, const NodeBufs& set) {
    return (f.step && l < 2) ? NodeBufs{f.sc.P[l], f.sc.q[l], set.Qt} : set;
}
// the h2x block of layer l, node stage included: moves the `act` rows, whose sources are in A1
static hipError_t block_h2x(const Forward& f, int l, const NodeBufs& b, const float* xc, const float* hn, float* xn) {
    return launch_attention(false, f.packed + h2x_off(l), f.graph, xc, hn, b, xn, nullptr, f.w.act, f.w.A1, f.s, f.h2x_lig);
}

// Small inputs (round 5): ONE stream and ONE node-stage launch per layer.  The h2x block of layer l and the x2h block of layer
// l + 1 both read h_{l+1} and nothing else that is new, so their node stages are jobs of the same node_stage_kernel launch and a
// layer is three dependent launches -- x2h edge, node stages, h2x edge -- with no event between them.  The two-stream schedule
// hides the second node stage behind the h2x block instead, at the price of a fork and a join event per layer, ~7 us
// each on the caller's queue: 80 us per layer at one graph, of which 14 are the events and 24 + 25 the two edge launches
// (profiles/step_timeline_r05a_p1s1_ov1.json).
static int forward_fused(const Forward& f) {
    const Workspace& w = f.w;
    hipStream_t s = f.s;
    auto add_x2h = [&](NodeStageJobs& jobs, int l) {
        const LayerPlan& p = f.plan[l];
        add_node_stage_jobs(jobs, f.packed + x2h_off(l), w.set[l & 1], p.dst, p.src, p.fold_flag);
    };
    NodeStageJobs jobs;
    jobs.n = 0;
    add_x2h(jobs, 0);
    HIP_TRY(launch_node_stage_jobs(jobs, f.h, f.lig_flag, f.n_nodes, s));
    const float *xc = f.x, *hc = f.h;
    for (int l = 0; l < f.num_layers; ++l) {
        float *hn, *xn;
        HIP_TRY(begin_layer(f, l, hn, xn));
        HIP_TRY(edge_x2h(f, l, w.set[l & 1], xc, hc, hn));
        jobs.n = 0;
        add_node_stage_jobs(jobs, f.packed + h2x_off(l), w.set[2], w.act, w.A1, nullptr, f.h2x_lig);
        if (l + 1 < f.num_layers) add_x2h(jobs, l + 1);
        HIP_TRY(launch_node_stage_jobs(jobs, hn, f.lig_flag, f.n_nodes, s));
        if (f.h2x_lig) HIP_TRY(launch_edge_h2x_lig(f.packed + h2x_off(l), f.graph, xc, hn, w.set[2], xn, nullptr, w.act, s));
        else HIP_TRY(launch_edge_mfma(false, f.packed + h2x_off(l), f.graph, xc, hn, w.set[2], xn, nullptr, w.act, s));
        xc = xn;
        hc = hn;
    }
    return CBGX_OK;
}

// Two-stream schedule (MFMA kernels, profiling off): the node stage of x2h(l+1) only needs h_{l+1}, which exists as
// soon as the x2h edge kernel of layer l has run, while the h2x block of layer l (which only moves coordinates) is
// still to come -- so it runs on an auxiliary stream next to that h2x block.  Three node-stage buffer sets: x2h
// alternates between two, h2x has its own.
static int forward_two_streams(const Forward& f, AuxStream* aux) {
    hipStream_t s = f.s;
    HIP_TRY(node_x2h(f, 0, bufs_x2h(f, 0, f.w.set[0]), f.h, s));
    const float *xc = f.x, *hc = f.h;
    for (int l = 0; l < f.num_layers; ++l) {
        float *hn, *xn;
        HIP_TRY(begin_layer(f, l, hn, xn));
        if (l > 0) HIP_TRY(hipStreamWaitEvent(s, aux->join, 0));       // node stage of this layer (aux stream) done
        HIP_TRY(edge_x2h(f, l, bufs_x2h(f, l, f.w.set[l & 1]), xc, hc, hn));
        if (l + 1 < f.num_layers) {
            HIP_TRY(hipEventRecord(aux->fork, s));
            HIP_TRY(hipStreamWaitEvent(aux->s, aux->fork, 0));
            HIP_TRY(node_x2h(f, l + 1, bufs_x2h(f, l + 1, f.w.set[(l + 1) & 1]), hn, aux->s));
            HIP_TRY(hipEventRecord(aux->join, aux->s));
        }
        HIP_TRY(block_h2x(f, l, f.w.set[2], xc, hn, xn));
        xc = xn;
        hc = hn;
    }
    return CBGX_OK;
}

// one stream, one node-stage buffer set, block after block (profiling, CBGX_OVERLAP=0, no auxiliary stream, first-generation kernels)
static int forward_serial(const Forward& f) {
    const Workspace& w = f.w;
    const NodeBufs& b = w.set[0];
    const float *xc = f.x, *hc = f.h;
    for (int l = 0; l < f.num_layers; ++l) {
        float *hn, *xn;
        HIP_TRY(begin_layer(f, l, hn, xn));
        if (f.dual) {
            HIP_TRY(node_x2h(f, l, bufs_x2h(f, l, b), hc, f.s));
            HIP_TRY(edge_x2h(f, l, bufs_x2h(f, l, b), xc, hc, hn));
        } else {
            const LayerPlan& p = f.plan[l];
            HIP_TRY(launch_attention(true, f.packed + x2h_off(l), f.graph, xc, hc, b, hn, nullptr, p.dst, p.src, f.s));
        }
        HIP_TRY(block_h2x(f, l, b, xc, hn, xn));
        xc = xn;
        hc = hn;
    }
    return CBGX_OK;
}

static int forward_impl(Forward f) {
    if (f.n_nodes < 0 || f.n_graphs < 0 || f.num_layers < 1) return fail(CBGX_E_INVALID, "forward: bad sizes");
    if (f.flags & ~(CBGX_FWD_H_ON_SOURCES | CBGX_FWD_GEN_IS_LIGAND)) return fail(CBGX_E_INVALID, "forward: unknown flags 0x%x", f.flags);
    if (f.num_classes > CBGX_MAX_CLASSES) return fail(CBGX_E_INVALID, "forward: num_classes=%d > %d", f.num_classes, CBGX_MAX_CLASSES);
    if (f.n_nodes == 0) return CBGX_OK;
    if (!f.packed || !f.x || !f.h || !f.graph_ptr || !f.lig_flag || !f.gen_flag || !f.x_out || !f.workspace)
        return fail(CBGX_E_INVALID, "forward: NULL pointer");
    if (f.logits && f.num_classes < 1) return fail(CBGX_E_INVALID, "forward: num_classes=%d", f.num_classes);
    if (int rc = carve_checked("forward", f.workspace, f.workspace_bytes, f.n_nodes, f.w)) return rc;
    f.graph = Graph{f.w.nbr, f.w.deg, f.w.e_w, f.lig_flag, f.gen_flag, f.n_nodes};
    HIP_TRY(hipMemsetAsync(f.w.counters, 0, f.w.counters_bytes, f.s));      // every list count of this call: one fill instead of ~15
    // Static-context cache (optional): static_h1 / static_h2 [N,128] hold the features that leave layer 0 / layer 1 in
    // the ligand-free pocket (rows of ligand atoms unused).  A protein node with no ligand atom among its neighbours sees
    // exactly that pocket in layer 0, so its output is the cached row; the set that differs grows by one hop per layer:
    //   D1 = lig | {i : nbr(i) has a ligand atom},   D2 = D1 | {i : nbr(i) meets D1};   sources S_k = D_k | nbr(D_k).
    // Layers 0 and 1 then run on D1 / D2 only, every other row of their output is a copy of the cache.
    f.cached = f.static_h1 && f.static_h2 && f.num_layers >= 4;
    // with the graph part of the cache, only the nodes that have a ligand atom within reach get a fresh neighbour list
    // and gate: everything else about the pocket's own graph was computed once (same order, same bits)
    f.graph_cached = f.cached && f.static_nbr && f.static_deg && f.static_ew && f.static_r32sq && g_edge_impl != 1;
    // H2X only ever moves gen_flag nodes (x_out = x + dx * gen_flag): they are listed once (`act`), every h2x block runs on the list.
    // Receptive-field pruning (only when the caller does not ask for h_out): the outputs that remain are x_out and the
    // logits of ligand rows, so the last x2h blocks only have to produce features that can still reach them:
    //   A1 = gen | lig | nbr(gen)      destinations of the last x2h (classifier rows, the last h2x's own + source rows)
    //   A2 = A1 | nbr(A1)              its sources = destinations of the x2h before it;   A3 = A2 | nbr(A2) its sources
    // Rows outside these sets are simply not written in the last two feature buffers (and never read).  A1 is built in every
    // call: it is also the set of possible *sources* of an H2X block, so the h2x node projection PS is produced for those rows only.
    // (CBGX_FWD_H_ON_SOURCES: h_out is wanted on A1 only -- the destinations of the last x2h block -- so the same pruning holds)
    f.prune = (f.h_out == nullptr || (f.flags & CBGX_FWD_H_ON_SOURCES)) && f.num_layers >= 3;
    // x2h layers run their (general, protein-only) list pairs (first-generation kernels: one list)
    f.dual = g_edge_impl != 1;
    f.h2x_lig = h2x_lig_selected(f.flags);
    // the step cache serves the large-input schedules of a graph-cached call; elsewhere, and with CBGX_STEP_CACHE=0, the block is not
    // touched and the launches are those of cbgx_unitransformer_forward_cached
    f.step = f.step_block && f.graph_cached && f.dual && f.n_nodes > NODE_STAGE_MAX_ROWS && step_cache_enabled();
    if (f.step) {
        f.sc = carve_step_cache(f.step_block, f.n_nodes);
        if (f.step_block_bytes < f.sc.total)
            return fail(CBGX_E_WORKSPACE, "forward: step cache %zu < %zu", f.step_block_bytes, f.sc.total);
        f.sc.L0.count = f.w.step_count[0];
        f.sc.U1.count = f.w.step_count[1];
    }
    if (int rc = forward_graph_stage(f)) return rc;
    if (int rc = forward_list_stage(f)) return rc;
    plan_layers(f);
    static const bool overlap_env = [] { const char* e = getenv("CBGX_OVERLAP"); return !e || atoi(e) != 0; }();
    AuxStream* aux = (overlap_env && g_edge_impl != 1 && !profile_is_on() && f.num_layers > 1) ? aux_for(f.s) : nullptr;
    // CBGX_FUSE_ROWS: largest input that takes the one-stream fused schedule (0 = never)
    static const int fuse_rows = [] { const char* e = getenv("CBGX_FUSE_ROWS"); return e ? atoi(e) : NODE_STAGE_MAX_ROWS; }();
    int rc;
    if (f.dual && f.num_layers > 1 && f.n_nodes <= fuse_rows && f.n_nodes <= NODE_STAGE_MAX_ROWS) rc = forward_fused(f);
    else if (aux) rc = forward_two_streams(f, aux);
    else rc = forward_serial(f);
    if (rc || !f.logits) return rc;
    // on what the last layer wrote (begin_layer).  Pruned mode: logits are only defined on ligand rows, which are a subset of A1
    return classifier_head(f.packed, f.num_layers, f.num_classes, f.h_out ? f.h_out : f.w.hbuf[(f.num_layers - 1) & 1], f.n_nodes,
                           f.w.set[0].P, f.logits, f.prune ? RowList(f.w.A1) : RowList(), f.s);
}

int cbgx_unitransformer_forward_v2(const float* packed, int num_layers, int num_classes, const float* x, const float* h,
                                   const int32_t* graph_ptr, const uint8_t* lig_flag, const uint8_t* gen_flag,
                                   int n_nodes, int n_graphs, float* x_out, float* h_out, float* logits, unsigned flags,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    return forward_impl(Forward{packed, num_layers, num_classes, x, h, graph_ptr, lig_flag, gen_flag, n_nodes, n_graphs, x_out,
                                h_out, logits, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, flags, workspace, workspace_bytes,
                                (hipStream_t)stream});
}

int cbgx_unitransformer_forward(const float* packed, int num_layers, int num_classes, const float* x, const float* h,
                                const int32_t* graph_ptr, const uint8_t* lig_flag, const uint8_t* gen_flag,
                                int n_nodes, int n_graphs, float* x_out, float* h_out, float* logits, void* workspace,
                                size_t workspace_bytes, void* stream) {
    return cbgx_unitransformer_forward_v2(packed, num_layers, num_classes, x, h, graph_ptr, lig_flag, gen_flag, n_nodes, n_graphs,
                                          x_out, h_out, logits, 0u, workspace, workspace_bytes, stream);
}

int cbgx_unitransformer_forward_cached(const float* packed, int num_layers, int num_classes, const float* x,
                                       const float* h, const int32_t* graph_ptr, const uint8_t* lig_flag,
                                       const uint8_t* gen_flag, int n_nodes, int n_graphs, const float* static_h1,
                                       const float* static_h2, const int32_t* static_nbr, const int32_t* static_deg,
                                       const float* static_ew, const float* static_r32sq, float* x_out, float* h_out,
                                       float* logits, unsigned flags, void* workspace, size_t workspace_bytes, void* stream) {
    if (!static_h1 || !static_h2) return fail(CBGX_E_INVALID, "forward_cached: NULL static context");
    return forward_impl(Forward{packed, num_layers, num_classes, x, h, graph_ptr, lig_flag, gen_flag, n_nodes, n_graphs, x_out,
                                h_out, logits, static_h1, static_h2, static_nbr, static_deg, static_ew, static_r32sq, flags, workspace,
                                workspace_bytes, (hipStream_t)stream});
}

int cbgx_unitransformer_forward_step_cached(const float* packed, int num_layers, int num_classes, const float* x,
                                            const float* h, const int32_t* graph_ptr, const uint8_t* lig_flag,
                                            const uint8_t* gen_flag, int n_nodes, int n_graphs, const float* static_h1,
                                            const float* static_h2, const int32_t* static_nbr, const int32_t* static_deg,
                                            const float* static_ew, const float* static_r32sq, float* x_out, float* h_out,
                                            float* logits, unsigned flags, void* step_cache, size_t step_cache_bytes, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    if (!static_h1 || !static_h2) return fail(CBGX_E_INVALID, "forward_step_cached: NULL static context");
    Forward f{packed, num_layers, num_classes, x, h, graph_ptr, lig_flag, gen_flag, n_nodes, n_graphs, x_out,
              h_out, logits, static_h1, static_h2, static_nbr, static_deg, static_ew, static_r32sq, flags, workspace,
              workspace_bytes, (hipStream_t)stream};
    f.step_block = step_cache;
    f.step_block_bytes = step_cache_bytes;
    return forward_impl(f);
}

size_t cbgx_step_cache_bytes(int n_nodes) {
    if (n_nodes <= NODE_STAGE_MAX_ROWS || !step_cache_enabled()) return 0;      // (no schedule would use it)
    return carve_step_cache(nullptr, n_nodes).total;
}

int cbgx_step_cache_reset(void* step_cache, size_t step_cache_bytes, int n_nodes, void* stream) {
    if (!step_cache || n_nodes < 1) return fail(CBGX_E_INVALID, "step_cache_reset: bad argument");
    const StepCache c = carve_step_cache(step_cache, n_nodes);
    if (step_cache_bytes < c.total) return fail(CBGX_E_WORKSPACE, "step_cache_reset: block %zu < %zu", step_cache_bytes, c.total);
    HIP_TRY(hipMemsetAsync(c.fresh0, 1, 3 * c.flag_stride, (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_step_cache_layout(int n_nodes, size_t* offsets) {
    if (!offsets || n_nodes < 1) return fail(CBGX_E_INVALID, "step_cache_layout: bad argument");
    const StepCache c = carve_step_cache(nullptr, n_nodes);
    const void* p[CBGX_STEP_CACHE_ARRAYS] = {c.P[0], c.q[0], c.hbuf[0], c.P[1], c.q[1], c.hbuf[1], c.fresh0, c.prevD1, c.prevD2};
    for (int k = 0; k < CBGX_STEP_CACHE_ARRAYS; ++k) offsets[k] = (size_t)reinterpret_cast<uintptr_t>(p[k]);     // (carved from NULL)
    return CBGX_OK;
}

// ---- the TargetDiff step entries: the two prologues and the six epilogues fill one aggregate; one check and one launch per kind -------
static int noise_args(const char* who, const uint64_t* keys, const int32_t* lig_graph, bool need_graph, const int32_t* lig_ptr,
                      int n_graphs, int purpose_base) {
    if (!keys || !lig_ptr || (need_graph && !lig_graph)) return fail(CBGX_E_INVALID, "%s: NULL pointer (noise)", who);
    if (n_graphs < 1) return fail(CBGX_E_INVALID, "%s: n_graphs=%d", who, n_graphs);
    if (purpose_base < 0 || purpose_base % CBGX_NOISE_PURPOSE_STRIDE)
        return fail(CBGX_E_INVALID, "%s: purpose_base=%d is not a non-negative multiple of %d", who, purpose_base,
                    CBGX_NOISE_PURPOSE_STRIDE);
    return CBGX_OK;
}

// what an epilogue entry was given (unset: not one of its arguments)
struct StepArgs {
    const char* who = "";       // the entry's short name: what its messages begin with
    // the step: the denoiser's outputs, the ligand atoms' rows in them, the ligand state and where the next one goes, the step index
    const float *x_den = nullptr, *logits = nullptr, *x_lig = nullptr, *c_lig = nullptr;
    const int32_t* lig_rows = nullptr;
    const uint8_t* gen_lig = nullptr;
    int n_lig = 0, num_classes = 0, t = 0, num_timesteps = 0;
    const float* const* tables = nullptr;
    float *x_next = nullptr, *c_next = nullptr;
    int32_t* v_next = nullptr;      // (optional)
    // traj: x_lig / c_lig = x_next / c_next are the bases of the [T+1] slot arrays and the step index lives on the device
    bool traj = false;
    int32_t* t_dev = nullptr;
    // the noise source: the tape pair (noise.eps / u), or the generator's operands (the other fields of `noise`)
    bool counter = false;
    StepNoise noise;
    // boundary: the embedder's ligand rows and the composed arrays that the next denoiser call reads
    bool boundary = false;
    const float *lig_emb_w = nullptr, *lig_emb_b = nullptr, *ind_w = nullptr, *ind_b = nullptr;
    float *x = nullptr, *h = nullptr;
};

// both prologue entries (t_dev: the trajectory one)
static int step_prologue(const char* who, const float* x_lig, const float* c_lig, bool traj, const int32_t* t_dev,
                         const int32_t* lig_rows, int n_lig, int num_classes, const float* lig_emb_w, const float* lig_emb_b,
                         const float* ind_w, const float* ind_b, float* x, float* h, void* stream) {
    if (n_lig == 0) return CBGX_OK;
    if (n_lig < 0 || num_classes < 1 || num_classes > 32) return fail(CBGX_E_INVALID, "%s: bad sizes", who);
    if (!x_lig || !c_lig || (traj && !t_dev) || !lig_rows || !lig_emb_w || !lig_emb_b || !ind_w || !ind_b || !x || !h)
        return fail(CBGX_E_INVALID, "%s: NULL pointer", who);
    HIP_TRY(launch_step_prologue(x_lig, c_lig, lig_rows, n_lig, num_classes, lig_emb_w, lig_emb_b, ind_w, ind_b, x, h,
                                 (hipStream_t)stream, t_dev));
    return CBGX_OK;
}

// the checks of an epilogue entry, none of which touches the device: sizes, NULL pointers, the seven tables, the noise operands
static int step_epilogue_check(const StepArgs& a) {
    if (a.n_lig < 0 || a.num_classes < 1 || a.num_classes > 32 || (!a.traj && (a.t < 0 || a.t >= a.num_timesteps))) {
        if (a.traj) return fail(CBGX_E_INVALID, "%s: bad sizes", a.who);
        return fail(CBGX_E_INVALID, "%s: bad sizes (n_lig=%d C=%d t=%d T=%d)", a.who, a.n_lig, a.num_classes, a.t, a.num_timesteps);
    }
    if (!a.x_den || !a.logits || !a.lig_rows || !a.x_lig || !a.c_lig || !a.gen_lig || !a.tables || !a.x_next || !a.c_next ||
        (a.traj && !a.t_dev) || (!a.counter && (!a.noise.eps || !a.noise.u)) ||
        (a.boundary && (!a.lig_emb_w || !a.lig_emb_b || !a.ind_w || !a.ind_b || !a.x || !a.h)))
        return fail(CBGX_E_INVALID, "%s: NULL pointer", a.who);
    for (int i = 0; i < 7; ++i)
        if (!a.tables[i]) return fail(CBGX_E_INVALID, "%s: table %d is NULL", a.who, i);
    if (a.counter)
        return noise_args(a.who, a.noise.keys, a.noise.lig_graph, true, a.noise.lig_ptr, a.noise.n_graphs, a.noise.purpose_base);
    return CBGX_OK;
}

static int step_epilogue(const StepArgs& a, void* stream) {
    if (a.n_lig == 0) return CBGX_OK;
    if (int rc = step_epilogue_check(a)) return rc;
    const float log_c = (float)log((double)a.num_classes);
    if (a.boundary)
        HIP_TRY(launch_step_boundary(a.x_den, a.logits, a.lig_rows, a.x_lig, a.c_lig, a.gen_lig, a.n_lig, a.num_classes, a.t, a.tables,
                                     log_c, a.noise, a.x_next, a.c_next, a.lig_emb_w, a.lig_emb_b, a.ind_w, a.ind_b, a.x, a.h,
                                     (hipStream_t)stream));
    else
        HIP_TRY(launch_step_epilogue(a.x_den, a.logits, a.lig_rows, a.x_lig, a.c_lig, a.gen_lig, a.n_lig, a.num_classes, a.t, a.tables,
                                     log_c, a.noise, a.x_next, a.c_next, a.v_next, (hipStream_t)stream, a.t_dev));
    return CBGX_OK;
}

int cbgx_targetdiff_prologue(const float* x_lig, const float* c_lig, const int32_t* lig_rows, int n_lig, int num_classes,
                             const float* lig_emb_w, const float* lig_emb_b, const float* ind_w, const float* ind_b,
                             float* x, float* h, void* stream) {
    return step_prologue("prologue", x_lig, c_lig, false, nullptr, lig_rows, n_lig, num_classes, lig_emb_w, lig_emb_b, ind_w, ind_b, x, h,
                         stream);
}

int cbgx_targetdiff_epilogue(const float* x_den, const float* logits, const int32_t* lig_rows, const float* x_lig,
                             const float* c_lig, const uint8_t* gen_lig, int n_lig, int num_classes, int t,
                             int num_timesteps, const float* const* tables, const float* eps, const float* u,
                             float* x_next, float* c_next, int32_t* v_next, void* stream) {
    StepArgs a;
    a.who = "epilogue";
    a.x_den = x_den, a.logits = logits, a.lig_rows = lig_rows, a.x_lig = x_lig, a.c_lig = c_lig, a.gen_lig = gen_lig;
    a.n_lig = n_lig, a.num_classes = num_classes, a.t = t, a.num_timesteps = num_timesteps, a.tables = tables;
    a.noise.eps = eps, a.noise.u = u;
    a.x_next = x_next, a.c_next = c_next, a.v_next = v_next;
    return step_epilogue(a, stream);
}

int cbgx_targetdiff_step_boundary(const float* x_den, const float* logits, const int32_t* lig_rows, const float* x_lig,
                                  const float* c_lig, const uint8_t* gen_lig, int n_lig, int num_classes, int t,
                                  int num_timesteps, const float* const* tables, const float* eps, const float* u,
                                  float* x_next, float* c_next, const float* lig_emb_w, const float* lig_emb_b,
                                  const float* ind_w, const float* ind_b, float* x, float* h, void* stream) {
    StepArgs a;
    a.who = "step_boundary";
    a.x_den = x_den, a.logits = logits, a.lig_rows = lig_rows, a.x_lig = x_lig, a.c_lig = c_lig, a.gen_lig = gen_lig;
    a.n_lig = n_lig, a.num_classes = num_classes, a.t = t, a.num_timesteps = num_timesteps, a.tables = tables;
    a.noise.eps = eps, a.noise.u = u;
    a.x_next = x_next, a.c_next = c_next;
    a.boundary = true, a.lig_emb_w = lig_emb_w, a.lig_emb_b = lig_emb_b, a.ind_w = ind_w, a.ind_b = ind_b, a.x = x, a.h = h;
    return step_epilogue(a, stream);
}

int cbgx_diffbp_epilogue(const float* x_den, const float* x_com, const float* x_in, const float* logits,
                         const int32_t* lig_rows, const int32_t* lig_ptr, const float* x_lig, const float* c_lig,
                         const uint8_t* gen_lig, int n_lig, int n_graphs, int num_classes, int t, int num_timesteps,
                         const float* alphas_cumprod, const float* betas, int absorbing_state, const float* eps,
                         const float* u, float* x_next, float* c_next, void* stream) {
    if (n_lig == 0 || n_graphs == 0) return CBGX_OK;
    if (n_lig < 0 || n_graphs < 0 || num_classes < 1 || num_classes > 32 || t < 0 || t >= num_timesteps ||
        absorbing_state < 0 || absorbing_state >= num_classes)
        return fail(CBGX_E_INVALID, "diffbp_epilogue: bad sizes (n_lig=%d B=%d C=%d t=%d T=%d)", n_lig, n_graphs, num_classes, t,
                    num_timesteps);
    if (!x_den || !x_com || !x_in || !logits || !lig_rows || !lig_ptr || !x_lig || !c_lig || !gen_lig || !alphas_cumprod ||
        !betas || !eps || !u || !x_next || !c_next)
        return fail(CBGX_E_INVALID, "diffbp_epilogue: NULL pointer");
    HIP_TRY(launch_diffbp_epilogue(x_den, x_com, x_in, logits, lig_rows, lig_ptr, x_lig, c_lig, gen_lig, n_graphs, num_classes, t,
                                   num_timesteps, alphas_cumprod, betas, absorbing_state, eps, u, x_next, c_next,
                                   (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_diffsbdd_step(const float* x_den, const float* logits, const int32_t* graph_ptr, const int32_t* lig_rows,
                       const int32_t* lig_ptr, const uint8_t* lig_flag, const float* x_lig, const float* c_lig, int n_lig,
                       int n_graphs, int num_classes, float inv_alpha, float coef, float sigma, int update_positions,
                       int update_types, const float* eps_x, const float* eps_c, const float* lig_emb_w,
                       const float* lig_emb_b, const float* ind_w, const float* ind_b, float* x_next, float* c_next,
                       float* x, float* h, float* shift, float* frame_shift, void* stream) {
    if (n_lig == 0 || n_graphs == 0) return CBGX_OK;
    if (n_lig < 0 || n_graphs < 0 || num_classes < 1 || num_classes > 32)
        return fail(CBGX_E_INVALID, "diffsbdd_step: bad sizes (n_lig=%d B=%d C=%d)", n_lig, n_graphs, num_classes);
    if (!x_den || !logits || !graph_ptr || !lig_rows || !lig_ptr || !lig_flag || !x_lig || !c_lig || !lig_emb_w || !lig_emb_b ||
        !ind_w || !ind_b || !x_next || !c_next || !x || !h || (update_positions && !eps_x) || (update_types && !eps_c))
        return fail(CBGX_E_INVALID, "diffsbdd_step: NULL pointer");
    HIP_TRY(launch_diffsbdd_step(x_den, logits, graph_ptr, lig_rows, lig_ptr, lig_flag, x_lig, c_lig, n_graphs, num_classes,
                                 inv_alpha, coef, sigma, update_positions, update_types, eps_x, eps_c, lig_emb_w, lig_emb_b, ind_w,
                                 ind_b, x_next, c_next, x, h, shift, frame_shift, (hipStream_t)stream));
    return CBGX_OK;
}

// ---- trajectory-resident variants (one captured hipGraph can then be replayed for every step) ---------------------
int cbgx_targetdiff_prologue_traj(const float* traj_x, const float* traj_c, const int32_t* t_dev, const int32_t* lig_rows,
                                  int n_lig, int num_classes, const float* lig_emb_w, const float* lig_emb_b,
                                  const float* ind_w, const float* ind_b, float* x, float* h, void* stream) {
    return step_prologue("prologue_traj", traj_x, traj_c, true, t_dev, lig_rows, n_lig, num_classes, lig_emb_w, lig_emb_b, ind_w, ind_b,
                         x, h, stream);
}

int cbgx_targetdiff_epilogue_traj(const float* x_den, const float* logits, const int32_t* lig_rows, float* traj_x,
                                  float* traj_c, const uint8_t* gen_lig, int n_lig, int num_classes, int32_t* t_dev,
                                  const float* const* tables, const float* eps, const float* u, void* stream) {
    StepArgs a;
    a.who = "epilogue_traj";
    a.x_den = x_den, a.logits = logits, a.lig_rows = lig_rows, a.x_lig = traj_x, a.c_lig = traj_c, a.gen_lig = gen_lig;
    a.n_lig = n_lig, a.num_classes = num_classes, a.tables = tables;
    a.noise.eps = eps, a.noise.u = u;
    a.x_next = traj_x, a.c_next = traj_c;
    a.traj = true, a.t_dev = t_dev;
    return step_epilogue(a, stream);
}

// ---- counter-based noise (rng.h): the fill entry and the TargetDiff step entries that generate in place ------------------------------
int cbgx_noise_fill(const uint64_t* stream_keys, const int32_t* lig_ptr, int n_graphs, int n_lig, int cols, int uniform,
                    int purpose, int step, const int32_t* step_dev, float* out, void* stream) {
    if (n_lig == 0 || n_graphs == 0 || cols == 0) return CBGX_OK;
    if (n_lig < 0 || n_graphs < 0 || cols < 0 || purpose < 0 || (!step_dev && step < 0))
        return fail(CBGX_E_INVALID, "noise_fill: bad sizes (n_lig=%d B=%d cols=%d purpose=%d step=%d)", n_lig, n_graphs, cols, purpose,
                    step);
    if (!stream_keys || !lig_ptr || !out) return fail(CBGX_E_INVALID, "noise_fill: NULL pointer");
    HIP_TRY(launch_noise_fill(stream_keys, lig_ptr, n_graphs, n_lig, cols, uniform, (uint32_t)purpose, step, step_dev, out,
                              (hipStream_t)stream));
    return CBGX_OK;
}

int cbgx_targetdiff_epilogue_rng(const float* x_den, const float* logits, const int32_t* lig_rows, const float* x_lig,
                                 const float* c_lig, const uint8_t* gen_lig, int n_lig, int num_classes, int t,
                                 int num_timesteps, const float* const* tables, const uint64_t* stream_keys,
                                 const int32_t* lig_graph, const int32_t* lig_ptr, int n_graphs, int purpose_base, float* x_next,
                                 float* c_next, int32_t* v_next, void* stream) {
    StepArgs a;
    a.who = "epilogue_rng";
    a.x_den = x_den, a.logits = logits, a.lig_rows = lig_rows, a.x_lig = x_lig, a.c_lig = c_lig, a.gen_lig = gen_lig;
    a.n_lig = n_lig, a.num_classes = num_classes, a.t = t, a.num_timesteps = num_timesteps, a.tables = tables;
    a.counter = true, a.noise.keys = stream_keys, a.noise.lig_graph = lig_graph, a.noise.lig_ptr = lig_ptr;
    a.noise.n_graphs = n_graphs, a.noise.purpose_base = purpose_base;
    a.x_next = x_next, a.c_next = c_next, a.v_next = v_next;
    return step_epilogue(a, stream);
}

int cbgx_targetdiff_step_boundary_rng(const float* x_den, const float* logits, const int32_t* lig_rows, const float* x_lig,
                                      const float* c_lig, const uint8_t* gen_lig, int n_lig, int num_classes, int t,
                                      int num_timesteps, const float* const* tables, const uint64_t* stream_keys,
                                      const int32_t* lig_graph, const int32_t* lig_ptr, int n_graphs, int purpose_base,
                                      float* x_next, float* c_next, const float* lig_emb_w, const float* lig_emb_b,
                                      const float* ind_w, const float* ind_b, float* x, float* h, void* stream) {
    StepArgs a;
    a.who = "step_boundary_rng";
    a.x_den = x_den, a.logits = logits, a.lig_rows = lig_rows, a.x_lig = x_lig, a.c_lig = c_lig, a.gen_lig = gen_lig;
    a.n_lig = n_lig, a.num_classes = num_classes, a.t = t, a.num_timesteps = num_timesteps, a.tables = tables;
    a.counter = true, a.noise.keys = stream_keys, a.noise.lig_graph = lig_graph, a.noise.lig_ptr = lig_ptr;
    a.noise.n_graphs = n_graphs, a.noise.purpose_base = purpose_base;
    a.x_next = x_next, a.c_next = c_next;
    a.boundary = true, a.lig_emb_w = lig_emb_w, a.lig_emb_b = lig_emb_b, a.ind_w = ind_w, a.ind_b = ind_b, a.x = x, a.h = h;
    return step_epilogue(a, stream);
}

int cbgx_targetdiff_epilogue_traj_rng(const float* x_den, const float* logits, const int32_t* lig_rows, float* traj_x,
                                      float* traj_c, const uint8_t* gen_lig, int n_lig, int num_classes, int32_t* t_dev,
                                      const float* const* tables, const uint64_t* stream_keys, const int32_t* lig_graph,
                                      const int32_t* lig_ptr, int n_graphs, int purpose_base, void* stream) {
    StepArgs a;
    a.who = "epilogue_traj_rng";
    a.x_den = x_den, a.logits = logits, a.lig_rows = lig_rows, a.x_lig = traj_x, a.c_lig = traj_c, a.gen_lig = gen_lig;
    a.n_lig = n_lig, a.num_classes = num_classes, a.tables = tables;
    a.counter = true, a.noise.keys = stream_keys, a.noise.lig_graph = lig_graph, a.noise.lig_ptr = lig_ptr;
    a.noise.n_graphs = n_graphs, a.noise.purpose_base = purpose_base;
    a.x_next = traj_x, a.c_next = traj_c;
    a.traj = true, a.t_dev = t_dev;
    return step_epilogue(a, stream);
}

}  // extern "C"

// libcbgx -- the body of the fused x2h / h2x edge kernels, shared by the translation units that instantiate it: edge_mfma.hip
// (exact-fp32 scores and aggregation, v_mfma_f32_16x16x4_f32) and edge_x2h_f16.hip (the same two contractions in split-f16
// arithmetic on the f16 matrix pipe, template flag F16), and edge_h2x_lig.hip (h2x on ligand rows with the query folded in registers,
// template flag HL).  The including file defines `c_mu` (the rbf centres, __constant__) in
// namespace cbgx before this header.  See edge_mfma.hip for the algebra, the lane mappings and the memory pipeline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edge_common.h"
#include "layout.h"

// Waves of a persistent workgroup that take items.  A launch whose item list is short next to the grid (one graph: 445 nodes, an
// h2x block: the ~25 movable atoms per graph) is ONE node's dependent chain per wave -- 18 - 20 us of a 27 us launch
// (profiles/probe_r04z2.log) -- and two such chains on one SIMD slow each other down.  So a workgroup puts only as many of its
// WAVES waves to work as the list needs, but at least CBGX_EDGE_MIN_WAVES = 2 (each on its own SIMD), and the launchers size the grid
// for that many nodes per workgroup: the other waves help fill the LDS image and leave.  Decided per launch from the DEVICE-side list length,
// so cached / pruned / listed launches of a large batch get it too (the ~250 movable atoms of a 10-graph batch).  Same arithmetic per
// node whatever the schedule.  History: round 4 prepared this as a host-side switch (-DCBGX_EDGE_SMALL_W4, 4-wave workgroups for
// inputs of <= 1016 nodes) next to a dynamic remainder of the persistent loop (-DCBGX_EDGE_DYN); round 5's first GPU call measured
// both (profiles/small_dyn_r05a.log): 4 waves 1 167 -> 1 328 graph-steps/s at one graph (edge launches 26.8 -> 21.0 us), the dynamic
// remainder 9 116 -> 8 278 at ten graphs (x2h launch 52.8 -> 71.4 us) and nothing on the headline or the training line -- deleted.
// Second GPU call (profiles/small_r05b.log, fused node stage in every row): at least 8 / 4 / 2 waves per workgroup = 1 362 / 1 680 /
// 1 796 graph-steps/s at one graph (x2h launch 26.9 / 20.7 / 17.9 us), 9 773 / 10 647 / 10 924 at ten; the headline does not move.
#ifndef CBGX_EDGE_MIN_WAVES
#define CBGX_EDGE_MIN_WAVES 2
#endif
// Which wave of which workgroup takes item o of a round (S = workgroups x active waves items per round).  0: workgroup-major, o =
// slot * waves + wave (rounds 1 - 4) -- a partial last round then fills ALL waves of its first few workgroups while the others idle:
// a 10-graph batch is 2.17 nodes per wave, and the 48 third-round items of an XCD sat on 6 of its 32 workgroups, two to a SIMD.
// 1: wave-major, o = wave * slots + slot -- the same items go to wave 0 of every workgroup first, one to a SIMD, where a node's
// chain runs ~1.5 x faster (the waves-per-workgroup measurements above).  Full rounds are the same load either way.
// 1: the protein-only role's query channels are requested before the wait for the node's rows, and the x2h epilogue's residual row /
// bias before the v path (ahead of the next item's row prefetch) instead of right before the epilogue.  (A/B knob; 0 = rounds 2 - 4.)
#ifndef CBGX_EDGE_EARLY_HEADER
#define CBGX_EDGE_EARLY_HEADER 1     // the first item's header travels with the LDS fill (0: requested after its barrier, as until round 5)
#endif
#ifndef CBGX_EDGE_EARLY_LOADS
#define CBGX_EDGE_EARLY_LOADS 1
#endif
#ifndef CBGX_EDGE_WAVE_MAJOR
#define CBGX_EDGE_WAVE_MAJOR 1
#endif

namespace cbgx {

// waves of a WAVES-wave workgroup that take items when `n_items` items are shared by `n_wg` workgroups (wave-uniform; the same
// formula sizes the roles of edge_x2h_dual_kernel and is restated in tests/test_bx_partition.py)
constexpr int EDGE_MIN_WAVES = CBGX_EDGE_MIN_WAVES;
__host__ __device__ __forceinline__ int edge_active_waves(int n_items, int n_wg, int waves) {
    const int per_wg = (n_items + n_wg - 1) / (n_wg > 0 ? n_wg : 1);
    const int lo = EDGE_MIN_WAVES < waves ? EDGE_MIN_WAVES : waves;
    return per_wg < lo ? lo : (per_wg > waves ? waves : per_wg);
}
// (launchers) the edge kernels address P with 32-bit byte offsets
static inline bool edge_offsets_fit(int n_nodes) { return (size_t)n_nodes * PROW * sizeof(float) < (1ull << 32); }
// (launchers) persistent grid of a one-role edge launch: sized for EDGE_MIN_WAVES nodes per workgroup -- a short list spreads over more
// CUs with one wave per SIMD (edge_active_waves) -- at most one workgroup per CU (LDS-limited) or `wg_limit` (>= 8: the caller keeps
// CUs free for another stream), and a multiple of 8 from 64 on -> XCD-aware node partition
static inline int edge_persistent_grid(int n_nodes, int wg_limit = 0) {
    int grid = (n_nodes + EDGE_MIN_WAVES - 1) / EDGE_MIN_WAVES;
    if (grid > 256) grid = 256;
    if (wg_limit >= 8 && grid > wg_limit) grid = wg_limit;
    if (grid >= 64) grid &= ~7;
    return grid;
}

// ---- edge-major path for one half (16 edges): pre-activation -> LayerNorm -> ReLU -> contraction with a
// per-lane row of B (Qt[i][a] for scores: registers `pre`; Wbv[a] for the h2x values: LDS `lds_brow`, already lane-offset).  Returns the 16x16 result tile:
// lane (c = a, q), reg r <-> edge 4q + r + 16hf.  `kv` selects the k (0) or v (1) quarter everywhere.
// `acc` enters as PD[i] + PS[j] (this node's and the neighbour's projection rows, channels 16t + 4q .. +3), summed by
// the caller as soon as the gathered rows arrive, so that the registers of the gather can be reused for the next one.
// FOLD (protein-only x2h kernel, first k half): `pre` is an OUTPUT here -- the folded query row Qt[i][a = c][16 t + 4 q ..] is
// computed from the node's eight query channels of head c (`q8`) and the fold table in LDS (layout.h PP_WFOLD) between the rbf MFMA
// block and the LayerNorm tail, i.e. after the q row has had a whole MFMA block to arrive: Qt never exists in memory.
// QS (x2h scores in split-f16, edge_x2h_f16.hip): 0 = exact fp32 (16x16x4 MFMAs, everything above).  1, 2 = the contraction runs as
// v_mfma_f32_16x16x16_f16, one K = 16 step per tile: A element j of lane (c = edge, q) = hid[16 t + 4 q + j] -- the four values the
// lane holds in acc[t] -- and B element j of lane (c = head, q) = the query row at the same channel, three products
// hi hi + lo hi + hi lo per tile; the operands are split and kept per tile PAIR (eight values: one register quad of f16 pairs).  `hid` arrives scaled by 2^kh (the caller has scaled the LayerNorm affine in LDS; ReLU
// commutes with a positive factor), the query row is scaled here by a power of two from its own maximum (zero row: 1); both put the
// largest value into [2^14, 2^15) and are undone in fp32 on the result: `*qun` = 2^-kq 2^-kh.  QS = 1 splits the query row and leaves
// the f16 pieces in `pre` (pre[t] = hi, pre[t + 1] = lo of the pair, as bits), QS = 2 (the node's second half) finds them there.
template <bool PRE, bool FOLD = false, int QS = 0>
__device__ __forceinline__ floatx4 edge_major_half(floatx4 (&acc)[8], bool lg, int kv,
                                                   const float* lds_frag, const float* lds_dwt, const float* lds_ln,
                                                   const float (&R)[5], bool has_prot, bool has_lig, int lig_i,
                                                   int lane, int q, const float* lds_brow,
                                                   float4 (&pre)[8], const RbfScale sc,
                                                   const float4 q8a = float4{0.f, 0.f, 0.f, 0.f},
                                                   const float4 q8b = float4{0.f, 0.f, 0.f, 0.f},
                                                   const float kh_inv = 1.f, float* qun = nullptr) {
    if (has_lig) {  // wave-uniform: only nodes with a ligand neighbour pay for the type correction
        const float* dw = lds_dwt + lig_i * 2 * H + kv * H + 4 * q;
        const float m = lg ? sc.S : 0.f;     // the tile is carried scaled by S (edge_common.h RbfScale)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] += f4(ld4(dw + 16 * t)) * m;
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (p == 0 ? !has_prot : !has_lig) continue;  // wave-uniform
        float Rm[5];
#pragma unroll
        for (int s = 0; s < 5; ++s) Rm[s] = (lg == (p == 1)) ? R[s] : 0.f;
        // split-f16 on the f16 matrix pipe, weight tuples as the A operand; two tiles at a time
        half4 B[4];
        rbf_tuples(Rm, B);
        const float* fa = lds_frag + (size_t)etype(p == 1, lig_i) * (8 * FRAG_BLK);
#pragma unroll
        for (int tg = 0; tg < 8; tg += 2) {
            const WTuples w0 = load_wtuples(fa, tg, lane), w1 = load_wtuples(fa, tg + 1, lane);
            acc[tg] = MFMAH(w0.t1, B[0], acc[tg]);         acc[tg + 1] = MFMAH(w1.t1, B[0], acc[tg + 1]);
            acc[tg] = MFMAH(w0.t1, B[1], acc[tg]);         acc[tg + 1] = MFMAH(w1.t1, B[1], acc[tg + 1]);
            acc[tg] = MFMAH(w0.t2, B[2], acc[tg]);         acc[tg + 1] = MFMAH(w1.t2, B[2], acc[tg + 1]);
            acc[tg] = MFMAH(w0.t3, B[3], acc[tg]);         acc[tg + 1] = MFMAH(w1.t3, B[3], acc[tg + 1]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);  // keep the tail's operand loads (g, b, B row) below the MFMA block
    if (FOLD) {
        // Qt[c][16 t + 4 q + r] = sum_d q[8 c + d] Wbk[8 c + d][16 t + 4 q + r] / sqrt(8): 64 conflict-free ds_read_b128 and 128
        // packed FMAs per node instead of 8 KB of Qt written by node_qfold_kernel and read back here
        const float qd[8] = {q8a.x, q8a.y, q8a.z, q8a.w, q8b.x, q8b.y, q8b.z, q8b.w};
        const float* wf = lds_brow;     // fold table, already lane-offset: (t, d) at 2048 t + 256 d floats
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            float2v lo = {0.f, 0.f}, hi = {0.f, 0.f};
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const floatx4 w4 = f4(ld4(wf + 2048 * t + 256 * d));
                const float2v qq = splat2(qd[d]);
                lo = lo2(w4) * qq + lo;
                hi = hi2(w4) * qq + hi;
            }
            pre[t] = make_float4(lo.x, lo.y, hi.x, hi.y);
        }
    }
    // LayerNorm: the first Linear is centred, so mean(pre) == 0 and var = mean(pre^2)
    float2v v2 = {0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        v2 = lo2(acc[t]) * lo2(acc[t]) + v2;
        v2 = hi2(acc[t]) * hi2(acc[t]) + v2;
    }
    const float v = xrow_sum(v2.x + v2.y);
    const float rstd = fast_rsqrt(__builtin_fmaf(v, sc.c1, 1e-5f)) * sc.c2;
    const float2v r2 = splat2(rstd);
    const float* lg_ = lds_ln + (2 * kv) * H + 4 * q;
    const float* lb_ = lds_ln + (2 * kv + 1) * H + 4 * q;
    // two interleaved accumulators: a dependent 16x16x4 MFMA needs 40 cycles, an independent one 32
    floatx4 out0 = {0.f, 0.f, 0.f, 0.f}, out1 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (QS != 0) {
        static_assert(PRE, "the split-f16 contraction is the x2h score path");
        if constexpr (QS == 1) {
            float m = 0.f;
#pragma unroll
            for (int t = 0; t < 8; ++t)
                m = fmaxf(fmaxf(m, fmaxf(fabsf(pre[t].x), fabsf(pre[t].y))), fmaxf(fabsf(pre[t].z), fabsf(pre[t].w)));
            m = xrow_max(m);                                        // head c's row maximum, in all four lanes that hold the row
            const int kq = split_exponent(m, true);
            const float up = pow2_scale(kq);
            *qun = pow2_scale(-kq) * kh_inv;
#pragma unroll
            for (int t = 0; t < 8; t += 2) {
                half8 hi, lo;
                split_f16x8(f4(pre[t]) * up, f4(pre[t + 1]) * up, hi, lo);
                pre[t] = __builtin_bit_cast(float4, hi);
                pre[t + 1] = __builtin_bit_cast(float4, lo);
            }
        }
#pragma unroll
        for (int t = 0; t < 8; t += 2) {
            floatx4 y[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const floatx4 g = f4(ld4(lg_ + 16 * (t + u))), b = f4(ld4(lb_ + 16 * (t + u)));
                const float2v ya = (lo2(acc[t + u]) * r2) * lo2(g) + lo2(b);
                const float2v yb = (hi2(acc[t + u]) * r2) * hi2(g) + hi2(b);
                y[u] = floatx4{fmaxf(ya.x, 0.f), fmaxf(ya.y, 0.f), fmaxf(yb.x, 0.f), fmaxf(yb.y, 0.f)};
            }
            half8 ah, al;
            split_f16x8(y[0], y[1], ah, al);
            const half8 bh = __builtin_bit_cast(half8, pre[t]), bl = __builtin_bit_cast(half8, pre[t + 1]);
            // K = 16 steps, one per tile (tile t -> out0, tile t + 1 -> out1): the K = 32 form of the same products
            // (v_mfma_f32_16x16x32_f16, one step per pair) gave results that differed between identical launches -- one node in
            // ~10^5 off by 1e-3 of |h| -- on the MI355X, with nothing else changed; this form is bit-reproducible
            const half4 ah0 = __builtin_shufflevector(ah, ah, 0, 1, 2, 3), ah1 = __builtin_shufflevector(ah, ah, 4, 5, 6, 7);
            const half4 al0 = __builtin_shufflevector(al, al, 0, 1, 2, 3), al1 = __builtin_shufflevector(al, al, 4, 5, 6, 7);
            const half4 bh0 = __builtin_shufflevector(bh, bh, 0, 1, 2, 3), bh1 = __builtin_shufflevector(bh, bh, 4, 5, 6, 7);
            const half4 bl0 = __builtin_shufflevector(bl, bl, 0, 1, 2, 3), bl1 = __builtin_shufflevector(bl, bl, 4, 5, 6, 7);
            out0 = MFMAH(ah0, bh0, out0); out1 = MFMAH(ah1, bh1, out1);
            out0 = MFMAH(al0, bh0, out0); out1 = MFMAH(al1, bh1, out1);
            out0 = MFMAH(ah0, bl0, out0); out1 = MFMAH(ah1, bl1, out1);
        }
        return (out0 + out1) * *qun;
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const floatx4 g = f4(ld4(lg_ + 16 * t)), b = f4(ld4(lb_ + 16 * t));
        const float2v ya = (lo2(acc[t]) * r2) * lo2(g) + lo2(b);
        const float2v yb = (hi2(acc[t]) * r2) * hi2(g) + hi2(b);
        const float4 bb = PRE ? pre[t] : ld4(lds_brow + 256 * t);    // h2x: Wbv[head c][16 t + 4 q ..] (layout.h, image "wbv")
        out0 = MFMA(fmaxf(ya.x, 0.f), bb.x, out0);
        out1 = MFMA(fmaxf(ya.y, 0.f), bb.y, out1);
        out0 = MFMA(fmaxf(yb.x, 0.f), bb.z, out0);
        out1 = MFMA(fmaxf(yb.y, 0.f), bb.w, out1);
    }
    return out0 + out1;
}

// Geometry of one work item in the two lane mappings the kernel uses:
//   E0: lane (c, q) <-> edges c and c + 16 (distances, rbf, edge-major tiles);  E1: lane (c, q) <-> edges 4q + r (+16)
// Invalid slots (e >= deg) point at the node itself, so every gather below is unconditional: a predicated load compiles
// to branch + load + wait per element, which is what used to serialise the memory latencies of a node.
struct ItemGeom {
    int node, d, lig_i;
    float xi, yi, zi;
    int j0[2];          // E0 neighbour ids
};
// E1 neighbour id of slot r of a half: the raw row entry (-1 padded) or the node itself
__device__ __forceinline__ int e1_id(int raw, int e, int d, int self) { return e < d ? raw : self; }

// LISTED: the launch iterates over a device-side node list (h2x always; x2h in the pruned last layers) -- a separate
// instantiation so that profilers report full-graph and listed launches under different kernel names.
//
// Memory pipeline of one iteration (every gather has at least one MFMA block between its issue and its first use):
//   previous iteration   ids / flags / coordinates of this node and its neighbours; PD[i], PS_k[j] rows (issued before
//                        that node's epilogue)
//   top                  both halves' PD + PS_k summed (frees the 24 gather registers); then Qt[i] rows, PS_v gathers of
//                        half 0 (x2h), ids of the next node (a)
//   after k half 0       PS_v gathers of half 1 (x2h), e_w; coordinates / flags of the next node's neighbours (b)
//   after k half 1       distances / flags of the next node's edges
//   before the epilogue  PD / PS_k rows of the next node (c)
// PP (x2h, listed): the protein-only specialisation -- every listed destination and all of its neighbours are protein atoms (the
// launcher's list guarantees it), so only the type-3 rbf tables are needed and the LDS image (layout.h A_IMG_PP) carries the second
// k Linear instead of the other three types: the query fold happens in registers, `Qt` is then the UNFOLDED query q[N,128].
// The body is a device function over (`wg`, `n_wg`) = this workgroup's index and the number of workgroups that share the item list:
// the plain kernels pass blockIdx.x / gridDim.x, the two-role x2h kernel (edge_x2h_dual_kernel) gives each role its own range.
// `lds` [IMG floats], `lds_mu` [G floats]: the calling kernel's shared arrays.
// F16 (x2h, edge_x2h_f16.hip): scores and aggregation in split-f16 on the f16 matrix pipe (edge_major_half QS; the aggregation
// below) instead of exact-fp32 16x16x4 MFMAs.  Once per launch the workgroup scales the LayerNorm affine of both paths in its LDS
// image by 2^kh, kh from the bound sqrt(127) max|gamma| + max|beta| of a LayerNorm output (split_exponent): the hidden activations
// then leave LayerNorm + ReLU with their largest possible value in [2^14, 2^15) at no per-node cost.
// HL (h2x, listed, edge_h2x_lig.hip): the ligand-row specialisation -- every listed destination is a ligand atom (the caller's promise,
// CBGX_FWD_GEN_IS_LIGAND), so lig_i = 1, only edge types 0 and 2 occur and the LDS image (layout.h A_IMG_H2L) carries the second k Linear
// next to the 16 rows of the second v Linear: the query is folded in k half 0 as in PP, `Qt` is the UNFOLDED query q[N,128].
template <bool X2H, int WAVES, bool LISTED, bool PP, bool F16 = false, bool HL = false>
__device__ __forceinline__ void edge_body(
    float* __restrict__ lds, float* __restrict__ lds_mu, const int wg, const int n_wg,
    const float* __restrict__ att, const float* __restrict__ x, const float* __restrict__ h,
    const float* __restrict__ P, const float* __restrict__ Qt, const int32_t* __restrict__ nbr,
    const int32_t* __restrict__ deg, const uint8_t* __restrict__ lig, const uint8_t* __restrict__ gen,
    const float* __restrict__ e_w, int n_nodes, float* __restrict__ out, float* __restrict__ dx_out,
    const int* __restrict__ act_arg, const int* __restrict__ act_count) {
    const int* __restrict__ act = LISTED ? act_arg : nullptr;
    static_assert(!PP || (X2H && LISTED), "the protein-only kernel is an x2h work-list kernel");
    static_assert(!F16 || X2H, "split-f16 scores and aggregation: x2h only");
    static_assert(!HL || (!X2H && LISTED && !PP), "the ligand-row kernel is an h2x work-list kernel");
    static_assert(PP_IMG_SIZE == IMG_SIZE_X2H, "both x2h images fill the same LDS array");
    constexpr int IMG = X2H ? (int)IMG_SIZE_X2H : (HL ? (int)H2L_IMG_SIZE : (int)IMG_SIZE_H2X);
    // work list mode of h2x: x_out = x for every node that cannot move -- by all workgroups, also those without an item.  The
    // flag and the position are requested together (one round trip, not two), and a workgroup with items does this behind its
    // LDS fill's loads instead of in front of them.
    auto copy_fixed_nodes = [&]() {
        if (!X2H && act) {
            for (int n = wg * (WAVES * 64) + threadIdx.x; n < n_nodes; n += n_wg * WAVES * 64) {
                unsigned gn = gen[n];
                float px = x[3 * n], py = x[3 * n + 1], pz = x[3 * n + 2];
                asm volatile("" : "+v"(gn), "+v"(px), "+v"(py), "+v"(pz));      // (otherwise the position load sinks into the `if`)
                if (!gn) {
                    out[3 * n] = px; out[3 * n + 1] = py; out[3 * n + 2] = pz;
                    if (dx_out) { dx_out[3 * n] = 0.f; dx_out[3 * n + 1] = 0.f; dx_out[3 * n + 2] = 0.f; }
                }
            }
        }
    };
    const int n_items = act ? *act_count : n_nodes;
    const int wv = edge_active_waves(n_items, n_wg, WAVES);     // waves of this workgroup that take items (see CBGX_EDGE_MIN_WAVES)
    {   // a workgroup with no item skips the LDS fill altogether (its wave 0 holds its first item in either mapping)
        int first;
        if ((n_wg & 7) == 0) {
            const int per_xcd = (((n_items + 7) >> 3) + wv - 1) / wv * wv;
            first = (wg & 7) * per_xcd + (wg >> 3) * (CBGX_EDGE_WAVE_MAJOR ? 1 : wv);
            if (first >= min(n_items, ((int)(wg & 7) + 1) * per_xcd)) { copy_fixed_nodes(); return; }
        } else {
            first = wg * (CBGX_EDGE_WAVE_MAJOR ? 1 : wv);
            if (first >= n_items) { copy_fixed_nodes(); return; }
        }
    }
    // the wave index -- and with it every node index of the persistent loop -- lives in scalar registers: node-level values
    // (degree, flag, position, row bases) are then scalar loads and SGPR operands instead of 64 identical lanes
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 15, q = lane >> 4;

    // XCD-aware persistent schedule: workgroup b runs on XCD b % 8 (observed dispatch order), so give every
    // XCD one contiguous eighth of the item range: a graph's PS / Qt rows are then pulled into one L2 only.  (A role of the
    // two-role kernel starts at a multiple of 8, so wg % 8 is still the XCD.)
    int i_begin, i_end, i_step;
    if ((n_wg & 7) == 0) {
        const int per_xcd = (((n_items + 7) >> 3) + wv - 1) / wv * wv;
        const int xcd = wg & 7, slot = wg >> 3, slots = n_wg >> 3;
        i_begin = xcd * per_xcd + (CBGX_EDGE_WAVE_MAJOR ? wave * slots + slot : slot * wv + wave);
        i_end = min(n_items, (xcd + 1) * per_xcd);
        i_step = slots * wv;
    } else {
        i_begin = CBGX_EDGE_WAVE_MAJOR ? wave * n_wg + wg : wg * wv + wave;
        i_end = n_items;
        i_step = n_wg * wv;
    }
    const bool has_item = wave < wv && i_begin < i_end;      // wave-uniform
    // The first item's header -- list entry -> node -> degree, class, position, neighbour row: two dependent round trips -- is
    // requested BEFORE the LDS fill and travels with it (CBGX_EDGE_EARLY_HEADER): behind the fill's barrier it opened every launch,
    // ~1.4 us of the ~8 us a small input's launch works (27 launches per denoising step).
    ItemGeom g;
    int r0 = 0, r1 = 0;
    int4 nb0 = {0, 0, 0, 0}, nb1 = {0, 0, 0, 0};      // the node's neighbour row in the E1 mapping (raw, -1 padded)
    int lig_first = 0;      // (raw: made wave-uniform after the barrier, so that nothing here waits for it)
    auto first_header = [&]() {
        const int i = __builtin_amdgcn_readfirstlane(act ? act[i_begin] : i_begin);
        g.node = i;
        g.d = deg[i]; lig_first = PP ? 0 : (HL ? 1 : lig[i]);
        g.xi = x[3 * i]; g.yi = x[3 * i + 1]; g.zi = x[3 * i + 2];
        const gptr nrow = sbase(nbr + (size_t)i * KNN);
        const unsigned oc = vop(4 * c), oq = vop(16 * q);
        r0 = ldoi(nrow, oc); r1 = ldoi(nrow, oc + 64);
        nb0 = ldoi4(nrow, oq); nb1 = ldoi4(nrow, oq + 64);
    };
    {
        // LDS fill: every load of the thread is requested before the first is written (19 float4 per thread for the x2h image).
        // Left as a plain loop the compiler emits load -> wait -> ds_write per iteration: 19 dependent L2 round trips, ~25 us at
        // the head of EVERY launch -- the whole duration of a small one (a 1-graph step is 18 such launches).
        const floatx4* src = reinterpret_cast<const floatx4*>(att + (PP ? A_IMG_PP : (HL ? A_IMG_H2L : A_IMG)));
        floatx4* dst = reinterpret_cast<floatx4*>(lds);
        constexpr int NV = (IMG / 4 + WAVES * 64 - 1) / (WAVES * 64);
        if constexpr (WAVES >= 8) {
            floatx4 v[NV];
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                const int t = threadIdx.x + u * (WAVES * 64);
                v[u] = src[t < IMG / 4 ? t : IMG / 4 - 1];
            }
            __builtin_amdgcn_sched_barrier(0);
            if (CBGX_EDGE_EARLY_HEADER && has_item) first_header();      // behind the fill's loads, ahead of its writes
            copy_fixed_nodes();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                const int t = threadIdx.x + u * (WAVES * 64);
                if (t < IMG / 4) dst[t] = v[u];
            }
        } else {
            if (CBGX_EDGE_EARLY_HEADER && has_item) first_header();
            copy_fixed_nodes();        // fewer threads: the same in passes of at most 20 float4 per thread (38 at once would not fit the registers)
            constexpr int NVC = 20;
#pragma unroll 1
            for (int u0 = 0; u0 < NV; u0 += NVC) {
                floatx4 v[NVC];
#pragma unroll
                for (int u = 0; u < NVC; ++u) {
                    const int t = threadIdx.x + (u0 + u) * (WAVES * 64);
                    v[u] = src[t < IMG / 4 ? t : IMG / 4 - 1];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < NVC; ++u) {
                    const int t = threadIdx.x + (u0 + u) * (WAVES * 64);
                    if (t < IMG / 4) dst[t] = v[u];
                }
            }
        }
        if (threadIdx.x < G) lds_mu[threadIdx.x] = c_mu[threadIdx.x];
    }
    __syncthreads();
    float khk_inv = 1.f, s2_un = 1.f;       // F16: 2^-kh of the k path; 2^-kh 2^-14 of the v path (the aggregation weights carry 2^14)
    if constexpr (F16) {
        float* ln = lds + (PP ? PP_LN : IMG_LN);        // [gamma_k | beta_k | gamma_v | beta_v][128]: eight values per lane, every wave
        const int l8 = 8 * (threadIdx.x & 63);
        const float4 a = ld4(ln + l8), b = ld4(ln + l8 + 4);
        float m = fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))),
                        fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w))));
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        auto row_value = [&](int l) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(m), l)); };
        const float gk = row_value(0), bk = row_value(16), gv = row_value(32), bv = row_value(48);
        const int khk = split_exponent(__builtin_fmaf(LN_OUT_MAX, gk, bk), false), khv = split_exponent(__builtin_fmaf(LN_OUT_MAX, gv, bv), false);
        khk_inv = pow2_scale(-khk);
        s2_un = pow2_scale(-khv) * (1.f / W_UP);
        __syncthreads();                                // every wave has read the unscaled affine
        for (int t = threadIdx.x; t < 4 * H; t += WAVES * 64) ln[t] *= pow2_scale(t < 2 * H ? khk : khv);
        __syncthreads();
    }
    // PP: the tables of edge type 3 sit at the head of the image; the table bases are biased so that etype() = 3 indexes them
    // HL: slots [k type 0 | v type 0 | k type 2 | v type 2]: etype() = 0 / 2 from a k base at slot 0 and a v base at slot 1; the dwt
    // base is biased so that lig_i = 1 indexes the image's only pair of rows
    const float* lds_fk = PP ? lds + PP_FRAG_K - 3 * 8 * (int)FRAG_BLK : (HL ? lds + H2L_FRAG : lds + IMG_FRAG_K);
    const float* lds_fv = PP ? lds + PP_FRAG_V - 3 * 8 * (int)FRAG_BLK : (HL ? lds + H2L_FRAG + 8 * (int)FRAG_BLK : lds + IMG_FRAG_V);
    const float* lds_dwt = HL ? lds + H2L_WT - 2 * H : lds + IMG_WT;     // (never read by PP: no ligand source)
    const float* lds_ln = lds + (PP ? PP_LN : (HL ? H2L_LN : IMG_LN));

    if (!has_item) return;     // (after the barrier: this wave has done its share of the LDS fill)
    if (!CBGX_EDGE_EARLY_HEADER) first_header();
    g.lig_i = __builtin_amdgcn_readfirstlane(lig_first);
    // power-of-two scales of the split-f16 rbf tables (wave-uniform: scalar registers)
    const RbfScale sck = load_rbf_scale(att, 0), scv = load_rbf_scale(att, 1);
    // h2x: bias of this lane's head, once per launch -- loaded inside the loop it sat behind the next node's 24-row prefetch in the
    // in-order vmcnt queue, so the wait for this one word drained the whole prefetch before the node's store
    const float bbv = X2H ? 0.f : att[A_BBV + c];

    // ---- first item: geometry and the k-path rows, everything unconditional -------------------------------------
    bool lg0[2];
    float dist0[2];
    float4 pd[8], ps0[8], ps1[8];
    {
        const int i = g.node;
        const unsigned oq = vop(16 * q);
        g.j0[0] = c < g.d ? r0 : i;
        g.j0[1] = c + 16 < g.d ? r1 : i;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int j = g.j0[hf];
            const int lj = PP ? 0 : ldob(sbase(lig), (unsigned)j);
            lg0[hf] = (c + 16 * hf < g.d) && lj;
            dist0[hf] = edge_len(g.xi, g.yi, g.zi, ldo1(sbase(x), 12u * j), ldo1(sbase(x), 12u * j + 4), ldo1(sbase(x), 12u * j + 8));
        }
        const gptr pdp = sbase(P + (size_t)i * PROW);
        const unsigned o0 = (unsigned)g.j0[0] * (PROW * 4) + (2 * H + 4 * q) * 4, o1 = (unsigned)g.j0[1] * (PROW * 4) + (2 * H + 4 * q) * 4;
#pragma unroll
        for (int t = 0; t < 8; ++t) { pd[t] = ldo4(pdp, oq + 64 * t); ps0[t] = ldo4(sbase(P), o0 + 64 * t); }
#pragma unroll
        for (int t = 0; t < 8; ++t) ps1[t] = ldo4(sbase(P), o1 + 64 * t);
    }

    for (int k = i_begin; k < i_end; k += i_step) {
        const int i = __builtin_amdgcn_readfirstlane(g.node), d = g.d, lig_i = g.lig_i;
        const bool more = k + i_step < i_end;   // wave-uniform
        const int k_next = k + i_step;
        // PP: the node's eight query channels of head c (32 bytes per lane), folded in k half 0.  Requested BEFORE the wait for the
        // rows below: in the latency regime (one node per wave: the rows were requested a moment ago) the two round trips then
        // overlap instead of following each other -- the fold sits one short MFMA block behind the top of the iteration
        float4 q8a = {0.f, 0.f, 0.f, 0.f}, q8b = {0.f, 0.f, 0.f, 0.f};
        if ((PP || HL) && CBGX_EDGE_EARLY_LOADS) {
            const gptr qp = sbase(Qt + (size_t)i * H);
            const unsigned oq8 = vop(32 * c);
            q8a = ldo4(qp, oq8); q8b = ldo4(qp, oq8 + 16);
        }
        // both halves' PD[i] + PS_k[j] as soon as the rows (requested one epilogue ago) are here: the 24 gather registers
        // are then free for this iteration's other gathers
        floatx4 acc0[8], acc1[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {   // (PD + PS) S: the tile is carried scaled by S (edge_common.h RbfScale)
            const floatx4 pds = f4(pd[t]) * sck.S;
            acc0[t] = f4(ps0[t]) * sck.S + pds; acc1[t] = f4(ps1[t]) * sck.S + pds;
        }
        __builtin_amdgcn_sched_barrier(0);
        // (a) next item: id, degree, flag, position, neighbour ids in both mappings.  The last iteration re-requests its own
        // node (every prefetch below is unconditional: no divergent joins for the register allocator, no predicated loads).
        // Issued BEFORE this node's gathers: vmcnt retires in order, so waiting for these few words later (b) leaves the
        // gathers in flight, while the other order would drain them.  The values stay in vector registers until (b).
        ItemGeom ng;
        const int inext = __builtin_amdgcn_readfirstlane(more ? (act ? act[k_next] : k_next) : i);
        ng.node = inext;
        const int nd_raw = deg[inext];
        const int nlig_raw = PP ? 0 : (HL ? 1 : ldob(sbase(lig), vop((unsigned)inext)));
        const gptr xrow = sbase(x + 3 * (size_t)inext);
        const unsigned ozero = vop(0u);
        const float nx_raw = ldo1(xrow, ozero), ny_raw = ldo1(xrow, ozero + 4), nz_raw = ldo1(xrow, ozero + 8);
        const gptr nrow = sbase(nbr + (size_t)inext * KNN);
        const unsigned oc = vop(4 * c);
        const int nr0 = ldoi(nrow, oc), nr1 = ldoi(nrow, oc + 64);
        __builtin_amdgcn_sched_barrier(0);
        // this node's folded query row (B operand of the score MFMAs): consumed after the first pre-activation block
        float4 qrow[8];
        if ((PP || HL) && !CBGX_EDGE_EARLY_LOADS) {
            const gptr qp = sbase(Qt + (size_t)i * H);
            const unsigned oq8 = vop(32 * c);
            q8a = ldo4(qp, oq8); q8b = ldo4(qp, oq8 + 16);
        }
        if (!PP && !HL) {
            const gptr qp = sbase(Qt + (size_t)i * HEADS * H);
            const unsigned oqr = vop((c * H + 4 * q) * 4);
#pragma unroll
            for (int t = 0; t < 8; ++t) qrow[t] = ldo4(qp, oqr + 64 * t);
        }
        // x2h: PS_v rows (channel-major gather, E1 mapping) of half 0 and this node's own PD_v, needed two MFMA blocks from here
        float4 sva[2][4], svb[2][4];
        float4 pa = {0.f, 0.f, 0.f, 0.f}, pb = {0.f, 0.f, 0.f, 0.f};
        if (X2H) {
            const int nbv[4] = {nb0.x, nb0.y, nb0.z, nb0.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned o = (unsigned)e1_id(nbv[r], 4 * q + r, d, i) * (PROW * 4) + (3 * H + 4 * c) * 4;
                sva[0][r] = ldo4(sbase(P), o);
                svb[0][r] = ldo4(sbase(P), o + 256);
            }
            const gptr pvp = sbase(P + (size_t)i * PROW);
            const unsigned ocv = vop((H + 4 * c) * 4);
            pa = ldo4(pvp, ocv);
            pb = ldo4(pvp, ocv + 256);
        }
        __builtin_amdgcn_sched_barrier(0);
        float R[2][5];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            // exp() of every slot, then a 0 / 1 factor: `valid ? exp(..) : 0` compiles to a divergent branch per value
            const float vm = c + 16 * hf < d ? RBF_UP : 0.f;   // 0 / 2^RBF_EXP: the rbf values enter the f16 pipe scaled
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const float u = dist0[hf] - lds_mu[4 * s + q];   // re-read per node: five registers less across the loop
                R[hf][s] = fast_exp(-0.5f * (u * u)) * vm;
            }
        }
        const unsigned long long b0 = __ballot(lg0[0]), b1 = __ballot(lg0[1]);
        const unsigned mask_lig = (unsigned)(b0 & 0xffffull) | ((unsigned)(b1 & 0xffffull) << 16);
        const unsigned mask_valid = d >= 32 ? 0xffffffffu : ((1u << d) - 1u);
        const bool has_lig = PP ? false : (mask_lig & mask_valid) != 0;
        const bool has_prot = PP ? true : ((~mask_lig) & mask_valid) != 0 || d == 0;

        // ---- k path: hidden (edge-major) -> scores -> softmax ------------------------------------------
        floatx4 sc[2];
        float qun = 1.f;
        sc[0] = edge_major_half<true, PP || HL, F16 ? 1 : 0>(acc0, lg0[0], 0, lds_fk, lds_dwt, lds_ln, R[0], has_prot, has_lig, lig_i, lane, q,
                                                             PP ? lds + PP_WFOLD + 4 * lane : (HL ? lds + H2L_WFOLD + 4 * lane : nullptr),
                                                             qrow, sck, q8a, q8b, khk_inv, &qun);
        __builtin_amdgcn_sched_barrier(0);
        // (b) next item: resolve its neighbour ids (they arrived during the first half), request their flags and
        // coordinates; then the second half of the PS_v gather and the gate values
        int nlj[2];
        float nxj[2][3];
        {
            ng.d = __builtin_amdgcn_readfirstlane(nd_raw);
            ng.lig_i = __builtin_amdgcn_readfirstlane(nlig_raw);
            ng.xi = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(nx_raw)));
            ng.yi = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(ny_raw)));
            ng.zi = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(nz_raw)));
            ng.j0[0] = c < ng.d ? nr0 : inext;
            ng.j0[1] = c + 16 < ng.d ? nr1 : inext;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int j = ng.j0[hf];
                nlj[hf] = PP ? 0 : ldob(sbase(lig), (unsigned)j);
                nxj[hf][0] = ldo1(sbase(x), 12u * j); nxj[hf][1] = ldo1(sbase(x), 12u * j + 4); nxj[hf][2] = ldo1(sbase(x), 12u * j + 8);
            }
        }
        float4 ew0 = {0.f, 0.f, 0.f, 0.f}, ew1 = {0.f, 0.f, 0.f, 0.f};
        if (X2H) {
            const int nbv[4] = {nb1.x, nb1.y, nb1.z, nb1.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned o = (unsigned)e1_id(nbv[r], 4 * q + r + 16, d, i) * (PROW * 4) + (3 * H + 4 * c) * 4;
                sva[1][r] = ldo4(sbase(P), o);
                svb[1][r] = ldo4(sbase(P), o + 256);
            }
        }
        const gptr ewp = sbase(e_w + (size_t)i * KNN);
        const unsigned oqe = vop(16 * q);
        ew0 = ldo4(ewp, oqe);
        ew1 = ldo4(ewp, oqe + 64);
        // h2x: this node's PD_v row and the PS_v rows of half 0 (edge-major), needed after the second k half: the registers of the
        // first half's accumulators carry them (until round 3 all 24 v rows were requested and waited for in one place, a full
        // exposed round trip per listed node)
        float4 vd[8], vs0[8], vs1[8];
        if (!X2H) {
            const gptr pdp = sbase(P + (size_t)i * PROW);
            const unsigned o0 = (unsigned)g.j0[0] * (PROW * 4) + (3 * H + 4 * q) * 4;
            const unsigned ovd = vop((H + 4 * q) * 4);
#pragma unroll
            for (int t = 0; t < 8; ++t) { vd[t] = ldo4(pdp, ovd + 64 * t); vs0[t] = ldo4(sbase(P), o0 + 64 * t); }
        }
        __builtin_amdgcn_sched_barrier(0);
        sc[1] = edge_major_half<true, false, F16 ? 2 : 0>(acc1, lg0[1], 0, lds_fk, lds_dwt, lds_ln, R[1], has_prot, has_lig, lig_i, lane, q,
                                                          nullptr, qrow, sck, float4{0.f, 0.f, 0.f, 0.f}, float4{0.f, 0.f, 0.f, 0.f},
                                                          khk_inv, &qun);
        __builtin_amdgcn_sched_barrier(0);
        if (!X2H) {   // PS_v rows of half 1: in flight during the softmax and the first v half
            const unsigned o1 = (unsigned)g.j0[1] * (PROW * 4) + (3 * H + 4 * q) * 4;
#pragma unroll
            for (int t = 0; t < 8; ++t) vs1[t] = ldo4(sbase(P), o1 + 64 * t);
        }
        // h2x: the neighbours' coordinates in the E1 mapping (equivariant update of the epilogue), requested here (the query
        // row and the k accumulators are dead) with the ids that came with this node's rows: the epilogue then has no load of its own (it used to run 24 dependent-looking dword loads, each
        // behind a vmcnt wait that also retired the next node's row prefetch: ~15 L2 round trips per listed node)
        float xj[2][4][3] = {};
        if (!X2H) {
            const int nbv[2][4] = {{nb0.x, nb0.y, nb0.z, nb0.w}, {nb1.x, nb1.y, nb1.z, nb1.w}};
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // invalid slots point at the node itself: rel = 0 and alpha = 0, so they add exactly nothing
                    const unsigned o = 12u * (unsigned)e1_id(nbv[hf][r], 4 * q + r + 16 * hf, d, i);
                    xj[hf][r][0] = ldo1(sbase(x), o); xj[hf][r][1] = ldo1(sbase(x), o + 4); xj[hf][r][2] = ldo1(sbase(x), o + 8);
                }
        }
        // next item: distances and ligand flags of its edges from the (b) loads
        bool nlg[2];
        float ndist[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            nlg[hf] = (c + 16 * hf < ng.d) && nlj[hf];
            ndist[hf] = edge_len(ng.xi, ng.yi, ng.zi, nxj[hf][0], nxj[hf][1], nxj[hf][2]);
        }
        // E1 mapping: lane (c = head a, q), reg (hf, r) <-> edge e = 4q + r + 16hf
        float al[2][4];
        float mx = -INFINITY;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool valid = 4 * q + r + 16 * hf < d;
                al[hf][r] = valid ? sc[hf][r] : -INFINITY;
                mx = fmaxf(mx, al[hf][r]);
            }
        mx = xrow_max(mx);
        float den = 0.f;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool valid = 4 * q + r + 16 * hf < d;
                al[hf][r] = valid ? fast_exp(al[hf][r] - mx) : 0.f;
                den += al[hf][r];
            }
        den = xrow_sum(den);
        const float inv_den = den > 0.f ? fast_rcp(den) : 0.f;
        const float ew[2][4] = {{ew0.x, ew0.y, ew0.z, ew0.w}, {ew1.x, ew1.y, ew1.z, ew1.w}};
        __builtin_amdgcn_sched_barrier(0);

        int4 nnb0, nnb1;   // next node's neighbour row in the E1 mapping, requested before the epilogue
        if (X2H) {
            float w[2][4];
            float sw = 0.f;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // softmax first (alpha = ex / den, like scatter_softmax), then the gate
                    w[hf][r] = (al[hf][r] * inv_den) * ew[hf][r];
                    sw += w[hf][r];
                }
            sw = xrow_sum(sw);   // sum_e alpha e_w for head a = c
            // residual row and bias of this lane's two outputs, used after the Wbv products of the epilogue: requested here, ahead
            // of the next item's 24-row prefetch (vmcnt retires in order: behind it, the wait for these two words drained the
            // prefetch -- and in the latency regime was a round trip of its own)
            const int n0 = 8 * c + 2 * q;
            const unsigned on0 = vop(n0 * 4);
            float2 hres, bias2;
            if (CBGX_EDGE_EARLY_LOADS) { hres = ldo2(sbase(h + (size_t)i * H), on0); bias2 = ldo2(sbase(att + A_BBV), on0); }
            // ---- v path, channel-major, one half at a time: lane (c, q) reg r <-> edge 4q + r + 16hf, m = 8c + t
            // aggregated straight into s2[t] = hid_v^T . w : lane (c = head a, q) reg r' <-> channel 64(t>>2) + 16q + 4r' + (t&3)
            floatx4 s2[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) s2[t] = floatx4{0.f, 0.f, 0.f, 0.f};
            const float pdv[8] = {pa.x * scv.S, pa.y * scv.S, pa.z * scv.S, pa.w * scv.S,
                                  pb.x * scv.S, pb.y * scv.S, pb.z * scv.S, pb.w * scv.S};
            // F16: the lane offset is laundered here, so that the four reads share one address computed in the loop -- hoisted, the four
            // loop-invariant addresses were what the register allocator spilled (a reload is a VMEM wait in front of the gathers)
            float4 ga, gb, ba, bb;
            if constexpr (F16) {
                const float* lnv = lds_ln + 2 * H + (int)vop(4 * c);
                ga = ld4(lnv); gb = ld4(lnv + 64);
                ba = ld4(lnv + H); bb = ld4(lnv + H + 64);
            } else {
                ga = ld4(lds_ln + 2 * H + 4 * c); gb = ld4(lds_ln + 2 * H + 64 + 4 * c);
                ba = ld4(lds_ln + 3 * H + 4 * c); bb = ld4(lds_ln + 3 * H + 64 + 4 * c);
            }
            const float gv[8] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
            const float bv[8] = {ba.x, ba.y, ba.z, ba.w, bb.x, bb.y, bb.z, bb.w};
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                floatx4 hv[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // a gathered float4 is four channels of one edge, a tile register quad is four edges of one channel:
                    // plain v_add_f32 writes each sum where the MFMA wants it.  The empty asm keeps the vectoriser from
                    // pairing the adds (it would build every pair with two v_mov first: 3 instructions per 2 sums).
                    const float4 sa = sva[hf][r], sb = svb[hf][r];
                    const float in[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        float sum = __builtin_fmaf(in[t], scv.S, pdv[t]);    // (PD_v + PS_v) S
                        asm("" : "+v"(sum));
                        hv[t][r] = sum;
                    }
                }
                if (has_lig) {
                    const float* dw = lds_dwt + lig_i * 2 * H + H + 4 * c;
                    const float4 da = ld4(dw), db = ld4(dw + 64);
                    const float dv[8] = {da.x, da.y, da.z, da.w, db.x, db.y, db.z, db.w};
                    const unsigned msh = mask_lig >> (4 * q);   // bit r (+16) <-> edge 4q + r (+16): immediate bit-field extracts
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float m = ((msh >> (r + 16 * hf)) & 1u) ? scv.S : 0.f;
#pragma unroll
                        for (int t = 0; t < 8; ++t) hv[t][r] = fmaf(m, dv[t], hv[t][r]);
                    }
                }
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    if (p == 0 ? !has_prot : !has_lig) continue;
                    float Rm[5];
#pragma unroll
                    for (int s = 0; s < 5; ++s) Rm[s] = (lg0[hf] == (p == 1)) ? R[hf][s] : 0.f;
                    // split-f16, rbf tuples as the A operand, weight tuples as B
                    half4 A[4];
                    rbf_tuples(Rm, A);
                    const float* fb = lds_fv + (size_t)etype(p == 1, lig_i) * (8 * FRAG_BLK);
#pragma unroll
                    for (int tg = 0; tg < 8; tg += 2) {
                        const WTuples w0 = load_wtuples(fb, tg, lane), w1 = load_wtuples(fb, tg + 1, lane);
                        hv[tg] = MFMAH(A[0], w0.t1, hv[tg]);         hv[tg + 1] = MFMAH(A[0], w1.t1, hv[tg + 1]);
                        hv[tg] = MFMAH(A[1], w0.t1, hv[tg]);         hv[tg + 1] = MFMAH(A[1], w1.t1, hv[tg + 1]);
                        hv[tg] = MFMAH(A[2], w0.t2, hv[tg]);         hv[tg + 1] = MFMAH(A[2], w1.t2, hv[tg + 1]);
                        hv[tg] = MFMAH(A[3], w0.t3, hv[tg]);         hv[tg + 1] = MFMAH(A[3], w1.t3, hv[tg + 1]);
                    }
                }
                // LayerNorm per edge r (zero mean by construction): in-lane over t, across the 16 lanes of the row
                {   // edges r and r + 1 share the packed instructions
                    float2v va = {0.f, 0.f}, vb = {0.f, 0.f};
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        va = lo2(hv[t]) * lo2(hv[t]) + va;
                        vb = hi2(hv[t]) * hi2(hv[t]) + vb;
                    }
                    float2v ra, rb;
                    ra.x = fast_rsqrt(__builtin_fmaf(row16_sum(va.x), scv.c1, 1e-5f)) * scv.c2;
                    ra.y = fast_rsqrt(__builtin_fmaf(row16_sum(va.y), scv.c1, 1e-5f)) * scv.c2;
                    rb.x = fast_rsqrt(__builtin_fmaf(row16_sum(vb.x), scv.c1, 1e-5f)) * scv.c2;
                    rb.y = fast_rsqrt(__builtin_fmaf(row16_sum(vb.y), scv.c1, 1e-5f)) * scv.c2;
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const float2v g2 = splat2(gv[t]), b2 = splat2(bv[t]);
                        const float2v ya = (lo2(hv[t]) * ra) * g2 + b2;
                        const float2v yb = (hi2(hv[t]) * rb) * g2 + b2;
                        hv[t] = floatx4{fmaxf(ya.x, 0.f), fmaxf(ya.y, 0.f), fmaxf(yb.x, 0.f), fmaxf(yb.y, 0.f)};
                    }
                }
                if constexpr (F16) {
                    // s2[t] += hv[t]^T . w as ONE 16x16x16 step per tile: A = the register quad hv[t][0..3] (k = 4q + r <-> edge
                    // 4q + r + 16hf), B = w[hf][0..3] 2^14; three products (hi hi, lo hi, hi lo), two tiles interleaved
                    half4 wh, wl;
                    split_f16x4(floatx4{w[hf][0], w[hf][1], w[hf][2], w[hf][3]} * W_UP, wh, wl);
#pragma unroll
                    for (int t = 0; t < 8; t += 2) {
                        half4 h0, l0, h1, l1;
                        split_f16x4(hv[t], h0, l0);
                        split_f16x4(hv[t + 1], h1, l1);
                        s2[t] = MFMAH(h0, wh, s2[t]);         s2[t + 1] = MFMAH(h1, wh, s2[t + 1]);
                        s2[t] = MFMAH(l0, wh, s2[t]);         s2[t + 1] = MFMAH(l1, wh, s2[t + 1]);
                        s2[t] = MFMAH(h0, wl, s2[t]);         s2[t + 1] = MFMAH(h1, wl, s2[t + 1]);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int t = 0; t < 8; ++t) s2[t] = MFMA(hv[t][r], w[hf][r], s2[t]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // (c) next item: its PD / PS_k rows fly during the epilogue (the v path's gather registers are free again)
            {
                const gptr pdp = sbase(P + (size_t)inext * PROW);
                const unsigned o0 = (unsigned)ng.j0[0] * (PROW * 4) + (2 * H + 4 * q) * 4;
                const unsigned o1 = (unsigned)ng.j0[1] * (PROW * 4) + (2 * H + 4 * q) * 4;
                const unsigned oq = vop(16 * q);
#pragma unroll
                for (int t = 0; t < 8; ++t) { pd[t] = ldo4(pdp, oq + 64 * t); ps0[t] = ldo4(sbase(P), o0 + 64 * t); }
#pragma unroll
                for (int t = 0; t < 8; ++t) ps1[t] = ldo4(sbase(P), o1 + 64 * t);
            }
            // (the residual row and bias of this lane's two outputs were requested before the v path); the next node's neighbour
            // row in the E1 mapping is last in the queue: it is only needed at the top of the next iteration
            if (!CBGX_EDGE_EARLY_LOADS) { hres = ldo2(sbase(h + (size_t)i * H), on0); bias2 = ldo2(sbase(att + A_BBV), on0); }
            {
                const gptr nrow2 = sbase(nbr + (size_t)inext * KNN);
                const unsigned oq2 = vop(16 * q);
                nnb0 = ldoi4(nrow2, oq2); nnb1 = ldoi4(nrow2, oq2 + 64);
            }
            __builtin_amdgcn_sched_barrier(0);
            // epilogue: out[8a + cc] = sum_m Wbv[8a + cc][m] S[a][m] + bbv[8a + cc] sum_e alpha e_w ; this lane holds
            // S[a = c][m] for m = 64 hh + 16 q + 4 r + j in s2[4 hh + j][r].  Wbv rows live in LDS as 16-byte chunks
            // K = 16 hh + 4 q + j holding the four channels r = 0..3 of that (hh, q, j) -- the register quad of s2[4 hh + j], so
            // the 8 x 32 products are packed FMAs on the accumulators as they are -- with the chunk index XOR-swizzled by
            // wbv_swizzle(head).  A ds_read_b128 is served in four groups of 16 lanes that mix two values of q
            // ({0-3, 12-15 | q} with {4-11 | q + 1}, MI355X_MICROARCH.md LDS): the permutation makes the 16 lanes of every
            // group land on 16 different 16-byte slots (XOR with the head index itself was 2-way conflicted on every read:
            // 256 of the node's 880 LDS cycles).
            float o8[8];
            const float* lds_wbv = lds + (PP ? PP_WBV : IMG_WBV);
            const int swz = wbv_swizzle(c);
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) {
                const float* wrow = lds_wbv + (size_t)(8 * c + cc) * H;
                float2v a2 = {0.f, 0.f};
#pragma unroll
                for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const floatx4 w4 = f4(ld4(wrow + (((16 * hh + 4 * q + j) ^ swz) << 2)));
                        a2 = lo2(w4) * lo2(s2[4 * hh + j]) + a2;
                        a2 = hi2(w4) * hi2(s2[4 * hh + j]) + a2;
                    }
                o8[cc] = xrow_sum(a2.x + a2.y);
            }
            // lane (c, q) writes outputs n = 8c + 2q, 8c + 2q + 1
            const float oa = q == 0 ? o8[0] : (q == 1 ? o8[2] : (q == 2 ? o8[4] : o8[6]));
            const float ob = q == 0 ? o8[1] : (q == 1 ? o8[3] : (q == 2 ? o8[5] : o8[7]));
            float2 o;
            if constexpr (F16) {      // s2 carries 2^kh (hidden) 2^14 (weights): undone on the two sums this lane writes
                o.x = hres.x + (oa * s2_un + bias2.x * sw);
                o.y = hres.y + (ob * s2_un + bias2.y * sw);
            } else {
                o.x = hres.x + (oa + bias2.x * sw);
                o.y = hres.y + (ob + bias2.y * sw);
            }
            sto2(sbase_w(out + (size_t)i * H), vop(n0 * 4), o);
        } else {
            // ---- h2x: v hidden edge-major, wv[e][a] = Wbv[a] . hid_v[e] + bbv[a] -------------------------------
            floatx4 wv[2];
            {
                const float* lds_brow = HL ? lds + H2L_WBV + 4 * lane : lds + IMG_WBV + 4 * lane;       // Wbv[head c][16 t + 4 q ..] at 256 t (layout.h)
                floatx4 acc[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) { vd[t] = make_float4(vd[t].x * scv.S, vd[t].y * scv.S, vd[t].z * scv.S, vd[t].w * scv.S); acc[t] = f4(vs0[t]) * scv.S + f4(vd[t]); }
                wv[0] = edge_major_half<false>(acc, lg0[0], 1, lds_fv, lds_dwt, lds_ln, R[0], has_prot, has_lig, lig_i, lane, q,
                                               lds_brow, qrow, scv);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < 8; ++t) acc[t] = f4(vs1[t]) * scv.S + f4(vd[t]);
                wv[1] = edge_major_half<false>(acc, lg0[1], 1, lds_fv, lds_dwt, lds_ln, R[1], has_prot, has_lig, lig_i, lane, q,
                                               lds_brow, qrow, scv);
                __builtin_amdgcn_sched_barrier(0);
            }
            // (c) next item: its PD / PS_k rows
            {
                const gptr pdp = sbase(P + (size_t)inext * PROW);
                const unsigned o0 = (unsigned)ng.j0[0] * (PROW * 4) + (2 * H + 4 * q) * 4;
                const unsigned o1 = (unsigned)ng.j0[1] * (PROW * 4) + (2 * H + 4 * q) * 4;
                const unsigned oq = vop(16 * q);
#pragma unroll
                for (int t = 0; t < 8; ++t) { pd[t] = ldo4(pdp, oq + 64 * t); ps0[t] = ldo4(sbase(P), o0 + 64 * t); }
#pragma unroll
                for (int t = 0; t < 8; ++t) ps1[t] = ldo4(sbase(P), o1 + 64 * t);
            }
            __builtin_amdgcn_sched_barrier(0);
            {
                const gptr nrow2 = sbase(nbr + (size_t)inext * KNN);
                const unsigned oq2 = vop(16 * q);
                nnb0 = ldoi4(nrow2, oq2); nnb1 = ldoi4(nrow2, oq2 + 64);
            }
            float dx = 0.f, dy = 0.f, dz = 0.f;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float coef = (al[hf][r] * inv_den) * ((wv[hf][r] + bbv) * ew[hf][r]);
                    const float cf = 4 * q + r + 16 * hf < d ? coef : 0.f;
                    dx = fmaf(cf, g.xi - xj[hf][r][0], dx);
                    dy = fmaf(cf, g.yi - xj[hf][r][1], dy);
                    dz = fmaf(cf, g.zi - xj[hf][r][2], dz);
                }
            dx = wave_sum(dx); dy = wave_sum(dy); dz = wave_sum(dz);
            if (lane < 3) {
                const float v = (lane == 0 ? dx : (lane == 1 ? dy : dz)) * (1.f / HEADS);
                const float xin = lane == 0 ? g.xi : (lane == 1 ? g.yi : g.zi);
                if (dx_out) dx_out[3 * i + lane] = v;
                out[3 * i + lane] = xin + (gen[i] ? v : 0.f);
            }
        }
        // rotate the pipelined geometry
        nb0 = nnb0; nb1 = nnb1;
        lg0[0] = nlg[0]; lg0[1] = nlg[1]; dist0[0] = ndist[0]; dist0[1] = ndist[1];
        g = ng;
    }
}

// Role split of the two-list x2h kernels (edge_x2h_dual_kernel, edge_x2h_f16_kernel): how many of the `n_wg` workgroups play the
// protein-only role, from the device-side list lengths.
#ifndef CBGX_DUAL_GEN_COST
#define CBGX_DUAL_GEN_COST 1.15f      // (an A/B knob of scripts/build_variant.py; the product build uses this value:
                                      //  1.0 / 1.15 / 1.3 / 1.45 / 1.7 -> 768 / 1185 / 1222 / 1220 / 748 us per launch in their sessions, profiles/ab_fwd_r04[df].log)
#endif
constexpr float DUAL_GEN_COST = CBGX_DUAL_GEN_COST;
template <int WAVES>
__device__ __forceinline__ int dual_pp_workgroups(const int c_pp, const int c_gen, const int n_wg) {
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
    return n_pp_wg;
}

}  // namespace cbgx

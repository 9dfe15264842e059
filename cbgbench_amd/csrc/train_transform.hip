// libcbgx -- the per-visit transforms of a training batch (the reference's add_pos_noise followed by center_pos / center_whole_pos,
// repo/datasets/transforms/translation.py), for a whole batch in ONE launch, one 256-thread workgroup per graph:
//   1. protein noise   noised = fmaf(sigma, eps, x) for every protein atom (sigma > 0 only; sigma == 0 copies x).  eps comes from the
//                      caller's tape (RNG false) or is drawn in place (RNG true): counter =
//                      (the atom's index inside its pocket, step 0, purpose base + TRAIN_PROTEIN_NORMAL, block 0), components 0..2, under
//                      the graph's stream key -- the expressions noise_fill_kernel (step.hip) stores, so the two routes agree bit for bit.
//   2. centre          the mean of the graph's centre set: the NOISED protein atoms (CENTER_PROTEIN), the ligand atoms with ctx != 0
//                      (CENTER_CONTEXT; a graph without one falls back to its whole ligand, translation.py:13-16), the ligand atoms
//                      (CENTER_LIGAND), or noised protein atoms followed by ligand atoms (CENTER_WHOLE).  The sum has a fixed order that
//                      depends on the graph's own atoms only: the candidates of the set are numbered in atom order (WHOLE: protein atoms
//                      first, then ligand atoms; CONTEXT: every ligand atom is a candidate, non-context atoms add nothing), thread k adds
//                      candidates k, k + 256, ... in that order, a fixed LDS tree (strides 128, 64, ..., 1) adds the 256 partial sums, and
//                      one IEEE division by the member count follows.  No atomics.  An empty set gives the zero vector.
//   3. shift           out = noised - centre for the protein atoms, out = x - centre for the ligand atoms, center_out[g] = centre.
// A thread keeps the noised coordinates of its first three protein atoms (pockets of up to 768 atoms) in registers between the sum and
// the subtraction; those of further atoms wait in x_rec_out, where the same thread wrote them.  No coordinate is drawn twice.
// Every product and sum is written as the rounding it is (fmaf / __fadd_rn / __fsub_rn / __fdiv_rn): nothing is left to contraction.
//
// train_transform_choose_kernel (cbgx_train_transform_choose{,_rng}; the body with CHOOSE) puts the reference's choose_ctx_gen (select.py:21-58) in front, in
// the same launch -- the centre set of CENTER_CONTEXT is the complement of the atoms it picks:
//   0. choice          graph g owns the decompositions dec_ptr[g] .. dec_ptr[g+1] (K of them); decomposition d names the ligand-local atoms
//                      gen_idx[gen_ptr[d] .. gen_ptr[d+1]].  k = choice_in[g] clamped into [0, K) (tape; NULL: 0), or
//                      scale_word(word 0 of the call at counter (0, 0, base + TRAIN_CHOOSE_CTX, 0) under the graph's key, K) (counter:
//                      rng::train_time's formula at its own address).  K == 0: k = -1 and every ligand atom is generated.
//      flag            gen_flag_out = 0 on the graph's ligand rows, barrier, = 1 on the rows decomposition k names (an index outside the
//                      ligand is skipped, duplicates write the same byte twice), barrier; steps 1 - 3 then read ctx = !gen_flag_out.  The
//                      flags live in global memory (a ligand has no size limit); a workgroup reads only the rows it wrote itself.
// The three CSRs are clamped to their arrays like rec_ptr / lig_ptr.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cbgx.h"     // CBGX_CENTER_*
#include "kernels.h"
#include "rng.h"
#include "train.h"

namespace cbgx {

constexpr int TT_THREADS = 256;
constexpr int TT_HELD = 3;      // protein atoms per thread whose noised coordinates stay in registers

// the 256 partial sums of four values -> their total in every thread; the order of the additions is fixed
__device__ __forceinline__ void tt_tree(float (*red)[TT_THREADS], float& a, float& b, float& c, float& d) {
    const int k = threadIdx.x;
    __syncthreads();            // (the previous round's reads of red[..][0] are over)
    red[0][k] = a; red[1][k] = b; red[2][k] = c; red[3][k] = d;
    __syncthreads();
    for (int s = TT_THREADS / 2; s > 0; s >>= 1) {
        if (k < s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) red[j][k] = __fadd_rn(red[j][k], red[j][k + s]);
        }
        __syncthreads();
    }
    a = red[0][0]; b = red[1][0]; c = red[2][0]; d = red[3][0];
}

// operands of the decomposition choice (train_transform_choose_kernel; the body without CHOOSE never reads them)
struct TTChoose {
    const int32_t* dec_ptr; const int32_t* gen_ptr; const int32_t* gen_idx; const int32_t* choice_in;
    int n_dec, n_idx;
    uint32_t purpose;           // base + TRAIN_CHOOSE_CTX
    uint8_t* gen_flag_out; int32_t* choice_out;
};

// the one body of the four kernels below
template <bool RNG, bool CHOOSE>
__device__ __forceinline__ void train_transform_body(
    const float* __restrict__ x_rec, const float* __restrict__ x_lig, const int32_t* __restrict__ rec_ptr,
    const int32_t* __restrict__ lig_ptr, const uint8_t* __restrict__ ctx, int n_rec, int n_lig, float sigma, int mode,
    const float* __restrict__ eps, const uint64_t* __restrict__ keys, uint32_t purpose, float* x_rec_out, float* __restrict__ x_lig_out,
    float* __restrict__ center_out, const TTChoose& ch) {
    __shared__ float red[4][TT_THREADS];
    const int g = blockIdx.x, k = threadIdx.x;
    // a malformed CSR must not reach outside the arrays: both ranges are clamped to them
    const int r0 = min(max(rec_ptr[g], 0), n_rec), r1 = min(max(rec_ptr[g + 1], r0), n_rec);
    const int l0 = min(max(lig_ptr[g], 0), n_lig), l1 = min(max(lig_ptr[g + 1], l0), n_lig);
    const int nr = r1 - r0, nl = l1 - l0;
    const bool noisy = sigma > 0.f;
    const bool rec_in_set = mode == CBGX_CENTER_PROTEIN || mode == CBGX_CENTER_WHOLE;
    uint64_t key = 0;
    if (RNG && (noisy || CHOOSE)) key = keys[g];
    // ---- decomposition choice and the generated-atom flag of the graph's ligand rows -------------------------------------------------
    if constexpr (CHOOSE) {
        const int d0 = min(max(ch.dec_ptr[g], 0), ch.n_dec), d1 = min(max(ch.dec_ptr[g + 1], d0), ch.n_dec);
        const int K = d1 - d0;                   // uniform over the workgroup, and so is every branch on it
        int kc = -1;
        if (K > 0) {
            if (RNG) kc = (int)rng::scale_word(rng::draw(key, 0u, 0u, ch.purpose, 0u).w0, (uint32_t)K);
            else kc = ch.choice_in ? min(max(ch.choice_in[g], 0), K - 1) : 0;
        }
        if (k == 0) ch.choice_out[g] = kc;
        const uint8_t rest = K > 0 ? 0 : 1;      // no decomposition: the whole ligand is generated
        for (int la = k; la < nl; la += TT_THREADS) ch.gen_flag_out[(size_t)(l0 + la)] = rest;
        if (K > 0) {
            __syncthreads();                     // the scatter overwrites bytes that other threads have just cleared
            const int d = d0 + kc;
            const int i0 = min(max(ch.gen_ptr[d], 0), ch.n_idx), i1 = min(max(ch.gen_ptr[d + 1], i0), ch.n_idx);
            for (int i = i0 + k; i < i1; i += TT_THREADS) {
                const int la = ch.gen_idx[i];
                if (la >= 0 && la < nl) ch.gen_flag_out[(size_t)(l0 + la)] = 1;
            }
        }
        __syncthreads();                         // the sum below reads rows that other threads of the workgroup wrote
    }
    auto in_ctx = [&](size_t a) -> bool {
        if constexpr (CHOOSE) return ch.gen_flag_out[a] == 0;
        else return ctx[a] != 0;
    };

    float sx = 0.f, sy = 0.f, sz = 0.f;
    float held[TT_HELD][3];
    // ---- protein atoms: noise, partial sum in index order k, k + 256, ... -------------------------------------------------------------
    auto noised = [&](int la, float& px, float& py, float& pz) {
        const size_t a = (size_t)(r0 + la);
        px = x_rec[3 * a + 0]; py = x_rec[3 * a + 1]; pz = x_rec[3 * a + 2];
        if (noisy) {
            float e0, e1, e2;
            if (RNG) {
                const rng::Words o = rng::draw(key, (uint32_t)la, 0u, purpose, 0u);
                e0 = rng::normal_component(o, 0); e1 = rng::normal_component(o, 1); e2 = rng::normal_component(o, 2);
            } else {
                e0 = eps[3 * a + 0]; e1 = eps[3 * a + 1]; e2 = eps[3 * a + 2];
            }
            px = fmaf(sigma, e0, px); py = fmaf(sigma, e1, py); pz = fmaf(sigma, e2, pz);
        }
        if (rec_in_set) { sx = __fadd_rn(sx, px); sy = __fadd_rn(sy, py); sz = __fadd_rn(sz, pz); }
    };
#pragma unroll
    for (int j = 0; j < TT_HELD; ++j) {
        const int la = k + TT_THREADS * j;
        held[j][0] = held[j][1] = held[j][2] = 0.f;
        if (la < nr) noised(la, held[j][0], held[j][1], held[j][2]);
    }
    for (int la = k + TT_THREADS * TT_HELD; la < nr; la += TT_THREADS) {
        float px, py, pz;
        noised(la, px, py, pz);
        const size_t a = (size_t)(r0 + la);
        x_rec_out[3 * a + 0] = px; x_rec_out[3 * a + 1] = py; x_rec_out[3 * a + 2] = pz;     // read back below by this same thread
    }
    // ---- ligand atoms of the centre set -----------------------------------------------------------------------------------------------
    float cnt = rec_in_set ? (float)nr : 0.f;      // member count of the set (total, not per thread: only thread totals are reduced)
    float mine = 0.f;                             // context members this thread has seen
    if (mode == CBGX_CENTER_WHOLE) {
        // candidate i = nr + la of the joint numbering belongs to thread i % 256
        const int first = ((k - nr) % TT_THREADS + TT_THREADS) % TT_THREADS;
        for (int la = first; la < nl; la += TT_THREADS) {
            const size_t a = (size_t)(l0 + la);
            sx = __fadd_rn(sx, x_lig[3 * a + 0]); sy = __fadd_rn(sy, x_lig[3 * a + 1]); sz = __fadd_rn(sz, x_lig[3 * a + 2]);
        }
        cnt = (float)nr + (float)nl;
    } else if (mode == CBGX_CENTER_CONTEXT && (CHOOSE || ctx)) {
        for (int la = k; la < nl; la += TT_THREADS) {
            const size_t a = (size_t)(l0 + la);
            if (in_ctx(a)) {
                sx = __fadd_rn(sx, x_lig[3 * a + 0]); sy = __fadd_rn(sy, x_lig[3 * a + 1]); sz = __fadd_rn(sz, x_lig[3 * a + 2]);
                mine += 1.f;
            }
        }
    }
    if (mode != CBGX_CENTER_LIGAND) tt_tree(red, sx, sy, sz, mine);
    bool lig_set = mode == CBGX_CENTER_LIGAND;
    if (mode == CBGX_CENTER_CONTEXT) {
        cnt = mine;                               // (counts below 2^24 are exact in fp32)
        lig_set = cnt == 0.f;                     // no context atom: the whole ligand (uniform over the workgroup)
    }
    if (lig_set) {
        sx = sy = sz = 0.f;
        float unused = 0.f;
        for (int la = k; la < nl; la += TT_THREADS) {
            const size_t a = (size_t)(l0 + la);
            sx = __fadd_rn(sx, x_lig[3 * a + 0]); sy = __fadd_rn(sy, x_lig[3 * a + 1]); sz = __fadd_rn(sz, x_lig[3 * a + 2]);
        }
        tt_tree(red, sx, sy, sz, unused);
        cnt = (float)nl;
    }
    float cx = 0.f, cy = 0.f, cz = 0.f;
    if (cnt > 0.f) { cx = __fdiv_rn(sx, cnt); cy = __fdiv_rn(sy, cnt); cz = __fdiv_rn(sz, cnt); }
    if (k == 0) {
        center_out[3 * (size_t)g + 0] = cx; center_out[3 * (size_t)g + 1] = cy; center_out[3 * (size_t)g + 2] = cz;
    }
    // ---- shift ------------------------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < TT_HELD; ++j) {
        const int la = k + TT_THREADS * j;
        if (la < nr) {
            const size_t a = (size_t)(r0 + la);
            x_rec_out[3 * a + 0] = __fsub_rn(held[j][0], cx);
            x_rec_out[3 * a + 1] = __fsub_rn(held[j][1], cy);
            x_rec_out[3 * a + 2] = __fsub_rn(held[j][2], cz);
        }
    }
    for (int la = k + TT_THREADS * TT_HELD; la < nr; la += TT_THREADS) {
        const size_t a = (size_t)(r0 + la);
        x_rec_out[3 * a + 0] = __fsub_rn(x_rec_out[3 * a + 0], cx);
        x_rec_out[3 * a + 1] = __fsub_rn(x_rec_out[3 * a + 1], cy);
        x_rec_out[3 * a + 2] = __fsub_rn(x_rec_out[3 * a + 2], cz);
    }
    for (int la = k; la < nl; la += TT_THREADS) {
        const size_t a = (size_t)(l0 + la);
        x_lig_out[3 * a + 0] = __fsub_rn(x_lig[3 * a + 0], cx);
        x_lig_out[3 * a + 1] = __fsub_rn(x_lig[3 * a + 1], cy);
        x_lig_out[3 * a + 2] = __fsub_rn(x_lig[3 * a + 2], cz);
    }
}

// cbgx_train_transform (RNG false) / cbgx_train_transform_rng (true): the argument block they have always had
template <bool RNG>
__global__ __launch_bounds__(TT_THREADS) void train_transform_kernel(
    const float* __restrict__ x_rec, const float* __restrict__ x_lig, const int32_t* __restrict__ rec_ptr,
    const int32_t* __restrict__ lig_ptr, const uint8_t* __restrict__ ctx, int n_rec, int n_lig, float sigma, int mode,
    const float* __restrict__ eps, const uint64_t* __restrict__ keys, uint32_t purpose, float* x_rec_out, float* __restrict__ x_lig_out,
    float* __restrict__ center_out) {
    train_transform_body<RNG, false>(x_rec, x_lig, rec_ptr, lig_ptr, ctx, n_rec, n_lig, sigma, mode, eps, keys, purpose, x_rec_out,
                                     x_lig_out, center_out, TTChoose{});
}

// cbgx_train_transform_choose / cbgx_train_transform_choose_rng: the decompositions in place of the context flag
template <bool RNG>
__global__ __launch_bounds__(TT_THREADS) void train_transform_choose_kernel(
    const float* __restrict__ x_rec, const float* __restrict__ x_lig, const int32_t* __restrict__ rec_ptr,
    const int32_t* __restrict__ lig_ptr, int n_rec, int n_lig, float sigma, int mode, const float* __restrict__ eps,
    const uint64_t* __restrict__ keys, uint32_t purpose, float* x_rec_out, float* __restrict__ x_lig_out,
    float* __restrict__ center_out, TTChoose ch) {
    train_transform_body<RNG, true>(x_rec, x_lig, rec_ptr, lig_ptr, nullptr, n_rec, n_lig, sigma, mode, eps, keys, purpose, x_rec_out,
                                    x_lig_out, center_out, ch);
}

hipError_t launch_train_transform(const float* x_rec, const float* x_lig, const int32_t* rec_ptr, const int32_t* lig_ptr,
                                  const uint8_t* ctx, int n_graphs, int n_rec, int n_lig, float sigma, int mode, const float* eps,
                                  const uint64_t* keys, uint32_t purpose, float* x_rec_out, float* x_lig_out, float* center_out,
                                  hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    if (keys)
        hipLaunchKernelGGL(train_transform_kernel<true>, dim3(n_graphs), dim3(TT_THREADS), 0, s, x_rec, x_lig, rec_ptr, lig_ptr, ctx,
                           n_rec, n_lig, sigma, mode, eps, keys, purpose, x_rec_out, x_lig_out, center_out);
    else
        hipLaunchKernelGGL(train_transform_kernel<false>, dim3(n_graphs), dim3(TT_THREADS), 0, s, x_rec, x_lig, rec_ptr, lig_ptr, ctx,
                           n_rec, n_lig, sigma, mode, eps, keys, purpose, x_rec_out, x_lig_out, center_out);
    return hipGetLastError();
}

hipError_t launch_train_transform_choose(const float* x_rec, const float* x_lig, const int32_t* rec_ptr, const int32_t* lig_ptr,
                                         const int32_t* dec_ptr, const int32_t* gen_ptr, const int32_t* gen_idx,
                                         const int32_t* choice_in, int n_graphs, int n_rec, int n_lig, int n_dec, int n_idx,
                                         float sigma, int mode, const float* eps, const uint64_t* keys, uint32_t purpose_base,
                                         float* x_rec_out, float* x_lig_out, float* center_out, uint8_t* gen_flag_out,
                                         int32_t* choice_out, hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    const TTChoose ch = {dec_ptr, gen_ptr, gen_idx, choice_in, n_dec, n_idx, purpose_base + (uint32_t)rng::TRAIN_CHOOSE_CTX,
                         gen_flag_out, choice_out};
    const uint32_t purpose = purpose_base + (uint32_t)rng::TRAIN_PROTEIN_NORMAL;
    if (keys)
        hipLaunchKernelGGL(train_transform_choose_kernel<true>, dim3(n_graphs), dim3(TT_THREADS), 0, s, x_rec, x_lig, rec_ptr, lig_ptr,
                           n_rec, n_lig, sigma, mode, eps, keys, purpose, x_rec_out, x_lig_out, center_out, ch);
    else
        hipLaunchKernelGGL(train_transform_choose_kernel<false>, dim3(n_graphs), dim3(TT_THREADS), 0, s, x_rec, x_lig, rec_ptr, lig_ptr,
                           n_rec, n_lig, sigma, mode, eps, keys, purpose, x_rec_out, x_lig_out, center_out, ch);
    return hipGetLastError();
}

}  // namespace cbgx

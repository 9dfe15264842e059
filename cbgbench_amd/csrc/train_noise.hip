// libcbgx -- counter-based noise of training and validation calls ("counter" noise mode of get_loss; rng.h says how a draw is addressed):
//   train_noise_draw_kernel   the draws of ONE get_loss call in one launch: the time of every graph (drawn, or the caller's), the position
//                             normals and one further per-atom buffer (TargetDiff's type uniforms, DiffBP's mask uniform, DiffSBDD's type
//                             normals), both at step = the graph's time.  DiffBP and DiffSBDD take the mode through it, followed by their
//                             tape noising kernels; so does every tensor path (replay arguments t= / noise=).
//   train_noise_rng_kernel    TargetDiff: train_noise_kernel of train_loss.hip with eps / u / t generated in place -- its losses read
//                             neither eps nor u again, so no noise buffer exists in that path.  A second kernel, not an instantiation of a
//                             shared template: train_loss.hip is untouched and its kernel stays the kernel it is.  The arithmetic around
//                             the draws is that kernel's, expression by expression (each product rounded, no contraction), and the draws
//                             are the expressions train_noise_draw_kernel stores, so the two routes agree bit for bit.
// The Philox words are named struct members selected by value (rng.h): no indexed read, no scratch, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "rng.h"
#include "train.h"

namespace cbgx {

// one workgroup per graph (an empty graph still gets its time written); a thread takes one (atom, block) pair = one Philox call
__global__ __launch_bounds__(256) void train_noise_draw_kernel(const uint64_t* __restrict__ keys, const int32_t* __restrict__ lig_ptr,
                                                               int n_lig, uint32_t base, uint32_t n_t,
                                                               const int64_t* __restrict__ t_in, int64_t* __restrict__ t_out,
                                                               float* __restrict__ a_out, float* __restrict__ b_out, int cols_b,
                                                               uint32_t purpose_b, int uniform_b) {
    const int g = blockIdx.x;
    const uint64_t key = keys[g];
    const int64_t tg = t_in ? t_in[g] : (int64_t)rng::train_time(key, base, n_t);
    if (threadIdx.x == 0) t_out[g] = tg;
    const uint32_t step = (uint32_t)tg;
    const int a0 = max(lig_ptr[g], 0), a1 = min(lig_ptr[g + 1], n_lig);
    const int first_b = a_out ? 1 : 0;
    const int per = first_b + (b_out ? (cols_b + 3) >> 2 : 0);     // Philox calls per atom
    for (int i = threadIdx.x; i < (a1 - a0) * per; i += blockDim.x) {
        const int la = i / per, j = i - la * per;
        const size_t a = (size_t)(a0 + la);
        if (j < first_b) {
            const rng::Words o = rng::draw(key, (uint32_t)la, step, base + rng::TRAIN_POS_NORMAL, 0u);
#pragma unroll
            for (int k = 0; k < 3; ++k) a_out[3 * a + k] = rng::normal_component(o, k);
        } else {
            const int b = j - first_b;
            const rng::Words o = rng::draw(key, (uint32_t)la, step, base + purpose_b, (uint32_t)b);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int col = 4 * b + k;
                if (col < cols_b) b_out[a * cols_b + col] = uniform_b ? rng::uniform_component(o, k) : rng::normal_component(o, k);
            }
        }
    }
}

hipError_t launch_train_noise_draw(const uint64_t* keys, const int32_t* lig_ptr, int n_graphs, int n_lig, uint32_t purpose_base,
                                   uint32_t n_t, const int64_t* t_in, int64_t* t_out, float* a, float* b, int cols_b,
                                   uint32_t purpose_b, int uniform_b, hipStream_t s) {
    if (n_graphs == 0) return hipSuccess;
    hipLaunchKernelGGL(train_noise_draw_kernel, dim3(n_graphs), dim3(256), 0, s, keys, lig_ptr, n_lig, purpose_base, n_t, t_in, t_out,
                       a, b, cols_b, purpose_b, uniform_b);
    return hipGetLastError();
}

// ---- TargetDiff ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float noise_lae(float a, float b) {      // _log_add_exp of the reference (train_loss.hip: lae)
    const float mx = fmaxf(a, b);
    return mx + logf(expf(a - mx) + expf(b - mx));
}
constexpr float NOISE_LOG_TINY = -69.07755278982137f;     // log(1e-30) (train_loss.hip: LOG_TINY)

// thread i < n_graphs writes the time of graph i (its own range of the grid: a graph without a ligand atom gets its time too); thread
// a < n_lig noises atom a at its graph's time, which it evaluates itself (no read of t_out: nothing to wait for)
__global__ __launch_bounds__(256) void train_noise_rng_kernel(
    const float* __restrict__ x0, const int64_t* __restrict__ v0, const int64_t* __restrict__ batch,
    const uint8_t* __restrict__ gen, int n_lig, int B, int C, const float* __restrict__ acp, const float* __restrict__ log_acp,
    const float* __restrict__ log_1m_acp, float log_c, const uint64_t* __restrict__ keys, const int32_t* __restrict__ lig_ptr,
    uint32_t base, uint32_t n_t, const int64_t* __restrict__ t_in, int64_t* __restrict__ t_out, float* __restrict__ x_t,
    float* __restrict__ c_t, int64_t* __restrict__ v_t) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < B) t_out[a] = t_in ? t_in[a] : (int64_t)rng::train_time(keys[a], base, n_t);
    if (a >= n_lig) return;
    const int gr = (int)batch[a];
    if (gr < 0 || gr >= B) return;      // a malformed batch must not index keys / lig_ptr outside their arrays
    const uint64_t key = keys[gr];
    const int tb = t_in ? (int)t_in[gr] : (int)rng::train_time(key, base, n_t);
    const uint32_t local = (uint32_t)(a - lig_ptr[gr]);
    const bool g = gen[a] != 0;
    const float ab = acp[tb];
    const float sa = sqrtf(ab), sb = sqrtf(1.0f - ab);
    rng::Words nw = rng::draw(key, local, (uint32_t)tb, base + rng::TRAIN_POS_NORMAL, 0u);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = x0[3 * a + k];
        const float xn = __fadd_rn(__fmul_rn(sa, x), __fmul_rn(sb, rng::normal_component(nw, k)));
        x_t[3 * a + k] = g ? xn : x;
    }
    const int v = (int)v0[a];
    const float la = log_acp[tb], lb = log_1m_acp[tb] - log_c;
    int best = 0;
    float best_v = -INFINITY;
    for (int k = 0; k < C; ++k) {
        if ((k & 3) == 0) nw = rng::draw(key, local, (uint32_t)tb, base + rng::TRAIN_TYPE_UNIFORM, (uint32_t)(k >> 2));
        const float lq = noise_lae((k == v ? 0.f : NOISE_LOG_TINY) + la, lb);
        const float gum = -logf(-logf(rng::uniform_component(nw, k & 3) + 1e-30f) + 1e-30f);
        const float s = gum + lq;
        if (s > best_v) { best_v = s; best = k; }
    }
    const int vn = g ? best : v;
    for (int k = 0; k < C; ++k) c_t[(size_t)a * C + k] = k == vn ? 1.f : 0.f;
    v_t[a] = vn;
}

hipError_t launch_train_noise_rng(const float* x0, const int64_t* v0, const int64_t* batch, const uint8_t* gen, int n_lig, int n_graphs,
                                  int C, const float* acp, const float* log_acp, const float* log_1m_acp, float log_c,
                                  const uint64_t* keys, const int32_t* lig_ptr, uint32_t purpose_base, uint32_t n_t,
                                  const int64_t* t_in, int64_t* t_out, float* x_t, float* c_t, int64_t* v_t, hipStream_t s) {
    const int n = n_lig > n_graphs ? n_lig : n_graphs;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(train_noise_rng_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x0, v0, batch, gen, n_lig, n_graphs, C, acp,
                       log_acp, log_1m_acp, log_c, keys, lig_ptr, purpose_base, n_t, t_in, t_out, x_t, c_t, v_t);
    return hipGetLastError();
}

}  // namespace cbgx

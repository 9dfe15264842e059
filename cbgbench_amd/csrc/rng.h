// libcbgx -- counter-based noise for the sampling step kernels ("counter" noise mode).
// Every random number of a sampling run is a pure function of an ADDRESS, so a kernel evaluates it where it is consumed and a graph
// gets the same numbers wherever it sits in a batch, on whatever rank, in whatever order:
//
//   generator   Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers
//               0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds
//   key         the two halves (low, high) of the graph's 64-bit STREAM KEY; the host derives it from (seed, pocket index, sample
//               index) with one Philox call: counter = (seed low, seed high, pocket, sample), key = STREAM_KEY0 / STREAM_KEY1, stream
//               key = word 0 | word 1 << 32   (cbgbench_amd/noise.py::stream_keys is the model of it)
//   counter     (index of the atom INSIDE ITS LIGAND, step, purpose, block); the four output words of one call are the components
//               4 * block .. 4 * block + 3 of the draw
//   purpose     what the number is for (enum below, mirrored as CBGX_NOISE_* in include/cbgx.h).  The entry points take a PURPOSE
//               BASE that is added to it: 0 for a plain run, a multiple of PURPOSE_STRIDE for a caller that wants further
//               independent draws for the same graph
//   uniform     (w >> 8) * 2^-24 in [0, 1): torch.rand's own 24-bit grid, exact in fp32
//   normal      Box-Muller on a pair of words (w_r, w_a): r = sqrt(-2 log(((w_r >> 8) + 1) * 2^-24)) -- the radius word is mapped to
//               (0, 1], the logarithm never sees 0 and r <= sqrt(48 ln 2) = 5.77 --, theta = 2 pi * ((w_a >> 8) * 2^-24); the pair
//               gives the two components r cos(theta), r sin(theta).  Words (0, 1) of a call are components 4 block + 0 / + 1, words
//               (2, 3) components 4 block + 2 / + 3: one call, four normals.
// The words and the uniforms are the same bits on every compiler; the normals go through the platform's logf / sqrtf / sincosf.
// No two draws of a run share an address as long as the atoms of a ligand keep their order (the one precondition of the mode).
//
// TRAINING AND VALIDATION draw from the same generator (purposes TRAIN_*).  The key of a graph is stream_key(seed, example index,
// visit): the example's index in its dataset -- a global identity -- stands where the pocket index stands, the training iteration
// (the same number on every rank) where the sample index stands; validation uses visit 0 under the purpose base PURPOSE_STRIDE, so
// no validation draw shares an address with a training draw of an example with the same number.
//   time        t_g = (uint64(w0) * n_t) >> 32 in [0, n_t), w0 = word 0 of the call at counter (0, 0, base + TRAIN_TIME, 0) under the
//               graph's key (train_time below); n_t = T for TargetDiff and DiffBP ('symmetric' sampler), T + 1 for DiffSBDD ('random').
//               Every t_g has the symmetric sampler's marginal (uniform on [0, T)); the antithetic pairing t, T - 1 - t inside a batch
//               is a function of batch position and is NOT kept.
//   per atom    counter = (index inside the ligand, step = the graph's integer time t_g, base + purpose, block): words, uniforms and
//               Box-Muller as above.  The step word is the graph's time in training and in eval mode, so the evaluation times of one
//               validation call draw at different addresses; DiffSBDD's second eval-mode network call (time 0) draws at step 0, which
//               none of its evaluation times linspace(1, T) uses.  Two evaluation times that coincide after truncation to an integer
//               (tiny T) get the same draw.
//   protein     the protein-coordinate augmentation of a visit (the config's add_pos_noise, applied before the model call): counter =
//               (index of the protein atom INSIDE ITS POCKET, step 0, base + TRAIN_PROTEIN_NORMAL, 0), components 0..2, under the same
//               graph key -- training base 0, validation base PURPOSE_STRIDE.  It does not depend on the graph's time.  Precondition: the
//               protein atoms of an example keep their order.
//   choice      the decomposition of its ligand a visit trains on (the config's choose_ctx_gen): k = (uint64(w0) * K) >> 32 in [0, K),
//               w0 = word 0 of the call at counter (0, 0, base + TRAIN_CHOOSE_CTX, 0) under the graph key -- the time's formula at an
//               address of its own; training base 0, validation base PURPOSE_STRIDE.
// Plain C++: a host compiler builds this header for the stand-alone known-answer program of tests/test_counter_noise.py.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CBGX_HD __host__ __device__ __forceinline__
#else
#define CBGX_HD inline
#endif

namespace cbgx {
namespace rng {

enum Purpose : uint32_t {
    POS_NORMAL = 0,     // position normal of a reverse step, components 0..2            (all three classes)
    TYPE_UNIFORM = 1,   // type uniform of a reverse step, components 0..C-1             (TargetDiff: the Gumbel draw)
    MASK_UNIFORM = 2,   // mask draw of a reverse step, component 0                      (DiffBP)
    TYPE_NORMAL = 3,    // type normal of a reverse step, components 0..C-1              (DiffSBDD)
    INIT_POS = 4,       // initial position normal, step 0, components 0..2              (DiffSBDD z_T)
    INIT_TYPE = 5,      // initial type normal, step 0, components 0..C-1                (DiffSBDD z_T)
    FINAL_POS = 6,      // position normal of sample_p_xh_given_z0, step 0               (DiffSBDD; the type normal the reference draws
                        // there and discards has no address)
    TRAIN_TIME = 7,         // the graph's time of a training call: counter (0, 0, base + TRAIN_TIME, 0), word 0
    TRAIN_POS_NORMAL = 8,   // position normal of a training / validation call, components 0..2, step = the graph's time  (all classes)
    TRAIN_TYPE_UNIFORM = 9, // type uniform, components 0..C-1                              (TargetDiff: the Gumbel draw)
    TRAIN_MASK_UNIFORM = 10,// mask draw, component 0                                       (DiffBP)
    TRAIN_TYPE_NORMAL = 11, // type normal, components 0..C-1                               (DiffSBDD)
    TRAIN_PROTEIN_NORMAL = 12, // protein-coordinate augmentation of a training visit (add_pos_noise), components 0..2: counter (the
                            // atom's index INSIDE ITS POCKET, step 0, base + TRAIN_PROTEIN_NORMAL, 0)   (train_transform.hip)
    TRAIN_CHOOSE_CTX = 13,  // which decomposition of its ligand a visit trains on (choose_ctx_gen): counter (0, 0, base +
                            // TRAIN_CHOOSE_CTX, 0), word 0 through scale_word                           (train_transform.hip)
    PURPOSE_STRIDE = 16 // purpose bases are multiples of this
};

constexpr uint32_t STREAM_KEY0 = 0x58474243u;   // "CBGX"
constexpr uint32_t STREAM_KEY1 = 0x53494F4Eu;   // "NOIS"

struct Words {
    uint32_t w0, w1, w2, w3;    // named, not an array: nothing can index them, so they live in registers
};

CBGX_HD void mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
    const uint64_t p = (uint64_t)a * (uint64_t)b;
    hi = (uint32_t)(p >> 32);
    lo = (uint32_t)p;
}

CBGX_HD Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {   // (constant trip count: compilers unroll it)
        uint32_t hi0, lo0, hi1, lo1;
        mulhilo(0xD2511F53u, c0, hi0, lo0);
        mulhilo(0xCD9E8D57u, c2, hi1, lo1);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Words{c0, c1, c2, c3};
}

// the four words of one address
CBGX_HD Words draw(uint64_t stream_key, uint32_t atom, uint32_t step, uint32_t purpose, uint32_t block) {
    return philox4x32_10(atom, step, purpose, block, (uint32_t)stream_key, (uint32_t)(stream_key >> 32));
}

CBGX_HD uint64_t stream_key(uint64_t seed, uint32_t pocket, uint32_t sample) {
    const Words o = philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), pocket, sample, STREAM_KEY0, STREAM_KEY1);
    return (uint64_t)o.w0 | ((uint64_t)o.w1 << 32);
}

// a word mapped to an integer in [0, n): floor(w * n / 2^32); w = 0xFFFFFFFF gives n - 1, never n
CBGX_HD uint32_t scale_word(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * (uint64_t)n) >> 32); }

// the time of a graph in a training call: in [0, n_t)
CBGX_HD uint32_t train_time(uint64_t stream_key, uint32_t purpose_base, uint32_t n_t) {
    return scale_word(draw(stream_key, 0u, 0u, purpose_base + TRAIN_TIME, 0u).w0, n_t);
}

CBGX_HD float uniform(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }            // [0, 1)
CBGX_HD float uniform_open0(uint32_t w) { return (float)((w >> 8) + 1u) * 5.9604644775390625e-8f; }   // (0, 1]

// component `j` (0..3) of the uniform draw of one call (selects between VALUES, not an indexed or address-selected read: the words
// stay in registers)
CBGX_HD float uniform_component(const Words o, int j) {
    const uint32_t w0 = o.w0, w1 = o.w1, w2 = o.w2, w3 = o.w3;
    const uint32_t lo = (j & 1) ? w1 : w0, hi = (j & 1) ? w3 : w2;
    return uniform((j & 2) ? hi : lo);
}

// component `j` (0..3) of the normal draw of one call: pair j / 2, cosine for even j, sine for odd j
CBGX_HD float normal_component(const Words o, int j) {
    const uint32_t w0 = o.w0, w1 = o.w1, w2 = o.w2, w3 = o.w3;
    const uint32_t wr = (j & 2) ? w2 : w0, wa = (j & 2) ? w3 : w1;
    const float r = sqrtf(-2.0f * logf(uniform_open0(wr)));
    float sn, cs;
    sincosf(6.283185307179586f * uniform(wa), &sn, &cs);
    return r * ((j & 1) ? sn : cs);
}

}  // namespace rng
}  // namespace cbgx

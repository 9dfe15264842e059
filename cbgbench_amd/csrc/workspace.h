// carving a caller's buffer into 256-byte-aligned regions (api.hip: forward workspace; api_train.hip: tape, training workspace)
#pragma once
#include <stddef.h>

#include <initializer_list>

#include "kernels.h"

namespace cbgx {

static inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// hands out consecutive regions of `base`, each rounded up to 256 bytes; `off` is the size carved so far.
// (base may be NULL when only the size is wanted: nothing is dereferenced)
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* b) : base((char*)b) {}
    template <class T>
    T* take(size_t bytes) {
        T* p = (T*)(base + off);
        off += align_up(bytes);
        return p;
    }
};

// The receptive-field walk every pruned path shares.  The caller has written the seed flags into `mask` and holds the list the first
// hop starts from; each hop marks the neighbours of the previous list's rows and compacts the grown mask into the next list of `out`.
static inline hipError_t walk_receptive_field(uint8_t* mask, NodeList from, const int32_t* nbr, const int32_t* deg, int n,
                                              std::initializer_list<NodeList> out, hipStream_t s) {
    for (const NodeList& to : out) {
        hipError_t e = launch_mark_nbr(from, n, nbr, deg, mask, s);
        if (e == hipSuccess) e = launch_build_active(mask, n, to, s);
        if (e != hipSuccess) return e;
        from = to;
    }
    return hipSuccess;
}

}  // namespace cbgx

// carving a caller's buffer into 256-byte-aligned regions (api.hip: forward workspace; api_train.hip: tape, training workspace)
#pragma once
#include <stddef.h>

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

// a node list built on the device: row ids (any order) and the address of their number
struct NodeList {
    int* rows;
    int* count;
};

}  // namespace cbgx

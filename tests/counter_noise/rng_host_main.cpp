// Stand-alone host build of cbgbench_amd/csrc/rng.h (tests/test_counter_noise.py): reads addresses, prints what the header makes of
// them, so that the test can compare with the numpy model bit for bit.  Input lines (hexadecimal fields):
//   P c0 c1 c2 c3 k0 k1       -> "P" + the four Philox4x32-10 words + the bit patterns of their four uniforms
//   D key atom step purpose block -> "D" + the four words of rng::draw + the bit patterns of the four uniform components and of the
//                                 four normal components (the normals are informative: libm, not the device's functions)
//   S seed pocket sample      -> "S" + the 64-bit stream key
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "rng.h"

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* in = std::fopen(argv[1], "r");
    if (!in) return 3;
    char kind;
    while (std::fscanf(in, " %c", &kind) == 1) {
        if (kind == 'P') {
            uint32_t c[4], k[2];
            if (std::fscanf(in, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &c[0], &c[1], &c[2], &c[3], &k[0],
                            &k[1]) != 6)
                return 4;
            const cbgx::rng::Words o = cbgx::rng::philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]);
            std::printf("P %08x %08x %08x %08x %08x %08x %08x %08x\n", o.w0, o.w1, o.w2, o.w3, bits(cbgx::rng::uniform(o.w0)),
                        bits(cbgx::rng::uniform(o.w1)), bits(cbgx::rng::uniform(o.w2)), bits(cbgx::rng::uniform(o.w3)));
        } else if (kind == 'D') {
            uint64_t key;
            uint32_t a[4];
            if (std::fscanf(in, "%" SCNx64 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &key, &a[0], &a[1], &a[2], &a[3]) != 5) return 4;
            const cbgx::rng::Words o = cbgx::rng::draw(key, a[0], a[1], a[2], a[3]);
            std::printf("D %08x %08x %08x %08x", o.w0, o.w1, o.w2, o.w3);
            for (int j = 0; j < 4; ++j) std::printf(" %08x", bits(cbgx::rng::uniform_component(o, j)));
            for (int j = 0; j < 4; ++j) std::printf(" %08x", bits(cbgx::rng::normal_component(o, j)));
            std::printf("\n");
        } else if (kind == 'S') {
            uint64_t seed;
            uint32_t p, s;
            if (std::fscanf(in, "%" SCNx64 " %" SCNx32 " %" SCNx32, &seed, &p, &s) != 3) return 4;
            std::printf("S %016" PRIx64 "\n", cbgx::rng::stream_key(seed, p, s));
        } else {
            return 5;
        }
    }
    std::fclose(in);
    return 0;
}

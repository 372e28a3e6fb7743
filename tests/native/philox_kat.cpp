// Host build of the bootstrap's generator (tapir_amd/csrc/philox4x32.hpp, the code the draw kernel runs).
// stdin: lines "kat c0 c1 c2 c3 k0 k1" (hex) -> the four output words; "draws seed id b n" (decimal) -> the n column indices.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "philox4x32.hpp"

int main() {
    char tag[16];
    while (std::scanf("%15s", tag) == 1) {
        if (!std::strcmp(tag, "kat")) {
            uint32_t c[4], k[2];
            if (std::scanf("%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &c[0], &c[1], &c[2], &c[3], &k[0], &k[1]) != 6) return 1;
            tphip::philox4x32_10(c, k[0], k[1]);
            std::printf("%08x %08x %08x %08x\n", c[0], c[1], c[2], c[3]);
        } else if (!std::strcmp(tag, "draws")) {
            uint64_t seed, id, b, n;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &seed, &id, &b, &n) != 4) return 1;
            for (uint64_t j = 0; 2 * j < n; ++j) {
                uint64_t d0, d1;
                tphip::bootstrap_draw_pair(seed, id, (uint32_t)b, (uint32_t)j, n, &d0, &d1);
                std::printf("%" PRIu64 " ", d0);
                if (2 * j + 1 < n) std::printf("%" PRIu64 " ", d1);
            }
            std::printf("\n");
        } else {
            return 1;
        }
    }
    return 0;
}

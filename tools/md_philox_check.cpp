// Stand-alone host check of grappa_amd/csrc/md_philox.h (Random123's known answers and 100,000 further calls), meant to run under the
// host sanitizers.  The header is plain C++, so no HIP is needed:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I grappa_amd/csrc tools/md_philox_check.cpp -o /tmp/md_philox_check
//     /tmp/md_philox_check
#include <cstdio>
#include "md_philox.h"
int main() {
    const uint32_t kat[3][10] = {{0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
                                 {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
                                 {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
    int bad = 0;
    for (auto& k : kat) {
        uint32_t out[4];
        grappa_philox4x32_10(k[4], k[5], k[0], k[1], k[2], k[3], out);
        for (int i = 0; i < 4; ++i) bad += out[i] != k[6 + i];
    }
    uint32_t acc = 0, out[4];
    for (uint32_t i = 0; i < 100000; ++i) {
        grappa_philox4x32_10(i * 2654435761u, ~i, i, i ^ 0xffffffffu, 0xffffffffu - i, i << 31, out);
        acc ^= out[0] ^ out[1] ^ out[2] ^ out[3];
    }
    std::printf("known answers wrong: %d, checksum %08x\n", bad, acc);
    return bad != 0;
}

// Stand-alone host check of coll_typed.h's two-ended rule (no HIP; tests/test_typed_rule2_cpu.py runs it): for a
// handful of (gran_s, gran_r, base_s, base_r, lo), typed_granule2's G divides each input and is the largest such
// power of two at most 16; typed_walk64_2 adds the two sizes to typed_walk64.  Exit status 0: all hold.
#include <cstdio>
#include <initializer_list>
#include "../../ompi_amd/csrc/coll_typed.h"

int main() {
    const uint64_t A = 0x7f0000001000, B = 0x7f0000002000;
    const struct { int64_t gs, gr; uint64_t bs, br, lo; } cases[] = {
        {16, 16, A, B, 0},     {16, 4, A, B, 0},      {8, 16, A, B + 8, 1048576}, {1, 2, A, B, 16}, {16, 16, A, B, 4},
        {16, 16, A + 2, B, 0}, {-8, 16, A, B, 32},    {12, 24, A, B, 0},          {16, 16, A + 1, B, 0}};
    int bad = 0;
    for (const auto &c : cases) {
        const int G = ompi_amd::typed_granule2(c.gs, c.gr, c.bs, c.br, c.lo);
        bool ok = G == 1 || G == 2 || G == 4 || G == 8 || G == 16, twice = G < 16;
        for (uint64_t v : {(uint64_t)(c.gs < 0 ? -c.gs : c.gs), (uint64_t)c.gr, c.bs, c.br, c.lo}) {
            ok = ok && v % (uint64_t)G == 0;
            twice = twice && v % (uint64_t)(2 * G) == 0;
        }
        if (!ok || twice) printf("case %d: G = %d\n", (int)(&c - cases), G), ++bad;
    }
    using ompi_amd::typed_walk64_2;  // typed_walk64's threshold, force, and either size past 32 bits of granules
    bad += typed_walk64_2(1 << 20, 4, false, 16, 24) + !typed_walk64_2(1 << 20, 4, true, 16, 24) +
           !typed_walk64_2(4ull << 32, 4, false, 16, 24) + typed_walk64_2((4ull << 32) - 4, 4, false, 16, 24) +
           !typed_walk64_2(1 << 20, 4, false, 4ull << 32, 24) + !typed_walk64_2(1 << 20, 4, false, 16, 4ull << 32);
    printf("typed rule 2: %d failures\n", bad);
    return bad ? 1 : 0;
}

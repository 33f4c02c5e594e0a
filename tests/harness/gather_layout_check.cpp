// Stand-alone check of the allgatherv / gather(v) / scatter(v) landing layouts
// in ompi_amd/csrc/coll_landing.h (tests/test_gather_layout_cpu.py builds it
// with -fsanitize=address,undefined and runs it).  Per pass every sender's
// slot must hold min(chunk, M) bytes at any phase mod 16 and be a multiple of
// 256 B; the need is slots x slot; allgatherv and gather(v) have one slot per
// rank, scatter(v) ONE slot whatever the communicator's size.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../ompi_amd/csrc/coll_landing.h"

using namespace ompi_amd;

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++failures <= 20) {                        \
                fprintf(stderr, "FAIL %s: ", #cond);       \
                fprintf(stderr, __VA_ARGS__);              \
                fprintf(stderr, "\n");                     \
            }                                              \
        }                                                  \
    } while (0)

static void check_one(const char *what, const land_layout &l, size_t slots, size_t chunk, size_t M) {
    const size_t piece = std::min(chunk, M);
    CHECK(l.slot >= piece + 16, "%s chunk %zu M %zu: slot %zu", what, chunk, M, l.slot);
    CHECK(l.slot % 256 == 0, "%s chunk %zu M %zu: slot %zu", what, chunk, M, l.slot);
    CHECK(l.slot < piece + 16 + 256, "%s chunk %zu M %zu: slot %zu wastes a round", what, chunk, M, l.slot);
    CHECK(l.need == slots * l.slot, "%s chunk %zu M %zu: need %zu, %zu slots of %zu", what, chunk, M,
          l.need, slots, l.slot);
    CHECK(l.result_off == l.need, "%s: result_off %zu need %zu", what, l.result_off, l.need);
    // the last byte a sender stores (phase 15) stays inside its slot
    CHECK((slots - 1) * l.slot + 15 + piece <= l.need, "%s chunk %zu M %zu: overrun", what, chunk, M);
}

int main() {
    const int ns[] = {1, 2, 3, 8, 16};
    const size_t Ms[] = {1, 15, 16, 17, 4096, (1u << 20) + 1};
    for (size_t M : Ms) {
        const size_t chunks[] = {256, 1024, M};
        for (size_t chunk : chunks) {
            size_t scatter_need = 0;
            for (int n : ns) {
                CHECK(allgatherv_slots(n) == n && gather_slots(n) == n && scatter_slots(n) == 1, "n %d", n);
                check_one("allgatherv", allgatherv_landing(n, chunk, M), (size_t)n, chunk, M);
                check_one("gather", gather_landing(n, chunk, M), (size_t)n, chunk, M);
                const land_layout s = scatter_landing(n, chunk, M);
                check_one("scatter", s, 1, chunk, M);
                if (n == ns[0]) scatter_need = s.need;
                CHECK(s.need == scatter_need, "scatter need %zu at n %d, %zu at n %d", s.need, n,
                      scatter_need, ns[0]);
                // the exchange they ride sizes the same slot
                CHECK(gather_landing(n, chunk, M).slot == alltoall_landing(n, chunk, M).slot, "n %d", n);
                CHECK(s.slot == alltoall_landing(n, chunk, M).slot, "n %d", n);
            }
        }
    }
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("gather layouts ok\n");
    return 0;
}

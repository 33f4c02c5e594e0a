// Stand-alone host program for ompi_amd/csrc/coll_typed.h (no HIP, no GPU):
// reads one case per line — gran typed_addr contig_addr pair_bytes force64 —
// from the file named on the command line and prints the granule and the
// walk (0: 32-bit, 1: 64-bit) the header picks for it.
// tests/test_typed_coll_cpu.py writes the cases and states the rule a second
// time, by brute force.
#include <cinttypes>
#include <cstdio>

#include "../../ompi_amd/csrc/coll_typed.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    int64_t gran;
    uint64_t typed, contig, pair;
    int force, n = 0;
    while (fscanf(f, "%" SCNd64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %d", &gran, &typed, &contig, &pair,
                  &force) == 5) {
        const int G = ompi_amd::typed_granule(gran, typed, contig);
        printf("%d %d\n", G, ompi_amd::typed_walk64(pair, G, force != 0) ? 1 : 0);
        ++n;
    }
    fclose(f);
    printf("typed rule: %d cases\n", n);
    return 0;
}

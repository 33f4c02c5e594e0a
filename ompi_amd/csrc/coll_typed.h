// Granule and walk choice of the typed exchange copies (coll_kernels.h's
// typed_pipe_copy).  Plain integer arithmetic that the host
// (the engine's counters) and the device (every copy) evaluate alike, with no
// HIP call, so a stand-alone host program can check it
// (tests/harness/typed_rule_check.cpp) as landing_layout_check.cpp checks
// coll_landing.h.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define OMPI_AMD_TYPED_HD __host__ __device__
#else
#define OMPI_AMD_TYPED_HD
#endif

namespace ompi_amd {

// G: the largest of 16, 8, 4, 2, 1 that divides the datatype's granule
// (ddt_view.gran: every run, displacement, stride and the extent), the typed
// base address of the block (buffer + displacement * extent) and the address
// of the contiguous end at the first stream byte moved.  One lane then moves
// one aligned G-byte access on either side, and no access crosses a run.
OMPI_AMD_TYPED_HD inline int typed_granule(int64_t gran, uint64_t typed_addr, uint64_t contig_addr) {
    const uint64_t m = (uint64_t)(gran < 0 ? -gran : gran) | typed_addr | contig_addr;
    int g = 16;
    while (g > 1 && (m & (uint64_t)(g - 1)) != 0) g >>= 1;
    return g;
}

// The 32-bit multiply-high walk (typed_offset_fast) indexes granules of the
// pair's packed stream in 32 bits: it runs while pair_bytes / G fits, the
// 64-bit walk (typed_offset<int64_t>) otherwise, or always when forced
// (param "typed_force64": a small test reaches it).
OMPI_AMD_TYPED_HD inline bool typed_walk64(uint64_t pair_bytes, int G, bool force64) {
    return force64 || pair_bytes / (uint64_t)G >= (1ull << 32);
}

}  // namespace ompi_amd

// Planning arithmetic of the staged tile kernels (ddt_kernels.hip): the
// environment settings with their accepted ranges, the instance gap rule,
// and the period / periods-per-tile / dynamic-LDS choice of tile_period.
// Host arithmetic only, no HIP call, so a stand-alone host program can check
// it (tests/harness/ddt_plan_check.cpp) as landing_layout_check.cpp checks
// coll_landing.h.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <utility>
#include <vector>

namespace ompi_amd {

// Division by a launch-invariant 32-bit divisor (ddt_device.h's fdiv_q):
// q = (t + ((n - t) >> s1)) >> s2 with t = umulhi(n, m).
struct fastdiv {
    uint32_t m, s1, s2;
};

inline fastdiv make_fdiv(uint32_t d) {  // host side
    if (d <= 1) return {0u, 0u, 0u};
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;  // ceil(log2 d)
    const uint64_t m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
    return {(uint32_t)m, 1u, l - 1};
}

constexpr int64_t kTileMaxGap = 128;            // bytes of gap the tile reads through
constexpr int64_t kTileDataDefault = 16 << 10;  // LDS data bytes per workgroup (tuned)
constexpr int64_t kTileMinWindow = 256 << 10;   // smaller windows: one generic launch
constexpr int64_t kRunMaxGapDefault = 4096;
// a workgroup's LDS on gfx950 (160 KiB): no tile plan may ask for more
constexpr int64_t kLdsMaxBytes = 160 << 10;
// accepted ranges of the byte settings (values outside fall back to the default)
constexpr int64_t kTileBytesMin = 4096, kTileBytesMax = 60 << 10;
// OMPI_AMD_DDT_UNPACK_TILE_BYTES: the tile's data area is max(setting, span)
// bytes beside a byte map of up to 16 KiB (instances of at most 8 KiB, two
// bytes per packed byte) and 48 B of phase and rounding, all inside
// kLdsMaxBytes: 160 KiB - 16 KiB - 48 B = 147,408 B.  The bound was 1 MiB,
// whose launches no workgroup can hold; 128 KiB is the largest power of two
// that fits.
constexpr int64_t kUnpackTileBytesMin = 1024, kUnpackTileBytesMax = 128 << 10;
constexpr int64_t kInstTileMaxSize = 8192;      // packed bytes of an instance period

// The settings, each parsed from its environment string (nullptr: unset).
struct ddt_knobs {
    bool tile_off = false;          // OMPI_AMD_DDT_TILE=0
    bool tile_wide = true;          // OMPI_AMD_DDT_TILE_WIDE (0: sub-16-B granules only)
    int64_t tile_bytes = kTileDataDefault;  // OMPI_AMD_DDT_TILE_BYTES
    int64_t unpack_tile_bytes = 0;  // OMPI_AMD_DDT_UNPACK_TILE_BYTES (0: derived)
    int unpack_nt = -1;             // OMPI_AMD_DDT_UNPACK_NT (-1: by run length)
    int64_t run_max_gap = kRunMaxGapDefault;  // OMPI_AMD_DDT_RUN_MAXGAP
};

inline bool parse_tile_off(const char *e) { return e && atoi(e) == 0; }
inline bool parse_tile_wide(const char *e) { return !(e && atoi(e) == 0); }
inline int64_t parse_tile_bytes(const char *e) {
    const int64_t x = e ? atoll(e) : 0;
    return (x >= kTileBytesMin && x <= kTileBytesMax) ? x : kTileDataDefault;
}
inline int64_t parse_unpack_tile_bytes(const char *e) {
    const int64_t x = e ? atoll(e) : 0;
    return (x >= kUnpackTileBytesMin && x <= kUnpackTileBytesMax) ? x : 0;
}
inline int parse_unpack_nt(const char *e) { return e ? atoi(e) : -1; }
inline int64_t parse_run_max_gap(const char *e) {
    return e ? std::max<int64_t>(0, atoll(e)) : kRunMaxGapDefault;
}

inline ddt_knobs knobs_from(const char *tile, const char *wide, const char *tile_bytes,
                            const char *unpack_tile_bytes, const char *unpack_nt,
                            const char *run_max_gap) {
    ddt_knobs k;
    k.tile_off = parse_tile_off(tile);
    k.tile_wide = parse_tile_wide(wide);
    k.tile_bytes = parse_tile_bytes(tile_bytes);
    k.unpack_tile_bytes = parse_unpack_tile_bytes(unpack_tile_bytes);
    k.unpack_nt = parse_unpack_nt(unpack_nt);
    k.run_max_gap = parse_run_max_gap(run_max_gap);
    return k;
}

inline int64_t plan_unpack_tile_bytes(const ddt_knobs &k, size_t runs) {
    if (k.unpack_tile_bytes) return k.unpack_tile_bytes;
    return runs >= 8 ? std::max<int64_t>(4096, k.tile_bytes / 2) : k.tile_bytes;
}

inline bool plan_unpack_nt(const ddt_knobs &k, int64_t max_run) {
    return k.unpack_nt >= 0 ? k.unpack_nt != 0 : max_run < 64;
}

// What the plan reads of a datatype program.
struct ddt_plan_type {
    size_t nelem = 0;
    int64_t count0 = 0, blen0 = 0, stride0 = 0, disp0 = 0;  // element 0
    int64_t size = 0, extent = 0, max_blen = 0;
    bool inst_tile = false;  // one instance may be the period (plan_inst_tile)
    int64_t lo = 0, hi = 0;  // lowest / one past highest typed byte of an instance
};

// One instance as the period: small instances whose runs ([begin, end) typed,
// typemap order) leave gaps of at most kTileMaxGap bytes within an instance
// and between consecutive instances.  The byte map holds typed offset - lo in
// 16 bits.
inline bool plan_inst_tile(const std::vector<std::pair<int64_t, int64_t>> &runs, int64_t size,
                           int64_t extent, int64_t *lo_out, int64_t *hi_out) {
    if (size > kInstTileMaxSize || runs.empty()) return false;
    int64_t lo = runs[0].first, hi = runs[0].second;
    for (const auto &r : runs) { lo = std::min(lo, r.first); hi = std::max(hi, r.second); }
    std::vector<std::pair<int64_t, int64_t>> sorted = runs;
    std::sort(sorted.begin(), sorted.end());
    int64_t gap = 0, reach = sorted[0].second;
    for (const auto &r : sorted) {
        gap = std::max(gap, r.first - reach);
        reach = std::max(reach, r.second);
    }
    gap = std::max(gap, extent - (hi - lo));
    if (!(hi - lo < 65536 && gap <= kTileMaxGap && extent > 0)) return false;
    *lo_out = lo;
    *hi_out = hi;
    return true;
}

struct ddt_tile_plan {
    bool ident = false;  // period = one run (identity map); else one instance
    int64_t psize = 0;   // packed bytes per period
    int64_t pext = 0;    // typed bytes between consecutive periods
    int64_t base = 0;    // typed offset of period 0's lowest byte
    int64_t span = 0;    // typed bytes from a period's lowest byte past its highest
    int64_t nper = 0;    // periods per tile
    int64_t map_bytes = 0;  // LDS bytes holding the map (0: identity)
    bool nt = false;     // unpack: typed-side stores non-temporal
    size_t lds = 0;      // dynamic LDS of the launch
};

// The period of the staged tile kernels for this layout (false: not periodic
// enough, a gap too wide to read through, or a tile no workgroup can hold).
inline bool plan_tile_period(const ddt_plan_type &t, size_t count, int G, bool unpack,
                             const ddt_knobs &k, ddt_tile_plan *out) {
    if (k.tile_off) return false;
    ddt_tile_plan P;
    if (t.nelem == 1 && t.count0 > 1 && (G < 16 || k.tile_wide) &&
        (count == 1 || t.extent == t.count0 * t.stride0) && t.stride0 > 0 &&
        t.stride0 - t.blen0 <= (unpack ? k.run_max_gap : kTileMaxGap) &&
        t.stride0 <= k.tile_bytes / 4) {
        P.ident = true;  // period = one run
        P.psize = t.blen0;
        P.pext = t.stride0;
        P.base = t.disp0;
        P.span = t.blen0;
    } else if (t.inst_tile && (t.nelem > 1 || G < 16 || k.tile_wide) &&
               t.hi - t.lo <= k.tile_bytes / 4) {
        P.psize = t.size;  // period = one instance
        P.pext = t.extent;
        P.base = t.lo;
        P.span = t.hi - t.lo;
        P.map_bytes = (P.psize * 2 + 15) & ~(int64_t)15;
    } else {
        return false;
    }
    if (P.pext < 0 || P.psize % G != 0) return false;
    // the unpack tile stages the packed bytes of its periods in the LDS sized
    // for their typed span: they must fit it (an instance that overlaps
    // itself packs more bytes than it spans)
    if (unpack && (P.psize > P.pext || P.psize > P.span)) return false;
    P.nt = unpack && plan_unpack_nt(k, P.ident ? P.psize : t.max_blen);
    const int64_t tb = unpack ? plan_unpack_tile_bytes(k, P.ident ? 1 : t.nelem) : k.tile_bytes;
    P.nper = std::max<int64_t>(1, (tb - P.span) / std::max<int64_t>(P.pext, 1) + 1);
    // LDS: the map, then the tile's typed span (the unpack stages only the
    // packed bytes of its periods, but sizing its LDS to those — more
    // workgroups per CU — measured slower: vector bl64 5.4 -> 4.9 TB/s,
    // profiles/r04_unpack_tile_sweep.jsonl), + 32 for the 16-B phase
    P.lds = (size_t)P.map_bytes +
            (size_t)(((P.nper - 1) * P.pext + P.span + 15) & ~(int64_t)15) + 32;
    if ((int64_t)P.lds > kLdsMaxBytes) return false;
    *out = P;
    return true;
}

}  // namespace ompi_amd
